"""Files built to sit on the edges of the farm reader's layout (csrc/chain_farm.hpp: 4096-byte tiles, one pad byte behind every
file), shared by tests/test_chain_farm_shared.py (the serial driver on the CPU) and tests/test_gpu_farm.py (the kernels)."""
import numpy as np

from test_chain_reader import TOKENS

TILE = 4096


def _line(rng, ncols, eol="\n"):
    return " ".join("% .10e" % v for v in rng.standard_normal(ncols) * 10.0 ** rng.integers(-3, 4)) + eol


def sized(seed, ncols, nbytes, trailing_newline=True, eol="\n"):
    """data lines of ``ncols`` fields, exactly ``nbytes`` bytes; without a trailing newline the last byte is a digit"""
    rng = np.random.default_rng(seed)
    width = len(_line(rng, ncols, eol))
    lines = [_line(rng, ncols, eol) for _ in range(max(nbytes // width - 1, 0))]
    body = "".join(lines)
    last = _line(rng, ncols, eol if trailing_newline else "")
    pad = nbytes - len(body) - len(last)
    assert pad >= 0, (nbytes, width)
    text = body + " " * pad + last          # (every line has one width: "% .10e"; leading blanks are legal)
    assert len(text) == nbytes and (trailing_newline or text[-1].isdigit())
    return text.encode()


def comment_to_the_last_byte(seed, ncols, nbytes):
    """data, then a '#' comment that runs to the very last byte (no line end): only the pad closes it"""
    rng = np.random.default_rng(seed)
    body = "".join(_line(rng, ncols) for _ in range(5))
    text = body + "# " + "c" * (nbytes - len(body) - 2)
    assert len(text) == nbytes
    return text.encode()


def boundary_files(big_rows=11000):
    """[(name, bytes)]: lengths 4095, 4096, 4097 and exactly 2 x 4096 without a trailing newline, each followed by a file whose first
    line is data; a comment to the last byte of a tile; a file shorter than a tile, an empty one, one of comments only; \\r\\n line
    ends, blank lines, the tokens the host patches; 3, 5 and 23 columns; more than 1 024 tiles in all (``big_rows`` x 23)."""
    rng = np.random.default_rng(77)
    out = [
        ("len4095_nonl", sized(1, 3, TILE - 1, trailing_newline=False)),
        ("data_first_a", sized(2, 5, 700)),
        ("len4096_nonl", sized(3, 5, TILE, trailing_newline=False)),
        ("data_first_b", sized(4, 3, 1300)),
        ("len4097_nonl", sized(5, 3, TILE + 1, trailing_newline=False)),
        ("data_first_c", sized(6, 23, 2 * TILE + 17)),
        ("len8192_nonl", sized(7, 23, 2 * TILE, trailing_newline=False)),
        ("data_first_d", sized(8, 3, 333)),
        ("comment_to_tile_end", comment_to_the_last_byte(9, 5, TILE)),
        ("data_first_e", sized(10, 5, 5000)),
        ("short", b"1 2 3\n4 5 6\n"),
        ("empty", b""),
        ("data_first_f", sized(11, 3, 4096)),
        ("comments_only", b"# nothing here\n#\n   # indented\n"),
        ("crlf", sized(12, 5, 6001, eol="\r\n")),
        ("blank_lines", ("\n\n" + "".join(_line(rng, 3) + ("\n" if i % 3 == 0 else "") for i in range(200)) + "\n  \n").encode()),
        ("glued_comments", "".join(_line(rng, 5, "") + "# tail\n" for _ in range(50)).encode()),
        ("tokens", ("\n".join(TOKENS) + "\n").encode()),
        ("tokens_3col", "".join(" ".join(TOKENS[(i + k) % len(TOKENS)] for k in range(3)) + "\n" for i in range(len(TOKENS))).encode()),
        ("big23", "".join(_line(rng, 23) for _ in range(big_rows)).encode()),
        ("after_big", sized(13, 5, 2 * TILE - 1, trailing_newline=False)),
        ("last_is_empty", b""),
    ]
    return out


RAGGED = b"1 2 3\n4 5 6\n7 8\n9 10 11\n"
RAGGED_MULTIPLE = b"1 2 3\n4 5\n6 7 8 9\n"          # 9 tokens, a multiple of 3, on lines of 3, 2 and 4
JUNK = b"1 2 3\n4 abc 6\n7 8 9\n"
