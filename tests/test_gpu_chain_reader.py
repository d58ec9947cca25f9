"""The device chain reader (MCE_CHAIN_READER=hip; mce_chain_dev_* / chain_io.loadtxt_device) against the host reader
(libmcechains.so) and np.loadtxt: the same array, bit for bit -- every comparison is on the uint64 view, so -0.0 and NaN payloads
count -- and the same exceptions."""
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from mcevidence_amd import chain_io
from test_chain_reader import TOKENS, _ALPHABET

pytestmark = pytest.mark.gpu

BAD_TOKENS = ["abc", "1e", "1e+", "--1", "1.2.3", "0x10", "1p3", "1,5", "nan(1)", "1d5", "e5", "."]      # test_chain_reader's list without ""


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode("ascii"))
    return str(p)


def test_token_column_matches_python_float(tmp_path):
    p = write(tmp_path, "tok.txt", "\n".join(TOKENS) + "\n")
    got, stats = chain_io.loadtxt_device(p, return_stats=True)
    want = np.array([float(t) for t in TOKENS]).reshape(-1, 1)
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))
    assert same(got, chain_io.loadtxt(p))                 # NaN signs and payloads as the host reader's strtod gives them
    assert stats["tokens"] == len(TOKENS) and 0 < stats["patched"] < len(TOKENS)
    for i, tok in enumerate(BAD_TOKENS):
        bad = write(tmp_path, "bad%d.txt" % i, "1 2\n3 %s\n5 6\n" % tok)
        with pytest.raises(ValueError) as dev:
            chain_io.loadtxt_device(bad)
        with pytest.raises(ValueError) as host:
            chain_io.loadtxt(bad)
        assert str(dev.value) == str(host.value)


def test_layout_variants_match_host_reader_and_numpy(tmp_path):
    body = ("# weight  minuslogL  a b\n"
            "  1   0.5E+01  -1.25   3\n"
            "\n"
            "2\t6.5\t1e-3\t4   # trailing comment\n"
            "   \t  \n"
            "#only a comment\n"
            "3 7.5 +2.5 5\r\n"
            "4 8.5 nan inf")                              # no trailing newline
    p = write(tmp_path, "a.txt", body)
    got = chain_io.loadtxt_device(p)
    assert got.shape == (4, 4)
    assert same(got, chain_io.loadtxt(p)) and np.array_equal(got, np.loadtxt(p, ndmin=2), equal_nan=True)
    cases = {
        "glued": "1 2#c\n3 4# 9 9\n4\t5 # x\n 6 7\n",       # '#' glued to a token
        "cr": "1 2\r3 4\r5 6",                            # bare \r ends a line
        "crlf": "1 2\r\n\r\n3 4\r\n",
        "spaces": "   1   2   \n\t3\t4\t\n  5    6 \n",
        "one": "1.5 2.5 3.5\n",
        "onetoken": "7",
        "col": "1\n2\n3\n",
        "comment_crosses_tiles": "1 2\n#" + "x" * 9000 + " 5 6 7\n3 4\n" + "# 8 9\n" * 900 + "5 6",
        "long_blank": "1 2\n" + " " * 5000 + "\n" + "\n" * 5000 + "3 4\n",
        "wide": " ".join(str(i) for i in range(3000)) + "\n" + " ".join(str(-i) for i in range(3000)) + "\n",
    }
    for name, text in cases.items():
        p = write(tmp_path, name + ".txt", text)
        got, want = chain_io.loadtxt_device(p), chain_io.loadtxt(p)
        assert same(got, want), name
        assert np.array_equal(got, np.loadtxt(p, ndmin=2)), name
    vf = write(tmp_path, "vf.txt", "1\v2\f3\n\v4 5\f 6\f\n")          # \v and \f separate fields (they do not end lines)
    assert same(chain_io.loadtxt_device(vf), chain_io.loadtxt(vf)) and chain_io.loadtxt_device(vf).shape == (2, 3)
    col = write(tmp_path, "col1.txt", "1\n2\n3\n")
    assert chain_io.loadtxt_device(col, ndmin=1).shape == (3,)
    for name, text in (("empty", "# nothing\n\n"), ("zero", "")):
        p = write(tmp_path, name + ".txt", text)
        assert chain_io.loadtxt_device(p).shape == chain_io.loadtxt(p).shape == (0, 1)
        assert chain_io.loadtxt_device(p, ndmin=1).shape == (0,)


def test_more_undecided_tokens_than_the_first_list(tmp_path):
    """one column of 5 000 'nan': every token is left to the host, more than the 4 096 entries of the single-file reader's first
    list (its second pass, with a list of the counted size) and more than the list of a farm handle made for this file alone (the
    list grown once).  The host copy, the device copy and the farm all give the host reader's array"""
    from mcevidence_amd import _capi, farm, resident
    p = write(tmp_path, "nan.txt", "nan\n" * 5000)
    want = chain_io.loadtxt(p)
    assert want.shape == (5000, 1) and np.isnan(want).all()
    text = np.fromfile(p, dtype=np.uint8)
    got, stats = _capi.chain_dev_parse(text.ctypes.data, text.size)
    assert stats["tokens"] == stats["patched"] == 5000 and same(got, want)
    rc = resident.ResidentChains.from_files([p], iw=0, ilike=0, itheta=0)
    assert rc.stats["files"][0]["patched"] == 5000 and same(rc.to_host(), want)
    farm.release_handles()          # a fresh handle of 64 KiB: room for 11 264 tokens, but its list starts at 1 344 entries
    try:
        one, = farm.read_files([p], wave_bytes=65536)
        st = farm.handle_stats()
        assert st["capacity"] == 65536 and st["patched"] == 5000 and st["grows"] == 2 and st["allocs_wave"] == 2, st     # the list and the fixes, once
        assert not isinstance(one, Exception) and same(one, want)
    finally:
        farm.release_handles()


def big_file(tmp_path, fmt, rows, cols=29, seed=7):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((rows, cols)) * np.asarray([1e-3, 1.0, 70.0, 100.0])[rng.integers(0, 4, (rows, cols))]
    p = str(tmp_path / ("big_%s.txt" % fmt.strip("%.")))
    with open(p, "w") as f:
        f.write("# a header line\n")
        step = 20_000
        for i in range(0, rows, step):
            blk = a[i:i + step]
            if fmt == "repr":
                f.write("\n".join(" ".join(map(repr, r)) for r in blk.tolist()) + "\n")
            else:
                np.savetxt(f, blk, fmt=fmt)
    return p, a


@pytest.mark.parametrize("fmt, cap", [("%.7E", 0.0), ("%.10e", 0.0), ("%.17g", 0.01), ("repr", 0.01), ("%.18e", 0.01)])
def test_big_file_equals_host_reader(tmp_path, fmt, cap):
    """200 000 x 29 values: the host reader's array, and the share of tokens patched on the host within the issue's cap"""
    p, a = big_file(tmp_path, fmt, 200_000)
    got, stats = chain_io.loadtxt_device(p, return_stats=True)
    want = chain_io.loadtxt(p)
    print(fmt, stats)
    assert got.shape == (200_000, 29) and same(got, want)
    assert stats["tokens"] == 200_000 * 29
    assert stats["patched"] <= cap * stats["tokens"]
    if fmt in ("%.17g", "repr", "%.18e"):
        assert same(got, a)                               # 17 significant digits round-trip


def test_file_beyond_256_mib(tmp_path):
    """offsets beyond 2^28: about 600 000 x 29 fields of 17-18 bytes"""
    block, _ = big_file(tmp_path, "%.10e", 50_000, seed=9)
    p = str(tmp_path / "huge.txt")
    with open(p, "wb") as f:
        for _ in range(12):                                # 600 000 rows
            f.write(open(block, "rb").read())
    assert os.path.getsize(p) > 256 << 20
    got, stats = chain_io.loadtxt_device(p, return_stats=True)
    print(stats)
    assert got.shape == (600_000, 29) and same(got, chain_io.loadtxt(p)) and stats["patched"] == 0


def test_errors_match_the_host_reader(tmp_path):
    rng = np.random.default_rng(3)
    rows = ["%.7E %.7E %.7E" % tuple(r) for r in rng.standard_normal((30_000, 3))]
    ragged = list(rows)
    ragged[17_123] = "1.0 2.0"
    junk = list(rows)
    junk[21_007] = "1.0 x2.0 3.0"
    longer = list(rows)
    longer[9] = "1 2 3 4"
    for name, lines in (("ragged", ragged), ("junk", junk), ("longer", longer)):
        p = write(tmp_path, name + ".txt", "# head\n" + "\n".join(lines) + "\n")
        with pytest.raises(ValueError) as host:
            chain_io.loadtxt(p)
        with pytest.raises(ValueError) as dev:
            chain_io.loadtxt_device(p)
        assert type(dev.value) is type(host.value) and str(dev.value) == str(host.value)
        assert "row" in str(dev.value) and "line" in str(dev.value)
    with pytest.raises(OSError):
        chain_io.loadtxt_device(str(tmp_path / "missing.txt"))
    with pytest.raises(OSError):
        chain_io.loadtxt_device(str(tmp_path))            # a directory


@settings(max_examples=300, deadline=None)
@given(st.text(alphabet=_ALPHABET, max_size=120))
def test_fuzzed_text_agrees_with_the_host_reader(tmp_path_factory, text):
    """arbitrary bytes from the chain-file alphabet: the device array equals the host reader's, or both raise the same class"""
    p = tmp_path_factory.mktemp("fz") / "f.txt"
    p.write_bytes(text.encode("ascii"))
    try:
        want = chain_io.loadtxt(str(p))
    except ValueError as e:
        with pytest.raises(ValueError) as dev:
            chain_io.loadtxt_device(str(p))
        assert str(dev.value) == str(e)
        return
    assert same(chain_io.loadtxt_device(str(p)), want), text


def test_eight_files_of_one_root_through_the_thread_pool(tmp_path, monkeypatch):
    from mcevidence_amd.chains import read_chain_files
    rng = np.random.default_rng(5)
    paths = []
    for i in range(8):
        p = str(tmp_path / ("root_%d.txt" % (i + 1)))
        np.savetxt(p, rng.standard_normal((20_000 + 1000 * i, 12)), fmt="%.8e" if i % 2 else "%.17g")
        paths.append(p)
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    want = read_chain_files(paths)
    monkeypatch.setenv("MCE_CHAIN_READER", "hip")
    got = read_chain_files(paths)
    assert len(got) == 8 and all(same(g, w) for g, w in zip(got, want))


def test_evidence_from_files_is_identical_under_both_readers(tmp_path, monkeypatch):
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    chains, names, ranges = planck_like_chains(seed=4, rows=(6000, 5500, 6200, 5800))
    root = str(tmp_path / "pl")
    write_cosmomc_chains(root, chains, ranges)
    out = {}
    for mode in ("native", "hip"):
        monkeypatch.setenv("MCE_CHAIN_READER", mode)
        mce = pkg.MCEvidence(root, kmax=4, burnlen=0.1, thinlen=2, verbose=0)
        out[mode] = (np.array(mce.gd.samples, copy=True), np.array(mce.evidence(), copy=True))
    assert np.array_equal(out["hip"][0], out["native"][0])
    assert out["hip"][1].shape == out["native"][1].shape and bool(np.all(out["hip"][1] == out["native"][1]))
