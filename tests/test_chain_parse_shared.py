"""The token parser the host and the device chain readers share (mcevidence_amd/csrc/chain_parse.hpp), on the CPU: every value it
returns is strtod's bit for bit, what it cannot decide it says so, and it decides enough that the device reader sends (almost)
nothing back to the host.  And MCE_CHAIN_READER=hip fails loudly without a device.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import REPO
from test_chain_reader import TOKENS

BAD_TOKENS = ["abc", "1e", "1e+", "--1", "1.2.3", "0x10", "1p3", "1,5", "nan(1)", "1d5", "e5", "."]      # (test_chain_reader's list; "" is the empty line)
SCALES = (1e-3, 1.0, 70.0, 100.0)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_parse") / "chain_parse_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "chain_parse_check.cpp"), "-o", exe])
    return exe


def run_check(exe, tmp_path, name, tokens):
    """-> dict(n, fast, exact, undecided); asserts that no token came out wrong"""
    p = tmp_path / (name + ".txt")
    p.write_text("\n".join(tokens) + "\n")
    out = subprocess.run([exe, "check", str(p)], capture_output=True, text=True, timeout=900)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", last)}
    assert stats["n"] == len(tokens) and stats["wrong"] == 0
    return stats


def fmt_tokens(values, fmt):
    if fmt == "repr":
        return [repr(v) for v in values.tolist()]
    return [fmt % v for v in values.tolist()]


def gaussian_values(seed, n=200_000):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * np.asarray(SCALES)[rng.integers(0, len(SCALES), n)]


def bit_pattern_values(seed, n=200_000):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    return v[np.isfinite(v)]


def test_power_of_five_table_matches_big_integer_arithmetic(checker):
    """the 128-bit table built with 32-bit limbs in the header against Python's integers (the recipe of Lemire's paper)"""
    want = {}
    for q in range(-342, 0):
        p5 = 5 ** -q
        z = 0
        while (1 << z) < p5:
            z += 1
        b = z + 127 if q >= -27 else 2 * z + 128
        c = (1 << b) // p5 + 1
        while c >= 1 << 128:
            c //= 2
        want[q] = c
    for q in range(0, 309):
        p5 = 5 ** q
        while p5 < 1 << 127:
            p5 *= 2
        while p5 >= 1 << 128:
            p5 //= 2
        want[q] = p5
    out = subprocess.check_output([checker, "table"]).decode().split("\n")
    got = {int(a): (int(b, 16) << 64) | int(c, 16) for a, b, c in (line.split() for line in out if line)}
    assert got == want


def test_named_tokens_and_bad_tokens(checker, tmp_path):
    s = run_check(checker, tmp_path, "named", TOKENS + BAD_TOKENS + [""])
    assert s["exact"] >= 30                         # most of the table is decided without strtod


@pytest.mark.parametrize("fmt", ["%.7E", "%.15g", "%.17g", "repr", "%.18e"])
def test_seeded_doubles_bit_identical_to_strtod(checker, tmp_path, fmt):
    """(a) 2 x 200 000 tokens per format (2 million in all): Gaussian values and random finite bit patterns"""
    g = fmt_tokens(gaussian_values(11), fmt)
    b = fmt_tokens(bit_pattern_values(12), fmt)
    s = run_check(checker, tmp_path, "seeded", g + b)
    assert s["n"] >= 390_000
    print(fmt, s)


def test_digit_strings_subnormals_and_the_edge_of_the_range(checker, tmp_path):
    """(a) random digit strings of 1-25 digits with exponents -350..350 (point anywhere), subnormals, neighbours of DBL_MAX"""
    rng = np.random.default_rng(13)
    toks = []
    for _ in range(300_000):
        nd = int(rng.integers(1, 26))
        digits = "".join(map(str, rng.integers(0, 10, nd)))
        dot = int(rng.integers(0, nd + 2))
        if dot <= nd:
            digits = digits[:dot] + "." + digits[dot:]
        if digits == ".":
            digits = "0."
        sign = ("", "-", "+")[int(rng.integers(0, 3))]
        toks.append("%s%se%d" % (sign, digits, int(rng.integers(-350, 351))))
    sub = rng.integers(1, 1 << 52, 50_000, dtype=np.uint64).view(np.float64)          # subnormals
    toks += ["%.17g" % v for v in sub.tolist()] + [repr(v) for v in sub[:10_000].tolist()]
    top = (np.uint64(0x7FEFFFFFFFFFFFFF) - rng.integers(0, 1 << 20, 20_000, dtype=np.uint64)).view(np.float64)
    toks += ["%.17g" % v for v in top.tolist()] + ["%.16e" % v for v in top[:5000].tolist()]
    toks += ["1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "1.797693134862315807e308", "1.8e308", "2e308",
             "17976931348623157e292", "4.9406564584124654e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.2250738585072014e-308",
             "2.2250738585072011e-308", "2.225073858507201e-308", "9007199254740993", "9007199254740993e0", "9007199254740995", "1e23", "8.5e37",
             "9.5e37", "1e-22", "1e-23", "123456789012345678e-5", "1234567890123456789e3", "12345678901234567890e3", "18446744073709551615",
             "18446744073709551616", "184467440737095516150", "0e400", "0e-400", "-0e999999", "1e100000", "1e-100000", "1e99999999999"]
    s = run_check(checker, tmp_path, "digits", toks)
    assert s["exact"] > 0.5 * s["n"]


@pytest.mark.parametrize("fmt, cap", [("%.7E", 0.0), ("%.8e", 0.0), ("%.10e", 0.0), ("%.15g", 0.0), ("%.17g", 0.01), ("repr", 0.01), ("%.18e", 0.01)])
def test_share_of_tokens_left_to_the_host(checker, tmp_path, fmt, cap):
    """(b) 200 000 Gaussian values scaled by {1e-3, 1, 70, 100}: finite values at <= 15 significant digits are all converted by the
    shared function; at 17-19 digits at most 1 % are left to strtod (the fast path alone leaves 48-100 %)"""
    s = run_check(checker, tmp_path, "share", fmt_tokens(gaussian_values(21), fmt))
    print(fmt, s)
    assert s["undecided"] <= cap * s["n"]
    if cap == 0.0:
        assert s["fast"] == s["n"]                  # the host reader's fast path alone covers the chain formats
    else:
        assert s["fast"] < 0.6 * s["n"]             # ... and not these: the cap needs the second exact path


def test_device_reader_fails_loudly_without_a_device(tmp_path, monkeypatch):
    """(c) no quiet host read: loadtxt_device and MCE_CHAIN_READER=hip raise RuntimeError when no device is visible"""
    from mcevidence_amd import _capi, chain_io
    from mcevidence_amd.chains import MCSamples
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    f = tmp_path / "a.txt"
    f.write_text("1 2 3\n4 5 6\n")
    with pytest.raises(RuntimeError, match="no HIP device"):
        chain_io.loadtxt_device(str(f))
    with pytest.raises(OSError):
        chain_io.loadtxt_device(str(tmp_path / "missing.txt"))
    chains, names, ranges = planck_like_chains(seed=3, rows=(300, 280))
    root = str(tmp_path / "pl")
    write_cosmomc_chains(root, chains, ranges)
    monkeypatch.setenv("MCE_CHAIN_READER", "hip")
    with pytest.raises(RuntimeError, match="no HIP device"):
        MCSamples(root)
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    assert MCSamples(root).samples.shape[0] > 0


def test_reader_mode_and_entry_points_are_declared():
    """the device reader's entry points are part of the C ABI (version unchanged) and of the binding"""
    from mcevidence_amd import _capi, chain_io
    for name in ("mce_chain_dev_open", "mce_chain_dev_read", "mce_chain_dev_close"):
        assert name in _capi.SIGNATURES and hasattr(_capi.load(), name)
    assert _capi.load().mce_abi_version() == 3 and callable(chain_io.loadtxt_device)
