"""libmcechains.so (include/mcechains.h) against np.loadtxt -- the call it replaces
(reference MCEvidence.py:564) -- bit for bit.  CPU only."""
import ctypes
import os
import platform
import re
import shutil

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from helpers import REPO
from mcevidence_amd import chain_io

HEADER = os.path.join(REPO, "include", "mcechains.h")


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_library_exports_every_declared_symbol():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(mce_chain_[a-z0-9_]+)\s*\(", txt)))
    lib = ctypes.CDLL(chain_io.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s)
    assert sorted(chain_io.SIGNATURES) == syms
    for name in ("MCC_ERR_IO", "MCC_ERR_PARSE", "MCC_ERR_RAGGED", "MCC_ERR_INVALID"):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, open(HEADER).read())
        assert m and int(m.group(1)) == getattr(chain_io, name)


TOKENS = ["0", "-0", "0.0", "-0.0", "1", "+1", "-1", "1.", ".5", "-.5", "+.5e1", "1e0", "1E5", "1e+5", "1e-5",
          "0.2231360E-01", "-0.1234567E+03", "6.0221409e+23", "1.7976931348623157e308", "2.2250738585072014e-308",
          "4.9e-324", "5e-324", "2.4703282292062327e-324", "1e-400", "1e400", "-1e400", "123456789012345678901234567890",
          "0.1", "0.30000000000000004", "9007199254740993", "9007199254740992", "9007199254740991", "1e22", "1e23",
          "8.5e37", "123456789e15", "1.2345678901234567890123456789", "0.000000000000000000000000000001",
          "00012", "1e0005", "inf", "-inf", "+Inf", "INFINITY", "nan", "NaN", "-nan",
          "3.14159265358979323846264338327950288", "2.2250738585072011e-308", "17976931348623158e292"]


@pytest.mark.parametrize("tok", TOKENS)
def test_tokens_match_python_float(tok):
    got, want = chain_io.parse_token(tok), float(tok)
    assert np.array([got]).view(np.uint64)[0] == np.array([want]).view(np.uint64)[0] or (np.isnan(got) and np.isnan(want))


@pytest.mark.parametrize("tok", ["", "abc", "1e", "1e+", "--1", "1.2.3", "0x10", "1p3", "1,5", "nan(1)", "1d5", "e5", "."])
def test_bad_tokens_are_rejected(tok):
    with pytest.raises(ValueError):
        chain_io.parse_token(tok)
    with pytest.raises(ValueError):
        float(tok)                          # and Python agrees they are not numbers


@settings(max_examples=300, deadline=None)
@given(st.floats(allow_nan=False, allow_infinity=True), st.sampled_from(["%r", "%.17g", "%.8E", "%.15e", "%.3f", "%g", "%.20e"]))
def test_formatted_doubles_round_trip_like_float(x, fmt):
    text = repr(x) if fmt == "%r" else fmt % x
    got, want = chain_io.parse_token(text), float(text)
    assert np.array([got]).view(np.uint64)[0] == np.array([want]).view(np.uint64)[0]


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode("ascii"))
    return str(p)


def test_layout_variants_match_numpy(tmp_path):
    body = ("# weight  minuslogL  a b\n"
            "  1   0.5E+01  -1.25   3\n"
            "\n"
            "2\t6.5\t1e-3\t4   # trailing comment\n"
            "   \t  \n"
            "#only a comment\n"
            "3 7.5 +2.5 5\r\n"
            "4 8.5 nan inf")                              # no trailing newline
    p = write(tmp_path, "a.txt", body)
    want = np.loadtxt(p, ndmin=2)
    for nt in (0, 1, 2, 7):
        got = chain_io.loadtxt(p, nthreads=nt)
        assert got.shape == (4, 4)
        assert np.array_equal(got, want, equal_nan=True)
    one = write(tmp_path, "one.txt", "1.5 2.5 3.5\n")
    assert same(chain_io.loadtxt(one), np.loadtxt(one, ndmin=2))
    col = write(tmp_path, "col.txt", "1\n2\n3\n")
    assert same(chain_io.loadtxt(col), np.loadtxt(col, ndmin=2))
    assert chain_io.loadtxt(col, ndmin=1).shape == (3,)
    empty = write(tmp_path, "empty.txt", "# nothing\n\n")
    with pytest.warns(UserWarning):
        want = np.loadtxt(empty, ndmin=2)
    assert chain_io.loadtxt(empty).shape == want.shape == (0, 1)


def test_errors(tmp_path):
    with pytest.raises(OSError):
        chain_io.loadtxt(str(tmp_path / "missing.txt"))
    with pytest.raises(OSError):
        chain_io.loadtxt(str(tmp_path))                   # a directory
    ragged = write(tmp_path, "r.txt", "1 2 3\n4 5\n6 7 8\n")
    with pytest.raises(ValueError, match="number of columns changed from 3 to 2 at row 2"):
        chain_io.loadtxt(ragged)
    with pytest.raises(ValueError):
        np.loadtxt(ragged)
    longer = write(tmp_path, "l.txt", "1 2\n3 4 5\n")
    with pytest.raises(ValueError, match="from 2 to 3"):
        chain_io.loadtxt(longer)
    junk = write(tmp_path, "j.txt", "1 2\n3 x4\n")
    with pytest.raises(ValueError, match="could not convert string 'x4' to float64 at row 1, column 2"):
        chain_io.loadtxt(junk)


@pytest.mark.parametrize("fmt", ["%.7E", "%.17g", "%r"])
def test_big_file_bit_identical_to_numpy_at_any_thread_count(tmp_path, fmt):
    rng = np.random.default_rng(5)
    n, c = 20011, 9
    a = rng.standard_normal((n, c)) * 10.0 ** rng.integers(-12, 12, (n, c))
    a[:, 0] = rng.integers(1, 9, n)
    lines = []
    for i, row in enumerate(a):
        if i % 977 == 0:
            lines.append("# block %d" % i)
        sep = "\t" if i % 3 == 0 else "  "
        lines.append(sep.join((repr(float(v)) if fmt == "%r" else fmt % v) for v in row))
    p = write(tmp_path, "big.txt", "\n".join(lines) + "\n")
    want = np.loadtxt(p, ndmin=2)
    for nt in (1, 3, 8, 64):
        assert same(chain_io.loadtxt(p, nthreads=nt), want)
    if fmt != "%.7E":
        assert same(want, a)                              # 17 significant digits round-trip exactly


def test_mcsamples_reads_files_through_the_native_reader(tmp_path, monkeypatch):
    """chains.MCSamples on CosmoMC files: native reader and NumPy give the same samples."""
    from mcevidence_amd.chains import MCSamples
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    chains, names, ranges = planck_like_chains(seed=3, rows=(700, 650))
    root = str(tmp_path / "pl")
    write_cosmomc_chains(root, chains, ranges)
    a = MCSamples(root, burnlen=0.2, thinlen=2)
    monkeypatch.setenv("MCE_CHAIN_READER", "numpy")
    b = MCSamples(root, burnlen=0.2, thinlen=2)
    assert same(a.samples, b.samples)


_ALPHABET = "0123456789+-.eE \t\n#naifNI\r"


@settings(max_examples=400, deadline=None)
@given(st.text(alphabet=_ALPHABET, max_size=120))
def test_fuzzed_text_never_crashes_and_agrees_with_numpy(tmp_path_factory, text):
    """arbitrary bytes from the chain-file alphabet: the reader either returns exactly what np.loadtxt
    returns or raises ValueError where np.loadtxt raises -- never crashes, never invents numbers."""
    import warnings
    p = tmp_path_factory.mktemp("fz") / "f.txt"
    p.write_bytes(text.encode("ascii"))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.loadtxt(str(p), ndmin=2)
        ok = True
    except ValueError:
        ok = False
    if ok:
        got = chain_io.loadtxt(str(p))
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (text, got, want)
    else:
        try:
            got = chain_io.loadtxt(str(p))
        except ValueError:
            return
        # np.loadtxt is stricter in a few spellings Python's float() accepts or vice versa; whatever the
        # native reader accepted must be what float() says, field by field
        fields = [[float(t) for t in line.split("#")[0].split()] for line in text.replace("\r", " ").split("\n")]
        fields = [f for f in fields if f]
        assert got.shape[0] == len(fields) and all(np.array_equal(np.array(f), g, equal_nan=True) for f, g in zip(fields, got)), text


def test_reader_under_address_and_ub_sanitizers(tmp_path):
    """the native reader built with -fsanitize=address,undefined (CPU build; GPU sanitizers are not
    available on this pool) and driven over mmap edge cases at every thread count."""
    import subprocess
    exe = str(tmp_path / "chain_reader_sanitize")
    src = [os.path.join(REPO, "tests", "native", "chain_reader_sanitize.cpp"), os.path.join(REPO, "mcevidence_amd", "csrc", "chain_reader.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"] + src + ["-o", exe])
    work = tmp_path / "files"
    work.mkdir()
    out = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr[-3000:]
    # and the thread split under ThreadSanitizer
    exe_t = str(tmp_path / "chain_reader_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread"] + src + ["-o", exe_t])
    work_t = tmp_path / "files_t"
    work_t.mkdir()
    # GCC's ThreadSanitizer refuses to start ("FATAL: ThreadSanitizer: unexpected memory mapping") where the kernel's address-space
    # randomisation places the program outside the ranges it shadows (high mmap entropy): the binary runs with randomisation off
    # for itself (a personality flag of that one process) wherever setarch can set it
    cmd_t = [exe_t, str(work_t)]
    setarch = shutil.which("setarch")
    if setarch and subprocess.run([setarch, platform.machine(), "-R", "true"], capture_output=True).returncode == 0:
        cmd_t = [setarch, platform.machine(), "-R"] + cmd_t
    out = subprocess.run(cmd_t, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "OK" in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
