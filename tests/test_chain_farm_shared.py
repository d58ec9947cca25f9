"""The rules the farm reader's host side and its kernels share (mcevidence_amd/csrc/chain_farm.hpp), on the CPU: the serial driver's
per-file rows, columns and ragged verdict and its token -> file map against ``chain_io.loadtxt`` per file, the row-table lookups
against a NumPy model, ``farm_waves`` / ``farm_layout``; the new C entry points validate their arguments without a device and the
farm fails loudly without one.  CPU only."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import REPO
from farm_cases import JUNK, RAGGED, RAGGED_MULTIPLE, TILE, boundary_files

from mcevidence_amd import _capi, chain_io, farm


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_farm") / "chain_farm_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "chain_farm_check.cpp"), "-o", exe])
    return exe


def run_structure(exe, tmp_path, waves):
    """waves: [[bytes, ...]] -> per wave (wave_bytes, offsets, [(nrows, ncols, ragged, tok0, ntok)], tok_file, tok_off_in_file)"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for files in waves:
            f.write(struct.pack("<q", len(files)))
            f.write(np.array([len(b) for b in files], dtype="<i8").tobytes())
            for b in files:
                f.write(b)
    out = subprocess.run([exe, "structure", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(waves)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = open(fout, "rb").read()
    got, at = [], 0
    for files in waves:
        n = len(files)
        wave_bytes, = struct.unpack_from("<q", raw, at)
        at += 8
        offs = np.frombuffer(raw, dtype="<i8", count=n, offset=at)
        at += 8 * n
        ver = np.frombuffer(raw, dtype="<i8", count=5 * n, offset=at).reshape(n, 5)
        at += 40 * n
        ntok, = struct.unpack_from("<q", raw, at)
        at += 8
        tok_file = np.frombuffer(raw, dtype="<i8", count=ntok, offset=at)
        at += 8 * ntok
        tok_off = np.frombuffer(raw, dtype="<i8", count=ntok, offset=at)
        at += 8 * ntok
        got.append((wave_bytes, offs, ver, tok_file, tok_off))
    assert at == len(raw)
    return got


def host_verdict(tmp_path, data):
    """(nrows, ncols, ragged) of the host reader for these bytes; a file with no data has 0 rows and 0 columns"""
    p = tmp_path / "one.txt"
    p.write_bytes(data)
    try:
        a = chain_io.loadtxt(str(p))
    except ValueError as e:
        if "could not convert" in str(e):              # (a field that is no number is the parse pass's business)
            return None
        return (0, 0, 1)
    return (0, 0, 0) if a.shape[0] == 0 else (a.shape[0], a.shape[1], 0)


def check_wave(tmp_path, files, got):
    wave_bytes, offs, ver, tok_file, tok_off = got
    want_offs, want_bytes = farm.farm_layout([len(b) for b in files])
    assert list(offs) == want_offs and wave_bytes == want_bytes
    at = 0
    for f, data in enumerate(files):
        nrows, ncols, ragged, tok0, ntok = (int(x) for x in ver[f])
        assert tok0 == at
        at += ntok
        want = host_verdict(tmp_path, data)
        if want is None:           # (the host reader met a field that is no number first: it says nothing about the lines behind it)
            pass
        elif want[2]:
            assert ragged, (f, ver[f], want)
        else:
            assert (nrows, ncols, ragged) == want, (f, ver[f], want)
        # the token -> file map: the file's tokens are its own, each starts inside the file at a byte that is no blank
        mine = tok_file[tok0:tok0 + ntok]
        assert np.all(mine == f)
        inside = tok_off[tok0:tok0 + ntok]
        assert np.all((inside >= 0) & (inside < max(len(data), 1)))
        assert all(data[int(o):int(o) + 1] not in (b" ", b"\n", b"\r", b"\t", b"#") for o in inside[:50])
    assert at == len(tok_file)


def test_serial_driver_on_the_adversarial_files(checker, tmp_path):
    """the files of the GPU tests, in the given order, reversed and one per wave: rows, columns, ragged and the token ranges per file
    equal the host reader's for that file alone"""
    named = boundary_files(big_rows=400) + [("ragged", RAGGED), ("ragged_multiple", RAGGED_MULTIPLE), ("junk", JUNK)]
    files = [b for _, b in named]
    waves = [files, files[::-1]] + [[b] for b in files]
    got = run_structure(checker, tmp_path, waves)
    for w, g in zip(waves, got):
        check_wave(tmp_path, w, g)
    # the verdict of a file does not depend on its neighbours
    fwd, rev = got[0][2], got[1][2][::-1]
    assert np.array_equal(fwd[:, :3], rev[:, :3]) and np.array_equal(fwd[:, 4], rev[:, 4])


def test_a_file_alone_gets_the_verdict_it_gets_inside_a_wave(checker, tmp_path):
    """every adversarial file: file_counts + row_ragged at nfiles = 1, t0 = 0 (what the single-file reader's chain_ncols_kernel and
    chain_rows_kernel call) give the rows, columns, ragged flag and token count the same functions give it inside a wave"""
    named = boundary_files(big_rows=400) + [("ragged", RAGGED), ("ragged_multiple", RAGGED_MULTIPLE), ("junk", JUNK)]
    files = [b for _, b in named]
    waves = [files, files[::-1]]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for w in waves:
            f.write(struct.pack("<q", len(w)))
            f.write(np.array([len(b) for b in w], dtype="<i8").tobytes())
            f.write(b"".join(w))
    out = subprocess.run([checker, "alone", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(waves)), out.stdout[-2000:] + out.stderr[-2000:]
    got = np.fromfile(fout, dtype="<i8").reshape(len(waves), len(files), 2, 4)
    assert np.array_equal(got[:, :, 0], got[:, :, 1]), [n for (n, _), g in zip(named, got[0]) if not np.array_equal(g[0], g[1])]
    assert np.array_equal(got[0], got[1][::-1])
    assert got[0, :, 0, 2].any() and not got[0, :, 0, 2].all() and (got[0, :, 0, 3] == 0).any()      # ragged, whole and empty files all occur


def test_serial_driver_on_random_layouts(checker, tmp_path):
    """200 layouts of 1-9 files, lengths 0-3 tiles +- 1 byte, text drawn from the reader's alphabet"""
    rng = np.random.default_rng(2024)
    alphabet = np.frombuffer(b"0123456789.-e \n\n#\r\t", dtype=np.uint8)
    waves = []
    for _ in range(200):
        files = []
        for _ in range(int(rng.integers(1, 10))):
            n = max(0, int(rng.integers(0, 4)) * TILE + int(rng.integers(-1, 2)))
            if rng.random() < 0.5:                        # well-formed rows, cut to the length (the last line may be cut: ragged or not)
                ncols = int(rng.integers(1, 6))
                rows = "".join(" ".join("%d" % v for v in rng.integers(0, 1000, ncols)) + "\n" for _ in range(n // (2 * ncols) + 1))
                data = rows.encode()[:n]
            else:
                data = alphabet[rng.integers(0, len(alphabet), n)].tobytes()
            files.append(data)
        waves.append(files)
    got = run_structure(checker, tmp_path, waves)
    for w, g in zip(waves, got):
        check_wave(tmp_path, w, g)


def test_row_table_lookups_against_numpy(checker, tmp_path):
    """1-40 roots of 1-5 parts, empty parts (a burn-in at or beyond the end of a file) included: global row -> (root, part, local)"""
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(60):
        nroots = int(rng.integers(1, 41))
        nparts = rng.integers(1, 6, nroots)
        rows = [int(rng.integers(0, 700)) if rng.random() > 0.3 else 0 for _ in range(int(nparts.sum()))]
        cases.append((nparts, np.array(rows, dtype=np.int64)))
    cases.append((np.array([3]), np.array([0, 0, 5], dtype=np.int64)))
    cases.append((np.array([2, 2]), np.array([4, 0, 0, 3], dtype=np.int64)))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for nparts, rows in cases:
            f.write(struct.pack("<q", len(nparts)))
            f.write(np.asarray(nparts, dtype="<i8").tobytes())
            f.write(rows.astype("<i8").tobytes())
    out = subprocess.run([checker, "rows", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(cases)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = open(fout, "rb").read()
    at = 0
    for nparts, rows in cases:
        n, = struct.unpack_from("<q", raw, at)
        at += 8
        got = np.frombuffer(raw, dtype="<i8", count=3 * n, offset=at).reshape(n, 3)
        at += 24 * n
        assert n == rows.sum()
        root_of_part = np.repeat(np.arange(len(nparts)), nparts)
        want = np.concatenate([np.stack([np.full(r, root_of_part[p]), np.full(r, p), np.arange(r)], axis=1) for p, r in enumerate(rows)] or
                              [np.zeros((0, 3), dtype=np.int64)])
        assert np.array_equal(got, want)
    assert at == len(raw)


def test_farm_waves_and_layout():
    rng = np.random.default_rng(3)
    for _ in range(200):
        nroots = int(rng.integers(0, 30))
        lens = [[int(rng.integers(0, 4 * TILE)) for _ in range(int(rng.integers(1, 5)))] for _ in range(nroots)]
        sizes = [farm.farm_layout(x)[1] for x in lens]
        limit = int(rng.integers(1, 12)) * TILE
        waves = farm.farm_waves(sizes, limit)
        assert [i for w in waves for i in w] == list(range(nroots))                       # every root once, in order
        for w in waves:
            assert w and (sum(sizes[i] for i in w) <= limit or len(w) == 1)               # over the limit: a single oversized root only
        for x in lens:                                                                    # the pad rule
            offs, total = farm.farm_layout(x)
            ends = offs[1:] + [total]
            assert offs[0] == 0 and total % TILE == 0
            for o, n, e in zip(offs, x, ends):
                assert o % TILE == 0 and e >= o + n + 1 and e - (o + n + 1) < TILE
    assert farm.farm_waves([], TILE) == []
    assert farm.farm_waves([TILE, TILE, TILE], 2 * TILE) == [[0, 1], [2]]
    assert farm.farm_waves([9 * TILE, TILE], 2 * TILE) == [[0], [1]]
    assert farm.farm_layout([]) == ([], TILE) and farm.farm_layout([0]) == ([0], TILE) and farm.farm_layout([TILE - 1, TILE]) == ([0, TILE], 3 * TILE)
    with pytest.raises(ValueError):
        farm.farm_waves([TILE], 100)


def test_new_entry_points_validate_without_a_device():
    lib = _capi.load()
    h, st = ctypes.c_void_p(), ctypes.c_void_p()
    for cap in (0, 100, TILE + 1, -TILE, 1 << 40):
        assert lib.mce_chain_farm_create(cap, 0, ctypes.byref(h), ctypes.byref(st)) == _capi.MCE_ERR_INVALID
    assert lib.mce_chain_farm_create(TILE, 0, None, ctypes.byref(st)) == _capi.MCE_ERR_INVALID
    ntok = ctypes.c_int64()
    files = (_capi.FarmFile * 1)()
    assert lib.mce_chain_farm_structure(None, None, None, 1, TILE, files, ctypes.byref(ntok)) == _capi.MCE_ERR_INVALID
    assert lib.mce_chain_farm_parse(None, None, files, 1) == _capi.MCE_ERR_INVALID
    assert lib.mce_chain_farm_stats(None, None, 12) == _capi.MCE_ERR_INVALID
    # the device-source batch call: the host call's argument checks, no device needed
    assert lib.mce_evidence_feed_batch_dev_f64(None, 1, 0) == _capi.MCE_ERR_INVALID
    assert lib.mce_evidence_feed_batch_dev_f64(None, 0, 0) == _capi.MCE_OK
    assert lib.mce_evidence_feed_batch_dev_f64(None, -1, 0) == _capi.MCE_ERR_INVALID
    probs = (_capi.FeedProblem * 1)()
    assert lib.mce_evidence_feed_batch_dev_f64(probs, 1, -1) == _capi.MCE_ERR_INVALID
    with pytest.raises(ValueError, match="null pointer"):
        _capi.evidence_feed_batch_dev([(0, 10, 3, 0, 0, 0, 3, 0, 3, 0, 0)])
    with pytest.raises(ValueError, match="invalid sizes"):
        _capi.evidence_feed_batch_dev([(4096, 1, 3, 0, 0, 0, 3, 0, 3, 4096, 4096)])
    # the segmented preparation
    assert _capi.chain_farm_prep_workspace_bytes(0, 1, 10) == 0 and _capi.chain_farm_prep_workspace_bytes(3, 7, 5000) > 0
    ok = dict(root_nparts=[1, 2], root_ncols=[5, 4], parts=[(4096, 10), (4096, 0), (8192, 3)], iw=0, ilike=1, itheta=2, pos_lnp=False,
              d_params=4096, d_w=4096, d_like=4096, d_fs=4096, ws=4096, ws_bytes=1 << 20)
    for bad in (dict(root_ncols=[5, 2]), dict(root_nparts=[1, 1]), dict(root_nparts=[1, 3]), dict(parts=[(4096, 10), (0, 4), (8192, 3)]),
                dict(parts=[(4096, 10), (4096, 0), (8192, 0)]), dict(iw=-1), dict(d_fs=0), dict(ws=0)):
        with pytest.raises(ValueError):
            _capi.chain_farm_prep_dev(**dict(ok, **bad))
    with pytest.raises(ValueError, match="workspace"):
        _capi.chain_farm_prep_dev(**dict(ok, ws_bytes=8))


def test_the_farm_fails_loudly_without_a_gpu(tmp_path):
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    import mcevidence_amd as pkg
    p = tmp_path / "a_1.txt"
    p.write_bytes(b"1 2 3 4\n1 3 4 5\n")
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.evidence_many_from_files([str(tmp_path / "a")])
    with pytest.raises(RuntimeError, match="no HIP device"):
        farm.read_files([str(p)])
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.chain_farm_create(TILE)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.chain_farm_prep_dev([1], [5], [(4096, 10)], 0, 1, 2, False, 4096, 4096, 4096, 4096, 4096, 1 << 20)
