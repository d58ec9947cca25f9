"""The selection rules the host check and the device kernels share (mcevidence_amd/csrc/chain_prep.hpp), on the CPU: its serial
driver gives the indices and weights of ``chains.integer_weight_thin`` / ``chains.max_weight_bin_thin`` and the start of
``MCSamples.removeBurn``; ``resident.plan`` states the decline table; the resident entry points fail loudly without a device and
validate their arguments without one.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import REPO
from prep_cases import BIN_UNITS, BURNS, LENGTHS, bin_cases, integer_cases, unit_of

from mcevidence_amd import _capi, chains, resident


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_prep") / "chain_prep_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "chain_prep_check.cpp"), "-o", exe])
    return exe


def bin_edges(n, unit):
    nbins = int(n * unit) if unit < 1 else int(n // unit)          # (chains.max_weight_bin_thin)
    return np.linspace(-1, n, nbins + 1)


def run_select(exe, tmp_path, cases):
    """cases: [(w, thinlen, force, edges)] -> [(rule, keep, new_w)] from the header's serial driver"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for w, thinlen, force, edges in cases:
            f.write(struct.pack("<qdqq", len(w), thinlen, force, len(edges)))
            f.write(np.ascontiguousarray(w, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(edges, dtype="<f8").tobytes())
    out = subprocess.run([exe, "select", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(cases)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = open(fout, "rb").read()
    got, at = [], 0
    for _ in cases:
        rule, nout = struct.unpack_from("<qq", raw, at)
        at += 16
        keep = np.frombuffer(raw, dtype="<i8", count=nout, offset=at)
        at += 8 * nout
        new_w = np.frombuffer(raw, dtype="<f8", count=nout, offset=at)
        at += 8 * nout
        got.append((rule, keep, new_w))
    assert at == len(raw)
    return got


def test_integer_rule_equals_integer_weight_thin(checker, tmp_path):
    """lengths 1 .. 70 001, weights from [0, hi], hi in {1, 2, 6, 50}, factors on either side of the maximum and equal to it, and
    weights up to 100 000 at 70 001 rows (the prefix sum passes 2^32): same indices, same weights"""
    cases = list(integer_cases())
    got = run_select(checker, tmp_path, [(w, f, 0, []) for _, w, f in cases])
    branches = set()
    for (name, w, f), (rule, keep, new_w) in zip(cases, got):
        want_keep, want_w = chains.integer_weight_thin(w, f)
        if f == 1.0:
            assert rule == 0 and np.array_equal(keep, np.arange(len(w))) and np.array_equal(new_w, w), name      # thinlen 1: no thinning
            continue
        assert rule == 1, name
        assert np.array_equal(keep, want_keep) and np.array_equal(new_w, want_w.astype(np.float64)), name
        branches.add(bool(f >= w.astype(int).max()))
        assert np.array_equal(chains.thin_rows(w, f)[0], keep), name
    assert branches == {True, False}


def test_bin_rule_equals_max_weight_bin_thin(checker, tmp_path):
    """units 0.5 .. n + 1 with a third of the weights tied: same indices, same weights (the rule is forced: below a unit of 1 the
    dispatch would draw Poisson weights)"""
    cases = list(bin_cases())
    got = run_select(checker, tmp_path, [(w, u, 2, bin_edges(len(w), u)) for _, w, u in cases])
    longer = 0
    for (name, w, u), (rule, keep, new_w) in zip(cases, got):
        want_keep, want_w = chains.max_weight_bin_thin(w, u)
        assert rule == 2 and np.array_equal(keep, want_keep) and np.array_equal(new_w, want_w), name
        longer += len(keep) > 1
    assert longer > len(cases) // 2
    # and the dispatch takes the bin rule by itself for weights that are not integers, or a factor that is not
    picks = [(w, u, 0, bin_edges(len(w), u)) for _, w, u in cases if u > 1] + [(np.round(w), 7.5, 0, bin_edges(len(w), 7.5)) for _, w, u in cases[::9]]
    for (w, u, _, _), (rule, keep, new_w) in zip(picks, run_select(checker, tmp_path, picks)):
        want_keep, want_w = chains.thin_rows(w, u)
        assert rule == 2 and np.array_equal(keep, want_keep) and np.array_equal(new_w, want_w)


def test_rule_choice_and_declines(checker, tmp_path):
    w = np.asarray([1.0, 2.0, 3.0, 2.0, 1.0] * 20)
    near = w.copy()
    near[3] += 1e-4 + 4e-7                     # fractional sum within 1e-6 of the threshold
    over = w.copy()
    over[3] += 3e-4
    under = w.copy()
    under[3] += 5e-5
    neg = w.copy()
    neg[7] = -1.0
    nan = w.copy()
    nan[7] = np.nan
    inf = w.copy()
    inf[7] = np.inf
    edges = bin_edges(len(w), 2.0)
    cases = [(w, 2.0, 0, edges), (near, 2.0, 0, edges), (over, 2.0, 0, edges), (under, 2.0, 0, edges), (neg, 2.0, 0, edges), (nan, 2.0, 0, edges),
             (inf, 2.0, 0, edges), (w, 0.0, 0, []), (w, 1.0, 0, []), (w, 0.5, 0, []), (w, -2.0, 0, []), (neg, 0.0, 0, [])]
    rules = [r for r, _, _ in run_select(checker, tmp_path, cases)]
    assert rules == [1, -2, 2, 1, -1, -1, -1, 0, 0, -3, -3, 0]
    # the two thinned ones agree with the host's dispatch
    got = run_select(checker, tmp_path, [cases[2], cases[3]])
    for (ww, f, _, _), (_, keep, new_w) in zip([cases[2], cases[3]], got):
        hk, hw = chains.thin_rows(ww, f)
        assert np.array_equal(keep, hk) and np.array_equal(new_w, np.asarray(hw, dtype=np.float64))


def test_burn_start_equals_remove_burn(checker, tmp_path):
    pairs = []
    for n in LENGTHS:
        for b in BURNS:
            pairs.append((n, unit_of(b, n)))
    fin = tmp_path / "burn.bin"
    fin.write_bytes(b"".join(struct.pack("<qd", n, b) for n, b in pairs))
    out = subprocess.check_output([checker, "burn", str(fin)]).decode().split()
    assert out[-1] == "records=%d" % len(pairs)
    for (n, b), got in zip(pairs, out):
        chain = np.zeros((n, 3))
        want = n - (chains.MCSamples.removeBurn(_Quiet(), b, chain).shape[0] if b > 0 else n)
        assert int(got) == want, (n, b)


class _Quiet(object):
    class logger(object):
        info = staticmethod(lambda *a, **k: None)


DECLINE_TABLE = [
    (dict(thinlen=0.5), "poisson"), (dict(thinlen=-2), "negative_thinlen"), (dict(isfunc=lambda s: 0.0), "isfunc"),
    (dict(brange=[3, 4]), "batches"), (dict(nbatch=3), "batches"), (dict(verbose=2), "verbose"), (dict(covtype="diag"), "covtype"),
    (dict(split=True, covtype="single"), "split_single"), (dict(ndim=128), "ndim"), (dict(ndim=None, nparam=200), "ndim"),
    (dict(distributed=True), "distributed"), (dict(ncols=[23, 23, 24]), "columns"), (dict(nrows=1), "rows"), (dict(nrows=0), "rows"),
]


def test_plan_states_the_decline_table():
    for kw, key in DECLINE_TABLE:
        assert resident.plan(**kw) == resident.REASONS[key], kw
    for kw in (dict(), dict(thinlen=0), dict(thinlen=1), dict(thinlen=2), dict(thinlen=7.5), dict(covtype="single"), dict(split=True), dict(ndim=127),
               dict(ndim=500, nparam=21), dict(ncols=[23, 23]), dict(nrows=2), dict(verbose=0), dict(split=True, covtype="all", ndim=6, nparam=21)):
        assert resident.plan(**kw) == "resident", kw
    assert len(set(resident.REASONS.values())) == len(resident.REASONS)


def test_resident_route_fails_loudly_without_a_device(tmp_path):
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    chs, names, ranges = planck_like_chains(seed=3, rows=(300, 280))
    root = str(tmp_path / "pl")
    write_cosmomc_chains(root, chs, ranges)
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.evidence_from_files(root, kmax=3)
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.evidence_from_files(root, thinlen=0.5)             # (a decline does not turn into a host run either)
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.ResidentChains.from_arrays(chs, thinlen=2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        pkg.ResidentChains.from_files(root)


def test_entry_points_validate_without_a_device():
    """null / inconsistent arguments are MCE_ERR_INVALID (ValueError) before any device call; the rest is MCE_ERR_NO_DEVICE"""
    lib = _capi.load()
    for name in ("mce_chain_dev_read_dev", "mce_chain_weights_dev", "mce_chain_select_count_dev", "mce_chain_select_fill_dev", "mce_chain_gather_dev",
                 "mce_chain_reduce_dev", "mce_chain_select_workspace_bytes", "mce_chain_gather_workspace_bytes", "mce_chain_reduce_workspace_bytes"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert lib.mce_abi_version() == 3
    assert _capi.chain_select_workspace_bytes(1000, 4) >= 1000 * 24 and _capi.chain_select_workspace_bytes(-1, 4) == 0
    assert _capi.chain_gather_workspace_bytes(4) >= 4 * 24 and _capi.chain_gather_workspace_bytes(0) == 0
    assert _capi.chain_reduce_workspace_bytes(1000) > 0
    P = 0x1000          # never dereferenced: every call below fails in its argument checks
    with pytest.raises(ValueError, match="null handle"):
        _capi.chain_dev_read_dev(None, P)
    with pytest.raises(ValueError):
        _capi.chain_weights_dev([(P, 10)], 4, 0, 2.0, 0, 1 << 20)                     # null workspace
    with pytest.raises(ValueError):
        _capi.chain_weights_dev([(0, 10)], 4, 0, 2.0, P, 1 << 20)                     # rows at a null pointer
    with pytest.raises(ValueError):
        _capi.chain_weights_dev([(P, -1)], 4, 0, 2.0, P, 1 << 20)                     # negative count
    with pytest.raises(ValueError):
        _capi.chain_weights_dev([(P, 10)], 4, 4, 2.0, P, 1 << 20)                     # weight column beyond the row
    with pytest.raises(ValueError):
        _capi.chain_weights_dev([(P, 10)], 4, 0, 2.0, P, 16)                          # workspace too small
    with pytest.raises(ValueError):
        _capi.chain_select_count_dev(10, 1, 2, 2.0, 0, 6, P, 1 << 20)                 # the bin rule without edges
    with pytest.raises(ValueError):
        _capi.chain_select_count_dev(10, 1, 0, 2.0, 0, 0, P, 1 << 20)                 # a rule that selects nothing
    with pytest.raises(ValueError):
        _capi.chain_select_count_dev(-3, 1, 1, 2.0, 0, 0, P, 1 << 20)
    with pytest.raises(ValueError):
        _capi.chain_select_fill_dev(10, 1, 1, 2.0, 0, 5, 0, P, P, 1 << 20)            # null output
    with pytest.raises(ValueError):
        _capi.chain_select_fill_dev(10, 1, 1, 2.0, 0, 0, P, P, P, 1 << 20)            # nothing to fill
    for iw, il, it in ((4, 1, 2), (0, 4, 2), (0, 1, 4), (-1, 1, 2)):                  # ncols <= max(iw, ilike, itheta)
        with pytest.raises(ValueError, match="columns"):
            _capi.chain_gather_dev([(P, 10)], 4, iw, il, it, 0, 0, 10, 0, 10, P, P, P, 0, P, 1 << 20)
    with pytest.raises(ValueError):
        _capi.chain_gather_dev([(P, 10)], 4, 0, 1, 2, 0, 0, 10, 0, 10, 0, 0, 0, 0, P, 1 << 20)      # no output at all
    with pytest.raises(ValueError):
        _capi.chain_gather_dev([(P, 10)], 4, 0, 1, 2, 0, 0, 7, 0, 7, P, P, P, 0, P, 1 << 20)        # n_thin != n without a row list
    with pytest.raises(ValueError):
        _capi.chain_reduce_dev(0, P, 10, False, P, P, 1 << 20)
    with pytest.raises(ValueError):
        _capi.chain_reduce_dev(P, P, -1, False, P, P, 1 << 20)
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_weights_dev([(P, 10)], 4, 0, 2.0, P, 1 << 20)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_select_count_dev(10, 1, 1, 2.0, 0, 0, P, 1 << 20)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_gather_dev([(P, 10)], 4, 0, 1, 2, 0, 0, 10, 0, 10, P, P, P, 0, P, 1 << 20)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_reduce_dev(P, P, 10, False, P, P, 1 << 20)
