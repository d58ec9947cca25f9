"""The resident route (mcevidence_amd/resident.py: chain files -> parsed on the device -> burn-in, thinning, split, column split,
fs / SumW there -> mce_evidence_feed_part_dev_f64) against chains.py, the reference's own pins and the host route.  Every
comparison of a result asserts ``route == "resident"`` first, so a fallback cannot pass for the feature.

Spans of the scan the kernels use (csrc/chain_prep_kernels.hpp): a TILE is 512 rows, one ROUND of the single-block scan takes
256 tiles = 131 072 rows, and the running sum carried from round to round is the second level (first crossed twice at 262 144)."""
import math
import mmap
import os

import numpy as np
import pytest

import mcevidence_amd as pkg
from mcevidence_amd import _capi, chain_io, chains, resident
from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
from helpers import host_pins
from prep_cases import LENGTHS, bin_cases, int_weights, integer_cases, tied_float_weights
from test_chain_reader import TOKENS

pytestmark = pytest.mark.gpu

TILE, ROUND = 512, 512 * 256
SPAN_LENGTHS = (TILE - 1, TILE, TILE + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND - 1, 2 * ROUND, 2 * ROUND + 1)
PINS = host_pins()
LNE_PARITY = 1e-9           # the project's stated parity bound on ln E (tests/helpers.py: LNE_TOL)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def chain_with_weights(w, ncols=3, seed=0):
    """a chain [len(w), ncols] whose column 0 is w (the other columns only have to be there)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((len(w), ncols))
    a[:, 0] = w
    return a


def check_selection(w, thinlen, name):
    rc = pkg.ResidentChains.from_arrays([chain_with_weights(w)], thinlen=thinlen)
    want_keep, want_w = chains.thin_rows(w, thinlen) if thinlen != 1 else (np.arange(len(w)), w)
    keep = rc.keep()
    assert keep.dtype == np.int64 and np.array_equal(keep, want_keep), name
    assert same(rc.weights(), np.asarray(want_w, dtype=np.float64)), name
    assert rc.nrows == len(want_keep), name
    return rc.rule


# ---------------------------------------------------------------------------------------------------------------- 1. selection
@pytest.mark.parametrize("n", LENGTHS)
def test_selection_equals_thin_rows_on_the_cpu_shapes(n):
    """keep() and the weights against chains.thin_rows: the integer cases of the CPU test (both branches, factor == max, the
    prefix beyond 2^32 at 70 001 rows) and its bin cases with a unit above 1 (0.5 and 1 never reach the device: Poisson / no-op)"""
    rules = set()
    for name, w, f in integer_cases(lengths=(n,)):
        rules.add(check_selection(w, f, name))
    for name, w, u in bin_cases(lengths=(n,)):
        if u > 1:
            rules.add(check_selection(w, u, name))
    assert rules >= ({"none", "integer", "bin"} if n > 1 else {"none", "integer"})


@pytest.mark.parametrize("n", SPAN_LENGTHS)
def test_selection_at_the_spans_of_the_scan(n):
    """one below, at and one above a tile (512 rows), a round of the block scan (131 072) and the second round's end (262 144)"""
    w = int_weights(n, 6, seed=n)
    for f in (3.0, 6.0, 50.0):                      # second branch (rows repeat), factor == max, first branch
        assert check_selection(w, f, "span n=%d f=%g" % (n, f)) == "integer"
    wf = tied_float_weights(n, seed=n + 1)
    for u in (2.0, 7.5):
        assert check_selection(wf, u, "span n=%d unit=%g" % (n, u)) == "bin"
    # heavy weights: the compaction's count and the prefix both cross the spans with large values
    wh = int_weights(n, 100000, seed=n + 2, lo=1)
    assert check_selection(wh, 100000.0, "span n=%d heavy" % n) == "integer"


@pytest.mark.parametrize("ncols, itheta", [(3, 2), (4, 2), (4, 3), (23, 2), (23, 3), (29, 2), (29, 3)])
@pytest.mark.parametrize("thin", [0, 3, 2.5])
def test_to_host_equals_numpy_burn_concatenate_thin(ncols, itheta, thin):
    """four chains of unequal length, one of them emptied by its burn-in; the uint64 view of to_host() against NumPy"""
    rng = np.random.default_rng(ncols * 10 + itheta)
    chs = []
    for i, n in enumerate((1300, 400, 2100, 777)):
        a = rng.standard_normal((n, ncols))
        a[:, 0] = 1.0 + rng.poisson(3.0, n)
        a[rng.integers(0, n, 5), 1] = -0.0          # (bit patterns count)
        chs.append(a)
    for burn in (500, 0.3):
        rc = pkg.ResidentChains.from_arrays(chs, burnlen=burn, thinlen=thin, itheta=itheta)
        burned = [c[(int(len(c) * burn) if burn < 1 else int(burn)):] for c in chs]
        assert burn != 500 or len(burned[1]) == 0
        s = np.concatenate(burned)
        if thin:
            keep, neww = chains.thin_rows(s[:, 0], thin)
            s = s[keep, :]
            s[:, 0] = neww
            assert np.array_equal(rc.keep(), keep)
        assert rc.rule == {0: "none", 3: "integer", 2.5: "bin"}[thin]
        assert rc.nrows == len(s) and rc.nparam == ncols - itheta
        assert same(rc.to_host(), s)


# ---------------------------------------------------------------------------------------------------------------- 2. the reader
def read_to_device_and_back(path):
    import torch
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            view = np.frombuffer(mm, dtype=np.uint8)
            handle, nrows, ncols = _capi.chain_dev_open(view.ctypes.data, len(view), 0)
            try:
                out = torch.empty((nrows, ncols), dtype=torch.float64, device="cuda:0")
                stats = _capi.chain_dev_read_dev(handle, out.data_ptr())
            finally:
                _capi.chain_dev_close(handle)
            del view
        finally:
            mm.close()
    return out.cpu().numpy(), stats


def test_reader_into_device_memory_equals_the_host_reader(tmp_path):
    p = str(tmp_path / "tok.txt")
    open(p, "w").write("\n".join(TOKENS) + "\n")
    got, stats = read_to_device_and_back(p)
    assert same(got, chain_io.loadtxt(p)) and 0 < stats["patched"] < len(TOKENS)          # (some tokens patched by the host)
    rng = np.random.default_rng(2)
    a = rng.standard_normal((20_000, 12)) * np.asarray([1e-3, 1.0, 70.0, 100.0])[rng.integers(0, 4, (20_000, 12))]
    p = str(tmp_path / "g17.txt")
    np.savetxt(p, a, fmt="%.17g")
    got, stats = read_to_device_and_back(p)
    assert same(got, chain_io.loadtxt(p)) and same(got, a) and stats["tokens"] == a.size
    rows = ["%.7E %.7E %.7E" % tuple(r) for r in rng.standard_normal((3000, 3))]
    for name, line in (("ragged", "1.0 2.0"), ("junk", "1.0 x2.0 3.0")):
        bad = list(rows)
        bad[2117] = line
        p = str(tmp_path / (name + ".txt"))
        open(p, "w").write("# head\n" + "\n".join(bad) + "\n")
        with pytest.raises(ValueError) as host:
            chain_io.loadtxt(p)
        with pytest.raises(ValueError) as dev:
            pkg.ResidentChains.from_files(p)
        assert str(dev.value) == str(host.value)


# ---------------------------------------------------------------------------------------------------------------- 3. the pins
@pytest.fixture(scope="module")
def planck_root(tmp_path_factory):
    td = tmp_path_factory.mktemp("chains")
    chs, names, ranges = planck_like_chains(seed=1)
    root = os.path.join(str(td), "base_plikHM_TT_lowTEB")
    write_cosmomc_chains(root, chs, ranges)
    return root, chs, ranges


@pytest.mark.parametrize("tag", ["burn0.3", "burn500", "thin2", "thin5", "thin10", "burn0.2_thin3"])
def test_reference_pins_burn_thin(planck_root, tag):
    root, _, _ = planck_root
    p = PINS["file_" + tag]
    rc = pkg.ResidentChains.from_files(root, **p["kw"])
    lnE, info = rc.evidence(ndim=6, priorvolume=1.0, kmax=3, info=True)
    assert info["route"] == "resident"
    assert rc.nrows == p["N"]
    s = rc.to_host()
    assert math.isclose(float(np.sum(s[:, 0])), p["sumw"], rel_tol=1e-12)
    assert math.isclose(float(np.sum(s[:, 1])), p["sumlike"], rel_tol=1e-12)
    assert math.isclose(float(np.sum(s[:, 2])), p["sum_p0"], rel_tol=1e-10)
    print(tag, "max |dlnE| against the pin:", float(np.max(np.abs(lnE - np.asarray(p["lnE"])))))
    assert np.allclose(lnE, p["lnE"], rtol=0, atol=1e-8)


def test_reference_pin_float_weights_take_the_bin_rule(planck_root, tmp_path):
    _, chs, _ = planck_root
    fch = [c.copy() for c in chs]
    rng = np.random.default_rng(5)
    for c in fch:
        c[:, 0] = c[:, 0] * (0.5 + rng.random(len(c)))
    rootf = os.path.join(str(tmp_path), "floatw")
    write_cosmomc_chains(rootf, fch, None)
    p = PINS["file_floatw_thin4"]
    rc = pkg.ResidentChains.from_files(rootf, thinlen=4)
    lnE, info = rc.evidence(ndim=6, priorvolume=1.0, kmax=3, info=True)
    assert info["route"] == "resident" and rc.rule == "bin"
    assert rc.nrows == p["N"]
    s = rc.to_host()
    assert math.isclose(float(np.sum(s[:, 0])), p["sumw"], rel_tol=1e-9)
    assert math.isclose(float(np.sum(s[:, 1])), p["sumlike"], rel_tol=1e-9)
    assert np.allclose(lnE, p["lnE"], rtol=0, atol=1e-8)


def test_reference_pins_C1(planck_root):
    root, _, _ = planck_root
    pi = pkg.params_info(root, cosmo=True)
    lnE, info = pkg.evidence_from_files(root, ndim=pi["ndim"], priorvolume=pi["volume"], kmax=2, verbose=0, info=True, require_resident=True)
    assert info["route"] == "resident"
    assert info["Nsamples"] == "26862" and info["NparamsMC"] == 21 and info["NparamsCosmo"] == 6 and PINS["C1_all"]["N"] == 26862
    assert np.allclose(lnE, PINS["C1_all"]["lnE"], rtol=0, atol=1e-8)
    for ic in (1, 2, 3, 4):
        lnE, info = pkg.evidence_from_files(root, ndim=6, priorvolume=pi["volume"], kmax=2, verbose=0, idchain=ic, info=True)
        assert info["route"] == "resident" and info["Nsamples"] == str(PINS["C1_chain%d" % ic]["N"])
        assert np.allclose(lnE, PINS["C1_chain%d" % ic]["lnE"], rtol=0, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------- 4. the host route
@pytest.fixture(scope="module")
def small_root(tmp_path_factory):
    td = tmp_path_factory.mktemp("small")
    chs, names, ranges = planck_like_chains(seed=4, rows=(6000, 5500, 6200, 5800))
    root = os.path.join(str(td), "pl")
    write_cosmomc_chains(root, chs, ranges)
    neg = [c.copy() for c in chs]
    for c in neg:
        c[:, 1] = -c[:, 1]
    rootn = os.path.join(str(td), "neg")
    write_cosmomc_chains(rootn, neg, None)
    pair = planck_like_chains(seed=6, rows=(6000, 6000))[0]
    rootp = os.path.join(str(td), "pair")
    write_cosmomc_chains(rootp, pair, None)
    return dict(plain=root, negated=rootn, pair=rootp)


HOST_CASES = {
    "thin20": dict(ctor=dict(thinlen=20), rule="integer"),                      # factor >= max weight: the first integer branch
    "thin2": dict(ctor=dict(thinlen=2), rule="integer"),
    "burn0.1_thin2": dict(ctor=dict(burnlen=0.1, thinlen=2), rule="integer"),
    "single": dict(ctor=dict(), covtype="single", rule="none"),
    "pos_lnp": dict(ctor=dict(), root="negated", pos_lnp=True, rule="none"),
    "ndim6": dict(ctor=dict(ndim=6), rule="none"),
    "split": dict(ctor=dict(split=True), seed=11, rule="none"),
    "split_thin3": dict(ctor=dict(split=True, thinlen=3, s1frac=0.4), seed=11, rule="integer"),
    "split_rows": dict(ctor=dict(), root="pair", split_rows=True, rule="none"),
    "recheck": dict(ctor=dict(), recheck=64, rule="none"),
}


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_against_the_host_route_on_the_same_files(small_root, monkeypatch, name):
    """to_host() bitwise equal to MCEvidence(root, ...).gd.samples and ln E within the parity bound of 1e-9"""
    case = HOST_CASES[name]
    root = small_root[case.get("root", "plain")]
    ctor = dict(case["ctor"])
    covtype = case.get("covtype", "all")
    pos = case.get("pos_lnp", False)
    kmax = 4
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    backend = pkg.HipBackend(recheck_rows=case["recheck"]) if "recheck" in case else None
    # ---- host
    if "seed" in case:
        np.random.seed(case["seed"])
    m = pkg.MCEvidence(root, kmax=kmax, verbose=0, **ctor, **({"backend": backend} if backend else {}))
    rows = (np.arange(6000), np.arange(6000, 12000)) if case.get("split_rows") else None
    if rows:
        m.set_split(*rows)
    want, winfo = m.evidence(covtype=covtype, pos_lnp=pos, info=True)
    host_next = np.random.random() if "seed" in case else None
    # ---- resident
    if "seed" in case:
        np.random.seed(case["seed"])
    rc = pkg.ResidentChains.from_files(root, burnlen=ctor.get("burnlen", 0), thinlen=ctor.get("thinlen", 0))
    got, info = rc.evidence(kmax=kmax, ndim=ctor.get("ndim"), covtype=covtype, pos_lnp=pos, split=ctor.get("split", False),
                            s1frac=ctor.get("s1frac", 0.5), split_rows=rows, info=True, backend=backend)
    assert info["route"] == "resident"
    if "seed" in case:
        assert np.random.random() == host_next           # the split consumed the RNG exactly as MCSamples.chain_split does
    assert rc.rule == case["rule"]
    assert same(rc.to_host(), m.gd.samples)
    for k in ("NparamsMC", "Nsamples_read", "Nparams_read", "NparamsCosmo", "Nsamples"):
        assert info[k] == winfo[k], k
    err = float(np.max(np.abs(got - want)))
    print("%s: max |lnE(resident) - lnE(host)| = %.3e" % (name, err))
    assert got.shape == want.shape and err <= LNE_PARITY


def test_evidence_from_files_and_the_cli_flag(small_root, monkeypatch, capsys):
    root = small_root["plain"]
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    want = pkg.MCEvidence(root, kmax=3, verbose=0, burnlen=0.1, thinlen=2, ndim=6).evidence()
    got, info = pkg.evidence_from_files(root, kmax=3, verbose=0, burnlen=0.1, thinlen=2, ndim=6, info=True)
    assert info["route"] == "resident" and "declined" not in info
    assert float(np.max(np.abs(got - want))) <= LNE_PARITY
    plain = pkg.evidence_from_files(root, kmax=3, verbose=0, burnlen=0.1, thinlen=2, ndim=6)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, got)
    # a call the table declines runs the host route unchanged, and says so
    np.random.seed(3)
    want = pkg.MCEvidence(root, kmax=3, verbose=0, thinlen=0.5).evidence()
    np.random.seed(3)
    got, info = pkg.evidence_from_files(root, kmax=3, verbose=0, thinlen=0.5, info=True)
    assert info["route"] == "host" and info["declined"] == resident.REASONS["poisson"] and np.array_equal(got, want)
    with pytest.raises(ValueError, match="Poisson"):
        pkg.evidence_from_files(root, kmax=3, verbose=0, thinlen=0.5, require_resident=True)
    from mcevidence_amd import cli
    args = [root, "-k", "3", "-vb", "0", "--burn", "0.1", "--thin", "2"]
    out, host = cli.main(args + ["--resident"]), cli.main(args)
    assert out.shape == host.shape and float(np.max(np.abs(out - host))) <= LNE_PARITY


# ---------------------------------------------------------------------------------------------------------------- 5. declines found on the device
@pytest.mark.parametrize("kind, reason", [("near", "ambiguous_weights"), ("negative", "bad_weights"), ("nan", "bad_weights")])
def test_weight_declines_found_on_the_device(tmp_path, monkeypatch, kind, reason):
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    chs = planck_like_chains(seed=8, rows=(3000, 2500))[0]
    if kind == "near":
        chs[0][17, 0] += 1e-4 + 4e-7                   # the fractional parts sum to within 1e-6 of the host's threshold
    elif kind == "negative":
        chs[1][5, 0] = -2.0
    else:
        chs[1][5, 0] = np.nan
    root = str(tmp_path / kind)
    write_cosmomc_chains(root, chs, None, fmt="%.17g")
    with pytest.raises(ValueError) as req:
        pkg.evidence_from_files(root, kmax=3, verbose=0, thinlen=2, ndim=6, require_resident=True)
    assert str(req.value) == resident.REASONS[reason]
    with pytest.raises(resident.ResidentDecline):
        pkg.ResidentChains.from_files(root, thinlen=2)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            want = pkg.MCEvidence(root, kmax=3, verbose=0, thinlen=2, ndim=6).evidence()
        except Exception as exc:                         # the host route's own exception must come through the fallback
            with pytest.raises(type(exc)) as got:
                pkg.evidence_from_files(root, kmax=3, verbose=0, thinlen=2, ndim=6, info=True)
            assert str(got.value) == str(exc)
            return
        got, info = pkg.evidence_from_files(root, kmax=3, verbose=0, thinlen=2, ndim=6, info=True)
    assert info["route"] == "host" and info["declined"] == resident.REASONS[reason]
    assert np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- 6. lifetime
def test_two_resident_chains_alive_then_released(small_root):
    import gc
    root = small_root["plain"]
    a = pkg.ResidentChains.from_files(root, thinlen=2)
    b = pkg.ResidentChains.from_files(small_root["pair"], burnlen=0.2)
    first, info = a.evidence(kmax=3, ndim=6, info=True)
    assert info["route"] == "resident"
    other = b.evidence(kmax=3, ndim=6)
    again = a.evidence(kmax=3, ndim=6)
    assert np.array_equal(first, again) and same(a.to_host(), a.to_host()) and not np.array_equal(first, other)
    del a, b
    gc.collect()
    _capi.release_device_memory()
    c = pkg.ResidentChains.from_files(root, thinlen=2)
    third, info = c.evidence(kmax=3, ndim=6, info=True)
    assert info["route"] == "resident" and np.array_equal(first, third)
