"""contours with hard prior bounds on the CPU: the serial driver of csrc/param_contours.hpp's steps 3" .. 8" (a stand-alone sanitized
program) and ``contours.measure_bounded`` on the cases of tests/contours_bounds_cases.py -- the grid that ends on a bound, every density
within its derived bound of the exact three-term boundary-kernel estimate at the reported parameters (mpmath on the query cells, the
extended format on all), the two forms within two bounds of each other, every decision bit for bit the serial rule's on the block's own
densities, at most two undecided cells per (pair, p) against the oracle; a pair of two open columns byte-equal to the rule without
bounds; pair independence; the statuses; the invalid arguments; the keyword; and the Exponential corner, which the rule without bounds fails.

The Exponential corner (docs/design/contours_bounds.md): two independent Exponential(1) columns bounded at 0.  The true region of
probability p is x + y <= t with 1 - exp(-t)(1 + t) = p, of area t^2 / 2, and dA/dp = exp(t).  The level is set by the sample: the share
of the sample inside a fixed region has the standard deviation sqrt(p (1 - p) / ess); at 5 sigma that is 5 exp(t) sqrt(p (1 - p) / ess)
= 0.19 at p = 0.68, 6.9 % of the area.  The cell-counting term of test_param_contours_shared.py's area check is deliberately NOT
added: it would be 0.8 and would let the estimate without the correction pass.  Observed on seeds 0 - 4 with ``measure_bounded`` (and, to the digits
printed, on the device): the 68 % area is 2.718 to 2.828 and misses t^2 / 2 = 2.769 by 0.006 to 0.059, the 95 % area is 11.08 to 11.40
(truth 11.252; not gated: its sampling term is 0.97), the corner density 1.01 to 1.11; the rule without bounds on the same draws has its
mode inside ((0.25 .. 0.34, 0.25 .. 0.36)), lower < 0 and a 68 % area of 3.85 to 4.00."""
import logging

import numpy as np
import pytest

import contours_bounds_cases as cb
import contours_cases as cc
from mcevidence_amd import contours as ct

INF = float("inf")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cb.build_checker(tmp_path_factory.mktemp("param_contours_bounds"))


@pytest.fixture(scope="module")
def plain_checker(tmp_path_factory):
    return cc.build_checker(tmp_path_factory.mktemp("param_contours_plain"))


def test_the_pieces_of_the_rule(checker):
    import subprocess
    out = subprocess.run([checker, "rule"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=11"), out.stdout + out.stderr


def test_every_case_has_every_kind_of_pair():
    kinds = set()
    for c in cb.cases().values():
        kinds |= set(c.kinds)
        assert c.x.shape[1] == c.d + 2 and np.all(c.lo < c.hi)
        if c.nc >= 3:
            opens = [c.open_t(t) for t in range(c.nc)]
            assert any(opens) and not all(opens), c.name
    assert kinds == set(cb.KINDS)
    assert cb.cases()["n513_nc6_G64_fractional"].kinds == cb.KINDS
    c = cb.cases()["n1025_nc6_G32_integer"]
    assert {(c.open_t(s), c.open_t(t)) for s, t in ct.pairs(c.nc)} == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("name", list(cb.cases()))
def test_serial_driver_and_numpy_against_the_oracle(name, checker, tmp_path):
    c = cb.cases()[name]
    native = cb.native_case(checker, tmp_path, c)
    host = ct.measure_bounded(c.a, c.x[:, :c.d], c.cols, c.bounds, c.probs, c.grid, c.scale)
    stats = {}
    for what, got in (("serial", native), ("numpy", host)):
        assert np.all(np.asarray(got["col_status"]) == 0), (name, got["col_status"])
        assert (got["status"], got["column"], got["rows"], got["grid"], got["nc"]) == (0, -1, c.n, c.grid, c.nc)
        for p, s, t in cb.oracle_pairs(c):
            cb.check_pair(c, got, p, s, t, what, stats=stats)
        cb.check_against_numpy(c, got, what)
    assert cb.check_decisions_native(checker, tmp_path, [native, host], c.probs, c.grid) == 2 * c.nc * (c.nc - 1) // 2
    assert stats["undecided"] <= cb.MAX_UNDECIDED


@pytest.mark.parametrize("name", list(cb.cases()))
def test_open_pairs_are_the_rule_without_bounds_bit_for_bit(name, checker, plain_checker, tmp_path):
    c = cb.cases()[name]
    native = cb.native_case(checker, tmp_path, c)
    plain, = cc.run_native(plain_checker, tmp_path, [(c.a, c.x, c.d)], c.cols, c.probs, c.grid, c.scale)
    host = ct.measure_bounded(c.a, c.x[:, :c.d], c.cols, c.bounds, c.probs, c.grid, c.scale)
    host_plain = ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid, c.scale)
    want = sum(1 for s, t in ct.pairs(c.nc) if c.open_t(s) and c.open_t(t))
    assert cb.assert_open_pairs_equal(c, native, plain, (name, "serial")) == want
    assert cb.assert_open_pairs_equal(c, host, host_plain, (name, "numpy")) == want
    # every bound open: the whole call is the call without bounds on every shared key
    o = cb.open_case(c)
    assert cb.equal_common(cb.native_case(checker, tmp_path, o), plain), name
    all_open = ct.measure_bounded(o.a, o.x[:, :o.d], o.cols, o.bounds, o.probs, o.grid, o.scale)
    assert cb.equal_common(all_open, host_plain), name
    assert np.all(all_open["at_lo"] == 0.0) and np.all(all_open["at_hi"] == 0.0) and np.all(np.isinf(all_open["bound_lo"]))


def test_a_pair_does_not_notice_the_others_nor_the_probabilities(checker, tmp_path):
    c = cb.cases()["n513_nc6_G64_fractional"]
    whole = cb.native_case(checker, tmp_path, c)
    host = ct.measure_bounded(c.a, c.x[:, :c.d], c.cols, c.bounds, c.probs, c.grid, c.scale)
    for s, t in ((1, 4), (0, 5), (3, 5)):
        sub = cb.sub_case(c, (s, t))
        p = ct.pairs(c.nc).index((s, t))
        alone = cb.native_case(checker, tmp_path, sub)
        assert cb.pair_values(whole, p).tobytes() == cb.pair_values(alone, 0).tobytes(), (s, t)
        other, = cb.run_native(checker, tmp_path, [(sub.a, sub.x, sub.d, sub.bounds)], sub.cols, (0.5,), sub.grid, sub.scale)
        assert whole["density"][p].tobytes() == other["density"][0].tobytes() and (whole["mode_x"][p], whole["mode_y"][p]) == (other["mode_x"][0], other["mode_y"][0])
        halone = ct.measure_bounded(sub.a, sub.x[:, :sub.d], sub.cols, sub.bounds, sub.probs, sub.grid, sub.scale)
        assert cb.pair_values(host, p).tobytes() == cb.pair_values(halone, 0).tobytes(), (s, t)


def test_a_transposed_pair_of_first_moments_is_noticed():
    """x-bounded and y-bounded orientations: the same two columns in either order give the transposed density"""
    c = cb.cases()["n17_nc3_G64_integer"]
    assert c.open_t(0) and not c.open_t(1)
    got = ct.measure_bounded(c.a, c.x[:, :c.d], c.cols, c.bounds, c.probs, c.grid, c.scale)
    x2 = c.x.copy()
    x2[:, [0, 1]] = c.x[:, [1, 0]]
    lo, hi = c.lo.copy(), c.hi.copy()
    lo[[0, 1]], hi[[0, 1]] = c.lo[[1, 0]], c.hi[[1, 0]]
    swapped = ct.measure_bounded(c.a, x2[:, :c.d], c.cols, (lo, hi), c.probs, c.grid, c.scale)
    b = cb.dense_cached(c, 0, 1, got, np.float64)[1]
    assert np.all(np.abs(swapped["density"][0].T - got["density"][0]) <= 2 * b)
    assert not np.allclose(got["density"][0], ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid, c.scale)["density"][0], rtol=1e-3)


def test_a_value_outside_its_bounds_fails_its_pairs_alone(checker, tmp_path, caplog):
    c = cb.cases()["n513_nc6_G64_fractional"]
    lo = c.lo.copy()
    used = c.x[c.use, c.cols[2]]
    lo[2] = float(np.sort(used)[3]) + 1.0 / 1024.0                # a few used values lie below the bound of chosen column 2
    bad = cb.Case("outside", c.a, c.x, c.d, c.cols, lo, c.hi, c.kinds, grid=c.grid)
    native = cb.native_case(checker, tmp_path, bad)
    host = ct.measure_bounded(bad.a, bad.x[:, :bad.d], bad.cols, bad.bounds, bad.probs, bad.grid, bad.scale, at=native)
    rest = cb.sub_case(c, (0, 1, 3, 4, 5))
    without = cb.native_case(checker, tmp_path, rest)
    for got in (native, host):
        assert list(got["col_status"]) == [0.0, 0.0, 8.0, 0.0, 0.0, 0.0]
        assert got["bound_lo"][2] == lo[2] and np.isnan(got["at_lo"][2]) and np.isnan(got["h"][2])
        for p, (s, t) in enumerate(ct.pairs(6)):
            if 2 in (s, t):
                cb.assert_failed_pair(got, p, 8.0, "outside")
    kept = [(s, t) for s, t in ct.pairs(6) if 2 not in (s, t)]
    for q, (s, t) in enumerate(kept):
        assert cb.pair_values(native, ct.pairs(6).index((s, t))).tobytes() == cb.pair_values(without, q).tobytes(), (s, t)
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        ct.build(host, (bad.probs, bad.grid, bad.scale, bad.cols))
    assert len([r for r in caplog.records if "contours" in r.getMessage() and r.levelno == logging.WARNING]) == 1


def test_status_7_comes_before_8(checker, tmp_path):
    c = cc.constant_column_case()                          # chosen column 1 is constant at 2.5
    lo, hi = np.array([-INF, 3.0, 2.0]), np.array([INF, 4.0, INF])   # ... and lies outside its bounds; column 2 has values below 2
    assert (c.x[c.use, 2] < 2.0).any()
    bad = cb.Case("seven_first", c.a, c.x, c.d, c.cols, lo, hi, ("open", "both", "gamma_at_0"), grid=c.grid)
    native = cb.native_case(checker, tmp_path, bad)
    host = ct.measure_bounded(bad.a, bad.x[:, :bad.d], bad.cols, bad.bounds, bad.probs, bad.grid, bad.scale)
    for got in (native, host):
        assert list(got["col_status"]) == [0.0, 7.0, 8.0]
        assert list(got["pair_status"]) == [7.0, 8.0, 7.0]  # (a pair takes its failing column's status, the x axis' first)
        for p, st in enumerate((7.0, 8.0, 7.0)):
            cb.assert_failed_pair(got, p, st, "seven_first")


def test_refused_systems_are_unchanged(checker, tmp_path):
    for name, a, x, status, column in cc.status_cases():
        bounds = (np.array([-INF, 0.0]), np.array([INF, INF]))
        native, = cb.run_native(checker, tmp_path, [(a, x, 2, bounds)], (0, 1), cc.PROBS, 32, 1.0)
        host = ct.measure_bounded(a, x, (0, 1), bounds, cc.PROBS, 32)
        for got in (native, host):
            cc.assert_failed_system({k: got[k] for k in got if k not in ct.BOUND_KEYS}, status, column, int(np.count_nonzero(a != 0)), name)
            for k in ct.BOUND_KEYS:
                assert np.isnan(got[k]).all(), (name, k)
        assert cc.equal_blocks(native, host), name


def test_keyword_and_bounds_spec(tmp_path):
    assert ct.spec({"probs": 0.9, "bounds": True}, ndim=2) == ((0.9,), 64, 1.0, (0, 1))
    assert ct.bounds_spec(True, ndim=2) is None and ct.bounds_spec(None) is None and ct.bounds_spec({"probs": 0.9}, ndim=2) is None
    assert not ct.bounds_wanted({"bounds": None}) and not ct.bounds_wanted((0.5,)) and ct.bounds_wanted({"bounds": "ranges"})
    names = ["a", "b", "c"]
    lo, hi = ct.bounds_spec({"bounds": {"c": (0, None), "a": (-1, 1)}, "params": ["c", "a"]}, names=names, ndim=3)
    assert list(lo) == [-1.0, 0.0] and list(hi) == [1.0, INF]
    lo, hi = ct.bounds_spec({"bounds": [(0, 1), None, (None, 5)]}, names=names, ndim=3)
    assert list(lo) == [0.0, -INF, -INF] and list(hi) == [1.0, INF, 5.0]
    lo, hi = ct.bounds_spec({"bounds": True, "params": [1, 2]}, names=names, ndim=3, bounds={"b": (0, 2)})
    assert list(lo) == [0.0, -INF] and list(hi) == [2.0, INF]
    with pytest.raises(ValueError, match="^contours="):
        ct.bounds_spec({"bounds": True}, names=names, ndim=3)
    with pytest.raises(ValueError, match="^contours="):
        ct.bounds_spec({"bounds": {"zz": (0, 1)}}, names=names, ndim=3)
    with pytest.raises(ValueError, match="^contours="):
        ct.bounds_spec({"bounds": [(1, 0), None, None]}, names=names, ndim=3)
    with pytest.raises(ValueError, match="^contours="):
        ct.bounds_spec({"bounds": "ranges"}, names=names, ndim=3, root=None)
    root = tmp_path / "chain"
    (tmp_path / "chain.ranges").write_text("a 0 N\nb N N\nc -2 2\n")
    (tmp_path / "chain.paramnames").write_text("a\nb\nc\n")
    lo, hi = ct.bounds_spec({"bounds": "ranges", "params": ["a", "c"]}, names=names, ndim=3, root=str(root))
    assert list(lo) == [0.0, -2.0] and list(hi) == [INF, 2.0]
    with pytest.raises(ValueError):
        ct.measure_bounded(np.ones(4), np.zeros((4, 2)), (0, 1), ([0.0, 1.0], [0.0, 2.0]), (0.5,), 32)


def test_symbols_and_sizes():
    from mcevidence_amd import _capi as capi
    lib = capi.load()
    for sym in ("mce_param_contours_bounded_out_doubles", "mce_param_contours_bounded_workspace_bytes", "mce_param_contours_bounded_dev", "mce_param_contours_bounded_f64"):
        assert hasattr(lib, sym) and sym in capi.SIGNATURES
    assert lib.mce_abi_version() == 3
    from mcevidence_amd import _capi
    assert _capi.param_contours_bounded_out_doubles(27, 2, 64) == 8 + 13 * 27 + 351 * (4 + 7 * 2 + 64 * 64) == _capi.contours_bounded_block_doubles(27, 2, 64)
    assert _capi.param_contours_bounded_out_doubles(1, 2, 64) == 0 and _capi.param_contours_bounded_out_doubles(3, 2, 128) == 0
    plain, bounded = (f(10 ** 6, 1, 27, 27, 2, 64) for f in (_capi.param_contours_workspace_bytes, _capi.param_contours_bounded_workspace_bytes))
    sums = 16 * 351 * 4096 * 8
    assert bounded - plain >= 2 * sums and bounded - plain < 2 * sums + (1 << 20)      # the per-part sums triple; the tables are small


def test_invalid_arguments_need_no_device():
    """MCE_ERR_INVALID before any device call: on a machine without a device the same calls answer the same"""
    from mcevidence_amd import _capi
    c = cb.cases()["n5_nc3_G64_fractional"]
    seg = [(c.x, c.d, c.a)]
    ok = [c.bounds]
    for cols, bounds, probs, grid, scale in (((0, 1, 2), [([0.0, 1.0, 1.0], [1.0, 1.0, 2.0])], cb.PROBS, 64, 1.0),      # lo == hi
                                             ((0, 1, 2), [([0.0, 3.0, 1.0], [1.0, 2.0, 2.0])], cb.PROBS, 64, 1.0),      # lo > hi
                                             ((0, 1, 2), [([0.0, np.nan, 1.0], [1.0, 2.0, 2.0])], cb.PROBS, 64, 1.0),   # NaN
                                             ((0, 1, 2), [([0.0, INF, 1.0], [1.0, INF, 2.0])], cb.PROBS, 64, 1.0),      # lo = +inf
                                             ((0, 1, 2), ok, cb.PROBS, 128, 1.0), ((0, 1, 2), ok, (1.5,), 64, 1.0), ((0, 1, 2), ok, cb.PROBS, 64, 0.0),
                                             ((0, 1, 3), ok, cb.PROBS, 64, 1.0), ((2, 1, 0), ok, cb.PROBS, 64, 1.0)):
        with pytest.raises(ValueError):                    # (MCE_ERR_INVALID; no visible device would be a RuntimeError)
            _capi.param_contours_bounded(seg, cols, bounds, probs, grid, scale)
        with pytest.raises(ValueError):
            _capi.param_contours_bounded_dev([(8, c.x.shape[1], len(c.a), c.d, 8)], cols, bounds, probs, grid, scale, 8, 1 << 30)
    with pytest.raises(ValueError):
        _capi.param_contours_bounded(seg, (0, 1, 2), [([0.0, 1.0], [1.0, 2.0])], cb.PROBS, 64, 1.0)
    lib = _capi.load()
    out = np.zeros(8)
    cols = np.array([0, 1], dtype=np.int32)
    probs = np.array([0.5])
    x, w = np.zeros((4, 2)), np.ones(4)
    arr = _capi._seg_array(_capi.SummarySeg, [(x.ctypes.data, 2, 4, 2, w.ctypes.data)])
    import ctypes
    for fn, tail in ((lib.mce_param_contours_bounded_f64, (0,)), (lib.mce_param_contours_bounded_dev, (None, 0, None))):
        assert fn(ctypes.cast(arr, ctypes.c_void_p), 1, cols.ctypes.data, 2, None, probs.ctypes.data, 1, 64, 1.0, out.ctypes.data, *tail) == _capi.MCE_ERR_INVALID
        assert "null pointer" in _capi.last_error()


def test_build_lines_and_save(tmp_path):
    c = cb.cases()["n17_nc3_G64_integer"]
    sp = (c.probs, c.grid, 1.0, c.cols)
    plain = ct.build(ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid), sp, ["a", "b", "c"])
    m = ct.build(ct.measure_bounded(c.a, c.x[:, :c.d], c.cols, c.bounds, c.probs, c.grid), sp, ["a", "b", "c"])
    assert set(m) - set(plain) == set(ct.BOUND_KEYS) and not set(plain) - set(m)
    assert len(ct.lines(m)) == 4 and ct.lines(m)[0] == ct.lines(plain)[0]
    ct.save(tmp_path / "c.npz", ["root", "other"], [{"contours": m}, {"contours": plain}])
    z = np.load(tmp_path / "c.npz")
    assert np.array_equal(z["bound_lo_0"], c.lo) and np.array_equal(z["at_lo_0"], m["at_lo"]) and z["at_hi_0"].shape == (3,) and "bound_hi_0" in z
    assert "density_1" in z and "bound_lo_1" not in z


@pytest.mark.parametrize("seed", range(5))
def test_the_exponential_corner(seed):
    c = cb.exponential_case(seed)
    got = ct.measure_bounded(c.a, c.x[:, :c.d], c.cols, c.bounds, c.probs, c.grid, c.scale)
    cb.assert_exponential_corner(c, got, "numpy")
    # the rule without bounds on the same draws fails the exact assertions and the area
    plain = ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid, c.scale)
    assert plain["mode_x"][0] > 0.0 and plain["mode_y"][0] > 0.0 and np.all(plain["lower_x"][:, 0] < 0.0)
    area = cb.region_area(plain, 0, 0.68, ends=(False,) * 4)
    print("numpy %s without bounds: mode (%.3f, %.3f)  68 %% area %.4f" % (c.name, plain["mode_x"][0], plain["mode_y"][0], area))
    assert abs(area - cb.EXP_T ** 2 / 2) > 0.3


def test_mcevidence_with_contour_bounds_and_the_untouched_default(tmp_path, caplog):
    from helpers import OracleBackend
    from mcevidence_amd import MCEvidence
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    root = str(tmp_path / "run")
    chains = []
    for i in range(2):
        ch = gaussian_chain(seed=50 + i, n=400, d=3, weights="int")
        ch[:, 2] = np.round(np.abs(ch[:, 2]) * 64) / 64                # the first parameter: cut at 0
        chains.append(ch)
    write_cosmomc_chains(root, chains, [("p0", 0.0, None), ("p1", -8.0, 8.0), ("p2", -INF, None)], fmt="%.17g")
    kw = dict(kmax=2, verbose=1, backend=OracleBackend())
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        lnE0, info0 = MCEvidence(root, contours={"grid": 32}, marginals={"grid": 64}, bounds="ranges", **kw).evidence(info=True)
        assert sum("not boundary-corrected" in r.getMessage() for r in caplog.records) == 1      # without the key: today's line, today's dict
        caplog.clear()
        m = MCEvidence(root, contours={"grid": 32, "bounds": "ranges"}, marginals={"grid": 64}, bounds="ranges", **kw)
        lnE, info = m.evidence(info=True)
        assert sum("not boundary-corrected" in r.getMessage() for r in caplog.records) == 0
    assert np.array_equal(lnE, lnE0)                                   # ln E is untouched
    cbd, c0 = info["contours"], info0["contours"]
    assert set(cbd) == set(c0) | set(ct.BOUND_KEYS) and not set(ct.BOUND_KEYS) & set(c0)
    assert list(cbd["bound_lo"]) == [0.0, -8.0, -INF] and list(cbd["at_lo"]) == [1.0, 0.0, 0.0] and list(cbd["at_hi"]) == [0.0] * 3
    assert cbd["grid_lo"][0] == 0.0 and np.all(cbd["lower_x"][:, 0] == 0.0) and c0["grid_lo"][0] < 0.0
    # the pair of the two columns whose grids are not cut: the bound (-8, 8) is far from the samples, its constants are 1, 0, 1, 1 there
    part = m.gd.data["s1"]
    direct = ct.measure_bounded(part.adjusted_weights, np.asarray(part.samples)[:, :3], (0, 1, 2), (np.array([0.0, -8.0, -INF]), np.array([INF, 8.0, INF])), (0.68, 0.95), 32)
    assert np.array_equal(cbd["density"], direct["density"]) and np.array_equal(cbd["level"], direct["level"])
    for form in ({"p0": (0, None), "p1": (-8, 8)}, [(0, None), (-8, 8), (None, None)]):
        other = MCEvidence(root, contours={"grid": 32, "bounds": form}, **kw).evidence(info=True)[1]["contours"]
        assert all(np.array_equal(np.asarray(other[k]), np.asarray(cbd[k]), equal_nan=True) for k in cbd if k not in ("names", "pairs"))
    # "bounds": True takes the call's bounds=, with or without marginals=
    other = MCEvidence(root, contours={"grid": 32, "bounds": True}, bounds="ranges", **kw).evidence(info=True)[1]["contours"]
    assert np.array_equal(other["density"], cbd["density"])
    with pytest.raises(ValueError, match="^contours="):
        MCEvidence(root, contours={"grid": 32, "bounds": True}, **kw).evidence()
    with pytest.raises(ValueError, match="^bounds=.*without marginals"):
        MCEvidence(root, contours={"grid": 32}, bounds="ranges", **kw)
    with pytest.raises(ValueError, match="^contours=.*not among"):
        MCEvidence(root, contours={"grid": 32, "bounds": {"zz": (0, 1)}}, **kw).evidence()
