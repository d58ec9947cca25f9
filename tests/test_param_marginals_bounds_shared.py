"""marginals with bounds on the CPU: the rule the host check and the device kernels share (mcevidence_amd/csrc/param_marginals_bounds.hpp:
its serial drivers, built with -fsanitize=address,undefined as a stand-alone program) and its NumPy form ``marginals.measure_bounded``
against the oracle of tests/marginals_bounds_cases.py, within the bounds derived in docs/design/marginals_bounds.md; a column without
bounds is today's column bit for bit; every decision redone bit for bit on the block's own densities, end weights included, and equal
to the oracle's on every decided grid point; a sample outside its bounds fails its column alone; the keyword's values, ``prior.bounds``,
the refusals and the untouched default; the command line's --bounds; the statistical checks on an exponential and a half-normal
posterior cut at 0, which today's ``measure`` fails."""
import logging
import math
import subprocess

import numpy as np
import pytest

import marginals_bounds_cases as bc
import marginals_cases as mc
from helpers import OracleBackend
from mcevidence_amd import marginals as mg
from mcevidence_amd import prior
from mcevidence_amd.evidence import MCEvidence
from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains

INF = float("inf")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return bc.build_checker(tmp_path_factory.mktemp("param_marginals_bounds"))


@pytest.fixture(scope="module")
def plain_checker(tmp_path_factory):
    return mc.build_checker(tmp_path_factory.mktemp("param_marginals_plain"))


def test_open_bounds_give_unit_constants_and_the_layout(checker):
    out = subprocess.run([checker, "consts"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().startswith("ok records="), out.stdout + out.stderr
    a0, a1, a2, den = mg.boundary_constants(np.array([-3.5, 0.0, 7.0]), -INF, INF, 0.125)
    assert np.all(a0 == 1.0) and np.all(a1 == 0.0) and np.all(a2 == 1.0) and np.all(den == 1.0)
    assert mg.PER_COL_BOUNDED == mg.PER_COL + 4 and mg.COLUMN_OUTSIDE == 8


@pytest.mark.parametrize("name", list(bc.cases()))
def test_serial_driver_and_numpy_form_against_the_oracle(name, checker, tmp_path):
    c = bc.cases()[name]
    nat, = bc.run_native(checker, tmp_path, [(c.a, c.x, c.d, c.bounds)], c.probs, c.grid, c.scale)
    host = mg.measure_bounded(c.a, c.x[:, :c.d], c.bounds, c.probs, c.grid, c.scale)
    stats = {}
    for what, got in (("native", nat), ("numpy ", host)):
        good = moments(c, got, what)
        assert list(good) == list(range(c.d)), (name, got["col_status"])
        for j in bc.oracle_columns(c):
            bc.check_column(c, got, j, what, stats=stats)
        for j in range(c.d):
            bc.check_grid(c, got, j)
    assert bc.check_decisions_native(checker, tmp_path, [nat, host], c.probs, c.grid) == 2 * c.d
    bc.check_against_numpy(c, nat, "native")
    assert stats["undecided"] <= bc.MAX_UNDECIDED
    print("largest error/bound of a density: %.3g" % stats["density"])


def moments(c, got, what):
    """marginals_cases.check_moments without its statement about lo and step (the grid of a bounded column is check_grid's)"""
    ex = c.exact
    clipped = dict(got)
    clipped["lo"] = np.array([ex["min"][j] - 3.0 * got["h"][j] for j in range(c.d)])
    clipped["step"] = np.array([((ex["max"][j] + 3.0 * got["h"][j]) - clipped["lo"][j]) / float(c.grid - 1) for j in range(c.d)])
    return mc.check_moments(c, clipped, what)


@pytest.mark.parametrize("name", list(bc.cases()))
def test_a_column_without_bounds_is_todays_column(name, checker, plain_checker, tmp_path):
    c = bc.cases()[name]
    o = bc.open_case(c)
    # every column open: the whole common layout, by the serial drivers and by the NumPy forms
    nat_b, = bc.run_native(checker, tmp_path, [(o.a, o.x, o.d, o.bounds)], o.probs, o.grid, o.scale)
    nat_p, = mc.run_native(plain_checker, tmp_path, [(o.a, o.x, o.d)], o.probs, o.grid, o.scale)
    assert bc.equal_common(nat_b, nat_p), name
    assert np.all(nat_b["at_lo"] == 0.0) and np.all(nat_b["at_hi"] == 0.0) and np.all(nat_b["bound_lo"] == -INF) and np.all(nat_b["bound_hi"] == INF)
    host_p = mg.measure(o.a, o.x[:, :o.d], o.probs, o.grid, o.scale)
    assert bc.equal_common(mg.measure_bounded(o.a, o.x[:, :o.d], o.bounds, o.probs, o.grid, o.scale), host_p), name
    # an open column next to bounded ones
    open_cols = [j for j in range(c.d) if c.lo[j] == -INF and c.hi[j] == INF]
    if open_cols:
        nat, = bc.run_native(checker, tmp_path, [(c.a, c.x, c.d, c.bounds)], c.probs, c.grid, c.scale)
        assert bc.equal_common(nat, nat_p, cols=open_cols), name
        assert bc.equal_common(mg.measure_bounded(c.a, c.x[:, :c.d], c.bounds, c.probs, c.grid, c.scale), host_p, cols=open_cols), name


def test_a_sample_outside_its_bounds_fails_its_column_alone(checker, tmp_path, caplog):
    c = bc.cases()["n511_d8_G1024_unit"]
    lo, hi = c.lo.copy(), c.hi.copy()
    used = c.x[c.use, 3]
    lo[3] = float(np.sort(used)[1])                           # the smallest sample of column 3 lies below its bound
    nat, = bc.run_native(checker, tmp_path, [(c.a, c.x, c.d, (lo, hi))], c.probs, c.grid, c.scale)
    host = mg.measure_bounded(c.a, c.x[:, :c.d], (lo, hi), c.probs, c.grid, c.scale)
    ref = mg.measure_bounded(c.a, c.x[:, :c.d], c.bounds, c.probs, c.grid, c.scale)
    others = [j for j in range(c.d) if j != 3]
    for got in (nat, host):
        assert got["status"] == 0 and list(got["col_status"]) == [0, 0, 0, 8, 0, 0, 0, 0]
        bc.assert_outside_column(got, 3)
        assert (got["bound_lo"][3], got["bound_hi"][3]) == (lo[3], hi[3])
    assert bc.equal_common(host, ref, cols=others)
    ref_nat, = bc.run_native(checker, tmp_path, [(c.a, c.x, c.d, c.bounds)], c.probs, c.grid, c.scale)
    assert bc.equal_common(nat, ref_nat, cols=others)
    # above the upper bound too; the constant column keeps its 7
    x = c.x.copy()
    x[c.use, 2] = 2.5
    hi2 = c.hi.copy()
    hi2[4] = float(np.sort(c.x[c.use, 4])[-2])
    both = mg.measure_bounded(c.a, x[:, :c.d], (c.lo, hi2), c.probs, c.grid, c.scale)
    assert list(both["col_status"]) == [0, 0, 7, 0, 8, 0, 0, 0]
    # ONE warning, nothing raised
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        m = mg.build(both, (c.probs, c.grid, c.scale))
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1 and "7, 8" in caplog.records[-1].getMessage()
    assert set(mg.BOUND_KEYS) <= set(m)
    # today's system statuses, with bounds
    for sname, a, xs, status, column in mc.status_cases():
        got = mg.measure_bounded(a, xs, (np.full(2, -INF), np.full(2, INF)), c.probs, 64)
        mc.assert_failed_system(got, 2, status, column, int(np.count_nonzero(a != 0)), sname)
        assert all(np.isnan(got[k]).all() for k in mg.BOUND_KEYS), sname
    nat = bc.run_native(checker, tmp_path, [(a, xs, 2, (np.array([-1.0, -INF]), np.array([INF, 5.0]))) for _, a, xs, _, _ in mc.status_cases()], c.probs, 64, 1.0)
    for (sname, a, xs, status, column), got in zip(mc.status_cases(), nat):
        mc.assert_failed_system(got, 2, status, column, int(np.count_nonzero(a != 0)), sname)
        assert all(np.isnan(got[k]).all() for k in mg.BOUND_KEYS), sname


def test_keyword_values_and_refusals(tmp_path):
    names = ["mnu", "r", "tau"]
    assert mg.bounds_spec(None, names=names) is None
    lo, hi = mg.bounds_spec({"mnu": (0, None), "tau": (0.01, 0.8)}, names=names)
    assert list(lo) == [0.0, -INF, 0.01] and list(hi) == [INF, INF, 0.8]
    lo, hi = mg.bounds_spec([(0, "N"), (None, None), (-INF, INF)], ndim=3)
    assert list(lo) == [0.0, -INF, -INF] and list(hi) == [INF, INF, INF]
    lo, hi = mg.bounds_spec([("N", 1.5), (0.0, INF), None], names=names)
    assert list(lo) == [-INF, 0.0, -INF] and list(hi) == [1.5, INF, INF]
    for bad in ({"mnu": (1.0, 1.0)}, {"mnu": (2.0, 1.0)}, {"mnu": (float("nan"), 1.0)}, {"omega": (0.0, 1.0)}, [(0, 1)], "file", [(0, 1, 2)] * 3, {"r": "x"}, 5):
        with pytest.raises(ValueError, match="^bounds="):
            mg.bounds_spec(bad, names=names)
    with pytest.raises(ValueError, match="^bounds='ranges' needs a root name"):
        mg.bounds_spec("ranges", names=names)
    with pytest.raises(ValueError, match="^bounds=.*without marginals"):
        mg.bounds_spec({"r": (0, 1)}, names=names, marginals=None)
    # prior.bounds: every listed name, an open side is an infinity, a fixed parameter is listed
    root = str(tmp_path / "run")
    chains = [gaussian_chain(seed=30 + i, n=300, d=3, weights="int") for i in range(2)]
    write_cosmomc_chains(root, chains, [("mnu", 0.0, None), ("fixed", 1.0, 1.0), ("r", -INF, 6.0), ("tau", -6.0, 6.0)], fmt="%.17g")
    assert prior.bounds(root) == {"mnu": (0.0, INF), "fixed": (1.0, 1.0), "r": (-INF, 6.0), "tau": (-6.0, 6.0)}
    assert "fixed" not in prior.params_info(root)["name"]
    with pytest.raises(ValueError, match="^bounds='ranges'"):
        prior.bounds(str(tmp_path / "nothing"))
    # without .paramnames the columns are the listed parameters that are not fixed, in the file's order; with it, by name
    lo, hi = mg.bounds_spec("ranges", names=["p0", "p1", "p2"], root=root)
    assert list(lo) == [0.0, -INF, -6.0] and list(hi) == [INF, 6.0, 6.0]
    with open(root + ".paramnames", "w") as fh:
        fh.write("tau\tTAU\nother\tO\nmnu\tM\n")
    lo, hi = mg.bounds_spec("ranges", names=["tau", "other", "mnu"], root=root)
    assert list(lo) == [-6.0, -INF, 0.0] and list(hi) == [6.0, INF, INF]
    # MontePython's log.param
    mp = tmp_path / "mp"
    mp.mkdir()
    (mp / "log.param").write_text("data.parameters['omega_b'] = [2.2, None, None, 0.01, 0.01, 'cosmo']\n"
                                  "data.parameters['M_tot'] = [0.1, 0, 5, 0.1, 1, 'cosmo']\ndata.parameters['A_x'] = [1, 0.5, None, 0.1, 1, 'nuisance']\n"
                                  "data.parameters['sigma8'] = [0, None, None, 0, 1, 'derived']\n")
    assert prior.bounds(str(mp)) == {"omega_b": (-INF, INF), "M_tot": (0.0, 5.0), "A_x": (0.5, INF), "sigma8": (-INF, INF)}
    # the routes refuse before any work
    from mcevidence_amd import farm, resident
    x = gaussian_chain(seed=1, n=200, d=2)
    with pytest.raises(ValueError, match="^bounds=.*without marginals"):
        MCEvidence([x], ndim=2, bounds=[(0, 1), (0, 1)], verbose=0)
    with pytest.raises(ValueError, match="^bounds='ranges' needs a root name"):
        MCEvidence([x], ndim=2, marginals=True, bounds="ranges", verbose=0)
    with pytest.raises(ValueError, match="^bounds=.*without marginals"):
        resident.plan(bounds={"a": (0, 1)})
    assert resident.plan(marginals=True, bounds="ranges", ndim=2, nparam=2, nrows=100) == resident.plan(marginals=True, ndim=2, nparam=2, nrows=100)
    assert farm._per_root_bounds("ranges", 3) == ["ranges"] * 3 and farm._per_root_bounds([(0, 1), (None, 2)], 2) == [[(0, 1), (None, 2)]] * 2
    assert farm._per_root_bounds(["ranges", None, {"a": (0, 1)}], 3) == ["ranges", None, {"a": (0, 1)}]
    assert farm._per_root_bounds([[(0, 1)], None], 2) == [[(0, 1)], None]
    with pytest.raises(ValueError, match="^bounds="):
        farm._per_root_bounds(["ranges", 3.0], 2)


def test_mcevidence_with_bounds_and_the_untouched_default(tmp_path, caplog):
    root = str(tmp_path / "run")
    rng = np.random.default_rng(8)
    chains = []
    for i in range(2):
        ch = gaussian_chain(seed=50 + i, n=400, d=3, weights="int")
        ch[:, 2] = np.round(np.abs(ch[:, 2]) * 64) / 64                # the first parameter: cut at 0
        chains.append(ch)
    write_cosmomc_chains(root, chains, [("p0", 0.0, None), ("p1", -8.0, 8.0), ("p2", -INF, None)], fmt="%.17g")
    kw = dict(kmax=2, verbose=0, backend=OracleBackend())
    plain = MCEvidence(root, marginals={"grid": 64}, **kw)
    lnE0, info0 = plain.evidence(info=True)
    m = MCEvidence(root, marginals={"grid": 64}, bounds="ranges", **kw)
    lnE, info = m.evidence(info=True)
    assert np.array_equal(lnE, lnE0)                                   # ln E is untouched
    mb, m0 = info["marginals"], info0["marginals"]
    assert set(mb) == set(m0) | set(mg.BOUND_KEYS) and not set(mg.BOUND_KEYS) & set(m0)
    assert list(mb["bound_lo"]) == [0.0, -8.0, -INF] and list(mb["bound_hi"]) == [INF, 8.0, INF] and list(mb["at_lo"]) == [1.0, 0.0, 0.0] and list(mb["at_hi"]) == [0.0] * 3
    assert mb["grid_lo"][0] == 0.0 and mb["lower"][0][0] == 0.0 and m0["grid_lo"][0] < 0.0
    # the open column is today's; the mapping and the sequence give what the file gives
    for k in ("density", "mode", "lower", "upper", "pieces", "edge", "h", "grid_lo", "grid_step"):
        assert np.array_equal(np.asarray(mb[k])[..., 2, :] if k == "density" else np.asarray(mb[k])[..., 2], np.asarray(m0[k])[..., 2, :] if k == "density" else np.asarray(m0[k])[..., 2]), k
    part = m.gd.data["s1"]
    direct = mg.measure_bounded(part.adjusted_weights, np.asarray(part.samples)[:, :3], (np.array([0.0, -8.0, -INF]), np.array([INF, 8.0, INF])), (0.68, 0.95), 64)
    assert np.array_equal(mb["density"], direct["density"]) and np.array_equal(mb["upper"], direct["upper"])
    for form in ({"p0": (0, None), "p1": (-8, 8)}, [(0, None), (-8, 8), (None, None)]):
        other = MCEvidence(root, marginals={"grid": 64}, bounds=form, **kw).evidence(info=True)[1]["marginals"]
        assert all(np.array_equal(np.asarray(other[k]), np.asarray(mb[k]), equal_nan=True) for k in mb if k != "names")
    with pytest.raises(ValueError, match="^bounds=.*not among the parameters"):
        MCEvidence(root, marginals=True, bounds={"zz": (0, 1)}, **kw).evidence()
    # contours next to bounds: one INFO line
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        MCEvidence(root, marginals={"grid": 64}, contours={"grid": 32}, bounds="ranges", kmax=2, verbose=1, backend=OracleBackend()).evidence()
    assert sum("not boundary-corrected" in r.getMessage() for r in caplog.records) == 1
    # a sample outside: one WARNING, ln E untouched
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        lnE8, info8 = MCEvidence(root, marginals={"grid": 64}, bounds={"p1": (0, None)}, **kw).evidence(info=True)
    assert np.array_equal(lnE8, lnE0) and list(info8["marginals"]["col_status"]) == [0.0, 8.0, 0.0]
    assert len([r for r in caplog.records if r.levelno == logging.WARNING and "marginals" in r.getMessage()]) == 1


def test_command_line_bounds(tmp_path, capsys):
    from mcevidence_amd import cli
    args = cli.build_parser().parse_args(["root", "--marginals", "--bounds"])
    assert cli._marginals_kw(args) == {"marginals": True, "bounds": "ranges"}
    args = cli.build_parser().parse_args(["root", "--marginals", "0.9", "--marginals-grid", "64", "--bounds", "mnu=0:", "tau=0.01:0.8", "r=N:1"])
    assert cli._marginals_kw(args) == {"marginals": {"probs": (0.9,), "grid": 64}, "bounds": {"mnu": ("0", None), "tau": ("0.01", "0.8"), "r": (None, "1")}}
    lo, hi = mg.bounds_spec(cli._marginals_kw(args)["bounds"], names=["mnu", "r", "tau"])
    assert list(lo) == [0.0, -INF, 0.01] and list(hi) == [INF, 1.0, 0.8]
    assert cli._marginals_kw(cli.build_parser().parse_args(["root", "--marginals"])) == {"marginals": True}
    with pytest.raises(ValueError, match="^bounds="):
        cli._marginals_kw(cli.build_parser().parse_args(["root", "--marginals", "--bounds", "mnu"]))
    with pytest.raises(SystemExit):
        cli.main(["root", "--bounds"])
    assert "--bounds belongs to --marginals" in capsys.readouterr().err
    # --marginals-out gains the per-column arrays
    m = mg.build(mg.measure_bounded(np.ones(50), np.arange(50.0)[:, None] / 8, (np.array([0.0]), np.array([INF])), (0.68,), 64), ((0.68,), 64, 1.0))
    mg.save(str(tmp_path / "o.npz"), ["a", "b"], [{"marginals": m}, {"marginals": mg.build(mg.measure(np.ones(50), np.arange(50.0)[:, None], (0.68,), 64), ((0.68,), 64, 1.0))}])
    z = np.load(str(tmp_path / "o.npz"))
    assert list(z["bound_lo_0"]) == [0.0] and list(z["at_lo_0"]) == [1.0] and list(z["at_hi_0"]) == [0.0] and "bound_lo_1" not in z.files and "density_1" in z.files


def kish(a):
    return a.sum() ** 2 / (a * a).sum()


@pytest.mark.parametrize("seed", range(5))
def test_posteriors_cut_at_zero(seed):
    """Exponential(1) and a half-normal, n = 20 000, weights 1..4, L = 0, G = 512: the mode and the lower limit are the bound exactly, and
    the upper limits lie within the quantile's sampling error at five sigma plus one grid step of the true HPD limits.  Today's ``measure``
    on the same draws fails the mode and lower assertions (measured: mode 0.23 .. 0.25, lower68 -0.05 .. -0.07)."""
    rng = np.random.default_rng(seed)
    n = 20000
    a = rng.integers(1, 5, n).astype(np.float64)
    ess = kish(a)
    bounds = (np.array([0.0]), np.array([INF]))
    x = rng.exponential(1.0, n)
    got = mg.measure_bounded(a, x[:, None], bounds, (0.68, 0.95), 512)
    assert got["mode"][0] == 0.0 and got["at_lo"][0] == 1.0 and got["at_hi"][0] == 0.0 and got["lo"][0] == 0.0
    for t, p in enumerate((0.68, 0.95)):
        assert got["lower"][t][0] == 0.0 and got["edge"][t][0] == 1.0 and got["pieces"][t][0] == 1.0
        xp = -math.log(1.0 - p)
        tol = 5.0 * math.sqrt(p * (1.0 - p)) / (math.exp(-xp) * math.sqrt(ess)) + got["step"][0]
        print("exponential seed %d p %.2f upper %.4f true %.4f tol %.4f" % (seed, p, got["upper"][t][0], xp, tol))
        assert abs(got["upper"][t][0] - xp) <= tol, (seed, p, got["upper"][t][0], xp, tol)
    assert 0.8 < got["density"][0][0] < 1.2                           # (true 1; today's rule gives 0.001 at its first grid point)
    # today's rule on the same draws: the mode and the lower limit are not the bound
    old = mg.measure(a, x[:, None], (0.68, 0.95), 512)
    assert old["mode"][0] != 0.0 and old["lower"][0][0] != 0.0 and old["mode"][0] > 0.1 and old["lower"][0][0] < 0.0
    # the half-normal (its mode is not asserted: the density is flat at 0)
    x = np.abs(rng.standard_normal(n))
    got = mg.measure_bounded(a, x[:, None], bounds, (0.68, 0.95), 512)
    for t, (p, xp) in enumerate(((0.68, 0.9945), (0.95, 1.960))):
        assert got["lower"][t][0] == 0.0 and got["edge"][t][0] == 1.0
        f = 2.0 * math.exp(-xp * xp / 2.0) / math.sqrt(2.0 * math.pi)
        tol = 5.0 * math.sqrt(p * (1.0 - p)) / (f * math.sqrt(ess)) + got["step"][0]
        print("half-normal seed %d p %.2f upper %.4f true %.4f tol %.4f" % (seed, p, got["upper"][t][0], xp, tol))
        assert abs(got["upper"][t][0] - xp) <= tol, (seed, p, got["upper"][t][0], xp, tol)


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    for sym in ("mce_param_marginals_bounded_out_doubles", "mce_param_marginals_bounded_workspace_bytes", "mce_param_marginals_bounded_dev",
                "mce_param_marginals_bounded_f64"):
        assert sym in _capi.SIGNATURES and hasattr(_capi.load(), sym), sym
    assert _capi.load().mce_abi_version() == 3
    assert _capi.param_marginals_bounded_out_doubles(3, 2, 64) == 8 + 3 * (14 + 8 + 64) == _capi.marginals_bounded_block_doubles(3, 2, 64)
    assert _capi.param_marginals_bounded_out_doubles(3, 2, 100) == 0 and _capi.param_marginals_bounded_workspace_bytes(1000, 2, 3, 2, 64) > \
        _capi.param_marginals_workspace_bytes(1000, 2, 3, 2, 64)
    x, w = np.arange(12.0).reshape(6, 2), np.ones(6)
    # argument errors come before any device call: they need no GPU
    for lo, hi in (([0.0, 1.0], [0.0, 2.0]), ([float("nan"), 0.0], [1.0, 1.0]), ([0.0, 3.0], [1.0, 2.0]), ([INF, 0.0], [INF, 1.0])):
        with pytest.raises(ValueError, match="bounds"):
            _capi.param_marginals_bounded([(x, 2, w)], [(lo, hi)], (0.68,), 64, 1.0)
    with pytest.raises(ValueError, match="probability 0"):
        _capi.param_marginals_bounded([(x, 2, w)], [([-INF, 0.0], [INF, 1.0])], (1.5,), 64, 1.0)
    with pytest.raises(ValueError, match="null pointer"):
        _capi.check(_capi.load().mce_param_marginals_bounded_f64(None, 1, None, None, 1, 64, 1.0, None, 0))
    with pytest.raises(ValueError):
        _capi.param_marginals_bounded([(x, 2, w)], [([0.0], [1.0])], (0.68,), 64, 1.0)


def test_under_a_process_group_every_rank_computes_its_own(monkeypatch):
    import torch.distributed as dist
    from mcevidence_amd import parallel, resident
    ch = gaussian_chain(seed=12, n=700, d=3, weights="int")
    ch[:, 2] = np.abs(ch[:, 2])
    kw = dict(kmax=3, verbose=0, backend=OracleBackend(), marginals=True, bounds=[(0, None), (None, None), (None, 9.0)])
    want = MCEvidence([ch], **kw).evidence(info=True)[1]["marginals"]
    m = MCEvidence([ch], **kw)

    def refuse(*a, **k):
        raise AssertionError("a collective was called")
    monkeypatch.setattr(parallel, "is_distributed", lambda *a, **k: True)
    for name in ("all_reduce", "all_gather", "all_gather_object", "broadcast", "broadcast_object_list", "barrier", "reduce", "gather", "all_to_all_single"):
        monkeypatch.setattr(dist, name, refuse)
    m._fill_marginals()
    got = m.info["marginals"]
    assert set(got) == set(want) and all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in set(got) - {"names", "probs"})
    assert list(got["at_lo"]) == [1.0, 0.0, 0.0] and got["mode"][0] >= 0.0
    assert resident.plan(distributed=True, marginals=True, bounds="ranges") == resident.REASONS["distributed"]
