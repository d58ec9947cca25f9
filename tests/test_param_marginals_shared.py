"""marginals on the CPU: the rule the host check and the device kernels share (mcevidence_amd/csrc/param_marginals.hpp: its serial
drivers, built with -fsanitize=address,undefined as a stand-alone program) and its NumPy form ``marginals.measure`` against the oracle of
tests/marginals_cases.py, within the bounds derived in docs/design/marginals.md, every decision redone bit for bit on the block's own
densities and equal to the oracle's on every decided grid point; ``MCEvidence(..., marginals=...)`` for the auto and the cross form; the
keyword's values and the refusals; ``resident.plan``; the status and column-status cases; the untouched default; the command line; the
statistical checks on Gaussian samples and on a bimodal mixture; the new C symbols."""
import logging
import math
import subprocess

import numpy as np
import pytest

import marginals_cases as mc
from helpers import OracleBackend, OracleFeedBackend
from mcevidence_amd import marginals as mg
from mcevidence_amd import summary as sm
from mcevidence_amd.evidence import MCEvidence, evidence_many
from mcevidence_amd.synth import gaussian_chain


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return mc.build_checker(tmp_path_factory.mktemp("param_marginals"))


def test_parts_grids_and_the_shared_underflow_constant(checker):
    out = subprocess.run([checker, "parts"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().startswith("ok records="), out.stdout + out.stderr
    assert mg.UNDERFLOW == 746.0 and [mc.nparts(n) for n in (1, 512, 513, 32768, 32769, mc.BIG)] == [1, 1, 2, 64, 64, 64]


@pytest.mark.parametrize("name", list(mc.cases()))
def test_serial_driver_and_numpy_form_against_the_oracle(name, checker, tmp_path):
    c = mc.cases()[name]
    nat, = mc.run_native(checker, tmp_path, [(c.a, c.x, c.d)], c.probs, c.grid, c.scale)
    host = mg.measure(c.a, c.x[:, :c.d], c.probs, c.grid, c.scale)
    stats = {}
    for what, got in (("native", nat), ("numpy ", host)):
        good = mc.check_moments(c, got, what)
        for j in mc.oracle_columns(c):
            if j in good:
                mc.check_column(c, got, j, what, stats=stats)
        for j in sorted(set(range(c.d)) - set(good)):
            mc.assert_failed_column(got, j, (what, name))
    assert mc.check_decisions_native(checker, tmp_path, [nat, host], c.probs, c.grid) == 2 * len(good)
    mc.check_against_numpy(c, nat, "native")
    if c.d == 8 and c.n >= 400:
        assert sorted(set(range(c.d)) - set(good)) == [2, 3]          # +-1e300 (overflow) and the constant column: 7, the others untouched
        assert np.unique(c.x[c.use, 4]).size == 3
    if name == "n4100_d8_G512_fractional":
        # the lone far outlier: most of the grid is exact zeros by the 746 rule; ties resolve by the lowest k
        assert np.count_nonzero(host["density"][5] == 0.0) > c.grid // 2 and np.count_nonzero(nat["density"][5] == 0.0) > c.grid // 2
    assert stats["undecided"] <= mc.MAX_UNDECIDED


def test_ties_resolve_by_the_lowest_grid_point(checker, tmp_path):
    # a density array with exact ties, as the outlier column has them among its zeros: the order is rho descending, then k ascending
    rho = np.zeros(64)
    rho[[10, 11, 40, 41]] = [2.0, 1.0, 1.0, 2.0]
    blk = dict(status=0, mean=np.zeros(1), col_status=np.zeros(1), lo=np.array([-1.0]), step=np.array([0.125]), density=rho[None, :])
    probs = (0.3, 0.5, 0.7, 0.999)
    mode, md, lower, upper, pieces, edge = mg.decide(rho, -1.0, 0.125, probs)
    assert mode == -1.0 + 10 * 0.125 and md == 2.0                    # k = 10 before k = 41
    assert list(pieces) == [1.0, 2.0, 2.0, 2.0] and list(lower) == [0.25] * 4 and list(upper) == [0.25, 4.125, 4.125, 4.125] and list(edge) == [0.0] * 4
    blk.update(mode=np.array([mode]), mode_density=np.array([md]), lower=lower[:, None], upper=upper[:, None], pieces=pieces[:, None], edge=edge[:, None])
    assert mc.check_decisions_native(checker, tmp_path, [blk], probs, 64) == 1
    # equal densities everywhere
    flat = np.full(64, 0.1)
    _, masks = mg.hpd_selection(flat, (0.5,))
    assert masks[0].sum() == 32 and masks[0][:32].all()                # equal densities: the lowest k first


def test_status_cases_of_both_forms(checker, tmp_path, caplog):
    cases = mc.status_cases()
    native = mc.run_native(checker, tmp_path, [(a, x, x.shape[1]) for _, a, x, _, _ in cases], mc.PROBS, 64, 1.0)
    for (name, a, x, status, column), nat in zip(cases, native):
        for got in (nat, mg.measure(a, x, mc.PROBS, 64, 1.0)):
            mc.assert_failed_system(got, x.shape[1], status, column, int(np.count_nonzero(a != 0)), name)
    # the dict: every value NaN, the status kept, ONE WARNING in the route-independent words, nothing raised
    for status in (3, 5, 6):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            d = mg.build(mg._nan_block(3, 2, 64, 7, status, -1), mg.spec(True))
        warned = [r for r in caplog.records if r.levelno == logging.WARNING]
        assert len(warned) == 1 and "marginals: status %d" % status in warned[0].getMessage() and mg.STATUS_WORDS[status] in warned[0].getMessage()
        assert d["status"] == status and d["rows"] == 7 and d["names"] == ["p0", "p1", "p2"] and d["density"].shape == (3, 64)
        assert all(np.isnan(d[k]).all() for k in ("sum_w", "ess", "mean", "sd", "h", "c", "grid_lo", "grid_step", "density", "mode", "lower", "pieces"))
    assert mg.STATUS_WORDS[3] == sm.STATUS_WORDS[3] and mg.STATUS_WORDS[5] == sm.STATUS_WORDS[5]
    # failing columns: ONE WARNING that names them, the other columns whole
    c = mc.cases()["n511_d8_G1024_unit"]
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        d = mg.build(mg.measure(c.a, c.x[:, :c.d], c.probs, c.grid), c.spec)
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "column status 7" in warned[0] and "2, 3" in warned[0]
    assert list(d["col_status"]) == [0, 0, 7, 7, 0, 0, 0, 0] and d["status"] == 0 and np.isfinite(d["density"][[0, 1, 4, 5, 6, 7]]).all()


def test_keyword_values():
    assert mg.spec(None) is None and mg.spec(False) is None and mg.spec(True) == ((0.68, 0.95), 512, 1.0) and mg.spec(0.9) == ((0.9,), 512, 1.0)
    assert mg.spec([0.5, 0.99]) == ((0.5, 0.99), 512, 1.0) and mg.spec({"grid": 64}) == ((0.68, 0.95), 64, 1.0)
    assert mg.spec({"probs": (0.5,), "grid": 1024, "scale": 0.5}) == ((0.5,), 1024, 0.5) and mg.spec({}) == mg.spec(True) == mg.spec({"probs": True})
    for bad in (0.0, 1.0, -0.5, (0.5, 1.5), (), tuple([0.5] * 8), "0.68", float("nan"), {"grid": 100}, {"grid": 2048}, {"grid": 64.5}, {"grid": True},
                {"scale": 0.0}, {"scale": -1.0}, {"scale": float("inf")}, {"scale": float("nan")}, {"scale": "x"}, {"probs": "x"}, {"probs": (0.5, 2.0)},
                {"bandwidth": 1.0}, {"probs": False}):
        with pytest.raises(ValueError, match="marginals="):
            mg.spec(bad)
    assert len(mg.spec(tuple([0.5] * 7))[0]) == 7 and all(mg.spec({"grid": g})[1] == g for g in (64, 128, 256, 512, 1024))


KEYS = {"probs", "grid", "scale", "rows", "sum_w", "ess", "names", "mean", "sd", "h", "c", "grid_lo", "grid_step", "density", "mode", "mode_density", "lower", "upper",
        "pieces", "edge", "col_status", "status", "column"}


def _inputs(m):
    part = m.gd.data["s1"]
    return np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)[:, :m.ndim]


def _check_dict(d, a, x, what, spec=((0.68, 0.95), 512, 1.0)):
    assert set(d) == KEYS and (d["probs"], d["grid"], d["scale"]) == spec, (what, set(d) ^ KEYS)
    ref = mg.measure(a, x, *spec)
    for k, r in (("sum_w", "W"), ("grid_lo", "lo"), ("grid_step", "step")) + tuple((k, k) for k in ("rows", "mean", "sd", "h", "c", "density", "mode", "mode_density",
                                                                                                   "lower", "upper", "pieces", "edge", "col_status", "status", "column")):
        assert np.array_equal(np.asarray(d[k]), np.asarray(ref[r]), equal_nan=True), (what, k)
    assert d["density"].shape == (x.shape[1], spec[1]) and d["lower"].shape == d["pieces"].shape == (len(spec[0]), x.shape[1]) and len(d["names"]) == x.shape[1]
    assert d["ess"] == ref["W"] * ref["W"] / ref["A2"] and np.all(d["lower"] <= d["mode"]) and np.all(d["mode"] <= d["upper"])
    # a density: positive, and its Riemann sum over the grid is 1 up to the tails beyond 3 h and the quadrature
    assert np.all(d["density"] >= 0.0) and np.all(np.abs(d["density"].sum(axis=1) * d["grid_step"] - 1.0) < 5e-3), d["density"].sum(axis=1) * d["grid_step"]


def test_mcevidence_auto_and_cross_forms():
    ch = gaussian_chain(seed=3, n=1500, d=4, weights="int")
    for split, backend in ((False, OracleBackend), (True, OracleBackend), (False, OracleFeedBackend), (True, OracleFeedBackend)):
        np.random.seed(5)
        m = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend(), marginals=True)
        lnE, info = m.evidence(info=True)
        a, x = _inputs(m)
        assert len(a) == (750 if split else 1500) and m.param_marginals is info["marginals"] and m.marginals_spec is True
        _check_dict(info["marginals"], a, x, "split=%s %s" % (split, backend.__name__))
        np.random.seed(5)
        plain, pinfo = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend()).evidence(info=True)
        assert np.array_equal(lnE, plain) and "marginals" not in pinfo
    # ndim below the sampled parameters, a dict, together with summary; with the jackknife set there is no sigma
    m = MCEvidence([ch], kmax=3, verbose=0, ndim=2, backend=OracleBackend(), marginals={"probs": (0.5, 0.9, 0.99), "grid": 128, "scale": 0.5}, summary=True, jackknife=4)
    lnE, info = m.evidence(info=True)
    _check_dict(info["marginals"], *_inputs(m), "dict", spec=((0.5, 0.9, 0.99), 128, 0.5))
    assert "summary" in info and "jackknife" in info and not any("sigma" in k for k in info["marginals"])
    ms = [MCEvidence([gaussian_chain(seed=s, n=401, d=3, weights="int")], kmax=3, verbose=0, backend=OracleBackend(), marginals=(0.9,)) for s in (1, 2)]
    for m, (lnE, info) in zip(ms, evidence_many(ms, info=True)):
        _check_dict(info["marginals"], *_inputs(m), "evidence_many", spec=((0.9,), 512, 1.0))


def test_without_the_keyword_nothing_changes():
    ch = gaussian_chain(seed=8, n=900, d=3, weights="int")
    a, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence(info=True)
    assert "marginals" not in info
    for off in (None, False):
        m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), marginals=off)
        b, info = m.evidence(info=True)
        assert "marginals" not in info and np.array_equal(a, b) and m.param_marginals is None
    c, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), marginals=True).evidence(info=True)
    assert np.array_equal(a, c) and "marginals" in info


def test_refused_combinations_and_the_plan():
    ch = gaussian_chain(seed=2, n=2000, d=3)
    with pytest.raises(ValueError, match="marginals with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=3, brange=[2.5, 3.2], bscale="logpower", backend=OracleBackend(), marginals=True)
    with pytest.raises(ValueError, match="marginals with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=2, backend=OracleBackend(), marginals=True)
    with pytest.raises(ValueError, match="marginals with isfunc"):
        MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend(), marginals=True)
    for bad in (1.5, tuple([0.5] * 8), {"grid": 100}):
        with pytest.raises(ValueError, match="marginals="):
            MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), marginals=bad)
    from mcevidence_amd import farm, resident
    assert resident.plan(marginals=True) == resident.RESIDENT == resident.plan(marginals={"grid": 64}) == resident.plan()
    with pytest.raises(ValueError, match="marginals="):
        resident.plan(marginals=2.0)
    assert not any("marginals" in k or "marginals" in v for k, v in resident.REASONS.items())
    for kw, key in ((dict(ischain=False), "ischain"), (dict(thinlen=-1), "negative_thinlen"), (dict(thinlen=0.5), "poisson"), (dict(isfunc=abs), "isfunc"),
                    (dict(nbatch=2), "batches"), (dict(verbose=2), "verbose"), (dict(covtype="diag"), "covtype"), (dict(split=True, covtype="single"), "split_single"),
                    (dict(split=True, jackknife=4), "jackknife_cross"), (dict(ndim=128), "ndim"), (dict(distributed=True), "distributed"),
                    (dict(ncols=[5, 6]), "columns"), (dict(nrows=1), "rows")):
        assert resident.plan(**kw) == resident.plan(marginals=True, **kw) == resident.REASONS[key], key
    # the farm's rule for one value or one per root
    assert farm._per_root_marginals(None, 3) == [None] * 3 and farm._per_root_marginals({"grid": 64}, 2) == [{"grid": 64}] * 2
    assert farm._per_root_marginals([0.9, 0.5], 2) == [[0.9, 0.5]] * 2 and farm._per_root_marginals([(0.9,), None, {"grid": 64}], 3) == [(0.9,), None, {"grid": 64}]
    with pytest.raises(ValueError, match="marginals: expected 2 entries, got 3"):
        farm._per_root_marginals([True, None, None], 2)
    with pytest.raises(ValueError, match="not a mixture"):
        farm._per_root_marginals([0.5, None], 2)


def test_status_through_mcevidence(caplog):
    ch = gaussian_chain(seed=6, n=800, d=3, weights="int")
    bad = ch.copy()
    bad[123, 3] = np.inf                                   # a value that is not finite in the second measured column
    plain = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend()).evidence()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        lnE, info = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend(), marginals=True).evidence(info=True)
        assert info["marginals"]["status"] == 0            # (the column is not measured)
        caplog.clear()
        m = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend(), marginals=True)
        m.ndim = 2                                         # (measure it without sending the row through a search)
        m._fill_marginals()
    d = m.info["marginals"]
    assert np.array_equal(lnE, plain) and d["status"] == 3 and d["column"] == 1 and d["rows"] == 800
    assert all(np.isnan(d[k]).all() for k in ("sum_w", "ess", "mean", "sd", "h", "density", "mode", "lower", "upper", "pieces", "edge"))
    assert sum("marginals: status 3" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING) == 1


def test_command_line(tmp_path, monkeypatch, capsys, caplog):
    from mcevidence_amd import cli, evidence
    from mcevidence_amd.synth import write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=400, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    with open(root + ".paramnames", "w") as fh:
        fh.write("om0\t\\Omega_0\nom1   \\Omega_1\nom2\n")
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    args = [root, "-k", "3", "--allparams"]
    # -vb 0 with --jackknife: printed once, in the order information, summary, marginals, ln(B)
    npz = str(tmp_path / "m.npz")
    cli.main(args + ["-vb", "0", "--information", "--summary", "--marginals", "--marginals-grid", "64", "--marginals-out", npz, "--jackknife=4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    first = lambda key: min(i for i, ln in enumerate(out) if ln.startswith(key))      # noqa: E731
    last = lambda key: max(i for i, ln in enumerate(out) if ln.startswith(key))       # noqa: E731
    assert sum(ln.startswith("marginals: parameter") for ln in out) == 1 and sum(ln.startswith("marginals: om") for ln in out) == 3
    assert last("D_KL") < first("summary:") <= last("summary:") < first("marginals:") <= last("marginals:") < first("ln(B)[k=1] =")
    head = out[first("marginals: parameter")]
    assert "lower68" in head and "upper95" in head and head.split()[-1] == "h" and len(out[first("marginals: om0")].split()) == 2 + 1 + 3 + 3 + 1
    z = np.load(npz)
    m = MCEvidence(root, kmax=3, verbose=0, backend=OracleBackend(), marginals={"grid": 64})
    m.evidence()
    assert list(z["roots"]) == [root] and list(z["names_0"]) == ["om0", "om1", "om2"] == m.param_marginals["names"]
    assert z["density_0"].shape == z["grid_0"].shape == (3, 64) and np.array_equal(z["density_0"], m.param_marginals["density"])
    assert np.array_equal(z["grid_0"][1], mg.grid_points(m.param_marginals["grid_lo"][1], m.param_marginals["grid_step"][1], 64))
    assert [ln.strip() for ln in mg.lines(m.param_marginals)][1:] == [ln for ln in out if ln.startswith("marginals: om")]
    # -vb 1: the class logs them after the summary lines, and the CLI does not print them a second time
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1", "--summary", "--marginals", "0.9", "--marginals-scale", "0.5", "--jackknife=4"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    msgs = [r.getMessage().strip() for r in caplog.records]
    assert not any(ln.startswith("marginals:") for ln in printed) and sum(m.startswith("marginals: parameter") for m in msgs) == 1
    assert max(i for i, m in enumerate(msgs) if m.startswith("summary:")) < min(i for i, m in enumerate(msgs) if m.startswith("marginals:"))
    assert "lower90" in [m for m in msgs if m.startswith("marginals: parameter")][0]
    # without --jackknife they come where the ln(B) lines come from, before them; without the flag there is no such line
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1", "--marginals"])
        n_with = sum(r.getMessage().strip().startswith("marginals:") for r in caplog.records)
        msgs = [r.getMessage().strip() for r in caplog.records]
        assert max(i for i, m in enumerate(msgs) if m.startswith("marginals:")) < min(i for i, m in enumerate(msgs) if m.startswith("ln(B)[k=1] ="))
        caplog.clear()
        cli.main(args + ["-vb", "1"])
    assert n_with == 4 and not any(r.getMessage().strip().startswith("marginals:") for r in caplog.records)
    p = cli.build_parser()
    a = p.parse_args([root, "--farm", "--marginals", "0.5", "0.9", "--marginals-grid", "1024", "--marginals-scale", "2"])
    assert cli._marginals_kw(a) == {"marginals": {"probs": (0.5, 0.9), "grid": 1024, "scale": 2.0}}
    assert cli._marginals_kw(p.parse_args([root, "--marginals", "--resident"])) == {"marginals": True} and cli._marginals_kw(p.parse_args([root])) == {}
    assert cli._marginals_kw(p.parse_args([root, "--tension", "a", "b", "--marginals", "0.9"])) == {"marginals": (0.9,)}
    for bad in (["--marginals-grid", "64"], ["--marginals-out", npz], ["--marginals", "--marginals-grid", "100"]):
        with pytest.raises(SystemExit):
            cli.main(args + bad)


Z68 = 0.9944578832097535                                   # the normal quantile of (1 + 0.68) / 2


@pytest.mark.parametrize("seed", range(5))
def test_gaussian_samples_give_their_hpd_interval(seed):
    """iid N(0, 1), unit weights, n = 20 000.  A Gaussian smoothed by a Gaussian of width h is a Gaussian of variance 1 + h^2: the 68 % HPD
    interval is +-0.9945 sqrt(1 + h^2).  The tolerances (docs/design/marginals.md): for a limit, the sampling error of a quantile at that
    level, sqrt(q (1 - q)) / (phi(z) sqrt(n)) = 1.37 / sqrt(n), at 5 sigma, plus one grid step; for the mode, the asymptotic standard
    deviation of the mode of a kernel estimate, sqrt(int K'^2 f(0) / (n h^3 f''(0)^2)) = sqrt(1 / (4 sqrt(pi) n h^3 phi(0))) for a Gaussian
    kernel on N(0, 1), at 5 sigma, plus one grid step."""
    n = 20000
    x = np.random.default_rng(seed).standard_normal((n, 1))
    d = mg.build(mg.measure(np.ones(n), x, mg.DEFAULT_PROBS), mg.spec(True))
    h, step = d["h"][0], d["grid_step"][0]
    want = Z68 * math.sqrt(1.0 + h * h)
    tol = 5.0 * 1.37 / math.sqrt(n) + step
    worst = max(abs(d["lower"][0][0] + want), abs(d["upper"][0][0] - want))
    mode_sd = math.sqrt(1.0 / (4.0 * math.sqrt(math.pi) * n * h ** 3 * (1.0 / math.sqrt(2.0 * math.pi))))
    print("seed %d: h %.4f step %.4f  68 %% limits off by %.4f = %.2f sigma + step (tolerance %.4f);  mode %.4f = %.2f of its sd %.4f" % (
        seed, h, step, worst, max(worst - step, 0.0) * math.sqrt(n) / 1.37, tol, d["mode"][0], abs(d["mode"][0]) / mode_sd, mode_sd))
    assert worst <= tol and abs(d["mode"][0]) <= 5.0 * mode_sd + step
    assert d["pieces"][0][0] == 1 and d["pieces"][1][0] == 1 and d["edge"][1][0] == 0 and d["ess"] == n
    assert abs(h - d["sd"][0] * (4.0 / (3.0 * n)) ** 0.2) <= 1e-15


def test_a_bimodal_posterior_has_two_pieces():
    """An equal mixture of N(-4, 1) and N(+4, 1): the 68 % HPD region is two intervals, one about each peak, while summary's equal-tailed
    68 % interval runs across the empty gap and contains 0, where the density is below a hundredth of the peaks' (2 exp(-8 / (1 + h^2)) = 0.006 of them for the rule's h = 0.6)"""
    rng = np.random.default_rng(11)
    n = 20000
    x = np.concatenate([rng.normal(-4.0, 1.0, n // 2), rng.normal(4.0, 1.0, n // 2 + 7)])[:, None]
    a = np.ones(x.shape[0])
    d = mg.build(mg.measure(a, x, (0.68,)), mg.spec((0.68,)))
    s = sm.build(sm.measure(a, x, None, sm.targets((0.68,))), (0.68,), 0.0)
    assert d["pieces"][0][0] == 2 and d["edge"][0][0] == 0
    assert s["lower"][0][0] < 0.0 < s["upper"][0][0]
    g = mg.grid_points(d["grid_lo"][0], d["grid_step"][0], d["grid"])
    at0 = d["density"][0][np.argmin(np.abs(g))]
    assert at0 < 1e-2 * d["mode_density"][0] and abs(abs(d["mode"][0]) - 4.0) < 0.5
    # the region is shorter than the equal-tailed interval
    _, masks = mg.hpd_selection(d["density"][0], (0.68,))
    assert masks[0].sum() * d["grid_step"][0] < 0.75 * (s["upper"][0][0] - s["lower"][0][0])


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    lib = _capi.load()
    for s in ("mce_param_marginals_out_doubles", "mce_param_marginals_workspace_bytes", "mce_param_marginals_dev", "mce_param_marginals_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_MARGINALS_HEAD == mg.HEAD == 8 and _capi.MCE_MARGINALS_MAX_P == mg.MAX_PROBS == 7
    assert _capi.param_marginals_out_doubles(27, 2, 512) == 8 + 27 * (10 + 8 + 512) == _capi.marginals_block_doubles(27, 2, 512)
    for bad in ((0, 2, 512), (128, 2, 512), (4, 0, 512), (4, 8, 512), (4, 2, 100), (4, 2, 2048)):
        assert _capi.param_marginals_out_doubles(*bad) == 0, bad
    small, big = _capi.param_marginals_workspace_bytes(1000, 1, 8, 2, 512), _capi.param_marginals_workspace_bytes(10 ** 6, 1, 27, 2, 512)
    assert 0 < small < 2 ** 20 and 64 * 27 * 512 * 8 < big < 2 ** 28
    for bad in ((-1, 1, 4, 2, 512), (10, 0, 4, 2, 512), (10, 1, 128, 2, 512), (10, 1, 4, 0, 512), (10, 1, 4, 8, 512), (10, 1, 4, 2, 500)):
        assert _capi.param_marginals_workspace_bytes(*bad) == 0, bad
    # argument errors come before any device call
    ok = (8, 4, 5, 4, 8)
    for segs, probs, grid, scale, words in (([], [0.5], 512, 1.0, "segments"), ([ok], [], 512, 1.0, "probabilities"), ([ok], [0.5] * 8, 512, 1.0, "probabilities"),
                                            ([ok], [0.0], 512, 1.0, "probability 0"), ([ok], [0.5, 1.0], 512, 1.0, "probability 1"), ([ok], [0.5], 100, 1.0, "grid"),
                                            ([ok], [0.5], 512, 0.0, "scale"), ([ok], [0.5], 512, float("inf"), "scale"), ([ok], [0.5], 512, float("nan"), "scale"),
                                            ([(8, 3, 5, 4, 8)], [0.5], 512, 1.0, "segment 0"), ([(8, 4, 5, 0, 8)], [0.5], 512, 1.0, "segment 0"),
                                            ([ok, (8, 200, 5, 128, 8)], [0.5], 512, 1.0, "segment 1"), ([(8, 4, -1, 4, 8)], [0.5], 512, 1.0, "segment 0"),
                                            ([(0, 4, 5, 4, 8)], [0.5], 512, 1.0, "segment 0")):
        with pytest.raises(ValueError, match=words):
            _capi.param_marginals_dev(segs, probs, grid, scale, 1, 1 << 30)
    with pytest.raises(ValueError):
        _capi.param_marginals([(np.zeros((3, 2)), 2, np.zeros(4))], [0.5], 512, 1.0)


def test_no_device_is_its_own_error():
    from mcevidence_amd import _capi
    c = mc.cases()["n64_d8_G64_integer"]
    if _capi.device_count() > 0:                           # (a device is visible: the same call answers)
        assert mg.measure_native(c.a, c.x[:, :c.d], *c.spec)["status"] == 0
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_marginals([c.system], c.probs, c.grid, c.scale)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_marginals_dev([(8, 4, 5, 4, 8)], [0.5], 512, 1.0, 8, 1 << 30)


def test_under_a_process_group_every_rank_computes_its_own(monkeypatch):
    import torch.distributed as dist
    from mcevidence_amd import parallel, resident
    ch = gaussian_chain(seed=12, n=700, d=3, weights="int")
    want = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), marginals=True).evidence(info=True)[1]["marginals"]
    m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), marginals=True)

    def refuse(*a, **k):
        raise AssertionError("a collective was called")
    monkeypatch.setattr(parallel, "is_distributed", lambda *a, **k: True)
    for name in ("all_reduce", "all_gather", "all_gather_object", "broadcast", "broadcast_object_list", "barrier", "reduce", "gather", "all_to_all_single"):
        monkeypatch.setattr(dist, name, refuse)
    m._fill_marginals()
    got = m.info["marginals"]
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in KEYS - {"names", "probs"}) and got["names"] == want["names"]
    assert resident.plan(distributed=True, marginals=True) == resident.REASONS["distributed"]
