"""contours on the CPU: the serial driver of csrc/param_contours.hpp (a stand-alone sanitized program) and ``contours.measure`` on the
cases of tests/contours_cases.py -- the moments and h within their bounds, every density within its bound of the exact product-kernel
estimate at the reported parameters (mpmath on the query cells, the extended format on all), the two forms within two bounds of each
other, every decision bit for bit the serial rule's on the block's own densities, at most two undecided cells per (pair, p) against the
oracle; the statuses; the keyword; the statistical check of the 68 % region's area.

The area check's tolerance (docs/design/contours.md): for n iid draws of N(0, Sigma) the estimate's expectation is N(0, Sigma + diag(h^2)),
whose region of p has the area A(p) = 2 pi sqrt(det(Sigma + diag(h^2))) ln(1 / (1 - p)).  (a) The level is set by the sample: the share
of the sample inside a fixed region has the standard deviation sqrt(p (1 - p) / n), and dA/dp = 2 pi sqrt(det) / (1 - p); at 5 sigma that
is A(p) * 5 sqrt(p / ((1 - p) n)) / ln(1 / (1 - p)).  (b) The area is counted in cells: every cell the boundary crosses may be counted
wrongly, and those lie within one cell diagonal of the ellipse, whose perimeter is at most 2 pi sqrt((a^2 + b^2) / 2) for the semi-axes
a, b.  Sigma is the sample's own weighted covariance, so its sampling error does not enter.  Observed on seeds 0 - 4: the error is
0.14 % to 0.67 % of the area, 0.003 to 0.015 of the tolerance (the cell term dominates it)."""
import logging

import numpy as np
import pytest

import contours_cases as cc
from mcevidence_amd import contours as ct


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cc.build_checker(tmp_path_factory.mktemp("param_contours"))


def test_parts_pairs_and_sizes(checker):
    import subprocess
    out = subprocess.run([checker, "parts"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=11"), out.stdout + out.stderr
    assert ct.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


@pytest.mark.parametrize("name", list(cc.cases()))
def test_serial_driver_and_numpy_against_the_oracle(name, checker, tmp_path):
    c = cc.cases()[name]
    native, = cc.run_native(checker, tmp_path, [(c.a, c.x, c.d)], c.cols, c.probs, c.grid, c.scale)
    host = ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid, c.scale)
    stats = {}
    for what, got in (("serial", native), ("numpy", host)):
        good = cc.check_moments(c, got, what)
        assert len(good) == c.nc
        for p, s, t in cc.oracle_pairs(c):
            cc.check_pair(c, got, p, s, t, what, stats=stats)
        cc.check_against_numpy(c, got, what)
    assert cc.check_decisions_native(checker, tmp_path, [native, host], c.probs, c.grid) == 2 * c.nc * (c.nc - 1) // 2
    assert stats["undecided"] <= cc.MAX_UNDECIDED


def test_a_pair_does_not_notice_the_others(checker, tmp_path):
    c = cc.cases()["n15_nc6_G64_fractional"]
    whole, = cc.run_native(checker, tmp_path, [(c.a, c.x, c.d)], c.cols, c.probs, c.grid, c.scale)
    alone, = cc.run_native(checker, tmp_path, [(c.a, c.x, c.d)], (1, 4), (0.5,), c.grid, c.scale)
    p = ct.pairs(6).index((1, 4))
    assert whole["density"][p].tobytes() == alone["density"][0].tobytes()
    assert (whole["mode_x"][p], whole["mode_y"][p]) == (alone["mode_x"][0], alone["mode_y"][0])


def test_status_cases(checker, tmp_path):
    for name, a, x, status, column in cc.status_cases():
        native, = cc.run_native(checker, tmp_path, [(a, x, 2)], (0, 1), cc.PROBS, 32, 1.0)
        host = ct.measure(a, x, (0, 1), cc.PROBS, 32)
        for got in (native, host):
            cc.assert_failed_system(got, status, column, int(np.count_nonzero(a != 0)), name)
            assert np.array_equal(got["col"], [0.0, 1.0])
        assert cc.equal_blocks(native, host), name


def test_a_constant_column_fails_its_pairs_alone(checker, tmp_path, caplog):
    c = cc.constant_column_case()
    native, = cc.run_native(checker, tmp_path, [(c.a, c.x, c.d)], c.cols, c.probs, c.grid, c.scale)
    host = ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid, c.scale, at=native)
    for got in (native, host):
        assert list(got["col_status"]) == [0.0, 7.0, 0.0] and list(got["pair_status"]) == [7.0, 0.0, 7.0]
        cc.assert_failed_pair(got, 0)
        cc.assert_failed_pair(got, 2)
        assert np.isnan(got["h"][1]) and np.isfinite(got["density"][1]).all()
    alone, = cc.run_native(checker, tmp_path, [(c.a, c.x, c.d)], (0, 2), c.probs, c.grid, c.scale)
    assert native["density"][1].tobytes() == alone["density"][0].tobytes()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        ct.build(host, (c.probs, c.grid, c.scale, c.cols))
    assert len([r for r in caplog.records if "contours" in r.getMessage()]) == 1


def test_keyword():
    assert ct.spec(None) is None and ct.spec(False) is None
    assert ct.spec(True, ndim=3) == ((0.68, 0.95), 64, 1.0, (0, 1, 2))
    assert ct.spec((0.5,), ndim=2) == ((0.5,), 64, 1.0, (0, 1))
    assert ct.spec({"probs": 0.9, "grid": 32, "scale": 0.5, "params": ["b", 0]}, ndim=3, names=["a", "b", "c"]) == ((0.9,), 32, 0.5, (0, 1))
    for bad in ({"grid": 128}, {"grid": 64.5}, {"params": [0]}, {"params": [0, 0]}, {"params": list(range(33))}, {"params": "ab"}, {"other": 1}, (0.0,), (1.5,),
                {"scale": 0.0}, {"params": [0, -1]}):
        with pytest.raises(ValueError):
            ct.spec(bad, ndim=40)
    with pytest.raises(ValueError, match="params"):
        ct.spec(True, ndim=33)
    with pytest.raises(ValueError):
        ct.spec(True, ndim=1)
    with pytest.raises(ValueError, match="not among"):
        ct.spec({"params": ["a", "zz"]}, ndim=3, names=["a", "b", "c"])
    with pytest.raises(ValueError):
        ct.spec({"params": [0, 5]}, ndim=3)
    with pytest.raises(ValueError, match="batched"):
        ct.refuse(True, nbatch=2)
    with pytest.raises(ValueError, match="isfunc"):
        ct.refuse(True, isfunc=lambda v: v)
    ct.refuse(None, nbatch=2)


def test_lines_and_save(tmp_path):
    c = cc.cases()["n17_nc3_G64_integer"]
    m = ct.build(ct.measure(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid), (c.probs, c.grid, 1.0, c.cols), ["a", "b", "c"])
    ln = ct.lines(m)
    assert len(ln) == 4 and len(set(ln)) == 4 and ln[1].split()[1:3] == ["a", "b"] and ln[3].split()[1:3] == ["b", "c"]
    ct.save(tmp_path / "c.npz", ["root"], [{"contours": m}])
    z = np.load(tmp_path / "c.npz")
    assert z["density_0"].shape == (3, 64, 64) and z["grid_x_0"].shape == (3, 64) and z["levels_0"].shape == (2, 3) and list(z["pairs_0"][1]) == [0, 2]


@pytest.mark.parametrize("seed", range(5))
def test_area_of_the_68_percent_region_of_a_correlated_normal(seed):
    rng = np.random.default_rng(seed)
    n, p = 20000, 0.68
    x = rng.multivariate_normal([0.0, 0.0], [[1.0, 0.8], [0.8, 1.0]], n)
    got = ct.measure(np.ones(n), x, (0, 1), (p,), 64)
    area = got["cells"][0][0] * got["step"][0] * got["step"][1]
    sigma = np.cov(x.T, bias=True) + np.diag(got["h"] ** 2)
    r2 = np.log(1.0 / (1.0 - p))
    want = 2 * np.pi * np.sqrt(np.linalg.det(sigma)) * r2
    lam = np.linalg.eigvalsh(sigma) * 2 * r2                        # the squared semi-axes
    tol = want * 5 * np.sqrt(p / ((1 - p) * n)) / r2 + 2 * np.pi * np.sqrt(lam.sum() / 2) * np.hypot(got["step"][0], got["step"][1])
    print("seed %d: area %.4f, expected %.4f, error %.4f, tolerance %.4f (%.3g of it)" % (seed, area, want, abs(area - want), tol, abs(area - want) / tol))
    assert abs(area - want) <= tol
    assert got["edge"][0][0] == 0.0


# ---- the public interface on the CPU (the oracle backends: the NumPy form) -------------------------------------------------------------
def _inputs(m):
    part = m.gd.data["s1"]
    return np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)[:, :m.ndim]


def test_mcevidence_auto_and_cross_forms():
    from helpers import OracleBackend, OracleFeedBackend
    from mcevidence_amd.evidence import MCEvidence, evidence_many
    from mcevidence_amd.synth import gaussian_chain
    ch = gaussian_chain(seed=3, n=1500, d=4, weights="int")
    for split, backend in ((False, OracleBackend), (True, OracleFeedBackend)):
        np.random.seed(5)
        m = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend(), contours={"grid": 32})
        lnE, info = m.evidence(info=True)
        a, x = _inputs(m)
        d = info["contours"]
        assert len(a) == (750 if split else 1500) and m.param_contours is d and m.contours_spec == {"grid": 32}
        ref = ct.measure(a, x, (0, 1, 2, 3), (0.68, 0.95), 32)
        assert d["cols"] == [0, 1, 2, 3] and d["pairs"] == ct.pairs(4) and d["names"] == ["p0", "p1", "p2", "p3"] and d["density"].shape == (6, 32, 32)
        assert np.array_equal(d["density"], ref["density"]) and np.array_equal(d["level"], ref["level"]) and np.array_equal(d["cells"], ref["cells"])
        cell = np.array([d["grid_step"][s] * d["grid_step"][t] for s, t in ct.pairs(4)])
        assert np.all(d["density"] >= 0.0) and np.all(np.abs(d["density"].sum(axis=(1, 2)) * cell - 1.0) < 1e-2)
        assert np.all(d["level"][0] > d["level"][1]) and np.all(d["cells"][0] < d["cells"][1]) and np.all(d["mode_density"] >= d["level"][0])
        np.random.seed(5)
        plain, pinfo = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend()).evidence(info=True)
        assert np.array_equal(lnE, plain) and "contours" not in pinfo
    # chosen parameters, together with marginals and the jackknife: no sigma here
    m = MCEvidence([ch], kmax=3, verbose=0, ndim=3, backend=OracleBackend(), contours={"probs": (0.5,), "params": [2, 0], "scale": 0.5}, marginals=True, jackknife=4)
    lnE, info = m.evidence(info=True)
    d = info["contours"]
    assert d["cols"] == [0, 2] and d["density"].shape == (1, 64, 64) and d["scale"] == 0.5 and "marginals" in info and "jackknife" in info and not any("sigma" in k for k in d)
    ms = [MCEvidence([gaussian_chain(seed=s, n=401, d=3, weights="int")], kmax=3, verbose=0, backend=OracleBackend(), contours=(0.9,)) for s in (1, 2)]
    for m, (lnE, info) in zip(ms, evidence_many(ms, info=True)):
        assert info["contours"]["probs"] == (0.9,) and info["contours"]["density"].shape == (3, 64, 64)


def test_without_the_keyword_nothing_changes():
    from helpers import OracleBackend
    from mcevidence_amd.evidence import MCEvidence
    from mcevidence_amd.synth import gaussian_chain
    ch = gaussian_chain(seed=8, n=900, d=3, weights="int")
    a, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence(info=True)
    assert "contours" not in info
    for off in (None, False):
        m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), contours=off)
        b, info = m.evidence(info=True)
        assert "contours" not in info and np.array_equal(a, b) and m.param_contours is None
    c, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), contours=True).evidence(info=True)
    assert np.array_equal(a, c) and "contours" in info


def test_refused_combinations_and_the_plan():
    from helpers import OracleBackend
    from mcevidence_amd import resident
    from mcevidence_amd.evidence import MCEvidence
    from mcevidence_amd.synth import gaussian_chain
    ch = gaussian_chain(seed=2, n=2000, d=3)
    with pytest.raises(ValueError, match="contours with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=3, brange=[2.5, 3.2], bscale="logpower", backend=OracleBackend(), contours=True)
    with pytest.raises(ValueError, match="contours with isfunc"):
        MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend(), contours=True)
    for bad in (1.5, tuple([0.5] * 8), {"grid": 128}, {"params": [1]}):
        with pytest.raises(ValueError, match="contours="):
            MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), contours=bad)
    # what only the data can refuse is refused when they are known: a column past ndim, an unknown name, fewer than two parameters
    for bad, nd in (({"params": [0, 3]}, 3), ({"params": ["p0", "nope"]}, 3), (True, 1)):
        with pytest.raises(ValueError, match="contours="):
            MCEvidence([ch], kmax=3, verbose=0, ndim=nd, backend=OracleBackend(), contours=bad).evidence()
    assert resident.plan(contours=True) == resident.RESIDENT == resident.plan(contours={"grid": 32, "params": [0, 5]}) == resident.plan()
    with pytest.raises(ValueError, match="contours="):
        resident.plan(contours=2.0)
    for kw, key in ((dict(isfunc=abs), "isfunc"), (dict(nbatch=2), "batches"), (dict(distributed=True), "distributed"), (dict(ndim=128), "ndim")):
        assert resident.plan(**kw) == resident.plan(contours=True, **kw) == resident.REASONS[key], key


def test_command_line(tmp_path, monkeypatch, capsys, caplog):
    from helpers import OracleBackend
    from mcevidence_amd import cli, evidence
    from mcevidence_amd.evidence import MCEvidence
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=400, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    with open(root + ".paramnames", "w") as fh:
        fh.write("om0\t\\Omega_0\nom1   \\Omega_1\nom2\n")
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    args = [root, "-k", "3", "--allparams"]
    npz = str(tmp_path / "c.npz")
    # -vb 0 with --jackknife: printed once, after the marginals lines and before the ln(B) lines
    cli.main(args + ["-vb", "0", "--marginals", "--marginals-grid", "64", "--contours", "--contours-grid", "32", "--contours-out", npz, "--jackknife=4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    first = lambda key: min(i for i, ln in enumerate(out) if ln.startswith(key))      # noqa: E731
    last = lambda key: max(i for i, ln in enumerate(out) if ln.startswith(key))       # noqa: E731
    assert sum(ln.startswith("contours: x") for ln in out) == 1 and sum(ln.startswith("contours: om") for ln in out) == 3
    assert last("marginals:") < first("contours:") <= last("contours:") < first("ln(B)[k=1] =")
    head = out[first("contours: x")]
    assert "level68" in head and "level95" in head and len(out[first("contours: om0")].split()) == 1 + 2 + 2 + 2 * 2
    z = np.load(npz)
    m = MCEvidence(root, kmax=3, verbose=0, backend=OracleBackend(), contours={"grid": 32})
    m.evidence()
    assert list(z["roots"]) == [root] and list(z["names_0"]) == ["om0", "om1", "om2"] == m.param_contours["names"]
    assert z["density_0"].shape == (3, 32, 32) and np.array_equal(z["density_0"], m.param_contours["density"]) and np.array_equal(z["levels_0"], m.param_contours["level"])
    assert [ln.strip() for ln in ct.lines(m.param_contours)][1:] == [ln for ln in out if ln.startswith("contours: om")]
    # -vb 1: the class logs them after the marginals lines, and the CLI does not print them a second time; names choose the columns
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1", "--marginals", "--contours", "0.9", "--contours-params", "om2", "0", "--contours-scale", "0.5", "--jackknife=4"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    msgs = [r.getMessage().strip() for r in caplog.records]
    assert not any(ln.startswith("contours:") for ln in printed) and sum(m.startswith("contours: x") for m in msgs) == 1
    assert [m.split()[1:3] for m in msgs if m.startswith("contours: om")] == [["om0", "om2"]]
    assert max(i for i, m in enumerate(msgs) if m.startswith("marginals:")) < min(i for i, m in enumerate(msgs) if m.startswith("contours:"))
    assert "level90" in [m for m in msgs if m.startswith("contours: x")][0]
    # without the flag there is no such line
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1"])
    assert not any(r.getMessage().strip().startswith("contours:") for r in caplog.records)
    p = cli.build_parser()
    a = p.parse_args([root, "--farm", "--contours", "0.5", "0.9", "--contours-grid", "32", "--contours-scale", "2", "--contours-params", "a", "3"])
    assert cli._contours_kw(a) == {"contours": {"probs": (0.5, 0.9), "grid": 32, "scale": 2.0, "params": ["a", 3]}}
    assert cli._contours_kw(p.parse_args([root, "--contours", "--resident"])) == {"contours": True} and cli._contours_kw(p.parse_args([root])) == {}
    assert cli._contours_kw(p.parse_args([root, "--tension", "a", "b", "--contours", "0.9"])) == {"contours": (0.9,)}
    for bad in (["--contours-grid", "64"], ["--contours-out", npz], ["--contours-params", "a", "b"], ["--contours", "--contours-grid", "128"]):
        with pytest.raises(SystemExit):
            cli.main(args + bad)


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    lib = _capi.load()
    for s in ("mce_param_contours_out_doubles", "mce_param_contours_workspace_bytes", "mce_param_contours_dev", "mce_param_contours_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_CONTOURS_HEAD == ct.HEAD == 8 and _capi.MCE_CONTOURS_MAX_COLS == ct.MAX_COLS == 32
    assert _capi.param_contours_out_doubles(27, 2, 64) == 8 + 9 * 27 + 351 * (4 + 14 + 4096) == _capi.contours_block_doubles(27, 2, 64)
    for bad in ((1, 2, 64), (33, 2, 64), (4, 0, 64), (4, 8, 64), (4, 2, 16), (4, 2, 128)):
        assert _capi.param_contours_out_doubles(*bad) == 0, bad
    small, big = _capi.param_contours_workspace_bytes(1000, 1, 8, 2, 2, 32), _capi.param_contours_workspace_bytes(10 ** 6, 1, 27, 27, 2, 64)
    assert 0 < small < 2 ** 20 and 16 * 351 * 4096 * 8 < big < 2 ** 28
    for bad in ((-1, 1, 4, 2, 2, 64), (10, 0, 4, 2, 2, 64), (10, 1, 128, 2, 2, 64), (10, 1, 4, 1, 2, 64), (10, 1, 4, 2, 0, 64), (10, 1, 4, 2, 8, 64), (10, 1, 4, 2, 2, 100)):
        assert _capi.param_contours_workspace_bytes(*bad) == 0, bad
    # argument errors come before any device call
    ok = (8, 4, 5, 4, 8)
    for segs, cols, probs, grid, scale, words in (([], [0, 1], [0.5], 64, 1.0, "segments"), ([ok], [0], [0.5], 64, 1.0, "columns"), ([ok], list(range(33)), [0.5], 64, 1.0, "columns"),
                                                  ([ok], [1, 1], [0.5], 64, 1.0, "strictly increasing"), ([ok], [2, 1], [0.5], 64, 1.0, "strictly increasing"),
                                                  ([ok], [-1, 1], [0.5], 64, 1.0, "strictly increasing"), ([ok], [0, 4], [0.5], 64, 1.0, "column 4 asked of segment 0"),
                                                  ([ok, (8, 3, 5, 3, 8)], [0, 3], [0.5], 64, 1.0, "column 3 asked of segment 1"),
                                                  ([ok], [0, 1], [], 64, 1.0, "probabilities"), ([ok], [0, 1], [0.5] * 8, 64, 1.0, "probabilities"),
                                                  ([ok], [0, 1], [0.0], 64, 1.0, "probability 0"), ([ok], [0, 1], [0.5], 128, 1.0, "grid"), ([ok], [0, 1], [0.5], 64, 0.0, "scale"),
                                                  ([ok], [0, 1], [0.5], 64, float("nan"), "scale"), ([(8, 3, 5, 4, 8)], [0, 1], [0.5], 64, 1.0, "segment 0"),
                                                  ([(0, 4, 5, 4, 8)], [0, 1], [0.5], 64, 1.0, "segment 0"), ([(8, 4, -1, 4, 8)], [0, 1], [0.5], 64, 1.0, "segment 0")):
        with pytest.raises(ValueError, match=words):
            _capi.param_contours_dev(segs, cols, probs, grid, scale, 1, 1 << 30)
    with pytest.raises(ValueError):
        _capi.param_contours([(np.zeros((3, 2)), 2, np.zeros(4))], [0, 1], [0.5], 64, 1.0)


def test_no_device_is_its_own_error():
    from mcevidence_amd import _capi
    c = cc.cases()["n16_nc2_G32_unit"]
    if _capi.device_count() > 0:                           # (a device is visible: the same call answers)
        assert ct.measure_native(c.a, c.x[:, :c.d], c.cols, c.probs, c.grid)["status"] == 0
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_contours([(c.x, c.d, c.a)], c.cols, c.probs, c.grid, c.scale)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_contours_dev([(8, 4, 5, 4, 8)], [0, 1], [0.5], 64, 1.0, 8, 1 << 30)


def test_under_a_process_group_every_rank_computes_its_own(monkeypatch):
    import torch.distributed as dist
    from helpers import OracleBackend
    from mcevidence_amd import parallel
    from mcevidence_amd.evidence import MCEvidence
    from mcevidence_amd.synth import gaussian_chain
    ch = gaussian_chain(seed=12, n=700, d=3, weights="int")
    want = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), contours={"grid": 32}).evidence(info=True)[1]["contours"]
    m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), contours={"grid": 32})

    def refuse(*a, **k):
        raise AssertionError("a collective was called")
    monkeypatch.setattr(parallel, "is_distributed", lambda *a, **k: True)
    for name in ("all_reduce", "all_gather", "all_gather_object", "broadcast", "broadcast_object_list", "barrier", "reduce", "gather", "all_to_all_single"):
        monkeypatch.setattr(dist, name, refuse)
    m._fill_contours()
    got = m.info["contours"]
    assert np.array_equal(got["density"], want["density"]) and np.array_equal(got["level"], want["level"]) and got["pairs"] == want["pairs"]
