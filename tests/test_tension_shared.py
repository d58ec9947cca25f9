"""tension without a GPU: ``tension.combine`` on hand-made inputs (the identity ln R - ln I = ln S, d <= 0, d - 2 ln S <= 0, a singular
C, the ``shared`` rules, the jackknife sigma as a root-sum-square, the printed lines, p and sigma_equiv against scipy), the Gaussian check
of docs/design/tension.md (iid draws of two Gaussian likelihoods and their product, every number within 5 standard errors of its
analytic value), ``evidence_tension`` on the host route and the ``--tension`` command line."""
import logging
import math

import numpy as np
import pytest

from helpers import OracleBackend
from mcevidence_amd import covariance as cv
from mcevidence_amd import information as inf
from mcevidence_amd import tension as tn

EPS = 2.0 ** -52


def run(lnE, mean_logL, bmd, mean, cov, names=None, sigma=None):
    """a hand-made (lnE, info) of one run"""
    lnE = np.asarray(lnE, dtype=np.float64)
    mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    d = len(mean)
    info = {"information": {"mean_logL": mean_logL, "var_logL": bmd / 2.0, "bmd": bmd, "ess": 100.0, "D_KL": mean_logL - lnE, "rows": 100, "sum_w": 100.0, "status": 0},
            "covariance": {"names": list(names) if names else ["p%d" % j for j in range(d)], "rows": 100, "sum_w": 100.0, "ess": 100.0, "mean": mean, "cov": cov,
                           "sd": np.sqrt(np.diagonal(cov)), "corr": cov, "status": 0, "column": -1}}
    if sigma is not None:
        info["jackknife"] = {"sigma": np.asarray(sigma[0], dtype=np.float64), "lnE": lnE, "groups": 4, "by": "blocks"}
        info["information"]["sigma"] = {"mean_logL": sigma[1], "bmd": sigma[2], "D_KL": np.asarray(sigma[0])}
    return lnE, info


def three(**kw):
    a = run([-10.25, -10.5], -3.1, 4.2, [0.0, 1.0, 2.0], np.diag([1.0, 2.0, 0.5]), **kw.get("a", {}))
    b = run([-7.125, -7.0], -2.7, 3.9, [0.5, 0.0, 2.5], np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.0], [0.0, 0.0, 1.5]]), **kw.get("b", {}))
    ab = run([-19.0, -19.5], -8.3, 4.5, [0.2, 0.6, 2.2], np.diag([0.5, 0.6, 0.3]), **kw.get("ab", {}))
    return a, b, ab


def test_the_definitions_and_the_identity():
    a, b, ab = three()
    t = tn.combine(a, b, ab, shared=3)
    assert set(t) == {"lnR", "lnI", "lnS", "d", "p", "sigma_equiv", "shift", "status"} and t["status"] == 0
    assert set(t["shift"]) == {"names", "delta", "chi2", "dof", "p", "sigma_equiv", "status"}
    assert np.array_equal(t["lnR"], ab[0] - a[0] - b[0]) and t["lnS"] == -8.3 - -3.1 - -2.7 and t["d"] == 4.2 + 3.9 - 4.5
    # ln R[k] - ln I[k] = ln S for every k, to a few eps of the largest term
    big = max(np.abs(np.concatenate([a[0], b[0], ab[0]])).max(), 8.3)
    assert np.all(np.abs(t["lnR"] - t["lnI"] - t["lnS"]) <= 8 * EPS * big)
    # a shifted prior volume moves every ln E, hence ln R and ln I alike, and leaves ln S, d, p where they are
    lnV = 3.75
    a2, b2, ab2 = (run(r[0] - lnV, r[1]["information"]["mean_logL"], r[1]["information"]["bmd"], r[1]["covariance"]["mean"], r[1]["covariance"]["cov"]) for r in (a, b, ab))
    t2 = tn.combine(a2, b2, ab2, shared=3)
    assert t2["lnS"] == t["lnS"] and t2["d"] == t["d"] and t2["p"] == t["p"] and np.allclose(t2["lnR"], t["lnR"] + lnV, rtol=0, atol=1e-13)
    assert np.all(np.abs(t2["lnR"] - t2["lnI"] - t2["lnS"]) <= 8 * EPS * (big + lnV))
    # p = Q(d / 2, (d - 2 ln S) / 2) and the shift, against a direct evaluation
    x = t["d"] - 2 * t["lnS"]
    assert t["p"] == tn.p_value(t["d"], x) and 0 < t["p"] < 1 and t["sigma_equiv"] == tn.sigma_equivalent(t["p"]) > 0
    delta = np.array([-0.5, 1.0, -0.5])
    C = a[1]["covariance"]["cov"] + b[1]["covariance"]["cov"]
    chi2 = float(delta @ np.linalg.inv(C) @ delta)
    s = t["shift"]
    assert np.array_equal(s["delta"], delta) and s["dof"] == 3 and s["status"] == 0 and abs(s["chi2"] - chi2) <= 1e-14 * chi2
    assert s["p"] == tn.p_value(3, s["chi2"]) and s["sigma_equiv"] == tn.sigma_equivalent(s["p"]) and s["names"] == ["p0", "p1", "p2"]
    assert "sigma" not in t
    # a run without the keywords
    with pytest.raises(ValueError, match="covariance=True"):
        tn.combine(a, (b[0], {"information": b[1]["information"]}), ab, shared=3)
    with pytest.raises(ValueError, match="columns"):
        tn.combine(a, (b[0][:1], b[1]), ab, shared=3)


def test_d_not_positive_and_chi2_not_positive(caplog):
    a, b, ab = three()
    ab[1]["information"]["bmd"] = 9.0                      # d = 4.2 + 3.9 - 9 < 0
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        t = tn.combine(a, b, ab, shared=3)
    warned = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert t["status"] == tn.NO_DIMENSION != 0 and math.isnan(t["p"]) and math.isnan(t["sigma_equiv"]) and t["d"] < 0 and len(warned) == 1
    assert "tension: status 1" in warned[0].getMessage() and t["shift"]["status"] == 0 and np.isfinite(t["lnR"]).all()
    a[1]["information"]["bmd"], b[1]["information"]["bmd"], ab[1]["information"]["bmd"] = 4.0, 4.5, 8.5      # d == 0 exactly is refused too
    t = tn.combine(a, b, ab, shared=3)
    assert t["d"] == 0.0 and t["status"] == tn.NO_DIMENSION and math.isnan(t["p"])
    # d - 2 ln S <= 0: p = 1, sigma_equiv = 0
    a, b, ab = three()
    ab[1]["information"]["mean_logL"] = -3.1 - 2.7 + 2.0   # ln S = 2 > d / 2 = 1.8
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        t = tn.combine(a, b, ab, shared=3)
    assert t["status"] == 0 and t["d"] - 2 * t["lnS"] < 0 and t["p"] == 1.0 and t["sigma_equiv"] == 0.0 and not caplog.records
    # an input that is not finite
    a, b, ab = three()
    a[1]["information"]["mean_logL"] = float("nan")
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        t = tn.combine(a, b, ab, shared=3)
    assert t["status"] == tn.NOT_FINITE and math.isnan(t["p"]) and len(caplog.records) == 1


def test_a_singular_c(caplog):
    a, b, ab = three()
    sing = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    a[1]["covariance"]["cov"] = sing
    b[1]["covariance"]["cov"] = sing.copy()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        t = tn.combine(a, b, ab, shared=3)
    s = t["shift"]
    warned = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert s["status"] == tn.SHIFT_NOT_POSITIVE != 0 and all(math.isnan(s[k]) for k in ("chi2", "p", "sigma_equiv")) and s["dof"] == 3
    assert len(warned) == 1 and "not positive definite" in warned[0].getMessage() and t["status"] == 0 and 0 < t["p"] < 1
    # the well-conditioned part alone is fine
    assert tn.combine(a, b, ab, shared=1)["shift"]["status"] == 0
    # a NaN covariance (a run of status 3)
    a[1]["covariance"]["cov"] = np.full((3, 3), np.nan)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        s = tn.combine(a, b, ab, shared=3)["shift"]
    assert s["status"] == tn.SHIFT_NOT_FINITE and math.isnan(s["chi2"]) and np.isnan(s["delta"]).all() and len(caplog.records) == 1


def test_the_shared_rules():
    na, nb = ["omegabh2", "omegach2", "tau", "A_planck"], ["tau", "omegabh2", "b_des", "omegach2"]
    a, b, ab = three(a=dict(names=na[:3]), b=dict(names=nb[:3]))
    # names on both sides: the common names in A's order, each side's own columns
    s = tn.combine(a, b, ab)["shift"]
    assert s["names"] == ["omegabh2", "tau"] and s["dof"] == 2
    assert np.array_equal(s["delta"], [0.0 - 0.0, 2.0 - 0.5])
    C = np.array([[1.0 + 1.0, 0.0 + 0.3], [0.0 + 0.3, 0.5 + 2.0]])
    d = np.array([0.0, 1.5])
    assert abs(s["chi2"] - float(d @ np.linalg.inv(C) @ d)) < 1e-14
    assert tn.shared_parameters(na, nb) == (["omegabh2", "omegach2", "tau"], [0, 1, 2], [1, 3, 0])
    # explicit names, an explicit count
    assert tn.combine(a, b, ab, shared=["tau"])["shift"]["names"] == ["tau"] and tn.combine(a, b, ab, shared=["tau"])["shift"]["delta"][0] == 1.5
    s2 = tn.combine(a, b, ab, shared=2)["shift"]
    assert s2["names"] == ["omegabh2", "omegach2"] and np.array_equal(s2["delta"], [-0.5, 1.0])
    with pytest.raises(ValueError, match="not a parameter of both"):
        tn.combine(a, b, ab, shared=["tau", "b_des"])
    with pytest.raises(ValueError, match="leading columns"):
        tn.combine(a, b, ab, shared=4)
    with pytest.raises(ValueError, match="leading columns"):
        tn.combine(a, b, ab, shared=0)
    # names on one side only: shared is required, as a count or as names both sides have
    a, b, ab = three(a=dict(names=na[:3]))
    with pytest.raises(ValueError, match="shared= is required"):
        tn.combine(a, b, ab)
    assert tn.combine(a, b, ab, shared=3)["shift"]["dof"] == 3
    with pytest.raises(ValueError, match="not a parameter of both"):
        tn.combine(a, b, ab, shared=["tau"])
    # names on neither side: p0.. or a count
    a, b, ab = three()
    with pytest.raises(ValueError, match="shared= is required"):
        tn.combine(a, b, ab)
    assert tn.combine(a, b, ab, shared=["p2", "p0"])["shift"]["names"] == ["p2", "p0"] and np.array_equal(tn.combine(a, b, ab, shared=["p2", "p0"])["shift"]["delta"], [-0.5, -0.5])


def test_jackknife_sigma_is_the_root_sum_square_and_the_lines():
    sg = dict(a=dict(sigma=([0.3, 0.4], 0.1, 0.5)), b=dict(sigma=([0.4, 0.3], 0.2, 0.6)), ab=dict(sigma=([1.2, 0.0], 0.2, 0.7)))
    a, b, ab = three(**sg)
    t = tn.combine(a, b, ab, shared=3)
    assert set(t["sigma"]) == {"lnR", "lnS", "d"}
    assert np.allclose(t["sigma"]["lnR"], [1.3, 0.5], rtol=1e-15) and abs(t["sigma"]["lnS"] - 0.3) < 1e-15 and abs(t["sigma"]["d"] - math.sqrt(0.25 + 0.36 + 0.49)) < 1e-15
    # without it on one of the three: absent
    a2, b2, ab2 = three(a=sg["a"], b=sg["b"])
    assert "sigma" not in tn.combine(a2, b2, ab2, shared=3)
    out = [ln.strip() for ln in tn.lines(t)]
    assert len(out) == 2 + 4 and out[0].startswith("ln R[k=1] = ") and "±" in out[0] and "ln I[k=1] = " in out[0] and out[1].startswith("ln R[k=2] = ")
    assert out[2].startswith("ln S = ") and "±" in out[2] and out[3].startswith("d = ") and "±" in out[3] and out[4].startswith("p = ") and "sigma = " in out[4]
    assert out[5].startswith("shift (p0, p1, p2): chi2 = ") and "dof = 3" in out[5] and "p = " in out[5] and "sigma = " in out[5]
    assert str(t["lnS"]) in out[2] and str(t["shift"]["chi2"]) in out[5] and str(t["p"]) in out[4]
    plain = tn.lines(tn.combine(*three(), shared=3))
    assert len(plain) == 6 and not any("±" in ln for ln in plain)
    assert "Gaussian" in tn.FOOTNOTE and "independent" in tn.FOOTNOTE


def test_p_and_sigma_against_scipy():
    sp = pytest.importorskip("scipy.special")
    worst = [0.0, 0.0]
    for dof in (0.5, 1.0, 2.0, 3.7, 4.0, 8.0, 27.0, 127.0):
        for chi2 in (1e-3, 0.5, 1.0, 4.0, 9.0, 16.0, 25.0, 60.0, 150.0, 400.0):
            p, want = tn.p_value(dof, chi2), float(sp.gammaincc(0.5 * dof, 0.5 * chi2))
            if want > 1e-300:
                worst[0] = max(worst[0], abs(p - want) / want)
                s, swant = tn.sigma_equivalent(p), -float(sp.ndtri(0.5 * p))
                worst[1] = max(worst[1], abs(s - swant) / max(abs(swant), 1e-300))
    print("p: %.3g relative, sigma_equiv: %.3g relative" % tuple(worst))
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12
    assert tn.p_value(4.0, 0.0) == 1.0 == tn.p_value(4.0, -3.0) and math.isnan(tn.p_value(0.0, 1.0)) and math.isnan(tn.p_value(-1.0, 1.0))
    assert abs(tn.sigma_equivalent(0.31731050786291415) - 1.0) < 1e-12 and abs(tn.sigma_equivalent(2.6997960632601866e-03) - 3.0) < 1e-12 and tn.sigma_equivalent(1.0) == 0.0


# ---- the Gaussian check ----------------------------------------------------------------------------------------------------------
GD, GN = 4, 20000


def gaussian_model():
    """A = N(mu_A, S_A), B = N(mu_B, S_B) with unequal, non-diagonal S; Delta mu such that chi^2_s = 9"""
    rng = np.random.default_rng(99)
    Ma, Mb = rng.standard_normal((GD, GD)), rng.standard_normal((GD, GD))
    Sa = Ma @ Ma.T + 0.5 * np.eye(GD)
    Sb = 0.3 * (Mb @ Mb.T) + np.diag([0.2, 1.0, 0.4, 2.0])
    v = np.array([1.0, -0.5, 0.25, 2.0])
    v *= 3.0 / math.sqrt(float(v @ np.linalg.solve(Sa + Sb, v)))
    mua = np.array([0.3, -1.0, 2.0, 0.0])
    return mua, Sa, mua - v, Sb


def _loglike(x, mu, S):
    r = x - mu
    return -0.5 * np.einsum("ij,ij->i", r, np.linalg.solve(S, r.T).T) - 0.5 * math.log(np.linalg.det(2 * math.pi * S))


def _run_of(x, logL, lnE):
    a = np.ones(len(x))
    info = {"information": inf.build(inf.moments(a, logL - logL.max()), logL.max(), lnE), "covariance": cv.build(cv.measure(a, x))}
    return np.asarray(lnE), info


@pytest.mark.parametrize("seed", range(5))
def test_gaussian_likelihoods_give_their_tension(seed):
    """iid draws of the three Gaussian posteriors, n = 20 000, unit weights, the likelihood column exact.  Analytically ln S = d / 2 -
    chi^2_s / 2 and d = 4, so d - 2 ln S = chi^2_s = 9 and both p are Q(2, 4.5).  Standard errors (docs/design/tension.md):
    ln S: sqrt(3 (d / 2) / n);  d: sqrt(3 (2 d^2 + 12 d) / n);  C_ij: sqrt((S_ii S_jj + S_ij^2) / n);
    chi^2: sqrt((4 chi^2_s + 2 (u'S_A u)^2 + 2 (u'S_B u)^2) / n) with u = (S_A + S_B)^-1 Delta mu."""
    mua, Sa, mub, Sb = gaussian_model()
    Pab = np.linalg.inv(Sa) + np.linalg.inv(Sb)
    Sab = np.linalg.inv(Pab)
    muab = Sab @ (np.linalg.solve(Sa, mua) + np.linalg.solve(Sb, mub))
    dmu = mua - mub
    u = np.linalg.solve(Sa + Sb, dmu)
    chi2_s = float(dmu @ u)
    assert abs(chi2_s - 9.0) < 1e-12
    rng = np.random.default_rng(seed)
    xa, xb, xab = (rng.multivariate_normal(m, S, size=GN, method="cholesky") for m, S in ((mua, Sa), (mub, Sb), (muab, Sab)))
    lnV = 12.0                                             # the flat prior's ln volume: ln E = ln(integral of L) - ln V
    runs = (_run_of(xa, _loglike(xa, mua, Sa), [-lnV]), _run_of(xb, _loglike(xb, mub, Sb), [-lnV]),
            _run_of(xab, _loglike(xab, mua, Sa) + _loglike(xab, mub, Sb),
                    [-0.5 * chi2_s - 0.5 * math.log(np.linalg.det(2 * math.pi * (Sa + Sb))) - lnV]))
    t = tn.combine(*runs, shared=GD)
    se_lnS, se_d = math.sqrt(3 * (GD / 2) / GN), math.sqrt(3 * (2 * GD * GD + 12 * GD) / GN)
    se_chi2 = math.sqrt((4 * chi2_s + 2 * float(u @ Sa @ u) ** 2 + 2 * float(u @ Sb @ u) ** 2) / GN)
    worst = {"lnS": abs(t["lnS"] - (GD / 2 - chi2_s / 2)) / se_lnS, "d": abs(t["d"] - GD) / se_d, "chi2": abs(t["shift"]["chi2"] - chi2_s) / se_chi2, "C": 0.0}
    for r, S in zip(runs, (Sa, Sb, Sab)):
        se = np.sqrt((np.outer(np.diagonal(S), np.diagonal(S)) + S * S) / GN)
        worst["C"] = max(worst["C"], float(np.max(np.abs(r[1]["covariance"]["cov"] - S) / se)))
    print("seed %d: ln S %.2f sigma, d %.2f sigma, shift chi2 %.2f sigma, C entries %.2f sigma;  p %.4f / shift p %.4f (analytic %.4f)" % (
        seed, worst["lnS"], worst["d"], worst["chi2"], worst["C"], t["p"], t["shift"]["p"], tn.p_value(GD, chi2_s)))
    assert all(w <= 5.0 for w in worst.values()), worst
    assert t["status"] == 0 and t["shift"]["status"] == 0 and 0.01 < t["p"] < 0.3 and 0.01 < t["shift"]["p"] < 0.3
    # the identity holds on the measured values too
    assert abs(t["lnR"][0] - t["lnI"][0] - t["lnS"]) <= 8 * EPS * 40.0


# ---- evidence_tension on the host route and the command line --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_roots(tmp_path_factory):
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    d = tmp_path_factory.mktemp("tension_roots")
    out = []
    for name, seed, npar, pnames in (("A", 1, 3, ["om", "h", "a_x"]), ("B", 2, 3, ["om", "h", "b_y"]), ("AB", 3, 4, ["om", "h", "a_x", "b_y"])):
        root = str(d / name)
        chains = [gaussian_chain(seed=10 * seed + i, n=500, d=npar, weights="int") for i in range(2)]
        write_cosmomc_chains(root, chains, [(p, -6.0, 6.0) for p in pnames], fmt="%.17g")
        with open(root + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (p, p) for p in pnames))
        out.append(root)
    return out


def test_evidence_tension_on_the_host_route(three_roots):
    from mcevidence_amd.evidence import MCEvidence
    ea, eb, eab, info = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), jackknife=4)
    assert info["route"] == "host" and len(info["roots"]) == 3 and all("covariance" in i and "information" in i and "jackknife" in i for i in info["roots"])
    t = info["tension"]
    assert t["shift"]["names"] == ["om", "h"] and t["shift"]["dof"] == 2 and len(t["lnR"]) == 2 and "sigma" in t and t["sigma"]["lnR"].shape == (2,)
    own = [MCEvidence(r, kmax=3, verbose=0, backend=OracleBackend(), information=True, covariance=True, jackknife=4).evidence(info=True) for r in three_roots]
    want = tn.combine(*own)
    assert np.array_equal(ea, own[0][0]) and np.array_equal(eab, own[2][0]) and np.array_equal(t["lnR"], want["lnR"]) and t["lnS"] == want["lnS"]
    assert t["shift"]["chi2"] == want["shift"]["chi2"] and np.array_equal(t["sigma"]["lnR"], want["sigma"]["lnR"])
    big = max(max(np.abs(e).max(), abs(i["information"]["mean_logL"]), np.abs(i["information"]["D_KL"]).max()) for e, i in zip((ea, eb, eab), info["roots"]))
    assert np.all(np.abs(t["lnR"] - t["lnI"] - t["lnS"]) <= 8 * EPS * big)
    assert tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), shared=["h"])[3]["tension"]["shift"]["names"] == ["h"]
    with pytest.raises(ValueError, match="route="):
        tn.evidence_tension(*three_roots, route="resident")
    with pytest.raises(ValueError, match="set by evidence_tension"):
        tn.evidence_tension(*three_roots, route="host", covariance=True)


def test_command_line(three_roots, monkeypatch, capsys):
    from mcevidence_amd import cli, evidence
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    monkeypatch.setattr(tn, "evidence_tension", lambda *a, **k: _host(*a, **k))
    p = cli.build_parser()
    assert p.parse_args(["AB", "--tension", "A", "B"]).tension == ["A", "B"] and p.parse_args(["AB"]).tension is None
    ra, rb, rab = three_roots
    got = cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0", "--jackknife=4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert [ln for ln in out if ln.startswith("Using file:")] == ["Using file:  %s" % r for r in (ra, rb, rab)]
    t = got[3]["tension"]
    want = [ln.strip() for ln in tn.lines(t)]
    at = [out.index(ln) for ln in want]
    assert at == sorted(at) and at[0] > max(i for i, ln in enumerate(out) if ln.startswith("ln(B)[k=2]")) and "±" in want[0]
    assert sum(ln.startswith("ln(B)[k=1] =") for ln in out) == 3 and sum(ln.startswith("<ln L> =") for ln in out) == 3
    assert tn.FOOTNOTE in out and out.index(tn.FOOTNOTE) > at[-1] and any(ln.startswith("* ±: delete-a-group jackknife") for ln in out)
    # without --jackknife: no +-
    cli.main([rab, "--tension", ra, rb, "-k", "2", "--allparams", "-vb", "0", "--burn", "0.1", "--thin", "2"])
    out = capsys.readouterr().out
    assert "ln R[k=1] = " in out and "±" not in out and "ln R[k=2]" not in out and tn.FOOTNOTE in out


def test_command_line_combinations(three_roots, monkeypatch, capsys):
    """--cross, --converge and --summary go to all three roots; --farm and --resident are refused"""
    from mcevidence_amd import cli, evidence
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    monkeypatch.setattr(tn, "evidence_tension", lambda *a, **k: _host(*a, **k))
    ra, rb, rab = three_roots
    for flag in ("--farm", "--resident"):
        with pytest.raises(SystemExit) as e:
            cli.main([rab, "--tension", ra, rb, flag])
        assert e.value.code == 2 and "does not combine" in capsys.readouterr().err
    np.random.seed(3)
    got = cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0", "--summary", "0.9", "--converge", "--cross"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert sum(ln.startswith("summary: parameter") for ln in out) == 3 and all("lower90" in ln for ln in out if ln.startswith("summary: parameter"))
    assert all("summary" in i and "converge" in i and i["summary"]["probs"] == (0.9,) for i in got[3]["roots"])
    assert sum("R-1" in ln for ln in out) == 3, out
    assert [i["covariance"]["rows"] for i in got[3]["roots"]] == [500, 500, 500]          # --cross: s1 is half of the 1000 rows
    assert "ln R[k=1] = " in "\n".join(out) and tn.FOOTNOTE in out


def _host(*a, **k):
    k["route"] = "host"
    return _REAL(*a, **k)


_REAL = tn.evidence_tension
