"""tension on the device routes: ``evidence_tension`` through the farm on three small roots against ``route="host"`` within the
propagated bounds of docs/design/tension.md, with and without ``jackknife``; the command line ``--tension`` prints the same numbers.

The bounds, from the checked quantities: |d ln E| <= LNE_TOL per root (the routes' stated agreement), so |d ln R| <= 3 LNE_TOL;
<ln L> and var(ln L) of every route lie within information.md's bounds b_c (+ eps |<ln L>| for the added logLmax) and b_v of the exact
values, so two routes differ by twice that; ln I = ln R - ln S; the shift's chi^2 = Delta' C^-1 Delta to first order in the bounds of
the means and covariances (cov_cases.bounds), |d chi^2| <= 2 |u|' dDelta + |u|' dC |u| with u = C^-1 Delta, plus 64 eps cond(C) chi^2 for
the two factorisations; p moves by at most |dd| + |dx| (the derivatives of Q(d / 2, x / 2) in d and x are below 1 in magnitude for
d >= 2).  A jackknife sigma is sqrt((G - 1) / G sum (g_b - mean g)^2): if every g_b moves by at most t it moves by at most 2 sqrt(G - 1) t,
and the root-sum-square of three by sqrt(3) times that; a deleted set's moments are held to twice the full set's bounds (its sums are
sub-sums of the full set's, over at least half its weight)."""
import math

import numpy as np
import pytest

import cov_cases as cc
import moments_cases as mc
from helpers import LNE_TOL

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def three_roots(tmp_path_factory):
    """A: 6 parameters, B: 5, AB: 8; the first three are shared; three chains of about a thousand rows each"""
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    d = tmp_path_factory.mktemp("tension_roots")
    names = {"A": ["om", "h", "tau", "a1", "a2", "a3"], "B": ["om", "h", "tau", "b1", "b2"], "AB": ["om", "h", "tau", "a1", "a2", "a3", "b1", "b2"]}
    out = []
    for k, (name, pn) in enumerate(names.items()):
        root = str(d / name)
        chains = []
        for i, n in enumerate((1100, 900, 1000)):
            ch = gaussian_chain(seed=100 * k + i, n=n, d=len(pn), weights="int")
            ch[:, 2:5] += 0.4 * k                          # the shared parameters sit elsewhere in every run
            chains.append(ch)
        write_cosmomc_chains(root, chains, [(p, -8.0, 8.0) for p in pn], fmt="%.17g")
        with open(root + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (p, p) for p in pn))
        out.append(root)
    return out


def _inputs(root, nfiles=3):
    rows = np.concatenate([np.loadtxt(root + "_%d.txt" % i) for i in range(1, nfiles + 1)])
    return rows[:, 0], rows[:, 2:], -rows[:, 1]


@pytest.mark.parametrize("jackknife", [None, 4])
def test_farm_against_the_host_route(three_roots, jackknife):
    from mcevidence_amd import tension as tn
    kw = dict(kmax=3, **({} if jackknife is None else {"jackknife": jackknife}))
    fa, fb, fab, finfo = tn.evidence_tension(*three_roots, route="farm", **kw)
    ha, hb, hab, hinfo = tn.evidence_tension(*three_roots, route="host", **kw)
    assert [i["route"] for i in finfo["roots"]] == ["farm"] * 3 and finfo["route"] == "farm" and hinfo["route"] == "host"
    f, h = finfo["tension"], hinfo["tension"]
    assert set(f) == set(h) and ("sigma" in f) == (jackknife is not None) and f["status"] == h["status"] == 0
    assert f["shift"]["names"] == h["shift"]["names"] == ["om", "h", "tau"] and f["shift"]["status"] == 0
    # the bounds of the three roots
    b_lnS = b_d = 0.0
    covs = []
    for root, hi in zip(three_roots, hinfo["roots"]):
        a, x, logL = _inputs(root)
        ex = mc.exact(a, logL - logL.max())
        b = mc.bounds(ex)
        b_lnS += 2.0 * (b["c"] + EPS * abs(logL.max() + ex["c"]))
        b_d += 2.0 * 2.0 * b["v"]
        covs.append(cc.Case(root, a, x))
    err = {"lnR": float(np.max(np.abs(f["lnR"] - h["lnR"]))) / (3 * LNE_TOL), "lnS": abs(f["lnS"] - h["lnS"]) / b_lnS, "d": abs(f["d"] - h["d"]) / b_d,
           "lnI": float(np.max(np.abs(f["lnI"] - h["lnI"]))) / (3 * LNE_TOL + b_lnS)}
    # the shift: first order in the bounds of the means and the covariances of A and B
    ca, cb = covs[0], covs[1]
    sh = [0, 1, 2]
    C = ca.exact["cov"][np.ix_(sh, sh)] + cb.exact["cov"][np.ix_(sh, sh)]
    delta = ca.exact["mean"][sh] - cb.exact["mean"][sh]
    u = np.abs(np.linalg.solve(C, delta))
    chi2 = float(delta @ np.linalg.solve(C, delta))
    b_chi2 = 2.0 * (2.0 * float(u @ (ca.bound["mean"][sh] + cb.bound["mean"][sh])) + float(u @ (ca.bound["cov"][np.ix_(sh, sh)] + cb.bound["cov"][np.ix_(sh, sh)]) @ u)) \
        + 64 * EPS * np.linalg.cond(C) * chi2
    err["chi2"] = abs(f["shift"]["chi2"] - h["shift"]["chi2"]) / b_chi2
    err["chi2 exact"] = abs(f["shift"]["chi2"] - chi2) / b_chi2
    err["p"] = abs(f["p"] - h["p"]) / (b_d + b_d + 2 * b_lnS)
    err["shift p"] = abs(f["shift"]["p"] - h["shift"]["p"]) / b_chi2
    if jackknife is not None:
        G = 4
        err["sigma lnR"] = float(np.max(np.abs(f["sigma"]["lnR"] - h["sigma"]["lnR"]))) / (2 * math.sqrt(3 * (G - 1)) * LNE_TOL)
        err["sigma lnS"] = abs(f["sigma"]["lnS"] - h["sigma"]["lnS"]) / (2 * math.sqrt(3 * (G - 1)) * 2 * b_lnS)
        err["sigma d"] = abs(f["sigma"]["d"] - h["sigma"]["d"]) / (2 * math.sqrt(3 * (G - 1)) * 2 * b_d)
        assert np.all(f["sigma"]["lnR"] > 0) and f["sigma"]["lnS"] > 0 and f["sigma"]["d"] > 0
    print("jackknife=%s farm against host, difference / bound: %s" % (jackknife, "  ".join("%s %.3g" % kv for kv in err.items())))
    assert all(v <= 1.0 for v in err.values()), err
    for e, g in ((fa, ha), (fb, hb), (fab, hab)):
        assert np.max(np.abs(e - g)) <= LNE_TOL
    # every root's covariance within its bounds of the exact model, and the identity on both routes
    for case, fi in zip(covs, finfo["roots"]):
        cc.check_info(case, fi["covariance"], "farm")
    big = max(max(np.abs(e).max(), abs(i["information"]["mean_logL"]), np.abs(i["information"]["D_KL"]).max()) for e, i in zip((fa, fb, fab), finfo["roots"]))
    assert np.all(np.abs(f["lnR"] - f["lnI"] - f["lnS"]) <= 8 * EPS * big) and np.all(np.abs(h["lnR"] - h["lnI"] - h["lnS"]) <= 8 * EPS * big)
    # the farm's three dicts are the bits of combine on three per-root resident runs
    import mcevidence_amd as pkg
    own = [pkg.evidence_from_files(r, information=True, covariance=True, info=True, verbose=0, require_resident=True, **kw) for r in three_roots]
    t = tn.combine(*own)
    assert np.array_equal(t["lnR"], f["lnR"]) and t["lnS"] == f["lnS"] and t["d"] == f["d"] and t["shift"]["chi2"] == f["shift"]["chi2"] and t["p"] == f["p"]


def test_command_line_prints_the_same_numbers(three_roots, capsys):
    from mcevidence_amd import cli
    from mcevidence_amd import tension as tn
    ra, rb, rab = three_roots
    got = cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0", "--jackknife=4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert [ln for ln in out if ln.startswith("Using file:")] == ["Using file:  %s" % r for r in (ra, rb, rab)]
    want = [ln.strip() for ln in tn.lines(got[3]["tension"])]
    at = [out.index(ln) for ln in want]
    assert at == sorted(at) and "±" in want[0] and tn.FOOTNOTE in out and out.index(tn.FOOTNOTE) > at[-1]
    assert [i["route"] for i in got[3]["roots"]] == ["farm"] * 3
    # the numbers are evidence_tension's own
    pv = [cli.prior.get_prior_volume(cli.build_parser().parse_args([r, "--allparams"]), cosmo=False) for r in (ra, rb, rab)]
    ea, eb, eab, info = tn.evidence_tension(ra, rb, rab, kmax=3, priorvolume=pv, jackknife={"groups": 4, "by": "blocks"})
    assert [ln.strip() for ln in tn.lines(info["tension"])] == want and np.array_equal(eab, got[2])
