"""The k-NN relative entropy on the GPU (docs/design/knn_divergence.md): mce_div_whiten_dev, mce_knn_f64_dev twice and
mce_knn_div_terms_dev through divergence.HipLevels and the ladder, against the mpmath oracle on the device's own lists and against
brute-force DELETION (tests/div_cases.py: delete the group from both chains, search again).  The bound is the note's; general position
(a smallest relative gap of 1e-9 between consecutive list distances) is asserted, so the device's lists and the model's are the same
rows.  Shapes are small on purpose; every case takes a second or two."""
import logging
from fractions import Fraction

import numpy as np
import pytest

import div_cases as dc

pytestmark = pytest.mark.gpu
GAP = 1e-9


@pytest.fixture(scope="module")
def capi():
    from mcevidence_amd import _capi
    _capi.require_device()
    return _capi


def _levels(c, G, K, gP=None, gQ=None):
    import torch
    from mcevidence_amd.divergence import HipLevels
    dev = torch.device("cuda", 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731
    gP = dc.blocks(len(c["zp"]), G) if gP is None and G > 0 else gP
    gQ = dc.blocks(len(c["zq"]), G) if gQ is None and G > 0 else gQ
    return HipLevels(up(c["zp"]), up(c["zq"]), up(c["a"]), up(c["b"]), gP, gQ, G, K), gP, gQ


def _host(t):
    return tuple(None if v is None else v.cpu().numpy() for v in t)


def _against_oracle_and_model(name, c, G, K, gP=None, gQ=None, seen=None):
    """the ladder on the device; its sums against the oracle on the device's own lists of the last rung, which must be the model's rows;
    D[b][k] against the deletion model; every rung's short rows ascending and the model's"""
    from mcevidence_amd import divergence as dv
    s, gP, gQ = _levels(c, G, K, gP, gQ)
    nP, d = len(c["zp"]), c["d"]

    class Checked(object):
        def level(self, L, rows):
            lists = s.lists(L, rows)
            sums, short = s.terms(*lists)
            dP, iP, dQ, iQ, sel = _host(lists)
            sel = np.arange(nP) if sel is None else sel
            gq = None if G == 0 else gP[sel]
            want = sel[dc.short_rows(iP, iQ, gq, gP if G > 0 else c["a"], gQ if G > 0 else c["b"], G, K, sel)]
            assert short.tolist() == want.tolist() == sorted(short.tolist()), (name, L, short, want)
            if seen is not None:
                seen[L] = short.tolist()
            return sums, short
    sums, per_level = dv.run_ladder(Checked(), nP, G, K)
    L = max(per_level)
    dP, iP, dQ, iQ, _ = _host(s.lists(L, None))
    mP, jP, mQ, jQ = dc.lists(c["zp"], c["zq"], L)
    gap = dc.min_relative_gap(mP, mQ)
    print("%s: smallest relative gap %.3g, rows per level %s" % (name, gap, per_level))
    if gap >= GAP:                                          # (the tie case has none: its tied rows carry equal weights instead)
        assert np.array_equal(iP, jP) and np.array_equal(iQ, jQ), name
    N, X, B = dc.oracle_sums(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, c["a"], c["a"], c["b"])
    ratio = dc.assert_sums(sums, N, X, B, what=name)
    wp, wq = dv.masses(c["a"], gP, G), dv.masses(c["b"], gQ, G)
    dc.assert_values(dv.values(sums, wp, wq), sums, dc.deletion_model(c, G, K, gP, gQ), B, what=name)
    return s, sums, per_level, gap, ratio


# ---- A: the smallest shapes at which the kernels can still go wrong ---------------------------------------------------------------
# nP, nQ, d, K, G: one row past a block, a block less one, exactly one, two and a row; a cross set of exactly K rows; one column and 27;
# one rank and sixteen (the 32-entry register form); no groups, two (the ladder's upper rungs), eight and sixty-four
A_CASES = {
    "17x16_d1_K1_G2": (17, 16, 1, 1, 2),
    "17x16_d3_K16_G0": (17, 16, 3, 16, 0),
    "255x300_d3_K1_G64": (255, 300, 3, 1, 64),
    "256x300_d3_K16_G0": (256, 300, 3, 16, 0),
    "257x300_d3_K4_G8": (257, 300, 3, 4, 8),
    "513x700_d27_K4_G2": (513, 700, 27, 4, 2),
}


@pytest.mark.parametrize("name", sorted(A_CASES))
def test_A_sums_against_the_oracle_and_the_deletion_model(capi, name):
    nP, nQ, d, K, G = A_CASES[name]
    c = dc.make_case(nP, nQ, d, seed=1)
    s, sums, per_level, gap, _ = _against_oracle_and_model(name, c, G, K)
    assert gap >= GAP
    # two runs give the same bits
    lists = s.lists(min(per_level), None)
    one, two = s.terms(*lists), s.terms(*lists)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    if name == "257x300_d3_K4_G8":
        # no row is short: the full slot with G = 8 is the G = 0 call, bit for bit
        assert per_level == {16: 257} and len(one[1]) == 0
        s0, _, _ = _levels(c, 0, K)
        full, short = s0.terms(*lists)
        assert len(short) == 0 and np.array_equal(full[0], one[0][0])
    if name == "513x700_d27_K4_G2":
        assert set(per_level) >= {16, 32} and per_level[32] > 0


# ---- B: fractional weights; every status between two good calls ------------------------------------------------------------------
def test_B_fractional_weights(capi):
    c = dc.make_case(300, 257, 3, seed=1, weights="frac")
    _, _, _, gap, _ = _against_oracle_and_model("300x257 fractional", c, 8, 8)
    assert gap >= GAP


def test_B_statuses_between_good_calls(capi, caplog):
    import torch
    from mcevidence_amd import divergence as dv
    c = dc.make_case(257, 300, 3, seed=4, weights="frac")
    dev = torch.device("cuda", 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)          # noqa: E731

    def run(xp=c["zp"], a=c["a"], xq=c["zq"], b=c["b"]):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            out = dv.estimate(up(xp), up(a), up(xq), up(b), kmax=4, groups=8)
        assert len([r for r in caplog.records if "knn divergence: status" in r.getMessage()]) == (1 if out["status"] else 0)
        return out

    def edit(v, i, x):
        v = v.copy()
        v[i] = x
        return v
    good = run()
    assert good["status"] == 0 and np.isfinite(good["D"]).all() and np.isfinite(good["sigma"]).all()
    for kw, want in ((dict(a=edit(c["a"], 100, -0.5)), (3, -1, "P")), (dict(b=edit(c["b"], 299, -0.5)), (3, -1, "Q")),
                     (dict(xp=edit(c["zp"], (256, 1), np.nan)), (4, 1, "P")), (dict(xq=edit(c["zq"], (7, 2), np.nan)), (4, 2, "Q"))):
        bad = run(**kw)
        assert (bad["status"], bad["column"], bad["chain"]) == want and np.isnan(bad["D"]).all() and np.isnan(bad["D_groups"]).all()
        again = run()
        assert all(np.array_equal(good[k], again[k]) for k in ("D", "sigma", "D_groups", "D_bias_corrected", "excluded", "sums")), want
    # a weight of 0 drops its row before anything else
    z = run(a=edit(c["a"], 5, 0.0), xp=edit(c["zp"], (5, 0), np.nan))
    assert z["status"] == 0 and z["rows_p"] == 256


# ---- C: the planted cluster -------------------------------------------------------------------------------------------------------
def test_C_planted_cluster_climbs_the_ladder(capi):
    seen = {}
    _, _, per_level, _, _ = _against_oracle_and_model("planted", dc.planted_case(), 8, 4, seen=seen)
    assert seen == {16: [10, 330, 500], 32: [10, 330, 500], 128: []} and per_level == {16: 640, 32: 3, 128: 3}


# ---- D: ties, and a group with no rows of P -----------------------------------------------------------------------------------------
def test_D_tie_case(capi):
    c = dc.tie_case()
    _, sums, per_level, _, _ = _against_oracle_and_model("ties", c, 4, 3)
    assert per_level == {16: 300}
    assert sums[0, 0, 1] == 6.0 + c["a"][100] + c["a"][200] and sums[0, 1, 1] == 6.0 + c["a"][200] and sums[0, 2, 1] == 0.0


def test_D_group_without_rows_of_P(capi):
    c = dc.make_case(257, 300, 3, seed=6)
    gP = (dc.blocks(257, 3)).astype(np.int32)              # groups 0, 1, 2 of 4: P has no row of group 3
    gQ = dc.blocks(300, 4)
    _, sums, _, gap, _ = _against_oracle_and_model("empty group", c, 4, 4, gP=gP, gQ=gQ)
    assert gap >= GAP and (sums[4, :, 0] != sums[0, :, 0]).all()          # (Q loses its group 3 all the same)


# ---- E: synthetic lists, straight to the host-pointer twin ------------------------------------------------------------------------
def test_E_synthetic_lists(capi):
    from mcevidence_amd import divergence as dv
    c = dc.make_case(300, 320, 3, seed=9)
    G, K, d = 8, 4, 3
    gP, gQ = dc.blocks(300, G), dc.blocks(320, G)
    w = (c["a"], c["a"], c["b"])
    lists16 = dc.lists(c["zp"], c["zq"], 16)
    ref, short = capi.knn_div_terms(*lists16, gP, gP, gQ, G, K, d, *w)
    want, wshort = dv.measure(*lists16, gP, gP, gQ, G, K, d, *w)
    assert short.tolist() == wshort.tolist() == []
    N, X, B = dc.oracle_sums(*lists16, gP, gP, gQ, G, K, d, *w)
    dc.assert_sums(ref, N, X, B, what="synthetic 16")
    # the same entries in lists of 32 (the wider register form) and of 128 (from memory): where no row is short, the same sums
    for L in (32, 128):
        got, short = capi.knn_div_terms(*dc.lists(c["zp"], c["zq"], L), gP, gP, gQ, G, K, d, *w)
        print("L = %d: largest difference from the sums of L = 16: %.3e" % (L, np.max(np.abs(got - ref))))
        assert len(short) == 0 and np.array_equal(got, ref), L
    # a list that ends early: row 7's cross list stops after 3 entries, row 9's auto list holds a row past the set: both short
    dP, iP, dQ, iQ = (v.copy() for v in lists16)
    iQ[7, 3:] = -1
    iP[9, 2:] = 300
    got, short = capi.knn_div_terms(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, *w)
    want, wshort = dv.measure(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, *w)
    assert short.tolist() == wshort.tolist() == [7, 9]
    N, X, B = dc.oracle_sums(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, *w, skip=(7, 9))
    dc.assert_sums(got, N, X, B, what="synthetic, two rows short")
    # qid gathered out of order: lists that keep the own row, which is skipped by its number; the short rows come back by that number
    sel = np.array([250, 3, 299, 17, 128, 64, 0, 200])
    dP, iP, dQ, iQ = dc.lists(c["zp"], c["zq"], 16, rows=sel, own=False)
    assert (iP[:, 0] == sel).all()
    iQ[2, 1:] = -1
    got, short = capi.knn_div_terms(dP, iP, dQ, iQ, gP[sel], gP, gQ, G, K, d, c["a"][sel], c["a"], c["b"], qid=sel)
    want, wshort = dv.measure(dP, iP, dQ, iQ, gP[sel], gP, gQ, G, K, d, c["a"][sel], c["a"], c["b"], qid=sel)
    assert short.tolist() == wshort.tolist() == [299]
    N, X, B = dc.oracle_sums(dP, iP, dQ, iQ, gP[sel], gP, gQ, G, K, d, c["a"][sel], c["a"], c["b"], qid=sel, skip=(2,))
    dc.assert_sums(got, N, X, B, what="synthetic, qid")
    # no groups: the group pointers may be missing
    got, short = capi.knn_div_terms(*lists16, None, None, None, 0, K, d, *w)
    assert len(short) == 0 and np.array_equal(got[0], ref[0])


# ---- F: the whitening ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,ld", [(257, 3, 5), (300, 27, 29), (17, 1, 2)])
def test_F_whitening_against_exact_arithmetic(capi, n, d, ld):
    import torch
    rng = np.random.default_rng(n + d)
    x = rng.standard_normal((n, ld)) * 3.0 + 1.0
    w = rng.uniform(0.25, 1.75, n)
    linv = np.tril(rng.standard_normal((d, d))) + 2.0 * np.eye(d)
    mean = rng.standard_normal(d)
    dev = torch.device("cuda", 0)
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    zd = torch.full((n, d), np.nan, dtype=torch.float64, device=dev)
    wsb = capi.div_whiten_workspace_bytes(n, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    report = capi.div_whiten_dev(xd.data_ptr(), ld, n, d, linv, mean, wd.data_ptr(), zd.data_ptr(), ws.data_ptr(), wsb)
    z = zd.cpu().numpy()
    z2, report2 = capi.div_whiten(x, d, linv, mean, w)
    assert np.array_equal(z, z2) and np.array_equal(report, report2)          # the host twin: the same bits
    assert report[1] == 0.0 and report[2] == -1.0 and report[3] == n and abs(report[0] - w.sum()) <= dc.gamma(n) * w.sum()
    fl, fm = [[Fraction(v) for v in row] for row in linv], [Fraction(v) for v in mean]
    worst = 0.0
    for i in range(n):
        y = [Fraction(x[i, j]) - fm[j] for j in range(d)]
        for k in range(d):
            exact = sum(fl[k][j] * y[j] for j in range(k + 1))
            bound = dc.gamma(d + 2) * float(sum(abs(fl[k][j] * y[j]) for j in range(k + 1)))
            err = abs(float(Fraction(z[i, k]) - exact))
            worst = max(worst, err / bound)
            assert err <= bound, (i, k, err, bound)
    print("whitening %d x %d: largest error over bound %.3f" % (n, d, worst))
    # the report: the lowest column that is not finite, the weights that are not > 0 or not finite, in an order the sizes fix
    xb, wb = x.copy(), w.copy()
    xb[n - 1, d - 1] = np.inf
    xb[0, 0 if d == 1 else 1] = np.nan
    wb[3], wb[n - 2] = 0.0, np.nan
    _, rb = capi.div_whiten(xb, d, linv, mean, wb)
    assert rb[1] == 2.0 and rb[2] == (0.0 if d == 1 else 1.0) and rb[3] == n


# ---- G: estimate, the tension route ------------------------------------------------------------------------------------------------
def test_G_estimate_on_device_tensors_against_measure(capi):
    """raw rows on the device: the result is ``measure`` through the ladder on the whitened rows the library itself produced"""
    import torch
    from mcevidence_amd import covariance as cv
    from mcevidence_amd import divergence as dv
    rng = np.random.default_rng(8)
    nP, nQ, d, K, G = 257, 300, 3, 4, 8
    A = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.2, 1.5]])
    xp = rng.standard_normal((nP, d)) @ A.T + np.array([1.0, -2.0, 0.5])
    xq = 1.4 * rng.standard_normal((nQ, d)) @ A.T + np.array([1.2, -1.8, 0.4])
    a, b = rng.integers(1, 5, nP).astype(float), rng.integers(1, 5, nQ).astype(float)
    dev = torch.device("cuda", 0)
    out = dv.estimate(*(torch.from_numpy(v).to(dev) for v in (xp, a, xq, b)), kmax=K, groups=G, names=["x", "y", "z"])
    host = dv.estimate(xp, a, xq, b, kmax=K, groups=G)          # host arrays are uploaded: the same passes, the same bits
    assert out["status"] == 0 and out["rows_per_level"] == {16: nP} and all(np.array_equal(out[k], host[k]) for k in ("D", "sigma", "D_groups", "sums"))
    cov = cv.from_block(capi.param_cov([(xp, d, a)])[0], d)
    linv = np.tril(np.linalg.solve(np.linalg.cholesky(cov["cov"]), np.eye(d)))
    zp, _ = capi.div_whiten(xp, d, linv, cov["mean"], a)
    zq, _ = capi.div_whiten(xq, d, linv, cov["mean"], b)
    c = dict(zp=zp, zq=zq, a=a, b=b, d=d)
    gP, gQ = dc.blocks(nP, G), dc.blocks(nQ, G)
    lists = dc.lists(zp, zq, 16)
    assert dc.min_relative_gap(lists[0], lists[2]) >= GAP
    want, short = dv.measure(*lists, gP, gP, gQ, G, K, d, a, a, b)
    N, X, B = dc.oracle_sums(*lists, gP, gP, gQ, G, K, d, a, a, b)
    assert len(short) == 0
    dc.assert_sums(out["sums"], N, X, B, what="estimate")
    dc.assert_sums(want, N, X, B, what="measure")
    D = np.vstack([out["D"][None, :], out["D_groups"]])
    dc.assert_values(D, out["sums"], dc.deletion_model(c, G, K), B, what="estimate")
    assert (out["sigma"] > 0).all() and out["names"] == ["x", "y", "z"]


@pytest.fixture(scope="module")
def three_roots(tmp_path_factory):
    """A: 6 parameters, B: 5, AB: 8; the first three are shared; three chains each; A and B of different lengths"""
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    d = tmp_path_factory.mktemp("gain_roots")
    names = {"A": ["om", "h", "tau", "a1", "a2", "a3"], "B": ["om", "h", "tau", "b1", "b2"], "AB": ["om", "h", "tau", "a1", "a2", "a3", "b1", "b2"]}
    out = []
    for k, (name, pn) in enumerate(names.items()):
        root = str(d / name)
        chains = []
        for i, n in enumerate((500 - 60 * k, 450, 400)):
            ch = gaussian_chain(seed=100 * k + i, n=n, d=len(pn), weights="int")
            ch[:, 2:5] += 0.9 * k                          # the shared parameters sit elsewhere in every run
            chains.append(ch)
        write_cosmomc_chains(root, chains, [(p, -9.0, 9.0) for p in pn], fmt="%.17g")
        with open(root + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (p, p) for p in pn))
        out.append(root)
    return out


def _same_dict(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _same_dict(a[k], b[k])
        elif k == "names":
            assert a[k] == b[k]
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_G_evidence_tension_gain_through_the_farm_and_on_the_host(capi, three_roots, capsys):
    from mcevidence_amd import cli
    from mcevidence_amd import divergence as dv
    from mcevidence_amd import tension as tn
    res = {}
    for route in ("farm", "host"):
        plain = tn.evidence_tension(*three_roots, route=route, kmax=3)
        got = tn.evidence_tension(*three_roots, route=route, kmax=3, gain="knn", gain_k=3, gain_groups=4)
        t = dict(got[3]["tension"])
        res[route] = t.pop("gain")
        _same_dict(plain[3]["tension"], t)                       # every number that exists today, bit for bit
        assert all(np.array_equal(x, y) for x, y in zip(plain[:3], got[:3]))          # ln E of the three roots too
    f, h = res["farm"], res["host"]
    names = {"AB|A": ["om", "h", "tau", "a1", "a2", "a3"], "AB|B": ["om", "h", "tau", "b1", "b2"], "A|B": ["om", "h", "tau"], "B|A": ["om", "h", "tau"]}
    rows = [np.concatenate([np.loadtxt(r + "_%d.txt" % i) for i in (1, 2, 3)]) for r in three_roots]
    cols = {"AB|A": (2, [0, 1, 2, 3, 4, 5], 0, [0, 1, 2, 3, 4, 5]), "AB|B": (2, [0, 1, 2, 6, 7], 1, [0, 1, 2, 3, 4]), "A|B": (0, [0, 1, 2], 1, [0, 1, 2]),
            "B|A": (1, [0, 1, 2], 0, [0, 1, 2])}
    for key in tn.GAIN_KEYS:
        assert f[key]["names"] == h[key]["names"] == names[key] and f[key]["status"] == h[key]["status"] == 0 and f[key]["groups"] == 4
        # both routes hand the rows of the same files to the same passes, whose every sum is in an order the sizes fix
        diff = np.max(np.abs(f[key]["D"] - h[key]["D"]))
        print("%s: D = %s ± %s, farm - host %.3e" % (key, f[key]["D"], f[key]["sigma"], diff))
        assert np.array_equal(f[key]["sums"], h[key]["sums"]) and np.array_equal(f[key]["D"], h[key]["D"]) and np.array_equal(f[key]["sigma"], h[key]["sigma"]), key
        # and the files' own rows through the public function give them again
        p, ip, q, iq = cols[key]
        ref = dv.estimate(rows[p][:, [2 + j for j in ip]], rows[p][:, 0], rows[q][:, [2 + j for j in iq]], rows[q][:, 0], kmax=3, groups=4)
        assert np.array_equal(ref["D"], h[key]["D"]) and np.array_equal(ref["sigma"], h[key]["sigma"]), key
    # the shared parameters sit 0.9 apart per run in three directions: A and B differ by far more than their error bars
    assert (f["A|B"]["D"] > 5.0 * f["A|B"]["sigma"]).all() and (f["B|A"]["D"] > 5.0 * f["B|A"]["sigma"]).all()
    ra, rb, rab = three_roots
    capsys.readouterr()
    got = cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0", "--gain-knn", "3", "--gain-groups", "4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    want = [ln.strip() for ln in tn.lines(got[3]["tension"])]
    at = [out.index(ln) for ln in want]
    assert at == sorted(at) and want[-4].startswith("gain D_KL(AB || A) (om, h, tau, a1, a2, a3): [k=1] ") and want[-5].startswith("shift (om, h, tau): chi2 = ")
    assert out.index(tn.FOOTNOTE_GAIN.strip()) == out.index(tn.FOOTNOTE) + 1
    for key in tn.GAIN_KEYS:
        assert np.array_equal(got[3]["tension"]["gain"][key]["D"], f[key]["D"])
    res = cli.main([ra, "--divergence", rb, "3", "--allparams", "-vb", "0", "--gain-groups", "4"])
    text = capsys.readouterr().out
    assert res["names"] == ["om", "h", "tau"] and np.array_equal(res["D"], f["A|B"]["D"])
    assert "D_KL(%s ‖ %s)[k=1] = %s ± %s" % (ra, rb, res["D"][0], res["sigma"][0]) in text
