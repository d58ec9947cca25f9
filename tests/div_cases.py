"""Cases, the brute-force deletion model, the high-precision oracle and the bound of the k-NN relative entropy tests
(tests/test_divergence_shared.py on the CPU, tests/test_gpu_divergence.py on the GPU; docs/design/knn_divergence.md).  Tests only; nothing
here is imported by the product.

The model is brute-force DELETION, as in tests/jack_cases.py: for every group b the rows of b are removed from P and from Q, an exact
search is run on what is left (``jack_cases.exact_lists``: distances by direct differences, sorted by (distance, row)) and the formula is
applied in NumPy.  The oracle is mpmath at 60 digits on GIVEN lists and weights.  The bound is the note's, with u = 2^-53 and
gamma(j) = j u / (1 - j u):

    |dN[b][k]| <= gamma(n_b + k + 12) sum a_i (d (|log nu| + |log rho|) + |log MA| + |log MB| + |log(WP_b - a_i)|) + gamma(n) sum a_i
"""
import numpy as np

import jack_cases as jc

U = 2.0 ** -53
SKIP = 255


def gamma(j):
    return j * U / (1.0 - j * U)


def blocks(n, G):
    return (np.arange(n, dtype=np.int64) * G // n).astype(np.int32)


def make_case(nP, nQ, d, seed=1, weights="int"):
    """Gaussian draws (already in the metric the searches use): P standard, Q broader and shifted; integer weights 1..4 or fractional"""
    rng = np.random.default_rng(seed)
    zp = rng.standard_normal((nP, d))
    zq = 0.3 + 1.5 * rng.standard_normal((nQ, d))
    if weights == "int":
        a, b = rng.integers(1, 5, nP).astype(np.float64), rng.integers(1, 5, nQ).astype(np.float64)
    else:
        a, b = rng.uniform(0.25, 1.75, nP), rng.uniform(0.25, 1.75, nQ)
    return dict(zp=np.ascontiguousarray(zp), zq=np.ascontiguousarray(zq), a=a, b=b, d=d)


def planted_case(seed=14):
    """nP = 640, nQ = 720, G = 8 (80 rows of P a group).  Rows 160..199 of P (all of group 2) are a cluster of spread 1e-3 at (2.5, 2.5,
    2.5); rows 10, 330 and 500 (groups 0, 4, 6) sit inside it, so with group 2 deleted their auto lists must reach past 40 cluster rows:
    short at 16 and at 32, not at 128."""
    rng = np.random.default_rng(seed)
    c = make_case(640, 720, 3, seed=seed)
    c["zp"][160:200] = 2.5 + 1e-3 * rng.standard_normal((40, 3))
    for r in (10, 330, 500):
        c["zp"][r] = 2.5 + 1e-3 * rng.standard_normal(3)
    return c


def tie_case(seed=5):
    """nP = 300, nQ = 320, d = 3: exact duplicates inside P (rows 40, 41, 42 equal), inside Q (rows 7, 8 equal) and across (P row 100 ==
    Q row 50; P row 200 == Q rows 60, 61).  Tied rows carry equal weights, so any order among them gives the same masses."""
    c = make_case(300, 320, 3, seed=seed)
    zp, zq, a, b = c["zp"], c["zq"], c["a"], c["b"]
    zp[41] = zp[40]
    zp[42] = zp[40]
    a[40:43] = 2.0
    zq[8] = zq[7]
    b[7:9] = 3.0
    zq[50] = zp[100]
    zq[60] = zp[200]
    zq[61] = zp[200]
    b[60:62] = 1.0
    return c


def lists(zp, zq, L, rows=None, own=True):
    """the model's two lists [nq, L] of the rows ``rows`` of P (None: all): exact, ascending by (distance, row), ended early (distance inf,
    row -1) where a set holds no more rows; ``own``: the own row is left out of the auto list (else it stays in, to be skipped by number)"""
    sel = np.arange(len(zp), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    if own:
        dP, iP = jc.exact_lists(zp[sel], zp, min(L, len(zp) - 1), own=sel)
    else:
        dP, iP = jc.exact_lists(zp[sel], zp, min(L, len(zp)))
    dQ, iQ = jc.exact_lists(zp[sel], zq, min(L, len(zq)))
    return pad(dP, iP, L) + pad(dQ, iQ, L)


def pad(dist, idx, L):
    have = dist.shape[1]
    if have >= L:
        return dist, idx
    return (np.concatenate([dist, np.full((dist.shape[0], L - have), np.inf)], axis=1),
            np.concatenate([idx, np.full((idx.shape[0], L - have), -1, dtype=np.int64)], axis=1))


def min_relative_gap(*dists):
    """the smallest (d[j + 1] - d[j]) / d[j + 1] between consecutive finite distances of any list"""
    best = np.inf
    for dist in dists:
        lo, hi = dist[:, :-1], dist[:, 1:]
        ok = np.isfinite(hi) & (hi > 0)
        if ok.any():
            best = min(best, float(np.min((hi[ok] - lo[ok]) / hi[ok])))
    return best


def deletion_model(c, G, K, gP=None, gQ=None):
    """D[G + 1, K], N[G + 1, K], X[G + 1, K], WPb[G + 1], WQb[G + 1] by deleting every group in turn from P and from Q and searching again"""
    zp, zq, a, b, d = c["zp"], c["zq"], c["a"], c["b"], c["d"]
    gP = (blocks(len(zp), G) if gP is None else gP) if G > 0 else np.full(len(zp), -2)
    gQ = (blocks(len(zq), G) if gQ is None else gQ) if G > 0 else np.full(len(zq), -2)
    N, X, D = np.zeros((G + 1, K)), np.zeros((G + 1, K)), np.full((G + 1, K), np.nan)
    WPb, WQb = np.zeros(G + 1), np.zeros(G + 1)
    for g in range(-1, G):
        ps, qs = np.flatnonzero(gP != g), np.flatnonzero(gQ != g)
        WPb[g + 1], WQb[g + 1] = a[ps].sum(), b[qs].sum()
        if not len(ps):
            continue
        dP, iP = jc.exact_lists(zp[ps], zp[ps], K, own=np.arange(len(ps)))
        dQ, iQ = jc.exact_lists(zp[ps], zq[qs], K)
        MA, MB = np.cumsum(a[ps][iP], axis=1), np.cumsum(b[qs][iQ], axis=1)
        ai = a[ps]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = d * (np.log(dQ) - np.log(dP)) + np.log(MA) - np.log(MB) - np.log(WPb[g + 1] - ai)[:, None]
        zero = (dP == 0.0) | (dQ == 0.0)
        N[g + 1] = np.where(zero, 0.0, ai[:, None] * s).sum(axis=0)
        X[g + 1] = np.where(zero, ai[:, None], 0.0).sum(axis=0)
        D[g + 1] = N[g + 1] / (WPb[g + 1] - X[g + 1]) + np.log(WQb[g + 1])
    return D, N, X, WPb, WQb


def entry_groups(idx, gr, nr, own):
    ok = (idx >= 0) & (idx < nr)
    grp = np.where(ok, 0 if gr is None else np.asarray(gr, dtype=np.int64)[np.where(ok, idx, 0)], SKIP)
    if own is not None:
        grp = np.where(idx == np.asarray(own)[:, None], SKIP, grp)
    return grp


def short_rows(iP, iQ, gq, grP, grQ, G, K, own):
    """positions of the rows either of whose lists runs out for some deleted group other than their own, or for none"""
    ga, gb = entry_groups(iP, grP if G > 0 else None, len(grP), own), entry_groups(iQ, grQ if G > 0 else None, len(grQ), None)
    short = ((ga != SKIP).sum(axis=1) < K) | ((gb != SKIP).sum(axis=1) < K)
    for g in range(G):
        short |= ((((ga != SKIP) & (ga != g)).sum(axis=1) < K) | (((gb != SKIP) & (gb != g)).sum(axis=1) < K)) & (np.asarray(gq) != g)
    return np.flatnonzero(short)


def oracle_sums(dP, iP, dQ, iQ, gq, grP, grQ, G, K, d, aq, aP, bQ, qid=None, skip=()):
    """(N[G + 1, K], X[G + 1, K], bound[G + 1, K]) of GIVEN lists and weights: mpmath at 60 digits, and the note's bound.  ``skip``:
    positions of rows that enter no sum (the short rows)."""
    import mpmath as mp
    mp.mp.dps = 60
    nq, L = dP.shape
    own = np.arange(nq) if qid is None else np.asarray(qid)
    ga = entry_groups(iP, grP if G > 0 else None, len(aP), own)
    gb = entry_groups(iQ, grQ if G > 0 else None, len(bQ), None)
    logs = {}

    def log(x):
        if x not in logs:
            logs[x] = mp.log(x)
        return logs[x]
    wall = mp.fsum(mp.mpf(float(v)) for v in aP)
    wgrp = [mp.fsum(mp.mpf(float(v)) for v in aP[np.asarray(grP) == g]) for g in range(G)]
    N, X, B = np.zeros((G + 1, K)), np.zeros((G + 1, K)), np.zeros((G + 1, K))
    skip = set(int(s) for s in skip)
    for g in range(-1, G):
        wpb = wall if g < 0 else wall - wgrp[g]
        accN, accX = [mp.mpf(0)] * K, [0.0] * K
        accB, accA, nb = [0.0] * K, 0.0, 0
        keepa, keepb = (ga != SKIP) & (ga != g), (gb != SKIP) & (gb != g)
        fa, fb = np.argsort(~keepa, axis=1, kind="stable")[:, :K], np.argsort(~keepb, axis=1, kind="stable")[:, :K]
        for q in range(nq):
            if q in skip or (G > 0 and gq[q] == g):
                continue
            assert keepa[q].sum() >= K and keepb[q].sum() >= K, "row %d is short for group %d" % (q, g)
            nb += 1
            ai = float(aq[q])
            accA += ai
            lw = mp.log(wpb - mp.mpf(ai))
            ja, jb = fa[q], fb[q]
            MA = MB = mp.mpf(0)
            for k in range(K):
                MA += mp.mpf(float(aP[iP[q, ja[k]]]))
                MB += mp.mpf(float(bQ[iQ[q, jb[k]]]))
                rho, nu = float(dP[q, ja[k]]), float(dQ[q, jb[k]])
                if rho == 0.0 or nu == 0.0:
                    accX[k] += ai
                    continue
                lr, ln, lA, lB = log(rho), log(nu), log(MA), log(MB)
                accN[k] += ai * (d * (ln - lr) + lA - lB - lw)
                accB[k] += ai * float(d * (abs(ln) + abs(lr)) + abs(lA) + abs(lB) + abs(lw))
        for k in range(K):
            N[g + 1, k], X[g + 1, k] = float(accN[k]), accX[k]
            B[g + 1, k] = gamma(nb + (k + 1) + 12) * accB[k] + gamma(len(aP)) * accA
    return N, X, B


def assert_sums(got, N, X, B, what=""):
    """the sums [G + 1, K, 2] against the oracle within the bound; X exactly (sums of weights that the cases keep exact)"""
    err = np.abs(got[:, :, 0] - N)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0, err / B, np.where(err == 0, 0.0, np.inf))
    print("%s: largest error over bound of N %.3e (largest bound %.3e)" % (what, ratio.max(), B.max()))
    assert (err <= B).all(), (what, ratio.max())
    assert np.array_equal(got[:, :, 1], X), (what, got[:, :, 1], X)
    return float(ratio.max())


def assert_values(D, sums, model, B, what=""):
    """D[b][k] of one search against the deletion model: both carry the bound of N, the division and the logarithm a few u more"""
    Dm, Nm, Xm, WPb, WQb = model
    tol = 2.0 * B / (WPb[:, None] - Xm) + 8.0 * U * (np.abs(Nm / (WPb[:, None] - Xm)) + np.abs(np.log(WQb))[:, None])
    err = np.abs(D - Dm)
    print("%s: largest |D - D_model| over its bound %.3e" % (what, np.nanmax(err / tol)))
    assert np.array_equal(sums[:, :, 1], Xm), what
    assert (err <= tol).all(), (what, np.nanmax(err / tol))


def write_case(path, dP, iP, dQ, iQ, gq, grP, grQ, G, K, d, aq, aP, bQ, qid=None):
    """the binary case file tests/native/div_check.cpp reads"""
    nq, L = dP.shape
    with open(path, "wb") as f:
        np.array([nq, L, len(aP), len(bQ), G, K, d, 0 if qid is None else 1], dtype=np.int64).tofile(f)
        for arr, dt in ((dP, np.float64), (iP, np.int64), (dQ, np.float64), (iQ, np.int64)):
            np.ascontiguousarray(arr, dtype=dt).tofile(f)
        if qid is not None:
            np.ascontiguousarray(qid, dtype=np.int64).tofile(f)
        if G > 0:
            for g in (gq, grP, grQ):
                np.ascontiguousarray(g, dtype=np.int32).tofile(f)
        for w in (aq, aP, bQ):
            np.ascontiguousarray(w, dtype=np.float64).tofile(f)


def ladder_session(fn, c, gP, gQ, G, K, seen=None):
    """a session for ``divergence.run_ladder`` over the model's lists: ``fn`` is ``divergence.measure`` or has its signature; every
    rung's short rows are checked against ``short_rows`` and noted in ``seen``"""
    n = len(c["zp"])

    class Session(object):
        def level(self, L, rows):
            sel = np.arange(n) if rows is None else np.asarray(rows)
            dP, iP, dQ, iQ = lists(c["zp"], c["zq"], L, rows=rows, own=rows is None)
            gq = None if G == 0 else gP[sel]
            sums, short = fn(dP, iP, dQ, iQ, gq, gP, gQ, G, K, c["d"], c["a"][sel], c["a"], c["b"], qid=None if rows is None else sel)
            want = sel[short_rows(iP, iQ, gq, gP if G > 0 else c["a"], gQ if G > 0 else c["b"], G, K, sel)]
            assert np.asarray(short).tolist() == want.tolist(), (L, short, want)
            if seen is not None:
                seen[L] = want.tolist()
            return sums, short
    return Session()


def read_result(path, G, K):
    vals = open(path).read().split()
    ns = int(vals[0])
    rows = np.array([int(v) for v in vals[1:1 + ns]], dtype=np.int64)
    return np.array([float(v) for v in vals[1 + ns:]]).reshape(G + 1, K, 2), rows
