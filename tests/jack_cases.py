"""Cases and the brute-force deletion model of the jackknife tests (tests/test_jackknife_shared.py on the CPU,
tests/test_gpu_jackknife.py on the GPU).  Tests only; nothing here is imported by the product.

The model is brute-force DELETION: for every group b the rows of b are removed from the queries and from the references, an exact
search is run on what is left (scikit-learn, algorithm="brute") and the sum is formed in NumPy.  scikit-learn's brute search ranks on
GEMM-form squared distances, which carry an absolute error of ~1e-16 |x|^2: inside the 1e-3 cluster of case C that is 1e-9 relative,
far above the n eps bound of the sums.  So the search is asked for MARGIN more rows than needed, the distances of the returned rows
are recomputed by direct differences in fp64 and the list is re-sorted by (distance, row): an exact search unless more than MARGIN
rows tie the K-th to within the GEMM form's error, which none of the cases has.
"""
import math

import numpy as np

MARGIN = 6
EPS = float(np.finfo(np.float64).eps)


def exact_lists(X, Y, L, own=None):
    """the L nearest rows of Y for every row of X, ascending by (exact distance, row); own[q] (or -1): a row of Y left out of q's list"""
    from sklearn.neighbors import NearestNeighbors
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    want = L + (1 if own is not None else 0)
    k = min(want + MARGIN, len(Y))
    _, idx = NearestNeighbors(algorithm="brute").fit(Y).kneighbors(X, n_neighbors=k)
    idx = idx.astype(np.int64)
    diff = X[:, None, :] - Y[idx]
    dist = np.sqrt(np.einsum("qkj,qkj->qk", diff, diff))
    if own is not None:
        dist = np.where(idx == np.asarray(own)[:, None], np.inf, dist)
    order = np.lexsort((idx, dist), axis=1)
    dist, idx = np.take_along_axis(dist, order, axis=1), np.take_along_axis(idx, order, axis=1)
    L = min(L, k - (1 if own is not None else 0))
    assert np.isfinite(dist[:, :L]).all()
    return dist[:, :L], idx[:, :L]


def terms(dist, d, w, fs):
    lnc = 0.5 * d * math.log(math.pi) - math.lgamma(1.0 + 0.5 * d)
    with np.errstate(divide="ignore"):
        return np.sign(w)[:, None] * np.exp((lnc - np.log(np.abs(w)) + fs)[:, None] + d * np.log(dist))


def deletion_model(X, Y, gq, gr, G, k0, kmax, w, fs):
    """(dotp_groups[G, kmax], dotp_full[kmax]) by deleting every group in turn and searching again; Y None: auto evidence"""
    auto = Y is None
    Y = X if auto else Y
    d, K = X.shape[1], kmax - k0
    groups, full = np.zeros((G, kmax)), np.zeros(kmax)
    for b in range(-1, G):
        qs, rs = np.flatnonzero(gq != b), np.flatnonzero(gr != b)
        if not len(qs):
            continue
        own = np.searchsorted(rs, qs) if auto else None          # (auto: gq is gr, so every kept query is a kept reference)
        dist, _ = exact_lists(X[qs], Y[rs], K, own=own)
        (full if b < 0 else groups[b])[k0:] = terms(dist, d, w[qs], fs[qs]).sum(axis=0)
    return groups, full


def short_rows(idx, gq, gr, G, K, own=None):
    """rows whose list ``idx`` (own row left out already, or given) runs out for some deleted group other than their own"""
    grp = np.asarray(gr)[idx]
    valid = np.ones(idx.shape, dtype=bool) if own is None else idx != np.asarray(own)[:, None]
    short = valid.sum(axis=1) < K
    for b in range(G):
        short |= ((valid & (grp != b)).sum(axis=1) < K) & (np.asarray(gq) != b)
    return np.flatnonzero(short)


def lnE_groups(dotp_groups, dotp_full, gq, G, k0, kmax, aw):
    """ln E of the full sample and of every deleted group from the sums, with J = 1, logLmax = 0, prior volume 1"""
    from mcevidence_amd.resident import mle_from_sums
    full = mle_from_sums(dotp_full, 1.0, float(np.sum(aw)), 0.0, len(gq), kmax, 0.0, k0 == 0)[1:]
    per = np.stack([mle_from_sums(dotp_groups[b], 1.0, float(np.sum(aw[gq != b])), 0.0, int((gq != b).sum()), kmax, 0.0, k0 == 0)[1:] for b in range(G)])
    return full, per


def blocks(n, G):
    return (np.arange(n, dtype=np.int64) * G // n).astype(np.int32)


def _finish(X, G, kmax, seed, w=None, Y=None, gq=None, gr=None):
    rng = np.random.default_rng(seed + 1000)
    n = len(X)
    w = rng.integers(1, 4, n).astype(np.float64) if w is None else w
    fs = -0.5 * np.einsum("ij,ij->i", X, X)
    fs = fs - fs.max()
    gq = blocks(n, G) if gq is None else gq
    return dict(X=np.ascontiguousarray(X), Y=Y, w=w, fs=fs, gq=gq, gr=gq if gr is None else gr, G=G, kmax=kmax, k0=1 if Y is None else 0, d=X.shape[1])


def case_iid(n=600, d=3, G=8, kmax=5, seed=11):
    """A: iid rows, integer weights 1..3"""
    return _finish(np.random.default_rng(seed).standard_normal((n, d)), G, kmax, seed)


def ar1_rows(n, d, phi, step, seed):
    rng = np.random.default_rng(seed)
    X = np.zeros((n, d))
    e = step * rng.standard_normal((n, d))
    for i in range(1, n):
        X[i] = phi * X[i - 1] + e[i]
    return X


def case_walk(n=600, d=3, G=8, kmax=5, seed=12):
    """B: an AR(1) walk (phi = 0.95, step 0.1): neighbours in space are neighbours in time, i.e. in group"""
    return _finish(ar1_rows(n, d, 0.95, 0.1, seed), G, kmax, seed)


def case_planted(seed=14):
    """C: n = 640, G = 8 (80 rows a group).  Rows 160..199 (all of group 2) are a cluster of spread 1e-3 at (2.5, 2.5, 2.5); rows 10,
    330 and 500 (groups 0, 4, 6) sit inside it, so with group 2 deleted their lists must reach past 40 cluster rows; an exact
    duplicate pair inside one group (400, 401) and one across groups (90, 410)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((640, 3))
    X[160:200] = 2.5 + 1e-3 * rng.standard_normal((40, 3))
    for r in (10, 330, 500):
        X[r] = 2.5 + 1e-3 * rng.standard_normal(3)
    X[401] = X[400]
    X[410] = X[90]
    return _finish(X, 8, 5, seed)


def case_capacity(seed=14):
    """I: G = 2, n = 3000, groups by row parity; rows 100..1199 (all put into group 0) are near-identical at (9, 9, 9), row 2000 (put
    into group 1) sits at their centre: with group 0 deleted its list must reach past 1100 rows, more than the last rung holds"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3000, 3))
    X[100:1200] = 9.0 + 1e-6 * rng.standard_normal((1100, 3))
    X[2000] = 9.0
    g = (np.arange(3000) % 2).astype(np.int32)
    g[100:1200] = 0
    g[2000] = 1
    return _finish(X, 2, 5, seed, gq=g)


def case_cross(n1=500, n2=700, d=4, G=8, kmax=4, seed=15, empty_group=None):
    """G / E: cross evidence of a shuffled s1 against s2, both cut from one chain of n1 + n2 rows; ``empty_group``: s1 takes no row of it"""
    rng = np.random.default_rng(seed)
    n = n1 + n2
    Z = rng.standard_normal((n, d))
    g = blocks(n, G)
    pool = np.arange(n) if empty_group is None else np.flatnonzero(g != empty_group)
    r1 = rng.permutation(pool)[:n1]
    r2 = np.setdiff1d(np.arange(n), r1)
    c = _finish(Z[r1], G, kmax, seed, Y=np.ascontiguousarray(Z[r2]), gq=g[r1], gr=g[r2])
    c["rows"] = (r1, r2, Z)
    return c


def write_case(path, dist, idx, c, qid=None):
    """the binary case file tests/native/jack_check.cpp reads"""
    nq, L = dist.shape
    with open(path, "wb") as f:
        np.array([nq, L, len(c["gr"]), c["G"], c["k0"], c["kmax"], c["d"], 0 if qid is None else 1], dtype=np.int64).tofile(f)
        np.ascontiguousarray(dist, dtype=np.float64).tofile(f)
        np.ascontiguousarray(idx, dtype=np.int64).tofile(f)
        if qid is not None:
            np.ascontiguousarray(qid, dtype=np.int64).tofile(f)
        gq, w, fs = (c["gq"], c["w"], c["fs"]) if qid is None else (c["gq"][qid], c["w"][qid], c["fs"][qid])
        np.ascontiguousarray(gq, dtype=np.int32).tofile(f)
        np.ascontiguousarray(c["gr"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(w, dtype=np.float64).tofile(f)
        np.ascontiguousarray(fs, dtype=np.float64).tofile(f)


def read_result(path, G, kmax):
    vals = open(path).read().split()
    ns = int(vals[0])
    rows = np.array([int(v) for v in vals[1:1 + ns]], dtype=np.int64)
    nums = np.array([float(v) for v in vals[1 + ns:]])
    return nums[:G * kmax].reshape(G, kmax), nums[G * kmax:], rows


def assert_sums(got_groups, got_full, want_groups, want_full, n, k0, what=""):
    """the bound of the sums: n eps relative (sums of n same-signed terms), every column from k0 on"""
    for got, want in ((got_groups, want_groups), (got_full, want_full)):
        g, w = np.asarray(got)[..., k0:], np.asarray(want)[..., k0:]
        rel = np.abs(g - w) / np.abs(w)
        print("%s sums: max relative difference %.3e (bound %.3e)" % (what, rel.max(), n * EPS))
        assert (rel <= n * EPS).all(), (what, rel.max(), n * EPS)
