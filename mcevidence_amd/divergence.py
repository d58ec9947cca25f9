"""``gain="knn"``: the relative entropy D_KL(P || Q) between two chains -- how much run P learnt beyond run Q -- from nearest-neighbour
distances (Wang, Kulkarni & Verdu 2009; Perez-Cruz 2008), with a delete-a-group jackknife error bar from ONE pair of neighbour searches
(docs/design/knn_divergence.md).  It needs no likelihood column and no prior volume.

The rule (csrc/knn_div.hpp), all in fp64.  P = (xp[nP, d], a[nP]) and Q = (xq[nQ, d], b[nQ]) are rows in the same d columns with their
weights; rows with weight 0 are dropped first.

    metric    W_P, the mean m and the covariance C of P (``covariance``'s rule);  L = cholesky(C);  both chains:  z = L^-1 (x - m)
    lists     for every P row i two ascending lists (distance, row): its neighbours among the OTHER P rows, and its neighbours in Q
    terms     b the deleted group (-1: none), a row i with gP[i] != b, a rank k = 1 .. K, entries of group b skipped in both lists:
              rho, MA = the distance of the k-th kept auto entry, the sum of the weights a of the first k kept auto entries (list order)
              nu,  MB = the same of the cross list with the weights b
              s = d (log nu - log rho) + log MA - log MB - log(WP_b - a_i),    WP_b = W_P - (the weight of P's group b)
    sums      N[b][k] = sum a_i s;   X[b][k] = sum a_i over rows with rho == 0 or nu == 0 (coincident rows enter X and not N)
              D[b][k] = N[b][k] / (WP_b - X[b][k]) + log WQ_b
    results   D[k] = D[-1][k],  sigma[k] = the jackknife sigma over the G values D[b][k],  D_bias_corrected[k] (reported, never
              substituted),  excluded[k] = X[-1][k] / W_P

With unit weights and no group deleted this is Wang et al.'s (d / n) sum ln(nu_k / rho_k) + ln(m / (n - 1)).  A row is SHORT when skipping
some group other than its own (or none) leaves fewer than K entries in either list: it enters no sum at that rung and is searched again
with longer lists (``ladder``: 16 -- 32 when K + 8 > 16 --, 32, 128, then a ``ValueError``).  The jackknife is conditional on the full
sample's metric.

status 3: a weight is not > 0 or not finite; 4: a value is not finite (``column``: the lowest such, ``chain``: "P" or "Q"); 6: fewer than
K + 1 rows are left in P, or fewer than K in Q, for some deleted group; 7: C is not positive definite.  They are found in the order the
passes run: P's weights, P's values, the row counts, the factorisation, Q's weights, Q's values.  A status other than 0 makes every value
NaN, logs one WARNING and raises nothing.

``measure`` is the rule in NumPy from lists (the route without a device and the model of the tests), ``group_ids`` the groups,
``summarise`` the values from the sums, ``estimate`` the whole of it, ``lines`` prints it.
"""
from __future__ import annotations

import logging
import math

import numpy as np

from . import covariance as _cov

logger = logging.getLogger("mcevidence_amd")

__all__ = ["measure", "group_ids", "masses", "summarise", "lines", "estimate", "ladder", "whiten", "LADDER", "STATUS_WORDS", "MAX_K", "MAX_DIM", "MAX_GROUPS"]

OK, BAD_WEIGHT, BAD_VALUE, FEW_ROWS, NOT_POSITIVE = 0, 3, 4, 6, 7
STATUS_WORDS = {
    OK: "ok",
    BAD_WEIGHT: "a weight is not > 0 or not finite",
    BAD_VALUE: "a row has a parameter value that is not finite",
    FEW_ROWS: "fewer than K + 1 rows of P or fewer than K rows of Q are left for some deleted group",
    NOT_POSITIVE: "the covariance of P is not positive definite",
}
LADDER = (16, 32, 128)
MAX_K = 16               # == MCE_DIV_MAX_K
MAX_DIM = 64             # == MCE_DIV_MAX_DIM
MAX_GROUPS = 64          # == MCE_JACK_MAX_GROUPS
SKIP = 255               # csrc/jack.hpp: kJackSkip
MARGIN = 6               # host lists: rows asked of the GEMM-form search beyond those wanted, before the exact re-sort


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def ladder(K):
    """the list lengths tried, in order: 16 (when K + 8 <= 16, else 32) -> 32 -> 128"""
    first = LADDER[0] if K + 8 <= LADDER[0] else LADDER[1]
    return tuple(L for L in LADDER if L >= first)


def _check_args(K, G):
    if not 1 <= int(K) <= MAX_K:
        raise ValueError("knn divergence: K=%r ranks (1 .. %d expected)" % (K, MAX_K))
    if int(G) != 0 and not 2 <= int(G) <= MAX_GROUPS:
        raise ValueError("knn divergence: G=%r groups (0, or 2 .. %d expected)" % (G, MAX_GROUPS))


def group_ids(n, groups):
    """by="blocks": int32 group ``row * groups // n`` of every row of a chain of ``n`` rows (each chain on its own)"""
    return (np.arange(int(n), dtype=np.int64) * int(groups) // max(int(n), 1)).astype(np.int32)


def masses(w, g, G):
    """[G + 1]: the sum of ``w``, then the sum over the rows of every group"""
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros(int(G) + 1)
    out[0] = float(np.sum(w))
    if G > 0:
        out[1:] = np.bincount(np.asarray(g, dtype=np.int64), weights=w, minlength=int(G))[:int(G)]
    return out


def _entry_groups(idx, gr, nr, own):
    """the group every list entry counts under: its row's (0 where there are no groups), or SKIP for a missing entry and the own row"""
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < nr)
    grp = np.where(ok, 0 if gr is None else np.asarray(gr, dtype=np.int64)[np.where(ok, idx, 0)], SKIP)
    if own is not None:
        grp = np.where(idx == own[:, None], SKIP, grp)
    return grp


def measure(distP, idxP, distQ, idxQ, gq, grP, grQ, G, K, d, aq, aP, bQ, qid=None):
    """The sums from ascending neighbour lists [nq, L] in NumPy -- the rule of csrc/knn_div.hpp.  ``distP`` / ``idxP``: the auto lists
    (neighbours in P; the own row -- ``qid[q]``, or q -- is skipped where a list holds it), ``distQ`` / ``idxQ``: the cross lists; ``gq`` [nq],
    ``grP`` [nP], ``grQ`` [nQ] the groups (ignored where ``G`` is 0); ``aq`` [nq], ``aP`` [nP], ``bQ`` [nQ] the weights.  Returns
    (sums[G + 1, K, 2] -- slot 0 the full sample, slot 1 + b group b deleted; N and X --, short_rows ascending int64)."""
    G, K = int(G), int(K)
    _check_args(K, G)
    distP, distQ = np.asarray(distP, dtype=np.float64), np.asarray(distQ, dtype=np.float64)
    aq, aP, bQ = (np.asarray(v, dtype=np.float64) for v in (aq, aP, bQ))
    nq, L = distP.shape
    if L < K:
        raise ValueError("knn divergence: lists of L=%d entries are shorter than the K=%d ranks of the sums" % (L, K))
    if G > 0:
        gq, grP, grQ = (np.asarray(g, dtype=np.int32) for g in (gq, grP, grQ))
        for g in (gq, grP, grQ):
            if len(g) and (g.min() < 0 or g.max() >= G):
                raise ValueError("knn divergence: a group id outside 0 .. %d" % (G - 1))
    else:
        gq, grP, grQ = np.full(nq, -2, dtype=np.int32), None, None
    own = np.arange(nq, dtype=np.int64) if qid is None else np.asarray(qid, dtype=np.int64)
    ga, gb = _entry_groups(idxP, grP, len(aP), own), _entry_groups(idxQ, grQ, len(bQ), None)
    keep = {b: ((ga != SKIP) & (ga != b), (gb != SKIP) & (gb != b)) for b in range(-1, G)}
    short = (keep[-1][0].sum(axis=1) < K) | (keep[-1][1].sum(axis=1) < K)
    for b in range(G):
        short |= ((keep[b][0].sum(axis=1) < K) | (keep[b][1].sum(axis=1) < K)) & (gq != b)
    wp = masses(aP, grP, G)
    idxP, idxQ = np.asarray(idxP, dtype=np.int64), np.asarray(idxQ, dtype=np.int64)
    sums = np.zeros((G + 1, K, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        lP, lQ = np.log(distP), np.log(distQ)
        for b in range(-1, G):
            rows = np.flatnonzero(~short & (gq != b))
            if not len(rows):
                continue
            fa = np.argsort(~keep[b][0][rows], axis=1, kind="stable")[:, :K]       # positions of the first K kept entries, ascending
            fb = np.argsort(~keep[b][1][rows], axis=1, kind="stable")[:, :K]
            lrho, lnu = np.take_along_axis(lP[rows], fa, axis=1), np.take_along_axis(lQ[rows], fb, axis=1)
            MA = np.cumsum(aP[np.take_along_axis(idxP[rows], fa, axis=1)], axis=1)
            MB = np.cumsum(bQ[np.take_along_axis(idxQ[rows], fb, axis=1)], axis=1)
            ai = aq[rows]
            lw = np.log((wp[0] if b < 0 else wp[0] - wp[1 + b]) - ai)
            s = d * (lnu - lrho) + np.log(MA) - np.log(MB) - lw[:, None]
            zero = np.isneginf(lrho) | np.isneginf(lnu)
            sums[b + 1, :, 0] = np.where(zero, 0.0, ai[:, None] * s).sum(axis=0)
            sums[b + 1, :, 1] = np.where(zero, ai[:, None], 0.0).sum(axis=0)
    return sums, own[short]


def values(sums, wp, wq):
    """D[G + 1, K] from the sums and the masses of P and Q ([G + 1] each: the whole, then the groups)"""
    sums, wp, wq = np.asarray(sums, dtype=np.float64), np.asarray(wp, dtype=np.float64), np.asarray(wq, dtype=np.float64)
    wpb = np.concatenate(([wp[0]], wp[0] - wp[1:]))
    wqb = np.concatenate(([wq[0]], wq[0] - wq[1:]))
    with np.errstate(all="ignore"):
        return sums[:, :, 0] / (wpb[:, None] - sums[:, :, 1]) + np.log(wqb)[:, None]


def summarise(sums, wp, wq):
    """dict(D[K], sigma[K], D_bias_corrected[K], D_groups[G, K], excluded[K]) from the sums [G + 1, K, 2] and the masses: sigma =
    sqrt((G - 1) / G sum_b (D_b - mean_b D_b)^2), bias-corrected = G D - (G - 1) mean_b D_b; NaN where there are no groups"""
    D = values(sums, wp, wq)
    G, K = D.shape[0] - 1, D.shape[1]
    out = {"D": D[0].copy(), "D_groups": D[1:].copy(), "sigma": np.full(K, np.nan), "D_bias_corrected": np.full(K, np.nan),
           "excluded": np.asarray(sums, dtype=np.float64)[0, :, 1] / float(np.asarray(wp)[0])}
    if G > 0:
        mean = D[1:].mean(axis=0)
        out["sigma"] = np.sqrt((G - 1.0) / G * ((D[1:] - mean) ** 2).sum(axis=0))
        out["D_bias_corrected"] = G * D[0] - (G - 1.0) * mean
    return out


def whiten(x, linv, mean):
    """z_k = sum_{j <= k} linv_kj (x_j - mean_j): plain products and sums in column order"""
    y = np.asarray(x, dtype=np.float64) - np.asarray(mean, dtype=np.float64)[None, :]
    z = np.zeros_like(y)
    for k in range(y.shape[1]):
        acc = np.zeros(y.shape[0])
        for j in range(k + 1):
            acc = acc + linv[k, j] * y[:, j]
        z[:, k] = acc
    return z


def _pad(dist, idx, L, np_like):
    """lists of fewer than L entries (a set that holds no more rows) end early: distance inf, row -1"""
    have = int(dist.shape[1])
    if have == L:
        return dist, idx
    if np_like:
        return (np.concatenate([dist, np.full((dist.shape[0], L - have), np.inf)], axis=1),
                np.concatenate([idx, np.full((idx.shape[0], L - have), -1, dtype=np.int64)], axis=1))
    import torch
    return (torch.cat([dist, torch.full((dist.shape[0], L - have), math.inf, dtype=dist.dtype, device=dist.device)], dim=1).contiguous(),
            torch.cat([idx, torch.full((idx.shape[0], L - have), -1, dtype=idx.dtype, device=idx.device)], dim=1).contiguous())


def host_lists(X, Y, L, own=None):
    """the min(L, rows of Y) nearest rows of Y for every row of X, ascending by (distance, row), the distances by direct differences
    (scikit-learn's brute search ranks on GEMM-form squared distances: MARGIN more rows are asked for and the list is sorted again);
    own[q]: a row of Y left out of q's list"""
    from sklearn.neighbors import NearestNeighbors
    X, Y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64)
    extra = 1 if own is not None else 0
    k = min(L + extra + MARGIN, len(Y))
    idx = NearestNeighbors(algorithm="brute").fit(Y).kneighbors(X, n_neighbors=k, return_distance=False).astype(np.int64)
    dist = np.empty(idx.shape)
    step = max(1, (64 << 20) // (8 * k * X.shape[1]))
    for i0 in range(0, len(X), step):
        diff = X[i0:i0 + step, None, :] - Y[idx[i0:i0 + step]]
        dist[i0:i0 + step] = np.sqrt(np.einsum("qkj,qkj->qk", diff, diff))
    if own is not None:
        dist = np.where(idx == np.asarray(own)[:, None], np.inf, dist)
    order = np.lexsort((idx, dist), axis=1)
    dist, idx = np.take_along_axis(dist, order, axis=1), np.take_along_axis(idx, order, axis=1)
    keep = min(L, len(Y) - extra)
    return np.ascontiguousarray(dist[:, :keep]), np.ascontiguousarray(idx[:, :keep])


class HostLevels(object):
    """a rung on the host: scikit-learn lists and ``measure``.  The first rung leaves the own row out of the auto list; the upper rungs
    search the rows still short without excluding anything and skip the own row by its number, as the device's do."""

    def __init__(self, zp, zq, a, b, gP, gQ, G, K):
        self.zp, self.zq, self.a, self.b, self.gP, self.gQ, self.G, self.K = zp, zq, a, b, gP, gQ, G, K

    def level(self, L, rows):
        nP = len(self.zp)
        if rows is None:
            sel = np.arange(nP, dtype=np.int64)
            dP, iP = host_lists(self.zp, self.zp, L, own=sel)
        else:
            sel = np.asarray(rows, dtype=np.int64)
            dP, iP = host_lists(self.zp[sel], self.zp, L)
        dQ, iQ = host_lists(self.zp[sel], self.zq, L)
        dP, iP = _pad(dP, iP, L, True)
        dQ, iQ = _pad(dQ, iQ, L, True)
        gq = None if self.G == 0 else self.gP[sel]
        return measure(dP, iP, dQ, iQ, gq, self.gP, self.gQ, self.G, self.K, self.zp.shape[1], self.a[sel], self.a, self.b, qid=sel)


class HipLevels(object):
    """a rung on the device: ``mce_knn_f64_dev`` twice and ``mce_knn_div_terms_dev``; the whitened rows, the weights and the groups are
    device tensors and stay where they are"""

    def __init__(self, zp, zq, a, b, gP, gQ, G, K):
        import torch
        from . import _capi
        self.torch, self.capi = torch, _capi
        self.zp, self.zq, self.a, self.b, self.G, self.K = zp, zq, a, b, G, K
        self.dev = zp.device
        self.gP = None if G == 0 else torch.from_numpy(np.ascontiguousarray(gP, dtype=np.int32)).to(self.dev)
        self.gQ = None if G == 0 else torch.from_numpy(np.ascontiguousarray(gQ, dtype=np.int32)).to(self.dev)
        self.kernel_ms = []

    def _search(self, Xq, Y, L, self_mode):
        torch, capi = self.torch, self.capi
        nq, nr, d = int(Xq.shape[0]), int(Y.shape[0]), int(Y.shape[1])
        dist = torch.empty((nq, L), dtype=torch.float64, device=self.dev)
        idx = torch.empty((nq, L), dtype=torch.int64, device=self.dev)
        wsb = capi.knn_workspace_bytes(nq, nr, d, L)
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
        stream = torch.cuda.current_stream().cuda_stream
        capi.knn_dev(Xq.data_ptr(), nq, Y.data_ptr(), nr, d, L, self_mode, 0, dist.data_ptr(), idx.data_ptr(), ws.data_ptr(), wsb, stream)
        torch.cuda.current_stream().synchronize()
        return dist, idx

    def lists(self, L, rows):
        """(distP, idxP, distQ, idxQ [nq, L], sel) on the device: the first rung (``rows`` None) leaves the own row out in the search; an
        upper rung searches the rows ``rows`` without excluding anything (``sel``: their numbers, by which the terms skip the own row).
        A search never asks for more rows than the set holds: such lists end early."""
        torch, capi = self.torch, self.capi
        nP, nQ = int(self.zp.shape[0]), int(self.zq.shape[0])
        with torch.cuda.device(self.dev):
            if rows is None:
                sel, Xq = None, self.zp
                dP, iP = self._search(Xq, self.zp, min(L, nP - 1), capi.SELF_EXCLUDE)
            else:
                sel = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.dev)
                Xq = self.zp.index_select(0, sel).contiguous()
                dP, iP = self._search(Xq, self.zp, min(L, nP), capi.SELF_NONE)
            dQ, iQ = self._search(Xq, self.zq, min(L, nQ), capi.SELF_NONE)
            return _pad(dP, iP, L, False) + _pad(dQ, iQ, L, False) + (sel,)

    def level(self, L, rows):
        return self.terms(*self.lists(L, rows))

    def terms(self, dP, iP, dQ, iQ, sel):
        """``mce_knn_div_terms_dev`` on lists that are on the device -> (sums[G + 1, K, 2], short rows) on the host"""
        torch, capi = self.torch, self.capi
        nP, nQ, d, L = int(self.zp.shape[0]), int(self.zq.shape[0]), int(self.zp.shape[1]), int(dP.shape[1])
        with torch.cuda.device(self.dev):
            aq = self.a if sel is None else self.a.index_select(0, sel)
            gq = None if self.G == 0 else (self.gP if sel is None else self.gP.index_select(0, sel))
            nq = int(dP.shape[0])
            sums = torch.empty((self.G + 1, self.K, 2), dtype=torch.float64, device=self.dev)
            short = torch.empty(nq, dtype=torch.int64, device=self.dev)
            nshort = torch.zeros(1, dtype=torch.int64, device=self.dev)
            wsb = capi.knn_div_workspace_bytes(nq, nP, self.G, self.K)
            ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            ptr = lambda t: 0 if t is None else t.data_ptr()          # noqa: E731
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.current_stream()
            t0.record(stream)
            capi.knn_div_terms_dev(dP.data_ptr(), iP.data_ptr(), dQ.data_ptr(), iQ.data_ptr(), nq, L, ptr(sel), ptr(gq), ptr(self.gP), nP, ptr(self.gQ), nQ,
                                   self.G, self.K, d, aq.data_ptr(), self.a.data_ptr(), self.b.data_ptr(), sums.data_ptr(), short.data_ptr(),
                                   nshort.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream)
            t1.record(stream)
            stream.synchronize()
            self.kernel_ms.append(float(t0.elapsed_time(t1)))
            ns = int(nshort.item())
            return sums.cpu().numpy(), short[:ns].cpu().numpy()


def run_ladder(session, nP, G, K):
    """every row at the first rung, the rows still short at the next; the level sums are added in level order.  Returns (sums,
    rows_per_level {L: rows searched at that rung})."""
    sums, rows, per_level = np.zeros((G + 1, K, 2)), None, {}
    for L in ladder(K):
        per_level[L] = int(nP if rows is None else len(rows))
        s, short = session.level(L, rows)
        sums += s
        rows = np.asarray(short, dtype=np.int64)
        if not len(rows):
            return sums, per_level
    raise ValueError("knn divergence: %d row%s still short after lists of %d neighbours -- some group fills their whole neighbourhood; use fewer "
                     "groups or thin the chains more" % (len(rows), "" if len(rows) == 1 else "s", LADDER[-1]))


def _result(names, d, K, G, nP, nQ, status=OK, column=-1, chain=None):
    nan = np.full(K, np.nan)
    return {"names": list(names) if names is not None else ["p%d" % j for j in range(d)], "D": nan.copy(), "sigma": nan.copy(),
            "D_bias_corrected": nan.copy(), "D_groups": np.full((G, K), np.nan), "excluded": nan.copy(), "rows_per_level": {}, "groups": G, "kmax": K,
            "rows_p": int(nP), "rows_q": int(nQ), "dof": int(d), "status": int(status), "column": int(column), "chain": chain}


def _fail(out, status, column=-1, chain=None):
    out["status"], out["column"], out["chain"] = int(status), int(column), chain
    where = "" if chain is None else " in %s%s" % (chain, "" if column < 0 else ", column %d" % column)
    logger.warning("knn divergence: status %d (%s%s): every value is NaN" % (status, STATUS_WORDS[status], where))
    return out


def _factor(cov):
    """(linv, mean) from ``covariance``'s dict, or None where C is not positive definite"""
    d = len(cov["mean"])
    try:
        L = np.linalg.cholesky(np.asarray(cov["cov"], dtype=np.float64))
        linv = np.linalg.solve(L, np.eye(d))
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(linv).all():
        return None
    return np.tril(linv), np.asarray(cov["mean"], dtype=np.float64)


def _native_default():
    try:
        from . import _capi
        return _capi.device_count() > 0
    except Exception:
        return False


def estimate(xp, a, xq, b, kmax=4, groups=8, device=None, names=None, native=None):
    """D_KL(P || Q)[k], k = 1 .. ``kmax``, of two runs' rows in their shared columns -- ``xp`` [nP, d] with weights ``a``, ``xq`` [nQ, d] with
    weights ``b``: NumPy arrays or torch tensors of one device -- with a delete-a-block jackknife over ``groups`` blocks of each chain
    (0: none).  ``native`` (None: whether a device is visible; torch tensors: always): the covariance, the whitening, the searches and the
    sums by the library, one rung at a time (``mce_param_cov_dev``, ``mce_div_whiten_dev``, then per rung ``mce_knn_f64_dev`` twice and
    ``mce_knn_div_terms_dev``); otherwise scikit-learn lists and ``measure``.  -> dict(names, D[k], sigma[k], D_bias_corrected[k],
    D_groups[G, k], excluded[k], rows_per_level, groups, kmax, rows_p, rows_q, dof, status, column, chain)."""
    K, G = int(kmax), int(groups)
    _check_args(K, G)
    tensor = _is_tensor(xp)
    if tensor != _is_tensor(xq) or tensor != _is_tensor(a) or tensor != _is_tensor(b):
        raise ValueError("knn divergence: rows and weights as NumPy arrays, or as torch tensors of one device")
    if xp.ndim != 2 or xq.ndim != 2 or xp.shape[1] != xq.shape[1] or xp.shape[0] != a.shape[0] or xq.shape[0] != b.shape[0]:
        raise ValueError("knn divergence: rows of %s and %s with %d and %d weights" % (tuple(xp.shape), tuple(xq.shape), a.shape[0], b.shape[0]))
    d = int(xp.shape[1])
    if not 1 <= d <= MAX_DIM:
        raise ValueError("knn divergence: %d shared parameters (1 .. %d expected)" % (d, MAX_DIM))
    native = (tensor or _native_default()) if native is None else bool(native)
    if tensor and not native:
        xp, a, xq, b = (v.cpu().numpy() for v in (xp, a, xq, b))
        tensor = False
    if not tensor:
        xp, xq = np.ascontiguousarray(xp, dtype=np.float64), np.ascontiguousarray(xq, dtype=np.float64)
        a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1), np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if native and not tensor:
        import torch
        from . import _capi
        _capi.require_device()
        dev = torch.device("cuda", int(device or 0))
        xp, a, xq, b = (torch.from_numpy(v).to(dev) for v in (xp, a, xq, b))
        tensor = True
    # rows with weight 0 are dropped before anything else (a NaN weight stays: it is what status 3 reports)
    if tensor:
        xp, a, xq, b = xp[a != 0.0].contiguous(), a[a != 0.0].contiguous(), xq[b != 0.0].contiguous(), b[b != 0.0].contiguous()
        ah, bh = a.cpu().numpy(), b.cpu().numpy()
    else:
        xp, a, xq, b = xp[a != 0.0], a[a != 0.0], xq[b != 0.0], b[b != 0.0]
        ah, bh = a, b
    nP, nQ = int(a.shape[0]), int(b.shape[0])
    out = _result(names, d, K, G, nP, nQ)
    gP, gQ = (group_ids(nP, G), group_ids(nQ, G)) if G > 0 else (None, None)

    # P's weights and values, with its mean and covariance
    if tensor:
        import torch
        from . import _capi
        from .posterior import COVARIANCE, Request, System
        with torch.cuda.device(xp.device):
            stream = torch.cuda.current_stream().cuda_stream
            cov = COVARIANCE.measure_dev([System(xp.data_ptr() if nP else 0, d, nP, d, a.data_ptr() if nP else 0, 0)], [Request(True, None)], xp.device.index,
                                         stream)[0]
    else:
        cov = _cov.measure(a, xp)
    if cov["status"] == _cov.NOT_FINITE:
        return _fail(out, BAD_VALUE if cov["column"] >= 0 else BAD_WEIGHT, cov["column"], "P")
    fewest_p = nP - (int(np.bincount(gP, minlength=G).max()) if G > 0 and nP else 0)
    fewest_q = nQ - (int(np.bincount(gQ, minlength=G).max()) if G > 0 and nQ else 0)
    if fewest_p < K + 1 or fewest_q < K or cov["status"] != _cov.OK:
        return _fail(out, FEW_ROWS)
    metric = _factor(cov)
    if metric is None:
        return _fail(out, NOT_POSITIVE)
    linv, mean = metric

    # both chains in P's metric; Q's weights and values
    if tensor:
        with torch.cuda.device(xp.device):
            zs = []
            for x, w, n in ((xp, a, nP), (xq, b, nQ)):
                z = torch.empty((n, d), dtype=torch.float64, device=x.device)
                wsb = _capi.div_whiten_workspace_bytes(n, d)
                ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
                report = _capi.div_whiten_dev(x.data_ptr(), d, n, d, linv, mean, w.data_ptr(), z.data_ptr(), ws.data_ptr(), wsb, stream)
                zs.append((z, report))
            (zp, _), (zq, rq) = zs
            bad_w, bad_col = rq[1] > 0, int(rq[2])
    else:
        with np.errstate(all="ignore"):
            zp, zq = whiten(xp, linv, mean), whiten(xq, linv, mean)
        bad_w = not (np.isfinite(b).all() and (b > 0.0).all())
        cols = np.flatnonzero(~np.isfinite(xq).all(axis=0))
        bad_col = int(cols[0]) if cols.size else -1
    if bad_w:
        return _fail(out, BAD_WEIGHT, -1, "Q")
    if bad_col >= 0:
        return _fail(out, BAD_VALUE, bad_col, "Q")

    session = (HipLevels if tensor else HostLevels)(zp, zq, a, b, gP, gQ, G, K)
    sums, per_level = run_ladder(session, nP, G, K)
    out.update(summarise(sums, masses(ah, gP, G), masses(bh, gQ, G)))
    out["rows_per_level"] = per_level
    out["sums"] = sums
    if getattr(session, "kernel_ms", None):
        out["kernel_ms"] = list(session.kernel_ms)
    return out


def lines(s, label="D_KL(P || Q)", ranks=True):
    """the lines printed for one estimate: one per rank, or (``ranks=False``) one line with every rank"""
    if not ranks:
        return ["   {} ({}): {}   rows {} against {}".format(label, ", ".join(s["names"]), "  ".join(
            "[k={}] {} ± {}".format(k + 1, s["D"][k], s["sigma"][k]) for k in range(len(s["D"]))), s["rows_p"], s["rows_q"])]
    return ["   {}[k={}] = {} ± {}   ({}; rows {} against {}; excluded {})".format(label, k + 1, s["D"][k], s["sigma"][k], ", ".join(s["names"]), s["rows_p"],
                                                                                  s["rows_q"], s["excluded"][k]) for k in range(len(s["D"]))]
