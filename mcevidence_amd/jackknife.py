"""Delete-a-group jackknife error bars on ln E from ONE nearest-neighbour search (docs/design/jackknife.md).

Deleting group b of G from the QUERIES removes their terms from the evidence sum; deleting it from the REFERENCE set changes a
query's k-th neighbour distance only where members of b are among its nearest neighbours, and the new k-th neighbour is then the
k-th entry of its ascending list that is not in b.  One search for a few more neighbours than ``kmax``, with rows, therefore fixes
all G leave-one-group-out sums exactly; a row whose list runs out for some group (a *short* row) is searched again for a longer
list: the ladder ``LADDER``.

``group_ids``       the group of every row of a partition (``by="blocks"``: stretches of the chain; ``by="chains"``: chain files)
``jackknife_host``  the rule in NumPy from ``(dist, idx)`` -- the route of a backend without a device, and the model of the tests
``summarise``       sigma and the bias-corrected value from the G leave-one-group-out values
``run_ladder``      the ladder over a session (``HipBackend.jackknife_lists`` -> ``HipSession``; ``HostSession`` otherwise)
``evidence_jackknife``   what ``MCEvidence.evidence_jackknife`` returns
``spec`` / ``resolve_groups`` / ``result``   the keyword, the number of groups and the result dict every route shares (the resident route
                    and the farm, docs/design/jackknife_resident.md, form the group ids and the leave-one-group-out sums on the device)

The rule is also csrc/jack.hpp (shared by the kernels and a serial driver); the kernels are csrc/jack_kernels.hpp.
"""
from __future__ import annotations

import math

import numpy as np

from .resident import mle_from_sums

__all__ = ["group_ids", "jackknife_host", "summarise", "run_ladder", "evidence_jackknife", "ladder", "LADDER", "MAX_GROUPS", "MAX_LIST", "spec",
           "resolve_groups", "result"]

LADDER = (16, 32, 128, 1024)
MAX_GROUPS = 64          # == MCE_JACK_MAX_GROUPS
MAX_LIST = 1024          # == MCE_GENERIC_MAX_K: the longest list a search returns (the top rung's list holds the own row too)
MAX_FAST = 32            # == MCE_MAX_K: the longest list of the MFMA search kernels
SKIP = 255               # csrc/jack.hpp: kJackSkip


def ladder(K, first=None):
    """the list lengths tried, in order: 16 (when K + 4 <= 16, else 32) -> 32 -> 128 -> 1024; ``first`` overrides the first rung"""
    if first is None:
        first = LADDER[0] if K + 4 <= LADDER[0] else LADDER[1]
    if first not in LADDER or first < K:
        raise ValueError("jackknife: the first rung must be one of %r and at least K=%d (got %r)" % (LADDER, K, first))
    return tuple(L for L in LADDER if L >= first)


def spec(jackknife):
    """the ``jackknife`` keyword of the resident route and the farm -- None / False (off), True (16 blocks), a number of blocks, or a dict
    with ``groups`` and ``by`` -- as a dict(groups, by), or None"""
    if jackknife is None or jackknife is False:
        return None
    kw = dict(jackknife) if isinstance(jackknife, dict) else ({} if jackknife is True else {"groups": int(jackknife)})
    unknown = sorted(set(kw) - {"groups", "by"})
    if unknown:
        raise ValueError("jackknife: unknown key%s %s ('groups' and 'by' expected)" % ("" if len(unknown) == 1 else "s", ", ".join(map(repr, unknown))))
    return {"groups": kw.get("groups", 16), "by": kw.get("by", "blocks")}


def resolve_groups(groups, by, nchains):
    """G of a call: ``groups`` under ``by="blocks"``, the number of chains under ``by="chains"`` (``nchains`` None: not known yet, nothing
    is said about it); the ValueErrors every route raises"""
    if by == "chains":
        if nchains is None:
            return None
        G = int(nchains)
        if G < 2:
            raise ValueError("jackknife by='chains' needs at least 2 chains (got %d)" % G)
    elif by == "blocks":
        G = int(groups)
    else:
        raise ValueError("jackknife: by=%r ('blocks' or 'chains' expected)" % (by,))
    if not (2 <= G <= MAX_GROUPS):
        raise ValueError("jackknife: G=%r groups (2 .. %d expected)" % (G, MAX_GROUPS))
    return G


def group_ids(gd, name, groups, by="blocks"):
    """int32 group of every row of partition ``name`` ("s1" / "s2") of an ``MCSamples``.  Groups cut the CHAIN, not the partition:
    ``by="blocks"``: ``row * groups // N`` with ``row`` the row's index in the concatenated burned / thinned sample and N that
    sample's length, so a split or shuffled s1 and s2 lose the same stretch of chain together; ``by="chains"``: the chain file (or
    input array) the row came from."""
    rows = np.asarray(gd.data[name].ichain, dtype=np.int64)
    n = int(gd.samples.shape[0])
    if by == "blocks":
        return (rows * int(groups) // n).astype(np.int32)
    if by == "chains":
        return np.asarray(gd.row_chain, dtype=np.int64)[rows].astype(np.int32)
    raise ValueError("jackknife: by=%r ('blocks' or 'chains' expected)" % (by,))


def _check_groups(G, gq, gr):
    if not (2 <= int(G) <= MAX_GROUPS):
        raise ValueError("jackknife: G=%r groups (2 .. %d expected)" % (G, MAX_GROUPS))
    for g in (gq, gr):
        if len(g) and (g.min() < 0 or g.max() >= G):
            raise ValueError("jackknife: a group id outside 0 .. %d" % (G - 1))


def _entry_groups(idx, gr, qid, k0):
    """the group every list entry counts under: its row's, or SKIP for a missing entry and (k0 = 1) for the own row"""
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(gr))
    grp = np.where(ok, np.asarray(gr, dtype=np.int64)[np.where(ok, idx, 0)], SKIP)
    if k0 == 1:
        own = np.arange(idx.shape[0], dtype=np.int64) if qid is None else np.asarray(qid, dtype=np.int64)
        grp = np.where(idx == own[:, None], SKIP, grp)
    return grp


def jackknife_host(dist, idx, gq, gr, G, k0, kmax, d, w, fs, qid=None):
    """The leave-one-group-out sums from ascending neighbour lists ``dist`` / ``idx`` [nq, L] in NumPy -- the rule of csrc/jack.hpp.
    ``gq`` [nq] / ``gr`` [nr]: groups of the query / reference rows; ``qid``: the queries' own reference rows (None: row q is
    reference row q), skipped in the lists when ``k0 == 1`` and reported for short rows.  Returns (dotp_groups[G, kmax],
    dotp_full[kmax], short_rows ascending int64): a short row -- one whose list, with some group other than its own (or none)
    skipped, holds fewer than K = kmax - k0 entries -- enters no sum."""
    dist = np.asarray(dist, dtype=np.float64)
    gq = np.asarray(gq, dtype=np.int32)
    gr = np.asarray(gr, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    fs = np.asarray(fs, dtype=np.float64)
    _check_groups(G, gq, gr)
    nq, L = dist.shape
    K = int(kmax) - int(k0)
    if K < 1 or L < K:
        raise ValueError("jackknife: lists of L=%d entries are shorter than the K=%d neighbours of the sums" % (L, K))
    grp = _entry_groups(idx, gr, qid, k0)
    valid = grp != SKIP
    keeps = {b: valid & (grp != b) for b in range(-1, G)}
    short = keeps[-1].sum(axis=1) < K
    for b in range(G):
        short |= (keeps[b].sum(axis=1) < K) & (gq != b)
    lnc = 0.5 * d * math.log(math.pi) - math.lgamma(1.0 + 0.5 * d)
    with np.errstate(divide="ignore"):
        base = lnc - np.log(np.abs(w)) + fs
        lnr = np.log(dist)
    sgn = np.where(w < 0.0, -1.0, 1.0)
    groups = np.zeros((G, kmax))
    full = np.zeros(kmax)
    for b in range(-1, G):
        rows = np.flatnonzero(~short & (gq != b))
        if not len(rows):
            continue
        first = np.argsort(~keeps[b][rows], axis=1, kind="stable")[:, :K]       # positions of the first K kept entries, ascending
        term = sgn[rows, None] * np.exp(base[rows, None] + d * np.take_along_axis(lnr[rows], first, axis=1))
        (full if b < 0 else groups[b])[k0:] = term.sum(axis=0)
    own = np.arange(nq, dtype=np.int64) if qid is None else np.asarray(qid, dtype=np.int64)
    return groups, full, own[short]


def summarise(lnE, lnE_groups):
    """(sigma[k], lnE_bias_corrected[k]) from the full-sample ln E [k] and the G leave-one-group-out values [G, k]:
    sigma = sqrt((G - 1) / G sum_b (lnE_b - mean_b lnE_b)^2), bias-corrected = G lnE - (G - 1) mean_b lnE_b."""
    lnE = np.asarray(lnE, dtype=np.float64)
    v = np.asarray(lnE_groups, dtype=np.float64)
    G = v.shape[0]
    mean = v.mean(axis=0)
    sigma = np.sqrt((G - 1.0) / G * ((v - mean) ** 2).sum(axis=0))
    return sigma, G * lnE - (G - 1.0) * mean


def group_share(idx, gr):
    """the largest share one group takes of a neighbour list (the rows of ``idx``), for the capacity error's message"""
    idx = np.asarray(idx, dtype=np.int64)
    best = 0.0
    for row in idx:
        g = np.asarray(gr)[row[(row >= 0) & (row < len(gr))]]
        if len(g):
            best = max(best, float(np.bincount(g).max()) / len(g))
    return best


def run_ladder(session, n1, G, k0, kmax, first=None):
    """The ladder: every row at the first rung, the rows still short at the next.  ``session.level(L, rows)`` returns the sums of the
    rows (None: all of them) from lists of L neighbours and the rows still short; level sums are added in level order.  Returns
    (dotp_groups, dotp_full, rows_per_level {L: rows searched at that rung})."""
    K = kmax - k0
    groups, full, rows, per_level = np.zeros((G, kmax)), np.zeros(kmax), None, {}
    for L in ladder(K, first):
        per_level[L] = int(n1 if rows is None else len(rows))
        g, f, short = session.level(L, rows)
        groups += g
        full += f
        rows = np.asarray(short, dtype=np.int64)
        if not len(rows):
            return groups, full, per_level
    raise ValueError("jackknife: %d row%s still short after lists of %d neighbours -- some group fills their whole neighbourhood (largest share of one "
                     "group in such a list: %.3f); use fewer groups or thin the chain more" % (len(rows), "" if len(rows) == 1 else "s", LADDER[-1],
                                                                                               session.share(LADDER[-1], rows)))


def _list_len(L, k0, nr):
    """neighbours asked of a search that excludes nothing, for the rung of L entries: L others and (auto evidence) the own row, within
    what a search returns.  The 32 rung asks for 32 in all -- own row included -- which keeps it on the MFMA kernels (K <= 32); one
    entry more would put its handful of rows on the plain exact kernel (measured: 24 rows against 1 M x 27, 0.75 s)."""
    want = L + k0
    if L <= MAX_FAST:
        want = min(want, MAX_FAST)
    return max(1, min(want, nr, MAX_LIST))


class HostSession(object):
    """The lists from scikit-learn and the sums from ``jackknife_host``: the route of a backend without ``jackknife_lists``.
    X, Y: whitened queries / references (Y None: auto evidence, Y = X with the own row skipped)."""

    def __init__(self, X, Y, kmax, weight, fs, gq, gr, G):
        from sklearn.neighbors import NearestNeighbors
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.k0 = 1 if Y is None else 0
        self.Y = self.X if Y is None else np.ascontiguousarray(Y, dtype=np.float64)
        self.kmax, self.w, self.fs, self.gq, self.gr, self.G = kmax, np.asarray(weight, dtype=np.float64), np.asarray(fs, dtype=np.float64), gq, gr, G
        self.nn = NearestNeighbors(algorithm="auto").fit(self.Y)

    def lists(self, L, rows):
        rows = np.arange(len(self.X), dtype=np.int64) if rows is None else rows
        return self.nn.kneighbors(self.X[rows], n_neighbors=_list_len(L, self.k0, len(self.Y)))

    def level(self, L, rows):
        sel = np.arange(len(self.X), dtype=np.int64) if rows is None else rows
        dist, idx = self.lists(L, sel)
        return jackknife_host(dist, idx, self.gq[sel], self.gr, self.G, self.k0, self.kmax, self.X.shape[1], self.w[sel], self.fs[sel], qid=sel)

    def share(self, L, rows):
        return group_share(self.lists(L, rows)[1], self.gr)


class _DeviceGroups(object):
    """the group ids of a session built from device tensors, copied to the host only where the capacity error's message wants them"""

    def __init__(self, g):
        self.g = g

    def __len__(self):
        return int(self.g.shape[0])

    def __array__(self, dtype=None, copy=None):
        a = self.g.cpu().numpy()
        return a if dtype is None else a.astype(dtype)


class HipSession(object):
    """Whitened rows, weights, terms and groups on the device; a level is one ``mce_knn_f64_dev`` and one ``mce_jack_dotp_dev``.
    ``whitened=False`` (auto evidence only): S1 are the RAW rows, whitened on the device by ``mce_evidence_feed_whiten_f64``
    (``jac`` is set); ``whitened=True``: S1 / S2 are whitened rows (S2 None: auto evidence), uploaded once."""

    def __init__(self, S1, S2, ndim, kmax, weight, fs, gq, gr, G, device=0, whitened=False):
        import torch
        from . import _capi
        _capi.require_device()
        _check_groups(G, gq, gr)
        self.torch, self.capi = torch, _capi
        self.dev = torch.device("cuda", device)
        self.kmax, self.G, self.d = int(kmax), int(G), int(ndim)
        self.k0 = 1 if S2 is None else 0
        n1 = int(np.asarray(S1).shape[0])
        self.n1, self.jac = n1, None
        f64 = dict(dtype=torch.float64, device=self.dev)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        fs = np.ascontiguousarray(fs, dtype=np.float64)
        if not whitened:
            if S2 is not None:
                raise ValueError("jackknife: cross evidence takes rows that are whitened already")
            self.X = torch.empty((n1, self.d), **f64)
            self.w = torch.empty(n1, **f64)
            self.fs = torch.empty(n1, **f64)
            self.jac, _, _ = _capi.evidence_feed_whiten(S1, self.d, self.kmax, weight, fs, self.X.data_ptr(), self.w.data_ptr(), self.fs.data_ptr(),
                                                        device=device, want_checksum=False)
            self.Y = self.X
        else:
            self.X = torch.from_numpy(np.ascontiguousarray(np.asarray(S1)[:, :self.d], dtype=np.float64)).to(self.dev)
            self.Y = self.X if S2 is None else torch.from_numpy(np.ascontiguousarray(np.asarray(S2)[:, :self.d], dtype=np.float64)).to(self.dev)
            self.w = torch.from_numpy(weight).to(self.dev)
            self.fs = torch.from_numpy(fs).to(self.dev)
        self.nr = int(self.Y.shape[0])
        self.gq = torch.from_numpy(np.ascontiguousarray(gq, dtype=np.int32)).to(self.dev)
        self.gr = self.gq if S2 is None else torch.from_numpy(np.ascontiguousarray(gr, dtype=np.int32)).to(self.dev)
        self.gr_host = np.asarray(gr)
        self.kernel_ms = []

    @classmethod
    def from_device(cls, X, w, fs, gq, kmax, G, jac=None, device=0):
        """Auto evidence from DEVICE tensors that are whitened already (what ``mce_evidence_feed_whiten_dev_f64`` leaves): X [n, d], w [n],
        fs [n] in fp64 and the int32 groups gq [n] (``mce_jack_groups_dev``).  Nothing is copied; the group ids are checked on the
        device by every ``mce_jack_dotp_dev``."""
        import torch
        from . import _capi
        if not (2 <= int(G) <= MAX_GROUPS):
            raise ValueError("jackknife: G=%r groups (2 .. %d expected)" % (G, MAX_GROUPS))
        self = cls.__new__(cls)
        self.torch, self.capi = torch, _capi
        self.dev = torch.device("cuda", device)
        self.kmax, self.G, self.d, self.k0 = int(kmax), int(G), int(X.shape[1]), 1
        self.n1 = self.nr = int(X.shape[0])
        self.jac = jac
        self.X = self.Y = X
        self.w, self.fs, self.gq, self.gr = w, fs, gq, gq
        self.gr_host = _DeviceGroups(gq)
        self.kernel_ms = []
        return self

    def _search(self, Xq, L, self_mode):
        """(dist, idx) [nq, L] on the device"""
        torch, capi = self.torch, self.capi
        nq = int(Xq.shape[0])
        dist = torch.empty((nq, L), dtype=torch.float64, device=self.dev)
        idx = torch.empty((nq, L), dtype=torch.int64, device=self.dev)
        wsb = capi.knn_workspace_bytes(nq, self.nr, self.d, L)
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize(self.dev)
        capi.knn_dev(Xq.data_ptr(), nq, self.Y.data_ptr(), self.nr, self.d, L, self_mode, 0, dist.data_ptr(), idx.data_ptr(), ws.data_ptr(), wsb)
        torch.cuda.synchronize(self.dev)
        return dist, idx

    def lists(self, L, rows):
        if rows is None:
            if self.k0 == 1:           # auto evidence, every row: the search leaves the own row out itself
                return self._search(self.X, max(1, min(L, self.nr - 1)), self.capi.SELF_EXCLUDE) + (None,)
            return self._search(self.X, _list_len(L, 0, self.nr), self.capi.SELF_NONE) + (None,)
        sel = self.torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.dev)
        return self._search(self.X.index_select(0, sel).contiguous(), _list_len(L, self.k0, self.nr), self.capi.SELF_NONE) + (sel,)

    def sums(self, dist, idx, sel):
        """``mce_jack_dotp_dev`` on lists that are on the device; ``sel``: the rows' numbers in s1 (None: all of s1)"""
        torch, capi = self.torch, self.capi
        nq, L = int(dist.shape[0]), int(dist.shape[1])
        w, fs, gq = (self.w, self.fs, self.gq) if sel is None else (self.w.index_select(0, sel), self.fs.index_select(0, sel), self.gq.index_select(0, sel))
        groups = torch.empty((self.G, self.kmax), dtype=torch.float64, device=self.dev)
        full = torch.empty(self.kmax, dtype=torch.float64, device=self.dev)
        short = torch.empty(nq, dtype=torch.int64, device=self.dev)
        nshort = torch.zeros(1, dtype=torch.int64, device=self.dev)
        wsb = capi.jack_workspace_bytes(nq, self.G, self.kmax)
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(self.dev)
        t0.record()
        capi.jack_dotp_dev(dist.data_ptr(), idx.data_ptr(), nq, L, 0 if sel is None else sel.data_ptr(), gq.data_ptr(), self.gr.data_ptr(), self.nr, self.G,
                           self.k0, self.kmax, self.d, w.data_ptr(), fs.data_ptr(), groups.data_ptr(), full.data_ptr(), short.data_ptr(), nshort.data_ptr(),
                           ws.data_ptr(), wsb)
        t1.record()
        torch.cuda.synchronize(self.dev)
        self.kernel_ms.append(float(t0.elapsed_time(t1)))
        ns = int(nshort.item())
        return groups.cpu().numpy(), full.cpu().numpy(), short[:ns].cpu().numpy()

    def level(self, L, rows):
        dist, idx, sel = self.lists(L, rows)
        return self.sums(dist, idx, sel)

    def share(self, L, rows):
        return group_share(self.lists(L, rows)[1].cpu().numpy(), self.gr_host)


def result(dotp_groups, dotp_full, per_level, jac, sumw, n1, sumw_groups, rows_groups, logLmax, kmax, logpv, G, by, cross=False):
    """the dict every route returns, from the ladder's sums and the leave-one-group-out bookkeeping: ``sumw`` / ``n1`` the full sample's
    weight sum and rows, ``sumw_groups[b]`` / ``rows_groups[b]`` those of the rows not in group b"""
    lnE = mle_from_sums(dotp_full, jac, sumw, logLmax, n1, kmax, logpv, cross)[1:]
    lnE_groups = np.zeros((G, kmax - 1))
    for b in range(G):
        lnE_groups[b] = mle_from_sums(dotp_groups[b], jac, sumw_groups[b], logLmax, int(rows_groups[b]), kmax, logpv, cross)[1:]
    sigma, bc = summarise(lnE, lnE_groups)
    return {"lnE": lnE, "sigma": sigma, "lnE_groups": lnE_groups, "lnE_bias_corrected": bc, "groups": G, "by": by, "rows_per_level": per_level}


def _refuse(mce, covtype):
    from . import parallel
    if mce.brange is not None or mce.nbatch > 1:
        raise ValueError("jackknife with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (mce.brange, mce.nbatch))
    if covtype not in ("all", "single"):
        raise ValueError("jackknife: covtype=%r ('all' or 'single' expected)" % (covtype,))
    if mce.split and covtype == "single":
        raise ValueError("jackknife with split=True and covtype='single' is not supported: s1 and s2 are whitened with different eigen-systems")
    if parallel.is_distributed():
        raise ValueError("jackknife under an initialised process group is not supported: run it in one process")


def evidence_jackknife(mce, groups=16, by="blocks", covtype="all", pvolume=None, pos_lnp=False, first=None):
    """``MCEvidence.evidence_jackknife``: ln E with a delete-a-group jackknife error bar.  Returns dict(lnE [kmax - 1], sigma,
    lnE_groups [G, kmax - 1], lnE_bias_corrected, groups, by, rows_per_level) -- the columns ``evidence()`` returns.  J, the
    eigen-system and logLmax are the full sample's: the jackknife is conditional on the full sample's whitening.  sigma is
    conservative (Efron-Stein), not a calibrated 1 sigma; the bias-corrected value is reported, never substituted for lnE."""
    if covtype is None:
        covtype = mce.covtype
    _refuse(mce, covtype)
    gd = mce.gd
    G = resolve_groups(groups, by, gd.nchains)
    kmax, ndim, split = mce.kmax, mce.ndim, bool(mce.split)
    k0 = 0 if split else 1
    s1, lnp, weight = gd.arrays("s1")
    s2 = gd.arrays("s2")[0] if split else None
    logL = np.asarray(-lnp if pos_lnp else lnp, dtype=np.float64)
    logLmax = float(np.amax(logL))
    fs = logL - logLmax
    weight = np.asarray(weight, dtype=np.float64)
    gq = group_ids(gd, "s1", G, by)
    gr = group_ids(gd, "s2", G, by) if split else gq
    n1 = int(s1.shape[0])

    make = getattr(mce.backend, "jackknife_lists", None)
    session = None
    if make is not None and not split and ndim <= 127:
        session = make(s1, None, ndim, kmax, weight, fs, gq, gr, G)                    # whitened on the device
        jac = session.jac
    if session is None:
        covstat = mce.get_covariance() if covtype == "all" else mce.get_covariance(s=s1[:, :ndim])
        jac = covstat["J"]
        X = mce.diagonalise_chain(s1[:, :ndim], covstat["eVec"], covstat["eVal"])
        Y = mce.diagonalise_chain(s2[:, :ndim], covstat["eVec"], covstat["eVal"]) if split else None
        session = make(X, Y, ndim, kmax, weight, fs, gq, gr, G, whitened=True) if make is not None else HostSession(X, Y, kmax, weight, fs, gq, gr, G)
    dotp_groups, dotp_full, per_level = run_ladder(session, n1, G, k0, kmax, first)

    logpv = math.log(mce.priorvolume if pvolume is None else pvolume)
    aw = np.asarray(gd.data["s1"].adjusted_weights, dtype=np.float64)
    rest = [gq != b for b in range(G)]
    out = result(dotp_groups, dotp_full, per_level, jac, np.sum(aw), n1, [np.sum(aw[r]) for r in rest], [int(r.sum()) for r in rest], logLmax, kmax, logpv,
                 G, by, split)
    if getattr(session, "kernel_ms", None):
        out["kernel_ms"] = list(session.kernel_ms)
    return out
