"""The host model and the cases of the run-time k-NN certificate (mcevidence_amd/csrc/verify_kernels.hpp: verify_scan_kernel,
verify_check_kernel, verify_row; mce_verify_knn_f64[_dev], mce_options.verify).  Shared by tests/test_oracle_verify.py (CPU) and
tests/test_gpu_verify_power.py (GPU).  The lists under test are the host oracle's (helpers.oracle_lists), corrupted by hand: the
certificate is on trial here, the searches are not.

THE RULE, as include/mcevidence_hip.h documents it.  With r_1 .. r_K the reported distances of a query row and d2_j the squared
distance to usable reference row j (every row but, under SELF_EXCLUDE, row self_offset + q), the row PASSES iff for every k = 1 .. K
    #{j : d2_j <  r_k^2 (1 - 1e-9)} <= k - 1
    #{j : d2_j <= r_k^2 (1 + 1e-9)} >= k
and no entry is NaN or negative; +inf in column k is accepted only if fewer than k usable rows exist.  Model.judge applies it with
d2 in np.longdouble by direct differences, column by column.  The scan does not look at a reference row beyond the LAST column's
upper threshold h, whatever the other columns hold; with N = #{d2 <= h} that changes no row's verdict:
  * a column whose lower threshold exceeds h has its first count cut down to N.  That hides a failure only if N <= k - 1 < K, and
    then the last column fails its second count (it needs N >= K);
  * a column whose upper threshold exceeds h has its second count cut down to N.  That fails it only if N < k <= K, and then the
    last column fails its second count in truth as well.
(h = NaN counts nothing, and the NaN fails the row; h = +inf cuts nothing.)

UNDECIDED rows.  The scan's d2 is not the exact one, and its thresholds are rounded: a row is undecided when some exact d2 lies within
relative G of one of the row's 2 K thresholds.  G is derived from the kernel, u = 2^-53:
  * each difference x_i - y_i is rounded once, (1 + e) with |e| <= u, so its square carries (1 + e)^2: 2 u;
  * the D squares are summed by D fused multiply-adds, one rounding of a partial sum of non-negative terms each: D u;
    together the scan's d2 is within (D + 2) u of the truth, to first order;
  * the threshold is fl(fl(r r) c) with c = fl(1 -+ 1e-9): one rounding for r r, one for the product: 2 u.  The model multiplies
    the exact r^2 by the SAME double c, so c itself contributes nothing;
  * the terms of second order ((D + 4)^2 u^2 < 2^-38 u) and the model's own arithmetic in np.longdouble ((D + 3) 2^-64 < 2^-4 u)
    are covered by 2 u more.
G = (D + 6) u: 1.5e-14 at D = 128, five orders below the 1e-9 of the rule and three below the 2e-11 by which a benign corruption
moves d2.
A threshold of exactly 0 (r = 0) is never undecided: the scan's d2 is 0 exactly when every difference is, as the exact one.
Undecided rows are counted on the model alone; a case with more than UNDECIDED_CAP of its judged rows undecided is refused, which at
these sizes means one row.

THE SAMPLE: sample_rows mirrors verify_row as the header documents it, row (seed % nq + floor(s nq / n)) % nq for s < n.
"""
import functools
import math
import zlib

import numpy as np

from helpers import ADVERSARIAL, CROSS, SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE, needs_two_columns, oracle_lists

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the model needs a long double wider than double"
TOL = 1e-9
C_LO, C_HI = LD(1.0 - TOL), LD(1.0 + TOL)           # the kernel's own doubles
UNDECIDED_CAP = 1e-5
U64 = 2 ** 64 - 1


def scan_rounding(D):
    """G (derivation above)"""
    return (D + 6.0) * 2.0 ** -53


def sample_rows(n, nq, seed):
    """the rows verify_row gives for samples 0 .. n - 1 of n <= nq (Python integers: no overflow to mirror)"""
    n = min(int(n), int(nq))
    return np.array([(seed % nq + s * nq // n) % nq for s in range(n)], dtype=np.int64)


def sample_rows_strided(n, nq, seed):
    """the pattern before the fix (stride = nq / n, at least 1): one contiguous block wherever nq / 2 < n < nq.  Kept to show, on the
    host, that the cases below tell the two apart"""
    n = min(int(n), int(nq))
    stride = max(1, nq // n)
    return np.array([(seed % nq + s * stride) % nq for s in range(n)], dtype=np.int64)


def rsplit_of(nr, nsample):
    """reference splits a launch takes -- capi.hip, mce_verify_knn_f64_dev:  nb = ceil(ns / 16) workgroups of queries,
    rsplit = max(1, min(64, ceil(nr / 4096), ceil(4 * 256 / nb))) with 256 the compute units assumed; split s scans rows
    [nr s / rsplit, nr (s + 1) / rsplit)"""
    nb = -(-nsample // 16)
    return max(1, min(64, -(-nr // 4096), -(-4 * 256 // nb)))


# ---- the model ------------------------------------------------------------------------------------------------------------------
def exact_d2(X, Y):
    """[nq][nr] squared distances in np.longdouble by direct differences (helpers.exact_distances, over all rows)"""
    Xl, Yl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(Y, dtype=np.float64).astype(LD)
    out = np.zeros((len(Xl), len(Yl)), dtype=LD)
    for i in range(Xl.shape[1]):
        t = Xl[:, i, None] - Yl[None, :, i]
        out += t * t
    return out


class Model:
    """the rule on one (X, Y, self mode, self offset): judge(dist) -> (fails[nq], undecided[nq])"""

    def __init__(self, X, Y, self_mode, self_offset=0):
        self.nq, self.D = X.shape
        self.G = LD(scan_rounding(self.D))
        d2 = exact_d2(X, Y)
        self.usable = len(Y)
        if self_mode == SELF_EXCLUDE:
            d2[np.arange(self.nq), self_offset + np.arange(self.nq)] = np.inf
            self.usable -= 1
        self.sorted = np.sort(d2, axis=1)[:, :self.usable]          # (the own row, at +inf, is cut off)

    def judge_row(self, q, r):
        S, U, K = self.sorted[q], self.usable, len(r)
        k = np.arange(K)
        nan, inf, fin = np.isnan(r), r == np.inf, np.isfinite(r)
        bad = nan | (r < 0) | (inf & (U > k))
        r2 = np.where(fin, r, 0.0).astype(LD) ** 2
        lo, hi = r2 * C_LO, r2 * C_HI
        bad |= fin & ((np.searchsorted(S, lo, "left") > k) | (np.searchsorted(S, hi, "right") < k + 1))
        near = np.zeros(K, dtype=bool)
        for thr in (lo, hi):
            inside = np.searchsorted(S, thr * (1 + self.G), "right") - np.searchsorted(S, thr * (1 - self.G), "left")
            near |= fin & (thr > 0) & (inside > 0)
        return bool(bad.any()), bool(near.any())

    def judge(self, dist, rows=None):
        """verdicts of the given rows of dist[nq][K] (all rows by default) -> (fails, undecided), bool[nq], False elsewhere"""
        fails, undecided = np.zeros(self.nq, dtype=bool), np.zeros(self.nq, dtype=bool)
        for q in (range(self.nq) if rows is None else rows):
            fails[q], undecided[q] = self.judge_row(int(q), np.asarray(dist[q], dtype=np.float64))
        return fails, undecided


# ---- the corruption catalogue ---------------------------------------------------------------------------------------------------
SMALLER, LARGER = 1.0 - 1e-8, 1.0 + 1e-8            # 20 times the 1e-9 tolerance on d2 (the factor is on d)
BENIGN = 1e-11                                      # a fiftieth of it


def touched_rows(nq, j, spread=False):
    """R: row 0, the last row, the first row of a last partial group of 16, sample position 256, three rows dealt from the counter j;
    `spread`: besides, every third row of the first half and every row of the last fifth (the partial samples)"""
    R = {0, nq - 1, (7 * j + 3) % nq, (11 * j + 5) % nq, (13 * j + 1) % nq}
    if nq % 16:
        R.add(16 * (nq // 16))
    if nq > 256:
        R.add(256)
    if spread:                                      # (denser at the end: a contiguous block and an even spread see different counts)
        R.update(range(0, nq // 2, 3))
        R.update(range(nq - nq // 5, nq))
    return np.array(sorted(R), dtype=np.int64)


def _padded(od, K):
    """the oracle's lists as [nq][K + 1]: +inf where the reference set ends (an unfilled slot)"""
    full = np.full((od.shape[0], K + 1), np.inf)
    full[:, :od.shape[1]] = od[:, :K + 1]
    return full


def _missed(c):
    def f(full, K, R):
        dist = full[:, :K].copy()
        dist[R] = np.delete(full[R], c, axis=1)
        return dist
    return f


def _scaled(c, factor, resort):
    def f(full, K, R):
        dist = full[:, :K].copy()
        dist[R, c] *= factor
        if resort:
            dist[R] = np.sort(dist[R], axis=1)
        return dist
    return f


def _twice(c):
    def f(full, K, R):
        dist = full[:, :K].copy()
        dist[R, c + 1:] = full[R, c:K - 1]
        return dist
    return f


def _own_in_front(full, K, R):
    dist = full[:, :K].copy()
    dist[R, 1:] = full[R, :K - 1]
    dist[R, 0] = 0.0
    return dist


def _set(cols, value):
    def f(full, K, R):
        dist = full[:, :K].copy()
        for c in (range(K) if cols == "all" else cols):
            dist[R, c] = value
        return dist
    return f


def _negated_last(full, K, R):
    dist = full[:, :K].copy()
    dist[R, K - 1] = -dist[R, K - 1]
    return dist


def _swapped(full, K, R):
    """the first and the last column that differ on the row (none: the row stays)"""
    dist = full[:, :K].copy()
    for q in R:
        other = np.flatnonzero(dist[q] != dist[q, 0])
        if len(other):
            dist[q, 0], dist[q, other[-1]] = dist[q, other[-1]], dist[q, 0]
    return dist


def catalogue(K, exclude, j):
    """[(name, f(full, K, R) -> dist, rows: "R" | "spread" | "all")] of the table in docs/design/adversarial_matrix.md; j deals the
    NaN's column"""
    out = [("a%d" % c, _missed(c), "R") for c in sorted({0, K // 2, K - 1})]
    out += [("b%d" % c, _scaled(c, SMALLER, True), "R") for c in sorted({0, K - 1})]
    out += [("c%d" % c, _scaled(c, LARGER, False), "R") for c in sorted({0, K - 1})]
    if K >= 2:
        out += [("d%d" % c, _twice(c), "R") for c in sorted({0, K - 2})]
    if exclude:
        out.append(("e", _own_in_front, "R"))
    out += [("f_inf_last", _set([K - 1], np.inf), "R"), ("f_inf_all", _set("all", np.inf), "R"), ("f_nan%d" % (j % K), _set([j % K], np.nan), "R"),
            ("f_neg_last", _negated_last, "R"), ("g", _swapped, "R")]
    out += [("h_up", lambda full, K, R: full[:, :K] * (1.0 + BENIGN), "all"), ("h_down", lambda full, K, R: full[:, :K] * (1.0 - BENIGN), "all")]
    # the partial samples: corruptions on many rows, unevenly spread
    out += [("spread_a%d" % (K - 1), _missed(K - 1), "spread"), ("spread_nan%d" % (j % K), _set([j % K], np.nan), "spread")]
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------------
KINDS = ("heavy_tails", "one_outlier", "huge_scale_offset", "tiny_scale", "few_distinct", "all_identical", "lattice_ties", "subnormal_fp16_coords",
         "queries_on_refs")
CROSS_KIND = "queries_on_refs"
DIMS = (1, 7, 8, 9, 16, 127, 128)
KS = (1, 2, 9, 31, 32)
NQ = (1, 15, 16, 17, 257)
NR = ("K+1", 33, 513, 4097)
SELFS = ("none", "include", "exclude", "shard")
STEPS = 90
#: the one case of the sampling fix: nq / 2 < ns < nq
SAMPLING_CASE = dict(kind="heavy_tails", d=7, K=2, nq=600, ns=301, nr=4097, self="exclude")
#: cases the model alone refused as dealt (an undecided row), and what was changed, keyed by the id as dealt
ADJUST = {
}


def case_id(c):
    return "%(kind)s-d%(d)d-K%(K)d-q%(nq)d-s%(ns)d-n%(nr)d-%(self)s" % c


def deal(steps=STEPS, adjust=None):
    """attribute k of step j is j mod m_k, the m_k pairwise coprime and each the smallest that holds its list (as
    tests/test_gpu_small_shapes.py deals): `steps` cases, not a product, and SAMPLING_CASE"""
    adjust = ADJUST if adjust is None else adjust
    lists = [KINDS, DIMS, KS, NQ, NR, SELFS]
    mods = []
    for lst in lists:
        m = len(lst)
        while any(math.gcd(m, o) != 1 for o in mods):
            m += 1
        mods.append(m)
    cases, seen, j = [], set(), 0
    while len(cases) < steps:
        kind, d, K, nq, nr, self_ = [lst[j % m % len(lst)] for lst, m in zip(lists, mods)]
        j += 1
        assert j < 100 * steps
        if d == 1 and needs_two_columns(kind):
            continue
        if kind == CROSS_KIND:
            self_ = "none"
        # the smallest reference count of the list that serves K and holds the query rows (a shard starts past row 0)
        need = max(K + (self_ in ("exclude", "shard")), 0 if self_ == "none" else nq + (self_ == "shard"))
        sizes = [K + 1 if t == "K+1" else t for t in NR]
        nr = K + 1 if nr == "K+1" else nr
        if nr < need:
            nr = min(s for s in sizes if s >= need)
        c = dict(kind=kind, d=d, K=K, nq=nq, ns=nq, nr=nr, self=self_, step=j - 1)
        c["dealt"] = case_id(c)
        if c["dealt"] in adjust:
            c.update({k: v for k, v in adjust[c["dealt"]].items() if k != "reason"})
        if case_id(c) in seen:
            continue
        seen.add(case_id(c))
        cases.append(c)
    last = dict(SAMPLING_CASE, step=j)
    last["dealt"] = case_id(last)
    return cases + [last]


CASES = deal()


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def case_inputs(c):
    """(X, Y, self_mode, self_offset).  none: separate sets (one draw of the kind cut in two; the cross kind's own generator);
    include, exclude: the first nq rows of the one buffer; shard: nq rows from row (nr - nq + 1) / 2 > 0 on"""
    rng = _rng("verify", c["kind"], c["d"], c["nr"], c["nq"], c["self"], c.get("salt", 0))
    nq, nr, d = c["nq"], c["nr"], c["d"]
    if c["kind"] == CROSS_KIND:
        X, Y = CROSS[CROSS_KIND](rng, nq, nr, d)
        return np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64), SELF_NONE, 0
    if c["self"] == "none":
        Z = np.ascontiguousarray(ADVERSARIAL[c["kind"]](rng, nq + nr, d), dtype=np.float64)
        return np.ascontiguousarray(Z[:nq]), np.ascontiguousarray(Z[nq:]), SELF_NONE, 0
    Y = np.ascontiguousarray(ADVERSARIAL[c["kind"]](rng, nr, d), dtype=np.float64)
    off = (nr - nq + 1) // 2 if c["self"] == "shard" else 0
    assert off + nq <= nr and (off > 0) == (c["self"] == "shard")
    return np.ascontiguousarray(Y[off:off + nq]), Y, SELF_INCLUDE if c["self"] == "include" else SELF_EXCLUDE, off


class Entry:
    """one corruption of a case: dist, the rows it touched, and the model's verdict per row"""

    def __init__(self, name, dist, R, fails):
        self.name, self.dist, self.R, self.fails = name, np.ascontiguousarray(dist), R, fails

    @property
    def count(self):
        return int(self.fails.sum())


class Built:
    """a case, judged by the model alone: inputs, the clean lists, the catalogue -> entries, judged and undecided (row, list) pairs"""

    def __init__(self, X, Y, sm, off, K, step):
        self.X, self.Y, self.sm, self.off, self.K = X, Y, sm, off, K
        nq = len(X)
        od = oracle_lists(X, Y, K, sm, off)[0]
        self.full = _padded(od, K)
        self.model = Model(X, Y, sm, off)
        self.clean = np.ascontiguousarray(self.full[:, :K])
        self.clean_fails, und = self.model.judge(self.clean)
        self.judged, self.undecided = nq, int(und.sum())
        self.entries = []
        for i, (name, f, rows) in enumerate(catalogue(K, sm == SELF_EXCLUDE, step)):
            R = np.arange(nq) if rows == "all" else touched_rows(nq, step + i, spread=rows == "spread")
            self.add(name, f(self.full, K, R), R)

    def add(self, name, dist, R):
        fails, und = self.model.judge(dist, R)
        fails |= self.clean_fails & ~np.isin(np.arange(len(fails)), R)
        self.judged += len(R)
        self.undecided += int(und.sum())
        self.entries.append(Entry(name, dist, R, fails))
        return self.entries[-1]

    def refuse_if_undecided(self, what):
        if self.undecided > UNDECIDED_CAP * self.judged:
            raise ValueError("%s: %d of %d judged rows are undecided on the model alone (cap %g): change the salt or the input"
                             % (what, self.undecided, self.judged, UNDECIDED_CAP))
        return self


@functools.lru_cache(maxsize=2)
def _built(key):
    c = next(c for c in CASES if case_id(c) == key)
    X, Y, sm, off = case_inputs(c)
    return Built(X, Y, sm, off, c["K"], c["step"]).refuse_if_undecided(key)


def built(c):
    return _built(case_id(c))


# ---- the planted neighbour: where a scan loses a row ----------------------------------------------------------------------------
PLANT_NR = (4096, 4097, 8193)
PLANT_NQ, PLANT_D, PLANT_OFF = 64, 9, 300
PLANT_CASES = [dict(nr=nr, self=self_, K=K) for nr in PLANT_NR for self_, K in (("none", 1), ("shard", 5))]


def plant_id(p):
    return "n%(nr)d-%(self)s-K%(K)d" % p


def plant_rows(nr, nsample=PLANT_NQ):
    """reference rows to plant at: the ends, the first block of 256 threads, and both sides of every boundary nr s / r of r = 2 .. 4
    splits and of the split count the launch takes (all-rows call and one-row call)"""
    J = {0, 255, 256, nr - 1}
    for r in {2, 3, 4, rsplit_of(nr, nsample), rsplit_of(nr, 1)}:
        for s in range(1, r):
            J.update((nr * s // r, nr * s // r - 1))
    return sorted(J)


@functools.lru_cache(maxsize=None)
def _planted(key):
    p = next(p for p in PLANT_CASES if plant_id(p) == key)
    nr, K, shard = p["nr"], p["K"], p["self"] == "shard"
    rng = _rng("plant", key)
    Y = rng.standard_normal((nr, PLANT_D))
    sm, off = (SELF_EXCLUDE, PLANT_OFF) if shard else (SELF_NONE, 0)
    X = Y[off:off + PLANT_NQ] if shard else rng.standard_normal((PLANT_NQ, PLANT_D))      # (shard: a view, so that a planted own-row neighbour is a query too)
    J = plant_rows(nr)
    assert not shard or not any(off <= j < off + PLANT_NQ for j in J)
    # one query per planted row, three apart (rows 1, 4, 7, ...).  Under exclude, first, the rows next to the own rows of queries 2
    # and 5 in memory, as their nearest: those are the own rows of queries 1 and 6, which move with them (X is a view)
    own_side = [(2, off + 2 - 1), (5, off + 5 + 1)] if shard else []
    targets = own_side + [(3 * i + 1, j) for i, j in enumerate(J)]
    assert max(q for q, _ in targets) < PLANT_NQ and len({j for _, j in targets}) == len(targets)
    for i, (q, j) in enumerate(targets):
        if i == 0 or i == len(own_side):
            od0 = oracle_lists(np.ascontiguousarray(X), Y, K, sm, off)[0]
        c = 0 if i < len(own_side) else i % K                   # the planted row becomes the c-th nearest (from 0) of its query
        lo = od0[q, c - 1] if c else 0.0
        step = np.zeros(PLANT_D)
        step[i % PLANT_D] = 0.5 * (lo + od0[q, c])
        Y[j] = X[q] + step
    X = np.ascontiguousarray(X)
    b = Built.__new__(Built)
    b.X, b.Y, b.sm, b.off, b.K = X, Y, sm, off, K
    od, oi, _ = oracle_lists(X, Y, K, sm, off)
    b.full, b.model = _padded(od, K), Model(X, Y, sm, off)
    b.clean = np.ascontiguousarray(b.full[:, :K])
    b.clean_fails, und = b.model.judge(b.clean)
    b.judged, b.undecided, b.entries = len(X), int(und.sum()), []
    # (query, planted row, its column in the oracle's list of the finished data: inside the K reported)
    b.planted = [(q, j, int(np.flatnonzero(oi[q] == j)[0])) for q, j in targets]
    assert all(c < K for _, _, c in b.planted) and len({q for q, _, _ in b.planted}) == len(targets), b.planted
    dist = b.clean.copy()
    for q, j, c in b.planted:
        dist[q] = np.delete(b.full[q], c)
    b.add("lost_all", dist, np.array(sorted(q for q, _, _ in b.planted)))
    return b.refuse_if_undecided(key)


def planted(p):
    return _planted(plant_id(p))
