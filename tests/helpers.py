"""Shared test helpers (tests only; the oracle is never imported by the product)."""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import oracle_np as orc  # noqa: E402
from mcevidence_amd.synth import gaussian_chain  # noqa: E402

GOLD = os.path.join(HERE, "golden")

#: stated fp64 tolerance on ln E (|dlnE| <= 1e-9)
LNE_TOL = 1e-9
#: row-level tolerance on kNN distances (GEMM-form fp64 vs exact differences)
DIST_RTOL = 1e-10


def load_golden():
    out = {}
    for tag in ("small", "medium", "big", "sym", "sym2", "c4_n20000", "c4", "c5_n200000", "c5"):
        jp = os.path.join(GOLD, "evidence_%s.json" % tag)
        if not os.path.exists(jp):
            continue
        arrays = np.load(os.path.join(GOLD, "evidence_%s.npz" % tag))
        for case in json.load(open(jp)):
            case = dict(case)
            case["tag"] = tag
            case.setdefault("seed_split", None)          # (config cases -- C4 -- carry an explicit split instead: explicit_split_of)
            case["arrays"] = {k[len(case["name"]) + 2:]: arrays[k] for k in arrays.files if k.startswith(case["name"] + "__")}
            out[case["name"]] = case
    return out


def host_pins():
    return json.load(open(os.path.join(GOLD, "host_pins.json")))


def chain_of(case):
    if case.get("config"):                      # a BASELINE.json config recipe (synth.config_chain): C4 = two chains stacked
        from mcevidence_amd.synth import config_chain
        return config_chain(case["config"], n=case.get("n_per_chain"))[0]
    return gaussian_chain(**case["chain"])


def explicit_split_of(case):
    """(s1_rows, s2_rows) of a config case with a caller-chosen split, else None"""
    if case.get("config"):
        from mcevidence_amd.synth import config_chain
        r1, r2 = config_chain(case["config"], n=case.get("n_per_chain"))[1]
        return None if r1 is None else (r1, r2)
    return None


class OracleBackend(object):
    """Test double for ``HipBackend``: the same interface served by the CPU oracle, so the
    host bookkeeping of ``MCEvidence`` can be pinned against the goldens without a GPU."""

    name = "oracle"

    def __init__(self, knn="brute"):
        self.knn = knn
        self.calls = []

    def knn_dotp(self, X, Y, weight, fs, kmax, k0, want_dist=False):
        ref = X if Y is None else Y
        K = kmax - k0
        if self.knn == "sklearn":
            d, _ = orc.knn_sklearn(X, ref, kmax + 1)
            d = d[:, k0:kmax]
        else:
            d, _ = orc.knn_brute(X, ref, K, self_mode=2 if k0 == 1 else 0)
        ndim = X.shape[1]
        full = np.zeros((X.shape[0], kmax))
        full[:, k0:] = d
        dotp = orc.dotp_literal(full, weight, fs, ndim, k0, kmax)
        self.calls.append(dict(nq=X.shape[0], nr=ref.shape[0], d=ndim, kmax=kmax, k0=k0))
        return dotp, (d if want_dist else None)


class OracleFeedBackend(OracleBackend):
    """OracleBackend that also offers the device-feeder routes (``evidence_feed`` and its batched
    form) -- NumPy covariance/eigen-system/whitening in front of the same oracle search."""

    def evidence_feed(self, S1, S2, ndim, cov_mode, kmax, weight, fs):
        s1 = np.asarray(S1)[:, :ndim]
        s2 = None if S2 is None else np.asarray(S2)[:, :ndim]

        def eig(rows):
            ev, U = np.linalg.eigh(np.atleast_2d(np.cov(rows.T)))
            if (ev <= 0).any():
                raise ValueError("math domain error")
            # the library's documented canonical form (include/mcevidence_hip.h): eigenvalues
            # descending, largest component of each eigenvector positive
            ev, U = ev[::-1], U[:, ::-1]
            sgn = np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])
            return ev, U * sgn
        if cov_mode == 0:
            ev, U = eig(s1 if s2 is None else np.concatenate([s1, s2]))
            ev2, U2 = ev, U
        else:
            ev, U = eig(s1)
            ev2, U2 = (ev, U) if s2 is None else eig(s2)
        X = (s1 @ U) / np.sqrt(ev)
        Y = None if s2 is None else (s2 @ U2) / np.sqrt(ev2)
        dotp, _ = self.knn_dotp(X, Y, weight, fs, kmax, 0 if s2 is not None else 1)
        return dotp, math.sqrt(float(np.prod(ev)))

    def evidence_feed_batch(self, problems):
        self.batches = getattr(self, "batches", []) + [len(problems)]
        return [self.evidence_feed(*p) for p in problems]


def lnE_from_dotp(case, dotp):
    return orc.mle_from_dotp(np.asarray(dotp), case["S"], case["k0"], case["kmax"], case["SumW"], case["J"],
                             case["logLmax"], case["lnPriorVolume"])


def build_mce(case, **kw):
    """The drop-in class set up as the reference was when it produced ``case``: the global RNG seeded before a random
    split, or the explicit split of a config case (C4: two independent chains stacked, s1 = the first)."""
    import mcevidence_amd as pkg
    if case["seed_split"] is not None:
        np.random.seed(case["seed_split"])
    mk = dict(case["mce"])
    split = explicit_split_of(case)
    if split is not None:
        mk.pop("split", None)
    mce = pkg.MCEvidence([chain_of(case)], verbose=0, **mk, **kw)
    if split is not None:
        mce.set_split(*split)
    return mce


# --------------------------------------------------------------------------------------------------------------------
# ill-conditioned chain families for the device feeders (tests/test_gpu_feeders.py, tests/test_oracle_feeders.py).
# Every family returns a chain in the reference's column layout (weight, -ln L, params...), seeded.  C is the covariance,
# Cn = diag(C)^-1/2 C diag(C)^-1/2 its correlation matrix; the eigenvalues of C are fixed to about eps * cond(Cn)
# relative by C itself (Demmel & Veselic 1992), whatever cond(C) is.
# --------------------------------------------------------------------------------------------------------------------
def _chain_from_rows(rows, z, rng):
    """weights 1..5, -ln L = z.z / 2 (the Gaussian the rows were drawn from, up to a constant)"""
    w = rng.integers(1, 6, rows.shape[0]).astype(np.float64)
    nll = 0.5 * np.einsum("ij,ij->i", z, z) + 0.5 * z.shape[1] * math.log(2.0 * math.pi)
    return np.column_stack([w, nll, rows])


def graded_cov(c):
    """Graded covariance number ``c`` (0..5, d = 6, 12, 27, 27, 40, 64) of one seeded recipe: C = diag(s) Cn diag(s) with
    s spanning 1e-4..1e2 (even c) or a permuted 1e-5..1e1 (odd c), and for c >= 2 a near-dependence 50 v v^T in Cn.
    c = 4 (d = 40, cond(C) 7.7e13, cond(Cn) 3.8e4) is the matrix on which a stopping rule relative to the LARGEST
    eigenvalues leaves the small ones wrong by 2e-9."""
    rng = np.random.default_rng(1)
    for k in range(c + 1):
        d = [6, 12, 27, 27, 40, 64][k]
        sig = np.logspace(-4, 2, d) if k % 2 == 0 else np.logspace(-5, 1, d)[rng.permutation(d)]
        L = np.eye(d) + 0.8 * rng.standard_normal((d, d)) / math.sqrt(d)
        Cn = L @ L.T
        if k >= 2:
            v = rng.standard_normal(d)
            Cn += 50 * np.outer(v, v)
        Cn = Cn / np.outer(np.sqrt(np.diag(Cn)), np.sqrt(np.diag(Cn)))
    return Cn * np.outer(sig, sig)


def sampled_chain(C, n, seed, mean=None):
    """n rows drawn from N(mean, C)"""
    rng = np.random.default_rng(seed)
    d = C.shape[0]
    z = rng.standard_normal((n, d))
    rows = z @ np.linalg.cholesky(C).T
    if mean is not None:
        rows += mean
    return _chain_from_rows(rows, z, rng)


def graded_chain(seed, n, d, lo=1e-5, hi=1e2, dep=50.0):
    """graded Gaussian: spreads log-spaced over [lo, hi] in random column order, random correlations plus one
    near-dependence of weight ``dep``"""
    rng = np.random.default_rng(seed)
    sig = np.logspace(math.log10(lo), math.log10(hi), d)[rng.permutation(d)]
    L = np.eye(d) + 0.8 * rng.standard_normal((d, d)) / math.sqrt(max(d, 1))
    Cn = L @ L.T
    if d > 1 and dep:
        v = rng.standard_normal(d)
        Cn += dep * np.outer(v, v)
    Cn = Cn / np.outer(np.sqrt(np.diag(Cn)), np.sqrt(np.diag(Cn)))
    return sampled_chain(Cn * np.outer(sig, sig), n, seed + 1000)


def planck_allparams_chain(seed, n, nderived=6, nnuis=15):
    """A Planck '--allparams' stand-in: the 6 base parameters of synth.PLANCK_PARAMS (their means and spreads, mildly
    correlated), ``nderived`` derived columns that are smooth non-linear functions of them plus noise of 1e-3 of their
    spread (near-functions), and ``nnuis`` nuisance amplitudes with spreads of ~10."""
    from mcevidence_amd.synth import PLANCK_PARAMS
    rng = np.random.default_rng(seed)
    mu = np.array([p[1] for p in PLANCK_PARAMS])
    sg = np.array([p[2] for p in PLANCK_PARAMS])
    mix = np.eye(6) + 0.3 * rng.standard_normal((6, 6))
    z = rng.standard_normal((n, 6))
    zz = z @ mix
    zz /= zz.std(axis=0)
    ob, oc, th, tau, logA, ns = (mu + zz * sg).T
    h = 0.6736 + 50.0 * (th - 1.04085) - 1.5 * (oc - 0.1197)               # H0 / 100 from theta and the densities
    derived = [100.0 * h, (ob + oc) / h ** 2, 0.811 * np.exp(0.5 * (logA - 3.089)) * (oc / 0.1197) ** 0.6,
               13.8 - 8.0 * (h - 0.6736), 0.1 * np.exp(logA) * np.exp(-2.0 * tau), 1090.0 + 300.0 * (ob - 0.02222) - 20.0 * (ns - 0.9655)]
    cols = [ob, oc, th, tau, logA, ns]
    for k in range(nderived):
        f = derived[k % len(derived)] * (1.0 + 0.01 * (k // len(derived)))
        cols.append(f + 1e-3 * f.std() * rng.standard_normal(n))
    nuis = 10.0 * rng.uniform(0.5, 2.0, nnuis) * rng.standard_normal((n, nnuis)) + rng.uniform(50, 500, nnuis)
    rows = np.column_stack(cols + [nuis])
    return _chain_from_rows(rows, np.column_stack([z, (nuis - nuis.mean(0)) / nuis.std(0)]), rng)


def offset_chain(seed, n, d, ratio=1e5):
    """offset-dominated: column means up to ``ratio`` times the column spread (theta: 1.04 +- 4.7e-4 in Planck)"""
    rng = np.random.default_rng(seed)
    sig = np.logspace(-3, 1, d)[rng.permutation(d)]
    A = np.eye(d) + 0.5 * rng.standard_normal((d, d)) / math.sqrt(d)
    Cn = A @ A.T
    Cn = Cn / np.outer(np.sqrt(np.diag(Cn)), np.sqrt(np.diag(Cn)))
    mean = sig * ratio * rng.uniform(-1.0, 1.0, d)
    mean[0] = sig[0] * ratio
    return sampled_chain(Cn * np.outer(sig, sig), n, seed + 1000, mean=mean)


def isotropic_chain(seed, n, blocks=(4, 5, 3, 6)):
    """near-repeated eigenvalues: the rows are recoloured so that their sample covariance is Q diag(lam) Q^T, with lam
    constant over blocks of the given sizes (10, 1, 0.1, ...) up to rounding -- isotropic eigen-spaces in which the
    eigenvectors are fixed by rounding alone, so only rotation-invariant quantities can be compared there."""
    rng = np.random.default_rng(seed)
    d = int(sum(blocks))
    lam = np.concatenate([np.full(b, 10.0 ** (1 - i)) for i, b in enumerate(blocks)])
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    z = rng.standard_normal((n, d))
    z -= z.mean(axis=0)
    z = z @ np.linalg.inv(np.linalg.cholesky(np.cov(z.T))).T
    rows = (z * np.sqrt(lam)) @ Q.T + rng.standard_normal(d)
    return _chain_from_rows(rows, z, rng)


def singular_chain(seed, n, d=5):
    """a column that is the sum of two others: singular by construction (rounding leaves it merely near-singular)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, d - 1))
    rows = np.column_stack([z, z[:, 0] + z[:, 1]])
    return _chain_from_rows(rows, z, rng)


# --------------------------------------------------------------------------------------------------------------------
# inputs chosen to stress the fp16 filter's bound (tests/test_gpu_parity.py, tests/test_gpu_adversarial.py): dynamic
# range, clustering far below the fp16 resolution of the extent, offsets, fp16 over/underflow before scaling
# --------------------------------------------------------------------------------------------------------------------
ADVERSARIAL = {            # name -> f(rng, n, d) -> rows
    "heavy_tails": lambda r, n, d: r.standard_t(1.5, size=(n, d)),
    "tight_clusters": lambda r, n, d: r.integers(0, 3, size=(n, 1)) * 1000.0 + 1e-3 * r.standard_normal((n, d)),
    "tiny_scale": lambda r, n, d: 1e-9 * r.standard_normal((n, d)),
    "huge_scale_offset": lambda r, n, d: 1e7 + 3e4 * r.standard_normal((n, d)),
    "anisotropic": lambda r, n, d: r.standard_normal((n, d)) * np.logspace(-4, 2, d)[None, :],
    "one_outlier": lambda r, n, d: np.vstack([r.standard_normal((n - 1, d)), np.full((1, d), 1e4)]),
    "lattice_ties": lambda r, n, d: r.integers(-3, 4, size=(n, d)).astype(float),
    "subnormal_fp16_coords": lambda r, n, d: np.hstack([r.standard_normal((n, 1)), 1e-6 * r.standard_normal((n, d - 1))]),
    "all_identical": lambda r, n, d: np.full((n, d), 3.25),
    "constant_column": lambda r, n, d: np.hstack([np.full((n, 1), -7.0), r.standard_normal((n, d - 1))]),
    "few_distinct": lambda r, n, d: r.standard_normal((5, d))[r.integers(0, 5, n)],
}


def _fp16_cell_straddlers(r, n, d):
    """64 clusters with centres of order 1 in the first three columns (1e-3 of that in the others), each 2^-14 of its centre
    wide: an eighth of the fp16 spacing there, so most clusters lie across a rounding boundary in some column and rows a
    small fraction of a cell apart differ by a whole cell once converted"""
    c = r.uniform(0.5, 1.0, size=(64, d)) * r.choice([-1.0, 1.0], size=(64, d))
    c[:, 3:] *= 1e-3
    lab = r.integers(0, 64, n)
    return c[lab] + 2.0 ** -14 * np.abs(c[lab]) * r.standard_normal((n, d))


#: kinds added with the every-row matrix (tests/test_gpu_adversarial.py); kept apart so that the older tests keep their cases
ADVERSARIAL_EXTRA = {
    "fp16_cell_straddlers": _fp16_cell_straddlers,
    # a lattice whose ties are broken by a jitter of 1e-4 of its spacing, below the fp16 resolution of the (mean-centred) coordinates:
    # nearly every row has its K-th and (K + 1)-th neighbours within 1e-4 relative -- a neighbour arriving when the threshold is
    # already tight passes the gate on its error terms alone -- and the order is the distances', not the row numbers'
    "jittered_lattice": lambda r, n, d: r.integers(-3, 4, size=(n, d)) + 1e-4 * r.standard_normal((n, d)),
}


def offset_clusters(S):
    """Three clusters S apart in column 0, each 1e-3 wide (tests/test_gpu_adversarial_f64.py): the input on which the fp64
    sweeps' refine margin matters.  The GEMM-form keys carry an absolute error that grows with S^2 while the neighbour
    spacings stay those of the 1e-3 clouds, so with S chosen just below the point where a row becomes key-ambiguous
    (offset_scale) many rows have one or two outsiders within the keys' error of the K-th neighbour, none has m + 1, and
    every row must come out exactly right."""
    return lambda r, n, d: r.integers(0, 3, (n, 1)) * S + 1e-3 * r.standard_normal((n, d))


#: the separations offset_clusters is tried at, largest first (offset_scale)
OFFSET_SCALES = (100, 30, 10, 3, 1)
#: kinds that need at least two columns
ADVERSARIAL_MIN2 = ("anisotropic", "subnormal_fp16_coords", "constant_column")


def _rows_cycled(A, n, rng=None):
    """n rows of A: a random choice without replacement while A has enough rows, cycled otherwise"""
    if rng is not None and n <= len(A):
        return A[rng.permutation(len(A))[:n]].copy()
    return A[np.arange(n) % len(A)].copy()


def _far_queries(r, nq, nr, d):
    Y = r.standard_normal((nr, d))
    X = _rows_cycled(Y, nq)
    X[:, 0] += 50.0
    return X, Y


def _query_outlier(r, nq, nr, d):
    Y = r.standard_normal((nr, d))
    X = r.standard_normal((nq, d))
    X[nq // 2] = 1e6
    return X, Y


def _queries_on_refs(r, nq, nr, d):
    Y = r.standard_normal((nr, d))
    return _rows_cycled(Y, nq, r), Y


#: separate query and reference sets (X != Y): name -> f(rng, nq, nr, d) -> (X, Y)
CROSS = {
    # every query outside the reference box, every K-th distance large
    "far_queries": _far_queries,
    # one query row at 1e6: the power-of-two scale puts every reference coordinate into fp16 subnormals
    "query_outlier_sets_scale": _query_outlier,
    # all references nearly equidistant from a query at fp16 resolution
    "refs_in_a_speck": lambda r, nq, nr, d: (10.0 * r.standard_normal((nq, d)), 5.0 + 1e-3 * r.standard_normal((nr, d))),
    # queries are copies of reference rows: the first distance is exactly 0 and the threshold reaches 0
    "queries_on_refs": _queries_on_refs,
    "lattice_queries": lambda r, nq, nr, d: (r.integers(-3, 4, size=(nq, d)).astype(float), r.standard_normal((nr, d))),
    "lattice_refs": lambda r, nq, nr, d: (r.standard_normal((nq, d)), r.integers(-3, 4, size=(nr, d)).astype(float)),
}
#: scale of the Gaussian partner of a one-set kind where a unit Gaussian makes neighbours that no fp64 reference can order: from
#: unit-Gaussian queries all rows of a 1e-9 cloud are equidistant to 1e-13 relative, and so are unit-Gaussian references from queries
#: at 1e7 (one row in a hundred / in a few thousand would be ambiguous) -- there the partner takes the kind's own spread
PARTNER_SCALE = {("tiny_scale", "refs"): 3e-9, ("huge_scale_offset", "queries"): 3e4}
for _kind, _gen in sorted({**ADVERSARIAL, **ADVERSARIAL_EXTRA}.items()):
    # every one-set kind as the queries of a Gaussian reference set, and as the references of Gaussian queries
    CROSS[_kind + "_as_queries"] = lambda r, nq, nr, d, _g=_gen, _s=PARTNER_SCALE.get((_kind, "queries"), 1.0): (
        _g(r, nq, d), _s * r.standard_normal((nr, d)))
    CROSS[_kind + "_as_refs"] = lambda r, nq, nr, d, _g=_gen, _s=PARTNER_SCALE.get((_kind, "refs"), 1.0): (
        _s * r.standard_normal((nq, d)), _g(r, nr, d))
del _kind, _gen
# the same two against a UNIT Gaussian partner, as the other kinds: only few queries and K = 1 stay under the cap of ambiguous rows
CROSS["tiny_scale_unit_refs"] = lambda r, nq, nr, d: (r.standard_normal((nq, d)), ADVERSARIAL["tiny_scale"](r, nr, d))
CROSS["huge_scale_offset_unit_queries"] = lambda r, nq, nr, d: (ADVERSARIAL["huge_scale_offset"](r, nq, d), r.standard_normal((nr, d)))


def needs_two_columns(kind):
    """a kind (one-set or cross) that is undefined at d = 1"""
    return kind in ADVERSARIAL_MIN2 or any(kind == k + s for k in ADVERSARIAL_MIN2 for s in ("_as_queries", "_as_refs"))


# --------------------------------------------------------------------------------------------------------------------
# kNN certificate: plain NumPy on the host, nothing shared with the library.
#   C1 rows        indices in [0, nr), distinct; the own row never reported (SELF_EXCLUDE) / first at distance 0 (SELF_INCLUDE)
#   C2 distances   dist[q, k] == the np.longdouble distance to row idx[q, k] within relative B; a true 0 is exactly 0;
#                  ascending, equal distances by ascending row
#   C3 complete    |dist[q, k] - od[q, k]| <= 2 B od[q, k] against the brute-force oracle asked for K + 1 neighbours
#   C4 same rows   idx[q] == oi[q, :K] on every row that is not ambiguous
# B = (D/2 + 2) 2^-53 is derived, not measured: each of the D differences carries a relative error u = 2^-53, its square
# 2u; a sum of D positive terms, in any order and with or without fma, adds at most D u; the square root halves the total
# ((3 + D) u / 2 < (D/2 + 1.5) u) and adds u of its own -- rounded up to (D/2 + 2) u.
# With C1 and C2, C3 proves the list a valid K-nearest set up to ties of relative width 3B.  A row is AMBIGUOUS when the
# oracle's own K + 1 distances hold an adjacent pair with 0 < gap <= 4B od[q, k + 1]: there two correct fp64 evaluations
# may order the pair differently, and the row is judged by C1 - C3 only.  Exact ties (gap == 0) are not ambiguous: both
# sides break them by row number.  At most AMBIGUOUS_CAP of the rows of a case may be ambiguous, which is checked on the
# oracle's output before the result under test is looked at.
#
# The fp64 sweeps (knn_mfma.hpp, knn_long.hpp) SELECT on GEMM-form keys and keep K + m entries (m = min(K + 2, 32) - K: the
# plan's kRefineMargin, 1 at K = 31, 0 at K = 32); the merge then reports the K nearest of them by exact direct differences.
# With `margin=m` the certificate judges that contract.
#
# E = key_bound: |key - d^2| <= E[q] = c(D) u (|a| + max_j |b_j|)^2, u = 2^-53, a = x - c and b = y - c the rows about the
# centre c the library subtracts (any c: d^2 = |a - b|^2 exactly), c(D) = 2 D + 4.  Derivation, from the kernels' arithmetic:
#   * centred coordinates: fl(x_i - c_i) = a_i (1 + e), |e| <= u, one rounding each (knn_mfma.hpp, long_pack_queries_kernel,
#     pack_refs_kernel); the factor -2 of the packed references is exact.  A product of two of them is off by 2 u |a_i b_i|, a
#     square by 2 u a_i^2.
#   * the two norms: one fma chain over the D squares (pack_refs_kernel, long_query_norms_kernel; knn_mfma.hpp adds four
#     chains of <= D/4 + 1 terms with two more additions: fewer roundings): at most D u |.|^2, with the squares' own error
#     (D + 2) u |a|^2 and (D + 2) u |b|^2.
#   * the MFMA chain of 4 KS terms seeded with |a|^2 adds the D products -2 a_i b_i and 1 * |b|^2; its padding terms are
#     0 * 0 and add exactly.  Each of the D + 1 non-zero terms enters the accumulator through one fused multiply-add: one
#     rounding of the partial sum, D + 1 in all.  Every partial sum is bounded by the sum of the terms' magnitudes,
#     |a|^2 + 2 sum |a_i b_i| + |b|^2 <= (|a| + |b|)^2 (Cauchy-Schwarz), so the chain adds at most (D + 1) u (|a| + |b|)^2
#     whatever the order of the terms -- the blocks of knn_long.hpp and the k-steps of knn_mfma.hpp alike.
#   * together: (D + 2) u (|a|^2 + |b|^2) + 4 u |a||b| + (D + 1) u (|a| + |b|)^2 <= (2 D + 3) u (|a| + |b|)^2, since
#     4 <= 2 (D + 2).  The terms of second order in u are below D^2 u times that; c(D) = 2 D + 4 covers them (and the
#     distance of NumPy's column mean from the library's, which moves |a| and |b| by parts in 1e12) for D <= 1024 with a
#     factor of (2 D + 3)^-1 >= 4.8e-4 to spare.  max_j runs over all references: no per-row sharpening is used.
#   Rows with identical coordinates get identical keys (an MFMA output element depends on its A row, B column and C-in only),
#   and equal keys are ordered by row, as the oracle orders equal distances.
# A row is KEY-AMBIGUOUS when a correct selection on keys within E of the truth may lose one of the true K.  A true
# neighbour i at position s of the oracle's order is lost only if K + m rows precede it in (key, row) order; the s rows
# before it in truth may, and otherwise only rows o with d_o^2 <= d_i^2 + 2 E whose coordinates differ from i's
# (key_o <= key_i needs d_o^2 - E <= d_i^2 + E).  So with the references collapsed to distinct points p_0, p_1, ... in
# the oracle's order, mult_j copies each, cum_j = mult_0 + ... + mult_j: the row is key-ambiguous iff for some j with
# cum_(j-1) < K:  min(cum_j, K) - 1 + sum of mult_j' over j' > j with d_j'^2 <= d_j^2 + 2 E  >=  K + m.  Without duplicate
# rows that is od[:, K + m]^2 - od[:, K - 1]^2 <= 2 E (both evaluated with the oracle's own 4B around them).
#   C3w            dist[q, k]^2 <= od[q, k]^2 (1 + 4B) + 2 E[q] for every k: what the K exact-nearest of the K + m key-nearest
#                  (the set S) satisfy.  Proof: take the true k + 1 nearest.  If one of them, t, is not in S, every member of S
#                  has key <= key_t, so d^2 <= d_t^2 + 2 E <= od_k^2 + 2 E for all K + m >= k + 1 of them; otherwise the k + 1
#                  are in S themselves.  Either way S holds k + 1 rows within od_k^2 + 2 E, and the (k + 1)-th smallest exact
#                  distance in S is no larger.  (The fp64 rounding of the refined and of the oracle's distance is the 4B; its
#                  product with 2 E is a part in 1e13 of E's spare.)
# With `margin`: rows neither oracle- nor key-ambiguous get C1 - C4, key-ambiguous rows C1, C2 and C3w, and in a strict case
# at most AMBIGUOUS_CAP of the rows may be ambiguous of either kind.  `weak=True` judges every row by C1, C2 and C3w, without
# a cap; WEAK lists the (kind, self class) pairs that need it, decided on the CPU alone
# (tests/test_oracle_certificate.py::test_weak_table_is_minimal_and_complete).
# --------------------------------------------------------------------------------------------------------------------
SELF_NONE, SELF_INCLUDE, SELF_EXCLUDE = 0, 1, 2
AMBIGUOUS_CAP = 1e-5
#: (kind, self class) judged weakly on the GEMM-form families; self classes: "one" (one buffer: exclude, include, none, shard),
#: "asq", "asr", "cross"
WEAK = frozenset({("tight_clusters", "one"), ("lattice_ties", "one")})


def cert_bound(D):
    return (0.5 * D + 2.0) * 2.0 ** -53


def key_bound_c(D):
    """c(D) of key_bound (derivation above)"""
    return 2.0 * D + 4.0


def key_bound(X, Y):
    """E[q]: absolute bound on |key - true d^2| of the fp64 sweeps' GEMM-form keys over every pair of query q (above)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    c = Y.mean(axis=0)
    na = np.sqrt(((X - c) ** 2).sum(axis=1))
    nb = np.sqrt(((Y - c) ** 2).sum(axis=1).max())
    return key_bound_c(X.shape[1]) * 2.0 ** -53 * (na + nb) ** 2


def refine_margin(K):
    """entries the fp64 sweeps keep beyond K (capi_plan.hpp: min(K + kRefineMargin, MCE_MAX_K) - K)"""
    return min(K + 2, 32) - K


def _key_ambiguous(X, Y, K, m, self_mode, self_offset, od, E):
    """mask of key-ambiguous rows (above); od: the oracle's K + m + 1 distances (fewer where the set ends)"""
    nq, D = X.shape
    B4 = 4.0 * cert_bound(D)
    if self_mode == SELF_INCLUDE and K == 1:
        return np.zeros(nq, dtype=bool)                        # (the own row alone: nothing is selected)
    Yu, inv, counts = np.unique(Y, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    if len(Yu) == len(Y):                                     # no duplicate rows: positions are points
        if od.shape[1] <= K + m:
            return np.zeros(nq, dtype=bool)                    # (fewer than K + m + 1 usable rows: every one is selected)
        return od[:, K + m] ** 2 * (1.0 - B4) <= od[:, K - 1] ** 2 * (1.0 + B4) + 2.0 * E
    # distinct points in the oracle's order; the own row (excluded, or reported apart) is no copy of its point
    P = min(K + m + 2, len(Yu))
    pd, pi = orc.knn_brute(X, np.ascontiguousarray(Yu), P, self_mode=0)
    mult = counts[pi].astype(np.int64)
    Kn = K
    if self_mode != SELF_NONE:
        mult -= pi == inv[self_offset + np.arange(nq)][:, None]
        if self_mode == SELF_INCLUDE:
            Kn = K - 1                                         # (the others: K - 1 of the K + m - 1 selected)
    if Kn < 1:
        return np.zeros(nq, dtype=bool)
    p2 = pd * pd
    cum = np.cumsum(mult, axis=1)
    amb = np.zeros(nq, dtype=bool)
    for j in range(P):
        before = cum[:, j] - mult[:, j]
        band = (p2[:, j + 1:] * (1.0 - B4) <= (p2[:, j] * (1.0 + B4) + 2.0 * E)[:, None])
        ahead = np.minimum(cum[:, j], Kn) - 1 + (mult[:, j + 1:] * band).sum(axis=1)
        amb |= (before < Kn) & (mult[:, j] > 0) & (ahead >= Kn + m)
    return amb


class CertificateError(AssertionError):
    """raised by knn_certificate; ``report`` is the per-row report"""

    def __init__(self, msg, report):
        super().__init__(msg)
        self.report = report


def oracle_lists(X, Y, K, self_mode, self_offset=0, margin=None, weak=False):
    """The oracle's side of the certificate: (od, oi, ambiguous) -- its K + 1 nearest (fewer where the reference set
    ends), in the order the library documents for ``self_mode``, and the mask of ambiguous rows.  Raises when more than
    AMBIGUOUS_CAP of the rows are ambiguous: such a case cannot judge anybody.
    ``margin=m`` (the fp64 sweeps: lists of K + m chosen on GEMM-form keys): K + m + 1 nearest, and the result is
    (od, oi, ambiguous, key_ambiguous, E) with E = key_bound(X, Y); the cap then counts rows ambiguous of either kind,
    unless ``weak`` (every row judged by C1, C2 and C3w: no cap)."""
    more = 1 if margin is None else margin + 1
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nq, D = X.shape
    nr = Y.shape[0]
    if self_mode == SELF_NONE:
        od, oi = orc.knn_brute(X, Y, min(K + more, nr), self_mode=0)
    elif self_mode == SELF_EXCLUDE:
        od, oi = orc.knn_brute(X, Y, min(K + more, nr - 1), self_mode=2, self_offset=self_offset)
    elif self_mode == SELF_INCLUDE:           # the own row first, at distance 0, whatever duplicates it has; then the others
        own = self_offset + np.arange(nq, dtype=np.int64)
        kk = min(K + more - 1, nr - 1)
        if kk > 0:
            od, oi = orc.knn_brute(X, Y, kk, self_mode=2, self_offset=self_offset)
        else:
            od, oi = np.empty((nq, 0)), np.empty((nq, 0), dtype=np.int64)
        od = np.column_stack([np.zeros(nq), od])
        oi = np.column_stack([own, oi])
    else:
        raise ValueError("self_mode %r" % (self_mode,))
    if od.shape[1] < K:
        raise ValueError("K = %d exceeds the usable reference rows" % K)
    gap = np.diff(od[:, :K + 1], axis=1)
    ambiguous = np.any((gap > 0) & (gap <= 4.0 * cert_bound(D) * od[:, 1:K + 1]), axis=1)
    if margin is None:
        either = ambiguous
    else:
        E = key_bound(X, Y)
        key_ambiguous = _key_ambiguous(X, Y, K, margin, self_mode, self_offset, od, E)
        either = ambiguous | key_ambiguous
    namb = int(either.sum())
    if namb > AMBIGUOUS_CAP * nq and not (weak and margin is not None):
        raise ValueError("%d of %d rows are ambiguous on the oracle alone (cap %g of the rows): first rows %s -- change the seed "
                         "or the input" % (namb, nq, AMBIGUOUS_CAP, np.flatnonzero(either)[:5].tolist()))
    if margin is None:
        return od, oi, ambiguous
    return od, oi, ambiguous, key_ambiguous, E


_LONGDOUBLE_OK = np.finfo(np.longdouble).eps < 2.0 ** -52


def _dist_within_bound(X, Y, idx, dist, B):
    """(ok, zero): per entry, whether dist[q, k] lies within relative B of the true distance from X[q] to Y[idx[q, k]],
    and whether that true distance is 0.  np.longdouble where it is wider than double (64-bit significand: its own
    error, (D + 2) 2^-64, is 2^-11 of B); exact rational arithmetic otherwise."""
    nq, K = idx.shape
    D = X.shape[1]
    ok = np.zeros((nq, K), dtype=bool)
    zero = np.zeros((nq, K), dtype=bool)
    if _LONGDOUBLE_OK:
        step = max(1, (1 << 21) // max(1, K * D))
        Bl = np.longdouble(B)
        for s in range(0, nq, step):
            e = min(nq, s + step)
            diff = X[s:e, None, :].astype(np.longdouble) - Y[idx[s:e]].astype(np.longdouble)
            t = np.sqrt((diff * diff).sum(-1))
            ok[s:e] = np.abs(dist[s:e].astype(np.longdouble) - t) <= Bl * t
            zero[s:e] = t == 0
        return ok, zero
    from fractions import Fraction
    lo, hi = (1 - Fraction(B)) ** 2, (1 + Fraction(B)) ** 2
    for q in range(nq):
        xq = [Fraction(v) for v in X[q].tolist()]
        for k in range(K):
            s2 = sum((a - Fraction(v)) ** 2 for a, v in zip(xq, Y[idx[q, k]].tolist()))
            g = dist[q, k]
            zero[q, k] = s2 == 0
            ok[q, k] = bool(np.isfinite(g)) and g >= 0 and lo * s2 <= Fraction(float(g)) ** 2 <= hi * s2
    return ok, zero


def knn_certificate(X, Y, K, dist, idx, self_mode, self_offset=0, kernel=None, oracle=None, max_report=8, margin=None, weak=False):
    """Certify a finished K-nearest search ``(dist, idx)`` of the queries X in the references Y, EVERY row (C1 - C4 above).
    Returns the report (dict: rows, K, B, ambiguous, ambiguous_rows, failures = []) or raises CertificateError whose message
    names the first failing rows, the check each failed and ``kernel`` (the caller's ``last_kernel()``); its ``report``
    lists every failure as (row, column, check, detail).  ``oracle``: a precomputed ``oracle_lists(...)`` of the same
    arguments (several searches of one input).
    ``margin=m``: the search selected K + m on GEMM-form keys and refined (the fp64 sweeps): key-ambiguous rows are judged by
    C1, C2 and C3w, and with ``weak`` every row is; the report also carries key_ambiguous and key_ambiguous_rows."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    nq, D = X.shape
    nr = Y.shape[0]
    B = cert_bound(D)
    # the reference first, and alone: how many rows it cannot judge
    if margin is None:
        assert not weak, "weak judges the margin contract: give margin"
        od, oi, ambiguous = oracle if oracle is not None else oracle_lists(X, Y, K, self_mode, self_offset)
        key_amb, E = np.zeros(nq, dtype=bool), None
    else:
        od, oi, ambiguous, key_amb, E = oracle if oracle is not None else oracle_lists(X, Y, K, self_mode, self_offset, margin=margin, weak=weak)
    relaxed = np.ones(nq, dtype=bool) if weak else key_amb      # rows judged by C1, C2 and C3w
    assert od.shape[0] == nq and od.shape[1] >= K
    dist = np.asarray(dist)
    idx = np.asarray(idx)
    assert dist.shape == (nq, K) and idx.shape == (nq, K), (dist.shape, idx.shape, (nq, K))
    assert dist.dtype == np.float64 and idx.dtype.kind in "iu"
    idx = idx.astype(np.int64)
    own = self_offset + np.arange(nq, dtype=np.int64)
    fails = {}              # (row, check) -> (column, detail): the first column of a row a check fails at

    def note(mask, check, detail):
        for q, k in zip(*np.nonzero(mask)):
            fails.setdefault((int(q), check), (int(k), detail(int(q), int(k))))

    # ---- C1
    inrange = (idx >= 0) & (idx < nr)
    note(~inrange, "C1 row out of range", lambda q, k: "idx=%d" % idx[q, k])
    safe = np.where(inrange, idx, 0)
    order = np.argsort(safe, axis=1, kind="stable")
    srt = np.take_along_axis(safe, order, axis=1)
    dup = np.zeros((nq, K), dtype=bool)                     # (marked at the list column of the later of two equal entries)
    np.put_along_axis(dup, order[:, 1:], srt[:, 1:] == srt[:, :-1], axis=1)
    note(dup, "C1 duplicate row", lambda q, k: "idx=%s" % idx[q].tolist())
    if self_mode == SELF_EXCLUDE:
        note(idx == own[:, None], "C1 own row reported", lambda q, k: "idx=%s" % idx[q].tolist())
    elif self_mode == SELF_INCLUDE:
        first = np.zeros((nq, K), dtype=bool)
        first[:, 0] = (idx[:, 0] != own) | (dist[:, 0] != 0.0)
        note(first, "C1 own row not first at distance 0", lambda q, k: "idx=%d dist=%r" % (idx[q, 0], dist[q, 0]))
    # ---- C2
    finite = np.isfinite(dist) & (dist >= 0)
    note(~finite, "C2 distance not finite", lambda q, k: "dist=%r" % dist[q, k])
    ok, zero = _dist_within_bound(X, Y, safe, np.where(finite, dist, 0.0), B)
    note(inrange & finite & ~ok, "C2 distance off its row's", lambda q, k: "dist=%r to row %d" % (dist[q, k], idx[q, k]))
    note(inrange & zero & (dist != 0.0), "C2 zero distance not exact", lambda q, k: "dist=%r to row %d" % (dist[q, k], idx[q, k]))
    desc = np.zeros((nq, K), dtype=bool)
    desc[:, 1:] = dist[:, 1:] < dist[:, :-1]
    note(desc, "C2 not ascending", lambda q, k: "dist=%r after %r" % (dist[q, k], dist[q, k - 1]))
    tie = np.zeros((nq, K), dtype=bool)
    tie[:, 1:] = (dist[:, 1:] == dist[:, :-1]) & (idx[:, 1:] < idx[:, :-1])
    if self_mode == SELF_INCLUDE and K > 1:
        tie[:, 1] = False                                      # (the own row leads whatever duplicates it has)
    note(tie, "C2 tie not by ascending row", lambda q, k: "rows %d, %d at %r" % (idx[q, k - 1], idx[q, k], dist[q, k]))
    # ---- C3
    odk = od[:, :K]
    note(~(np.abs(np.where(finite, dist, np.inf) - odk) <= 2.0 * B * odk) & ~relaxed[:, None], "C3 not the K nearest",
         lambda q, k: "dist=%r oracle=%r (row %d, oracle row %d)" % (dist[q, k], od[q, k], idx[q, k], oi[q, k]))
    if margin is not None:
        # ---- C3w
        note(~(np.where(finite, dist, np.inf) ** 2 <= odk * odk * (1.0 + 4.0 * B) + 2.0 * E[:, None]) & relaxed[:, None],
             "C3w beyond the K nearest by more than the keys' error",
             lambda q, k: "dist^2=%r oracle^2=%r 2E=%r (row %d, oracle row %d)" % (dist[q, k] ** 2, od[q, k] ** 2, 2.0 * E[q], idx[q, k], oi[q, k]))
    # ---- C4
    note((idx != oi[:, :K]) & ~ambiguous[:, None] & ~relaxed[:, None], "C4 rows differ from the oracle's",
         lambda q, k: "row %d, oracle row %d at %r / %r" % (idx[q, k], oi[q, k], dist[q, k], od[q, k]))

    failures = sorted((q, k, c, t) for (q, c), (k, t) in fails.items())
    report = dict(rows=nq, K=K, B=B, ambiguous=int(ambiguous.sum()), ambiguous_rows=np.flatnonzero(ambiguous), failures=failures,
                  failed_rows=sorted({f[0] for f in failures}), kernel=kernel, key_ambiguous=int(key_amb.sum()),
                  key_ambiguous_rows=np.flatnonzero(key_amb), weak=weak)
    if failures:
        lines = ["row %d column %d: %s (%s)" % f for f in failures[:max_report]]
        raise CertificateError("kNN certificate failed on %d of %d rows (nq=%d nr=%d d=%d K=%d self_mode=%d self_offset=%d, "
                               "%d ambiguous rows); kernel: %s\n  %s" % (len(report["failed_rows"]), nq, nq, nr, D, K, self_mode, self_offset,
                                                                     report["ambiguous"], kernel, "\n  ".join(lines)), report)
    return report


# --------------------------------------------------------------------------------------------------------------------
# Sum certificate: the evidence sums dotp[k] = sum_q sign(w_q) exp(lnC_D + D ln r_qk - ln |w_q| + fs_q) of the fused and
# partitioned entry points (mce_knn_dotp_*), judged against np.longdouble on inputs where EVERY row counts.  w and fs are free
# inputs: equalised_inputs() sets fs_q = -D ln od[q, col] + u_q, u_q in (-1, 0], so that every term of column `col` is of order 1
# (C_D / w e^u) whatever the data's dynamic range -- one wrong neighbour on one row then moves the sum by a share of 1 / n, not by
# a share of nothing.  Plain NumPy on the host, nothing shared with the library.
#
# T_k = sum_bound(): the tolerance on column k, derived from the kernel's arithmetic (reduce_kernels.hpp), u = 2^-53, not measured:
#   * the squared distance: the refined (merge_lists_kernel: one fma chain over the D squared differences) or filter-exact d^2 is
#     within 2B relative, B = (D/2 + 2) u as derived above cert_bound for its square root (without the root's halving and rounding).
#   * the exponent a = lnC - ln |w| + fs + (D/2) ln d^2 (`base + 0.5 * D * log(d2)`):  ln (d^2 (1 + 2B)) moves by 2B, times D/2: D B.
#     log |w| is off by L_log u |ln |w||, log d^2 by L_log u |ln d^2| (times D/2; 0.5 * D is exact); `lnc - log|w|` rounds once
#     (u (|lnC| + |ln |w||)), `+ fs` once (u (|lnC| + |ln |w|| + |fs|)), the product `0.5 D * log d2` once (u (D/2) |ln d^2|), the
#     last addition once (u |a|).  With amax = max over the rows of |lnC| + |ln |w|| + |fs| + (D/2) |ln d^2| -- the SUM of the
#     magnitudes, not |a|: the equalised fs cancels against the volume term -- the four roundings stay below 3 u amax and the two
#     logarithms below L_log u amax:  |delta a| <= D B + (L_log + 3) u amax.
#     lnC itself comes from the host (capi_search.hpp ln_unit_ball: 0.5 d log(pi) - lgamma(1 + d/2) in double): a product and a
#     logarithm of 1 ulp, glibc's stated 4 ulp on lgamma, one subtraction -- below 5 u ((D/2) ln pi + |ln Gamma(1 + D/2)|), added to
#     delta a (the truth takes lnC from exact factorials in np.longdouble).
#   * the term t = sign(w) exp(a) is therefore within  delta a (1 + delta a) + L_exp u  relative.
#   * the summation: a fixed tree, in which a term passes through 6 additions of wave_sum and 4 of block_sum in the merge (or
#     dotp_partial_kernel), at most ceil(blocks / 256) = ceil(n / 65536) additions of the strided pass of dotp_final_kernel and 10
#     more of its block_sum, then the host's addition of the W parts: every partial sum is bounded by A_k = sum_q |t_qk|, so the
#     tree adds at most (ceil(n / 65536) + 20 + W) u A_k (n: the query rows of the call; a part's launch covers fewer).
#   * the unfused dotp_partial_kernel takes D ln r from r = sqrt(d^2): one more rounding of r, times D (`unfused=True`; the d^2
#     term stays: the distances it is given are an exact search's, within B).
#   T_k = [delta a (1 + delta a) + L_exp u + (ceil(n / 65536) + 20 + W) u] A_k (1 + 2^-20)
# L_log, L_exp: the ulp errors of the device's double log and exp.  No document shipped with the ROCm installation states them
# (searched: share/doc, share/html); SUM_LOG_ULP = SUM_EXP_ULP = 2 is taken, twice the 1 ulp the HIP math reference is believed to
# state.  The choice is not delicate: the effects to be seen are >= 1e-10 A_k, the bound comes out at 1e-14 ... 1e-12 A_k.
#
# A row is BLIND when taking its next neighbour instead (od[q, c] -> od[q, c + 1] at the equalised column c) changes that
# column's sum by more than 0 and at most 2 T: a result within T of a sum that is wrong by that much passes.  Exact ties
# (change == 0) are not blind: either row is a valid answer.  Counted on the oracle alone before the library is called; a case with
# more than AMBIGUOUS_CAP of its rows blind is refused.
# --------------------------------------------------------------------------------------------------------------------
SUM_LOG_ULP = 2.0
SUM_EXP_ULP = 2.0
_LD = np.longdouble
_LD_PI = 4 * np.arctan(_LD(1))


def ln_unit_ball_ld(D):
    """ln (pi^(D/2) / Gamma(1 + D/2)) in np.longdouble; Gamma from its recurrence down to Gamma(1) = 1 or Gamma(1/2) = sqrt(pi)"""
    x, lg = _LD(D) / 2, _LD(0)
    while x > 0:
        lg += np.log(x)
        x -= 1
    if D % 2:
        lg += np.log(_LD_PI) / 2
    return _LD(D) / 2 * np.log(_LD_PI) - lg


def exact_distances(X, Y, oi):
    """np.longdouble distances from X[q] to the rows Y[oi[q, :]] (the oracle's rows; its own fp64 distances are rounded)"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    out = np.empty(oi.shape, dtype=_LD)
    step = max(1, (1 << 21) // max(1, oi.shape[1] * X.shape[1]))
    for s in range(0, len(X), step):
        diff = X[s:s + step, None, :].astype(_LD) - Y[oi[s:s + step]].astype(_LD)
        out[s:s + step] = np.sqrt((diff * diff).sum(-1))
    return out


def _ln_terms(od, w, fs, D):
    """(ln |t| [nq, cols] in np.longdouble, -inf where the term is exactly 0; sign(w) [nq, 1])"""
    od = np.asarray(od, dtype=_LD)
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = ln_unit_ball_ld(D) + _LD(D) * np.log(od) - np.log(np.abs(w.astype(_LD)))[:, None] + np.asarray(fs, dtype=_LD)[:, None]
    ln[(od == 0) | np.isneginf(np.asarray(fs, dtype=np.float64))[:, None]] = -np.inf
    return ln, np.where(w < 0, _LD(-1), _LD(1))[:, None]


def equalised_inputs(od, D, col, rng, nspecial=3):
    """(w, fs) for the oracle's distances od[nq, >= col + 1]: w from the integers 1 .. 5, fs_q = -D ln od[q, col] + u_q with
    u_q in (-1, 0] (fs_q = u_q where od[q, col] == 0); three rows dealt by rng get fs = -inf, three others a negative weight
    (``nspecial`` of each: a set of a handful of rows asks for fewer, so that some row still counts)."""
    od = np.asarray(od, dtype=_LD)
    nq = od.shape[0]
    w = rng.integers(1, 6, nq).astype(np.float64)
    u = -rng.random(nq)
    r = od[:, col]
    with np.errstate(divide="ignore"):
        fs = np.where(r > 0, -_LD(D) * np.log(np.where(r > 0, r, _LD(1))), _LD(0)) + u
    fs = np.asarray(fs, dtype=np.float64)
    special = rng.permutation(nq)[:2 * nspecial]
    fs[special[:nspecial]] = -np.inf
    w[special[nspecial:]] *= -1.0
    return w, fs


def sum_truth(od, w, fs, D, k0, kmax):
    """(S, A): S[k] = sum_q t_qk and A[k] = sum_q |t_qk| for k0 <= k < kmax (0 below k0), t = sign(w) exp(lnC_D + D ln r - ln |w| + fs)
    in np.longdouble in the log domain; od[:, k - k0] is the distance of reference column k (further columns are ignored)."""
    ln, sgn = _ln_terms(np.asarray(od)[:, :kmax - k0], w, fs, D)
    t = np.exp(ln)
    S, A = np.zeros(kmax, dtype=_LD), np.zeros(kmax, dtype=_LD)
    S[k0:] = (sgn * t).sum(axis=0)
    A[k0:] = t.sum(axis=0)
    return S, A


def sum_amax(od, w, fs, D, k0, kmax):
    """the largest |lnC| + |ln |w|| + |fs| + D |ln r| over the terms that are not exactly 0 (0.0 if there is none)"""
    od = np.asarray(od, dtype=_LD)[:, :kmax - k0]
    fs = np.asarray(fs, dtype=np.float64)
    live = (od > 0) & np.isfinite(fs)[:, None]
    if not live.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (abs(ln_unit_ball_ld(D)) + np.abs(np.log(np.abs(np.asarray(w, dtype=_LD))))[:, None] + np.abs(fs.astype(_LD))[:, None]
             + _LD(D) * np.abs(np.log(np.where(live, od, _LD(1)))))
    return float(np.max(np.where(live, m, 0)))


def sum_bound(D, n, A, amax, W=1, unfused=False):
    """T[k]: the tolerance on |S_hat[k] - S[k]| (derivation above); n: query rows, W: parts added on the host"""
    u = 2.0 ** -53
    B = cert_bound(D)
    lnpi_half = 0.5 * D * math.log(math.pi)
    da = D * B + (SUM_LOG_ULP + 3.0) * u * amax + 5.0 * u * (lnpi_half + abs(math.lgamma(1.0 + 0.5 * D)))
    if unfused:
        da += D * u
    rel = da * (1.0 + da) + SUM_EXP_ULP * u + (math.ceil(n / 65536.0) + 20 + W) * u
    return np.asarray(A, dtype=_LD) * _LD(rel * (1.0 + 2.0 ** -20))


def blind_rows(od, w, fs, D, c, T):
    """mask of the rows whose next neighbour at list column c (od[q, c] -> od[q, c + 1]) changes the column's sum by more than 0
    and at most 2 T (T: sum_bound of that column); rows without a next neighbour are not blind"""
    od = np.asarray(od, dtype=_LD)
    if od.shape[1] <= c + 1:
        return np.zeros(od.shape[0], dtype=bool)
    ln, _ = _ln_terms(od[:, c:c + 2], w, fs, D)
    t = np.exp(ln)
    eff = np.abs(t[:, 1] - t[:, 0])
    return (eff > 0) & (eff <= 2 * _LD(T))


def sum_oracle(od, D, k0, kmax, first, rng, n=None, W=1, unfused=False, nspecial=3):
    """The oracle's side of the sum certificate, before the library is called.  od: np.longdouble distances, kmax - k0 + 1 columns
    (fewer where the set ends).  first: equalise the FIRST list column (a wrong nearest neighbour seen with the power the last
    column gives a wrong K-th) -- unless a term of another column would then overflow, which falls back to the last.
    nspecial: the rows of each special kind (equalised_inputs).
    -> dict(w, fs, S, A, T, amax, col (list column equalised), blind (rows), rows); raises ValueError above AMBIGUOUS_CAP."""
    od = np.asarray(od, dtype=_LD)
    nq, K = od.shape[0], kmax - k0
    state = rng.bit_generator.state
    for c in ((0, K - 1) if first else (K - 1,)):
        rng.bit_generator.state = state
        w, fs = equalised_inputs(od, D, c, rng, nspecial)
        ln, _ = _ln_terms(od[:, :K], w, fs, D)
        if c == K - 1 or float(ln.max()) < 700.0:
            break
    S, A = sum_truth(od, w, fs, D, k0, kmax)
    amax = sum_amax(od, w, fs, D, k0, kmax)
    T = sum_bound(D, nq if n is None else n, A, amax, W=W, unfused=unfused)
    blind = blind_rows(od, w, fs, D, c, T[k0 + c])
    if int(blind.sum()) > AMBIGUOUS_CAP * nq:
        raise ValueError("%d of %d rows are blind to the sum certificate (cap %g of the rows): first rows %s" % (
            int(blind.sum()), nq, AMBIGUOUS_CAP, np.flatnonzero(blind)[:5].tolist()))
    return dict(w=w, fs=fs, S=S, A=A, T=T, amax=amax, col=c, blind=int(blind.sum()), blind_rows=np.flatnonzero(blind), rows=nq)


def sum_certificate(S_hat, S, A, T, k0, what=""):
    """|S_hat[k] - S[k]| <= T[k] for k >= k0, S_hat[k] == 0 exactly where A[k] == 0 and for k < k0, every entry finite.
    Returns the largest |S_hat - S| / T over the columns with T > 0 (0.0 if none)."""
    S_hat = np.asarray(S_hat)
    assert S_hat.dtype == np.float64 and S_hat.shape == np.shape(S), (S_hat.dtype, S_hat.shape)
    assert np.all(np.isfinite(S_hat)), "sum certificate: not finite: %s %s" % (S_hat.tolist(), what)
    assert np.all(S_hat[:k0] == 0.0), "sum certificate: columns below k0 = %d not 0: %s %s" % (k0, S_hat[:k0].tolist(), what)
    err = np.abs(S_hat.astype(_LD) - S)
    worst = 0.0
    for k in range(k0, len(S_hat)):
        if A[k] == 0:
            assert S_hat[k] == 0.0, "sum certificate: column %d must be exactly 0 (every term is), got %r %s" % (k, S_hat[k], what)
            continue
        assert err[k] <= T[k], "sum certificate: column %d: |S_hat - S| = %.3g > T = %.3g (%.3g T; S = %.17g, S_hat = %.17g, A = %.6g) %s" % (
            k, float(err[k]), float(T[k]), float(err[k] / T[k]), float(S[k]), S_hat[k], float(A[k]), what)
        worst = max(worst, float(err[k] / T[k]))
    return worst


def kd_partition_shares(capi, Yd, n, d, kmax, W, wd, fd, ws, wsb):
    """The distributed k-d preparation of a pruned auto-evidence search on W ranks, run one after the other on this GPU with the
    exchange emulated (tests/test_gpu_parity.py::test_distributed_kd_preparation_is_the_single_gpu_order): every rank's
    mce_prune_part_prepare_dev, the all-reduce(SUM) of the permutation arrays, then per rank its share with the replicated
    preparation (mce_knn_dotp_part_f64_dev), the summed permutation copied back, and its share on that shared order
    (mce_knn_dotp_part_prepared_f64_dev).  Yd, wd, fd, ws: torch tensors on the device.
    -> dict(ranges [(off, cnt, lo, hi)], perms, total, single, replicated [W arrays], prepared [W arrays])"""
    import torch
    ranges, perms = [], []
    for r in range(W):
        off, cnt, lo, hi = capi.prune_part_prepare_dev(Yd.data_ptr(), n, d, kmax, r, W, ws.data_ptr(), wsb, 0, want_range=True)
        torch.cuda.synchronize()
        ranges.append((off, cnt, lo, hi))
        perms.append(ws[off:off + 4 * cnt].view(torch.int32).clone())
    total = torch.stack(perms).sum(dim=0)
    # reference order: the replicated preparation
    ref = torch.zeros(kmax, dtype=torch.float64, device="cuda")
    capi.knn_dotp_part_dev(Yd.data_ptr(), n, d, kmax, 0, W, wd.data_ptr(), fd.data_ptr(), ref.data_ptr(), ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    single = ws[off:off + 4 * cnt].view(torch.int32).clone()
    replicated, prepared = [], []
    for r in range(W):
        rep = torch.zeros(kmax, dtype=torch.float64, device="cuda")
        capi.knn_dotp_part_dev(Yd.data_ptr(), n, d, kmax, r, W, wd.data_ptr(), fd.data_ptr(), rep.data_ptr(), ws.data_ptr(), wsb, 0)
        torch.cuda.synchronize()
        ws[off:off + 4 * cnt].view(torch.int32).copy_(total)            # what the all-reduce hands every rank
        got = torch.zeros(kmax, dtype=torch.float64, device="cuda")
        capi.knn_dotp_part_prepared_dev(Yd.data_ptr(), n, d, kmax, r, W, wd.data_ptr(), fd.data_ptr(), got.data_ptr(), ws.data_ptr(), wsb, 0)
        torch.cuda.synchronize()
        replicated.append(rep)
        prepared.append(got)
    return dict(ranges=ranges, perms=perms, total=total, single=single, replicated=replicated, prepared=prepared)
