"""The oracle and the cases of ``covariance=`` (docs/design/tension.md): the rule of mcevidence_amd/csrc/param_cov.hpp in exact integer
arithmetic (the fp64 inputs scaled by a power of two), the bound every fp64 route is held to, and the smallest inputs at which each
pass can go wrong.  Shared by tests/test_param_cov_shared.py (CPU) and tests/test_gpu_param_cov.py (GPU); every case is built once per
process, when it is first asked for.

The bounds (nothing in them is fitted to output), with eps = 2^-52, n the used rows, M1_i = sum|a x_i| / W and
M2_ij = sum a |x_i - m_i| |x_j - m_j| / W about the exact mean:

    |dm_i|  <= 2 n eps M1_i                                          (summary.md)
    |dW|    <= (n - 1) eps W,   |dess| <= 3 n eps ess                 (summary.md)
    |dC_ij| <= 2 (n + 3) eps M2_ij + (2 n eps)^2 M1_i M1_j + U_ij
    |dsd_j| <= 2 eps sd_j   against sqrt of the route's own C_jj

U_ij = 2^-1074 (n (1 + max(Y_i, Y_j) max(1, a_max)) / W + 1), Y_i = max_r |x_ri - m_i|, is the underflow floor: a product that lands
in the denormal range is rounded with an ABSOLUTE error of at most 2^-1074 whatever its size, the weight product, the term and the
quotient each once; it is below 1e-300 for columns of order one, about 1e-173 for pairs with the +-1e150 column of case D (far below those entries'
own bounds), and only matters to the denormal columns of case D.
"""
import functools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
TINY = 2.0 ** -1074


def _ints(v):
    """exact integers V and K with v[i] == V[i] / 2^K"""
    ratios = [float(x).as_integer_ratio() for x in v]
    K = max([den.bit_length() - 1 for _, den in ratios] + [0])
    return [num * ((1 << K) // den) for num, den in ratios], K


def _float(fr):
    try:
        return float(fr)
    except OverflowError:
        return float("inf") if fr > 0 else float("-inf")


def exact(a, x):
    """the rule in exact arithmetic on the rows with a != 0 (a status-0 system) -> dict: W, A2, ess, rows, mean[d], cov[d][d], M1[d],
    M2[d][d], Y[d], amax.  The sums are integer sums: in int64 where the scaled values are small enough for every sum to fit, in
    Python integers otherwise."""
    a = np.asarray(a, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(a.size, -1)
    use = a != 0.0
    a, x = a[use], x[use]
    n, d = x.shape
    A, Ka = _ints(a)
    Wi = sum(A)
    W = Fraction(Wi, 1 << Ka)
    A2 = Fraction(sum(v * v for v in A), 1 << (2 * Ka))
    cols = [_ints(x[:, j]) for j in range(d)]
    Kx = [k for _, k in cols]
    amax_i = max(abs(v) for v in A)
    xmax_i = max([abs(v) for X, _ in cols for v in X] + [1])
    small = amax_i * xmax_i * xmax_i * n < (1 << 62)
    if small:
        Am = np.array(A, dtype=np.int64)
        Xm = np.array([X for X, _ in cols], dtype=np.int64).T                       # [n, d]
        S1 = [int(v) for v in (Am[:, None] * Xm).sum(axis=0)]
        S2 = (Xm.T @ (Am[:, None] * Xm)).astype(object)
        S1abs = [int(v) for v in (Am[:, None] * np.abs(Xm)).sum(axis=0)]
    else:
        S1 = [sum(u * v for u, v in zip(A, X)) for X, _ in cols]
        S1abs = [sum(u * abs(v) for u, v in zip(A, X)) for X, _ in cols]
        S2 = np.zeros((d, d), dtype=object)
        for i in range(d):
            AX = [u * v for u, v in zip(A, cols[i][0])]
            for j in range(i, d):
                S2[i, j] = sum(u * v for u, v in zip(AX, cols[j][0]))
    m = [Fraction(S1[j], Wi << Kx[j]) for j in range(d)]
    out = dict(W=float(W), A2=float(A2), ess=float(W * W / A2), rows=n, mean=np.array([_float(v) for v in m]), cov=np.zeros((d, d)),
               M1=np.array([_float(Fraction(S1abs[j], Wi << Kx[j])) for j in range(d)]), amax=float(np.max(np.abs(a))) if n else 0.0)
    for i in range(d):
        for j in range(i, d):
            out["cov"][i, j] = out["cov"][j, i] = _float(Fraction(int(S2[i, j]), Wi << (Kx[i] + Kx[j])) - m[i] * m[j])
    # |x - m| about the exact mean, to 2 eps: the mean as a double and the remainder
    hi = out["mean"]
    lo = np.array([_float(m[j] - Fraction(float(hi[j]))) if np.isfinite(hi[j]) else 0.0 for j in range(d)])
    with np.errstate(all="ignore"):
        y = np.abs((x - hi[None, :]) - lo[None, :])
        out["M2"] = (y.T @ (a[:, None] * y)) / out["W"]
        out["Y"] = y.max(axis=0) if n else np.zeros(d)
    return out


def bounds(ex):
    n = ex["rows"]
    bm = 2.0 * n * EPS * ex["M1"]
    with np.errstate(all="ignore"):
        floor = TINY * (n * (1.0 + np.maximum(ex["Y"][:, None], ex["Y"][None, :]) * max(1.0, ex["amax"])) / ex["W"] + 1.0)
        return dict(mean=bm, cov=2.0 * (n + 3) * EPS * ex["M2"] + bm[:, None] * bm[None, :] + floor, ess=3.0 * n * EPS * ex["ess"],
                    W=(n - 1) * EPS * ex["W"])


class Case(object):
    """one system: a (weights), x (rows, [n, ld] with d measured columns), the exact values and the bounds"""

    def __init__(self, name, a, x, d=None):
        self.name = name
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.a.size, -1)
        self.d = self.x.shape[1] if d is None else int(d)
        self.exact = exact(self.a, self.x[:, :self.d])
        self.bound = bounds(self.exact)

    @property
    def system(self):
        """what ``_capi.param_cov`` takes"""
        return (self.x, self.d, self.a)


def check(case, got, what=""):
    """``got``: a block dict (``covariance.measure`` / ``covariance.from_block``).  Prints the largest error / bound, asserts every value
    within its bound and the matrix symmetric"""
    ex, b = case.exact, case.bound
    assert got["status"] == 0 and got["column"] == -1 and got["rows"] == ex["rows"], (case.name, got["status"], got["column"], got["rows"])
    cov = np.asarray(got["cov"])
    assert cov.shape == (case.d, case.d) and np.array_equal(cov, cov.T), case.name
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(got["mean"])), case.name
    ess = got["W"] * got["W"] / got["A2"]
    r = {"W": abs(got["W"] - ex["W"]) / max(b["W"], 5e-324), "ess": abs(ess - ex["ess"]) / b["ess"]}
    with np.errstate(all="ignore"):
        r["mean"] = float(np.max(np.abs(got["mean"] - ex["mean"]) / np.maximum(b["mean"], 5e-324)))
        r["cov"] = float(np.max(np.abs(cov - ex["cov"]) / np.maximum(b["cov"], 5e-324)))
    print("%s %-18s n=%-5d d=%-3d error/bound: W %.3g  ess %.3g  mean %.3g  cov %.3g" % (what, case.name, ex["rows"], case.d, r["W"], r["ess"], r["mean"], r["cov"]))
    assert all(v <= 1.0 for v in r.values()), (case.name, r)
    return r


def check_info(case, inf, what=""):
    """``info["covariance"]`` -> ``check`` on its block, then sd and corr: sd_j = sqrt(C_jj) of the dict's own C within 2 eps sd, corr by
    first-order propagation from C's bounds: |dcorr_ij| <= b_ij / (sd_i sd_j) + |corr_ij| (b_ii / (2 C_ii) + b_jj / (2 C_jj)) + 4 eps"""
    with np.errstate(all="ignore"):
        A2 = inf["sum_w"] ** 2 / inf["ess"]
    r = check(case, dict(W=inf["sum_w"], A2=A2, rows=inf["rows"], status=inf["status"], column=inf["column"], mean=inf["mean"], cov=inf["cov"]), what)
    cov, sd, corr = np.asarray(inf["cov"]), np.asarray(inf["sd"]), np.asarray(inf["corr"])
    assert np.all(np.abs(sd - np.sqrt(np.diagonal(cov))) <= 2.0 * EPS * sd), case.name
    ex, b = case.exact["cov"], case.bound["cov"]
    esd = np.sqrt(np.diagonal(ex))
    pos = sd > 0.0
    assert np.array_equal(np.diagonal(corr)[pos], np.ones(int(pos.sum()))) and np.isnan(np.diagonal(corr)[~pos]).all(), case.name
    ok = (esd[:, None] > 0.0) & (esd[None, :] > 0.0) & pos[:, None] & pos[None, :]
    with np.errstate(all="ignore"):
        ecorr = ex / (esd[:, None] * esd[None, :])
        rel = np.diagonal(b) / (2.0 * np.diagonal(ex))
        bc = b / (esd[:, None] * esd[None, :]) + np.abs(ecorr) * (rel[:, None] + rel[None, :]) + 4.0 * EPS
        rc = np.abs(corr - ecorr) / bc
    if ok.any():
        # (first order: only where C's own bounds are small against C_ii and C_jj)
        ok &= (rel[:, None] < 1e-3) & (rel[None, :] < 1e-3)
    if ok.any():
        print("%s %-18s corr error/bound %.3g" % (what, case.name, float(np.max(rc[ok]))))
        assert np.all(rc[ok] <= 1.0), (case.name, float(np.max(rc[ok])))
    assert np.isnan(corr[~(pos[:, None] & pos[None, :])]).all(), case.name
    return r


def _quantised(rng, n, d, bits=12):
    """standard normal columns of graded scale, on a grid of 2^-bits: every exact sum of the oracle fits int64"""
    x = rng.standard_normal((n, d)) * (1.0 + np.arange(d) % 16)[None, :]
    return np.round(x * (1 << bits)) / (1 << bits)


CPU_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 1025)


@functools.lru_cache(maxsize=None)
def cpu_cases():
    """n in CPU_SIZES x {unit, integer, fractional weights} at d = 3 on unquantised values (the oracle's Python-integer path); d = 17 on
    the grid; d = 127 at n <= 65"""
    rng = np.random.default_rng(4242)
    out = []
    for n in CPU_SIZES:
        for kind in ("unit", "integer", "fractional"):
            a = np.ones(n) if kind == "unit" else (rng.integers(1, 5, size=n).astype(np.float64) if kind == "integer" else rng.uniform(0.05, 3.0, size=n))
            x = rng.standard_normal((n, 3)) @ np.array([[1.0, 0.5, -0.25], [0.0, 2.0, 0.75], [0.0, 0.0, 0.1]]) + np.array([3.0, -40.0, 0.5])
            out.append(Case("%s_%d" % (kind, n), a, x))
        out.append(Case("grid17_%d" % n, rng.integers(1, 5, size=n).astype(np.float64), _quantised(rng, n, 19), d=17))
    for n in (1, 5, 65):
        out.append(Case("grid127_%d" % n, rng.integers(1, 5, size=n).astype(np.float64), _quantised(rng, n, 127)))
    return out


GPU_EDGE_N = (1, 2, 3, 4, 5, 63, 64, 65, 511, 512, 513, 1025)
GPU_EDGE_D = (1, 15, 16, 17, 27, 112, 113, 127)


def _structure(rng, n):
    """D: two identical columns, a negated copy, a constant column, +-1e150 beside +-1e-150"""
    base = rng.standard_normal(n)
    return np.stack([base, base.copy(), -base, np.full(n, 2.5), 1e150 * rng.choice([-1.0, 1.0], size=n), 1e-150 * rng.choice([-1.0, 1.0], size=n),
                     rng.standard_normal(n)], axis=1)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """A .. D and the systems F mixes: name -> Case"""
    rng = np.random.default_rng(31337)
    cases = []
    for d in (17, 127):                                  # A: weights 1..4, ld = d + 2
        for n in GPU_EDGE_N:
            cases.append(Case("A_%d_%d" % (n, d), rng.integers(1, 5, size=n).astype(np.float64), _quantised(rng, n, d + 2), d=d))
    for d in GPU_EDGE_D:
        if d not in (17, 127):
            cases.append(Case("A_513_%d" % d, rng.integers(1, 5, size=513).astype(np.float64), _quantised(rng, 513, d + 2), d=d))
    x = 50.0 + 1e-6 * rng.choice([-1.0, 1.0], size=(1000, 3))
    cases.append(Case("B_centring", rng.integers(1, 5, size=1000).astype(np.float64), x))
    n = 700
    a = rng.uniform(0.05, 3.0, size=n)
    x = rng.standard_normal((n, 5))
    zero = np.arange(n) % 5 == 2                         # a fifth of the rows: weight 0 over NaN / +-inf values
    a[zero] = 0.0
    x[zero] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=(int(zero.sum()), 5))
    cases.append(Case("C_skipped", a, x))
    cases.append(Case("D_structure", rng.integers(1, 5, size=600).astype(np.float64), _structure(rng, 600)))
    x = np.stack([rng.integers(-40, 41, size=600) * 5e-324, rng.integers(-3, 4, size=600) * 2.5e-310, rng.standard_normal(600)], axis=1)
    cases.append(Case("D_denormal", rng.integers(1, 5, size=600).astype(np.float64), x))
    # F: five systems of three (d, ld) shapes
    for name, n, d, ld in (("F_a", 700, 8, 8), ("F_b", 1300, 8, 8), ("F_c", 513, 27, 30), ("F_d", 64, 27, 30), ("F_e", 1025, 40, 41)):
        cases.append(Case(name, rng.uniform(0.05, 3.0, size=n), rng.standard_normal((n, ld)) + np.arange(ld)[None, :], d=d))
    return {c.name: c for c in cases}


def status_cases():
    """(name, a, x, status, column): what status 3 and status 5 refuse, and an empty system"""
    rng = np.random.default_rng(7)
    n, d = 300, 4
    ga, gx = rng.integers(1, 5, size=n).astype(np.float64), rng.standard_normal((n, d))
    out = []
    for name, edit, st, col in (("nan_weight", lambda a, x: a.__setitem__(17, np.nan), 3, -1),
                                ("inf_weight", lambda a, x: a.__setitem__(255, np.inf), 3, -1),
                                ("negative_weight", lambda a, x: a.__setitem__(256, -2.0), 3, -1),
                                ("weight_before_column", lambda a, x: (a.__setitem__(256, -2.0), x.__setitem__((4, 0), np.nan)), 3, -1),
                                ("inf_value", lambda a, x: x.__setitem__((77, 2), np.inf), 3, 2),
                                ("lowest_column", lambda a, x: (x.__setitem__((290, 3), np.nan), x.__setitem__((12, 1), -np.inf)), 3, 1),
                                ("all_zero", lambda a, x: a.__setitem__(slice(None), 0.0), 5, -1)):
        a, x = ga.copy(), gx.copy()
        edit(a, x)
        out.append((name, a, x, st, col))
    out.append(("empty", np.zeros(0), np.zeros((0, d)), 5, -1))
    return out
