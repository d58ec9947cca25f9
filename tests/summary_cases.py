"""The oracle and the cases of ``summary=`` (docs/design/summary.md): the rule of mcevidence_amd/csrc/param_summary.hpp in exact
rational arithmetic, the bound every fp64 route is held to, and the smallest inputs at which each pass can go wrong.  Shared by
tests/test_param_summary_shared.py (CPU) and tests/test_gpu_param_summary.py (GPU); every case is built once per process, when it is
first asked for.

The bounds (nothing in them is fitted to output), with eps = 2^-52, n the used rows, M1 = sum|a x| / W, M2 = sum a (x - m)^2 / W
(information.md's derivation with rho = 1: the weights of a status-0 system are not negative):

    |dm|   <= 2 n eps M1
    |dv|   <= 2 (n + 1) eps M2 + (2 n eps M1)^2
    |dess| <= 3 n eps ess
    |dW|   <= (n - 1) eps W

min, max and the best fit are exact.  A quantile is asked for EXACTLY where the exact cumulative weight at the selected value and at the
largest value below it both lie at least 4 n eps W from the exact q W (a sum in any order errs by (n - 1) eps W, the target by n eps W
at most); the other (case, column, target) triples are counted as dropped and the callers assert how many there may be.
"""
import functools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
TARGETS = np.array([0.5, (1.0 - 0.68) / 2.0, (1.0 + 0.68) / 2.0, (1.0 - 0.95) / 2.0, (1.0 + 0.95) / 2.0])


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


def exact(a, x, f, q):
    """the rule in exact arithmetic on the rows with a != 0 (a status-0 system) -> dict: W, A2, ess, rows, mean[d], var[d], M1[d],
    min[d], max[d], bestfit_row, bestfit_f, bestfit[d], quant[nq][d] and keep[nq][d] (is the triple asked for exactly?)"""
    a = np.asarray(a, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(a.size, -1)
    q = np.asarray(q, dtype=np.float64)
    use = a != 0.0
    rows_at = np.flatnonzero(use)
    a, x = a[use], x[use]
    n, d = x.shape
    A, Ka = _ints(a)
    Wi = sum(A)
    W = Fraction(Wi, 1 << Ka)
    A2 = Fraction(sum(v * v for v in A), 1 << (2 * Ka))
    out = dict(W=float(W), A2=float(A2), ess=float(W * W / A2), rows=n, mean=np.zeros(d), var=np.zeros(d), M1=np.zeros(d), min=x.min(axis=0) + 0.0,
               max=x.max(axis=0) + 0.0, quant=np.zeros((q.size, d)), keep=np.zeros((q.size, d), dtype=bool), bestfit_row=-1, bestfit_f=float("nan"),
               bestfit=np.full(d, np.nan))
    if f is not None:
        fu = np.asarray(f, dtype=np.float64)[use]
        best = int(np.argmax(fu))
        out["bestfit_row"], out["bestfit_f"], out["bestfit"] = int(rows_at[best]), float(fu[best]), x[best].copy()
    margin = Fraction(4 * n) * Fraction(EPS) * W
    want = [Fraction(float(t)) * W for t in q]
    for j in range(d):
        X, Kx = _ints(x[:, j])
        s1 = sum(u * v for u, v in zip(A, X))
        s2 = sum(u * v * v for u, v in zip(A, X))
        m = Fraction(s1, Wi << Kx)
        v = Fraction(s2, Wi << (2 * Kx)) - m * m
        out["mean"][j], out["var"][j] = _float(m), _float(v)
        out["M1"][j] = _float(Fraction(sum(u * abs(w) for u, w in zip(A, X)), Wi << Kx))
        order = np.argsort(x[:, j], kind="stable")
        xs = x[order, j]
        cum = np.cumsum(np.array([A[i] for i in order], dtype=object))
        for t, target in enumerate(want):
            ti = target * (1 << Ka)                      # the target at the integers' scale
            lo, hi = 0, n - 1                            # first position whose cumulative weight reaches the target
            while lo < hi:
                mid = (lo + hi) // 2
                if cum[mid] >= ti:
                    hi = mid
                else:
                    lo = mid + 1
            val = xs[lo]
            first, last = np.searchsorted(xs, val, side="left"), np.searchsorted(xs, val, side="right") - 1
            c_sel = Fraction(int(cum[last]), 1 << Ka)
            c_below = Fraction(int(cum[first - 1]), 1 << Ka) if first > 0 else Fraction(0)
            out["quant"][t, j] = val + 0.0
            out["keep"][t, j] = c_sel - target >= margin and target - c_below >= margin
    return out


def bounds(ex):
    n = ex["rows"]
    bm = 2.0 * n * EPS * ex["M1"]
    with np.errstate(all="ignore"):
        return dict(mean=bm, var=2.0 * (n + 1) * EPS * ex["var"] + bm * bm, ess=3.0 * n * EPS * ex["ess"], W=(n - 1) * EPS * ex["W"])


class Case(object):
    """one system: a (weights), x (rows, [n, ld] with d measured columns), f (fs or None), the exact values and the bounds"""

    def __init__(self, name, a, x, f, d=None, q=TARGETS):
        self.name = name
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.a.size, -1)
        self.f = None if f is None else np.ascontiguousarray(f, dtype=np.float64)
        self.d = self.x.shape[1] if d is None else int(d)
        self.q = np.asarray(q, dtype=np.float64)
        self.exact = exact(self.a, self.x[:, :self.d], self.f, self.q)
        self.bound = bounds(self.exact)

    @property
    def system(self):
        """what ``_capi.param_summary`` takes"""
        return (self.x, self.d, self.a, self.f)


def check(case, got, what="", counts=None):
    """``got``: a block dict (``summary.measure`` / ``summary.from_block``).  Prints the largest error / bound, asserts every value
    within its bound, min / max / best fit exact and every kept quantile exact; adds (kept, dropped) to ``counts``"""
    ex, b = case.exact, case.bound
    assert got["status"] == 0 and got["column"] == -1 and got["rows"] == ex["rows"], (case.name, got["status"], got["column"], got["rows"])
    ess = got["W"] * got["W"] / got["A2"]
    r = {"W": abs(got["W"] - ex["W"]) / max(b["W"], 5e-324), "ess": abs(ess - ex["ess"]) / b["ess"]}
    fin = np.isfinite(ex["var"])
    with np.errstate(all="ignore"):
        r["mean"] = float(np.max(np.abs(got["mean"] - ex["mean"]) / np.maximum(b["mean"], 5e-324)))
        r["var"] = float(np.max(np.where(fin, np.abs(got["var"] - ex["var"]) / np.maximum(b["var"], 5e-324), 0.0)))
    assert np.all(np.isposinf(np.asarray(got["var"])[~fin])), (case.name, "a variance beyond the fp64 range is +inf")
    keep = ex["keep"]
    print("%s %-16s n=%-5d d=%-3d error/bound: W %.3g  ess %.3g  mean %.3g  var %.3g   quantiles kept %d of %d" % (
        what, case.name, ex["rows"], case.d, r["W"], r["ess"], r["mean"], r["var"], keep.sum(), keep.size))
    assert all(v <= 1.0 for v in r.values()), (case.name, r)
    assert np.array_equal(got["min"], ex["min"]) and np.array_equal(got["max"], ex["max"]), case.name
    assert np.array_equal(np.asarray(got["quant"])[keep], ex["quant"][keep]), (case.name, np.argwhere(keep & (np.asarray(got["quant"]) != ex["quant"])))
    if case.f is not None:
        assert got["bestfit_row"] == ex["bestfit_row"] and got["bestfit_f"] == ex["bestfit_f"] and np.array_equal(got["bestfit"], ex["bestfit"]), case.name
    else:
        assert got["bestfit_row"] == -1 and np.isnan(got["bestfit_f"]) and np.isnan(got["bestfit"]).all(), case.name
    if counts is not None:
        counts[0] += int(keep.sum())
        counts[1] += int(keep.size - keep.sum())
    return r


def block_of(d, bestfit_f):
    """``info["summary"]`` -> the block dict ``check`` takes (the dict holds logLmax + f, so f itself is the caller's)"""
    with np.errstate(all="ignore"):
        A2 = d["sum_w"] ** 2 / d["ess"]
    return dict(W=d["sum_w"], A2=A2, rows=d["rows"], status=d["status"], column=d["column"], mean=d["mean"], var=d["var"], min=d["min"], max=d["max"],
                bestfit=d["bestfit"], bestfit_row=d["bestfit_row"], bestfit_f=bestfit_f,
                quant=np.concatenate([np.asarray(d["median"])[None, :]] + [np.asarray(r)[None, :] for lo, hi in zip(d["lower"], d["upper"]) for r in (lo, hi)]))


def _odd(a):
    """integer weights with an odd total: q W then falls between two cumulative weights for q = 0.5"""
    if int(a.sum()) % 2 == 0:
        a[-1] += 1.0
    return a


def _fs(rng, x):
    f = -0.5 * np.sum(x * x, axis=1) + 1e-3 * rng.standard_normal(x.shape[0])
    return f - f.max()


CPU_SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 1025, 4100)
CPU_KINDS = ("unit", "integer", "fractional", "duplicated")


@functools.lru_cache(maxsize=None)
def cpu_cases():
    """n in CPU_SIZES x {unit, integer 1..4, fractional weights on a continuous column; integer weights on a heavily duplicated column}"""
    rng = np.random.default_rng(5150)
    out = []
    for n in CPU_SIZES:
        for kind in CPU_KINDS:
            x = rng.standard_normal((n, 1))
            if kind == "unit":
                a = np.ones(n)
            elif kind == "fractional":
                a = rng.uniform(0.05, 3.0, size=n)
            else:
                a = _odd(rng.integers(1, 5, size=n).astype(np.float64))
            if kind == "duplicated":
                x = rng.choice(np.array([-1.5, -0.25, 0.0, 0.125, 0.5, 2.0, 3.75]), size=(n, 1))
            out.append(Case("%s_%d" % (kind, n), a, x, _fs(rng, x)))
    kept, triples = sum(int(c.exact["keep"].sum()) for c in out), sum(c.exact["keep"].size for c in out)
    assert 10 * (triples - kept) <= triples, "the acceptance rule drops %d of %d triples: more than 1 in 10" % (triples - kept, triples)
    return out


def _adversary_columns(rng, n):
    """E: the columns that try the keys' order"""
    cols = [rng.standard_normal(n) - 0.5,                                                         # negative and positive values
            rng.choice(np.array([-0.0, 0.0, -5e-324, 5e-324, 2.5e-310, -2.5e-310, 1.0, -1.0]), size=n),   # -0.0 beside +0.0, denormals
            rng.choice(np.array([-1e300, 1e300, -1.0, 1.0, 0.5]), size=n),                        # +-1e300
            1.0 + EPS * rng.integers(0, 4, size=n),                                               # neighbours one ulp apart
            np.sort(rng.standard_normal(n))[::-1],                                                # sorted descending
            rng.choice(np.array([-2.0, 0.25, 7.0]), size=n),                                      # 3 distinct values
            np.full(n, 2.5)]                                                                      # constant
    return np.stack(cols, axis=1)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """A .. E, K and the systems G mixes: name -> Case"""
    rng = np.random.default_rng(90210)
    cases = []
    x = rng.standard_normal((600, 8))
    cases.append(Case("A_unit", np.ones(600), x, _fs(rng, x)))
    for n in (511, 512, 513, 1025):                      # the tile edges, at every width
        for d in (1, 8, 27, 127):
            x = rng.standard_normal((n, d + 2)) * (1.0 + np.arange(d + 2))[None, :]
            cases.append(Case("B_%d_%d" % (n, d), _odd(rng.integers(1, 5, size=n).astype(np.float64)), x, _fs(rng, x[:, :2]), d=d))
    x = 50.0 + 1e-6 * rng.choice([-1.0, 1.0], size=(1000, 3))
    cases.append(Case("C_narrow", _odd(rng.integers(1, 5, size=1000).astype(np.float64)), x, _fs(rng, x - 50.0)))
    n = 700
    a = rng.uniform(0.05, 3.0, size=n)
    x = rng.standard_normal((n, 5))
    f = _fs(rng, x)
    zero = np.arange(n) % 5 == 2                         # a fifth of the rows: weight 0 over NaN / +-inf values and NaN f
    a[zero] = 0.0
    x[zero] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=(int(zero.sum()), 5))
    f[zero] = np.nan
    cases.append(Case("D_zeros", a, x, f))
    for n in (1, 2, 1000):
        x = _adversary_columns(rng, n)
        cases.append(Case("E_keys_%d" % n, _odd(rng.integers(1, 5, size=n).astype(np.float64)), x, _fs(rng, x[:, :1])))
    x = rng.standard_normal((4100, 8))
    cases.append(Case("L_4100", _odd(rng.integers(1, 5, size=4100).astype(np.float64)), x, _fs(rng, x)))
    # the designed exact tie: unit weights, n = 1000, q = 0.5: 0.5 * 1000 is exact, the answer is the 500th smallest value
    x = rng.permutation(np.arange(1000.0))[:, None] * 0.37
    cases.append(Case("T_tie", np.ones(1000), x, None, q=np.array([0.5])))
    # K: ties of the best fit (the lowest row wins), a maximum in the last row of the last tile, all f = -inf
    x = rng.standard_normal((1025, 2))
    f = _fs(rng, x) - 1.0
    f[[700, 33, 512]] = 0.0
    cases.append(Case("K_ties", np.ones(1025), x, f))
    f = _fs(rng, x) - 1.0
    f[1024] = 0.0
    cases.append(Case("K_last", np.ones(1025), x, f))
    a = np.ones(1025)
    a[:3] = 0.0                                          # (the lowest USED row is row 3)
    cases.append(Case("K_minus_inf", a, x, np.full(1025, -np.inf)))
    return {c.name: c for c in cases}


def status_cases():
    """(name, a, x, f, status, column): what status 3 and status 5 refuse, and an empty system"""
    rng = np.random.default_rng(7)
    n, d = 300, 4
    ga, gx = rng.integers(1, 5, size=n).astype(np.float64), rng.standard_normal((n, d))
    gf = _fs(rng, gx)
    out = []
    for name, edit, st, col in (("nan_weight", lambda a, x, f: a.__setitem__(17, np.nan), 3, -1),
                                ("inf_weight", lambda a, x, f: a.__setitem__(255, np.inf), 3, -1),
                                ("negative_weight", lambda a, x, f: a.__setitem__(256, -2.0), 3, -1),
                                ("weight_before_like", lambda a, x, f: (a.__setitem__(256, -2.0), f.__setitem__(3, np.nan), x.__setitem__((4, 0), np.nan)), 3, -1),
                                ("nan_f", lambda a, x, f: f.__setitem__(299, np.nan), 3, -2),
                                ("like_before_column", lambda a, x, f: (f.__setitem__(299, np.nan), x.__setitem__((5, 1), np.inf)), 3, -2),
                                ("inf_value", lambda a, x, f: x.__setitem__((77, 2), np.inf), 3, 2),
                                ("lowest_column", lambda a, x, f: (x.__setitem__((290, 3), np.nan), x.__setitem__((12, 1), -np.inf)), 3, 1),
                                ("all_zero", lambda a, x, f: a.__setitem__(slice(None), 0.0), 5, -1)):
        a, x, f = ga.copy(), gx.copy(), gf.copy()
        edit(a, x, f)
        out.append((name, a, x, f, st, col))
    out.append(("empty", np.zeros(0), np.zeros((0, d)), np.zeros(0), 5, -1))
    return out
