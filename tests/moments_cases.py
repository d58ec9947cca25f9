"""The oracle and the cases of ``information=`` (docs/design/information.md): the rule of mcevidence_amd/csrc/like_moments.hpp in
exact rational arithmetic, the bound every fp64 route is held to, and the smallest inputs at which each pass can go wrong.  Shared by
tests/test_like_moments_shared.py (CPU) and tests/test_gpu_information.py (GPU); built once per process.

The bound (nothing in it is fitted to output), with eps = 2^-52, n the used rows, rho = sum|a| / |W|, M1 = sum|a f| / |W|,
M2 = sum|a| (f - c)^2 / |W|:

    |dc|   <= 2 n rho eps M1
    |dv|   <= 2 (n + 1) rho eps M2 + (2 n rho eps M1)^2
    |dess| <= 3 n rho eps ess
    |dW|   <= n rho eps |W|                                  (a sum of n terms errs by <= (n - 1) eps of the sum of magnitudes)

A case is accepted only if its bound on v is below 1e-6 v and its bound on c below 1e-9 max(1, |c|): asserted here.
"""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52


def exact(a, f):
    """the rule in rationals on the rows with a != 0 -> dict of floats: W, c, v, A2, ess, rows, and the bound's rho, M1, M2"""
    a = np.asarray(a, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    use = a != 0.0
    A = [Fraction(float(x)) for x in a[use]]
    F = [Fraction(float(x)) for x in f[use]]
    n = len(A)
    W = sum(A, Fraction(0))
    S = sum((x * y for x, y in zip(A, F)), Fraction(0))
    A2 = sum((x * x for x in A), Fraction(0))
    c = S / W
    v = sum((x * (y - c) ** 2 for x, y in zip(A, F)), Fraction(0)) / W
    absW = abs(W)
    rho = sum((abs(x) for x in A), Fraction(0)) / absW
    M1 = sum((abs(x * y) for x, y in zip(A, F)), Fraction(0)) / absW
    M2 = sum((abs(x) * (y - c) ** 2 for x, y in zip(A, F)), Fraction(0)) / absW
    return dict(W=float(W), c=float(c), v=float(v), A2=float(A2), ess=float(W * W / A2), rows=n, rho=float(rho), M1=float(M1), M2=float(M2))


def bounds(ex):
    n, rho = ex["rows"], ex["rho"]
    bc = 2.0 * n * rho * EPS * ex["M1"]
    return dict(c=bc, v=2.0 * (n + 1) * rho * EPS * ex["M2"] + bc * bc, ess=3.0 * n * rho * EPS * ex["ess"], W=n * rho * EPS * abs(ex["W"]))


class Case(object):
    """one system: a (weights), f (fs), the exact values and the bounds"""

    def __init__(self, name, a, f):
        self.name = name
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.f = np.ascontiguousarray(f, dtype=np.float64)
        self.exact = exact(self.a, self.f)
        self.bound = bounds(self.exact)
        assert self.bound["v"] < 1e-6 * self.exact["v"], (name, self.bound["v"], self.exact["v"])
        assert self.bound["c"] < 1e-9 * max(1.0, abs(self.exact["c"])), (name, self.bound["c"], self.exact["c"])


def ratios(case, got):
    """error / bound of W, c, v and ess of ``got`` (a dict with W, c, v, A2: ``information.moments``' or the device block's)"""
    ex, b = case.exact, case.bound
    ess = got["W"] * got["W"] / got["A2"]
    return {k: abs(x - ex[k]) / b[k] for k, x in (("W", got["W"]), ("c", got["c"]), ("v", got["v"]), ("ess", ess))}


def check(case, got, what=""):
    """prints error / bound of every value, then asserts all of them <= 1 and the status and the used rows"""
    r = ratios(case, got)
    print("%s %-12s n=%-5d error/bound: W %.3g  c %.3g  v %.3g  ess %.3g" % (what, case.name, case.exact["rows"], r["W"], r["c"], r["v"], r["ess"]))
    assert got["status"] == 0 and got["rows"] == case.exact["rows"], (case.name, got)
    assert all(x <= 1.0 for x in r.values()), (case.name, r)
    return max(r.values())


def _chi2_fs(rng, n, dof):
    """fs of a Gaussian posterior in dof dimensions: -chi^2_dof / 2, shifted so that its maximum is 0"""
    f = -0.5 * rng.chisquare(dof, size=n)
    return f - f.max()


def _build():
    rng = np.random.default_rng(20191)
    cases = []
    cases.append(Case("A_unit", np.ones(600), _chi2_fs(rng, 600, 4)))
    for n in (511, 512, 513, 1025):                      # the tile edges
        cases.append(Case("B_%d" % n, rng.integers(1, 5, size=n).astype(np.float64), _chi2_fs(rng, n, 6)))
    cases.append(Case("C_narrow", rng.integers(1, 5, size=1000).astype(np.float64), -50.0 + 1e-6 * rng.choice([-1.0, 1.0], size=1000)))
    a = rng.uniform(0.05, 3.0, size=700)
    f = _chi2_fs(rng, 700, 5)
    zero = np.arange(700) % 5 == 2
    a[zero] = 0.0
    f[zero] = np.where(np.arange(zero.sum()) % 2 == 0, -np.inf, np.nan)       # never read into a sum
    cases.append(Case("D_zeros", a, f))
    a = rng.integers(1, 5, size=600).astype(np.float64)
    a[300] = -2.0
    cases.append(Case("E_negative", a, _chi2_fs(rng, 600, 4)))
    cases.append(Case("L_4100", rng.integers(1, 5, size=4100).astype(np.float64), _chi2_fs(rng, 4100, 27)))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def status_cases():
    """(name, a, f, status): what status 3 and status 5 refuse, and an empty system"""
    rng = np.random.default_rng(7)
    n = 300
    good_a, good_f = rng.integers(1, 5, size=n).astype(np.float64), _chi2_fs(rng, n, 3)
    out = []
    for name, i, av, fv, st in (("nan_weight", 17, np.nan, None, 3), ("inf_weight", 255, np.inf, None, 3), ("minus_inf_f", 256, None, -np.inf, 3),
                                ("nan_f", 299, None, np.nan, 3)):
        a, f = good_a.copy(), good_f.copy()
        if av is not None:
            a[i] = av
        if fv is not None:
            f[i] = fv
        out.append((name, a, f, st))
    out.append(("all_zero", np.zeros(n), good_f.copy(), 5))
    out.append(("negative_sum", -good_a, good_f.copy(), 5))
    out.append(("empty", np.zeros(0), np.zeros(0), 5))
    return out
