"""The oracle, the derived bounds and the cases of ``marginals=`` (mcevidence_amd/csrc/param_marginals.hpp, docs/design/marginals.md),
shared by tests/test_param_marginals_shared.py (the serial driver and ``marginals.measure`` on the CPU) and
tests/test_gpu_param_marginals.py (the device).

THE ORACLE.  W, ess, m and v are summary's exact rational model (tests/summary_cases.py).  A density is held against the exact kernel
density estimate AT THE REPORTED h, c, lo and step of the block under test: the fp64 inputs are taken as the exact numbers they are (every
x and a is an integer times a power of two), g_k = lo + k step exactly, exp and the sums by mpmath at 60 digits, at no more than 64 grid
points per column: k = 0, G - 1, the mode, the points on either side of every 256-point block boundary and, while the budget of kernel
values lasts, points spread over the grid.  For the checks that need every grid point (all densities; the decisions) ``dense`` evaluates
the same formulas in the x87 extended format (64-bit mantissa, 15-bit exponent: no subnormal range near 2^-1074) and is itself held to
the mpmath values on the query points within a hundredth of the bound.

THE BOUNDS (u = 2^-53, gamma(k) = k u / (1 - k u)); nothing in them is fitted to an output:
  * W, ess, m, v: summary's (summary_cases.bounds)
  * h = (s sd) (4 / (3 ess))^0.2, relative: v's bound halved by the square root, plus u for it; ess's bound, plus 2 u for the product and
    the division under the power, times the exponent 0.2; the stated error of pow (POW_ULPS ulp = 2 POW_ULPS u); 2 u for the two products
  * a grid point: two roundings: |dg| <= u |k step| + u |g|
  * an argument c (g - x)^2: the subtraction rounds once and inherits dg: de = dg + u |g - x|; the square and the product round once
    each: darg = c (2 |g - x| de + de^2) (1 + 3 u) + 3 u arg.  This is where a narrow column far from 0 pays: dg is u |g|, not u |g - x|
  * a term a exp(-arg): the argument's error becomes the relative factor expm1(darg); exp's stated EXP_ULPS ulp = 2 EXP_ULPS u; one
    rounding for the product; and (a + 1) 2^-1074 absolute for the subnormal range (which also covers the 746 rule: a kernel value it
    sets to +0.0 is below 0.17 * 2^-1074)
  * a sum of n positive terms in any order: gamma(n + 2) relative
  * the normalisation (W h) sqrt(2 pi): W's bound, two products, the constant's rounding and the division: (n - 1) 2 u + 5 u relative,
    and 2^-1074 absolute where the quotient is subnormal

THE DECISIONS have no tolerance on the block's OWN densities (``marginals.decide`` and the native serial driver redo them bit for bit).
Against the oracle a grid point is UNDECIDED for p where its exact density lies within its bound plus the threshold point's bound of the
exact threshold, or where the exact running sum at the cut lies within 4 G u Z of p Z (then the cut's neighbours in the order are
undecided too); on every other point the selection must agree.  The inputs are asymmetric, so that at most MAX_UNDECIDED points per
(column, p) are undecided.
"""
import functools

import mpmath
import numpy as np

import summary_cases as sc
from mcevidence_amd import marginals as mg

U = 2.0 ** -53
EXP_ULPS = 1.0                                         # the stated error of the fp64 exp of the device library, of glibc and of NumPy
POW_ULPS = 2.0                                         # of pow
TINY = 2.0 ** -1074
TILE, BLOCK, MAX_PARTS = 512, 256, 64                  # seg_tiles.hpp, param_marginals.hpp
MAX_UNDECIDED = 2
PROBS = (0.68, 0.95)
MP_BUDGET = 40000                                      # kernel values by mpmath per column
LD = np.longdouble
SQRT_2PI = LD("2.506628274631000502415765284811045253")       # (np.pi is a double: not enough here)

mpmath.mp.dps = 60


def gamma(k):
    return k * U / (1.0 - k * U)


def nparts(n):
    return min(MAX_PARTS, -(-n // TILE))


def query_points(G, n, mode_k):
    """k = 0, G - 1, the mode, either side of every block boundary, then points spread over the grid: at most 64, and at most MP_BUDGET
    kernel values (the mandatory points always)"""
    must = [0, G - 1, int(mode_k)] + [k for b in range(BLOCK, G, BLOCK) for k in (b - 1, b)]
    cap = max(len(set(must)), min(64, MP_BUDGET // max(n, 1)))
    out = []
    for k in must + [int(v) for v in np.linspace(1, G - 2, 64 - len(set(must))) if G > 2]:
        if k not in out and len(out) < cap:
            out.append(k)
    return sorted(out)


def oracle_points(a, xcol, W_exact, h, c, lo, step, ks):
    """the exact densities at the grid points ``ks`` (mpmath)"""
    A = [mpmath.mpf(float(v)) for v in a]
    X = [mpmath.mpf(float(v)) for v in xcol]
    mc, norm = mpmath.mpf(float(c)), mpmath.mpf(W_exact) * mpmath.mpf(float(h)) * mpmath.sqrt(2 * mpmath.pi)
    out = []
    for k in ks:
        g = mpmath.mpf(float(lo)) + int(k) * mpmath.mpf(float(step))
        out.append(mpmath.fsum(ai * mpmath.exp(-mc * (g - xi) ** 2) for ai, xi in zip(A, X)) / norm)
    return out


def _mp(v):
    """an extended-format number as the exact mpmath number it is (it may lie below the fp64 range)"""
    m, e = np.frexp(LD(v))
    hi = float(m)
    return (mpmath.mpf(hi) + mpmath.mpf(float(m - LD(hi)))) * mpmath.mpf(2) ** int(e)


def dense(a, xcol, W_exact, h, c, lo, step, G, LD=LD):
    """every grid point in the extended format -> (rho[G], bound[G]); a, xcol: the used rows.  ``LD=np.float64`` evaluates the same
    formulas in fp64: good for the BOUND alone (it needs no more than a few digits; n 2^-1074 is added for what fp64 loses of the terms
    below 2^-1022), where every column of a wide system is asked"""
    a, x = np.asarray(a, dtype=LD), np.asarray(xcol, dtype=LD)
    n = a.size
    k = np.arange(G, dtype=LD)
    g = LD(lo) + k * LD(step)
    dg = U * np.abs(k * LD(step)) + U * np.abs(g)
    norm = LD(W_exact) * LD(h) * LD(SQRT_2PI)
    rel_norm = (n - 1) * 2 * U + 5 * U
    rho, bound = np.zeros(G, dtype=LD), np.zeros(G, dtype=LD)
    rows = max(1, (1 << 22) // G)
    S, B = np.zeros(G, dtype=LD), np.zeros(G, dtype=LD)
    with np.errstate(all="ignore"):
        for r0 in range(0, n, rows):
            e = g[None, :] - x[r0:r0 + rows, None]
            de = dg[None, :] + U * np.abs(e)
            arg = LD(c) * e * e
            darg = LD(c) * (2 * np.abs(e) * de + de * de) * (1 + 3 * U) + 3 * U * arg
            term = a[r0:r0 + rows, None] * np.exp(-arg)
            E, q = np.expm1(darg), 2 * EXP_ULPS * U + U + 2 * EXP_ULPS * U * U
            rel = E + (1 + E) * q                      # (1 + E) (1 + 2 EXP_ULPS u) (1 + u) - 1 without the cancellation
            S += term.sum(axis=0)
            B += (term * rel + (a[r0:r0 + rows, None] + 1) * TINY).sum(axis=0)
        if LD is np.float64:                           # (a term below 2^-1022 has lost digits here: 2^-1074 each at most)
            B = B + n * TINY
        B = B + gamma(n + 2) * (S + B)
        rho = S / norm
        bound = B / norm + (rho + B / norm) * rel_norm + LD(TINY)
        if LD is np.float64:                           # (its own quotients round to 2^-1074 down there)
            bound = bound + 2 * TINY
    return rho, bound


class Case(object):
    """one system: a (weights), x (rows, [n, ld] with d measured columns), the grid, the scale, summary's exact moments and their bounds"""

    def __init__(self, name, a, x, d=None, grid=512, scale=1.0, probs=PROBS):
        self.name = name
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.a.size, -1)
        self.d = self.x.shape[1] if d is None else int(d)
        self.grid, self.scale, self.probs = int(grid), float(scale), tuple(probs)
        self.use = self.a != 0.0
        self.n = int(self.use.sum())

    @functools.cached_property
    def exact(self):
        return sc.exact(self.a, self.x[:, :self.d], None, [0.5])

    @functools.cached_property
    def bound(self):
        return sc.bounds(self.exact)

    @property
    def system(self):
        """what ``_capi.param_marginals`` takes"""
        return (self.x, self.d, self.a)

    @property
    def spec(self):
        return (self.probs, self.grid, self.scale)


def within_ulps(a, b, ulps):
    return abs(a - b) <= ulps * 2 * U * abs(b)


def check_moments(case, got, what=""):
    """W, ess, m, v within summary's bounds and h within the bound that follows; -> the columns with status 0"""
    ex, b, n = case.exact, case.bound, case.n
    assert got["status"] == 0 and got["column"] == -1 and got["rows"] == n and got["grid"] == case.grid, (case.name, got["status"], got["column"], got["rows"])
    good = np.flatnonzero(np.asarray(got["col_status"]) == 0)
    ess = got["W"] * got["W"] / got["A2"]
    r = {"W": abs(got["W"] - ex["W"]) / max(b["W"], 5e-324), "ess": abs(ess - ex["ess"]) / b["ess"], "mean": 0.0, "var": 0.0, "h": 0.0}
    for j in good:
        r["mean"] = max(r["mean"], abs(got["mean"][j] - ex["mean"][j]) / max(b["mean"][j], 5e-324))
        r["var"] = max(r["var"], abs(got["var"][j] - ex["var"][j]) / max(b["var"][j], 5e-324))
        h_exact = case.scale * mpmath.sqrt(mpmath.mpf(ex["var"][j])) * (mpmath.mpf(4) / (3 * mpmath.mpf(ex["ess"]))) ** mpmath.mpf("0.2")
        # (ex holds the exact values rounded to fp64: one more u each)
        rel = 0.5 * (b["var"][j] / ex["var"][j] + U) + U + 0.2 * (b["ess"] / ex["ess"] + U + 2 * U) + 2 * POW_ULPS * U + 2 * U + 2 * U
        r["h"] = max(r["h"], float(abs(mpmath.mpf(float(got["h"][j])) - h_exact) / (h_exact * rel)))
        # the reported values hang together as the rule says (c and the grid from the REPORTED h)
        # (products, sums and differences are correctly rounded everywhere; sqrt and the divisions within their stated 1 ulp)
        h = got["h"][j]
        lo = ex["min"][j] - 3.0 * h
        assert got["lo"][j] == lo and within_ulps(got["sd"][j], np.sqrt(got["var"][j]), 1) and within_ulps(got["c"][j], 1.0 / ((2.0 * h) * h), 1), (case.name, j)
        assert within_ulps(got["step"][j], ((ex["max"][j] + 3.0 * h) - lo) / float(case.grid - 1), 1), (case.name, j)
    print("%s %-18s n=%-5d d=%-3d G=%-4d error/bound: W %.3g  ess %.3g  mean %.3g  var %.3g  h %.3g" % (
        what, case.name, n, case.d, case.grid, r["W"], r["ess"], r["mean"], r["var"], r["h"]))
    assert all(v <= 1.0 for v in r.values()), (case.name, r)
    return good


def check_column(case, got, j, what="", oracle=True, stats=None):
    """column j of a block: every density against ``dense`` within the bound (the query points against mpmath), the decisions redone
    bit for bit on the block's own densities, and the selection against the oracle on every decided point; -> (rho, bound) of ``dense``"""
    a, x = case.a[case.use], case.x[case.use, j]
    G = case.grid
    h, c, lo, step = (float(got[k][j]) for k in ("h", "c", "lo", "step"))
    rho, bound = _dense_cached(case, j, h, c, lo, step)
    dev = np.asarray(got["density"][j], dtype=np.float64)
    err = np.abs(dev.astype(LD) - rho)
    worst = float(np.max(err / bound))
    worst_mp = worst_ld = 0.0
    if oracle:
        ks = query_points(G, a.size, int(np.argmax(dev)))
        for k, ex in zip(ks, _oracle_cached(case, j, h, c, lo, step, tuple(ks))):
            bk = _mp(bound[k])
            worst_ld = max(worst_ld, float(abs(_mp(rho[k]) - ex) / (bk / 100)))
            worst_mp = max(worst_mp, float(abs(mpmath.mpf(float(dev[k])) - ex) / bk))
    # the decisions on the block's own densities: no tolerance
    mode, mode_density, lower, upper, pieces, edge = mg.decide(dev, lo, step, case.probs)
    assert got["mode"][j] == mode and got["mode_density"][j] == mode_density and mode_density == dev.max(), (case.name, j, "mode")
    for t in range(len(case.probs)):
        assert (got["lower"][t][j], got["upper"][t][j], got["pieces"][t][j], got["edge"][t][j]) == (lower[t], upper[t], pieces[t], edge[t]), (case.name, j, t)
    # against the oracle: every decided point
    _, masks = mg.hpd_selection(dev, case.probs)
    undecided = decisions(rho, bound, case.probs, masks, (case.name, j))
    # (and the oracle alone: the selection of its own densities rounded to fp64 stays within the same cap)
    assert decisions(rho, bound, case.probs, mg.hpd_selection(rho.astype(np.float64), case.probs)[1], (case.name, j, "oracle")) == undecided
    if stats is not None:
        stats["density"] = max(stats.get("density", 0.0), worst, worst_mp)
        stats["undecided"] = max(stats.get("undecided", 0), max(undecided))
        stats["zeros"] = stats.get("zeros", 0) + int(np.count_nonzero(dev == 0.0))
    print("%s %-18s col %-3d error/bound: all %.3g  mpmath %.3g  (extended format / mpmath: %.3g of a hundredth)  undecided %s" % (
        what, case.name, j, worst, worst_mp, worst_ld, undecided))
    assert worst <= 1.0 and worst_mp <= 1.0 and worst_ld <= 1.0, (case.name, j, worst, worst_mp, worst_ld)
    assert max(undecided) <= MAX_UNDECIDED, (case.name, j, undecided)
    return rho, bound


def check_against_numpy(case, got, what=""):
    """ALL densities of a block against the NumPy form's at the block's reported h, c, lo and step: within two bounds (each form within
    one of the exact value); -> the largest ratio"""
    host = mg.measure(case.a, case.x[:, :case.d], case.probs, case.grid, case.scale, at=got)
    assert np.array_equal(host["col_status"], got["col_status"]), (case.name, host["col_status"], got["col_status"])
    worst = 0.0
    for j in np.flatnonzero(np.asarray(got["col_status"]) == 0):
        _, b = dense(case.a[case.use], case.x[case.use, j], case.exact["W"], got["h"][j], got["c"][j], got["lo"][j], got["step"][j], case.grid, LD=np.float64)
        ratio = float(np.max(np.abs(np.asarray(got["density"][j]) - host["density"][j]) / (2 * b)))
        assert ratio <= 1.0, (case.name, j, ratio)
        worst = max(worst, ratio)
    print("%s %-18s every density against the NumPy form's at the reported parameters: %.3g of the two bounds" % (what, case.name, worst))
    return worst


_CACHE = {}


def _dense_cached(case, j, h, c, lo, step):
    """(two forms that report the same h, c, lo and step are held to one evaluation of the oracle)"""
    key = ("dense", case.name, j, h, c, lo, step)
    if key not in _CACHE:
        _CACHE[key] = dense(case.a[case.use], case.x[case.use, j], case.exact["W"], h, c, lo, step, case.grid)
    return _CACHE[key]


def _oracle_cached(case, j, h, c, lo, step, ks):
    key = ("mp", case.name, j, h, c, lo, step, ks)
    if key not in _CACHE:
        W = sc.Fraction(case.exact["W"])
        _CACHE[key] = oracle_points(case.a[case.use], case.x[case.use, j], mpmath.mpf(W.numerator) / W.denominator, h, c, lo, step, ks)
    return _CACHE[key]


def decisions(rho, bound, probs, masks, who=""):
    """the selection ``masks`` against the exact densities: asserts agreement on every decided point; -> the undecided points per p"""
    G = rho.size
    order = np.lexsort((np.arange(G), -rho))
    cum = np.cumsum(rho[order])
    Z = cum[-1]
    out = []
    for p, sel in zip(probs, masks):
        target = LD(p) * Z
        cut = min(int(np.searchsorted(cum, target, side="left")), G - 1)
        kc = order[cut]
        und = np.abs(rho - rho[kc]) <= bound + bound[kc]
        near = 4 * G * U * Z
        if abs(cum[cut] - target) <= near or (cut > 0 and abs(cum[cut - 1] - target) <= near):
            und[order[max(cut - 1, 0):cut + 2]] = True
        want = np.zeros(G, dtype=bool)
        want[order[:cut + 1]] = True
        wrong = np.flatnonzero(~und & (want != np.asarray(sel)))
        assert wrong.size == 0, (who, p, wrong[:8], "decided points selected differently")
        out.append(int(und.sum()))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 1025, 4100)
BIG = 33300                                            # 66 tiles: 64 parts of 1 or 2 tiles


def weights(rng, n, kind):
    """unit; integer 1..4; fractional with a fifth of the rows at weight 0 (-> the rows to overwrite with NaN / inf)"""
    if kind == "unit":
        return np.ones(n), np.zeros(0, dtype=int)
    if kind == "integer":
        return (rng.integers(1, 5, n).astype(np.float64) if n > 3 else np.array([3.0, 1.0, 2.0])[:n]), np.zeros(0, dtype=int)
    a = rng.integers(1, 64, n) / 16.0
    if n <= 3:                                         # (two rows of one weight are mirror images: every point would tie with its mirror)
        a = np.array([3.0, 1.0, 2.0])[:n] / 16.0
    zero = np.arange(1, n, 5) if n > 2 else np.zeros(0, dtype=int)
    a[zero] = 0.0
    return a, zero


def skewed(rng, n, scale=1.0, shift=0.0):
    """a skewed, asymmetric column of integers / 64"""
    return np.round((rng.gamma(3.0, 1.0, n) * scale + shift) * 64.0) / 64.0


SPECIAL = ("narrow", "huge", "constant", "three", "outlier")


def special_column(rng, n, kind):
    if kind == "narrow":                               # 50 +- 1e-6: fails unless g - x is bounded honestly
        return 50.0 + rng.choice([-1.0, 0.0, 0.0, 1.0, 1.0, 1.0], n) * 2.0 ** -20
    if kind == "huge":                                 # the variance overflows: col_status 7
        return rng.choice([-1e300, 1e300], n)
    if kind == "constant":
        return np.full(n, 2.5)
    if kind == "three":
        return rng.choice([-1.0, 0.25, 3.0], n, p=[0.5, 0.3, 0.2])
    v = skewed(rng, n, 1.0 / 64.0)                     # a lone far outlier: most of the grid is exact zeros by the 746 rule
    v[5 * (n // 15) + 3] = 2.0 ** 20                   # (a row that keeps its weight in every kind of weights)
    return v


def make(name, n, d, grid, kind, seed, special=False, scale=1.0):
    rng = np.random.default_rng(seed)
    a, zero = weights(rng, n, kind)
    x = np.stack([skewed(rng, n, 1.0 + 0.5 * (j % 3), float(j % 5) - 2.0) for j in range(d + 2)], axis=1)
    if special:
        for j, k in enumerate(SPECIAL):
            x[:, 1 + j] = special_column(rng, n, k)
    if zero.size:
        x[zero] = np.tile([np.nan, np.inf, -np.inf], -(-x.shape[1] // 3))[:x.shape[1]]
    return Case(name, a, x, d=d, grid=grid, scale=scale)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}: every size of the tile scheme, every d, every grid, every kind of weights; ld = d + 2"""
    out = {}
    plan = [(2, 1, 64, "integer"), (3, 8, 512, "fractional"), (63, 1, 1024, "unit"), (64, 8, 64, "integer"), (65, 1, 512, "fractional"),
            (511, 8, 1024, "unit"), (512, 1, 512, "integer"), (513, 127, 512, "fractional"), (1025, 27, 1024, "integer"), (4100, 8, 512, "fractional"),
            (4100, 27, 64, "unit"), (BIG, 1, 64, "integer")]
    for i, (n, d, G, kind) in enumerate(plan):
        special = d == 8 and n >= 511
        name = "n%d_d%d_G%d_%s" % (n, d, G, kind)
        out[name] = make(name, n, d, G, kind, 100 + i, special=special)
    out["scale_quarter"] = make("scale_quarter", 1025, 1, 512, "unit", 77, scale=0.25)
    return out


def oracle_columns(case):
    """the columns the oracle is asked about: the first, the last, the narrow one and the outlier's (``check_against_numpy`` and the
    bit-for-bit decisions cover every column)"""
    return sorted(set([0, case.d - 1] + ([1, 5] if case.d == 8 and case.n >= 400 else [])))


def status_cases():
    """[(name, a, x[n, 2], status, column)]: summary's refusals without a likelihood, and fewer than 2 used rows"""
    rng = np.random.default_rng(5)
    x = np.round(rng.standard_normal((40, 2)) * 64) / 64
    a = rng.integers(1, 5, 40).astype(np.float64)
    out = []
    for name, fn, status, column in (
            ("negative_weight", lambda a, x: a.__setitem__(7, -1.0), 3, -1), ("nan_weight", lambda a, x: a.__setitem__(7, np.nan), 3, -1),
            ("inf_weight", lambda a, x: a.__setitem__(39, np.inf), 3, -1), ("inf_value", lambda a, x: x.__setitem__((3, 1), np.inf), 3, 1),
            ("nan_values", lambda a, x: (x.__setitem__((3, 1), np.nan), x.__setitem__((30, 0), np.nan)), 3, 0),
            ("weight_before_value", lambda a, x: (a.__setitem__(2, -2.0), x.__setitem__((3, 0), np.nan)), 3, -1),
            ("no_weight", lambda a, x: a.__setitem__(slice(None), 0.0), 5, -1),
            ("one_row", lambda a, x: (a.__setitem__(slice(None), 0.0), a.__setitem__(11, 2.0)), 6, -1)):
        ai, xi = a.copy(), x.copy()
        fn(ai, xi)
        out.append((name, ai, xi, status, column))
    out.append(("empty", np.zeros(0), np.zeros((0, 2)), 5, -1))
    out.append(("single", np.ones(1), np.array([[1.0, 2.0]]), 6, -1))
    return out


def assert_failed_system(got, d, status, column, rows, who=""):
    assert (got["status"], got["column"], got["rows"]) == (status, column, rows), (who, got["status"], got["column"], got["rows"])
    for k in ("W", "A2", "mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density", "col_status", "lower", "upper", "pieces", "edge", "density"):
        assert np.isnan(got[k]).all() and np.shape(got[k])[-1:] in ((), (d,), (got["grid"],)), (who, k)


def assert_failed_column(got, j, who=""):
    assert got["col_status"][j] == 7 and np.all(np.asarray(got["pieces"])[:, j] == -1.0), (who, j)
    for k in ("mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density"):
        assert np.isnan(got[k][j]), (who, j, k)
    for k in ("lower", "upper", "edge"):
        assert np.isnan(np.asarray(got[k])[:, j]).all(), (who, j, k)
    assert np.isnan(got["density"][j]).all(), (who, j)


def equal_blocks(a, b):
    """bit for bit, NaN equal to NaN"""
    return all(np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), equal_nan=True) for k in a)


# ---- the native program (tests/native/param_marginals_check.cpp), a stand-alone sanitized build ----------------------------------
def build_checker(directory):
    import os
    import subprocess
    from helpers import REPO
    exe = os.path.join(str(directory), "param_marginals_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "param_marginals_check.cpp"), "-o", exe])
    return exe


def _run(exe, mode, fin, fout, count):
    import subprocess
    out = subprocess.run([exe, mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % count), out.stdout[-2000:] + out.stderr[-2000:]
    return np.frombuffer(open(fout, "rb").read(), dtype="<f8")


def run_native(exe, tmp_path, systems, probs, grid, scale):
    """[(a, x[n, ld], d)] through the serial driver -> one block dict per system"""
    import struct
    fin, fout = tmp_path / "mar_in.bin", tmp_path / "mar_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<qd", grid, scale))
        for a, x, d in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            x = x if x.ndim == 2 else x.reshape(len(a), -1)
            fh.write(struct.pack("<qqq", len(a), d, x.shape[1]) + x.tobytes() + np.ascontiguousarray(a, dtype="<f8").tobytes())
    raw = _run(exe, "marginals", fin, fout, len(systems))
    blocks, at = [], 0
    for a, x, d in systems:
        size = mg.HEAD + d * (mg.PER_COL + mg.PER_P * probs.size + grid)
        blocks.append(mg.from_block(raw[at:at + size], d, probs.size, grid))
        at += size
    assert at == raw.size
    return blocks


def check_decisions_native(exe, tmp_path, blocks, probs, grid):
    """the serial rule (steps 5 and 6) applied to each block's OWN density arrays equals the block's decisions bit for bit"""
    import struct
    fin, fout = tmp_path / "dec_in.bin", tmp_path / "dec_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    cols = [(b, j) for b in blocks if b["status"] == 0 for j in range(len(b["mean"])) if b["col_status"][j] == 0]
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<q", grid))
        for b, j in cols:
            fh.write(struct.pack("<dd", b["lo"][j], b["step"][j]) + np.ascontiguousarray(b["density"][j], dtype="<f8").tobytes())
    raw = _run(exe, "decide", fin, fout, len(cols)).reshape(len(cols), 2 + mg.PER_P * probs.size)
    for (b, j), rec in zip(cols, raw):
        got = [b["mode"][j], b["mode_density"][j]] + [b[k][t][j] for t in range(probs.size) for k in ("lower", "upper", "pieces", "edge")]
        assert np.array_equal(np.array(got), rec), (j, got, rec)
    return len(cols)
