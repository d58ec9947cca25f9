"""The oracle, the derived bounds and the cases of ``marginals=`` with ``bounds=`` (mcevidence_amd/csrc/param_marginals_bounds.hpp,
docs/design/marginals_bounds.md), shared by tests/test_param_marginals_bounds_shared.py (the serial driver and
``marginals.measure_bounded`` on the CPU) and tests/test_gpu_param_marginals_bounds.py (the device).  What tests/marginals_cases.py
says about the oracle holds here: a density is held against the exact boundary-kernel estimate AT THE REPORTED h, c, lo and step of the
block under test, with the bounds L and U and every x and a the exact numbers they are; exp, erf and the sums by mpmath at 60 digits at
no more than 64 grid points per column (k = 0, G - 1, the mode, either side of every 256-point block boundary, then points spread over
the grid); ``dense`` evaluates the two sums at every grid point in the x87 extended format (the boundary constants of all G points by
mpmath: they cost G evaluations a column) and is itself held to mpmath on the query points within a hundredth of the bound.

THE BOUNDS extend marginals_cases' (u = 2^-53, gamma(k) = k u / (1 - k u)); nothing in them is fitted to an output:
  * a term t = a exp(-arg): marginals_cases' (relative ``rel``, (a + 1) 2^-1074 absolute); S: those summed, gamma(n + 2) relative
  * a term of R, m = t (x - g): the negated difference e inherits de = dg + u |e| from the subtraction; the extra product rounds once:
    dm = dt (|e| + de) + t de + u (t + dt) (|e| + de) + 2^-1074.  R's terms change sign, so its sum carries gamma(n + 2) on the sum
    of |m|: an ABSOLUTE bound
  * T0 = S / norm as marginals_cases' rho; T1 = (R / h) / norm: one more division (u) and 2^-1074 for each quotient
  * p = (g - L) / h: dp = (dg + u |g - L|) / h + u |p| (an open side: p is +inf exactly, nothing to bound); z = p / sqrt 2: the
    constant's rounding and the division, 2 u; erf(z): ERF_ULPS ulp and the slope 2 / sqrt(pi) exp(-z'^2) at the z' of the interval
    nearest 0; phi: the argument t^2 / 2 as the relative factor expm1(|t| dt + dt^2 / 2 + u t^2 / 2), exp's EXP_ULPS ulp, the division
    and the constant (2 u), 2^-1074; psi = t phi: the product rule and u
  * a0, a1, a2 and den = a0 a2 - a1^2: every difference keeps the ABSOLUTE errors of its operands and rounds once; so does
    a2 T0 - a1 T1.  A narrow range (U - L of a few h) makes den small and earns a large bound honestly
  * f0 = T0 / a0, f1 = num / den, r = f1 / f0: quotient rule with the divisor at its lower end, u each; min(r, 4) - 1 does not widen
    dr; exp: the relative factor expm1(dr + u |r - 1|), EXP_ULPS ulp, the last product (u).  Where f0 cannot be told from 0 within its
    bound (the subnormal tail) the density is only known to lie in [0, (f0 + df0) e^3]: that is the bound there
THE ASSUMPTIONS: exp within EXP_ULPS = 1 ulp as in marginals_cases.  erf: glibc's manual states 1 ulp on x86_64; for the device
library no statement is found here, and the OpenCL full-profile requirement, 16 ulp, is ASSUMED for every route (ERF_ULPS = 16).

THE DECISIONS have no tolerance on the block's OWN densities (``marginals.decide_bounded`` and the native serial driver redo them bit for
bit, end weights included).  Against the oracle a grid point is UNDECIDED as marginals_cases defines it, the running sums with the 1/2
weights; at most MAX_UNDECIDED per (column, p).
"""
import functools
import math

import mpmath
import numpy as np

import marginals_cases as mc
from mcevidence_amd import marginals as mg

U_ = mc.U
TINY = mc.TINY
EXP_ULPS = mc.EXP_ULPS
ERF_ULPS = 16.0
LD = mc.LD
MAX_UNDECIDED = mc.MAX_UNDECIDED
PROBS = mc.PROBS
E3 = math.exp(3.0) * 1.0000001
INF = float("inf")

mpmath.mp.dps = 60


def _ld(v):
    """an mpmath number in the extended format (two pieces)"""
    hi = float(v)
    if math.isinf(hi):
        return LD(hi)
    return LD(hi) + LD(float(v - mpmath.mpf(hi)))


def _phi_mp(t):
    return mpmath.mpf(0) if t == mpmath.inf else mpmath.exp(-t * t / 2) / mpmath.sqrt(2 * mpmath.pi)


def consts_mp(g, L, U, h):
    """step 5' exactly; g, h: mpmath numbers, L, U: floats (an open side: its terms are 1 and 0)"""
    p = mpmath.inf if L == -INF else (g - mpmath.mpf(L)) / h
    q = mpmath.inf if U == INF else (mpmath.mpf(U) - g) / h
    ep = mpmath.mpf(1) if p == mpmath.inf else mpmath.erf(p / mpmath.sqrt(2))
    eq = mpmath.mpf(1) if q == mpmath.inf else mpmath.erf(q / mpmath.sqrt(2))
    php, phq = _phi_mp(p), _phi_mp(q)
    a0 = (eq + ep) / 2
    a1 = php - phq
    a2 = a0 - (0 if q == mpmath.inf else q * phq) - (0 if p == mpmath.inf else p * php)
    return a0, a1, a2, a0 * a2 - a1 * a1


def density_exact(T0, T1, a0, a1, a2, den, exp=mpmath.exp):
    f0 = T0 / a0
    f1 = (a2 * T0 - a1 * T1) / den
    r = f1 / f0
    return f0 * exp(min(r, 4) - 1)


def oracle_points(a, xcol, W_exact, h, c, lo, step, L, U, ks):
    """the exact densities at the grid points ``ks`` (mpmath)"""
    A = [mpmath.mpf(float(v)) for v in a]
    X = [mpmath.mpf(float(v)) for v in xcol]
    mh, mcc = mpmath.mpf(float(h)), mpmath.mpf(float(c))
    norm = mpmath.mpf(W_exact) * mh * mpmath.sqrt(2 * mpmath.pi)
    out = []
    for k in ks:
        g = mpmath.mpf(float(lo)) + int(k) * mpmath.mpf(float(step))
        t = [ai * mpmath.exp(-mcc * (g - xi) ** 2) for ai, xi in zip(A, X)]
        S, R = mpmath.fsum(t), mpmath.fsum(ti * (xi - g) for ti, xi in zip(t, X))
        out.append(density_exact(S / norm, R / mh / norm, *consts_mp(g, L, U, mh)))
    return out


def consts_bounds(g, dg, L, U, h, a0, a1, a2):
    """the absolute bounds of the COMPUTED a0, a1, a2 and den at the grid points g (fp64 arithmetic is enough for a bound)"""
    g, dg = np.asarray(g, dtype=np.float64), np.asarray(dg, dtype=np.float64)
    a0, a1, a2 = (np.asarray(v, dtype=np.float64) for v in (a0, a1, a2))

    def side(dist, open_):
        if open_:                                      # p = +inf exactly: erf 1, phi 0, psi 0, nothing rounded
            z = np.zeros_like(g)
            return z, z, z, z, z, z
        t = np.abs(dist) / h
        dt = (dg + U_ * np.abs(dist)) / h + U_ * t
        z = t / math.sqrt(2.0)
        dz = dt / math.sqrt(2.0) + 2 * U_ * z
        zin = np.maximum(z - dz, 0.0)
        erf = np.array([math.erf(v) for v in z])
        derf = ERF_ULPS * 2 * U_ * erf + 2.0 / math.sqrt(math.pi) * np.exp(-zin * zin) * dz + U_
        phi = np.exp(-t * t / 2.0) / math.sqrt(2 * math.pi)
        tin = np.maximum(t - dt, 0.0)
        phi_hi = np.exp(-tin * tin / 2.0) / math.sqrt(2 * math.pi)
        dphi = phi_hi * (np.expm1(t * dt + dt * dt / 2.0 + U_ * t * t / 2.0) + (2 * EXP_ULPS + 2) * U_ * 1.01) + TINY
        psi = t * phi
        dpsi = (t + dt) * dphi + phi_hi * dt + U_ * (psi + (t + dt) * dphi) + TINY
        return erf, derf, phi, dphi, psi, dpsi
    ep, dep, php, dphp, psp, dpsp = side(g - L, L == -INF)
    eq, deq, phq, dphq, psq, dpsq = side(U - g, U == INF)
    da0 = 0.5 * (dep + deq) + U_ * np.abs(a0)
    da1 = dphp + dphq + U_ * np.abs(a1)
    da2 = da0 + dpsq + dpsp + U_ * (np.abs(a0) + psq + np.abs(a2) + da0 + dpsq + dpsp)
    dden = (np.abs(a0) * da2 + np.abs(a2) * da0 + da0 * da2 + 2 * np.abs(a1) * da1 + da1 * da1
            + U_ * (np.abs(a0 * a2) + a1 * a1) * 1.01 + U_ * np.abs(a0 * a2 - a1 * a1) * 1.01)
    return da0, da1, da2, dden


def dense(a, xcol, W_exact, h, c, lo, step, L, U, G, LD=LD):
    """every grid point -> (rho[G], bound[G]); the sums in the extended format (``LD=np.float64``: in fp64, good for the BOUND alone), the
    boundary constants by mpmath (fp64: ``marginals.boundary_constants``); a, xcol: the used rows"""
    a, x = np.asarray(a, dtype=LD), np.asarray(xcol, dtype=LD)
    n = a.size
    k = np.arange(G, dtype=LD)
    g = LD(lo) + k * LD(step)
    dg = U_ * np.abs(k * LD(step)) + U_ * np.abs(g)
    norm = LD(W_exact) * LD(h) * LD(mc.SQRT_2PI)
    rel_norm = (n - 1) * 2 * U_ + 5 * U_
    rows = max(1, (1 << 22) // G)
    S, BS, R, BR, RA = (np.zeros(G, dtype=LD) for _ in range(5))
    with np.errstate(all="ignore"):
        for r0 in range(0, n, rows):
            ar = a[r0:r0 + rows, None]
            e = g[None, :] - x[r0:r0 + rows, None]
            ae = np.abs(e)
            de = dg[None, :] + U_ * ae
            arg = LD(c) * e * e
            darg = LD(c) * (2 * ae * de + de * de) * (1 + 3 * U_) + 3 * U_ * arg
            term = ar * np.exp(-arg)
            E, q = np.expm1(darg), 2 * EXP_ULPS * U_ + U_ + 2 * EXP_ULPS * U_ * U_
            dt = term * (E + (1 + E) * q) + (ar + 1) * TINY
            S += term.sum(axis=0)
            BS += dt.sum(axis=0)
            m = term * -e
            R += m.sum(axis=0)
            RA += np.abs(m).sum(axis=0)
            BR += (dt * (ae + de) + term * de + U_ * (term + dt) * (ae + de) + TINY).sum(axis=0)
        if LD is np.float64:                           # (a term below 2^-1022 has lost digits here: 2^-1074 each at most)
            BS = BS + n * TINY
            BR = BR + n * TINY * (1 + np.abs(g) + np.max(np.abs(x)))
        BS = BS + mc.gamma(n + 2) * (S + BS)
        BR = BR + mc.gamma(n + 2) * (RA + BR)
        T0, T1 = S / norm, R / LD(h) / norm
        dT0 = BS / norm + (T0 + BS / norm) * rel_norm + LD(TINY)
        dT1 = BR / LD(h) / norm + (np.abs(T1) + BR / LD(h) / norm) * (rel_norm + 2 * U_) + LD(TINY) * (1 + 1 / norm)
        gf = g.astype(np.float64)
        if LD is np.float64:
            a0, a1, a2, den = mg.boundary_constants(gf, L, U, float(h))
            dT0, dT1 = dT0 + 2 * TINY, dT1 + 2 * TINY
        else:
            cm = [consts_mp(mpmath.mpf(float(lo)) + int(kk) * mpmath.mpf(float(step)), L, U, mpmath.mpf(float(h))) for kk in range(G)]
            a0, a1, a2, den = (np.array([_ld(v[i]) for v in cm], dtype=LD) for i in range(4))
        da0, da1, da2, dden = consts_bounds(gf, dg.astype(np.float64), L, U, float(h), a0, a1, a2)
        f0 = T0 / a0
        df0 = (dT0 + f0 * da0) / np.maximum(a0 - da0, TINY) + U_ * f0 + TINY
        num = a2 * T0 - a1 * T1
        dnum = (np.abs(a2) * dT0 + T0 * da2 + da2 * dT0 + np.abs(a1) * dT1 + np.abs(T1) * da1 + da1 * dT1
                + U_ * (np.abs(a2 * T0) + np.abs(a1 * T1)) * 1.01 + U_ * np.abs(num) * 1.01 + 2 * TINY)
        f1 = num / den
        den_lo, f0_lo = den - dden, f0 - df0
        df1 = (dnum + np.abs(f1) * dden) / np.where(den_lo > 0, den_lo, 1.0) + U_ * np.abs(f1) + TINY
        r = f1 / f0
        dr = (df1 + np.abs(r) * df0) / np.where(f0_lo > 0, f0_lo, 1.0) + U_ * np.abs(r)
        ex = np.minimum(r, LD(4)) - 1
        dex = dr + U_ * (np.abs(ex) + dr)
        rho = np.where(f0 > 0, f0 * np.exp(ex), 0.0)
        q = (2 * EXP_ULPS + 1) * U_ * 1.01
        Ex = np.expm1(dex)
        bound = rho * (Ex + (1 + Ex) * q) + df0 * np.exp(ex + dex) * (1 + q) + TINY
        unknown = ~(f0_lo > 0) | ~(den_lo > 0) | ~np.isfinite(bound)
        bound = np.where(unknown, np.where(den_lo > 0, (f0 + df0) * E3 + TINY, np.inf), bound)
    return rho, bound


class Case(mc.Case):
    """marginals_cases.Case with the bounds of its measured columns: lo[d], hi[d]"""

    def __init__(self, name, a, x, lo, hi, d=None, grid=512, scale=1.0, probs=PROBS):
        mc.Case.__init__(self, name, a, x, d=d, grid=grid, scale=scale, probs=probs)
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)

    @property
    def bounds(self):
        return (self.lo, self.hi)


def end_weights(got, j, G):
    return mg.end_weights(G, got["at_lo"][j] == 1.0, got["at_hi"][j] == 1.0)


def decisions(rho, bound, w, probs, masks, who=""):
    """marginals_cases.decisions with the end weights w"""
    G = rho.size
    order = np.lexsort((np.arange(G), -rho))
    cum = np.cumsum((rho * w)[order])
    Z = cum[-1]
    out = []
    for p, sel in zip(probs, masks):
        target = LD(p) * Z
        cut = min(int(np.searchsorted(cum, target, side="left")), G - 1)
        kc = order[cut]
        und = np.abs(rho - rho[kc]) <= bound + bound[kc]
        near = 4 * G * U_ * Z
        if abs(cum[cut] - target) <= near or (cut > 0 and abs(cum[cut - 1] - target) <= near):
            und[order[max(cut - 1, 0):cut + 2]] = True
        want = np.zeros(G, dtype=bool)
        want[order[:cut + 1]] = True
        wrong = np.flatnonzero(~und & (want != np.asarray(sel)))
        assert wrong.size == 0, (who, p, wrong[:8], "decided points selected differently")
        out.append(int(und.sum()))
    return out


_CACHE = {}


def _dense_cached(case, j, h, c, lo, step):
    key = ("dense", case.name, j, h, c, lo, step)
    if key not in _CACHE:
        _CACHE[key] = dense(case.a[case.use], case.x[case.use, j], case.exact["W"], h, c, lo, step, case.lo[j], case.hi[j], case.grid)
    return _CACHE[key]


def _oracle_cached(case, j, h, c, lo, step, ks):
    key = ("mp", case.name, j, h, c, lo, step, ks)
    if key not in _CACHE:
        W = mc.sc.Fraction(case.exact["W"])
        _CACHE[key] = oracle_points(case.a[case.use], case.x[case.use, j], mpmath.mpf(W.numerator) / W.denominator, h, c, lo, step, case.lo[j], case.hi[j], ks)
    return _CACHE[key]


def check_grid(case, got, j):
    """step 3' on the reported h: the grid ends on a bound it would cross, and nowhere else"""
    ex, h, G = case.exact, got["h"][j], case.grid
    L, U = case.lo[j], case.hi[j]
    lo0, hi0 = ex["min"][j] - 3.0 * h, ex["max"][j] + 3.0 * h
    at_lo, at_hi = L >= lo0, U <= hi0
    lo, hi = (L if at_lo else lo0), (U if at_hi else hi0)
    assert (got["at_lo"][j], got["at_hi"][j]) == (float(at_lo), float(at_hi)) and got["lo"][j] == lo, (case.name, j, got["at_lo"][j], got["at_hi"][j], got["lo"][j], lo)
    assert mc.within_ulps(got["step"][j], (hi - lo) / float(G - 1), 1) and (got["bound_lo"][j], got["bound_hi"][j]) == (L, U), (case.name, j)


def check_column(case, got, j, what="", oracle=True, stats=None):
    """column j of a bounded block: marginals_cases.check_column with the boundary kernel and the end weights; -> (rho, bound)"""
    a, G = case.a[case.use], case.grid
    h, c, lo, step = (float(got[k][j]) for k in ("h", "c", "lo", "step"))
    check_grid(case, got, j)
    rho, bound = _dense_cached(case, j, h, c, lo, step)
    dev = np.asarray(got["density"][j], dtype=np.float64)
    worst = float(np.max(np.abs(dev.astype(LD) - rho) / bound))
    worst_mp = worst_ld = 0.0
    if oracle:
        ks = mc.query_points(G, 2 * a.size, int(np.argmax(dev)))
        for k, ex in zip(ks, _oracle_cached(case, j, h, c, lo, step, tuple(ks))):
            if not np.isfinite(bound[k]):
                continue
            bk = mc._mp(bound[k])
            worst_ld = max(worst_ld, float(abs(mc._mp(rho[k]) - ex) / (bk / 100)))
            worst_mp = max(worst_mp, float(abs(mpmath.mpf(float(dev[k])) - ex) / bk))
    at_lo, at_hi = got["at_lo"][j] == 1.0, got["at_hi"][j] == 1.0
    mode, mode_density, lower, upper, pieces, edge = mg.decide_bounded(dev, lo, step, case.probs, at_lo, at_hi)
    assert got["mode"][j] == mode and got["mode_density"][j] == mode_density and mode_density == dev.max(), (case.name, j, "mode")
    for t in range(len(case.probs)):
        assert (got["lower"][t][j], got["upper"][t][j], got["pieces"][t][j], got["edge"][t][j]) == (lower[t], upper[t], pieces[t], edge[t]), (case.name, j, t)
    w = end_weights(got, j, G)
    _, masks = mg.hpd_selection_bounded(dev, case.probs, at_lo, at_hi)
    undecided = decisions(rho, bound, w, case.probs, masks, (case.name, j))
    assert decisions(rho, bound, w, case.probs, mg.hpd_selection_bounded(rho.astype(np.float64), case.probs, at_lo, at_hi)[1], (case.name, j, "oracle")) == undecided
    if stats is not None:
        stats["density"] = max(stats.get("density", 0.0), worst, worst_mp)
        stats["undecided"] = max(stats.get("undecided", 0), max(undecided))
    print("%s %-22s col %-3d (L %g, U %g, at %d%d) error/bound: all %.3g  mpmath %.3g  (extended format / mpmath: %.3g of a hundredth)  undecided %s" % (
        what, case.name, j, case.lo[j], case.hi[j], at_lo, at_hi, worst, worst_mp, worst_ld, undecided))
    assert worst <= 1.0 and worst_mp <= 1.0 and worst_ld <= 1.0, (case.name, j, worst, worst_mp, worst_ld)
    assert max(undecided) <= MAX_UNDECIDED, (case.name, j, undecided)
    return rho, bound


def check_against_numpy(case, got, what=""):
    """ALL densities of a bounded block against ``measure_bounded``'s at the block's reported h, c, lo and step: within two bounds"""
    host = mg.measure_bounded(case.a, case.x[:, :case.d], case.bounds, case.probs, case.grid, case.scale, at=got)
    assert np.array_equal(host["col_status"], got["col_status"]), (case.name, host["col_status"], got["col_status"])
    worst = 0.0
    for j in np.flatnonzero(np.asarray(got["col_status"]) == 0):
        _, b = dense(case.a[case.use], case.x[case.use, j], case.exact["W"], got["h"][j], got["c"][j], got["lo"][j], got["step"][j], case.lo[j], case.hi[j],
                     case.grid, LD=np.float64)
        ratio = float(np.max(np.abs(np.asarray(got["density"][j]) - host["density"][j]) / (2 * b)))
        assert ratio <= 1.0, (case.name, j, ratio)
        worst = max(worst, ratio)
    print("%s %-22s every density against the NumPy form's at the reported parameters: %.3g of the two bounds" % (what, case.name, worst))
    return worst


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
KINDS = ("open", "lower_at_min", "lower_below_min", "both", "upper", "gamma_at_0")


def _bounds_of(kind, col, a, grid):
    """the bounds of one column by its kind; every bound an integer / 1024"""
    used = col[a != 0.0]
    mn, mx = float(used.min()), float(used.max())
    if kind == "open":
        return -INF, INF
    if kind == "lower_at_min":
        return mn, INF
    if kind == "lower_below_min":                      # 1.5 h below the smallest sample: the grid is not cut, the constants are not 1
        h = float(mg.measure(a, col[:, None], (0.5,), grid)["h"][0])
        return math.floor((mn - 1.5 * h) * 1024.0) / 1024.0, INF
    if kind == "both":
        return mn, mx
    if kind == "upper":
        return -INF, mx
    return 0.0, INF


def make(name, n, d, grid, wkind, seed, kinds=None):
    rng = np.random.default_rng(seed)
    a, zero = mc.weights(rng, n, wkind)
    kinds = [KINDS[j % 6] for j in range(d)] if kinds is None else list(kinds)
    x = np.stack([mc.skewed(rng, n, 1.0 + 0.5 * (j % 3), float(j % 5) - 2.0) for j in range(d + 2)], axis=1)
    for j, kind in enumerate(kinds):
        if kind == "gamma_at_0":                       # an exponential-like column: the density is highest at the bound
            x[:, j] = np.round(rng.gamma(1.0, 1.0, n) * 64.0) / 64.0
    if zero.size:
        x[zero] = np.tile([np.nan, np.inf, -np.inf], -(-x.shape[1] // 3))[:x.shape[1]]
    lo, hi = np.full(d, -INF), np.full(d, INF)
    for j, kind in enumerate(kinds):
        lo[j], hi[j] = _bounds_of(kind, x[:, j], a, grid)
    return Case(name, a, x, lo, hi, d=d, grid=grid)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}: n in {2, 3, 511, 512, 513, 1025, 33300}, d in {1, 8, 127}, G in {64, 512, 1024}, every kind of weights; ld = d + 2; the
    columns of a case run through KINDS, a case of one column has the kind named"""
    out = {}
    plan = [(2, 1, 64, "integer", ("both",)), (3, 8, 512, "fractional", None), (511, 8, 1024, "unit", None), (512, 1, 512, "integer", ("lower_at_min",)),
            (513, 127, 512, "fractional", None), (1025, 8, 1024, "integer", None), (1025, 1, 512, "unit", ("lower_below_min",)),
            (mc.BIG, 1, 64, "integer", ("gamma_at_0",))]
    for i, (n, d, G, wkind, kinds) in enumerate(plan):
        name = "n%d_d%d_G%d_%s" % (n, d, G, wkind)
        out[name] = make(name, n, d, G, wkind, 300 + i, kinds)
    return out


def open_case(c):
    """the same rows without bounds"""
    return Case(c.name + "_open", c.a, c.x, np.full(c.d, -INF), np.full(c.d, INF), d=c.d, grid=c.grid, scale=c.scale, probs=c.probs)


def oracle_columns(case):
    """the columns the oracle is asked about: one of every kind, and the last"""
    return sorted(set(list(range(min(case.d, 6))) + [case.d - 1]))


COMMON = ("W", "A2", "rows", "status", "column", "grid", "mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density", "col_status", "lower", "upper",
          "pieces", "edge", "density")


def equal_common(bounded, plain, cols=None):
    """the values of the common layout, bit for bit, NaN equal to NaN (``cols``: these columns alone)"""
    for k in COMMON:
        u, v = np.asarray(bounded[k], dtype=np.float64), np.asarray(plain[k], dtype=np.float64)
        if cols is not None and u.ndim >= 1:
            u, v = (u[..., cols, :], v[..., cols, :]) if k == "density" else (u[..., cols], v[..., cols])
        if not np.array_equal(u, v, equal_nan=True):
            return False
    return True


def assert_outside_column(got, j, who=""):
    assert got["col_status"][j] == 8 and np.all(np.asarray(got["pieces"])[:, j] == -1.0), (who, j, got["col_status"][j])
    for k in ("mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density", "at_lo", "at_hi"):
        assert np.isnan(got[k][j]), (who, j, k)
    for k in ("lower", "upper", "edge"):
        assert np.isnan(np.asarray(got[k])[:, j]).all(), (who, j, k)
    assert np.isnan(got["density"][j]).all(), (who, j)


# ---- the native program (tests/native/param_marginals_bounds_check.cpp), a stand-alone sanitized build -----------------------------
def build_checker(directory):
    import os
    import subprocess
    from helpers import REPO
    exe = os.path.join(str(directory), "param_marginals_bounds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "param_marginals_bounds_check.cpp"), "-o", exe])
    return exe


def run_native(exe, tmp_path, systems, probs, grid, scale):
    """[(a, x[n, ld], d, (lo[d], hi[d]))] through the serial driver -> one block dict per system"""
    import struct
    fin, fout = tmp_path / "marb_in.bin", tmp_path / "marb_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<qd", grid, scale))
        for a, x, d, (lo, hi) in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            x = x if x.ndim == 2 else x.reshape(len(a), -1)
            fh.write(struct.pack("<qqq", len(a), d, x.shape[1]) + x.tobytes() + np.ascontiguousarray(a, dtype="<f8").tobytes()
                     + np.ascontiguousarray(lo, dtype="<f8").tobytes() + np.ascontiguousarray(hi, dtype="<f8").tobytes())
    raw = mc._run(exe, "marginals", fin, fout, len(systems))
    blocks, at = [], 0
    for a, x, d, _ in systems:
        size = mg.HEAD + d * (mg.PER_COL_BOUNDED + mg.PER_P * probs.size + grid)
        blocks.append(mg.from_block_bounded(raw[at:at + size], d, probs.size, grid))
        at += size
    assert at == raw.size
    return blocks


def check_decisions_native(exe, tmp_path, blocks, probs, grid):
    """the serial rule (steps 7' and 8') applied to each block's OWN density arrays equals the block's decisions bit for bit"""
    import struct
    fin, fout = tmp_path / "decb_in.bin", tmp_path / "decb_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    cols = [(b, j) for b in blocks if b["status"] == 0 for j in range(len(b["mean"])) if b["col_status"][j] == 0]
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<q", grid))
        for b, j in cols:
            fh.write(struct.pack("<dddd", b["lo"][j], b["step"][j], b["at_lo"][j], b["at_hi"][j]) + np.ascontiguousarray(b["density"][j], dtype="<f8").tobytes())
    raw = mc._run(exe, "decide", fin, fout, len(cols)).reshape(len(cols), 2 + mg.PER_P * probs.size)
    for (b, j), rec in zip(cols, raw):
        got = [b["mode"][j], b["mode_density"][j]] + [b[k][t][j] for t in range(probs.size) for k in ("lower", "upper", "pieces", "edge")]
        assert np.array_equal(np.array(got), rec), (j, got, rec)
    return len(cols)
