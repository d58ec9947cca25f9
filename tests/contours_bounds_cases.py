"""The oracle, the derived bounds and the cases of ``contours=`` with the key ``"bounds"`` (mcevidence_amd/csrc/param_contours.hpp's steps
3" .. 8", docs/design/contours_bounds.md), shared by tests/test_param_contours_bounds_shared.py (the serial driver and
``contours.measure_bounded`` on the CPU) and tests/test_gpu_param_contours_bounds.py (the device).  The manner is
tests/contours_cases.py's and tests/marginals_bounds_cases.py's, whose helpers are used where they fit.

THE ORACLE.  A density is held against the exact three-term boundary-kernel estimate AT THE REPORTED h, c, lo and step of the block under
test, the bounds L and U and every x and a the exact numbers they are: exp, erf and the three sums by mpmath at 60 digits on at most 64
cells of at most three pairs per case (contours_cases.query_cells: the four corners -- the cell of weight 1/4 and the cell where both
boundary kernels act -- the mode, either side of every 16-cell block boundary in both axes, then cells off the diagonal).  ``dense``
evaluates the three sums at every cell in the x87 extended format (the boundary constants of the 2 G grid points by mpmath) and is itself
held to mpmath on the query cells within a hundredth of the bound.

THE BOUND composes contours_cases' terms for S with marginals_bounds_cases' terms (u = 2^-53, gamma(k) = k u / (1 - k u)); nothing in it is
fitted to an output:
  * E = K(arg): contours_cases' relative rel_E per axis; a E_x: one more rounding, r1 = (1 + rel_x)(1 + u) - 1
  * S: contours_cases' bound_of, as it stands (its terms, gamma(n + 2) relative on a sum of non-negative terms)
  * the arm x - g = -e inherits de = dg + u |e| from the subtraction.  A' = (a E_x)(x - g): dA' = a E_x r1 (|e| + de) + a E_x de
    + u a E_x (1 + r1)(|e| + de) + 2^-1074; a term of R_x is A' E_y: d = dA' E_y (1 + rel_y) + |A'| E_y rel_y + u (|A'| + dA') E_y (1 + rel_y)
    + 2^-1074.  B' = E_y (y - g) and R_y's term (a E_x) B' likewise with the axes' parts exchanged.  R's terms change sign, so its sum
    carries gamma(n + 2) on the sum of |terms| (and of their bounds): an ABSOLUTE bound
  * T00 = S / norm: contours_cases' normalisation, (n - 1) 2 u + 6 u relative and 2^-1074;  T10 = (R_x / h) / norm: one more division,
    2 u more, and 2^-1074 for each quotient
  * the constants a0, a1, a2, den of an axis: marginals_bounds_cases.consts_bounds as it stands, with ERF_ULPS = 16 as assumed there
  * every product p = q r of two bounded values: dp = |q| dr + |r| dq + dq dr + u (|p| + that) + 2^-1074; every difference keeps the
    ABSOLUTE bounds of its operands and rounds once.  So u0 v0, det = ((u0 v0) dx) dy, the products of four constants
    k00 = (u0 u2)(v0 v2) - (u1 u1)(v1 v1), k10 = (u0 u1) dy, k01 = (v0 v1) dx, and w = (T00 k00 - T10 k10) - T01 k01
  * f0 = T00 / (u0 v0), f1 = w / det, r = f1 / f0: the quotient rule with the divisor at its lower end, u each; min(r, 4) - 1 does not widen
    dr; exp: the relative factor expm1(dr + u |r - 1|), EXP_ULPS ulp, the last product (u)
  * where f0 cannot be told from 0 within its bound (the subnormal tail) the density is only known to lie in [0, (f0 + df0) e^3]: that is
    the bound there; where det cannot be told from 0 the bound is infinite (the rule switches to f0 there) and the cell is not held
A pair whose two columns are open goes through the same text: its constants are 1, 0, 1, 1 exactly and their bounds 0.

THE DECISIONS have no tolerance on the block's OWN densities (``contours.decide_bounded`` and the native serial driver redo them bit for
bit, the cell weights included).  Against the oracle a cell is UNDECIDED as contours_cases defines it, the running sums with the weights;
at most MAX_UNDECIDED per (pair, p), the threshold cell one of them.
"""
import functools
import math

import mpmath
import numpy as np

import contours_cases as cc
import marginals_bounds_cases as mbc
import marginals_cases as mc
import summary_cases as sc
from mcevidence_amd import contours as ct
from mcevidence_amd import marginals as mg

U_, TINY, LD, EXP_ULPS, gamma = cc.U, cc.TINY, cc.LD, cc.EXP_ULPS, cc.gamma
MAX_UNDECIDED = cc.MAX_UNDECIDED
PROBS = cc.PROBS
INF = float("inf")
E3 = mbc.E3
KINDS = mbc.KINDS
COMMON = ("W", "A2", "rows", "status", "column", "grid", "nc") + ct.COL_KEYS + ct.PAIR_KEYS + ct.P_KEYS + ("density",)

mpmath.mp.dps = 60


def is_open(L, U):
    return L == -INF and U == INF


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def density_exact(T00, T10, T01, u, v):
    """step 6" exactly (mpmath numbers)"""
    f0 = T00 / (u[0] * v[0])
    if not f0 > 0:
        return mpmath.mpf(0)
    det = u[0] * v[0] * u[3] * v[3]
    f1 = (T00 * (u[0] * u[2] * v[0] * v[2] - u[1] ** 2 * v[1] ** 2) - T10 * (u[0] * u[1] * v[3]) - T01 * (v[0] * v[1] * u[3])) / det
    return f0 * mpmath.exp(min(f1 / f0, 4) - 1)


def oracle_cells(a, xs, xt, W_exact, prm_s, prm_t, bnd_s, bnd_t, cells):
    """the exact densities at ``cells`` = [(kx, ky)] (mpmath); prm = (h, c, lo, step), bnd = (L, U)"""
    A = [mpmath.mpf(float(v)) for v in a]

    def axis(x, prm, bnd, ks):
        h, c, lo, step = (mpmath.mpf(float(v)) for v in prm)
        X = [mpmath.mpf(float(v)) for v in x]
        out = {}
        for k in ks:
            g = lo + int(k) * step
            E = [mpmath.exp(-c * (g - xi) ** 2) for xi in X]
            out[k] = (E, [e * (xi - g) for e, xi in zip(E, X)], mbc.consts_mp(g, bnd[0], bnd[1], h))
        return out
    Ax = axis(xs, prm_s, bnd_s, sorted(set(k for k, _ in cells)))
    Ay = axis(xt, prm_t, bnd_t, sorted(set(k for _, k in cells)))
    hs, ht = mpmath.mpf(float(prm_s[0])), mpmath.mpf(float(prm_t[0]))
    norm = mpmath.mpf(W_exact) * hs * ht * 2 * mpmath.pi
    out = []
    for kx, ky in cells:
        Ex, Mx, u = Ax[kx]
        Ey, My, v = Ay[ky]
        S = mpmath.fsum(ai * ex * ey for ai, ex, ey in zip(A, Ex, Ey))
        Rx = mpmath.fsum(ai * mx * ey for ai, mx, ey in zip(A, Mx, Ey))
        Ry = mpmath.fsum(ai * ex * my for ai, ex, my in zip(A, Ex, My))
        out.append(density_exact(S / norm, Rx / hs / norm, Ry / ht / norm, u, v))
    return out


def _axis(x, prm, G, T):
    """contours_cases._axis, and the arm: E[r][k], its relative bound, |e|, de, g, dg in the type T"""
    h, c, lo, step = (T(v) for v in prm)
    E, rel = cc._axis(x, prm, G, T)
    k = np.arange(G, dtype=T)
    g = lo + k * step
    dg = U_ * np.abs(k * step) + U_ * np.abs(g)
    e = g[None, :] - np.asarray(x, dtype=T)[:, None]
    return E, rel, e, dg[None, :] + U_ * np.abs(e), g, dg


def _prod(q, dq, r, dr):
    """p = q r of two bounded values -> (p, its absolute bound)"""
    p = q * r
    d = np.abs(q) * dr + np.abs(r) * dq + dq * dr
    return p, d + U_ * (np.abs(p) + d) * 1.01 + TINY


def _consts(g, dg, bnd, h, lo, step, G, T):
    """a0, a1, a2, den of an axis [G] and their absolute bounds (marginals_bounds_cases.consts_bounds); by mpmath in the extended format"""
    gf = g.astype(np.float64)
    if T is np.float64:
        a = mg.boundary_constants(gf, bnd[0], bnd[1], float(h))
        a = tuple(np.asarray(v, dtype=np.float64) for v in a)
    else:
        cm = [mbc.consts_mp(mpmath.mpf(float(lo)) + int(k) * mpmath.mpf(float(step)), bnd[0], bnd[1], mpmath.mpf(float(h))) for k in range(G)]
        a = tuple(np.array([mbc._ld(v[i]) for v in cm], dtype=T) for i in range(4))
    da = mbc.consts_bounds(gf, np.asarray(dg, dtype=np.float64), bnd[0], bnd[1], float(h), a[0], a[1], a[2])
    return a, da


def dense(a, xs, xt, W_exact, prm_s, prm_t, bnd_s, bnd_t, G, T=LD):
    """every cell -> (rho[G, G], bound[G, G]): the sums in the extended format (``T=np.float64``: in fp64, good for the BOUND alone), the
    boundary constants by mpmath (fp64: ``marginals.boundary_constants``); a, xs, xt: the used rows"""
    a = np.asarray(a, dtype=T)
    n = a.size
    with np.errstate(all="ignore"):
        Ex, rx, ex, dex, gx, dgx = _axis(xs, prm_s, G, T)
        Ey, ry, ey, dey, gy, dgy = _axis(xt, prm_t, G, T)
        hs, ht = T(prm_s[0]), T(prm_t[0])
        aE = a[:, None] * Ex
        r1 = (1 + rx) * (1 + U_) - 1
        Eyh = Ey * (1 + ry)

        def dot(A, B):                                 # (a sum that only enters a BOUND: fp64 is enough, with a margin for its own rounding)
            return np.dot(np.asarray(A, dtype=np.float64).T, np.asarray(B, dtype=np.float64)) * (1 + 1e-9)
        # S: contours_cases.bound_of's terms
        S = np.dot(aE.T, Ey)
        BS = dot(aE * rx, Ey) + dot(aE, Ey * ry) + dot(aE * rx, Ey * ry) + (2 * U_ + U_ * U_) * dot(aE * (1 + rx), Eyh)
        BS = BS + float(np.sum(2 * a + 3)) * TINY + n * TINY
        BS = BS + gamma(n + 2) * (S + BS)
        # R_x = sum of ((a E_x)(x - g)) E_y
        armx, army = np.abs(ex) + dex, np.abs(ey) + dey
        Ax = aE * -ex
        dAx = aE * r1 * armx + aE * dex + U_ * aE * (1 + r1) * armx + TINY
        Rx = np.dot(Ax.T, Ey)
        RAx = dot(np.abs(Ax), Ey)
        BRx = dot(dAx, Eyh) + dot(np.abs(Ax), Ey * ry) + U_ * dot(np.abs(Ax) + dAx, Eyh) + n * TINY
        # R_y = sum of (a E_x)(E_y (y - g))
        By = Ey * -ey
        dBy = Ey * ry * army + Ey * dey + U_ * Eyh * army + TINY
        Ry = np.dot(aE.T, By)
        RAy = dot(aE, np.abs(By))
        BRy = dot(aE * r1, np.abs(By) + dBy) + dot(aE, dBy) + U_ * dot(aE * (1 + r1), np.abs(By) + dBy) + n * TINY
        if T is np.float64:                            # (a term below 2^-1022 has lost digits here: 2^-1074 each at most)
            reach = 1 + float(np.max(np.abs(ex))) + float(np.max(np.abs(ey)))
            BRx = BRx + float(np.sum(2 * a + 4)) * TINY * reach
            BRy = BRy + float(np.sum(2 * a + 4)) * TINY * reach
        BRx = BRx + gamma(n + 2) * (RAx + BRx)
        BRy = BRy + gamma(n + 2) * (RAy + BRy)
        norm = T(W_exact) * hs * ht * T(cc.TWO_PI)
        rel_norm = (n - 1) * 2 * U_ + 6 * U_
        T00, T10, T01 = S / norm, Rx / hs / norm, Ry / ht / norm
        dT00 = BS / norm + (T00 + BS / norm) * rel_norm + 3 * TINY
        dT10 = BRx / hs / norm + (np.abs(T10) + BRx / hs / norm) * (rel_norm + 2 * U_) + TINY * (1 + 1 / norm)
        dT01 = BRy / ht / norm + (np.abs(T01) + BRy / ht / norm) * (rel_norm + 2 * U_) + TINY * (1 + 1 / norm)
        if is_open(*bnd_s):                            # (the sum is not formed: +0.0 by definition, and a1 = 0 exactly)
            T10, dT10 = np.zeros_like(T10), np.zeros_like(dT10)
        if is_open(*bnd_t):
            T01, dT01 = np.zeros_like(T01), np.zeros_like(dT01)
        (u0, u1, u2, dx), (du0, du1, du2, ddx) = ([np.asarray(q)[:, None] for q in part] for part in _consts(gx, dgx, bnd_s, prm_s[0], prm_s[2], prm_s[3], G, T))
        (v0, v1, v2, dy), (dv0, dv1, dv2, ddy) = ([np.asarray(q)[None, :] for q in part] for part in _consts(gy, dgy, bnd_t, prm_t[0], prm_t[2], prm_t[3], G, T))
        uv0, duv0 = _prod(u0, du0, v0, dv0)
        f0 = T00 / uv0
        df0 = (dT00 + f0 * duv0) / np.maximum(uv0 - duv0, TINY) + U_ * f0 + TINY
        d1, dd1 = _prod(uv0, duv0, dx, ddx)
        det, ddet = _prod(d1, dd1, dy, ddy)
        u02, du02 = _prod(u0, du0, u2, du2)
        v02, dv02 = _prod(v0, dv0, v2, dv2)
        u11, du11 = _prod(u1, du1, u1, du1)
        v11, dv11 = _prod(v1, dv1, v1, dv1)
        m1, dm1 = _prod(u02, du02, v02, dv02)
        m2, dm2 = _prod(u11, du11, v11, dv11)
        k00 = m1 - m2
        dk00 = dm1 + dm2 + U_ * (np.abs(k00) + dm1 + dm2) * 1.01
        u01, du01 = _prod(u0, du0, u1, du1)
        v01, dv01 = _prod(v0, dv0, v1, dv1)
        k10, dk10 = _prod(u01, du01, dy, ddy)
        k01, dk01 = _prod(v01, dv01, dx, ddx)
        w0, dw0 = _prod(T00, dT00, k00, dk00)
        w1, dw1 = _prod(T10, dT10, k10, dk10)
        w2, dw2 = _prod(T01, dT01, k01, dk01)
        w = (w0 - w1) - w2
        dw = dw0 + dw1 + dw2 + 2 * U_ * (np.abs(w0) + np.abs(w1) + np.abs(w2) + dw0 + dw1 + dw2) * 1.01 + 2 * TINY
        f1 = w / det
        det_lo, f0_lo = det - ddet, f0 - df0
        df1 = (dw + np.abs(f1) * ddet) / np.where(det_lo > 0, det_lo, 1.0) + U_ * np.abs(f1) + TINY
        r = f1 / f0
        dr = (df1 + np.abs(r) * df0) / np.where(f0_lo > 0, f0_lo, 1.0) + U_ * np.abs(r)
        exx = np.minimum(r, T(4)) - 1
        dexx = dr + U_ * (np.abs(exx) + dr)
        rho = np.where(f0 > 0, f0 * np.exp(exx), 0.0)
        q = (2 * EXP_ULPS + 1) * U_ * 1.01
        Ex_ = np.expm1(dexx)
        bound = rho * (Ex_ + (1 + Ex_) * q) + df0 * np.exp(exx + dexx) * (1 + q) + TINY
        unknown = ~(f0_lo > 0) | ~(det_lo > 0) | ~np.isfinite(bound)
        bound = np.where(unknown, np.where(det_lo > 0, (f0 + df0) * E3 + TINY, np.inf), bound)
    return rho, bound


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
class Case(cc.Case):
    """contours_cases.Case with the bounds of its CHOSEN columns: lo[nc], hi[nc], and their kinds"""

    def __init__(self, name, a, x, d, cols, lo, hi, kinds, grid=64, scale=1.0, probs=PROBS):
        cc.Case.__init__(self, name, a, x, d, cols, grid=grid, scale=scale, probs=probs)
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        self.kinds = tuple(kinds)

    @property
    def bounds(self):
        return (self.lo, self.hi)

    def open_t(self, t):
        return is_open(self.lo[t], self.hi[t])


def _bounds_of(kind, a, xpair, grid, scale):
    """the bounds of column 0 of ``xpair`` by its kind (marginals_bounds_cases'), at THIS rule's h; every bound an integer / 1024"""
    col = xpair[:, 0]
    used = col[a != 0.0]
    mn, mx = float(used.min()), float(used.max())
    if kind == "open":
        return -INF, INF
    if kind == "lower_at_min":
        return mn, INF
    if kind == "lower_below_min":                      # 1.5 h below the smallest sample: the grid is not cut, the constants are not 1
        h = float(ct.measure(a, xpair, (0, 1), (0.5,), grid, scale)["h"][0])
        return math.floor((mn - 1.5 * h) * 1024.0) / 1024.0, INF
    if kind == "both":
        return mn, mx
    if kind == "upper":
        return -INF, mx
    return 0.0, INF


def make(name, n, d, cols, grid, wkind, seed, kinds=None, scale=1.0):
    """contours_cases.make's generators; chosen column t is of the kind kinds[t] (none given: KINDS[t % 6])"""
    rng = np.random.default_rng(seed)
    a, zero = cc.weights(rng, n, wkind)
    x = np.stack([cc.column(rng, n, j) for j in range(d + 2)], axis=1)
    kinds = [KINDS[t % 6] for t in range(len(cols))] if kinds is None else list(kinds)
    for t, kind in enumerate(kinds):
        if kind == "gamma_at_0":                       # an exponential-shaped column: the density is highest at the bound
            x[:, cols[t]] = np.round(rng.gamma(1.0, 1.0, n) * 64.0) / 64.0
    lo, hi = np.full(len(cols), -INF), np.full(len(cols), INF)
    for t, kind in enumerate(kinds):
        other = cols[(t + 1) % len(cols)]
        lo[t], hi[t] = _bounds_of(kind, a, x[:, [cols[t], other]], grid, scale)
    if zero.size:
        x[zero] = np.tile([np.nan, np.inf, -np.inf], -(-x.shape[1] // 3))[:x.shape[1]]
    return Case(name, a, x, d, cols, lo, hi, kinds, grid=grid, scale=scale)


# (n, nc, G, weights, the chosen columns' kinds): the k-step tail (2, 5), the chunk edge (16, 17), the tile edge (513), three parts (1025),
# 17 tiles: the part cap with uneven parts (8705); nc = 6: a full group and a one-column group; ld = d + 2.  The first nc = 6 case runs
# through all six kinds in their order; the second has two open columns, so that an open-open pair stands next to bounded ones; a case of
# three columns has an open one, on the x axis in one and on the y axis in another
K = dict(o="open", m="lower_at_min", b="lower_below_min", w="both", u="upper", g="gamma_at_0")
PLAN = [(2, 2, 32, "integer", "om"), (5, 3, 64, "fractional", "bow"), (16, 2, 32, "unit", "ug"), (17, 3, 64, "integer", "omb"),
        (513, 6, 64, "fractional", "ombwug"), (1025, 6, 32, "integer", "wogomu"), (8705, 3, 64, "unit", "ugo")]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for i, (n, nc, G, kind, kinds) in enumerate(PLAN):
        name = "n%d_nc%d_G%d_%s" % (n, nc, G, kind)
        out[name] = make(name, n, nc, tuple(range(nc)), G, kind, 500 + i, kinds=[K[k] for k in kinds])
    out["n513_d127_last_two"] = make("n513_d127_last_two", 513, 127, (125, 126), 64, "fractional", 600, kinds=("gamma_at_0", "open"))
    return out


def open_case(c):
    """the same rows with every bound open"""
    return Case(c.name + "_open", c.a, c.x, c.d, c.cols, np.full(c.nc, -INF), np.full(c.nc, INF), ("open",) * c.nc, grid=c.grid, scale=c.scale, probs=c.probs)


def sub_case(c, ts):
    """the chosen columns ``ts`` of a case alone"""
    ts = list(ts)
    return Case(c.name + "_sub", c.a, c.x, c.d, [c.cols[t] for t in ts], c.lo[ts], c.hi[ts], [c.kinds[t] for t in ts], grid=c.grid, scale=c.scale, probs=c.probs)


def oracle_pairs(case):
    """the pairs the oracle is asked about: at most three, a bounded-bounded, an open-bounded / bounded-open and the last among them"""
    allp = ct.pairs(case.nc)
    P = len(allp)
    want = []
    for pick in (lambda s, t: not case.open_t(s) and not case.open_t(t), lambda s, t: case.open_t(s) != case.open_t(t), lambda s, t: case.open_t(s) and case.open_t(t)):
        want += [p for p, (s, t) in enumerate(allp) if pick(s, t)][:1]
    want = sorted(set(want + [P - 1]))[:3]
    return [(p, allp[p][0], allp[p][1]) for p in want]


# ---- the checks ----------------------------------------------------------------------------------------------------------------------
def _prm(got, t):
    return tuple(float(got[k][t]) for k in ("h", "c", "lo", "step"))


def _bnd(case, t):
    return (float(case.lo[t]), float(case.hi[t]))


_CACHE = {}


def _cached(kind, case, s, t, got, fn):
    key = (kind, case.name, tuple(case.cols), s, t, _prm(got, s), _prm(got, t))
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def dense_cached(case, s, t, got, T=LD):
    a, xs, xt = cc.pair_data(case, s, t)
    return _cached("dense" if T is LD else "dense64", case, s, t, got,
                   lambda: dense(a, xs, xt, case.exact["W"], _prm(got, s), _prm(got, t), _bnd(case, s), _bnd(case, t), case.grid, T))


def ends_of(got, s, t):
    return (got["at_lo"][s] == 1.0, got["at_hi"][s] == 1.0, got["at_lo"][t] == 1.0, got["at_hi"][t] == 1.0)


def check_grid(case, got, t):
    """step 3" on the reported h: the grid ends on a bound it would cross, and nowhere else"""
    ex, h, G = case.exact, got["h"][t], case.grid
    L, U = case.lo[t], case.hi[t]
    lo0, hi0 = ex["min"][t] - 3.0 * h, ex["max"][t] + 3.0 * h
    at_lo, at_hi = L >= lo0, U <= hi0
    lo, hi = (L if at_lo else lo0), (U if at_hi else hi0)
    assert (got["at_lo"][t], got["at_hi"][t]) == (float(at_lo), float(at_hi)) and got["lo"][t] == lo, (case.name, t, got["at_lo"][t], got["at_hi"][t], got["lo"][t], lo)
    assert mc.within_ulps(got["step"][t], (hi - lo) / float(G - 1), 1) and (got["bound_lo"][t], got["bound_hi"][t]) == (L, U), (case.name, t)


def assert_decisions(got, p, s, t, probs, who=""):
    """the block's decisions of pair p are the serial rule's on the block's own densities, bit for bit (``contours.decide_bounded``)"""
    mx, my, md, per = ct.decide_bounded(got["density"][p], got["lo"][s], got["step"][s], got["lo"][t], got["step"][t], probs, ends_of(got, s, t))
    assert (got["mode_x"][p], got["mode_y"][p], got["mode_density"][p]) == (mx, my, md) and md == np.max(got["density"][p]), (who, p, "mode")
    for i, k in enumerate(ct.P_KEYS):
        assert np.array_equal(np.asarray(got[k])[:, p], per[:, i]), (who, p, k, np.asarray(got[k])[:, p], per[:, i])


def decisions(rho, bound, w, probs, dens, ends, who=""):
    """contours_cases.decisions with the cell weights w (flat): the selection of the densities ``dens`` against the exact densities
    ``rho``; asserts agreement on every decided cell; -> the undecided cells per p"""
    N = rho.size
    G = int(round(N ** 0.5))
    order = np.lexsort((np.arange(N), -rho))
    cum = np.cumsum((rho * w)[order])
    Z = cum[-1]
    got_order, got_cuts = ct.selection_bounded(dens, probs, ends)
    out = []
    for p, gcut in zip(probs, got_cuts):
        target = LD(p) * Z
        cut = min(int(np.searchsorted(cum, target, side="left")), N - 1)
        kc = order[cut]
        und = np.abs(rho - rho[kc]) <= bound + bound[kc]
        near = 4 * G * G * U_ * Z
        if abs(cum[cut] - target) <= near or (cut > 0 and abs(cum[cut - 1] - target) <= near):
            und[order[max(cut - 1, 0):cut + 2]] = True
        want = np.zeros(N, dtype=bool)
        want[order[:cut + 1]] = True
        sel = np.zeros(N, dtype=bool)
        sel[got_order[:gcut + 1]] = True
        wrong = np.flatnonzero(~und & (want != sel))
        assert wrong.size == 0, (who, p, wrong[:8], "decided cells selected differently")
        assert und[kc]
        out.append(int(und.sum()))
    return out


def check_pair(case, got, p, s, t, what="", stats=None):
    """pair p of a bounded block: every density against ``dense`` within the bound (the query cells against mpmath), the decisions redone
    bit for bit on the block's own densities, and the selection against the oracle on every decided cell"""
    a, xs, xt = cc.pair_data(case, s, t)
    G = case.grid
    for z in (s, t):
        check_grid(case, got, z)
    rho, bound = dense_cached(case, s, t, got)
    dev = np.asarray(got["density"][p], dtype=np.float64)
    held = np.isfinite(bound)
    worst = float(np.max(np.where(held, np.abs(dev.astype(LD) - rho) / np.where(held, bound, 1), 0)))
    cells = cc.query_cells(G, 3 * a.size, int(np.argmax(dev)))
    W = sc.Fraction(case.exact["W"])
    exact = _cached("mp", case, s, t, got,
                    lambda: oracle_cells(a, xs, xt, mpmath.mpf(W.numerator) / W.denominator, _prm(got, s), _prm(got, t), _bnd(case, s), _bnd(case, t), cells))
    worst_mp = worst_ld = 0.0
    for (kx, ky), ex in zip(cells, exact):
        if not held[kx, ky]:
            continue
        bk = mc._mp(bound[kx, ky])
        worst_ld = max(worst_ld, float(abs(mc._mp(rho[kx, ky]) - ex) / (bk / 100)))
        worst_mp = max(worst_mp, float(abs(mpmath.mpf(float(dev[kx, ky])) - ex) / bk))
    assert_decisions(got, p, s, t, case.probs, (case.name, what))
    ends = ends_of(got, s, t)
    w = ct.cell_weights(G, ends).reshape(-1)
    undecided = decisions(rho.reshape(-1), bound.reshape(-1), w, case.probs, dev, ends, (case.name, p))
    assert decisions(rho.reshape(-1), bound.reshape(-1), w, case.probs, rho.astype(np.float64), ends, (case.name, p, "oracle")) == undecided
    if stats is not None:
        stats["density"] = max(stats.get("density", 0.0), worst, worst_mp)
        stats["undecided"] = max(stats.get("undecided", 0), max(undecided))
    print("%s %-24s pair %-3d (%d %s, %d %s) ends %d%d%d%d error/bound: all %.3g  mpmath %.3g on %d cells  (extended format / mpmath: %.3g of a hundredth)  "
          "cells not held %d  undecided %s" % (what, case.name, p, case.cols[s], case.kinds[s], case.cols[t], case.kinds[t], ends[0], ends[1], ends[2], ends[3], worst,
                                               worst_mp, len(cells), worst_ld, int((~held).sum()), undecided))
    assert worst <= 1.0 and worst_mp <= 1.0 and worst_ld <= 1.0, (case.name, p, worst, worst_mp, worst_ld)
    assert max(undecided) <= MAX_UNDECIDED, (case.name, p, undecided)


def assert_failed_pair(got, p, status, who=""):
    assert got["pair_status"][p] == status and np.all(np.asarray(got["cells"])[:, p] == -1.0), (who, p, got["pair_status"][p])
    for k in ("mode_x", "mode_y", "mode_density"):
        assert np.isnan(got[k][p]), (who, p, k)
    for k in ("level", "lower_x", "upper_x", "lower_y", "upper_y", "edge"):
        assert np.isnan(np.asarray(got[k])[:, p]).all(), (who, p, k)
    assert np.isnan(got["density"][p]).all(), (who, p)


def check_against_numpy(case, got, what=""):
    """ALL densities of a bounded block against ``measure_bounded``'s at the block's reported h, c, lo and step: within two bounds; all
    decisions bit for bit on the block's own densities; -> the largest ratio"""
    host = ct.measure_bounded(case.a, case.x[:, :case.d], case.cols, case.bounds, case.probs, case.grid, case.scale, at=got)
    assert np.array_equal(host["col_status"], got["col_status"]) and np.array_equal(host["pair_status"], got["pair_status"]), (
        case.name, host["col_status"], got["col_status"], host["pair_status"], got["pair_status"])
    worst = 0.0
    for p, (s, t) in enumerate(ct.pairs(case.nc)):
        if got["pair_status"][p] != 0:
            assert_failed_pair(got, p, got["pair_status"][p], case.name)
            continue
        _, b = dense_cached(case, s, t, got, np.float64)
        held = np.isfinite(b)
        ratio = float(np.max(np.where(held, np.abs(np.asarray(got["density"][p]) - host["density"][p]) / np.where(held, 2 * b, 1), 0)))
        assert ratio <= 1.0, (case.name, p, ratio)
        worst = max(worst, ratio)
        assert_decisions(got, p, s, t, case.probs, (case.name, what))
    print("%s %-24s every density against the NumPy form's at the reported parameters: %.3g of the two bounds" % (what, case.name, worst))
    return worst


def uncut(got, t):
    return got["at_lo"][t] == 0.0 and got["at_hi"][t] == 0.0


def assert_open_pairs_equal(case, got, plain, who=""):
    """every pair of two open columns whose grids are uncut: density, mode and decisions byte-equal to the rule without bounds; -> their
    number"""
    count = 0
    for p, (s, t) in enumerate(ct.pairs(case.nc)):
        if not (case.open_t(s) and case.open_t(t)) or got["pair_status"][p] != 0:
            continue
        assert uncut(got, s) and uncut(got, t), (who, p)
        for k in ct.PAIR_KEYS:
            assert np.array_equal(got[k][p], plain[k][p]), (who, p, k)
        for k in ct.P_KEYS:
            assert np.array_equal(np.asarray(got[k])[:, p], np.asarray(plain[k])[:, p]), (who, p, k)
        assert np.array_equal(got["density"][p], plain["density"][p]), (who, p, "density")
        count += 1
    return count


def equal_common(bounded, plain):
    """the shared keys bit for bit, NaN equal to NaN"""
    return all(np.array_equal(np.asarray(bounded[k], dtype=np.float64), np.asarray(plain[k], dtype=np.float64), equal_nan=True) for k in COMMON)


def pair_values(got, p):
    """everything a block says about pair p, as one array"""
    return np.concatenate([np.array([got[k][p] for k in ct.PAIR_KEYS]), np.concatenate([np.asarray(got[k])[:, p] for k in ct.P_KEYS]), np.asarray(got["density"][p]).reshape(-1)])


# ---- the exponential corner: the test that fails without the feature -----------------------------------------------------------------
EXP_T = 2.3534                                         # 1 - exp(-t)(1 + t) = 0.68


def exponential_case(seed, n=20000, grid=64):
    """two independent Exponential(1) columns bounded at 0, weights 1 .. 4"""
    rng = np.random.default_rng(seed)
    x = np.round(rng.exponential(1.0, (n, 2)) * 1024.0) / 1024.0
    a = rng.integers(1, 5, n).astype(np.float64)
    return Case("exponential_seed%d" % seed, a, np.concatenate([x, np.zeros((n, 2))], axis=1), 2, (0, 1), [0.0, 0.0], [INF, INF], ("gamma_at_0",) * 2, grid=grid)


def region_area(got, p, q, ends=None):
    """the cells-weighted area of the region of probability q of pair p"""
    G = got["grid"]
    s, t = ct.pairs(got["nc"])[p]
    ends = ends_of(got, s, t) if ends is None else ends
    order, cuts = ct.selection_bounded(got["density"][p], (q,), ends)
    w = ct.cell_weights(G, ends).reshape(-1)
    return float(np.sum(w[order[:cuts[0] + 1]]) * got["step"][s] * got["step"][t])


def assert_exponential_corner(case, got, who=""):
    """the exact assertions and the area of the 68 % region within the sampling term alone"""
    assert got["status"] == 0 and np.all(got["col_status"] == 0), (who, got["status"], got["col_status"])
    assert np.array_equal(got["at_lo"], [1.0, 1.0]), (who, got["at_lo"])
    assert got["mode_x"][0] == 0.0 and got["mode_y"][0] == 0.0, (who, got["mode_x"][0], got["mode_y"][0])
    assert np.all(np.asarray(got["lower_x"])[:, 0] == 0.0) and np.all(np.asarray(got["lower_y"])[:, 0] == 0.0), (who, got["lower_x"], got["lower_y"])
    assert np.all(np.asarray(got["edge"])[:, 0] == 1.0), (who, got["edge"])
    ess = got["W"] ** 2 / got["A2"]
    area68, area95 = region_area(got, 0, 0.68), region_area(got, 0, 0.95)
    tol = 5.0 * math.exp(EXP_T) * math.sqrt(0.68 * 0.32 / ess)
    print("%s %s corner density %.4f  68 %% area %.4f (truth %.4f, tolerance %.4f)  95 %% area %.4f (truth 11.252)" % (
        who, case.name, got["density"][0][0, 0], area68, EXP_T ** 2 / 2, tol, area95))
    assert abs(area68 - EXP_T ** 2 / 2) <= tol, (who, area68, EXP_T ** 2 / 2, tol)
    return area68, area95


# ---- the native program (tests/native/param_contours_bounds_check.cpp), a stand-alone sanitized build -----------------------------
def build_checker(directory):
    import os
    import subprocess
    from helpers import REPO
    exe = os.path.join(str(directory), "param_contours_bounds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "param_contours_bounds_check.cpp"), "-o", exe])
    return exe


def run_native(exe, tmp_path, systems, cols, probs, grid, scale):
    """[(a, x[n, ld], d, (lo[nc], hi[nc]))] through the serial driver -> one block dict per system"""
    import struct
    fin, fout = tmp_path / "conb_in.bin", tmp_path / "conb_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<qdq", grid, scale, len(cols)) + np.asarray(cols, dtype="<i8").tobytes())
        for a, x, d, (lo, hi) in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            x = x if x.ndim == 2 else x.reshape(len(a), -1)
            fh.write(struct.pack("<qqq", len(a), d, x.shape[1]) + x.tobytes() + np.ascontiguousarray(a, dtype="<f8").tobytes()
                     + np.ascontiguousarray(lo, dtype="<f8").tobytes() + np.ascontiguousarray(hi, dtype="<f8").tobytes())
    raw = cc._run(exe, "contours", fin, fout, len(systems))
    nc = len(cols)
    size = ct.HEAD + ct.PER_COL_BOUNDED * nc + (nc * (nc - 1) // 2) * (ct.PER_PAIR + ct.PER_P * probs.size + grid * grid)
    assert raw.size == size * len(systems)
    return [ct.from_block_bounded(raw[i * size:(i + 1) * size], nc, probs.size, grid) for i in range(len(systems))]


def native_case(exe, tmp_path, case):
    blk, = run_native(exe, tmp_path, [(case.a, case.x, case.d, case.bounds)], case.cols, case.probs, case.grid, case.scale)
    return blk


def check_decisions_native(exe, tmp_path, blocks, probs, grid):
    """the serial rule (steps 7" and 8") applied to each block's OWN density arrays equals the block's decisions bit for bit"""
    import struct
    fin, fout = tmp_path / "decb_in.bin", tmp_path / "decb_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    recs = [(b, p, s, t) for b in blocks if b["status"] == 0 for p, (s, t) in enumerate(ct.pairs(b["nc"])) if b["pair_status"][p] == 0]
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<q", grid))
        for b, p, s, t in recs:
            fh.write(struct.pack("<dddddddd", b["lo"][s], b["step"][s], b["lo"][t], b["step"][t], b["at_lo"][s], b["at_hi"][s], b["at_lo"][t], b["at_hi"][t])
                     + np.ascontiguousarray(b["density"][p], dtype="<f8").tobytes())
    raw = cc._run(exe, "decide", fin, fout, len(recs)).reshape(len(recs), 3 + ct.PER_P * probs.size)
    for (b, p, s, t), rec in zip(recs, raw):
        got = [b["mode_x"][p], b["mode_y"][p], b["mode_density"][p]] + [b[k][q][p] for q in range(probs.size) for k in ct.P_KEYS]
        assert np.array_equal(np.array(got), rec), (p, got, rec)
    return len(recs)
