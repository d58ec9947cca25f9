"""``contours=``: the 2-D joint posterior density of every pair of chosen parameters next to ln E -- a product-Gaussian kernel density
estimate on a regular G x G grid, its mode and the levels and regions that enclose given shares of it (the off-diagonal panels of a
triangle plot).

The rule (csrc/param_contours.hpp; docs/design/contours.md) takes what ``marginals=`` takes, plus a strictly increasing list ``cols`` of
2 .. 32 chosen columns.  The pairs are (cols[s], cols[t]), s < t, in the order (0,1), (0,2), .., (nc-2, nc-1); the first column of a pair
is its x axis.  In fp64, with G in {32, 64} and the bandwidth scale s:

    W, A2, ess, m_j, v_j, sd_j, min_j, max_j as ``marginals``
    h_j = (s * sd_j) * (1 / ess) ** (1 / 6),   c_j = 1 / ((2 * h_j) * h_j)
    lo_j = min_j - 3 * h_j,  step_j = ((max_j + 3 * h_j) - lo_j) / (G - 1),  g_jk = lo_j + k * step_j  (two roundings)
    E_j[r][k] = K(c_j (g_jk - x_rj)^2),  K(arg) = +0.0 where arg >= 746, else exp(-arg)
    S_ij[kx][ky] = sum over the used rows of (a_r * E_i[r][kx]) * E_j[r][ky],   rho = S / (((W * h_i) * h_j) * (2 pi))
    mode: the cell with the largest rho, the lowest flat index kx * G + ky among equals
    region of p: the cells by rho descending, then flat index ascending; rho accumulated serially in that order, Z the last running sum;
    selected: the positions up to and including the first whose running sum is >= p * Z (none: all of them); level the rho of the last
    selected position, cells their number, lower_x .. upper_y the bounding box in grid points, edge 1 where a selected cell lies on the
    grid's border

The densities are defined at the reported h, c, lo and step.  status 3, 5 and 6 are ``marginals``'; col_status 7 likewise, on this rule's
h, c and step; a pair with such a column has pair_status 7, NaN values and cells -1, and the other pairs do not notice.  Either logs one
WARNING, raises nothing and leaves ln E alone.  ``measure`` is the rule in NumPy, ``from_block`` takes the device's result block
(``_capi.param_contours_dev``), ``build`` makes ``info["contours"]`` from either, ``lines`` the lines that are logged and printed.

WITH HARD PRIOR BOUNDS (the key ``"bounds"`` of the keyword's dict; csrc/param_contours.hpp's steps 3" .. 8";
docs/design/contours_bounds.md) the grid of a column ends on a bound it would cross, the density is the three-term linear boundary
kernel of the product kernel on the rectangle in its positive form, and the running sum of a region gives a cell on such a grid end half
its weight per axis:

    R_x = sum of ((a_r E_i) (x_ri - g_kx)) E_j,  R_y = sum of (a_r E_i) (E_j (x_rj - g_ky))   (+0.0 for a column open on both sides)
    T00 = S / norm,  T10 = (R_x / h_i) / norm,  T01 = (R_y / h_j) / norm,  norm = ((W h_i) h_j) (2 pi)
    u = (a0, a1, a2), dx = den of ``marginals.boundary_constants`` on the x axis, v and dy on the y axis, at this rule's h, lo, step
    f0 = T00 / (u0 v0),  det = ((u0 v0) dx) dy
    f1 = ((T00 ((u0 u2) (v0 v2) - (u1 u1) (v1 v1)) - T10 ((u0 u1) dy)) - T01 ((v0 v1) dx)) / det
    rho = f0 > 0 ? f0 exp(min(f1 / f0, 4) - 1) : +0.0;  where det is not > 0 and finite: rho = f0

A used value outside a bound: col_status 8 (7 comes first); a pair takes the status of its failing column, the x axis' first.  A pair
whose two columns are open is the pair of the rule above bit for bit.  ``measure_bounded``, ``decide_bounded``, ``from_block_bounded``
and ``measure_bounded_native`` are the bounded forms; ``bounds_spec`` resolves the key.
"""
from __future__ import annotations

import logging

import numpy as np

from . import marginals as _marginals
from . import summary as _summary

logger = logging.getLogger("mcevidence_amd")

__all__ = ["wanted", "spec", "refuse", "pairs", "measure", "measure_native", "decide", "selection", "from_block", "build", "lines", "save", "GRIDS", "DEFAULT_GRID",
           "MAX_COLS", "STATUS_WORDS", "bounds_wanted", "bounds_spec", "measure_bounded", "decide_bounded", "selection_bounded", "from_block_bounded",
           "measure_bounded_native", "boundary_density", "COLUMN_OUTSIDE", "BOUND_KEYS"]

OK, COLUMN_BAD, COLUMN_OUTSIDE = 0, 7, _marginals.COLUMN_OUTSIDE
STATUS_WORDS = dict(_marginals.STATUS_WORDS)
GRIDS = (32, 64)
DEFAULT_GRID = 64
MAX_COLS = 32
TWO_PI = 6.283185307179586
HEAD, PER_COL, PER_PAIR, PER_P = 8, 9, 4, 7
COL_KEYS = ("col", "mean", "var", "sd", "h", "c", "lo", "step", "col_status")
PAIR_KEYS = ("mode_x", "mode_y", "mode_density", "pair_status")
P_KEYS = ("level", "cells", "lower_x", "upper_x", "lower_y", "upper_y", "edge")
BOUND_KEYS = _marginals.BOUND_KEYS                     # the column rows a bounded block has after col_status
PER_COL_BOUNDED = PER_COL + len(BOUND_KEYS)
_EXPECTED = ("None, True, up to %d probabilities 0 < p < 1, or a dict of probs, grid (one of %s), scale (finite, > 0) and params (2 to %d distinct names or "
             "indices of the first ndim parameters) expected" % (_marginals.MAX_PROBS, ", ".join(str(g) for g in GRIDS), MAX_COLS))
CHUNK_ROWS = 2048                                      # rows of the kernel matrices ``measure`` holds at a time


def wanted(contours):
    """is the keyword set?  (None / False: nothing changes)"""
    return contours is not None and contours is not False


def spec(contours, ndim=None, names=None):
    """the keyword's value -> (probs, grid, scale, cols), or None where it is not set; anything else: ``ValueError``.  ``cols``: the
    chosen columns, sorted; None while ``ndim`` is not known and no ``params`` are given (the default: all of the first ``ndim``)"""
    if not wanted(contours):
        return None
    bad = ValueError("contours=%r: %s" % (contours, _EXPECTED))
    params = None
    inner = contours
    if isinstance(contours, dict):
        if set(contours) - {"probs", "grid", "scale", "params", "bounds"}:
            raise bad
        params = contours.get("params")
        inner = {"probs": contours.get("probs", True), "grid": 512, "scale": contours.get("scale", 1.0)}
        grid = contours.get("grid", DEFAULT_GRID)
    else:
        grid = DEFAULT_GRID
    try:
        probs, _, scale = _marginals.spec(inner)
    except ValueError:
        raise bad
    if isinstance(grid, bool) or not isinstance(grid, (int, np.integer)) or int(grid) not in GRIDS:
        raise bad
    cols = None
    if params is not None:
        if isinstance(params, (str, bytes)) or not np.ndim(params):
            raise bad
        cols = []
        for p in params:
            if isinstance(p, (str, bytes)):
                p = p.decode() if isinstance(p, bytes) else p
                if names is None and ndim is None:     # (the data are not known yet: the name is looked up when they are)
                    cols.append(p)
                    continue
                if names is None or p not in list(names):
                    raise ValueError("contours=%r: the parameter %r is not among the names %s" % (contours, p, "(none known)" if names is None else list(names)))
                cols.append(list(names).index(p))
            elif isinstance(p, (int, np.integer)) and not isinstance(p, bool) and p >= 0:
                cols.append(int(p))
            else:
                raise bad
        if len(set(cols)) != len(cols) or not 2 <= len(cols) <= MAX_COLS or (ndim is not None and max(cols) >= ndim):
            raise bad
        cols = None if any(isinstance(p, str) for p in cols) else tuple(sorted(cols))
    elif ndim is not None:
        if ndim > MAX_COLS:
            raise ValueError("contours=%r: %d parameters; choose 2 to %d of them with params" % (contours, ndim, MAX_COLS))
        if ndim < 2:
            raise bad
        cols = tuple(range(int(ndim)))
    return probs, int(grid), scale, cols


def refuse(contours, brange=None, nbatch=1, isfunc=None):
    """the combinations every route refuses (and the values ``spec`` refuses), in ``information.refuse``'s words"""
    if spec(contours) is None:
        return
    if brange is not None or nbatch > 1:
        raise ValueError("contours with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (brange, nbatch))
    if isfunc:
        raise ValueError("contours with isfunc is not supported: importance sampling changes the weights and leaves the likelihood column unchanged")


def pairs(nc):
    """[(s, t)]: the pairs of the chosen columns in the rule's order"""
    return [(s, t) for s in range(nc) for t in range(s + 1, nc)]


def _nan_block(cols, npr, G, rows, status, column):
    nan = float("nan")
    nc = len(cols)
    P = nc * (nc - 1) // 2
    blk = dict(W=nan, A2=nan, rows=int(rows), status=int(status), column=int(column), grid=int(G), nc=nc)
    for k in COL_KEYS:
        blk[k] = np.full(nc, nan)
    blk["col"] = np.asarray(cols, dtype=np.float64)
    for k in PAIR_KEYS:
        blk[k] = np.full(P, nan)
    for k in P_KEYS:
        blk[k] = np.full((npr, P), nan)
    blk["density"] = np.full((P, G, G), nan)
    return blk


def cell_weights(G, ends):
    """the weights of step 8" [G, G]: ``ends`` = (at_lo, at_hi) of the x axis, then of the y axis; 1, 1/2 or 1/4, formed first"""
    return np.multiply.outer(_marginals.end_weights(G, ends[0], ends[1]), _marginals.end_weights(G, ends[2], ends[3]))


def _selection(rho, probs, ends=None):
    flat = np.asarray(rho, dtype=np.float64).reshape(-1)
    order = np.lexsort((np.arange(flat.size), -flat))  # rho descending, then the flat index ascending
    G = int(round(flat.size ** 0.5))
    cum = np.cumsum(flat[order] if ends is None else (cell_weights(G, ends).reshape(-1) * flat)[order])      # (serial, in that order)
    return order, [min(int(np.searchsorted(cum, p * cum[-1], side="left")), flat.size - 1) for p in probs]


def selection(rho, probs):
    """step 6 on one pair's densities [G, G] -> (order of the flat indices, [the cut position of every p])"""
    return _selection(rho, probs)


def selection_bounded(rho, probs, ends):
    """step 8": ``selection`` with the running sum of ``cell_weights`` times rho"""
    return _selection(rho, probs, tuple(bool(e) for e in ends))


def decide(rho, lox, stepx, loy, stepy, probs):
    """steps 5 and 6 on one pair's densities -> (mode_x, mode_y, mode_density, per[np][7]: level, cells, lower_x, upper_x, lower_y,
    upper_y, edge)"""
    return _decide(rho, lox, stepx, loy, stepy, probs)


def decide_bounded(rho, lox, stepx, loy, stepy, probs, ends):
    """steps 7" and 8" on one pair's densities -> what ``decide`` returns; ``ends`` = (at_lo, at_hi) of the x axis, then of the y axis"""
    return _decide(rho, lox, stepx, loy, stepy, probs, tuple(bool(e) for e in ends))


def _decide(rho, lox, stepx, loy, stepy, probs, ends=None):
    rho = np.asarray(rho, dtype=np.float64)
    G = rho.shape[0]
    flat = rho.reshape(-1)
    order, cuts = _selection(rho, probs, ends)
    gx, gy = _marginals.grid_points(lox, stepx, G), _marginals.grid_points(loy, stepy, G)
    per = []
    for cut in cuts:
        kx, ky = order[:cut + 1] // G, order[:cut + 1] % G
        edge = bool(np.any((kx == 0) | (kx == G - 1) | (ky == 0) | (ky == G - 1)))
        per.append([flat[order[cut]], float(cut + 1), gx[kx.min()], gx[kx.max()], gy[ky.min()], gy[ky.max()], 1.0 if edge else 0.0])
    return gx[order[0] // G], gy[order[0] % G], flat[order[0]], np.array(per).reshape(len(cuts), PER_P)


def kernel_values(c, lo, step, G, x):
    """E[r][k] = K(c (g_k - x_r)^2)"""
    e = _marginals.grid_points(lo, step, G)[None, :] - x[:, None]
    arg = c * (e * e)
    return np.where(arg >= _marginals.UNDERFLOW, 0.0, np.exp(-arg))


def boundary_density(T00, T10, T01, u, v):
    """step 6" on [G, G] arrays: u = (a0, a1, a2, den) of the x axis [G], v of the y axis [G]"""
    with np.errstate(all="ignore"):
        u0, u1, u2, dx = (np.asarray(q, dtype=np.float64)[:, None] for q in u)
        v0, v1, v2, dy = (np.asarray(q, dtype=np.float64)[None, :] for q in v)
        uv0 = u0 * v0
        f0 = T00 / uv0
        det = (uv0 * dx) * dy
        k00 = (u0 * u2) * (v0 * v2) - (u1 * u1) * (v1 * v1)
        f1 = ((T00 * k00 - T10 * ((u0 * u1) * dy)) - T01 * ((v0 * v1) * dx)) / det
        pos = f0 > 0.0
        slope = np.minimum(np.where(pos, f1 / np.where(pos, f0, 1.0), 0.0), _marginals.MAX_SLOPE)
        rho = np.where(pos, f0 * np.exp(slope - 1.0), 0.0)
        return np.where(pos & ~(np.isfinite(det) & (det > 0.0)), f0, rho)


def measure(a, x, cols, probs, grid=DEFAULT_GRID, scale=1.0, at=None):
    """The rule on host arrays: weights ``a`` [n], values ``x`` [n, d], the chosen columns ``cols`` -> dict(W, A2, rows, status, column,
    grid, nc, col .. col_status [nc], mode_x, mode_y, mode_density, pair_status [P], level .. edge [np][P], density [P][G][G]); the kernel
    matrices are formed in chunks of rows.  ``at``: another route's block -- its reported h, c, lo and step are taken instead of this
    form's own (the densities are defined at the reported values, and two routes' pow may differ in the last place)"""
    return _measure(a, x, cols, probs, grid, scale, at)


def measure_bounded(a, x, cols, bounds, probs, grid=DEFAULT_GRID, scale=1.0, at=None):
    """The rule with bounds on host arrays: ``measure``'s arguments and ``bounds`` = (lo[nc], hi[nc]) of the chosen columns
    (``bounds_spec``) -> ``measure``'s dict with bound_lo, bound_hi, at_lo, at_hi [nc].  col_status 8: a used value outside its bounds"""
    return _measure(a, x, cols, probs, grid, scale, at, bounds=bounds)


def _measure(a, x, cols, probs, grid, scale, at, bounds=None):
    """``measure`` (``bounds`` None: no first-moment sums, no boundary step, no bound keys) and ``measure_bounded``"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    probs = tuple(float(p) for p in probs)
    cols = [int(j) for j in cols]
    G = int(grid)
    if x.shape[0] != a.size:
        raise ValueError("contours: %d weights, %d rows" % (a.size, x.shape[0]))
    if not 2 <= len(cols) <= MAX_COLS or any(b <= a_ for a_, b in zip(cols, cols[1:])) or cols[0] < 0 or cols[-1] >= x.shape[1]:
        raise ValueError("contours: cols=%r (2 to %d strictly increasing columns below %d expected)" % (cols, MAX_COLS, x.shape[1]))
    nc, npr = len(cols), len(probs)
    if bounds is not None:
        L, U = (np.asarray(v, dtype=np.float64).reshape(-1) for v in bounds)
        if L.size != nc or U.size != nc or not np.all(L < U):
            raise ValueError("contours: bounds=%r (one lo < hi per chosen column expected)" % (bounds,))
    use = a != 0.0                                     # (a NaN weight is used: it is what status 3 reports)
    a, x = a[use], x[use]
    with np.errstate(all="ignore"):
        W = float(np.sum(a))
        status, column = OK, _summary.COLUMN_NONE
        badcols = np.flatnonzero(~np.isfinite(x).all(axis=0)) if a.size else np.zeros(0, dtype=int)
        if not (np.isfinite(a).all() and (a >= 0.0).all()):
            status = _marginals.NOT_FINITE
        elif badcols.size:
            status, column = _marginals.NOT_FINITE, int(badcols[0])
        elif not W > 0.0:
            status = _marginals.NO_WEIGHT
        elif a.size < 2:
            status = _marginals.FEW_ROWS
        out = _nan_block(cols, npr, G, a.size, status, column)
        if bounds is not None:
            for k in BOUND_KEYS:
                out[k] = np.full(nc, np.nan)
        if status != OK:
            return out
        if bounds is not None:
            out["bound_lo"], out["bound_hi"] = L.copy(), U.copy()
        xc = x[:, cols]
        A2 = float(np.sum(a * a))
        out["W"], out["A2"] = W, A2
        ess = W * W / A2
        mean = np.sum(a[:, None] * xc, axis=0) / W
        dev = xc - mean[None, :]
        var = np.sum(a[:, None] * (dev * dev), axis=0) / W
        sd = np.sqrt(var)
        h = (scale * sd) * np.float64(1.0 / ess) ** (1.0 / 6.0)
        c = 1.0 / ((2.0 * h) * h)
        mn, mx = xc.min(axis=0), xc.max(axis=0)
        lo = mn - 3.0 * h
        if bounds is None:
            step = ((mx + 3.0 * h) - lo) / float(G - 1)
        else:                                          # step 3": the column's own grid has to be one; then the ends move onto the bounds
            hi = mx + 3.0 * h
            base = _marginals._col_ok(sd, h, c, (hi - lo) / float(G - 1))
            outside = (mn < L) | (mx > U)
            at_lo, at_hi = L >= lo, U <= hi
            lo, hi = np.where(at_lo, L, lo), np.where(at_hi, U, hi)
            step = (hi - lo) / float(G - 1)
        if at is not None:
            keep = np.asarray(at["col_status"]) == OK
            h, c, lo, step = (np.where(keep, np.asarray(at[k], dtype=np.float64), v) for k, v in (("h", h), ("c", c), ("lo", lo), ("step", step)))
            if bounds is not None:
                at_lo, at_hi = (np.where(keep, np.asarray(at[k]) == 1.0, v) for k, v in (("at_lo", at_lo), ("at_hi", at_hi)))
        if bounds is None:
            good = (sd > 0.0) & np.isfinite(h) & (h > 0.0) & np.isfinite(c) & (c > 0.0) & np.isfinite(step) & (step > 0.0)
            out["col_status"] = np.where(good, float(OK), float(COLUMN_BAD))
        else:
            good = base & ~outside & np.isfinite(step) & (step > 0.0)
            out["col_status"] = np.where(base, np.where(outside, float(COLUMN_OUTSIDE), np.where(good, float(OK), float(COLUMN_BAD))), float(COLUMN_BAD))
            out["at_lo"], out["at_hi"] = np.where(good, at_lo.astype(np.float64), np.nan), np.where(good, at_hi.astype(np.float64), np.nan)
            is_open = np.isneginf(L) & np.isposinf(U)
            consts = [_marginals.boundary_constants(_marginals.grid_points(lo[t], step[t], G), L[t], U[t], h[t]) if good[t] else None for t in range(nc)]
        for k, v in (("mean", mean), ("var", var), ("sd", sd), ("h", h), ("c", c), ("lo", lo), ("step", step)):
            out[k] = np.where(good, v, np.nan)
        for p, (s, t) in enumerate(pairs(nc)):
            if not (good[s] and good[t]):
                out["pair_status"][p] = out["col_status"][s] if not good[s] else out["col_status"][t]
                out["cells"][:, p] = -1.0
                continue
            S = np.zeros((G, G))
            Rx, Ry = np.zeros((G, G)), np.zeros((G, G))    # (+0.0 where the column is open on both sides, and without bounds not read)
            for r0 in range(0, a.size, CHUNK_ROWS):
                sl = slice(r0, r0 + CHUNK_ROWS)
                ex = a[sl, None] * kernel_values(c[s], lo[s], step[s], G, xc[sl, s])
                ey = kernel_values(c[t], lo[t], step[t], G, xc[sl, t])
                S += ex.T @ ey
                if bounds is not None and not is_open[s]:
                    Rx += (ex * -(_marginals.grid_points(lo[s], step[s], G)[None, :] - xc[sl, s][:, None])).T @ ey
                if bounds is not None and not is_open[t]:
                    Ry += ex.T @ (ey * -(_marginals.grid_points(lo[t], step[t], G)[None, :] - xc[sl, t][:, None]))
            norm = ((W * h[s]) * h[t]) * TWO_PI
            rho = S / norm
            ends = None
            if bounds is not None:
                rho = boundary_density(rho, (Rx / h[s]) / norm, (Ry / h[t]) / norm, consts[s], consts[t])
                ends = (bool(at_lo[s]), bool(at_hi[s]), bool(at_lo[t]), bool(at_hi[t]))
            out["density"][p] = rho
            out["pair_status"][p] = float(OK)
            out["mode_x"][p], out["mode_y"][p], out["mode_density"][p], per = _decide(rho, lo[s], step[s], lo[t], step[t], probs, ends)
            for i, k in enumerate(P_KEYS):
                out[k][:, p] = per[:, i]
        return out


def from_block(block, nc, npr, G):
    """one system's result block of ``mce_param_contours_dev`` -> what ``measure`` returns"""
    return _from_block(block, nc, npr, G, COL_KEYS)


def from_block_bounded(block, nc, npr, G):
    """one system's result block of ``mce_param_contours_bounded_dev`` -> what ``measure_bounded`` returns"""
    return _from_block(block, nc, npr, G, COL_KEYS + BOUND_KEYS)


def _from_block(block, nc, npr, G, col_keys):
    block = np.asarray(block, dtype=np.float64)
    P = nc * (nc - 1) // 2
    at = HEAD
    col = block[at:at + len(col_keys) * nc].reshape(len(col_keys), nc)
    at += len(col_keys) * nc
    pair = block[at:at + PER_PAIR * P].reshape(PER_PAIR, P)
    at += PER_PAIR * P
    per = block[at:at + PER_P * npr * P].reshape(npr, PER_P, P)
    at += PER_P * npr * P
    out = dict(W=float(block[0]), A2=float(block[1]), rows=int(block[2]), status=int(block[3]), column=int(block[4]), grid=int(G), nc=int(nc))
    for i, k in enumerate(col_keys):
        out[k] = col[i].copy()
    for i, k in enumerate(PAIR_KEYS):
        out[k] = pair[i].copy()
    for i, k in enumerate(P_KEYS):
        out[k] = per[:, i, :].copy()
    out["density"] = block[at:at + P * G * G].reshape(P, G, G).copy()
    return out


def measure_native(a, x, cols, probs, grid=DEFAULT_GRID, scale=1.0, device=None):
    """``measure`` by the library from HOST arrays (``mce_param_contours_f64``, uploaded to ``device``)"""
    from . import _capi
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    blk, = _capi.param_contours([(x, x.shape[1], a)], cols, probs, grid, scale, device=int(device or 0))
    return from_block(blk, len(cols), len(probs), grid)


def measure_bounded_native(a, x, cols, bounds, probs, grid=DEFAULT_GRID, scale=1.0, device=None):
    """``measure_bounded`` by the library from HOST arrays (``mce_param_contours_bounded_f64``, uploaded to ``device``)"""
    from . import _capi
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    blk, = _capi.param_contours_bounded([(x, x.shape[1], a)], cols, [bounds], probs, grid, scale, device=int(device or 0))
    return from_block_bounded(blk, len(cols), len(probs), grid)


def bounds_wanted(contours):
    """does the keyword ask for boundary-corrected densities?  (the key ``"bounds"`` of its dict, other than None / False)"""
    return isinstance(contours, dict) and contours.get("bounds") is not None and contours.get("bounds") is not False


def bounds_spec(contours, names=None, ndim=None, root=None, bounds=None):
    """the keyword's ``"bounds"`` -> (lo[nc], hi[nc]) of the CHOSEN columns, or None where the key is not set.  True: the call's
    ``bounds=`` value (``ValueError`` beginning ``contours=`` where there is none); "ranges", a mapping name -> (lo, hi) or a sequence of
    one pair per parameter in use: as ``bounds=`` takes them (``marginals.bounds_spec``).  ``names``: the parameters in use"""
    if not bounds_wanted(contours):
        return None
    value = contours["bounds"]
    if value is True:
        if bounds is None:
            raise ValueError("contours=%r: \"bounds\": True takes the call's bounds=, and there is none" % (contours,))
        value = bounds
    sp = spec(contours, ndim=ndim, names=names)
    if sp[3] is None:
        raise ValueError("contours=%r: the chosen columns are not known here" % (contours,))
    try:
        lo, hi = _marginals.bounds_spec(value, names=names, ndim=ndim, root=root, marginals=True)
    except ValueError as e:
        raise ValueError("contours=%r: %s" % (contours, e))
    cols = list(sp[3])
    return lo[cols], hi[cols]


def build(blk, spec_, names=None):
    """``info["contours"]`` from a block (``measure`` / ``from_block``) and the keyword's ``spec``; a status other than 0, or pairs with
    one, log ONE WARNING"""
    probs, grid, scale, cols = spec_
    nc = len(blk["col"])
    chosen = [int(j) for j in blk["col"]]
    bad = [chosen[t] for t in range(nc) if blk["col_status"][t] == COLUMN_BAD]
    outside = [chosen[t] for t in range(nc) if blk["col_status"][t] == COLUMN_OUTSIDE]
    if blk["status"] != OK:
        logger.warning("contours: status %d (%s): every value is NaN" % (blk["status"], STATUS_WORDS[blk["status"]]))
    elif bad or outside:
        logger.warning("contours: " + "; ".join("column status %d (%s) in column%s %s" % (st, STATUS_WORDS[st], "s" if len(js) > 1 else "", ", ".join(str(j) for j in js))
                                                for st, js in ((COLUMN_BAD, bad), (COLUMN_OUTSIDE, outside)) if js) + ": NaN in their pairs")
    with np.errstate(all="ignore"):
        ess = blk["W"] * blk["W"] / blk["A2"]
    all_names = list(names) if names is not None else None
    out = {"probs": tuple(probs), "grid": int(grid), "scale": float(scale), "rows": blk["rows"], "sum_w": blk["W"], "ess": ess, "cols": chosen,
           "names": [all_names[j] if all_names is not None and j < len(all_names) else "p%d" % j for j in chosen],
           "pairs": [(chosen[s], chosen[t]) for s, t in pairs(nc)], "grid_lo": blk["lo"], "grid_step": blk["step"], "status": blk["status"], "column": blk["column"]}
    for k in ("mean", "sd", "h", "c", "col_status") + PAIR_KEYS + P_KEYS + ("density",) + (BOUND_KEYS if "bound_lo" in blk else ()):
        out[k] = blk[k]
    return out


def lines(m):
    """the lines logged and printed after the marginals lines and before the ln(B) lines: one header, then per pair: name_x name_y mode_x
    mode_y [level cells per p]"""
    head = " contours: {:<12s} {:<12s} {:>14s} {:>14s}".format("x", "y", "mode_x", "mode_y")
    for p in m["probs"]:
        head += " {:>14s} {:>6s}".format("level%g" % (100 * p), "cells")
    out = [head]
    nc = len(m["names"])
    for i, (s, t) in enumerate(pairs(nc)):
        ln = " contours: {:<12s} {:<12s} {:>14.8g} {:>14.8g}".format(m["names"][s], m["names"][t], m["mode_x"][i], m["mode_y"][i])
        for k in range(len(m["probs"])):
            n = m["cells"][k][i]
            ln += " {:>14.8g} {:>6s}".format(m["level"][k][i], "nan" if n != n else "%d" % n)
        out.append(ln)
    return out


def save(path, roots, infos):
    """``--contours-out``: one ``.npz`` with, per root r, names_r, pairs_r [P][2], grid_x_r / grid_y_r [P][G] (the two axes of every
    pair), density_r [P][G][G] and levels_r [np][P]; ``roots`` the list of their names"""
    arrays = {"roots": np.array([str(r) for r in roots])}
    for r, inf in enumerate(infos):
        m = (inf or {}).get("contours")
        if not m:
            continue
        G, nc = m["grid"], len(m["names"])
        axes = [_marginals.grid_points(lo, st, G) for lo, st in zip(m["grid_lo"], m["grid_step"])]
        arrays["names_%d" % r] = np.array(m["names"])
        arrays["pairs_%d" % r] = np.array(m["pairs"], dtype=np.int64).reshape(-1, 2)
        arrays["grid_x_%d" % r] = np.stack([axes[s] for s, _ in pairs(nc)])
        arrays["grid_y_%d" % r] = np.stack([axes[t] for _, t in pairs(nc)])
        arrays["density_%d" % r] = np.asarray(m["density"])
        arrays["levels_%d" % r] = np.asarray(m["level"])
        for k in BOUND_KEYS:
            if k in m:
                arrays["%s_%d" % (k, r)] = np.asarray(m[k])
    np.savez(path, **arrays)
