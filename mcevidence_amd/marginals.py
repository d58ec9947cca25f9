"""``marginals=``: the 1-D marginalised posterior density of every parameter next to ln E -- a Gaussian kernel density estimate on a
regular grid, its mode and its highest-posterior-density (HPD) regions.

The rule (csrc/param_marginals.hpp; docs/design/marginals.md) takes what ``summary=`` takes: the s1 partition the estimator sums over,
a_i the weights, x_ij the RAW (unwhitened) values of the first ``ndim`` parameter columns.  A row with a_i == 0 is skipped entirely.  In
fp64, with G grid points and the bandwidth scale s:

    W = sum a,  A2 = sum a^2,  ess = W * W / A2,  m_j, v_j (the second pass about the computed m_j), sd_j = sqrt(v_j), min_j, max_j
    h_j = (s * sd_j) * (4 / (3 * ess)) ** 0.2,   c_j = 1 / ((2 * h_j) * h_j)
    lo_j = min_j - 3 * h_j,  hi_j = max_j + 3 * h_j,  step_j = (hi_j - lo_j) / (G - 1),  g_k = lo_j + k * step_j  (two roundings)
    S_jk = sum over the used rows of a_i K(c_j (g_k - x_ij)^2),  K(arg) = +0.0 where arg >= 746, else exp(-arg)
    rho_jk = S_jk / ((W * h_j) * sqrt(2 pi))
    mode: the grid point with the largest rho, the lowest k among equals
    HPD region of p: the grid points by rho descending, then k ascending; rho accumulated serially in that order, Z the last running
    sum; selected: the positions up to and including the first whose running sum is >= p * Z (none: all of them); lower / upper the
    smallest / largest selected g, pieces the maximal runs of consecutive selected k, edge 1 where k = 0 or k = G - 1 is selected

The densities are defined at the reported h, c, lo and step.  status 3 and 5 are ``summary``'s, 6: fewer than 2 used rows; with a status
other than 0 every value is NaN.  col_status 7: sd_j is 0, or h_j, c_j or step_j is not finite and > 0 -- that column is NaN with
pieces -1, and the other columns do not notice.  Either logs one WARNING, raises nothing and leaves ln E alone.  ``measure`` is the rule
in NumPy, ``from_block`` takes the device's result block (``_capi.param_marginals_dev``), ``build`` makes ``info["marginals"]`` from
either, ``lines`` the lines that are logged and printed, ``save`` the ``.npz`` file of ``--marginals-out``.

``bounds=`` next to ``marginals=`` (csrc/param_marginals_bounds.hpp; docs/design/marginals_bounds.md) honours hard prior bounds (L, U) of
a column: a used value outside them is col_status 8; the grid ends on a bound it would cross (at_lo / at_hi); S_jk is joined by
R_jk = sum a_i K(..) (x_ij - g_k), and with T0 = S / norm, T1 = (R / h) / norm and the moments a0, a1, a2 of the standard normal kernel
inside the bounds the density is Jones' linear boundary kernel in its positive form, rho = f0 exp(min(f1 / f0, 4) - 1), f0 = T0 / a0,
f1 = (a2 T0 - a1 T1) / (a0 a2 - a1^2); the HPD sums count half a cell where the grid ends on a bound.  A column without bounds keeps its
bits.  ``bounds_spec`` resolves the keyword's value, ``measure_bounded`` is the rule in NumPy, ``from_block_bounded`` takes the block of
``_capi.param_marginals_bounded_dev``.
"""
from __future__ import annotations

import logging
import math
import os

import numpy as np

from . import summary as _summary

logger = logging.getLogger("mcevidence_amd")

__all__ = ["wanted", "spec", "refuse", "measure", "measure_native", "decide", "hpd_selection", "grid_points", "from_block", "build", "lines", "save", "STATUS_WORDS", "DEFAULT_PROBS",
           "MAX_PROBS", "GRIDS", "DEFAULT_GRID", "UNDERFLOW", "bounds_spec", "measure_bounded", "measure_bounded_native", "decide_bounded",
           "hpd_selection_bounded", "boundary_constants", "boundary_density", "from_block_bounded", "COLUMN_OUTSIDE"]

OK, NOT_FINITE, NO_WEIGHT, FEW_ROWS, COLUMN_BAD = 0, 3, 5, 6, 7
STATUS_WORDS = dict(_summary.STATUS_WORDS)
STATUS_WORDS[FEW_ROWS] = "fewer than 2 rows with a weight"
STATUS_WORDS[COLUMN_BAD] = "the column is constant, or its bandwidth or grid step is not finite and positive"
DEFAULT_PROBS = (0.68, 0.95)
MAX_PROBS = 7
GRIDS = (64, 128, 256, 512, 1024)
DEFAULT_GRID = 512
UNDERFLOW = 746.0                                      # kKdeUnderflow of csrc/kde_shift.hpp: a kernel value at or above it is +0.0
SQRT_2PI = 2.5066282746310002
HEAD = 8                                               # MCE_MARGINALS_HEAD: W, A2, rows used, status, column, grid, np, reserved
COL_KEYS = ("mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density", "col_status")
PER_COL = len(COL_KEYS)                                # the per-column rows of a result block
PER_P = 4                                              # lower, upper, pieces, edge
_EXPECTED = "None, True, up to %d probabilities 0 < p < 1, or a dict of probs, grid (one of %s) and scale (finite, > 0) expected" % (
    MAX_PROBS, ", ".join(str(g) for g in GRIDS))
CHUNK_BYTES = 1 << 25                                  # of the (rows, G) kernel matrix ``measure`` holds at a time


def wanted(marginals):
    """is the keyword set?  (None / False: nothing changes)"""
    return marginals is not None and marginals is not False


def spec(marginals):
    """the keyword's value -> (probs, grid, scale), or None where it is not set; anything else: ``ValueError``"""
    if not wanted(marginals):
        return None
    bad = ValueError("marginals=%r: %s" % (marginals, _EXPECTED))
    probs, grid, scale = DEFAULT_PROBS, DEFAULT_GRID, 1.0
    if isinstance(marginals, dict):
        if set(marginals) - {"probs", "grid", "scale"}:
            raise bad
        probs, grid, scale = marginals.get("probs", True), marginals.get("grid", DEFAULT_GRID), marginals.get("scale", 1.0)
    else:
        probs = marginals
    if probs is True or probs is None:
        probs = DEFAULT_PROBS
    elif isinstance(probs, (str, bytes, dict)) or probs is False:
        raise bad
    try:
        probs = tuple(float(p) for p in (probs if np.ndim(probs) else (probs,)))
        scale = float(scale)
        if isinstance(grid, bool) or int(grid) != grid:
            raise bad
        grid = int(grid)
    except (TypeError, ValueError):
        raise bad
    if not 1 <= len(probs) <= MAX_PROBS or not all(0.0 < p < 1.0 for p in probs) or grid not in GRIDS or not (np.isfinite(scale) and scale > 0.0):
        raise bad
    return probs, grid, scale


def refuse(marginals, brange=None, nbatch=1, isfunc=None):
    """the combinations every route refuses (and the values ``spec`` refuses), in ``information.refuse``'s words"""
    if spec(marginals) is None:
        return
    if brange is not None or nbatch > 1:
        raise ValueError("marginals with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (brange, nbatch))
    if isfunc:
        raise ValueError("marginals with isfunc is not supported: importance sampling changes the weights and leaves the likelihood column unchanged")


def _nan_block(d, npr, G, rows, status, column):
    nan = float("nan")
    col = np.full(d, nan)
    blk = dict(W=nan, A2=nan, rows=int(rows), status=int(status), column=int(column), grid=int(G))
    for k in COL_KEYS:
        blk[k] = col.copy()
    for k in ("lower", "upper", "pieces", "edge"):
        blk[k] = np.full((npr, d), nan)
    blk["density"] = np.full((d, G), nan)
    return blk


def grid_points(lo, step, G):
    """g_k = lo + k * step: a product and a sum, two roundings"""
    return lo + np.arange(G, dtype=np.float64) * step


def end_weights(G, at_lo, at_hi):
    """the weights of step 8': half a cell where the grid ends on a bound"""
    w = np.ones(G)
    if at_lo:
        w[0] = 0.5
    if at_hi:
        w[G - 1] = 0.5
    return w


def _hpd_selection(rho, probs, ends=None):
    """step 6 (``ends`` = (at_lo, at_hi): step 8', with ``end_weights``) on one column's densities"""
    rho = np.asarray(rho, dtype=np.float64)
    G = rho.size
    order = np.lexsort((np.arange(G), -rho))           # rho descending, then k ascending
    cum = np.cumsum(rho[order] if ends is None else (end_weights(G, *ends) * rho)[order])      # (serial, in that order)
    masks = []
    for p in probs:
        cut = min(int(np.searchsorted(cum, p * cum[-1], side="left")), G - 1)
        sel = np.zeros(G, dtype=bool)
        sel[order[:cut + 1]] = True
        masks.append(sel)
    return order, masks


def hpd_selection(rho, probs):
    """step 6 on one column's densities -> (order, [the mask of the selected grid points of every p])"""
    return _hpd_selection(rho, probs)


def _decide(rho, lo, step, probs, ends=None):
    rho = np.asarray(rho, dtype=np.float64)
    G = rho.size
    order, masks = _hpd_selection(rho, probs, ends)
    g = grid_points(lo, step, G)
    lower, upper, pieces, edge = [], [], [], []
    for sel in masks:
        at = np.flatnonzero(sel)
        lower.append(g[at[0]])
        upper.append(g[at[-1]])
        pieces.append(float(np.count_nonzero(sel & ~np.concatenate(([False], sel[:-1])))))
        edge.append(1.0 if sel[0] or sel[-1] else 0.0)
    return g[order[0]], rho[order[0]], np.array(lower), np.array(upper), np.array(pieces), np.array(edge)


def decide(rho, lo, step, probs):
    """steps 5 and 6 on one column's densities -> (mode, mode_density, lower[np], upper[np], pieces[np], edge[np])"""
    return _decide(rho, lo, step, probs)


def _col_ok(sd, h, c, step):
    return (sd > 0.0) & np.isfinite(h) & (h > 0.0) & np.isfinite(c) & (c > 0.0) & np.isfinite(step) & (step > 0.0)


def measure(a, x, probs, grid=DEFAULT_GRID, scale=1.0, at=None):
    """The rule on host arrays: weights ``a`` [n], values ``x`` [n, d] -> dict(W, A2, rows, status, column, grid, mean, var, sd, h, c,
    lo, step, mode, mode_density, col_status [d], lower, upper, pieces, edge [np][d], density [d][G]); the kernel matrix is formed in
    chunks of rows.  ``at``: another route's block -- its reported h, c, lo and step are taken instead of this form's own (the densities
    are defined at the reported values, and two routes' pow may differ in the last place): what a comparison of two routes needs"""
    return _measure(a, x, probs, grid, scale, at)


def _measure(a, x, probs, grid, scale, at, bounds=None):
    """``measure`` (``bounds`` None: no R, no boundary step, no bound keys) and ``measure_bounded`` (``bounds`` = (lo[d], hi[d]))"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    probs = tuple(float(p) for p in probs)
    G = int(grid)
    if x.shape[0] != a.size:
        raise ValueError("marginals: %d weights, %d rows" % (a.size, x.shape[0]))
    d, npr = x.shape[1], len(probs)
    if bounds is not None:
        L, U = (np.asarray(v, dtype=np.float64).reshape(-1) for v in bounds)
        if L.size != d or U.size != d or not np.all(L < U):
            raise ValueError("bounds=%r: one lo < hi per column expected" % (bounds,))
    use = a != 0.0                                     # (a NaN weight is used: it is what status 3 reports)
    a, x = a[use], x[use]
    with np.errstate(all="ignore"):
        W = float(np.sum(a))
        status, column = OK, _summary.COLUMN_NONE
        badcols = np.flatnonzero(~np.isfinite(x).all(axis=0)) if a.size else np.zeros(0, dtype=int)
        if not (np.isfinite(a).all() and (a >= 0.0).all()):
            status = NOT_FINITE
        elif badcols.size:
            status, column = NOT_FINITE, int(badcols[0])
        elif not W > 0.0:
            status = NO_WEIGHT
        elif a.size < 2:
            status = FEW_ROWS
        out = _nan_block(d, npr, G, a.size, status, column)
        if bounds is not None:
            for k in BOUND_KEYS:
                out[k] = np.full(d, np.nan)
        if status != OK:
            return out
        if bounds is not None:
            out["bound_lo"], out["bound_hi"] = L.copy(), U.copy()
        A2 = float(np.sum(a * a))
        out["W"], out["A2"] = W, A2
        ess = W * W / A2
        mean = np.sum(a[:, None] * x, axis=0) / W
        dev = x - mean[None, :]
        var = np.sum(a[:, None] * (dev * dev), axis=0) / W
        sd = np.sqrt(var)
        h = (scale * sd) * np.float64(4.0 / (3.0 * ess)) ** 0.2
        c = 1.0 / ((2.0 * h) * h)
        mn, mx = x.min(axis=0), x.max(axis=0)
        lo = mn - 3.0 * h
        if bounds is None:
            step = ((mx + 3.0 * h) - lo) / float(G - 1)
        else:                                          # step 3': the column's own grid has to be one; then the ends move onto the bounds
            hi = mx + 3.0 * h
            base = _col_ok(sd, h, c, (hi - lo) / float(G - 1))
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
            good = _col_ok(sd, h, c, step)
            out["col_status"] = np.where(good, float(OK), float(COLUMN_BAD))
        else:
            good = base & ~outside & np.isfinite(step) & (step > 0.0)
            out["col_status"] = np.where(base, np.where(outside, float(COLUMN_OUTSIDE), np.where(good, float(OK), float(COLUMN_BAD))), float(COLUMN_BAD))
        rows_at_a_time = max(1, CHUNK_BYTES // (8 * G))
        for j in range(d):
            if not good[j]:
                out["pieces"][:, j] = -1.0
                continue
            for k, v in (("mean", mean), ("var", var), ("sd", sd), ("h", h), ("c", c), ("lo", lo), ("step", step)):
                out[k][j] = v[j]
            g = grid_points(lo[j], step[j], G)
            S, R = np.zeros(G), None if bounds is None else np.zeros(G)
            for r0 in range(0, a.size, rows_at_a_time):
                e = g[None, :] - x[r0:r0 + rows_at_a_time, j][:, None]
                arg = c[j] * (e * e)
                t = a[r0:r0 + rows_at_a_time, None] * np.where(arg >= UNDERFLOW, 0.0, np.exp(-arg))
                S += np.sum(t, axis=0)
                if R is not None:
                    R += np.sum(t * -e, axis=0)
            norm = (W * h[j]) * SQRT_2PI
            if bounds is None:
                rho, ends = S / norm, None
            else:
                out["at_lo"][j], out["at_hi"][j] = float(at_lo[j]), float(at_hi[j])
                rho = boundary_density(S / norm, (R / h[j]) / norm, *boundary_constants(g, L[j], U[j], h[j]))
                ends = (bool(at_lo[j]), bool(at_hi[j]))
            out["density"][j] = rho
            out["mode"][j], out["mode_density"][j], out["lower"][:, j], out["upper"][:, j], out["pieces"][:, j], out["edge"][:, j] = _decide(
                rho, lo[j], step[j], probs, ends)
        return out


def _from_block(block, d, npr, G, keys):
    """one system's result block with the per-column rows ``keys`` -> what ``_measure`` returns"""
    block = np.asarray(block, dtype=np.float64)
    P = len(keys)
    col = block[HEAD:HEAD + P * d].reshape(P, d)
    per = block[HEAD + P * d:HEAD + (P + PER_P * npr) * d].reshape(npr, PER_P, d)
    out = dict(W=float(block[0]), A2=float(block[1]), rows=int(block[2]), status=int(block[3]), column=int(block[4]), grid=int(G))
    for i, k in enumerate(keys):
        out[k] = col[i].copy()
    for i, k in enumerate(("lower", "upper", "pieces", "edge")):
        out[k] = per[:, i, :].copy()
    out["density"] = block[HEAD + (P + PER_P * npr) * d:].reshape(d, G).copy()
    return out


def from_block(block, d, npr, G):
    """one system's result block of ``mce_param_marginals_dev`` -> what ``measure`` returns"""
    return _from_block(block, d, npr, G, COL_KEYS)


def _host_system(a, x):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64)
    return a, (x.reshape(a.size, -1) if x.ndim != 2 else x)


def measure_native(a, x, probs, grid=DEFAULT_GRID, scale=1.0, device=None):
    """``measure`` by the library from HOST arrays (``mce_param_marginals_f64``, uploaded to ``device``)"""
    from . import _capi
    a, x = _host_system(a, x)
    blk, = _capi.param_marginals([(x, x.shape[1], a)], probs, grid, scale, device=int(device or 0))
    return from_block(blk, x.shape[1], len(probs), grid)


def build(blk, spec_, names=None):
    """``info["marginals"]`` from a block (``measure`` / ``from_block``, or their bounded forms: then with bound_lo, bound_hi, at_lo and
    at_hi) and the keyword's ``spec``; a status other than 0, or columns with one, log ONE WARNING"""
    probs, grid, scale = spec_
    d = len(blk["mean"])
    bad = [j for j in range(d) if blk["col_status"][j] in (COLUMN_BAD, COLUMN_OUTSIDE)]
    if blk["status"] != OK:
        logger.warning("marginals: status %d (%s): every value is NaN" % (blk["status"], STATUS_WORDS[blk["status"]]))
    elif bad:
        kinds = sorted(set(int(blk["col_status"][j]) for j in bad))
        logger.warning("marginals: column status %s (%s) in column%s %s: NaN there" % (
            ", ".join(str(k) for k in kinds), "; ".join(STATUS_WORDS[k] for k in kinds), "s" if len(bad) > 1 else "", ", ".join(str(j) for j in bad)))
    with np.errstate(all="ignore"):
        ess = blk["W"] * blk["W"] / blk["A2"]
    out = {"probs": tuple(probs), "grid": int(grid), "scale": float(scale), "rows": blk["rows"], "sum_w": blk["W"], "ess": ess,
           "names": list(names) if names is not None else ["p%d" % j for j in range(d)],
           "mean": blk["mean"], "sd": blk["sd"], "h": blk["h"], "c": blk["c"], "grid_lo": blk["lo"], "grid_step": blk["step"],
           "density": blk["density"], "mode": blk["mode"], "mode_density": blk["mode_density"], "lower": blk["lower"], "upper": blk["upper"],
           "pieces": blk["pieces"], "edge": blk["edge"], "col_status": blk["col_status"], "status": blk["status"], "column": blk["column"]}
    for k in BOUND_KEYS:
        if k in blk:
            out[k] = blk[k]
    return out


# ---- bounds=: hard prior bounds (csrc/param_marginals_bounds.hpp; docs/design/marginals_bounds.md) -------------------------------
COLUMN_OUTSIDE = 8
STATUS_WORDS[COLUMN_OUTSIDE] = "a sample lies outside the column's bounds"
PER_COL_BOUNDED = 14                                   # PER_COL's rows, then bound_lo, bound_hi, at_lo, at_hi
BOUND_KEYS = ("bound_lo", "bound_hi", "at_lo", "at_hi")
FAR = 40.0                                             # kMarbFar: phi and psi are 0 from here on
MAX_SLOPE = 4.0                                        # kMarbMaxSlope: the cap on f1 / f0
SQRT_2 = 1.4142135623730951
_BOUNDS_EXPECTED = "None, 'ranges', a mapping name -> (lo, hi) or a sequence of one (lo, hi) pair per parameter expected"
_erf = np.frompyfunc(math.erf, 1, 1)


def _bound_side(v, sign, whole):
    """one side of a pair: None, 'N' or an infinity: open"""
    if v is None or (isinstance(v, str) and v.strip() in ("N", "None")):
        return sign * np.inf
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("bounds=%r: %s" % (whole, _BOUNDS_EXPECTED))
    if v != v:
        raise ValueError("bounds=%r: a bound is NaN" % (whole,))
    return sign * np.inf if np.isinf(v) else v


def bounds_spec(bounds, names=None, ndim=None, root=None, marginals=True):
    """the keyword's value -> (lo[d], hi[d]) float64 arrays (-inf / +inf: that side is open), or None where it is not set.  ``names``: the
    d parameters in use (None: p0, p1, ..); ``root``: what ``"ranges"`` reads (``prior.bounds``), None on a route without a root name.
    A name the file or the mapping does not list is unbounded.  ``ValueError`` beginning ``bounds=``: lo >= hi, a NaN, a mapping's name
    that is not among the parameters in use, a sequence of another length, ``"ranges"`` without a root, ``bounds`` without
    ``marginals``"""
    if bounds is None:
        return None
    if not wanted(marginals):
        raise ValueError("bounds=%r without marginals: the bounds are those of the 1-D marginal densities" % (bounds,))
    if names is None and ndim is None:
        raise ValueError("bounds=%r: the number of parameters is not known here" % (bounds,))
    d = len(names) if names is not None else int(ndim)
    names = list(names) if names is not None else ["p%d" % j for j in range(d)]
    pairs = [(None, None)] * d
    if isinstance(bounds, str):
        if bounds != "ranges":
            raise ValueError("bounds=%r: %s" % (bounds, _BOUNDS_EXPECTED))
        if root is None:
            raise ValueError("bounds='ranges' needs a root name whose .ranges or log.param file lists the bounds: give a mapping or a sequence here")
        from . import prior
        try:
            listed = prior.bounds(root)
        except ValueError as e:
            raise ValueError("bounds='ranges': %s" % (str(e).split(": ", 1)[-1],))
        pairs = [listed.get(n, (None, None)) for n in names]
        import os
        if not os.path.isfile(str(root) + ".paramnames") and not any(n in listed for n in names):
            # (a root without .paramnames: the columns are the listed parameters that are not fixed, in the file's order)
            free = [p for p in listed.values() if p[0] < p[1]]
            pairs = [free[j] if j < len(free) else (None, None) for j in range(d)]
    elif isinstance(bounds, dict):
        unknown = [k for k in bounds if k not in names]
        if unknown:
            raise ValueError("bounds=%r: %s not among the parameters in use (%s)" % (bounds, ", ".join(repr(k) for k in unknown), ", ".join(names)))
        pairs = [bounds.get(n, (None, None)) for n in names]
    else:
        try:
            pairs = [None if p is None else tuple(p) for p in bounds]
        except TypeError:
            raise ValueError("bounds=%r: %s" % (bounds, _BOUNDS_EXPECTED))
        if len(pairs) != d:
            raise ValueError("bounds=%r: %d pairs for %d parameters" % (bounds, len(pairs), d))
    lo, hi = np.full(d, -np.inf), np.full(d, np.inf)
    for j, p in enumerate(pairs):
        if p is None:
            continue
        if len(p) != 2:
            raise ValueError("bounds=%r: %s" % (bounds, _BOUNDS_EXPECTED))
        lo[j], hi[j] = _bound_side(p[0], -1.0, bounds), _bound_side(p[1], +1.0, bounds)
        if not lo[j] < hi[j]:
            raise ValueError("bounds=%r: lo >= hi for %s (%r, %r)" % (bounds, names[j], p[0], p[1]))
    return lo, hi


def _contours_take_bounds(contours):
    """does ``contours=`` ask for boundary-corrected 2-D densities (its key ``"bounds"``)?  ``True`` there takes the call's ``bounds=``"""
    return isinstance(contours, dict) and contours.get("bounds") is not None and contours.get("bounds") is not False


def refuse_bounds(bounds, marginals, root=True, contours=None):
    """what every route refuses before any work: ``bounds`` without ``marginals`` (unless ``contours`` takes them: its ``"bounds"`` is
    True), a string other than "ranges", "ranges" on a route without a root name (``root=None``)"""
    if bounds is None:
        return
    if not wanted(marginals) and not (_contours_take_bounds(contours) and contours["bounds"] is True):
        raise ValueError("bounds=%r without marginals: the bounds are those of the 1-D marginal densities" % (bounds,))
    if isinstance(bounds, str):
        if bounds != "ranges":
            raise ValueError("bounds=%r: %s" % (bounds, _BOUNDS_EXPECTED))
        if root is None:
            raise ValueError("bounds='ranges' needs a root name whose .ranges or log.param file lists the bounds: give a mapping or a sequence here")


def note_contours(contours):
    """marginals with bounds next to contours that do not ask for the bounds themselves: ONE INFO line"""
    if contours is not None and contours is not False and not _contours_take_bounds(contours):
        logger.info("contours: the 2-D densities are not boundary-corrected; bounds= applies to the 1-D marginals alone")


def _phi(t):
    with np.errstate(all="ignore"):
        return np.where(t >= FAR, 0.0, np.exp(-((t * t) / 2.0)) / SQRT_2PI)


def _psi(t):
    with np.errstate(all="ignore"):
        return np.where(t >= FAR, 0.0, t * _phi(t))


def boundary_constants(g, L, U, h):
    """step 5' at the grid points ``g`` -> (a0, a1, a2, den)"""
    with np.errstate(all="ignore"):
        p, q = (g - L) / h, (U - g) / h
        a0 = 0.5 * (_erf(q / SQRT_2).astype(np.float64) + _erf(p / SQRT_2).astype(np.float64))
        a1 = _phi(p) - _phi(q)
        a2 = (a0 - _psi(q)) - _psi(p)
        return a0, a1, a2, a0 * a2 - a1 * a1


def boundary_density(T0, T1, a0, a1, a2, den):
    """step 6': Jones' linear boundary kernel in its positive form"""
    with np.errstate(all="ignore"):
        f0 = T0 / a0
        f1 = (a2 * T0 - a1 * T1) / den
        pos = f0 > 0.0
        slope = np.minimum(np.where(pos, f1 / np.where(pos, f0, 1.0), 0.0), MAX_SLOPE)
        rho = np.where(pos, f0 * np.exp(slope - 1.0), 0.0)
        return np.where(pos & ~(np.isfinite(den) & (den > 0.0)), f0, rho)


def hpd_selection_bounded(rho, probs, at_lo, at_hi):
    """step 8' on one column's densities -> (order, [the mask of the selected grid points of every p]): ``hpd_selection`` with half a
    cell where the grid ends on a bound"""
    return _hpd_selection(rho, probs, (at_lo, at_hi))


def decide_bounded(rho, lo, step, probs, at_lo, at_hi):
    """steps 7' and 8' on one column's densities -> what ``decide`` returns"""
    return _decide(rho, lo, step, probs, (at_lo, at_hi))


def measure_bounded(a, x, bounds, probs, grid=DEFAULT_GRID, scale=1.0, at=None):
    """The rule with bounds on host arrays: ``measure``'s arguments and ``bounds`` = (lo[d], hi[d]) (``bounds_spec``) -> ``measure``'s
    dict with bound_lo, bound_hi, at_lo, at_hi [d] (at_lo / at_hi: 1 where the grid ends on the bound).  col_status 8: a used value
    outside its bounds.  ``at``: another route's block, whose reported h, c, lo and step are taken, as in ``measure``"""
    return _measure(a, x, probs, grid, scale, at, bounds=bounds)


def from_block_bounded(block, d, npr, G):
    """one system's result block of ``mce_param_marginals_bounded_dev`` -> what ``measure_bounded`` returns"""
    return _from_block(block, d, npr, G, COL_KEYS + BOUND_KEYS)


def measure_bounded_native(a, x, bounds, probs, grid=DEFAULT_GRID, scale=1.0, device=None):
    """``measure_bounded`` by the library from HOST arrays (``mce_param_marginals_bounded_f64``, uploaded to ``device``)"""
    from . import _capi
    a, x = _host_system(a, x)
    blk, = _capi.param_marginals_bounded([(x, x.shape[1], a)], [bounds], probs, grid, scale, device=int(device or 0))
    return from_block_bounded(blk, x.shape[1], len(probs), grid)


def lines(m):
    """the lines logged and printed after the summary lines and before the ln(B) lines: one header, then per parameter: name mode
    [lower upper pieces per p] h"""
    head = " marginals: {:<12s} {:>14s}".format("parameter", "mode")
    for p in m["probs"]:
        head += " {:>14s} {:>14s} {:>3s}".format("lower%g" % (100 * p), "upper%g" % (100 * p), "pcs")
    out = [head + " {:>14s}".format("h")]
    for j, name in enumerate(m["names"]):
        ln = " marginals: {:<12s} {:>14.8g}".format(name, m["mode"][j])
        for k in range(len(m["probs"])):
            pcs = m["pieces"][k][j]
            ln += " {:>14.8g} {:>14.8g} {:>3s}".format(m["lower"][k][j], m["upper"][k][j], "nan" if pcs != pcs else "%d" % pcs)
        out.append(ln + " {:>14.8g}".format(m["h"][j]))
    return out


def save(path, roots, infos):
    """``--marginals-out``: one ``.npz`` with, per root r, names_r, grid_r [d][G] (the grid points) and density_r [d][G]; ``roots`` the
    list of their names"""
    arrays = {"roots": np.array([str(r) for r in roots])}
    for r, inf in enumerate(infos):
        m = (inf or {}).get("marginals")
        if not m:
            continue
        G = m["grid"]
        arrays["names_%d" % r] = np.array(m["names"])
        arrays["grid_%d" % r] = np.stack([grid_points(lo, st, G) for lo, st in zip(m["grid_lo"], m["grid_step"])]) if len(m["names"]) else np.zeros((0, G))
        arrays["density_%d" % r] = np.asarray(m["density"])
        for k in ("bound_lo", "bound_hi", "at_lo", "at_hi"):   # (with bounds= alone)
            if k in m:
                arrays["%s_%d" % (k, r)] = np.asarray(m[k])
    np.savez(path, **arrays)
