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
"""
from __future__ import annotations

import logging

import numpy as np

from . import summary as _summary

logger = logging.getLogger("mcevidence_amd")

__all__ = ["wanted", "spec", "refuse", "measure", "measure_native", "decide", "hpd_selection", "grid_points", "from_block", "build", "lines", "save", "STATUS_WORDS", "DEFAULT_PROBS",
           "MAX_PROBS", "GRIDS", "DEFAULT_GRID", "UNDERFLOW"]

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
PER_COL = 10                                           # mean, var, sd, h, c, lo, step, mode, mode_density, col_status
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
    for k in ("mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density", "col_status"):
        blk[k] = col.copy()
    for k in ("lower", "upper", "pieces", "edge"):
        blk[k] = np.full((npr, d), nan)
    blk["density"] = np.full((d, G), nan)
    return blk


def grid_points(lo, step, G):
    """g_k = lo + k * step: a product and a sum, two roundings"""
    return lo + np.arange(G, dtype=np.float64) * step


def hpd_selection(rho, probs):
    """step 6 on one column's densities -> (order, [the mask of the selected grid points of every p])"""
    rho = np.asarray(rho, dtype=np.float64)
    G = rho.size
    order = np.lexsort((np.arange(G), -rho))           # rho descending, then k ascending
    cum = np.cumsum(rho[order])                        # (serial, in that order)
    masks = []
    for p in probs:
        cut = min(int(np.searchsorted(cum, p * cum[-1], side="left")), G - 1)
        sel = np.zeros(G, dtype=bool)
        sel[order[:cut + 1]] = True
        masks.append(sel)
    return order, masks


def decide(rho, lo, step, probs):
    """steps 5 and 6 on one column's densities -> (mode, mode_density, lower[np], upper[np], pieces[np], edge[np])"""
    rho = np.asarray(rho, dtype=np.float64)
    G = rho.size
    order, masks = hpd_selection(rho, probs)
    g = grid_points(lo, step, G)
    lower, upper, pieces, edge = [], [], [], []
    for sel in masks:
        at = np.flatnonzero(sel)
        lower.append(g[at[0]])
        upper.append(g[at[-1]])
        pieces.append(float(np.count_nonzero(sel & ~np.concatenate(([False], sel[:-1])))))
        edge.append(1.0 if sel[0] or sel[-1] else 0.0)
    return g[order[0]], rho[order[0]], np.array(lower), np.array(upper), np.array(pieces), np.array(edge)


def measure(a, x, probs, grid=DEFAULT_GRID, scale=1.0, at=None):
    """The rule on host arrays: weights ``a`` [n], values ``x`` [n, d] -> dict(W, A2, rows, status, column, grid, mean, var, sd, h, c,
    lo, step, mode, mode_density, col_status [d], lower, upper, pieces, edge [np][d], density [d][G]); the kernel matrix is formed in
    chunks of rows.  ``at``: another route's block -- its reported h, c, lo and step are taken instead of this form's own (the densities
    are defined at the reported values, and two routes' pow may differ in the last place): what a comparison of two routes needs"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    probs = tuple(float(p) for p in probs)
    G = int(grid)
    if x.shape[0] != a.size:
        raise ValueError("marginals: %d weights, %d rows" % (a.size, x.shape[0]))
    d, npr = x.shape[1], len(probs)
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
        if status != OK:
            return out
        A2 = float(np.sum(a * a))
        out["W"], out["A2"] = W, A2
        ess = W * W / A2
        mean = np.sum(a[:, None] * x, axis=0) / W
        dev = x - mean[None, :]
        var = np.sum(a[:, None] * (dev * dev), axis=0) / W
        sd = np.sqrt(var)
        h = (scale * sd) * np.float64(4.0 / (3.0 * ess)) ** 0.2
        c = 1.0 / ((2.0 * h) * h)
        lo = x.min(axis=0) - 3.0 * h
        step = ((x.max(axis=0) + 3.0 * h) - lo) / float(G - 1)
        if at is not None:
            keep = np.asarray(at["col_status"]) == OK
            h, c, lo, step = (np.where(keep, np.asarray(at[k], dtype=np.float64), v) for k, v in (("h", h), ("c", c), ("lo", lo), ("step", step)))
        good = (sd > 0.0) & np.isfinite(h) & (h > 0.0) & np.isfinite(c) & (c > 0.0) & np.isfinite(step) & (step > 0.0)
        out["col_status"] = np.where(good, float(OK), float(COLUMN_BAD))
        rows_at_a_time = max(1, CHUNK_BYTES // (8 * G))
        for j in range(d):
            if not good[j]:
                out["pieces"][:, j] = -1.0
                continue
            for k, v in (("mean", mean), ("var", var), ("sd", sd), ("h", h), ("c", c), ("lo", lo), ("step", step)):
                out[k][j] = v[j]
            g = grid_points(lo[j], step[j], G)
            S = np.zeros(G)
            for r0 in range(0, a.size, rows_at_a_time):
                e = g[None, :] - x[r0:r0 + rows_at_a_time, j][:, None]
                arg = c[j] * (e * e)
                S += np.sum(a[r0:r0 + rows_at_a_time, None] * np.where(arg >= UNDERFLOW, 0.0, np.exp(-arg)), axis=0)
            rho = S / ((W * h[j]) * SQRT_2PI)
            out["density"][j] = rho
            out["mode"][j], out["mode_density"][j], out["lower"][:, j], out["upper"][:, j], out["pieces"][:, j], out["edge"][:, j] = decide(
                rho, lo[j], step[j], probs)
        return out


def from_block(block, d, npr, G):
    """one system's result block of ``mce_param_marginals_dev`` -> what ``measure`` returns"""
    block = np.asarray(block, dtype=np.float64)
    col = block[HEAD:HEAD + PER_COL * d].reshape(PER_COL, d)
    per = block[HEAD + PER_COL * d:HEAD + (PER_COL + PER_P * npr) * d].reshape(npr, PER_P, d)
    out = dict(W=float(block[0]), A2=float(block[1]), rows=int(block[2]), status=int(block[3]), column=int(block[4]), grid=int(G))
    for i, k in enumerate(("mean", "var", "sd", "h", "c", "lo", "step", "mode", "mode_density", "col_status")):
        out[k] = col[i].copy()
    for i, k in enumerate(("lower", "upper", "pieces", "edge")):
        out[k] = per[:, i, :].copy()
    out["density"] = block[HEAD + (PER_COL + PER_P * npr) * d:].reshape(d, G).copy()
    return out


def measure_native(a, x, probs, grid=DEFAULT_GRID, scale=1.0, device=None):
    """``measure`` by the library from HOST arrays (``mce_param_marginals_f64``, uploaded to ``device``)"""
    from . import _capi
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    blk, = _capi.param_marginals([(x, x.shape[1], a)], probs, grid, scale, device=int(device or 0))
    return from_block(blk, x.shape[1], len(probs), grid)


def build(blk, spec_, names=None):
    """``info["marginals"]`` from a block (``measure`` / ``from_block``) and the keyword's ``spec``; a status other than 0, or columns
    with one, log ONE WARNING"""
    probs, grid, scale = spec_
    d = len(blk["mean"])
    bad = [j for j in range(d) if blk["col_status"][j] == COLUMN_BAD]
    if blk["status"] != OK:
        logger.warning("marginals: status %d (%s): every value is NaN" % (blk["status"], STATUS_WORDS[blk["status"]]))
    elif bad:
        logger.warning("marginals: column status %d (%s) in column%s %s: NaN there" % (COLUMN_BAD, STATUS_WORDS[COLUMN_BAD], "s" if len(bad) > 1 else "",
                                                                                      ", ".join(str(j) for j in bad)))
    with np.errstate(all="ignore"):
        ess = blk["W"] * blk["W"] / blk["A2"]
    return {"probs": tuple(probs), "grid": int(grid), "scale": float(scale), "rows": blk["rows"], "sum_w": blk["W"], "ess": ess,
            "names": list(names) if names is not None else ["p%d" % j for j in range(d)],
            "mean": blk["mean"], "sd": blk["sd"], "h": blk["h"], "c": blk["c"], "grid_lo": blk["lo"], "grid_step": blk["step"],
            "density": blk["density"], "mode": blk["mode"], "mode_density": blk["mode_density"], "lower": blk["lower"], "upper": blk["upper"],
            "pieces": blk["pieces"], "edge": blk["edge"], "col_status": blk["col_status"], "status": blk["status"], "column": blk["column"]}


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
    np.savez(path, **arrays)
