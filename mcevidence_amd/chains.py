"""Host-side chain container: reading, burn-in, thinning, s1/s2 split.

Mirrors the interface of the reference's ``MCSamples`` / ``SamplesMIXIN``
(``/root/reference/MCEvidence.py:107-607``) -- same attribute names
(``data['s1'].samples / .weights / .loglikes / .adjusted_weights``), same column
convention (col 0 weight, col 1 -ln L, cols 2.. parameters; overridable with
``iw/ilike/itheta``), same burn-in and thinning rules -- written from scratch.
This stays on the host by design (BASELINE.json north_star).

Behaviour kept on purpose (pinned by tests/golden/host_pins.json):
  * chains passed in memory (list/tuple of arrays) IGNORE ``burnlen``/``thinlen``;
    only chains read from files are burned/thinned (reference :151 vs :606);
  * the random split uses the global NumPy RNG (``np.random.choice``), so
    ``np.random.seed(s)`` before construction reproduces the reference split;
  * integer-weight thinning can replicate rows (getdist's algorithm).
Deliberate deviations (the reference crashes by accident there): a dict of arrays
is accepted (reference: TypeError on py3), ``thinlen == 1`` is a no-op (reference:
TypeError), a bare ndarray raises TypeError with a message (reference: bare ``raise``).
"""
from __future__ import annotations

import glob
import logging
import os

import numpy as np

logger = logging.getLogger("mcevidence_amd")


def rank0_draw(draw):
    """Every random decision of the host bookkeeping (the s1/s2 split, Poisson thinning, random batches)
    comes from the process's own global NumPy RNG, as in the reference (:225, :417-445, :917).  Under
    ``torchrun`` each rank is its own process with its own unseeded RNG, and the query-sharded hot path
    (``parallel.sharded_knn_dotp``) needs every rank to hold the SAME rows: rank 0 draws, the others
    receive its result (one ``broadcast_object_list``; the other ranks' RNGs are not advanced).
    Outside a process group this is just ``draw()``."""
    from . import parallel
    if not parallel.is_distributed():
        return draw()
    import torch.distributed as dist
    group = parallel.current_group()           # the group of the evidence computation (parallel.set_group), default: world
    lead = dist.get_rank(group) == 0
    box = [draw() if lead else None]
    dist.broadcast_object_list(box, src=0 if group is None else dist.get_global_rank(group, 0), group=group)
    return box[0]


def read_chain_file(path):
    """One chain text file -> fp64 array [rows, columns]: what ``np.loadtxt(f)`` gives the reference
    (:564), read by the native multi-threaded reader (``chain_io`` / ``libmcechains.so``).
    ``MCE_CHAIN_READER=numpy`` selects NumPy's reader instead, ``MCE_CHAIN_READER=hip`` the device reader
    (``chain_io.loadtxt_device``: same array, parsed on the GPU; RuntimeError without one)."""
    mode = os.environ.get("MCE_CHAIN_READER", "native")
    if mode == "hip":
        from . import chain_io
        return chain_io.loadtxt_device(path)
    if mode == "numpy" or not _native_reader():
        return np.loadtxt(path, ndmin=2)
    from . import chain_io
    return chain_io.loadtxt(path)


_NATIVE_READER = None


def _native_reader():
    """Is libmcechains.so there?  Reading chains is host bookkeeping, not the hot path: without the native
    reader (an install that lost the library) the files are read by ``np.loadtxt`` -- the reference's own
    reader (:564), same values, ~10x slower -- with ONE warning.  (The HIP hot path has no such fallback.)"""
    global _NATIVE_READER
    if _NATIVE_READER is None:
        from . import chain_io
        _NATIVE_READER = os.path.exists(chain_io.LIB_PATH)
        if not _NATIVE_READER:
            import warnings
            warnings.warn("mcevidence_amd: %s not found (build it with `make -C mcevidence_amd/csrc`); "
                          "reading chain files with numpy.loadtxt instead" % chain_io.LIB_PATH, RuntimeWarning)
    return _NATIVE_READER


def read_chain_files(paths):
    """The chain files of one root, in order.  Small files (a Planck chain is ~3 MB: one reader thread
    each) are parsed concurrently -- the native reader runs outside the GIL."""
    paths = list(paths)
    mode = os.environ.get("MCE_CHAIN_READER", "native")
    if len(paths) < 2 or mode == "numpy" or (mode != "hip" and not _native_reader()):
        return [read_chain_file(f) for f in paths]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(len(paths), 8)) as pool:
        return list(pool.map(read_chain_file, paths))


class Partition(object):
    """One partition (s1 or s2) of the samples."""

    def __init__(self, samples=None, weights=None, loglikes=None, rows=None):
        self.samples = samples
        # the two bookkeeping columns as contiguous vectors: as strided views of the chain array every pass over
        # them (negation, max, upload) costs 3-7 ms per million rows
        self.weights = None if weights is None else np.ascontiguousarray(weights)
        self.loglikes = None if loglikes is None else np.ascontiguousarray(loglikes)
        self.ichain = rows
        # a copy that importance sampling may alter independently (reference :244-247)
        self.adjusted_weights = None if weights is None else np.array(weights, copy=True)

    def __len__(self):
        return 0 if self.samples is None else len(self.samples)


# ---------------------------------------------------------------------------
# thinning index rules
# ---------------------------------------------------------------------------
def integer_weight_thin(weights, factor):
    """Indices that keep one row per ``factor`` units of (integer) weight; rows
    heavier than ``factor`` are repeated.  Same rule as getdist's
    ``WeightedSamples.thin_indices`` which the reference adopts (:481-532).
    Returns (indices, weights[indices])."""
    w = np.asarray(weights)
    wi = w.astype(int)
    if abs(float(np.sum(wi)) - float(np.sum(w))) > 1e-4:
        raise ValueError("integer-weight thinning needs integer weights")
    if factor != int(factor):
        raise ValueError("thin factor must be an integer")
    factor = int(factor)
    n = len(wi)
    if factor >= np.max(wi):
        _, keep = np.unique(np.cumsum(wi) // factor, return_index=True)
    else:
        # unroll every row into w unit-weight copies and keep the copy that completes each
        # group of `factor` units: group m ends at unit m*factor, which lies in the first row
        # whose cumulative weight reaches it (rows heavier than `factor` are kept repeatedly).
        csum = np.cumsum(wi)
        ends = factor * np.arange(1, int(csum[-1]) // factor + 1)
        keep = np.searchsorted(csum, ends, side="left")
    return keep, wi[keep]


def max_weight_bin_thin(weights, unit):
    """Non-integer weights: cut the chain into ~N/unit equal index bins and keep the
    heaviest row of each (reference ``weighted_thin`` :447-479)."""
    w = np.asarray(weights)
    n = len(w)
    if unit == 0:
        return np.arange(n), w
    nbins = int(n * unit) if unit < 1 else int(n // unit)
    edges = np.linspace(-1, n, nbins + 1)
    which = np.digitize(np.arange(n), edges)
    # first index of the maximum inside every bin, bins in ascending order
    order = np.lexsort((np.arange(n), -w, which))
    first = np.ones(n, dtype=bool)
    first[1:] = which[order][1:] != which[order][:-1]
    keep = order[first].astype(np.intp)
    return keep, w[keep]


def poisson_thin(weights, retain_fraction):
    """0 < thinlen < 1: new weight ~ Poisson(w * fraction) drawn row by row from the
    global NumPy RNG; rows with zero draws are dropped (reference :417-445)."""
    w = np.asarray(weights) * retain_fraction
    draws = rank0_draw(lambda: np.array([float(np.random.poisson(x)) for x in w]))
    keep = np.where(draws > 0)[0]
    return keep, draws[keep]


def thin_rows(weights, nthin):
    """Dispatch of reference ``get_thin_index`` (:272-287). Returns (indices, new_weights)."""
    if nthin < 1:
        return poisson_thin(weights, nthin)
    try:
        return integer_weight_thin(weights, nthin)
    except ValueError:
        return max_weight_bin_thin(weights, nthin)


# ---------------------------------------------------------------------------
# thin_corr: thinning by the measured autocorrelation length (docs/design/chain_corr.md; csrc/chain_corr.hpp has the same rule)
# ---------------------------------------------------------------------------
CORR_MIN = 0.05
CORR_MAX_LAG = 1024
CORR_UNITS = {1: "weight", 2: "rows"}           # by rule: integer weights -> weight units, otherwise row units
CORR_OK, CORR_NO_CUT, CORR_CONSTANT, CORR_NOT_FINITE = 0, 1, 2, 3
CORR_BAD_WEIGHTS = "a weight is negative, not finite or beyond 2^53"


def thin_corr_scale(thin_corr, thinlen=0):
    """The scale ``thin_corr`` asks for -- None / False: off (returns None), True: 1.0, a number > 0: itself.  Together with a
    ``thinlen`` other than 0 it is a ValueError: the two say how to thin in different ways."""
    if thin_corr is None or thin_corr is False:
        return None
    scale = 1.0 if thin_corr is True else float(thin_corr)
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError("thin_corr must be True or a number > 0 (got %r)" % (thin_corr,))
    if thinlen:
        raise ValueError("thin_corr=%r and thinlen=%r are both set: thin by the measured length (thin_corr) or by a given one (thinlen)"
                         % (thin_corr, thinlen))
    return scale


def corr_factor(scale, length):
    """the thinning factor: max(1, ceil(scale * L))"""
    return max(1, int(np.ceil(scale * length)))


def corr_status_error(status, column, cap, min_corr):
    """the ValueError of a measurement that did not end well, in the words every route uses"""
    if status == CORR_NO_CUT:
        return ValueError("thin_corr: the autocorrelation of parameter column %d stays above corr_min=%g up to cap=%d lags; raise corr_max_lag "
                          "or burn more" % (column, min_corr, cap))
    if status == CORR_CONSTANT:
        return ValueError("thin_corr: parameter column %d is constant (its S(0) is not > 0); leave it out with ndim" % column)
    return ValueError("thin_corr: a value that is not finite in parameter column %d" % column)


def corr_info(res, scale):
    """``info["thin_corr"]`` from a measurement (``correlation_length`` / ``_capi.chain_corr_dev``); raises for a non-zero status"""
    if res["status"] != CORR_OK:
        raise corr_status_error(res["status"], res["column"], res["cap"], res.get("min_corr", CORR_MIN))
    length = float(np.max(res["per_param"]))
    return {"length": length, "per_param": [float(x) for x in res["per_param"]], "cut": [int(x) for x in res["cut"]],
            "factor": corr_factor(scale, length), "units": CORR_UNITS[res["rule"]], "cap": int(res["cap"])}


def correlation_length(parts, iw=0, itheta=2, ndim=None, min_corr=CORR_MIN, max_lag=CORR_MAX_LAG):
    """The pooled, per-parameter integrated autocorrelation length of burned chains ``parts`` (2-D arrays, not concatenated), in NumPy.

    The series of a part is each row repeated ``trunc(w)`` times (integer weights, as ``integer_weight_thin`` decides: weight units;
    rows of weight 0 vanish) or the rows themselves (row units).  Columns ``itheta .. itheta + ndim`` are measured (``ndim=None``: all):
    ``S_j(t)`` sums the products of the centred series ``t`` apart over every part (a pair never spans two parts), ``n(t)`` counts them,
    ``rho_j(t) = (S_j(t) / n(t)) / (S_j(0) / n(0))``; ``cut_j`` is the first ``t`` in ``1 .. cap = min(max_lag, longest series // 4)`` with
    ``rho_j(t) <= min_corr`` and ``L_j = 1 + 2 sum(rho_j(1 .. cut_j - 1))``.  Lags are summed up to the last cut and no further.
    Returns dict(rule 1 | 2, status, column, units, cap, per_param, cut, rho [lags summed, ndim], rho_rows, min_corr); status 0 ok,
    1 a column without a cut, 2 a constant column, 3 a value that is not finite (``corr_status_error`` words them)."""
    if not (0.0 <= min_corr < 1.0) or not (1 <= int(max_lag) <= 65536):          # (the bounds mce_chain_corr_dev sets)
        raise ValueError("thin_corr: corr_min=%r (0 <= corr_min < 1 expected), corr_max_lag=%r (1 .. 65536 expected)" % (min_corr, max_lag))
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    parts = [p for p in parts if p.shape[0] > 0]
    if not parts:
        raise ValueError("the chains array is empty")
    nparam = parts[0].shape[1] - itheta
    nd = nparam if ndim is None else min(int(ndim), nparam)
    if nd < 1:
        raise ValueError("ndim must be >= 1 (got %r)" % (ndim,))
    w = np.concatenate([p[:, iw] for p in parts])
    if not np.all((w >= 0) & (w <= 2.0 ** 53)):
        raise ValueError("thin_corr: " + CORR_BAD_WEIGHTS)
    wi = w.astype(np.int64)
    rule = 1 if abs(float(np.sum(wi)) - float(np.sum(w))) <= 1e-4 else 2          # (integer_weight_thin's own test)
    series = []
    for p in parts:
        y = p[:, itheta:itheta + nd]
        if rule == 1:
            y = np.repeat(y, p[:, iw].astype(np.int64), axis=0)
        if y.shape[0]:
            lo, hi = y.min(axis=0), y.max(axis=0)
            with np.errstate(invalid="ignore"):
                m = np.where(lo == hi, lo, y.sum(axis=0) / y.shape[0])             # (a column constant over the part centres to exact zeros)
                y = y - m
        series.append(y)
    units = [y.shape[0] for y in series]
    cap = min(int(max_lag), max(units) // 4)
    out = dict(rule=rule, status=CORR_OK, column=-1, units=int(sum(units)), cap=cap, per_param=np.zeros(nd), cut=np.zeros(nd, dtype=np.int64),
               rho=np.ones((1, nd)), rho_rows=1, min_corr=float(min_corr))

    def lagged(t):
        s = np.zeros(nd)
        for y in series:
            if y.shape[0] > t:
                with np.errstate(invalid="ignore", over="ignore"):
                    s += np.einsum("ij,ij->j", y[:y.shape[0] - t], y[t:])
        return s, float(sum(max(u - t, 0) for u in units))

    s0, n0 = lagged(0)
    bad = np.nonzero(~np.isfinite(s0))[0]
    if len(bad):
        out.update(status=CORR_NOT_FINITE, column=int(bad[0]))
        return out
    flat = np.nonzero(~(s0 > 0))[0]
    if len(flat):
        out.update(status=CORR_CONSTANT, column=int(flat[0]))
        return out
    cut, acc, rows = out["cut"], np.zeros(nd), [np.ones(nd)]
    for t in range(1, cap + 1):
        s, nt = lagged(t)
        rho = (s / nt) / (s0 / n0)
        rows.append(rho)
        found = (cut == 0) & (rho <= min_corr)
        acc += np.where((cut == 0) & ~found, rho, 0.0)
        cut[found] = t
        if np.all(cut > 0):
            break
    out.update(per_param=1.0 + 2.0 * acc, rho=np.asarray(rows), rho_rows=len(rows))
    missing = np.nonzero(cut == 0)[0]
    if len(missing):
        out.update(status=CORR_NO_CUT, column=int(missing[0]))
    return out


# ---------------------------------------------------------------------------
# converge: the Gelman-Rubin R-1 of the chains (docs/design/chain_conv.md; csrc/chain_conv.hpp has the same rule)
# ---------------------------------------------------------------------------
CONV_OK, CONV_CONSTANT, CONV_NOT_FINITE, CONV_NOT_POSITIVE, CONV_FEW_SEGMENTS = 0, 2, 3, 4, 5
CONV_MAX_SEGMENTS = 128
CONV_MAX_DIM = 127
CONV_BY = ("auto", "chains", "halves")
CONV_PD_TOL = 64.0 * 2.0 ** -52                 # Wn is positive definite when its smallest eigenvalue is > CONV_PD_TOL * ndim


def converge_spec(converge, converge_by="auto"):
    """What ``converge`` / ``converge_by`` ask for -- None / False: off (returns None); True: measure only, ``(None, by)``; a number
    > 0: the threshold, ``(threshold, by)``."""
    if converge is None or converge is False:
        return None
    if converge_by not in CONV_BY:
        raise ValueError("converge_by must be one of %s (got %r)" % (", ".join(repr(b) for b in CONV_BY), converge_by))
    if converge is True:
        return None, converge_by
    threshold = float(converge)
    if not (threshold > 0.0 and np.isfinite(threshold)):
        raise ValueError("converge must be True or a threshold > 0 (got %r)" % (converge,))
    return threshold, converge_by


def conv_segments(nrows, by="auto"):
    """The segments of parts of ``nrows`` rows each -> (the ``by`` taken, [(part, first row, rows)]): ``"chains"`` one per part,
    ``"halves"`` rows ``[0, n // 2)`` and ``[n // 2, n)`` of every part, ``"auto"`` chains when at least two parts have rows, otherwise
    halves.  More than CONV_MAX_SEGMENTS segments, or fewer than two with rows, is a ValueError."""
    nrows = [int(n) for n in nrows]
    if by not in CONV_BY:
        raise ValueError("converge_by must be one of %s (got %r)" % (", ".join(repr(b) for b in CONV_BY), by))
    if by == "auto":
        by = "chains" if sum(1 for n in nrows if n > 0) >= 2 else "halves"
    if by == "chains":
        segs = [(p, 0, n) for p, n in enumerate(nrows)]
    else:
        segs = [(p, f, m) for p, n in enumerate(nrows) for f, m in ((0, n // 2), (n // 2, n - n // 2))]
    if len(segs) > CONV_MAX_SEGMENTS:
        raise ValueError("converge: %d segments (at most %d: %d chains by halves)" % (len(segs), CONV_MAX_SEGMENTS, CONV_MAX_SEGMENTS // 2))
    if sum(1 for _, _, m in segs if m > 0) < 2:
        raise conv_status_error(CONV_FEW_SEGMENTS, -1)
    return by, segs


def conv_status_error(status, column):
    """the ValueError of a measurement that did not end well, in the words every route uses"""
    if status == CONV_FEW_SEGMENTS:
        return ValueError("converge: fewer than 2 segments with rows and weight; use converge_by=\"halves\", or give more rows")
    if status == CONV_CONSTANT:
        return ValueError("converge: parameter column %d is constant within the chains (its variance is not > 0); leave it out with ndim" % column)
    if status == CONV_NOT_FINITE and column < 0:
        return ValueError("converge: a weight is negative or not finite")
    return ValueError("converge: a value that is not finite in parameter column %d" % column)


def conv_info(res, by, segments, rows, threshold=None, log=None):
    """``info["converge"]`` from one system's measurement (``r_minus_1``, ``per_param``, ``status``, ``column``, ``used``); raises for
    the statuses 2, 3 and 5; status 4 (the within-chain correlation matrix is not positive definite) and a threshold exceeded are
    logged as WARNINGs."""
    log = log or logger
    status = int(res["status"])
    if status not in (CONV_OK, CONV_NOT_POSITIVE):
        raise conv_status_error(status, int(res["column"]))
    per = [float(x) for x in res["per_param"]]
    r = float(res["r_minus_1"]) if status == CONV_OK else float("nan")
    worst = int(np.argmax(per))
    out = {"r_minus_1": r, "per_param": per, "worst_param": worst, "by": by, "segments": int(res["used"]),
           "segments_skipped": int(segments) - int(res["used"]), "rows": int(rows), "threshold": threshold, "converged": None, "status": status}
    if status == CONV_NOT_POSITIVE:
        log.warning("converge: the within-chain correlation matrix is not positive definite (fewer independent rows than parameters, or "
                    "linearly dependent columns): R-1 is not defined; the largest per-parameter value is %.4g (parameter %d)" % (per[worst], worst))
    if threshold is not None:
        out["converged"] = bool(r <= threshold)          # (NaN: False)
        if not out["converged"]:
            log.warning("converge: R-1 = %.4g exceeds the threshold %g (worst parameter %d: %.4g); the chains have not converged and ln E "
                        "is not to be trusted" % (r, threshold, worst, per[worst]))
    return out


def conv_line(c):
    """``info["converge"]`` in one line, as the command line prints it before the ln(B) lines"""
    j = c["worst_param"]
    tail = "" if c["converged"] is None else "; threshold %g: %s" % (c["threshold"], "converged" if c["converged"] else "NOT converged")
    return "R-1 = %.6g (worst parameter %d: %.6g) by %s over %d segments%s" % (c["r_minus_1"], j, c["per_param"][j], c["by"], c["segments"], tail)


def _conv_measure(segs, iw, itheta, nd):
    """the rule on one system's segments (2-D arrays) -> dict(r_minus_1, per_param, status, column, used)"""
    out = dict(r_minus_1=float("nan"), per_param=np.full(nd, np.nan), status=CONV_OK, column=-1, used=0)
    w = [s[:, iw] for s in segs]
    x = [s[:, itheta:itheta + nd] for s in segs]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        W = np.array([float(np.sum(v)) for v in w])
        use = [k for k in range(len(segs)) if len(w[k]) > 0 and W[k] > 0.0]
        out["used"] = M = len(use)
        if any(not np.all((v >= 0) & np.isfinite(v)) for v in w):
            out.update(status=CONV_NOT_FINITE, column=-1)
            return out
        bad = np.nonzero(np.any([~np.all(np.isfinite(v), axis=0) for v in x if len(v)], axis=0))[0]
        if len(bad):
            out.update(status=CONV_NOT_FINITE, column=int(bad[0]))
            return out
        if M < 2:
            out.update(status=CONV_FEW_SEGMENTS)
            return out
        c = np.sum([w[k] @ x[k] for k in range(len(segs))], axis=0) / np.sum(W)                    # step 1
        a = np.array([(w[k] @ (x[k] - c)) / W[k] for k in use])                                   # step 2
        Wu = W[use]
        o = (Wu @ a) / np.sum(Wu)                                                                 # step 3
        delta = a - o
        Wc = np.zeros((nd, nd))
        for m, k in enumerate(use):                                                               # steps 4, 5
            y = (x[k] - c) - a[m]
            Wc += ((y * w[k][:, None]).T @ y) / W[k]
        Wc /= M
        diag = np.diag(Wc).copy()
        flat = np.nonzero(~(diag > 0))[0]
        if len(flat):
            out.update(status=CONV_CONSTANT, column=int(flat[0]))
            return out
        sigma = np.sqrt(diag)                                                                     # step 6
        out["per_param"] = np.sum(delta * delta, axis=0) / (M - 1) / diag
        Wn = Wc / np.outer(sigma, sigma)                                                          # step 7
        Wn = 0.5 * (Wn + Wn.T)
        np.fill_diagonal(Wn, 1.0)
        lam, U = np.linalg.eigh(Wn)
        if not (np.all(np.isfinite(lam)) and lam[0] > CONV_PD_TOL * nd):
            out.update(status=CONV_NOT_POSITIVE, column=0)
            return out
        v = ((delta / sigma) @ U) / np.sqrt(lam)                                                  # step 8
        T = (v.T @ v) / (M - 1)
        out["r_minus_1"] = float(np.linalg.eigvalsh(T + np.eye(nd))[-1] - 1.0)
    return out


def gelman_rubin(parts, iw=0, itheta=2, ndim=None, by="auto", threshold=None):
    """The Gelman-Rubin statistic "R-1" of burned chains ``parts`` (2-D arrays, one per chain, not concatenated), in NumPy: the
    variance of the segment means over the mean of the segment variances in the worst direction of parameter space, segments counting
    equally (GetDist's ``getGelmanRubin``).  The RAW weights of column ``iw`` weigh the columns ``itheta .. itheta + ndim`` (``ndim=None``:
    all; at most 127).  ``by``: ``conv_segments``.  A segment without rows or of total weight 0 is skipped.  Returns what
    ``info["converge"]`` holds: dict(r_minus_1, per_param, worst_param, by, segments, segments_skipped, rows, threshold, converged,
    status).  A constant column, a value that is not finite, a bad weight or fewer than two segments is a ValueError
    (``conv_status_error``); a within-chain correlation matrix that is not positive definite gives ``r_minus_1 = nan``, status 4 and
    a warning."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if not parts or any(p.ndim != 2 or p.shape[1] != parts[0].shape[1] for p in parts):
        raise ValueError("chains must be 2-D arrays of one column count")
    nparam = parts[0].shape[1] - itheta
    nd = nparam if ndim is None else min(int(ndim), nparam)
    if nd < 1 or nd > CONV_MAX_DIM:
        raise ValueError("converge: ndim=%r (1 .. %d expected)" % (nd, CONV_MAX_DIM))
    by, table = conv_segments([p.shape[0] for p in parts], by)
    res = _conv_measure([parts[p][f:f + m] for p, f, m in table], iw, itheta, nd)
    return conv_info(res, by, len(table), sum(p.shape[0] for p in parts), threshold)


# ---------------------------------------------------------------------------
class MCSamples(object):
    """Container for one or more MCMC chains.

    str_or_dict : chain file root / file name / wildcard (str), or list/tuple/dict of
                  2-D arrays (one per chain).
    csplit      : object with .split/.frac/.shuffle, or None (no split).
    kwargs      : iw, ilike, itheta, log_level, burnlen, thinlen, idchain, idpattern; thin_corr (None / False: off, True: scale 1,
                  a number > 0: the scale), corr_min, corr_max_lag, ndim: files are thinned by ``ceil(scale * L)``, L their measured
                  autocorrelation length over the first ``ndim`` parameters (``correlation_length``); the result is ``thin_corr_info``.
                  converge (None / False: off, True: measure, a number > 0: a threshold), converge_by ("auto", "chains", "halves"):
                  the Gelman-Rubin R-1 of the burned, unthinned chains over the first ``ndim`` parameters (``gelman_rubin``) -- files
                  and arrays alike, a single array by halves; the result is ``converge_info``.
    """

    def __init__(self, str_or_dict, trueval=None, debug=False, csplit=None, names=None, labels=None,
                 px="x", **kwargs):
        self.debug = debug
        self.names = None
        self.labels = None
        self.trueval = trueval
        self.px = px
        self.split = bool(csplit.split) if csplit is not None else False
        self.s1frac = csplit.frac if csplit is not None else 0.5
        self.shuffle = csplit.shuffle if csplit is not None else True
        self.iw = kwargs.pop("iw", 0)
        self.ilike = kwargs.pop("ilike", 1)
        self.itheta = kwargs.pop("itheta", 2)
        kwargs.pop("log_level", None)
        self.logger = logger
        self.chains = None
        self.thin_corr_info = None
        self.converge_info = None
        self._converge = converge_spec(kwargs.pop("converge", None), kwargs.pop("converge_by", "auto"))
        self._converge_ndim = kwargs.get("ndim")

        if isinstance(str_or_dict, str):
            self.logger.info("Loading chain from " + str_or_dict)
            self.data = self.load_from_file(str_or_dict, **kwargs)
        elif isinstance(str_or_dict, (list, tuple, dict)):
            seq = list(str_or_dict.values()) if isinstance(str_or_dict, dict) else list(str_or_dict)
            if len(seq) and isinstance(seq[0], str):
                # a list of file names: read them, then treat like a file root (burn/thin honoured)
                self.data = self.load_from_file(seq, **kwargs)
            else:
                self.chains = [np.asarray(c, dtype=np.float64) for c in seq]
                self.data = self.chains2samples()          # NO kwargs: burn/thin ignored (reference :151)
        else:
            raise TypeError("first argument must be a chain file name (str) or a list/tuple/dict of 2-D "
                            "chain arrays, got %s" % type(str_or_dict).__name__)
        self.nparamMC = self.get_shape()[1]
        ndim = self.nparamMC
        self.names = ["p%s" % i for i in range(ndim)]
        self.labels = ["%s_%s" % (self.px, i) for i in range(ndim)]

    # -- reading ----------------------------------------------------------
    def load_from_file(self, fname, **kwargs):
        """CosmoMC text chains: ``root_1.txt .. root_n.txt`` (all, or ``idchain``), an
        explicit file, a list of files, or a wildcard (reference :567-606)."""
        if isinstance(fname, (list, tuple)):
            flist = list(fname)
        elif os.path.isfile(fname):
            flist = [fname]
        elif "*" in fname or "?" in fname:
            flist = sorted(glob.glob(fname))
        else:
            idchain = kwargs.pop("idchain", 0)
            if idchain > 0:
                flist = ["%s_%d.txt" % (fname, idchain)]
            else:
                pattern = kwargs.pop("idpattern", "_?.txt")
                flist = sorted(glob.glob(fname + pattern))
        kwargs.pop("idchain", None)
        kwargs.pop("idpattern", None)
        if not flist:
            raise IOError("no chain files found for %r" % (fname,))
        self.logger.debug("Reading from files: " + ", ".join(flist))
        self.chains = read_chain_files(flist)
        return self.chains2samples(**kwargs)

    # -- burn / concatenate / thin / split -----------------------------------
    def chains2samples(self, **kwargs):
        if self.chains is None or len(self.chains) == 0:
            raise ValueError("the chains array is empty")
        burnlen = kwargs.pop("burnlen", 0)
        thinlen = kwargs.pop("thinlen", 0)
        scale = thin_corr_scale(kwargs.pop("thin_corr", None), thinlen)
        self.nchains = len(self.chains)
        if burnlen > 0:
            self.chains = [self.removeBurn(burnlen, chain=c) for c in self.chains]
        if self._converge is not None:                      # the burned, unthinned chains, whatever the thinning
            self.converge_info = gelman_rubin(self.chains, self.iw, self.itheta, self._converge_ndim, self._converge[1], self._converge[0])
            self.logger.debug(conv_line(self.converge_info))
        if scale is not None:
            thinlen = self.measure_thin(scale, kwargs.pop("ndim", None), kwargs.pop("corr_min", CORR_MIN), kwargs.pop("corr_max_lag", CORR_MAX_LAG))
        self.chain_offsets = np.cumsum([0] + [c.shape[0] for c in self.chains])
        self.ichain = np.concatenate([(i + 1) * np.ones(len(c)) for i, c in enumerate(self.chains)])
        self.samples = np.concatenate(self.chains)
        self.row_chain = self.ichain.astype(np.int64) - 1          # the chain (0-based) of every surviving row: thin() keeps it in step
        if abs(thinlen) > 0:
            self.samples = self.thin(nthin=thinlen, chain=self.samples)
        self.chains = None
        return self.chain_split(self.samples)

    def removeBurn(self, remove, chain):
        """burnlen < 1 is a fraction of the chain, otherwise a row count (reference :350-391)."""
        start = int(chain.shape[0] * remove) if remove < 1 else int(remove)
        self.logger.info("Removing %s lines as burn in" % start)
        return chain[start:, :]

    def measure_thin(self, scale, ndim, corr_min, corr_max_lag):
        """thin_corr: the thinning factor from the burned chains' autocorrelation length, as a thinlen"""
        res = correlation_length(self.chains, self.iw, self.itheta, ndim, corr_min, corr_max_lag)
        self.thin_corr_info = corr_info(res, scale)
        self.logger.info("thin_corr: autocorrelation length %.3f %s units (cap %d) -> thinning factor %d"
                         % (self.thin_corr_info["length"], self.thin_corr_info["units"], res["cap"], self.thin_corr_info["factor"]))
        return float(self.thin_corr_info["factor"])

    def thin(self, nthin=1, chain=None):
        if nthin == 1:
            return chain
        if nthin < 0:
            raise ValueError("negative thinlen (autocorrelation-length thinning) is not supported")
        w = chain[:, self.iw]
        keep, neww = thin_rows(w, nthin)
        out = chain[keep, :]
        out[:, self.iw] = neww
        if getattr(self, "row_chain", None) is not None and len(self.row_chain) == len(w):
            self.row_chain = self.row_chain[keep]
        self.logger.info("Thinning with thin length=%s: #old_chain=%s, #new_chain=%s" % (nthin, len(w), len(neww)))
        return out

    def chain_split(self, s):
        """split=True: s1 = random ``int(N*s1frac)`` rows (global RNG), s2 = the rest in
        ascending row order (reference :221-249)."""
        if self.split:
            nrow = len(s)
            pick = rank0_draw(lambda: np.random.choice(range(nrow), size=int(nrow * self.s1frac), replace=False))
            rest = np.setxor1d(range(nrow), pick)
            self.logger.info("%s chain with nrow=%s split to ns1=%s, ns2=%s" % (self.nchains, nrow, len(pick), len(rest)))
            return self._partitions(s, pick, rest)
        return self._partitions(s, None, None)

    def set_split(self, s1_rows, s2_rows):
        """Use an explicit, caller-chosen split (e.g. two independent chains) instead of
        the random one; rows index the concatenated sample array."""
        self.split = True
        self.data = self._partitions(self.samples, np.asarray(s1_rows), np.asarray(s2_rows))

    def _partitions(self, s, rows1, rows2):
        def part(rows):
            a = s if rows is None else s[rows, :]
            return Partition(a[:, self.itheta:], a[:, self.iw], a[:, self.ilike],
                             range(len(s)) if rows is None else rows)
        if rows1 is None:
            return {"s1": part(None), "s2": Partition()}
        return {"s1": part(rows1), "s2": part(rows2)}

    # -- accessors ----------------------------------------------------------
    def get_shape(self, name="s1"):
        def shp(p):
            return (0, 0) if p.samples is None else p.samples.shape
        if name in ("s1", "s2"):
            return shp(self.data[name])
        a, b = shp(self.data["s1"]), shp(self.data["s2"])
        return (a[0] + b[0], a[1])

    def arrays(self, name="s1"):
        """(samples, lnp, weights) with lnp = -loglikes (reference :394-405)."""
        if name in ("s1", "s2"):
            p = self.data[name]
            if p.samples is None:
                return None, None, None
            return p.samples, -p.loglikes, p.weights
        return self.all_sample_arrays()

    def all_sample_arrays(self):
        s, lnp, w = self.arrays("s1")
        s2, lnp2, w2 = self.arrays("s2")
        if s2 is None:
            return s, lnp, w
        return np.concatenate((s, s2)), np.concatenate((lnp, lnp2)), np.concatenate((w, w2))

    def importance_sample(self, func, name="s1"):
        """adjusted_weights *= exp(-func(samples)); the original weights (used in the
        volume sum) are untouched (reference :265-270)."""
        self.data[name].adjusted_weights *= np.exp(-func(self.data[name].samples))
