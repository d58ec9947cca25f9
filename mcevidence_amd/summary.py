"""``summary=``: what the chain says about the parameters, next to ln E -- weighted posterior means and standard deviations, equal-tailed
credible limits, the median and the best-fit sample.

The rule (csrc/param_summary.hpp; docs/design/summary.md) takes the s1 partition the estimator sums over: a_i the weights, x_ij the RAW
(unwhitened) values of the first ``ndim`` parameter columns, f_i the route's fs.  A row with a_i == 0 is skipped entirely.  In fp64,
every sum in an order the sizes alone fix:

    W = sum a,  A2 = sum a^2,  ess = W^2 / A2
    m_j = sum a x_j / W,  v_j = sum a (x_j - m_j)^2 / W   (the second pass about the computed m_j),  sd_j = sqrt(v_j),  min_j, max_j
    targets: q = 0.5, and for every probability p  q_lo = (1.0 - p) / 2.0,  q_hi = (1.0 + p) / 2.0
    Q_j(q) = the smallest x among the used rows with C_j(x) >= q * W,  C_j(x) = sum of a over the used rows with x_ij <= x
    best fit: the used row with the largest f, the lowest row among equals;  bestfit_loglike = logLmax + f

No interpolation: a quantile is always a value of the chain.  status 3: a weight that is negative or not finite (column -1), a used row
whose f is NaN (column -2), a used row with a value that is not finite (column: the lowest such); 5: W is not > 0.  A status other than 0
makes every value NaN, logs one WARNING and raises nothing.  ``measure`` is the rule in NumPy, ``from_block`` takes the device's result
block (``_capi.param_summary_dev``), ``build`` makes ``info["summary"]`` from either, ``lines`` the lines that are logged and printed.
"""
from __future__ import annotations

import logging
import os

import numpy as np

logger = logging.getLogger("mcevidence_amd")

__all__ = ["wanted", "spec", "targets", "refuse", "measure", "from_block", "build", "lines", "param_names", "STATUS_WORDS", "DEFAULT_PROBS", "MAX_PROBS"]

OK, NOT_FINITE, NO_WEIGHT = 0, 3, 5
COLUMN_NONE, COLUMN_LIKE = -1, -2
STATUS_WORDS = {
    OK: "ok",
    NOT_FINITE: "a weight is negative or not finite, or a row with a weight has a likelihood that is NaN or a parameter value that is not finite",
    NO_WEIGHT: "the weights do not sum to a positive number",
}
DEFAULT_PROBS = (0.68, 0.95)
MAX_PROBS = 7
HEAD = 8                                               # MCE_SUMMARY_HEAD: W, A2, rows used, status, column, best-fit row, best-fit f, reserved
PER_COL = 5                                            # mean, var, min, max, bestfit -- then one row per target


def wanted(summary):
    """is the keyword set?  (None / False: nothing changes)"""
    return summary is not None and summary is not False


def spec(summary):
    """the keyword's value -> the tuple of probabilities, or None where it is not set; anything else: ``ValueError``"""
    if not wanted(summary):
        return None
    if summary is True:
        return DEFAULT_PROBS
    if isinstance(summary, (str, bytes, dict)):
        raise ValueError("summary=%r: None, True or up to %d probabilities 0 < p < 1 expected" % (summary, MAX_PROBS))
    try:
        probs = tuple(float(p) for p in (summary if np.ndim(summary) else (summary,)))
    except (TypeError, ValueError):
        raise ValueError("summary=%r: None, True or up to %d probabilities 0 < p < 1 expected" % (summary, MAX_PROBS))
    if not 1 <= len(probs) <= MAX_PROBS or not all(0.0 < p < 1.0 for p in probs):
        raise ValueError("summary=%r: None, True or up to %d probabilities 0 < p < 1 expected" % (summary, MAX_PROBS))
    return probs


def targets(probs):
    """the targets the quantile search is run for: 0.5, then (1 - p) / 2 and (1 + p) / 2 of every probability, as fp64 operations"""
    q = [0.5]
    for p in probs:
        q += [(1.0 - p) / 2.0, (1.0 + p) / 2.0]
    return np.array(q, dtype=np.float64)


def refuse(summary, brange=None, nbatch=1, isfunc=None):
    """the combinations every route refuses (and the values ``spec`` refuses)"""
    if spec(summary) is None:
        return
    if brange is not None or nbatch > 1:
        raise ValueError("summary with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (brange, nbatch))
    if isfunc:
        raise ValueError("summary with isfunc is not supported: importance sampling changes the weights and leaves the likelihood column unchanged")


def _nan_block(d, nq, rows, status, column):
    nan = float("nan")
    col = np.full(d, nan)
    return dict(W=nan, A2=nan, rows=int(rows), status=int(status), column=int(column), bestfit_row=-1, bestfit_f=nan, mean=col.copy(), var=col.copy(),
                min=col.copy(), max=col.copy(), bestfit=col.copy(), quant=np.full((nq, d), nan))


def measure(a, x, f, q):
    """The rule on host arrays: weights ``a`` [n], values ``x`` [n, d], ``f`` [n] or None, targets ``q`` -> dict(W, A2, rows, status,
    column, bestfit_row, bestfit_f, mean, var, min, max, bestfit, quant[len(q)][d]); NaN values where the status is not 0."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if x.shape[0] != a.size or (f is not None and np.size(f) != a.size):
        raise ValueError("summary: %d weights, %d rows, %s likelihoods" % (a.size, x.shape[0], "no" if f is None else np.size(f)))
    d, nq = x.shape[1], q.size
    use = a != 0.0                                     # (a NaN weight is used: it is what status 3 reports)
    rows_at = np.flatnonzero(use)
    a, x = a[use], x[use]
    f = None if f is None else np.asarray(f, dtype=np.float64).reshape(-1)[use]
    with np.errstate(all="ignore"):
        W = float(np.sum(a))
        status, column = OK, COLUMN_NONE
        badcols = np.flatnonzero(~np.isfinite(x).all(axis=0)) if a.size else np.zeros(0, dtype=int)
        if not (np.isfinite(a).all() and (a >= 0.0).all()):
            status = NOT_FINITE
        elif f is not None and np.isnan(f).any():
            status, column = NOT_FINITE, COLUMN_LIKE
        elif badcols.size:
            status, column = NOT_FINITE, int(badcols[0])
        elif not W > 0.0:
            status = NO_WEIGHT
        if status != OK:
            return _nan_block(d, nq, a.size, status, column)
        out = _nan_block(d, nq, a.size, OK, COLUMN_NONE)
        out["W"], out["A2"] = W, float(np.sum(a * a))
        mean = np.sum(a[:, None] * x, axis=0) / W
        dev = x - mean[None, :]
        out["mean"], out["var"] = mean, np.sum(a[:, None] * (dev * dev), axis=0) / W
        out["min"], out["max"] = x.min(axis=0) + 0.0, x.max(axis=0) + 0.0
        if f is not None:
            best = int(np.argmax(f))                   # (the first of equals: the lowest row)
            out["bestfit_row"], out["bestfit_f"], out["bestfit"] = int(rows_at[best]), float(f[best]), x[best].copy()
        want = q * W
        for j in range(d):
            order = np.argsort(x[:, j], kind="stable")
            at = np.minimum(np.searchsorted(np.cumsum(a[order]), want, side="left"), a.size - 1)
            out["quant"][:, j] = x[order[at], j] + 0.0
        return out


def from_block(block, d, nq):
    """one system's result block of ``mce_param_summary_dev`` -> what ``measure`` returns"""
    block = np.asarray(block, dtype=np.float64)
    col = block[HEAD:].reshape(PER_COL + nq, d)
    return dict(W=float(block[0]), A2=float(block[1]), rows=int(block[2]), status=int(block[3]), column=int(block[4]), bestfit_row=int(block[5]),
                bestfit_f=float(block[6]), mean=col[0].copy(), var=col[1].copy(), min=col[2].copy(), max=col[3].copy(), bestfit=col[4].copy(),
                quant=col[PER_COL:].copy())


def param_names(root, d):
    """first token of each line of ``<root>.paramnames`` where that file exists (p0, p1, .. beyond its lines and without it)"""
    names = []
    path = root + ".paramnames" if isinstance(root, str) else None
    if path and os.path.isfile(path):
        with open(path) as fh:
            names = [ln.split()[0] for ln in fh if ln.split()]
    return [names[j] if j < len(names) else "p%d" % j for j in range(d)]


def build(blk, probs, logLmax, names=None):
    """``info["summary"]`` from a block (``measure`` / ``from_block``), the probabilities and logLmax; a status other than 0 logs the
    WARNING"""
    probs = tuple(probs)
    d = len(blk["mean"])
    if blk["status"] != OK:
        logger.warning("summary: status %d (%s): every value is NaN" % (blk["status"], STATUS_WORDS[blk["status"]]))
    with np.errstate(all="ignore"):
        ess = blk["W"] * blk["W"] / blk["A2"]
        sd = np.sqrt(blk["var"])
        like = float(logLmax) + blk["bestfit_f"]
    quant = np.asarray(blk["quant"])
    return {"probs": probs, "q": targets(probs), "rows": blk["rows"], "sum_w": blk["W"], "ess": ess,
            "names": list(names) if names is not None else ["p%d" % j for j in range(d)],
            "mean": blk["mean"], "sd": sd, "var": blk["var"], "min": blk["min"], "max": blk["max"], "median": quant[0],
            "lower": quant[1::2], "upper": quant[2::2],
            "bestfit": blk["bestfit"], "bestfit_row": blk["bestfit_row"], "bestfit_loglike": like, "status": blk["status"], "column": blk["column"]}


def lines(s):
    """the lines logged and printed before the ln(B) lines: one header, then per parameter: name mean sd [lower upper per p] bestfit"""
    head = "   summary: {:<12s} {:>14s} {:>14s}".format("parameter", "mean", "sd")
    for p in s["probs"]:
        head += " {:>14s} {:>14s}".format("lower%g" % (100 * p), "upper%g" % (100 * p))
    out = [head + " {:>14s}".format("bestfit")]
    for j, name in enumerate(s["names"]):
        ln = "   summary: {:<12s} {:>14.8g} {:>14.8g}".format(name, s["mean"][j], s["sd"][j])
        for k in range(len(s["probs"])):
            ln += " {:>14.8g} {:>14.8g}".format(s["lower"][k][j], s["upper"][k][j])
        out.append(ln + " {:>14.8g}".format(s["bestfit"][j]))
    return out
