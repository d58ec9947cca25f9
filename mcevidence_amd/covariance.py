"""``covariance=``: the weighted mean and covariance matrix of the parameters, next to ln E -- what the tension statistics between data
sets (tension.py) need beside the evidence-side numbers.

The rule (csrc/param_cov.hpp; docs/design/tension.md) takes the s1 partition the estimator sums over: a_i the weights, x_ij the RAW
(unwhitened) values of the first ``ndim`` parameter columns.  A row with a_i == 0 is skipped entirely.  In fp64, every sum in an order
the sizes alone fix:

    W = sum a,  A2 = sum a^2,  ess = W^2 / A2,  rows = the used count
    m_j = sum a x_j / W
    C_ij = sum a (x_i - m_i)(x_j - m_j) / W  for i <= j   (the second pass about the computed m);  C_ji = C_ij is one stored value
    sd_j = sqrt(C_jj),  corr_ij = C_ij / (sd_i sd_j)   (NaN where an sd is 0; corr_jj is exactly 1 where sd_j > 0)

The normalisation is ``summary``'s (/ W, no n - 1).  status 3: a weight that is negative or not finite (column -1), a used row with a
value that is not finite (column: the lowest such); 5: W is not > 0.  A status other than 0 makes every value NaN, logs one WARNING and
raises nothing.  ``measure`` is the rule in NumPy, ``from_block`` takes the device's result block (``_capi.param_cov_dev``), ``build``
makes ``info["covariance"]`` from either.
"""
from __future__ import annotations

import logging

import numpy as np

from .summary import param_names

logger = logging.getLogger("mcevidence_amd")

__all__ = ["wanted", "spec", "refuse", "measure", "from_block", "build", "unpack", "param_names", "STATUS_WORDS"]

OK, NOT_FINITE, NO_WEIGHT = 0, 3, 5
COLUMN_NONE = -1
STATUS_WORDS = {
    OK: "ok",
    NOT_FINITE: "a weight is negative or not finite, or a row with a weight has a parameter value that is not finite",
    NO_WEIGHT: "the weights do not sum to a positive number",
}
HEAD = 8                                               # MCE_COV_HEAD: W, A2, rows used, status, column, reserved x 3


def wanted(covariance):
    """is the keyword set?  (None / False: nothing changes)"""
    return covariance is not None and covariance is not False


def spec(covariance):
    """the keyword's value -> True, or None where it is not set; anything else: ``ValueError``"""
    if not wanted(covariance):
        return None
    if covariance is True:
        return True
    raise ValueError("covariance=%r: None or True expected" % (covariance,))


def refuse(covariance, brange=None, nbatch=1, isfunc=None):
    """the combinations every route refuses (and the values ``spec`` refuses)"""
    if spec(covariance) is None:
        return
    if brange is not None or nbatch > 1:
        raise ValueError("covariance with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (brange, nbatch))
    if isfunc:
        raise ValueError("covariance with isfunc is not supported: importance sampling changes the weights and leaves the likelihood column unchanged")


def _nan_block(d, rows, status, column):
    nan = float("nan")
    return dict(W=nan, A2=nan, rows=int(rows), status=int(status), column=int(column), mean=np.full(d, nan), cov=np.full((d, d), nan))


def measure(a, x):
    """The rule on host arrays: weights ``a`` [n], values ``x`` [n, d] -> dict(W, A2, rows, status, column, mean[d], cov[d][d]); NaN
    values where the status is not 0.  cov is symmetric by construction: the upper triangle is computed, the lower is its copy."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(a.size, -1) if x.ndim != 2 else x
    if x.shape[0] != a.size:
        raise ValueError("covariance: %d weights, %d rows" % (a.size, x.shape[0]))
    d = x.shape[1]
    use = a != 0.0                                     # (a NaN weight is used: it is what status 3 reports)
    a, x = a[use], x[use]
    with np.errstate(all="ignore"):
        W = float(np.sum(a))
        status, column = OK, COLUMN_NONE
        badcols = np.flatnonzero(~np.isfinite(x).all(axis=0)) if a.size else np.zeros(0, dtype=int)
        if not (np.isfinite(a).all() and (a >= 0.0).all()):
            status = NOT_FINITE
        elif badcols.size:
            status, column = NOT_FINITE, int(badcols[0])
        elif not W > 0.0:
            status = NO_WEIGHT
        if status != OK:
            return _nan_block(d, a.size, status, column)
        out = _nan_block(d, a.size, OK, COLUMN_NONE)
        out["W"], out["A2"] = W, float(np.sum(a * a))
        mean = np.sum(a[:, None] * x, axis=0) / W
        y = x - mean[None, :]
        cov = np.empty((d, d))
        for i in range(d):
            left = a * y[:, i]
            cov[i, i:] = np.sum(left[:, None] * y[:, i:], axis=0) / W
            cov[i:, i] = cov[i, i:]
        out["mean"], out["cov"] = mean, cov
        return out


def unpack(tri, d):
    """the packed upper triangle (row-major, i <= j) -> the symmetric [d, d] matrix"""
    cov = np.empty((d, d))
    iu = np.triu_indices(d)
    cov[iu] = np.asarray(tri, dtype=np.float64)
    cov[(iu[1], iu[0])] = cov[iu]
    return cov


def from_block(block, d):
    """one system's result block of ``mce_param_cov_dev`` -> what ``measure`` returns"""
    block = np.asarray(block, dtype=np.float64)
    return dict(W=float(block[0]), A2=float(block[1]), rows=int(block[2]), status=int(block[3]), column=int(block[4]),
                mean=block[HEAD:HEAD + d].copy(), cov=unpack(block[HEAD + d:HEAD + d + d * (d + 1) // 2], d))


def build(blk, names=None):
    """``info["covariance"]`` from a block (``measure`` / ``from_block``); a status other than 0 logs the WARNING"""
    d = len(blk["mean"])
    if blk["status"] != OK:
        logger.warning("covariance: status %d (%s): every value is NaN" % (blk["status"], STATUS_WORDS[blk["status"]]))
    cov = np.asarray(blk["cov"])
    with np.errstate(all="ignore"):
        ess = blk["W"] * blk["W"] / blk["A2"]
        sd = np.sqrt(np.diagonal(cov)).copy()
        corr = cov / (sd[:, None] * sd[None, :])
    corr[~((sd[:, None] > 0.0) & (sd[None, :] > 0.0))] = np.nan
    corr[np.diag_indices(d)] = np.where(sd > 0.0, 1.0, np.nan)
    return {"names": list(names) if names is not None else ["p%d" % j for j in range(d)], "rows": blk["rows"], "sum_w": blk["W"], "ess": ess,
            "mean": blk["mean"], "cov": cov, "sd": sd, "corr": corr, "status": blk["status"], "column": blk["column"]}
