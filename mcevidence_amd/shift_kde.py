"""``shift="kde"``: the non-Gaussian parameter shift between two data sets (Raveri & Doux, arXiv:2105.03324) -- the posterior mass of
the parameter DIFFERENCE that lies above the density at "no difference", from a leave-one-out Gaussian kernel density estimate (KDE) on
the difference chain.  The Gaussian shift of tension.py assumes Gaussian posteriors; this one does not.

The rule (csrc/kde_shift.hpp; docs/design/shift_kde.md), all in fp64:

    difference chain   n = min(nA, nB); the longer chain is read at the rows floor(i n_long / n), the shorter at i; for s < boost the
                       offset o_s = floor(s n / boost):  x[s n + i] = xa[i'] - xb[((i + o_s) mod n)'],  w = a b; more than ``max_rows``
                       rows are thinned by the stride ceil(rows / max_rows)
    whitening          W, A2, mean m, covariance C of (x, w) (``covariance``'s rule);  L = cholesky(C),  ess = W^2 / A2,
                       h^2 = scale^2 (4 / ((d + 2) ess))^(2 / (d + 4)),  c = 1 / (2 h^2),  z_i = L^-1 (x_i - m),  z_0 = L^-1 (point - m)
    sums               (a kernel value exp(-a) with a >= 746 is +0.0: its exact value is below 0.17 * 2^-1074)
                       S_i = sum_{j != i} w_j exp(-c max(0, |z_i - z_j|^2)),  t_i = S_i / (W - w_i)   (leave-one-out: with the self term
                       a tail sample's own kernel dominates its density and p collapses at d >= 4);
                       S_0 = sum w_j K_0j,  Q_0 = sum w_j^2 K_0j^2,  t_0 = S_0 / W,  s_0 = sqrt(Q_0) / W
    masses             M(tau) = sum w_i [t_i > tau] at t_0, t_0 - s_0, t_0 + s_0;  M_eq = sum w_i [t_i == t_0]
    results            p = 1 - M(t_0) / W,  p_lo = 1 - M(t_0 - s_0) / W,  p_hi = 1 - M(t_0 + s_0) / W,  n_local = S_0^2 / Q_0,
                       ess_eff = min(Kish(w), Kish(a over the rows used), Kish(b over the rows used)),
                       sigma_p = sqrt(p (1 - p) / ess_eff + ((p_hi - p_lo) / 2)^2),
                       sigma_equiv = sigma_equivalent(max(p, 1 / ess_eff)), ``limit`` where the floor was taken

A row with w == 0 is skipped entirely.  status 3: a weight that is negative or not finite; 4: a used row with a value that is not finite
(column: the lowest such); 5: W is not > 0; 6: fewer than 2 used rows; 7: C is not positive definite.  A status other than 0 makes every
value NaN, logs one WARNING and raises nothing.  ``n_local`` counts the samples the density at the point is built from: below 10 a second
WARNING asks for a larger bandwidth or more rows, and the values stay as they are.

``measure`` is the rule in NumPy (the pair matrix in blocks of at most 64 MB), ``measure_dev`` the device's (``mce_kde_shift_dev`` for
device tensors, ``mce_kde_shift_f64`` for host arrays), ``estimate`` the whole of it, ``build`` makes the dict, ``lines`` prints it.
The estimator's own assumptions: independent data sets, and independent rows -- autocorrelated rows inflate ess.
"""
from __future__ import annotations

import logging
import math

import numpy as np

from . import covariance as _cov

logger = logging.getLogger("mcevidence_amd")

__all__ = ["difference_chain", "bandwidth", "whitening", "measure", "measure_dev", "from_block", "estimate", "build", "lines", "STATUS_WORDS", "FOOTNOTE"]

OK, BAD_WEIGHT, BAD_VALUE, NO_WEIGHT, FEW_ROWS, NOT_POSITIVE = 0, 3, 4, 5, 6, 7
STATUS_WORDS = {
    OK: "ok",
    BAD_WEIGHT: "a weight is negative or not finite",
    BAD_VALUE: "a row with a weight has a parameter value that is not finite",
    NO_WEIGHT: "the weights do not sum to a positive number",
    FEW_ROWS: "fewer than 2 rows with a weight",
    NOT_POSITIVE: "the covariance of the difference chain is not positive definite",
}
OUT = 16                                               # MCE_KDE_OUT: W, A2, rows, status, column, c, S0, Q0, M(t0), M(t0-s0), M(t0+s0), M_eq, reserved x 4
MAX_DIM = 64
MAX_ROWS = 262144
PAIR_BLOCK_BYTES = 64 << 20
N_LOCAL_MIN = 10.0
UNDERFLOW = 746.0                                      # kKdeUnderflow: a kernel value whose argument is at or above it is +0.0 by the rule
FOOTNOTE = ("  the KDE shift assumes independent data sets and independent rows: autocorrelated rows inflate ess (use --thin-corr); its band "
            "[p_lo, p_hi] is the noise of the density at no difference.")


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def difference_chain(xa, a, xb, b, boost=1, max_rows=MAX_ROWS):
    """rows ``xa`` [nA, d], ``xb`` [nB, d] and weights ``a``, ``b`` of two runs in their shared columns (NumPy arrays, or torch tensors of one
    device) -> dict(x[rows, d], w[rows], a[rows], b[rows]): the difference rows, their weights a b and the factors (for ess_eff)"""
    boost, max_rows = int(boost), int(max_rows)
    if boost < 1 or max_rows < 2:
        raise ValueError("shift kde: boost=%d, max_rows=%d: at least 1 and 2 expected" % (boost, max_rows))
    na, nb = int(a.shape[0]), int(b.shape[0])
    if xa.shape[0] != na or xb.shape[0] != nb or xa.ndim != 2 or xb.ndim != 2 or xa.shape[1] != xb.shape[1]:
        raise ValueError("shift kde: rows of %s and %s with %d and %d weights" % (tuple(xa.shape), tuple(xb.shape), na, nb))
    n = min(na, nb)
    i = np.arange(n, dtype=np.int64)
    ia = np.tile(i * na // n if n else i, boost)
    ib = np.concatenate([((i + (s * n) // boost) % n) * nb // n for s in range(boost)]) if n else i
    stride = -(-ia.size // max_rows) if ia.size > max_rows else 1
    ia, ib = ia[::stride], ib[::stride]
    if _is_tensor(xa):
        import torch
        ia, ib = torch.as_tensor(ia, device=xa.device), torch.as_tensor(ib, device=xa.device)
    fa, fb = a[ia], b[ib]
    return {"x": xa[ia] - xb[ib], "w": fa * fb, "a": fa, "b": fb}


def bandwidth(d, ess, scale=1.0):
    """h^2 = scale^2 (4 / ((d + 2) ess))^(2 / (d + 4)): Silverman's rule for whitened rows"""
    return float(scale) ** 2 * (4.0 / ((d + 2.0) * ess)) ** (2.0 / (d + 4.0))


def whitening(cov_blk, scale=1.0):
    """``covariance.measure``'s dict of the difference chain -> dict(status, column, linv, mean, ess, h, c); status 7 where the Cholesky
    factorisation fails, the covariance's own status (3 -> 3 or 4 by its column, 5) where it has one"""
    d = len(cov_blk["mean"])
    out = {"status": OK, "column": -1, "linv": None, "mean": np.asarray(cov_blk["mean"], dtype=np.float64), "ess": float("nan"), "h": float("nan"), "c": float("nan")}
    if cov_blk["status"] != OK:
        out["status"] = cov_blk["status"] if cov_blk["status"] != _cov.NOT_FINITE else (BAD_VALUE if cov_blk["column"] >= 0 else BAD_WEIGHT)
        out["column"] = cov_blk["column"]
        return out
    if cov_blk["rows"] < 2:
        out["status"] = FEW_ROWS
        return out
    try:
        L = np.linalg.cholesky(np.asarray(cov_blk["cov"], dtype=np.float64))
        linv = np.linalg.solve(L, np.eye(d))
    except np.linalg.LinAlgError:
        out["status"] = NOT_POSITIVE
        return out
    if not np.isfinite(linv).all():
        out["status"] = NOT_POSITIVE
        return out
    out["linv"] = np.tril(linv)
    out["ess"] = cov_blk["W"] * cov_blk["W"] / cov_blk["A2"]
    h2 = bandwidth(d, out["ess"], scale)
    out["h"], out["c"] = math.sqrt(h2), 1.0 / (2.0 * h2)
    return out


def _nan_block(rows, status, column, n=None):
    nan = float("nan")
    return dict(W=nan, A2=nan, rows=int(rows), status=int(status), column=int(column), c=nan, S0=nan, Q0=nan, M=np.full(3, nan), M_eq=nan,
                dens=None if n is None else np.full(n + 1, nan))


def _whiten(x, linv, mean):
    """z_k = sum_{j <= k} linv_kj (x_j - mean_j): plain products and sums in column order"""
    y = x - mean[None, :]
    z = np.zeros_like(y)
    for k in range(y.shape[1]):
        acc = np.zeros(y.shape[0])
        for j in range(k + 1):
            acc = acc + linv[k, j] * y[:, j]
        z[:, k] = acc
    return z


def _kernel(arg):
    """exp(-arg), +0.0 where arg >= UNDERFLOW (kde_shift.hpp: kKdeUnderflow)"""
    return np.where(arg >= UNDERFLOW, 0.0, np.exp(-arg))


def measure(x, w, linv, mean, point, c, want_dens=True):
    """The rule on host arrays -> dict(W, A2, rows, status, column, c, S0, Q0, M[3], M_eq, dens[n + 1] (t_i, NaN for a row that is not
    used, t_0 last), z[n, d]); NaN values where the status is not 0"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(w.size, -1) if x.ndim != 2 else x
    if x.shape[0] != w.size:
        raise ValueError("shift kde: %d weights, %d rows" % (w.size, x.shape[0]))
    n, d = x.shape
    linv, mean, point = np.asarray(linv, dtype=np.float64).reshape(d, d), np.asarray(mean, dtype=np.float64).reshape(d), np.asarray(point, dtype=np.float64).reshape(d)
    use = w != 0.0                                     # (a NaN weight is used: it is what status 3 reports)
    a, xu = w[use], x[use]
    with np.errstate(all="ignore"):
        W = float(np.sum(a))
        status, column = OK, -1
        badcols = np.flatnonzero(~np.isfinite(xu).all(axis=0)) if a.size else np.zeros(0, dtype=int)
        if not (np.isfinite(a).all() and (a >= 0.0).all()):
            status = BAD_WEIGHT
        elif badcols.size:
            status, column = BAD_VALUE, int(badcols[0])
        elif not W > 0.0:
            status = NO_WEIGHT
        elif a.size < 2:
            status = FEW_ROWS
        if status != OK:
            return _nan_block(a.size, status, column, n)
        z = _whiten(xu, linv, mean)
        z0 = _whiten(point[None, :], linv, mean)[0]
        zn = np.sum(z * z, axis=1)
        K0 = a * _kernel(c * np.sum((z - z0[None, :]) ** 2, axis=1))
        S0, Q0 = float(np.sum(K0)), float(np.sum(K0 * K0))
        m = a.size
        S = np.empty(m)
        step = max(1, PAIR_BLOCK_BYTES // (8 * m))
        for i0 in range(0, m, step):
            i1 = min(m, i0 + step)
            D = (zn[i0:i1, None] + zn[None, :]) - 2.0 * (z[i0:i1] @ z.T)
            K = _kernel(c * np.maximum(D, 0.0))
            K[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0        # leave one out
            S[i0:i1] = K @ a
        t = S / (W - a)
        t0, s0 = S0 / W, math.sqrt(Q0) / W
        M = np.array([np.sum(a[t > tau]) for tau in (t0, t0 - s0, t0 + s0)])
        dens = np.full(n + 1, np.nan)
        dens[:n][use] = t
        dens[n] = t0
        zfull = np.zeros((n, d))
        zfull[use] = z
    return dict(W=W, A2=float(np.sum(a * a)), rows=int(a.size), status=OK, column=-1, c=float(c), S0=S0, Q0=Q0, M=M, M_eq=float(np.sum(a[t == t0])),
                dens=dens if want_dens else None, z=zfull)


def from_block(block, dens=None):
    """one system's result block of ``mce_kde_shift_dev`` -> what ``measure`` returns (without z)"""
    b = np.asarray(block, dtype=np.float64)
    return dict(W=float(b[0]), A2=float(b[1]), rows=int(b[2]), status=int(b[3]), column=int(b[4]), c=float(b[5]), S0=float(b[6]), Q0=float(b[7]),
                M=b[8:11].copy(), M_eq=float(b[11]), dens=dens)


def measure_dev(x, w, linv, mean, point, c, device=None, want_dens=False):
    """The device's form of ``measure``: ``x`` [n, d] and ``w`` [n] as torch tensors of one device (``mce_kde_shift_dev`` on the current
    stream) or as host arrays (``mce_kde_shift_f64``, uploaded by the library to ``device``)"""
    from . import _capi
    if not _is_tensor(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        blk, dens, _ = _capi.kde_shift([(x, x.shape[1], w, linv, mean, point, c)], device=int(device or 0), want_dens=want_dens)[0]
        return from_block(blk, dens)
    import torch
    x, w = x.contiguous(), w.contiguous()
    n, d = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(x.device):
        wsb = _capi.kde_shift_workspace_bytes(n, 1, d)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
        dens = torch.empty(n + 1, dtype=torch.float64, device=x.device) if want_dens else None
        blk = _capi.kde_shift_dev([(x.data_ptr() if n else 0, d, n, d, w.data_ptr() if n else 0, linv, mean, point, c, dens.data_ptr() if want_dens else 0, 0)],
                                  ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)[0]
    return from_block(blk, dens.cpu().numpy() if want_dens else None)


def _kish(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.sum(v)) ** 2 / float(np.sum(v * v))


def build(blk, white, chain, boost=1, scale=1.0, names=None):
    """``t["shift_kde"]`` from a block (``measure`` / ``from_block``), the whitening and the difference chain's weights (host arrays)"""
    from .tension import sigma_equivalent
    nan = float("nan")
    d = len(white["mean"])
    status = white["status"] if white["status"] != OK else blk["status"]
    column = white["column"] if white["status"] != OK else blk["column"]
    out = {"names": list(names) if names is not None else ["p%d" % j for j in range(d)], "p": nan, "p_lo": nan, "p_hi": nan, "sigma_p": nan,
           "sigma_equiv": nan, "limit": False, "n_local": nan, "ess_eff": nan, "ess": nan, "rows": int(blk["rows"]), "h": nan, "t0": nan,
           "bandwidth_scale": float(scale), "boost": int(boost), "dof": d, "status": int(status), "column": int(column)}
    if status != OK:
        logger.warning("shift kde: status %d (%s): every value is NaN" % (status, STATUS_WORDS[status]))
        return out
    W = blk["W"]
    use = np.asarray(chain["w"]) != 0.0
    out["p"], out["p_lo"], out["p_hi"] = (1.0 - float(m) / W for m in blk["M"])
    out["n_local"] = blk["S0"] * blk["S0"] / blk["Q0"] if blk["Q0"] > 0.0 else 0.0
    out["ess"] = W * W / blk["A2"]
    out["ess_eff"] = min(_kish(np.asarray(chain["w"])[use]), _kish(np.asarray(chain["a"])[use]), _kish(np.asarray(chain["b"])[use]))
    out["sigma_p"] = math.sqrt(max(out["p"] * (1.0 - out["p"]), 0.0) / out["ess_eff"] + (0.5 * (out["p_hi"] - out["p_lo"])) ** 2)
    floor = 1.0 / out["ess_eff"]
    out["limit"] = bool(out["p"] < floor)
    out["sigma_equiv"] = sigma_equivalent(max(out["p"], floor))
    out["h"], out["t0"] = white["h"], blk["S0"] / W
    if out["n_local"] < N_LOCAL_MIN:
        logger.warning("shift kde: n_local = %.3g < %g: raise bandwidth_scale or the number of rows" % (out["n_local"], N_LOCAL_MIN))
    return out


def estimate(xa, a, xb, b, boost=1, bandwidth_scale=1.0, max_rows=MAX_ROWS, device=None, names=None, native=True, point=None, want_dens=False):
    """The whole rule for two runs' rows in their shared columns.  ``native``: the covariance and the sums by the library (device tensors:
    ``mce_param_cov_dev`` and ``mce_kde_shift_dev`` where they are; host arrays: the host-pointer twins on ``device``); otherwise by
    ``covariance.measure`` and ``measure`` in NumPy.  -> ``build``'s dict (with ``dens`` under ``want_dens``)"""
    if not float(bandwidth_scale) > 0.0 or not math.isfinite(float(bandwidth_scale)):
        raise ValueError("shift kde: bandwidth_scale=%r: a positive number expected" % (bandwidth_scale,))
    ch = difference_chain(xa, a, xb, b, boost, max_rows)
    x, w = ch["x"], ch["w"]
    n, d = int(x.shape[0]), int(x.shape[1])
    if not 1 <= d <= MAX_DIM:
        raise ValueError("shift kde: %d shared parameters (1 .. %d expected)" % (d, MAX_DIM))
    tensor = _is_tensor(x)
    if tensor and not native:
        x, w, ch = x.cpu().numpy(), w.cpu().numpy(), {k: v.cpu().numpy() for k, v in ch.items()}
        tensor = False
    if not native:
        cov = _cov.measure(w, x)
    elif tensor:
        import torch
        from .posterior import COVARIANCE, Request, System
        x, w = x.contiguous(), w.contiguous()
        with torch.cuda.device(x.device):
            cov = COVARIANCE.measure_dev([System(x.data_ptr() if n else 0, d, n, d, w.data_ptr() if n else 0, 0)], [Request(True, None)], x.device.index,
                                         torch.cuda.current_stream().cuda_stream)[0]
    else:
        from . import _capi
        x, w = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
        cov = _cov.from_block(_capi.param_cov([(x, d, w)], device=int(device or 0))[0], d)
    white = whitening(cov, bandwidth_scale)
    host = {k: (v.cpu().numpy() if _is_tensor(v) else np.asarray(v)) for k, v in ch.items() if k != "x"}
    if white["status"] != OK:
        blk = _nan_block(cov["rows"], white["status"], white["column"], n if want_dens else None)
    else:
        pt = np.zeros(d) if point is None else np.asarray(point, dtype=np.float64)
        if native:
            blk = measure_dev(x, w, white["linv"], white["mean"], pt, white["c"], device=device, want_dens=want_dens)
        else:
            blk = measure(x, w, white["linv"], white["mean"], pt, white["c"], want_dens=want_dens)
    out = build(blk, white, host, boost=boost, scale=bandwidth_scale, names=names)
    if want_dens:
        out["dens"] = blk["dens"]
    return out


def lines(s):
    """the line printed after the Gaussian shift"""
    return ["   shift kde ({}): p = {} [{}, {}]   sigma = {}{}   n_local = {}  rows = {}  h = {}".format(
        ", ".join(s["names"]), s["p"], s["p_lo"], s["p_hi"], ">= " if s["limit"] else "", s["sigma_equiv"], s["n_local"], s["rows"], s["h"])]
