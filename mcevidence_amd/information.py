"""``information=``: what lies between ln E and the fit -- <ln L>_P, D_KL(P || pi) and the Bayesian model dimensionality.

ln E = <ln L>_P - D_KL(P || pi), and d = 2 Var_P(ln L) (Handley & Lemos 2019).  Both come from the weight and the likelihood columns
every route already holds; neither needs a second neighbour search.  The rule (csrc/like_moments.hpp; docs/design/information.md)
takes the s1 partition the estimator sums over: a_i the weights, f_i = logL_i - logLmax.  A row with a_i == 0 is skipped entirely.  In
fp64, every sum in an order the sizes alone fix:

    W = sum a,  S = sum a f,  A2 = sum a^2,  c = S / W,  v = sum a (f - c)^2 / W        (the second pass about the computed c)
    mean_logL = logLmax + c,  var_logL = v,  bmd = 2 v,  ess = W^2 / A2,  D_KL[k] = mean_logL - lnE[k]

status 3: a weight that is not finite, or a used row whose f is not finite (-inf included); 5: W is not > 0.  A status other than 0
makes every value NaN, logs one WARNING and raises nothing.  ``moments`` is the rule in NumPy, ``from_block`` takes the device's result
block (``_capi.like_moments_dev``), ``build`` makes ``info["information"]`` from either, ``with_jackknife`` adds the error bars
(``with_jackknife_moments``: from the deleted sets' moments, where the columns stay on the device).

D_KL is the divergence from the FLAT prior over the given volume when the likelihood column is -ln L over that box; with priors folded
into the column, or ``ndim`` below the sampled parameters, it carries exactly the caveats ln E carries.
"""
from __future__ import annotations

import logging

import numpy as np

logger = logging.getLogger("mcevidence_amd")

__all__ = ["moments", "from_block", "from_leave_out", "build", "with_jackknife", "with_jackknife_moments", "leave_one_out", "lines", "wanted", "refuse", "STATUS_WORDS"]

OK, NOT_FINITE, NO_WEIGHT = 0, 3, 5
STATUS_WORDS = {
    OK: "ok",
    NOT_FINITE: "a weight is not finite, or a row with a weight has a likelihood that is not finite",
    NO_WEIGHT: "the weights do not sum to a positive number",
}


def wanted(information):
    """is the keyword set?  (None / False: nothing changes)"""
    return information is not None and information is not False


def refuse(information, brange=None, nbatch=1, isfunc=None):
    """the combinations every route refuses"""
    if not wanted(information):
        return
    if brange is not None or nbatch > 1:
        raise ValueError("information with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (brange, nbatch))
    if isfunc:
        raise ValueError("information with isfunc is not supported: importance sampling changes the weights and leaves the likelihood column unchanged")


def moments(a, f):
    """The rule on host arrays -> dict(W, c, v, A2, rows, status); NaN values where the status is not 0."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    if a.shape != f.shape:
        raise ValueError("information: %d weights, %d likelihoods" % (a.size, f.size))
    use = a != 0.0                                     # (a NaN weight is used: it is what status 3 reports)
    a, f = a[use], f[use]
    nan = float("nan")
    bad = not (np.isfinite(a).all() and np.isfinite(f).all())
    with np.errstate(all="ignore"):
        W = float(np.sum(a))
        status = NOT_FINITE if bad else (NO_WEIGHT if not W > 0.0 else OK)
        if status != OK:
            return dict(W=nan, c=nan, v=nan, A2=nan, rows=int(a.size), status=status)
        c = float(np.sum(a * f)) / W
        d = f - c
        v = float(np.sum(a * (d * d))) / W
        return dict(W=W, c=c, v=v, A2=float(np.sum(a * a)), rows=int(a.size), status=OK)


def from_block(block):
    """one system's result block of ``mce_like_moments_dev`` ({W, c, v, A2, rows used, status}) -> what ``moments`` returns"""
    W, c, v, A2, rows, status = (float(x) for x in block)
    return dict(W=W, c=c, v=v, A2=A2, rows=int(rows), status=int(status))


def _values(mom, logLmax, lnE):
    with np.errstate(all="ignore"):
        mean = float(logLmax) + mom["c"]
        return mean, mom["v"], 2.0 * mom["v"], mom["W"] * mom["W"] / mom["A2"], mean - np.asarray(lnE, dtype=np.float64)


def build(mom, logLmax, lnE):
    """``info["information"]`` from the moments, logLmax and the ln E columns the call returns; a status other than 0 logs the WARNING"""
    mean, var, bmd, ess, dkl = _values(mom, logLmax, lnE)
    if mom["status"] != OK:
        logger.warning("information: status %d (%s): every value is NaN" % (mom["status"], STATUS_WORDS[mom["status"]]))
    return {"mean_logL": mean, "var_logL": var, "bmd": bmd, "ess": ess, "D_KL": dkl, "rows": mom["rows"], "sum_w": mom["W"], "status": mom["status"]}


def leave_one_out(a, f, gq, G):
    """the rule applied to the rows with ``gq != b`` for every group b -> list of ``moments`` dicts"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    gq = np.asarray(gq).reshape(-1)
    out = []
    for b in range(int(G)):
        rest = gq != b
        out.append(moments(a[rest], f[rest]))
    return out


def with_jackknife(inf, a, f, gq, logLmax, jk):
    """adds sigma {mean_logL, bmd, D_KL}, groups and by to ``inf``: the delete-a-group values against ``jk["lnE_groups"]``, through
    ``jackknife.summarise``'s formula"""
    return with_jackknife_moments(inf, leave_one_out(a, f, gq, int(jk["groups"])), logLmax, jk)


def with_jackknife_moments(inf, moms, logLmax, jk):
    """``with_jackknife`` from the G deleted sets' ``moments`` dicts themselves (the resident route and the farm: the blocks of
    ``mce_jack_leave_out_dev``, the columns never on the host)"""
    from .jackknife import summarise
    G = int(jk["groups"])
    vals = [_values(m, logLmax, jk["lnE_groups"][b]) for b, m in enumerate(moms)]
    sig = lambda full, col: summarise(np.atleast_1d(full), np.array([np.atleast_1d(v[col]) for v in vals]))[0]      # noqa: E731
    inf["sigma"] = {"mean_logL": float(sig(inf["mean_logL"], 0)[0]), "bmd": float(sig(inf["bmd"], 2)[0]), "D_KL": sig(inf["D_KL"], 4)}
    inf["groups"] = G
    inf["by"] = jk["by"]
    return inf


def from_leave_out(block):
    """one slot of ``mce_jack_leave_out_dev`` ({rows, SumW, W, c, v, A2, rows used, status}) -> what ``moments`` returns"""
    return from_block(block[2:8])


def lines(inf):
    """the lines printed before the ln(B) lines: <ln L>, d, N_eff and D_KL[k=..]; with sigma they carry +- sigma"""
    sg = inf.get("sigma")
    pm = (lambda key, k=None: " ± {}".format(sg[key] if k is None else sg[key][k])) if sg else (lambda key, k=None: "")
    out = ["   <ln L> = {}{}".format(inf["mean_logL"], pm("mean_logL")),
           "   d = {}{}".format(inf["bmd"], pm("bmd")),
           "   N_eff = {}".format(inf["ess"])]
    for k in range(len(inf["D_KL"])):
        out.append("   D_KL[k={}] = {}{}".format(k + 1, inf["D_KL"][k], pm("D_KL", k)))
    return out
