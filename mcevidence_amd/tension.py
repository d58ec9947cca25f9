"""Tension statistics between two data sets A and B under one model, from three runs: A alone, B alone and the joint run AB.

Each run gives ln E[k], ``info["information"]`` (<ln L>_P, D_KL[k], the Bayesian model dimensionality) and ``info["covariance"]`` (the
weighted mean and covariance of the parameters).  ``combine`` is host arithmetic on those (docs/design/tension.md):

    ln R[k] = ln E_AB[k] - ln E_A[k] - ln E_B[k]                      the evidence ratio: > 0 agreement, < 0 tension, prior dependent
    ln I[k] = D_KL_A[k] + D_KL_B[k] - D_KL_AB[k]                      the information ratio
    ln S    = <ln L>_AB - <ln L>_A - <ln L>_B  ( = ln R[k] - ln I[k] for every k: the prior volume cancels)   the suspiciousness
    d       = d_A + d_B - d_AB                                        the dimensionality both data sets constrain
    p       = Q(d / 2, (d - 2 ln S) / 2)                              d - 2 ln S is chi^2_d distributed for Gaussian posteriors
    sigma_equiv = -ndtri(p / 2)                                       the two-sided Gaussian equivalent of p

(Handley & Lemos 2019, arXiv:1902.04029), Q the regularised upper incomplete gamma function; p = 1 where d - 2 ln S <= 0.  Where d <= 0
the chains do not show a shared constrained direction: p and sigma_equiv are NaN, ``status`` is 1 and one WARNING is logged.  ``status``
2: a value of an input is not finite (an input's own status was not 0).

The parameter shift in the parameters both runs share:  Delta = m_A - m_B,  C = C_A[sh, sh] + C_B[sh, sh],  chi^2 = Delta^T C^-1 Delta
by Cholesky factorisation and solve, dof = len(sh), p = Q(dof / 2, chi^2 / 2).  C_A + C_B is the covariance of the difference ONLY for
independent data sets, and chi^2 is chi^2_dof distributed ONLY for Gaussian posteriors: both are assumed, neither is checked.
``shift.status`` 1: C is not positive definite (every value NaN, one WARNING); 2: a mean or covariance entry is not finite.

The Gaussian assumption of the shift can be dropped: ``parameter_shift_kde`` (``evidence_tension(shift="kde" | "both")``, shift_kde.py)
estimates the posterior mass of the parameter DIFFERENCE above the density at "no difference" by a leave-one-out kernel density estimate
on the difference chain (Raveri & Doux 2021, arXiv:2105.03324) and puts its dict into ``t["shift_kde"]``; independent data sets stay
assumed.

ln I and D_KL measure a posterior against the flat prior only.  How much one run learnt beyond ANOTHER is the relative entropy between
their posteriors: ``knn_divergence`` (``evidence_tension(gain="knn")``, divergence.py) estimates D_KL(P || Q) of two chains from
nearest-neighbour distances, with a delete-a-block jackknife error bar from one pair of searches, and ``t["gain"]`` holds the four of
them: "AB|A" and "AB|B" (the information gained by adding the other data set, over the parameters the pair of runs shares), "A|B" and
"B|A" (between the two data sets, over the parameters A and B share).  It needs no likelihood column and no prior volume.

ln R is only meaningful when the three runs share the prior on the shared parameters and each ln E carries its own full prior volume
(``priorvolume``); nothing here can check that.

With ``jackknife`` set on all three runs, ``sigma`` holds the root-sum-square of the three runs' jackknife sigmas of ln E[k], <ln L> and
d: the three chains are independent; like every jackknife sigma here it is conservative.
"""
from __future__ import annotations

import logging
import math

import numpy as np

logger = logging.getLogger("mcevidence_amd")

__all__ = ["combine", "evidence_tension", "lines", "shared_parameters", "p_value", "sigma_equivalent", "parameter_shift_kde", "knn_divergence", "GAIN_KEYS", "FOOTNOTE",
           "FOOTNOTE_KDE", "FOOTNOTE_GAIN"]

OK, NO_DIMENSION, NOT_FINITE = 0, 1, 2
SHIFT_OK, SHIFT_NOT_POSITIVE, SHIFT_NOT_FINITE = 0, 1, 2
FOOTNOTE = ("* tension: p and sigma of ln S assume Gaussian posteriors (d - 2 ln S ~ chi^2_d); the parameter shift assumes Gaussian posteriors and "
            "independent data sets (C = C_A + C_B); ln R depends on the prior volume the three runs share.")


from .shift_kde import FOOTNOTE as FOOTNOTE_KDE  # noqa: E402  (the second footnote sentence, printed where the KDE shift was asked for)

GAIN_KEYS = ("AB|A", "AB|B", "A|B", "B|A")
FOOTNOTE_GAIN = ("  gain: k-NN relative entropy D_KL(P || Q)[k] between two chains, in nats, whitened with P's covariance; \u00b1: delete-a-block jackknife, "
                 "conditional on that metric; the estimator's bias grows with the number of parameters and with k, and autocorrelated rows "
                 "shrink its error bar (use --thin-corr).")


def _gammaincc_large(a, x):
    """Q(a, x) for a > 20 by the series of P below x = a + 1 and by the continued fraction of Q (modified Lentz) above it: there
    ``torch.special.gammaincc`` switches to an asymptotic expansion that is good to 1e-9 only (Q(63.5, 75) = 0.0799419870175 against its
    0.0799419871053), this is good to 1e-12"""
    front = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        ap, term = a, 1.0 / a
        total = term
        for _ in range(100000):
            ap += 1.0
            term *= x / ap
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return 1.0 - total * front
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        step = d * c
        h *= step
        if abs(step - 1.0) < 1e-16:
            break
    return front * h


def p_value(dof, chi2):
    """Q(dof / 2, chi2 / 2) in fp64 (``torch.special.gammaincc``; above dof = 40 ``_gammaincc_large``); 1 where chi2 <= 0; NaN where dof
    is not > 0 or an argument is NaN"""
    import torch
    dof, chi2 = float(dof), float(chi2)
    if not dof > 0.0 or math.isnan(chi2):
        return float("nan")
    if chi2 <= 0.0:
        return 1.0
    # (a = dof / 2 > 20 is where torch's implementation takes its asymptotic branch)
    if dof > 40.0 and math.isfinite(dof) and math.isfinite(chi2):
        return min(max(_gammaincc_large(0.5 * dof, 0.5 * chi2), 0.0), 1.0)
    return float(torch.special.gammaincc(torch.tensor(0.5 * dof, dtype=torch.float64), torch.tensor(0.5 * chi2, dtype=torch.float64)))


def sigma_equivalent(p):
    """-ndtri(p / 2): the lower tail, so that a small p keeps its digits (``torch.special.ndtri`` in fp64)"""
    import torch
    p = float(p)
    if math.isnan(p):
        return float("nan")
    return -float(torch.special.ndtri(torch.tensor(0.5 * p, dtype=torch.float64))) + 0.0


def _default_names(names):
    return list(names) == ["p%d" % j for j in range(len(names))]


def shared_parameters(names_a, names_b, shared=None):
    """-> (names, columns in A, columns in B).  None: the names A and B have in common, in A's order -- both sides must have names from a
    ``.paramnames`` file (names other than p0, p1, ..); a count: that many leading columns of both; a list: those names on both sides"""
    names_a, names_b = list(names_a), list(names_b)
    if shared is None:
        if _default_names(names_a) or _default_names(names_b):
            raise ValueError("tension: shared= is required (names, or a count of leading columns) where a run has no .paramnames file")
        shared = [n for n in names_a if n in names_b]
    if isinstance(shared, (int, np.integer)) and not isinstance(shared, bool):
        k = int(shared)
        if not 1 <= k <= min(len(names_a), len(names_b)):
            raise ValueError("tension: shared=%d leading columns of %d and %d parameters" % (k, len(names_a), len(names_b)))
        return names_a[:k], list(range(k)), list(range(k))
    shared = [str(n) for n in shared]
    missing = [n for n in shared if n not in names_a or n not in names_b]
    if missing or not shared or len(set(shared)) != len(shared):
        raise ValueError("tension: shared=%r: %s" % (shared, "not a parameter of both runs: %r" % missing if missing else "one or more distinct names expected"))
    return shared, [names_a.index(n) for n in shared], [names_b.index(n) for n in shared]


def _shift(cov_a, cov_b, shared):
    names, ia, ib = shared_parameters(cov_a["names"], cov_b["names"], shared)
    nan = float("nan")
    delta = np.asarray(cov_a["mean"], dtype=np.float64)[ia] - np.asarray(cov_b["mean"], dtype=np.float64)[ib]
    C = np.asarray(cov_a["cov"], dtype=np.float64)[np.ix_(ia, ia)] + np.asarray(cov_b["cov"], dtype=np.float64)[np.ix_(ib, ib)]
    out = {"names": names, "delta": delta, "chi2": nan, "dof": len(names), "p": nan, "sigma_equiv": nan, "status": SHIFT_OK}
    if not (np.isfinite(delta).all() and np.isfinite(C).all()):
        out["status"] = SHIFT_NOT_FINITE
        out["delta"] = np.full(len(names), nan)
        logger.warning("tension: shift status %d (a mean or a covariance entry of a run is not finite): every value is NaN" % SHIFT_NOT_FINITE)
        return out
    try:
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        out["status"] = SHIFT_NOT_POSITIVE
        logger.warning("tension: shift status %d (C_A + C_B is not positive definite in the shared parameters): every value is NaN" % SHIFT_NOT_POSITIVE)
        return out
    z = np.linalg.solve(L, delta)                          # (L is triangular: chi^2 = |L^-1 Delta|^2)
    out["chi2"] = float(z @ z)
    out["p"] = p_value(out["dof"], out["chi2"])
    out["sigma_equiv"] = sigma_equivalent(out["p"])
    return out


def _rss(*xs):
    return np.sqrt(sum(np.asarray(x, dtype=np.float64) ** 2 for x in xs))


def parameter_shift_kde(rows_a, w_a, rows_b, w_b, boost=1, bandwidth_scale=1.0, max_rows=262144, device=None, names=None):
    """The non-Gaussian parameter shift of two runs from their rows in the SHARED columns (``rows_a`` [nA, d], ``rows_b`` [nB, d]) and
    their weights: NumPy arrays (uploaded by the library to ``device``, 0 when None) or torch tensors of one device.  The difference chain
    pairs row i of the one with row i + o_s of the other for ``boost`` offsets o_s, is thinned to at most ``max_rows`` rows and whitened by
    its own covariance; the density of every row and of "no difference" is a leave-one-out Gaussian KDE of bandwidth ``bandwidth_scale``
    times Silverman's.  -> dict(names, p, p_lo, p_hi, sigma_p, sigma_equiv, limit, n_local, ess_eff, ess, rows, h, t0, bandwidth_scale,
    boost, dof, status, column); shift_kde.py has the rule, the statuses and the assumptions (independent data sets and rows)."""
    from . import shift_kde
    return shift_kde.estimate(rows_a, w_a, rows_b, w_b, boost=boost, bandwidth_scale=bandwidth_scale, max_rows=max_rows, device=device, names=names)


def knn_divergence(rows_p, w_p, rows_q, w_q, kmax=4, groups=8, device=None, names=None):
    """The relative entropy D_KL(P || Q)[k], k = 1 .. ``kmax``, between two runs from their rows in the SHARED columns (``rows_p`` [nP, d],
    ``rows_q`` [nQ, d]) and their weights: NumPy arrays or torch tensors of one device.  Both chains are whitened with P's covariance; the
    estimate is the k-NN one of Wang, Kulkarni & Verdu (2009) with weights, its error bar a delete-a-block jackknife over ``groups`` blocks
    of each chain (0: none) from ONE pair of neighbour searches.  -> dict(names, D[k], sigma[k], D_bias_corrected[k], D_groups[G, k],
    excluded[k], rows_per_level, groups, kmax, rows_p, rows_q, dof, status, column, chain); divergence.py has the rule, the statuses and
    the assumptions (independent rows)."""
    from . import divergence
    return divergence.estimate(rows_p, w_p, rows_q, w_q, kmax=kmax, groups=groups, device=device, names=names)


def combine(a, b, ab, shared=None, shift_kde=None, gain=None):
    """``a``, ``b``, ``ab``: (lnE[kmax - 1], info) of the runs on A, on B and on both, each with ``info["information"]`` and
    ``info["covariance"]`` -> dict(lnR[k], lnI[k], lnS, d, p, sigma_equiv, shift{names, delta, chi2, dof, p, sigma_equiv, status},
    status) and, with ``info["jackknife"]`` in all three, sigma{lnR[k], lnS, d}.  The module's docstring has the definitions and the
    assumptions (Gaussian posteriors; independent data sets for the shift).  ``shift_kde``: ``parameter_shift_kde``'s dict, which goes
    into ``t["shift_kde"]`` as it is; ``gain``: the dict of ``knn_divergence``'s dicts, which goes into ``t["gain"]`` as it is."""
    runs = []
    for name, (lnE, info) in (("a", a), ("b", b), ("ab", ab)):
        if "information" not in info or "covariance" not in info:
            raise ValueError("tension: run %s has no info[%r]: run it with information=True, covariance=True" % (name, "information" if "information" not in info else "covariance"))
        runs.append((np.atleast_1d(np.asarray(lnE, dtype=np.float64)), info))
    (ea, ia), (eb, ib), (eab, iab) = runs
    if not ea.shape == eb.shape == eab.shape:
        raise ValueError("tension: ln E of %d, %d and %d columns" % (ea.size, eb.size, eab.size))
    fa, fb, fab = ia["information"], ib["information"], iab["information"]
    with np.errstate(all="ignore"):
        lnR = eab - ea - eb
        lnI = np.asarray(fa["D_KL"], dtype=np.float64) + np.asarray(fb["D_KL"], dtype=np.float64) - np.asarray(fab["D_KL"], dtype=np.float64)
        lnS = float(fab["mean_logL"]) - float(fa["mean_logL"]) - float(fb["mean_logL"])
        d = float(fa["bmd"]) + float(fb["bmd"]) - float(fab["bmd"])
    out = {"lnR": lnR, "lnI": lnI, "lnS": lnS, "d": d, "p": float("nan"), "sigma_equiv": float("nan"), "status": OK}
    if not (math.isfinite(lnS) and math.isfinite(d)):
        out["status"] = NOT_FINITE
        logger.warning("tension: status %d (<ln L> or the dimensionality of a run is not finite): p is NaN" % NOT_FINITE)
    elif not d > 0.0:
        out["status"] = NO_DIMENSION
        logger.warning("tension: status %d (d = d_A + d_B - d_AB = %g is not > 0): p is NaN" % (NO_DIMENSION, d))
    else:
        out["p"] = p_value(d, d - 2.0 * lnS)
        out["sigma_equiv"] = sigma_equivalent(out["p"])
    out["shift"] = _shift(ia["covariance"], ib["covariance"], shared)
    jks = [i.get("jackknife") for i in (ia, ib, iab)]
    sgs = [f.get("sigma") for f in (fa, fb, fab)]
    if all(j is not None for j in jks) and all(s is not None for s in sgs):
        out["sigma"] = {"lnR": _rss(*[j["sigma"] for j in jks]), "lnS": float(_rss(*[s["mean_logL"] for s in sgs])), "d": float(_rss(*[s["bmd"] for s in sgs]))}
    if shift_kde is not None:
        out["shift_kde"] = shift_kde
    if gain is not None:
        out["gain"] = gain
    return out


def lines(t):
    """the lines printed after the three roots: ln R / ln I per k, ln S, d, p and its sigma, then the shift (and the KDE shift where it was
    asked for), then the four gain lines where they were asked for; +- where the jackknife ran"""
    sg = t.get("sigma")
    pm = (lambda key, k=None: " ± {}".format(sg[key] if k is None else sg[key][k])) if sg else (lambda key, k=None: "")
    out = []
    for k in range(len(t["lnR"])):
        out.append("   ln R[k={}] = {}{}   ln I[k={}] = {}".format(k + 1, t["lnR"][k], pm("lnR", k), k + 1, t["lnI"][k]))
    out.append("   ln S = {}{}".format(t["lnS"], pm("lnS")))
    out.append("   d = {}{}".format(t["d"], pm("d")))
    out.append("   p = {}   sigma = {}".format(t["p"], t["sigma_equiv"]))
    s = t["shift"]
    out.append("   shift ({}): chi2 = {}  dof = {}  p = {}   sigma = {}".format(", ".join(s["names"]), s["chi2"], s["dof"], s["p"], s["sigma_equiv"]))
    if t.get("shift_kde") is not None:
        from . import shift_kde
        out.extend(shift_kde.lines(t["shift_kde"]))
    if t.get("gain") is not None:
        from . import divergence
        for key in GAIN_KEYS:
            p, q = key.split("|")
            out.extend(divergence.lines(t["gain"][key], label="gain D_KL({} || {})".format(p, q), ranks=False))
    return out


_FARM_ONLY = ("device", "wave_bytes", "return_exceptions", "require_resident")


def _host_rows(m):
    """(rows, weights) of the s1 partition of an ``MCEvidence`` object: what ``covariance=`` measures"""
    part = m.gd.data["s1"]
    return np.asarray(part.samples, dtype=np.float64)[:, :m.ndim], np.asarray(part.adjusted_weights, dtype=np.float64)


def _farm_rows(root, ndim, kw, i):
    """the rows and weights of root ``i`` (0: A, 1: B) read once more, on the device where the resident route takes the root, else on the
    host; the per-root keywords are the farm's"""
    from . import resident as _res
    from .farm import _per_root
    one = lambda k, default: _per_root(kw[k], 3, k)[i] if k in kw else default          # noqa: E731
    read = {k: kw[k] for k in ("idchain", "idpattern", "iw", "ilike", "itheta") if k in kw}
    corr = {}
    if one("thin_corr", None) not in (None, False):
        corr = {"thin_corr": one("thin_corr", None), **{k: kw[k] for k in ("corr_min", "corr_max_lag") if kw.get(k) is not None}}
    try:
        rc = _res.ResidentChains.from_files(root, burnlen=one("burnlen", 0), thinlen=one("thinlen", 0), device=kw.get("device", 0), ndim=one("ndim", None),
                                            **read, **corr)
        x, w = rc.rows()
        return x[:, :ndim], w
    except _res.ResidentDecline:
        from .evidence import MCEvidence
        m = MCEvidence(root, ndim=one("ndim", None), burnlen=one("burnlen", 0), thinlen=one("thinlen", 0), verbose=0, **read, **corr)
        return _host_rows(m)


def _refuse_gain(kw):
    """the combinations ``gain=`` refuses"""
    from . import parallel
    if kw.get("brange") is not None or kw.get("nbatch", 1) > 1:
        raise ValueError("gain with batched runs (brange=%r, nbatch=%r) is not supported: one batch, every sample" % (kw.get("brange"), kw.get("nbatch", 1)))
    if kw.get("isfunc"):
        raise ValueError("gain with isfunc is not supported: importance sampling changes the weights and leaves the likelihood column unchanged")
    if parallel.is_distributed():
        raise ValueError("gain under an initialised process group is not supported: run it in one process")


def _pair_shared(names_p, names_q):
    """the parameters a joint run and one of its parts share: by name where both have names, else the leading columns of the shorter"""
    if _default_names(names_p) or _default_names(names_q):
        return shared_parameters(names_p, names_q, min(len(names_p), len(names_q)))
    return shared_parameters(names_p, names_q, None)


def _gain(covs, rows, shared, gain_k, gain_groups, device):
    """``t["gain"]``: covs the three runs' info["covariance"] (A, B, AB), rows(i, nd) their rows and weights"""
    data = [rows(i, len(covs[i]["names"])) for i in range(3)]
    if len({type(x) for x, _ in data}) > 1:                    # (a root on the device, another on the host: all on the host)
        data = [tuple(v.cpu().numpy() if hasattr(v, "cpu") else v for v in xw) for xw in data]
    pairs = {"AB|A": (2, 0, _pair_shared(covs[2]["names"], covs[0]["names"])), "AB|B": (2, 1, _pair_shared(covs[2]["names"], covs[1]["names"])),
             "A|B": (0, 1, shared_parameters(covs[0]["names"], covs[1]["names"], shared))}
    pairs["B|A"] = (1, 0, (pairs["A|B"][2][0], pairs["A|B"][2][2], pairs["A|B"][2][1]))
    out = {}
    for key in GAIN_KEYS:
        p, q, (names, ip, iq) = pairs[key]
        (xp, wp), (xq, wq) = data[p], data[q]
        out[key] = knn_divergence(xp[:, ip], wp, xq[:, iq], wq, kmax=gain_k, groups=gain_groups, device=device, names=names)
    return out


def evidence_tension(root_a, root_b, root_ab, shared=None, route="farm", shift="gaussian", boost=1, bandwidth_scale=1.0, gain=None, gain_k=4,
                     gain_groups=8, **kw):
    """The three runs and their tension: ``route="farm"``: ``evidence_many_from_files([root_a, root_b, root_ab], information=True,
    covariance=True, info=True, **kw)`` (a root the farm does not cover takes its per-root route); ``route="host"``: three
    ``MCEvidence(root, information=True, covariance=True, **kw).evidence(info=True)``.  ``kw``: the farm's keywords (``kmax``, ``ndim``,
    ``priorvolume``, ``burnlen``, ``thinlen``, ``thin_corr``, ``jackknife``, ..; the four of them that may be sequences have one entry per
    root, in the order A, B, AB; ``marginals`` with ``bounds`` go to all three roots, ``bounds="ranges"`` reading every root's own file; so does the key ``"bounds"`` of ``contours``).  Returns (lnE_a, lnE_b, lnE_ab, info): ``info["tension"]`` is ``combine``'s dict, ``info["roots"]`` the
    three runs' info dicts, ``info["route"]`` the route asked for.  The assumptions are ``combine``'s.  ``shift``: "gaussian" (the dict and
    the lines as they are without the keyword), "kde" or "both": ``parameter_shift_kde`` with ``boost`` and ``bandwidth_scale`` on the rows
    and weights ``covariance=`` measured in A and B, in ``info["tension"]["shift_kde"]`` -- the Gaussian shift stays in either case.  The
    host route uses its three objects' rows (``mce_kde_shift_f64``); the farm route reads A and B once more after the farm pass
    (``ResidentChains.from_files(...).rows()``, the sums by ``mce_kde_shift_dev``; a root the resident plan declines: its host rows).
    ``gain``: None (the dict and the lines as they are without the keyword) or "knn": ``knn_divergence`` with ``gain_k`` ranks and
    ``gain_groups`` jackknife blocks for the four pairs of ``GAIN_KEYS``, in ``info["tension"]["gain"]``; it takes its rows exactly where
    ``shift="kde"`` takes them, for AB too."""
    if route not in ("farm", "host"):
        raise ValueError("tension: route=%r: 'farm' or 'host' expected" % (route,))
    if shift not in ("gaussian", "kde", "both"):
        raise ValueError("tension: shift=%r: 'gaussian', 'kde' or 'both' expected" % (shift,))
    if gain not in (None, "knn"):
        raise ValueError("tension: gain=%r: None or 'knn' expected" % (gain,))
    if gain is not None:
        _refuse_gain(kw)
    roots = [root_a, root_b, root_ab]
    for k in ("information", "covariance", "info"):
        if k in kw:
            raise ValueError("tension: %s is set by evidence_tension" % k)
    if route == "farm":
        from .farm import evidence_many_from_files
        outs = evidence_many_from_files(roots, information=True, covariance=True, info=True, **kw)
        rows = (lambda i, nd: _farm_rows(roots[i], nd, kw, i)) if shift != "gaussian" or gain is not None else None
    else:
        from .evidence import MCEvidence
        from .farm import _per_root
        kw = {k: v for k, v in kw.items() if k not in _FARM_ONLY}
        call = {k: kw.pop(k) for k in ("pos_lnp",) if k in kw}
        if kw.get("covtype", "all") != "all":
            call["covtype"] = kw["covtype"]
        if kw.get("thin_corr", None) in (None, False):
            for k in ("thin_corr", "corr_min", "corr_max_lag"):
                kw.pop(k, None)
        if kw.get("converge", None) in (None, False):
            for k in ("converge", "converge_by"):
                kw.pop(k, None)
        per = {k: _per_root(kw.pop(k), 3, k) for k in ("ndim", "priorvolume", "burnlen", "thinlen") if k in kw}
        kw.setdefault("verbose", 0)
        outs, ms = [], []
        for i, r in enumerate(roots):
            m = MCEvidence(r, information=True, covariance=True, **{k: v[i] for k, v in per.items()}, **kw)
            outs.append(m.evidence(info=True, **call))
            if (shift != "gaussian" and i < 2) or gain is not None:          # (kept for their rows; otherwise one object at a time, as before)
                ms.append(m)
            del m
        rows = lambda i, nd: _host_rows(ms[i])                                     # noqa: E731
    kde = None
    if shift != "gaussian":
        ca, cb = outs[0][1]["covariance"], outs[1][1]["covariance"]
        names, ia, ib = shared_parameters(ca["names"], cb["names"], shared)
        (xa, wa), (xb, wb) = rows(0, len(ca["names"])), rows(1, len(cb["names"]))
        if type(xa) is not type(xb):                            # (one root on the device, one on the host: both on the host)
            xa, wa, xb, wb = [v.cpu().numpy() if hasattr(v, "cpu") else v for v in (xa, wa, xb, wb)]
        kde = parameter_shift_kde(xa[:, ia], wa, xb[:, ib], wb, boost=boost, bandwidth_scale=bandwidth_scale, device=kw.get("device", None), names=names)
    gains = None
    if gain is not None:
        gains = _gain([o[1]["covariance"] for o in outs], rows, shared, gain_k, gain_groups, kw.get("device", None))
    t = combine(outs[0], outs[1], outs[2], shared=shared, shift_kde=kde, gain=gains)
    return outs[0][0], outs[1][0], outs[2][0], {"tension": t, "roots": [o[1] for o in outs], "route": route}
