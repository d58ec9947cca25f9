"""The statistics reported next to ln E -- information, summary, marginals, contours, covariance -- as ONE table the routes loop over.

Each statistic has a module of its own (information.py, summary.py, marginals.py, contours.py, covariance.py) with the rule in NumPy, the
reader of the library's result block and the builder of its ``info[...]`` entry.  What the routes (evidence.py: host; resident.py: one
chain on the device; farm.py: many roots per wave) need of a statistic is the same every time, and is stated here once: a ``Stat`` of
plain functions per statistic, ``STATS`` in logging order, and ``measure_wave``, the farm's rule for who shares a device call and who
fails alone.  docs/design/posterior_stats.md has the fields, the wave rule and what adding a statistic takes.

A call's values travel as one dict ``values``: the five keywords by their ``key`` and ``"bounds"``.  A ``Request`` is what is known of a
statistic once a root's parameter count and names are: its resolved spec and its resolved bounds (None: the plain form), hashable, so that
equal values give equal requests.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import contours as _contours
from . import covariance as _covariance
from . import information as _information
from . import marginals as _marginals
from . import summary as _summary

__all__ = ["STATS", "BY_KEY", "INFORMATION", "SUMMARY", "MARGINALS", "CONTOURS", "COVARIANCE", "Stat", "System", "Request", "Asking", "wanted", "values_of",
           "check", "carry", "per_root_bounds", "measure_wave", "log_lines", "param_names"]

#: one system on the device: the address of the raw rows, their stride in doubles, the rows, the measured columns, the addresses of w and fs
System = namedtuple("System", "params ld rows nd w fs")
#: a statistic's resolved spec and resolved bounds ((lo, hi) tuples of floats, or None: the plain form)
Request = namedtuple("Request", "spec bounds")
#: a ready root of a wave: what names it in the results, its system, its values, its parameter names and its root name (or None)
Asking = namedtuple("Asking", "id system values names root")
#: key: the keyword and the info key; attr / spec_attr: where ``MCEvidence`` keeps the last result and the keyword's value; the rest: below
Stat = namedtuple("Stat", "key attr spec_attr per_root check resolve group measure_dev measure_host build lines")

KEYS = ("information", "summary", "marginals", "contours", "covariance")
param_names = _summary.param_names
_SEQ = (list, tuple, np.ndarray)


def wanted(value):
    """is a statistic's keyword set?  (None / False: nothing changes)"""
    return value is not None and value is not False


def values_of(get):
    """the values dict of a call from ``get(keyword)`` (a dict's ``.get``, for one)"""
    return {k: get(k) for k in KEYS + ("bounds",)}


def feed_problem(s, cov_mode, kmax):
    """the 11-tuple ``_capi.evidence_feed_batch_dev`` takes for an auto evidence of system ``s``"""
    return (s.params, s.rows, s.ld, 0, 0, 0, s.nd, cov_mode, kmax, s.w, s.fs)


# ---- one value or one entry per root (the farm) ------------------------------------------------------------------------------------
def spread(value, n, name):
    if isinstance(value, _SEQ):
        if len(value) != n:
            raise ValueError("%s: expected %d entries, got %d" % (name, n, len(value)))
        return list(value)
    return [value] * n


def _entries(value, n, name, is_entry, words, is_one=None):
    """a keyword whose value may itself be a sequence -> one value per root, by the ENTRIES: a list / tuple whose entries are all None
    or ``is_entry`` is one entry per root and must have ``n`` of them; one with no such entry (a sequence of bare numbers), or one
    ``is_one`` takes, is ONE value for every root; anything else is refused in ``words``"""
    if isinstance(value, _SEQ) and len(value) > 0 and not (is_one is not None and is_one(value)):
        slot = [v is None or is_entry(v) for v in value]
        if all(slot):
            return spread(list(value), n, name)
        if any(slot) or is_one is not None:
            raise ValueError("%s=%r: %s" % (name, value, words))
    return [value] * n


def _per_root_summary(value, n):
    return _entries(value, n, "summary", lambda v: isinstance(v, (bool, np.bool_) + _SEQ),
                    "either probabilities (one value for every root) or one entry per root (None, True or a sequence of probabilities each), not a mixture")


def _per_root_marginals(value, n):
    """(contours take this rule too, with its words)"""
    return _entries(value, n, "marginals", lambda v: isinstance(v, (bool, np.bool_, dict) + _SEQ),
                    "either one value for every root or one entry per root (None, True, a sequence of probabilities or a dict each), not a mixture")


def _is_pair(v):
    return isinstance(v, _SEQ) and len(v) == 2 and not any(isinstance(e, _SEQ + (dict,)) for e in v)


def per_root_bounds(value, n):
    """``bounds``: None, "ranges", a mapping or a sequence of (lo, hi) pairs is ONE value; a list of such is one entry per root"""
    return _entries(value, n, "bounds", lambda v: isinstance(v, (str, dict)) or (isinstance(v, _SEQ) and all(_is_pair(e) for e in v)),
                    "either one value for every root or one entry per root (None, 'ranges', a mapping or a sequence of (lo, hi) pairs each), not a mixture",
                    is_one=lambda value: all(_is_pair(v) for v in value))


# ---- what is validated before any work ---------------------------------------------------------------------------------------------
def _check_bounds(values, root=True, **batch):
    _marginals.refuse_bounds(values.get("bounds"), values.get("marginals"), root=root, contours=values.get("contours"))


def check(values, root=True, keys=None, **batch):
    """what every route refuses up front, in the order it always did: summary, marginals, bounds, contours, covariance (``keys``: these
    only).  ``batch``: brange, nbatch, isfunc, where the route has them; ``root``: None on a route without a root name"""
    for key, fn in _CHECKS:
        if keys is None or key in keys:
            fn(values, root=root, **batch)


def carry(values):
    """the keywords a root takes with it to another route: the statistics it asks for, and ``bounds`` where its marginals, or contours
    that ask for the call's, take them"""
    out = {k: values[k] for k in KEYS if wanted(values.get(k))}
    takes = "marginals" in out or ("contours" in out and _contours.bounds_wanted(out["contours"]) and out["contours"]["bounds"] is True)
    if values.get("bounds") is not None and takes:
        out["bounds"] = values["bounds"]
    return out


# ---- resolve: None, or the Request of a root whose parameter count and names are known ----------------------------------------------
def _frozen(bnd):
    return None if bnd is None else tuple(tuple(float(x) for x in side) for side in bnd)


def _resolve_flag(key):
    return lambda values, names, ndim, root: Request(True, None) if wanted(values.get(key)) else None


def _resolve_summary(values, names, ndim, root):
    probs = _summary.spec(values.get("summary"))
    return None if probs is None else Request(probs, None)


def _resolve_covariance(values, names, ndim, root):
    return None if _covariance.spec(values.get("covariance")) is None else Request(True, None)


def _resolve_marginals(values, names, ndim, root):
    value, bounds = values.get("marginals"), values.get("bounds")
    sp = _marginals.spec(value)
    _marginals.refuse_bounds(bounds, value, root=root, contours=values.get("contours"))
    if sp is None:                                     # (bounds= without marginals= is here only where contours take it)
        return None
    bnd = _marginals.bounds_spec(bounds, names=names, root=root, marginals=value)
    if bnd is not None:
        _marginals.note_contours(values.get("contours"))
    return Request(sp, _frozen(bnd))


def _resolve_contours(values, names, ndim, root):
    value = values.get("contours")
    if not wanted(value):
        return None
    sp = _contours.spec(value, ndim=ndim, names=names)
    return Request(sp, _frozen(_contours.bounds_spec(value, names=names, ndim=ndim, root=root, bounds=values.get("bounds"))))


def _group(req):
    """what two roots agree on to share one device call"""
    return req.spec, req.bounds is not None


# ---- measure_dev: ONE library call for systems of one group ------------------------------------------------------------------------
def _blocks_dev(workspace_bytes, ws_args, call, from_block, systems, device, stream):
    """what the per-parameter statistics share: the workspace (``workspace_bytes`` of the rows of all systems, their number, their
    widest and ``ws_args``), the one library call (``call``: what follows the systems and their spec) and ``from_block`` of every
    system's block"""
    import torch
    wsb = workspace_bytes(sum(s[2] for s in systems), len(systems), max(s[3] for s in systems), *ws_args)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device="cuda:%d" % int(device))
    return [from_block(b, s) for b, s in zip(call(ws.data_ptr(), wsb, stream), systems)]


def _bounds_of(requests):
    """None for a plain group, the (lo, hi) of every system for a bounded one"""
    return None if requests[0].bounds is None else [r.bounds for r in requests]


def _moments_dev(systems, requests, device, stream):
    """``mce_like_moments_dev`` -> one ``information.moments`` dict per system"""
    import torch
    from . import _capi
    wsb = _capi.like_moments_workspace_bytes(sum(s.rows for s in systems), len(systems))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device="cuda:%d" % int(device))
    return [_information.from_block(b) for b in _capi.like_moments_dev([(s.fs, s.w, s.rows) for s in systems], ws.data_ptr(), wsb, stream)]


def _summary_dev(systems, requests, device, stream, pass_elems=0):
    """``mce_param_summary_dev`` -> one ``summary.measure`` dict per system"""
    from . import _capi
    q = _summary.targets(requests[0].spec)
    nmax = max(s.rows for s in systems)
    return _blocks_dev(lambda rows, nseg, dmax: _capi.param_summary_workspace_bytes(rows, nmax, nseg, dmax, len(q), pass_elems), (),
                       lambda *a: _capi.param_summary_dev([tuple(s) for s in systems], q, *a, pass_elems), lambda b, s: _summary.from_block(b, s.nd, len(q)),
                       systems, device, stream)


def _marginals_dev(systems, requests, device, stream):
    """``mce_param_marginals_dev``, or ``mce_param_marginals_bounded_dev`` for a bounded group -> one ``marginals.measure`` /
    ``measure_bounded`` dict per system"""
    from . import _capi
    (probs, grid, scale), bounds, segs = requests[0].spec, _bounds_of(requests), [s[:5] for s in systems]
    if bounds is None:
        return _blocks_dev(_capi.param_marginals_workspace_bytes, (len(probs), grid), lambda *a: _capi.param_marginals_dev(segs, probs, grid, scale, *a),
                           lambda b, s: _marginals.from_block(b, s.nd, len(probs), grid), systems, device, stream)
    return _blocks_dev(_capi.param_marginals_bounded_workspace_bytes, (len(probs), grid), lambda *a: _capi.param_marginals_bounded_dev(segs, bounds, probs, grid, scale, *a),
                       lambda b, s: _marginals.from_block_bounded(b, s.nd, len(probs), grid), systems, device, stream)


def _contours_dev(systems, requests, device, stream):
    """``mce_param_contours_dev``, or ``mce_param_contours_bounded_dev`` for a bounded group -> one ``contours.measure`` /
    ``measure_bounded`` dict per system"""
    from . import _capi
    (probs, grid, scale, cols), bounds, segs = requests[0].spec, _bounds_of(requests), [s[:5] for s in systems]
    if bounds is None:
        return _blocks_dev(_capi.param_contours_workspace_bytes, (len(cols), len(probs), grid), lambda *a: _capi.param_contours_dev(segs, cols, probs, grid, scale, *a),
                           lambda b, s: _contours.from_block(b, len(cols), len(probs), grid), systems, device, stream)
    return _blocks_dev(_capi.param_contours_bounded_workspace_bytes, (len(cols), len(probs), grid),
                       lambda *a: _capi.param_contours_bounded_dev(segs, cols, bounds, probs, grid, scale, *a),
                       lambda b, s: _contours.from_block_bounded(b, len(cols), len(probs), grid), systems, device, stream)


def _covariance_dev(systems, requests, device, stream):
    """``mce_param_cov_dev`` -> one ``covariance.measure`` dict per system"""
    from . import _capi
    segs = [s[:5] for s in systems]
    return _blocks_dev(_capi.param_cov_workspace_bytes, (), lambda *a: _capi.param_cov_dev(segs, *a), lambda b, s: _covariance.from_block(b, s.nd), systems, device, stream)


# ---- measure_host: the host route's choice between NumPy and the library ------------------------------------------------------------
def host_device(backend):
    """the device the HIP backend's host arrays are uploaded to, or None: the rule in NumPy"""
    if getattr(backend, "name", None) != "hip":
        return None
    import torch
    devs = getattr(backend, "devices", None)
    return devs[0] if devs else (torch.cuda.current_device() if torch.cuda.is_available() else 0)


def _marginals_host(a, x, fs, req, backend):
    device, sp, bnd = host_device(backend), req.spec, req.bounds
    if device is None:
        return _marginals.measure(a, x, *sp) if bnd is None else _marginals.measure_bounded(a, x, bnd, *sp)
    return _marginals.measure_native(a, x, *sp, device=device) if bnd is None else _marginals.measure_bounded_native(a, x, bnd, *sp, device=device)


def _contours_host(a, x, fs, req, backend):
    device, (probs, grid, scale, cols), bnd = host_device(backend), req.spec, req.bounds
    if device is None:
        return _contours.measure(a, x, cols, probs, grid, scale) if bnd is None else _contours.measure_bounded(a, x, cols, bnd, probs, grid, scale)
    return (_contours.measure_native(a, x, cols, probs, grid, scale, device=device) if bnd is None else
            _contours.measure_bounded_native(a, x, cols, bnd, probs, grid, scale, device=device))


def _refuse(module, key):
    return lambda values, root=True, **batch: module.refuse(values.get(key), **batch)


INFORMATION = Stat("information", None, "information", lambda v, n: spread(v, n, "information"), _refuse(_information, "information"),
                   _resolve_flag("information"), _group, _moments_dev, lambda a, x, fs, req, backend: _information.moments(a, fs),
                   lambda blk, req, names, logLmax, lnE: _information.build(blk, logLmax, lnE), _information.lines)
SUMMARY = Stat("summary", "param_summary", "summary_spec", _per_root_summary, _refuse(_summary, "summary"), _resolve_summary, _group, _summary_dev,
               lambda a, x, fs, req, backend: _summary.measure(a, x, fs, _summary.targets(req.spec)),
               lambda blk, req, names, logLmax, lnE: _summary.build(blk, req.spec, logLmax, names), _summary.lines)
MARGINALS = Stat("marginals", "param_marginals", "marginals_spec", _per_root_marginals, _refuse(_marginals, "marginals"), _resolve_marginals, _group,
                 _marginals_dev, _marginals_host, lambda blk, req, names, logLmax, lnE: _marginals.build(blk, req.spec, names), _marginals.lines)
CONTOURS = Stat("contours", "param_contours", "contours_spec", _per_root_marginals, _refuse(_contours, "contours"), _resolve_contours, _group,
                _contours_dev, _contours_host, lambda blk, req, names, logLmax, lnE: _contours.build(blk, req.spec, names), _contours.lines)
COVARIANCE = Stat("covariance", "param_cov", "covariance", lambda v, n: spread(v, n, "covariance"), _refuse(_covariance, "covariance"),
                  _resolve_covariance, _group, _covariance_dev, lambda a, x, fs, req, backend: _covariance.measure(a, x),
                  lambda blk, req, names, logLmax, lnE: _covariance.build(blk, names), lambda result: [])

#: in logging order
STATS = (INFORMATION, SUMMARY, MARGINALS, CONTOURS, COVARIANCE)
BY_KEY = {st.key: st for st in STATS}
_CHECKS = (("information", INFORMATION.check), ("summary", SUMMARY.check), ("marginals", MARGINALS.check), ("bounds", _check_bounds),
           ("contours", CONTOURS.check), ("covariance", COVARIANCE.check))


def log_lines(info):
    """the lines of the statistics ``info`` holds, in logging order: what goes before the ln(B) lines"""
    return [line for st in STATS if (info or {}).get(st.key) for line in st.lines(info[st.key])]


# ---- the wave rule ------------------------------------------------------------------------------------------------------------------
def measure_wave(ready, device=0, stream=0, measure=None):
    """The statistics of a wave's ready roots (``Asking``s) -> (found: {id: {key: (block, request)}}, failed: {id: ValueError}, the roots
    still ready).  Per statistic, in ``STATS``' order: every root's request is resolved; a ``ValueError`` there fails that root alone and
    takes it out of ``ready`` before the next statistic; the others are grouped by ``group(request)`` and every group, in sorted order,
    is ONE ``measure(stat, systems, requests)`` call (default: the statistic's ``measure_dev`` on ``device`` and ``stream``).  Nothing
    here touches the device."""
    if measure is None:
        measure = lambda st, systems, requests: st.measure_dev(systems, requests, device, stream)       # noqa: E731
    found, failed = {a.id: {} for a in ready}, {}
    for st in STATS:
        reqs = {}
        for a in ready:
            try:
                req = st.resolve(a.values, a.names, a.system.nd, a.root)
                if req is not None:
                    reqs[a.id] = req
            except ValueError as e:
                failed[a.id] = e
        ready = [a for a in ready if a.id not in failed]
        for g in sorted(set(st.group(r) for r in reqs.values())):
            who = [a for a in ready if a.id in reqs and st.group(reqs[a.id]) == g]
            for a, blk in zip(who, measure(st, [a.system for a in who], [reqs[a.id] for a in who])):
                found[a.id][st.key] = (blk, reqs[a.id])
    return found, failed, ready
