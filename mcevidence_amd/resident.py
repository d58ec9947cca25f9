"""The resident route: chain files -> ln E without the chain ever coming back to the host.

``MCEvidence(root, ...)`` reads the files into host arrays, burns, concatenates, thins and splits them in NumPy
(``chains.py``) and uploads the parameter rows again for the search.  Here the files are parsed on the device
(``mce_chain_dev_read_dev``), and burn-in, concatenation, thinning, the optional s1/s2 split, the column split and the
``fs`` / ``SumW`` reductions run there too (``mce_chain_*_dev``: csrc/chain_prep_kernels.hpp, rules in
csrc/chain_prep.hpp); the result goes to ``mce_evidence_feed_part_dev_f64`` (part 0 of 1) in place.  Only scalars come
back.  Opt-in: nothing else in the package takes this route by itself.

``ResidentChains.from_files`` / ``.from_arrays`` build the resident chain, ``.evidence(...)`` returns what
``MCEvidence(root, ...).evidence(...)`` returns.  ``evidence_from_files`` takes the keywords of both, runs this route
where ``plan`` says it applies and ``MCEvidence(root, ...).evidence(...)`` unchanged where it does not
(``info["route"]``, ``info["declined"]``).  docs/design/chain_resident.md has the passes and the decline table.
"""
from __future__ import annotations

import glob
import logging
import math
import os
import time

import numpy as np

from . import chains as _chains
from . import information as _information
from . import posterior as _post

logger = logging.getLogger("mcevidence_amd")

__all__ = ["ResidentChains", "ResidentDecline", "evidence_from_files", "plan", "REASONS"]

RESIDENT = "resident"

#: why the route declines (``plan``, and the weight cases found on the device)
REASONS = {
    "poisson": "0 < thinlen < 1 draws Poisson weights from the host's RNG",
    "negative_thinlen": "thinlen < 0: the host route raises",
    "isfunc": "importance sampling (isfunc) alters the weights on the host",
    "batches": "batched runs (brange / nbatch > 1) slice the chain on the host",
    "verbose": "verbose > 1 logs per-neighbour volumes from the distances",
    "covtype": "covtype other than 'all' / 'single' is the host route's business",
    "split_single": "split with covtype='single' whitens s1 and s2 with different eigen-systems",
    "ndim": "ndim > 127: beyond the device feeders",
    "distributed": "a process group is initialised: multi-rank chains are not resident",
    "columns": "the files' column counts differ",
    "rows": "fewer than 2 rows left",
    "not_files": "not a chain file root or a list of file names",
    "ischain": "ischain=False: the host route raises",
    "ambiguous_weights": "the weights' fractional parts sum to within 1e-6 of the integer-weight threshold 1e-4",
    "bad_weights": "a weight is negative, not finite or beyond 2^53",
    "thin_corr": "thin_corr: the autocorrelation length is measured root by root (the per-root resident route)",
    "jackknife_cross": "jackknife of a cross evidence whitens on the host",
}


#: mce_chain_weights_dev's verdicts (csrc/chain_prep.hpp: kRule*, kDecline*)
RULE_NAME = {0: "none", 1: "integer", 2: "bin"}
DECLINE_REASON = {-1: "bad_weights", -2: "ambiguous_weights", -3: "negative_thinlen"}


class ResidentDecline(Exception):
    """The resident route does not apply; ``reason`` says why (one of ``REASONS``' values)."""

    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


def plan(thinlen=0, isfunc=None, brange=None, nbatch=1, verbose=1, covtype="all", split=False, ndim=None, nparam=None,
         distributed=False, ncols=None, nrows=None, ischain=True, thin_corr=None, converge=None, converge_by="auto", jackknife=None, nchains=None,
         summary=None, covariance=None, marginals=None, contours=None, bounds=None):
    """``"resident"`` or the reason why the route declines.  A pure function of the call's keywords and of what is known
    about the data at the time (``ncols``: the files' column counts, ``nrows``: rows left after burn-in / thinning,
    ``nparam``: parameter columns; None: not known yet).  ``thin_corr`` (thinning by the measured autocorrelation length) is resident
    work and declines nothing; together with a ``thinlen`` other than 0 it is the ValueError every route raises.  ``converge`` /
    ``converge_by`` (the Gelman-Rubin R-1 of the burned chains) are resident work too and decline nothing; a value they cannot take
    is the ValueError every route raises.  ``jackknife`` (the delete-a-group error bars; ``nchains``: the chains, where known) is resident
    work for an auto evidence; with a split it declines to the host route, which whitens s1 and s2 there; a number of groups or a
    ``by`` it cannot take is the ValueError every route raises.  ``summary``, ``marginals``, ``contours``, ``covariance`` and ``bounds``
    (the statistics of posterior.py) are resident work too: they are validated -- a value they cannot take is the ValueError every route
    raises -- and decline nothing."""
    _post.check(dict(summary=summary, marginals=marginals, contours=contours, covariance=covariance, bounds=bounds))
    if not ischain:
        return REASONS["ischain"]
    _chains.thin_corr_scale(thin_corr, thinlen)
    _chains.converge_spec(converge, converge_by)
    jspec = jack_spec(jackknife, nchains)
    if thinlen < 0:
        return REASONS["negative_thinlen"]
    if 0 < thinlen < 1:
        return REASONS["poisson"]
    if isfunc:
        return REASONS["isfunc"]
    if brange is not None or nbatch > 1:
        return REASONS["batches"]
    if verbose is not None and verbose > 1:
        return REASONS["verbose"]
    if covtype not in ("all", "single"):
        return REASONS["covtype"]
    if split and covtype == "single":
        return REASONS["split_single"]
    if jspec is not None and split:
        return REASONS["jackknife_cross"]
    eff = ndim if nparam is None else (nparam if ndim is None else min(int(ndim), nparam))
    if eff is not None and eff > 127:
        return REASONS["ndim"]
    if distributed:
        return REASONS["distributed"]
    if ncols is not None and len(set(int(c) for c in ncols)) > 1:
        return REASONS["columns"]
    if nrows is not None and nrows < 2:
        return REASONS["rows"]
    return RESIDENT


def _resolve_files(fname, idchain=0, idpattern="_?.txt"):
    """the files ``MCSamples.load_from_file`` reads for ``fname``"""
    if isinstance(fname, (list, tuple)):
        flist = list(fname)
    elif os.path.isfile(fname):
        flist = [fname]
    elif "*" in fname or "?" in fname:
        flist = sorted(glob.glob(fname))
    elif idchain > 0:
        flist = ["%s_%d.txt" % (fname, idchain)]
    else:
        flist = sorted(glob.glob(fname + idpattern))
    if not flist:
        raise IOError("no chain files found for %r" % (fname,))
    return flist


def _is_file_root(method):
    return isinstance(method, str) or (isinstance(method, (list, tuple)) and len(method) > 0 and all(isinstance(f, str) for f in method))


def _distributed():
    """is a process group initialised?  (multi-rank chains are not resident)"""
    try:
        import torch.distributed as dist
    except Exception:
        return False
    return bool(dist.is_available() and dist.is_initialized())


def _ms(t0):
    return (time.perf_counter() - t0) * 1e3


# ---- the host rules every route shares (this module, farm.py, evidence.py) -------------------------------------------------------
def burn_start(n, burnlen):
    """the first row kept of a chain of ``n`` rows (chains.MCSamples.removeBurn; csrc/chain_prep.hpp: burn_start)"""
    return min(n, int(n * burnlen) if burnlen < 1 else int(burnlen)) if burnlen > 0 else 0


def check_columns(iw, ilike, itheta, ncols):
    if ncols <= max(iw, ilike, itheta) or min(iw, ilike, itheta) < 0:
        raise ValueError("columns iw=%d ilike=%d itheta=%d of a chain with %d" % (iw, ilike, itheta, ncols))


def effective_ndim(ndim, nparam):
    """the parameter columns the search takes"""
    nd = nparam if ndim is None else int(ndim)
    if nd < 1:
        raise ValueError("ndim must be >= 1 (got %r)" % (ndim,))
    if nd > nparam:
        logger.warning("ndim=%s exceeds the %s parameter columns of the chain; using all of them" % (ndim, nparam))
        nd = nparam
    return nd


def check_reduced(logLmax, SumW, nan_like, bad_w):
    """what the host route raises for these reduce scalars (``mce_chain_reduce_dev`` / ``_farm_prep_dev``)"""
    if bad_w:
        raise ValueError("weight contains NaN or infinity")
    if nan_like or math.isinf(logLmax):
        raise ValueError("fs contains NaN or +infinity")


def mle_from_sums(dotp, jac, SumW, logLmax, n1, kmax, log_prior_volume, cross):
    """ln E_k from the reduced sums (reference :1120-1131): MLE[kmax]; entry 0 stays 0 without ``cross``"""
    k0 = 0 if cross else 1
    mle = np.zeros(kmax)
    for k in range(k0, kmax):
        k_nn = k if k0 == 1 else k + 1
        mle[k] = math.log(SumW * (dotp[k] / (n1 * k_nn + 1.0)) * jac) + logLmax - log_prior_volume
    return mle


def conv_device_segments(parts, ncols, by):
    """the segments of burned parts ``[(device address, rows)]`` -> (the ``by`` taken, [(device address, rows)]): a half is a segment
    whose address is offset (chains.conv_segments)"""
    by, table = _chains.conv_segments([n for _, n in parts], by)
    return by, [((parts[p][0] + f * int(ncols) * 8) if m > 0 else 0, m) for p, f, m in table]


def conv_measure_dev(systems, ncols, iw, itheta, nd, device, stream):
    """ONE ``mce_chain_conv_dev`` call for ``systems`` (a list of segment lists ``[(device address, rows)]`` of one ``ncols`` and
    ``nd``) -> one result dict per system (``chains.conv_info`` takes it)"""
    import torch
    from . import _capi
    segs = [sg for sy in systems for sg in sy]
    seg_sys = [y for y, sy in enumerate(systems) for _ in sy]
    wsb = _capi.chain_conv_workspace_bytes(sum(n for _, n in segs), len(segs), len(systems), nd)
    if wsb == 0:
        raise ValueError("converge: ndim=%r (1 .. %d expected)" % (nd, _chains.CONV_MAX_DIM))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:%d" % int(device))
    res = _capi.chain_conv_dev(segs, seg_sys, len(systems), ncols, iw, itheta, nd, ws.data_ptr(), wsb, stream)
    return [dict(r_minus_1=res["r_minus_1"][y], per_param=res["per_param"][y], status=res["status"][y], column=res["column"][y], used=res["used"][y])
            for y in range(len(systems))]


# ---- the jackknife of a chain that stays on the device (docs/design/jackknife_resident.md; this module and farm.py) -----------------
def jack_spec(jackknife, nchains=None):
    """None, or dict(groups, by, G) of the ``jackknife`` keyword: G is the number of groups (None while ``by="chains"`` does not
    know the chains yet); raises the ValueErrors the host route raises, with its words"""
    from . import jackknife as _jk
    spec = _jk.spec(jackknife)
    if spec is not None:
        spec["G"] = _jk.resolve_groups(spec["groups"], spec["by"], nchains)
    return spec


def jack_groups_dev(systems, device, stream):
    """ONE ``mce_jack_groups_dev`` call for ``systems`` = [(src: the int64 device tensor of the kept rows or None, parts [(address, rows)],
    n, G, by)] of auto evidences (row i is sample row i, the sample has n rows) -> one int32 device tensor [n] per system"""
    import torch
    from . import _capi
    outs = [torch.empty(max(int(n), 1), dtype=torch.int32, device="cuda:%d" % int(device))[:int(n)] for _, _, n, _, _ in systems]
    segs = []
    for (src, parts, n, G, by), out in zip(systems, outs):
        first = None
        if by == "chains":
            first = np.concatenate([[0], np.cumsum([m for _, m in parts])])[:len(parts)]
        segs.append((0, src.data_ptr() if src is not None else 0, first, n, n, G, by, out.data_ptr()))
    _capi.jack_groups_dev(segs, stream)
    return outs


def jack_leave_out_dev(systems, device, stream):
    """ONE ``mce_jack_leave_out_dev`` call for ``systems`` = [(device address of w, of fs or 0: no moments, the int32 group tensor, rows,
    G)] -> one [G + 1, 8] block per system (``_capi.JACK_LEAVE_OUT_FIELDS``)"""
    import torch
    from . import _capi
    wsb = _capi.jack_leave_out_workspace_bytes(sum(n for _, _, _, n, _ in systems), len(systems), max(G for _, _, _, _, G in systems))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device="cuda:%d" % int(device))
    return _capi.jack_leave_out_dev([(w, fs, g.data_ptr(), n, G) for w, fs, g, n, G in systems], ws.data_ptr(), wsb, stream)


def jack_run(params, n1, ld, nd, kmax, w, fs, gq, spec, device, backend):
    """the ladder of one auto evidence whose rows are on the device: ``mce_evidence_feed_whiten_dev_f64`` on the gathered rows (device
    addresses ``params`` [n1, ld], ``w``, ``fs``), then ``jackknife.run_ladder`` over a ``HipSession`` of device tensors -> (dotp_groups,
    dotp_full, rows_per_level, jacobian, kernel_ms)"""
    import torch
    from . import _capi
    from .jackknife import HipSession, run_ladder
    dev = "cuda:%d" % int(device)
    X = torch.empty((n1, nd), dtype=torch.float64, device=dev)
    w2 = torch.empty(n1, dtype=torch.float64, device=dev)
    fs2 = torch.empty(n1, dtype=torch.float64, device=dev)
    with backend._scoped():
        jac, _, _ = _capi.evidence_feed_whiten_dev(params, n1, ld, nd, kmax, w, fs, X.data_ptr(), w2.data_ptr(), fs2.data_ptr(), device=device,
                                                   want_checksum=False)
    session = HipSession.from_device(X, w2, fs2, gq, kmax, spec["G"], jac, device)
    groups, full, per_level = run_ladder(session, n1, spec["G"], 1, kmax)
    return groups, full, per_level, jac, list(session.kernel_ms)


def jack_result(run, block, spec, SumW, logLmax, n1, kmax, log_prior_volume):
    """``info["jackknife"]`` from the ladder's sums and the leave-out block: S_b and SumW_b are the block's rows and weight sums"""
    from .jackknife import result
    groups, full, per_level, jac, kernel_ms = run
    out = result(groups, full, per_level, jac, SumW, n1, block[1:, 1], block[1:, 0], logLmax, kmax, log_prior_volume, spec["G"], spec["by"])
    if kernel_ms:
        out["kernel_ms"] = kernel_ms
    return out


def jack_information(inf, block, logLmax, jk):
    """sigma, groups and by of ``info["information"]`` from the deleted sets' moments of the leave-out block"""
    return _information.with_jackknife_moments(inf, [_information.from_leave_out(b) for b in block[1:]], logLmax, jk)


def route_info(route, nparam, nd, nread, nsample):
    """the info dict of ``MCEvidence.evidence(info=True)`` for a route that kept the chain on the device"""
    return {"NparamsMC": nparam, "Nsamples_read": nread, "Nparams_read": nparam, "NparamsCosmo": nd,
            "Nsamples": ", ".join(str(x) for x in nsample), "route": route}


#: the order ``ResidentChains.evidence`` resolves (and so validates) its statistics in; it measures them in ``posterior.STATS``' order
_RESOLVED = ("information", "summary", "covariance", "marginals", "contours")


class ResidentChains(object):
    """One or more chains on GPU ``device``, burned, concatenated and thinned there.

    ``nrows`` / ``nparam``: the shape ``MCSamples(...).samples[:, itheta:]`` has; ``rule``: ``"none" | "integer" | "bin"``
    (the thinning rule taken); ``keep()``: the kept rows in the burned, concatenated numbering (the host's ``keep``);
    ``to_host()``: the array ``MCSamples(...).samples`` holds; ``stats``: reader statistics per file and milliseconds per
    stage.  ``thin_corr`` (None / False, True or a scale > 0; with ``corr_min``, ``corr_max_lag`` and the estimator's ``ndim``) thins by
    the autocorrelation length measured on the device (``mce_chain_corr_dev``) instead of a given ``thinlen``; ``thin_corr`` holds what
    was found.  ``converge`` (None / False, True or a threshold > 0; with ``converge_by`` and ``ndim``) measures the Gelman-Rubin R-1 of
    the burned, unthinned parts on the device (``mce_chain_conv_dev``); ``converge`` then holds what ``info["converge"]`` reports.
    Raises ``ResidentDecline`` where the route does not apply, ``RuntimeError`` without a GPU."""

    def __init__(self, tensors, burnlen=0, thinlen=0, iw=0, ilike=1, itheta=2, device=0, reader_stats=None, thin_corr=None,
                 corr_min=_chains.CORR_MIN, corr_max_lag=_chains.CORR_MAX_LAG, ndim=None, converge=None, converge_by="auto"):
        import torch
        self._torch = torch
        self.device = int(device)
        self.iw, self.ilike, self.itheta = int(iw), int(ilike), int(itheta)
        self.stats = {"files": list(reader_stats or []), "ms": {}}
        self.nchains = len(tensors)
        if not tensors:
            raise ValueError("the chains array is empty")
        scale = _chains.thin_corr_scale(thin_corr, thinlen)
        self.thin_corr = None
        spec = _chains.converge_spec(converge, converge_by)
        self.converge = None
        for st in _post.STATS:                             # (information, summary, marginals, contours, covariance:
            setattr(self, st.key, None)                    #  what the last evidence(<key>=..) found)
        self.names_root = None                             # (the root whose .paramnames file names the parameters, where there is one)
        self.jackknife = None                              # (what the last evidence(jackknife=...) found,
        self.jackknife_block = None                        #  and its leave-one-group-out block: _capi.JACK_LEAVE_OUT_FIELDS per slot)
        reason = plan(thinlen=thinlen, ncols=[t.shape[1] for t in tensors], distributed=_distributed())
        if reason != RESIDENT:
            raise ResidentDecline(reason)
        self.ncols = int(tensors[0].shape[1])
        check_columns(self.iw, self.ilike, self.itheta, self.ncols)
        self.nparam = self.ncols - self.itheta
        self._tensors = list(tensors)                     # (owners of the memory the parts point into)
        self._parts = []
        for t in self._tensors:
            n = int(t.shape[0])
            start = burn_start(n, burnlen)
            if burnlen > 0:
                logger.info("Removing %s lines as burn in" % start)
            self._parts.append((t.data_ptr() + start * self.ncols * 8, n - start))
        self.nburned = sum(n for _, n in self._parts)
        self._src = self._new_w = None
        self.rule = "none"
        self.totals = None
        if self.nburned < 1:                              # (nothing to select from; fewer than 2 rows decline in evidence())
            raise ResidentDecline(REASONS["rows"])
        t0 = time.perf_counter()
        if spec is not None:
            self._converge(spec, ndim)
            self.stats["ms"]["converge"] = _ms(t0)
            t0 = time.perf_counter()
        if scale is not None:
            thinlen = self._measure(scale, ndim, corr_min, corr_max_lag)
            self.stats["ms"]["corr"] = _ms(t0)
            t0 = time.perf_counter()                      # ("select" keeps its meaning: the thinning alone)
        if thinlen not in (0, 1):
            self._select(float(thinlen))
        self.stats["ms"]["select"] = _ms(t0)
        self.nrows = self.nburned if self._src is None else int(self._src.shape[0])

    # -- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, arrays, burnlen=0, thinlen=0, iw=0, ilike=1, itheta=2, device=0, **corr):
        """Host arrays (one per chain) uploaded as they are.  Unlike ``MCSamples``, which ignores ``burnlen`` / ``thinlen``
        for chains passed in memory (and keeps doing so), this entry HONOURS them, with the rules files get: it exists so
        that the device preparation can be used and tested apart from the reader."""
        from . import _capi
        _capi.require_device()
        import torch
        seq = list(arrays.values()) if isinstance(arrays, dict) else list(arrays)
        with torch.cuda.device(int(device)):
            tensors = []
            for a in seq:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.ndim != 2:
                    raise ValueError("a chain must be a 2-D array, got shape %r" % (a.shape,))
                tensors.append(torch.from_numpy(a).to("cuda:%d" % int(device)))
            return cls(tensors, burnlen, thinlen, iw, ilike, itheta, device, **corr)

    @classmethod
    def from_files(cls, root_or_paths, burnlen=0, thinlen=0, iw=0, ilike=1, itheta=2, idchain=0, idpattern="_?.txt", device=0,
                   **corr):
        """Chain text files parsed on the device and left there; the files are those ``MCSamples.load_from_file`` reads.  ``corr``:
        thin_corr, corr_min, corr_max_lag, ndim, converge, converge_by."""
        import mmap
        from . import _capi, chain_io
        _capi.require_device()
        import torch
        flist = _resolve_files(root_or_paths, idchain, idpattern)
        logger.debug("Reading from files: " + ", ".join(flist))
        t0 = time.perf_counter()
        tensors, stats = [], []
        with torch.cuda.device(int(device)):
            for path in flist:
                with open(path, "rb") as f:
                    size = os.fstat(f.fileno()).st_size
                    mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if size > 0 else None
                    try:
                        view = np.frombuffer(mm, dtype=np.uint8) if mm is not None else None
                        try:
                            handle, nrows, ncols = None, 0, 0
                            try:
                                handle, nrows, ncols = _capi.chain_dev_open(view.ctypes.data if view is not None else None, size, device)
                                out = torch.empty((nrows, ncols), dtype=torch.float64, device="cuda:%d" % int(device))
                                stats.append(dict(_capi.chain_dev_read_dev(handle, out.data_ptr() if nrows * ncols else 0), path=path))
                            finally:
                                if handle is not None:
                                    _capi.chain_dev_close(handle)
                        except ValueError as dev_err:
                            raise chain_io.refused(path, dev_err)
                        finally:
                            del view
                    finally:
                        if mm is not None:
                            mm.close()
                if nrows == 0:                               # (np.loadtxt: an empty file is an array of shape (0, 1))
                    out = torch.empty((0, 1), dtype=torch.float64, device="cuda:%d" % int(device))
                tensors.append(out)
            self = cls(tensors, burnlen, thinlen, iw, ilike, itheta, device, reader_stats=stats, **corr)
        self.stats["ms"]["read"] = _ms(t0) - self.stats["ms"]["select"] - self.stats["ms"].get("corr", 0.0) - self.stats["ms"].get("converge", 0.0)
        return self

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _ws(self, nbytes):
        return self._torch.empty(max(int(nbytes), 1), dtype=self._torch.uint8, device="cuda:%d" % self.device)

    def _measure(self, scale, ndim, corr_min, corr_max_lag):
        """thin_corr: the thinning factor from the autocorrelation length of the burned parts, measured on the device"""
        from . import _capi
        nd = effective_ndim(ndim, self.nparam)
        if nd > 127:
            raise ResidentDecline(REASONS["ndim"])
        nparts = len(self._parts)
        wsb = _capi.chain_corr_workspace_bytes(self.nburned, nparts, nd, corr_max_lag)
        if wsb == 0:
            raise ValueError("thin_corr: corr_max_lag=%r" % (corr_max_lag,))
        ws = self._ws(wsb)
        res = _capi.chain_corr_dev(self._parts, self.ncols, self.iw, self.itheta, nd, corr_min, corr_max_lag, ws.data_ptr(), wsb, self._stream())
        if res["rule"] < 0:
            raise ResidentDecline(REASONS[DECLINE_REASON[res["rule"]]])
        res["min_corr"] = corr_min
        self.thin_corr = _chains.corr_info(res, scale)
        logger.info("thin_corr: autocorrelation length %.3f %s units (cap %d) -> thinning factor %d"
                    % (self.thin_corr["length"], self.thin_corr["units"], res["cap"], self.thin_corr["factor"]))
        return float(self.thin_corr["factor"])

    def _converge(self, spec, ndim):
        """converge: the Gelman-Rubin R-1 of the burned, unthinned parts, measured on the device"""
        nd = effective_ndim(ndim, self.nparam)
        if nd > _chains.CONV_MAX_DIM:
            raise ResidentDecline(REASONS["ndim"])
        by, segs = conv_device_segments(self._parts, self.ncols, spec[1])
        res, = conv_measure_dev([segs], self.ncols, self.iw, self.itheta, nd, self.device, self._stream())
        self.converge = _chains.conv_info(res, by, len(segs), self.nburned, spec[0])
        logger.info(_chains.conv_line(self.converge))

    def _select(self, thinlen):
        from . import _capi
        torch = self._torch
        n, nparts = self.nburned, len(self._parts)
        wsb = _capi.chain_select_workspace_bytes(n, nparts)
        ws = self._ws(wsb)
        st = self._stream()
        rule, self.totals = _capi.chain_weights_dev(self._parts, self.ncols, self.iw, thinlen, ws.data_ptr(), wsb, st)
        if rule < 0:
            raise ResidentDecline(REASONS[DECLINE_REASON[rule]])
        if rule == 0:
            return
        edges, nedges = None, 0
        if RULE_NAME[rule] == "bin":
            nbins = int(n * thinlen) if thinlen < 1 else int(n // thinlen)      # (chains.max_weight_bin_thin)
            edges = torch.from_numpy(np.linspace(-1, n, nbins + 1)).to("cuda:%d" % self.device)
            nedges = int(edges.shape[0])
        n_out = _capi.chain_select_count_dev(n, nparts, rule, thinlen, edges.data_ptr() if edges is not None else 0, nedges, ws.data_ptr(), wsb, st)
        src = torch.empty(n_out, dtype=torch.int64, device="cuda:%d" % self.device)
        new_w = torch.empty(n_out, dtype=torch.float64, device="cuda:%d" % self.device)
        _capi.chain_select_fill_dev(n, nparts, rule, thinlen, nedges, n_out, src.data_ptr(), new_w.data_ptr(), ws.data_ptr(), wsb, st)
        torch.cuda.current_stream(self.device).synchronize()        # (the workspace and the edges go out of scope here)
        self._src, self._new_w, self.rule = src, new_w, RULE_NAME[rule]
        logger.info("Thinning with thin length=%s: #old_chain=%s, #new_chain=%s" % (thinlen, n, n_out))

    # -- accessors -----------------------------------------------------------------------------------------------------
    def keep(self):
        """host copy of the kept rows (burned, concatenated numbering); every row when nothing was thinned"""
        return np.arange(self.nburned, dtype=np.int64) if self._src is None else self._src.cpu().numpy()

    def weights(self):
        """host copy of the weight column after thinning"""
        with self._torch.cuda.device(self.device):
            return self._gather(None, want=("w",))["w"].cpu().numpy()

    def rows(self):
        """(params [nrows, nparam], w [nrows]): the kept rows' parameter columns and weights as device tensors, from one gather pass"""
        with self._torch.cuda.device(self.device):
            out = self._gather(None, want=("params", "w"))
        return out["params"], out["w"]

    def _gather(self, rows, want):
        """one gather pass -> dict of device tensors among params / w / like / full; ``rows``: int64 device tensor or None"""
        from . import _capi
        torch = self._torch
        dev = "cuda:%d" % self.device
        n_out = self.nrows if rows is None else int(rows.shape[0])
        out = {}
        if "params" in want:
            out["params"] = torch.empty((n_out, self.nparam), dtype=torch.float64, device=dev)
        if "w" in want:
            out["w"] = torch.empty(n_out, dtype=torch.float64, device=dev)
        if "like" in want:
            out["like"] = torch.empty(n_out, dtype=torch.float64, device=dev)
        if "full" in want:
            out["full"] = torch.empty((n_out, self.ncols), dtype=torch.float64, device=dev)
        wsb = _capi.chain_gather_workspace_bytes(len(self._parts))
        ws = self._ws(wsb)
        ptr = lambda k: out[k].data_ptr() if k in out else 0                    # noqa: E731
        _capi.chain_gather_dev(self._parts, self.ncols, self.iw, self.ilike, self.itheta,
                               self._src.data_ptr() if self._src is not None else 0, self._new_w.data_ptr() if self._new_w is not None else 0,
                               self.nrows, rows.data_ptr() if rows is not None else 0, n_out, ptr("params"), ptr("w"), ptr("like"), ptr("full"),
                               ws.data_ptr(), wsb, self._stream())
        return out

    def _reduce(self, s1, pos_lnp):
        """(fs, (max(logL), SumW, NaN likelihoods, weights that are not finite)) of the gathered ``s1``; the stream is synchronised"""
        from . import _capi
        n1 = int(s1["w"].shape[0])
        fs = self._torch.empty(n1, dtype=self._torch.float64, device="cuda:%d" % self.device)
        wsb = _capi.chain_reduce_workspace_bytes(n1)
        ws = self._ws(wsb)
        return fs, _capi.chain_reduce_dev(s1["like"].data_ptr(), s1["w"].data_ptr(), n1, pos_lnp, fs.data_ptr(), ws.data_ptr(), wsb, self._stream())

    def to_host(self):
        """the array ``MCSamples(...).samples`` holds: the burned, concatenated, thinned rows, all columns"""
        with self._torch.cuda.device(self.device):
            return self._gather(None, want=("full",))["full"].cpu().numpy()

    def _index_list(self, rows):
        rows = np.asarray(rows)
        if rows.dtype == bool:
            rows = np.nonzero(rows)[0]
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < -self.nrows or rows.max() >= self.nrows):
            raise IndexError("split row out of range for a chain of %d rows" % self.nrows)
        rows = np.where(rows < 0, rows + self.nrows, rows)
        return self._torch.from_numpy(rows).to("cuda:%d" % self.device)

    # -- the estimator ---------------------------------------------------------------------------------------------------
    def evidence(self, kmax=5, ndim=None, priorvolume=1, covtype="all", pos_lnp=False, split=False, s1frac=0.5, split_rows=None,
                 info=False, backend=None, information=None, jackknife=None, summary=None, covariance=None, marginals=None,
                 contours=None, bounds=None):
        """ln E as ``MCEvidence(...).evidence(...)`` returns it (``MLE[1:]``, and the info dict if ``info=True``; it
        carries ``info["route"] = "resident"``).  ``split=True``: the reference's random split, drawn on the host with the
        call ``MCSamples.chain_split`` makes (same RNG consumption); ``split_rows=(s1, s2)``: ``set_split``.
        ``backend``: a ``HipBackend`` whose ``recheck_rows`` applies to the search.  ``information`` (None or True): <ln L>_P, D_KL and
        the model dimensionality in ``info["information"]``, from one ``mce_like_moments_dev`` call on the gathered weights and fs.
        ``jackknife`` (None, True, a number of groups or dict(groups, by)): the delete-a-group error bars of the host route's
        ``evidence_jackknife`` in ``info["jackknife"]`` (and ``self.jackknife``) -- after the usual feed, whose result is returned
        unchanged, the gathered rows are whitened on the device, ``mce_jack_groups_dev`` forms the group ids, the ladder runs on device
        tensors and ONE ``mce_jack_leave_out_dev`` call gives S_b, SumW_b and, with ``information``, the deleted sets' moments.
        ``summary``, ``marginals``, ``contours``, ``covariance`` and ``bounds``: the statistics of posterior.py
        (docs/design/posterior_stats.md), each from ONE library call on the gathered rows and weights BEFORE the feed and the jackknife
        ladder, while the rows are certainly raw (the ladder whitens them); in ``info[<key>]`` and ``self.<key>``."""
        from . import _capi
        from .evidence import HipBackend
        backend = backend or HipBackend()
        kmax = max(2, int(kmax))
        nd = effective_ndim(ndim, self.nparam)
        cross = bool(split) or split_rows is not None
        reason = plan(covtype=covtype, split=cross, ndim=nd, nparam=self.nparam, distributed=_distributed(), nrows=self.nrows, jackknife=jackknife,
                      nchains=self.nchains)
        if reason != RESIDENT:
            raise ResidentDecline(reason)
        jspec = jack_spec(jackknife, self.nchains)
        values = dict(information=information, summary=summary, marginals=marginals, contours=contours, covariance=covariance, bounds=bounds)
        names = _post.param_names(self.names_root, nd) if _post.carry(values) else None
        reqs = {k: _post.BY_KEY[k].resolve(values, names, nd, self.names_root) for k in _RESOLVED}
        torch = self._torch
        ms = self.stats["ms"]
        with torch.cuda.device(self.device):
            rows1 = rows2 = None
            if split_rows is not None:
                rows1, rows2 = self._index_list(split_rows[0]), self._index_list(split_rows[1])
            elif split:
                nrow = self.nrows
                pick = _chains.rank0_draw(lambda: np.random.choice(range(nrow), size=int(nrow * s1frac), replace=False))
                rest = np.setxor1d(range(nrow), pick)
                logger.info("%s chain with nrow=%s split to ns1=%s, ns2=%s" % (self.nchains, nrow, len(pick), len(rest)))
                rows1, rows2 = self._index_list(pick), self._index_list(rest)
            t0 = time.perf_counter()
            s1 = self._gather(rows1, want=("params", "w", "like"))
            s2 = self._gather(rows2, want=("params",)) if cross else None
            n1 = int(s1["w"].shape[0])
            n2 = int(s2["params"].shape[0]) if cross else 0
            ms["gather"] = _ms(t0)
            if n1 < 2 or (cross and n2 < 1):
                raise ValueError("invalid sizes n1=%d n2=%d" % (n1, n2))
            t0 = time.perf_counter()
            fs, (logLmax, SumW, nan_like, bad_w) = self._reduce(s1, pos_lnp)
            ms["reduce"] = _ms(t0)
            check_reduced(logLmax, SumW, nan_like, bad_w)
            system = _post.System(s1["params"].data_ptr(), self.nparam, n1, nd, s1["w"].data_ptr(), fs.data_ptr())
            blocks = {}

            def measure(st):
                if reqs[st.key] is not None:
                    t0 = time.perf_counter()
                    blocks[st.key], = st.measure_dev([system], [reqs[st.key]], self.device, self._stream())
                    ms[st.key] = _ms(t0)
            for st in _post.STATS[1:]:                 # (summary, marginals, contours, covariance: before the feed)
                measure(st)
            t0 = time.perf_counter()
            with backend._scoped():
                dotp, jac, _, _ = _capi.evidence_feed_part_dev(s1["params"].data_ptr(), n1, self.nparam, s2["params"].data_ptr() if cross else 0, n2,
                                                               self.nparam, nd, 0 if covtype == "all" else 1, kmax, s1["w"].data_ptr(), fs.data_ptr(),
                                                               0, 1, device=self.device, want_checksum=False)
            ms["feed"] = _ms(t0)
            measure(_post.INFORMATION)
            mom = blocks.get("information")
            jrun = jblock = None
            if jspec is not None:
                t0 = time.perf_counter()
                gq, = jack_groups_dev([(self._src, self._parts, n1, jspec["G"], jspec["by"])], self.device, self._stream())
                jrun = jack_run(s1["params"].data_ptr(), n1, self.nparam, nd, kmax, s1["w"].data_ptr(), fs.data_ptr(), gq, jspec, self.device, backend)
                jblock, = jack_leave_out_dev([(s1["w"].data_ptr(), fs.data_ptr() if mom is not None else 0, gq, n1, jspec["G"])], self.device, self._stream())
                ms["jackknife"] = _ms(t0)
        out = mle_from_sums(dotp, jac, SumW, logLmax, n1, kmax, math.log(priorvolume), cross)[1:]
        for st in _post.STATS:
            setattr(self, st.key, st.build(blocks[st.key], reqs[st.key], names, logLmax, out) if st.key in blocks else None)
        self.jackknife_block = jblock
        self.jackknife = None if jrun is None else jack_result(jrun, jblock, jspec, SumW, logLmax, n1, kmax, math.log(priorvolume))
        if self.jackknife is not None and self.information is not None:
            jack_information(self.information, jblock, logLmax, self.jackknife)
        if not info:
            return out
        inf = route_info(RESIDENT, self.nparam, nd, self.nrows if split_rows is not None else n1, [n1, n2] if cross else [n1])
        if self.thin_corr is not None:
            inf["thin_corr"] = self.thin_corr
        if self.converge is not None:
            inf["converge"] = self.converge
        for key, found in [("information", self.information), ("jackknife", self.jackknife)] + [(st.key, getattr(self, st.key)) for st in _post.STATS[1:]]:
            if found is not None:
                inf[key] = found
        return out, inf


def log_information(inf):
    """the lines of the statistics (information, summary, marginals, contours), before the ln(B) lines"""
    for line in _post.log_lines(inf):
        logger.info(line)


_EVIDENCE_KEYS = ("rand", "info", "profile", "pvolume", "pos_lnp", "nproc", "prewhiten")


def evidence_from_files(root, *, require_resident=False, **kwargs):
    """``MCEvidence(root, **ctor).evidence(**call)`` with the keywords of both in ``kwargs``, through the resident route
    where it applies (``plan``) and through that very expression where it does not.  With ``info=True`` the info dict
    says which: ``info["route"]`` is ``"resident"`` or ``"host"``, and ``info["declined"]`` gives the reason.
    ``require_resident=True`` turns a decline into ``ValueError(reason)``.  ``jackknife`` (None, True, a number of groups or dict(groups,
    by)) puts the delete-a-group error bars in ``info["jackknife"]`` on either route.  Without a GPU: ``RuntimeError``."""
    from . import _capi
    from .evidence import MCEvidence
    _capi.require_device()
    call = {k: kwargs.pop(k) for k in list(kwargs) if k in _EVIDENCE_KEYS}
    ctor = dict(kwargs)
    want_info = bool(call.get("info", False))
    covtype = ctor.get("covtype", "all")               # (given: the call's covtype too; not given: evidence()'s default)
    covtype = "single" if covtype is None else covtype
    split = bool(ctor.get("split", False))
    values = _post.values_of(ctor.get)                 # (the statistics' keywords and bounds)
    _post.check(values, root=root if isinstance(root, str) else None, brange=ctor.get("brange"), nbatch=ctor.get("nbatch", 1), isfunc=ctor.get("isfunc"))
    reason = RESIDENT if _is_file_root(root) else REASONS["not_files"]
    if reason == RESIDENT:
        reason = plan(thinlen=ctor.get("thinlen", 0.0), isfunc=ctor.get("isfunc"), brange=ctor.get("brange"), nbatch=ctor.get("nbatch", 1),
                      verbose=max(ctor.get("verbose", 1), 2 if ctor.get("debug") else 0), covtype=covtype, split=split, ndim=None,
                      distributed=_distributed(), ischain=ctor.get("ischain", True), thin_corr=ctor.get("thin_corr"),
                      converge=ctor.get("converge"), converge_by=ctor.get("converge_by", "auto"), jackknife=ctor.get("jackknife"),
                      **{k: v for k, v in values.items() if k != "information"})
    if reason == RESIDENT:
        level = logging.INFO if ctor.get("verbose", 1) == 1 else logging.WARNING
        if not logging.getLogger().handlers:
            logging.basicConfig()
        logger.setLevel(level)
        rc = None
        try:
            rc = ResidentChains.from_files(root, burnlen=ctor.get("burnlen", 0.0), thinlen=ctor.get("thinlen", 0.0), iw=ctor.get("iw", 0),
                                           ilike=ctor.get("ilike", 1), itheta=ctor.get("itheta", 2), idchain=ctor.get("idchain", 0),
                                           idpattern=ctor.get("idpattern", "_?.txt"), thin_corr=ctor.get("thin_corr"),
                                           corr_min=ctor.get("corr_min", _chains.CORR_MIN), corr_max_lag=ctor.get("corr_max_lag", _chains.CORR_MAX_LAG),
                                           ndim=ctor.get("ndim"), converge=ctor.get("converge"), converge_by=ctor.get("converge_by", "auto"))
            rc.names_root = root if isinstance(root, str) else None
            pv = call.get("pvolume")
            got = rc.evidence(kmax=ctor.get("kmax", 5), ndim=ctor.get("ndim"), priorvolume=ctor.get("priorvolume", 1) if pv is None else pv,
                              covtype=covtype, pos_lnp=call.get("pos_lnp", False), split=split, s1frac=ctor.get("s1frac", 0.5), info=True,
                              backend=ctor.get("backend"), jackknife=ctor.get("jackknife"), **values)
            mle, inf = got
            if ctor.get("verbose", 1) > 0:
                log_information(inf)
                for k in range(1, len(mle) + 1):
                    logger.info("   ln(B)[k={}] = {}".format(k, mle[k - 1]))
            return (mle, inf) if want_info else mle
        except ResidentDecline as d:                     # (nothing half done is kept: the device buffers die with rc)
            reason = d.reason
        finally:
            del rc
    if require_resident:
        raise ValueError(reason)
    m = MCEvidence(root, **ctor)
    if "covtype" in ctor:
        call["covtype"] = ctor["covtype"]
    out = m.evidence(**call)
    if want_info:
        out[1]["route"] = "host"
        out[1]["declined"] = reason
    return out
