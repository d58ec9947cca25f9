"""The resident farm: many chain roots -> ln E in batched GPU passes.

The reference's Planck driver runs ``MCEvidence(root).evidence()`` once per (data set, model, chain) over hundreds to thousands
of small roots.  ``evidence_many_from_files(roots, ...)`` serves that pattern without the chains leaving the GPU: the files of
many roots are read into ONE pinned staging buffer, go up in one copy per wave and are parsed in one pass
(``mce_chain_farm_structure`` / ``_parse``: csrc/capi_farm.hpp), the roots that are not thinned are prepared in one set of
launches (``mce_chain_farm_prep_dev``), thinned roots by the per-root calls of ``resident.ResidentChains`` on views of the wave's
buffer, and all of them are fed by one ``mce_evidence_feed_batch_dev_f64`` call per wave.  Opt-in; a root the farm does not cover
takes ``resident.evidence_from_files``.  docs/design/chain_farm.md has the layout, the passes and the error table.
"""
from __future__ import annotations

import ctypes
import logging
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import posterior as _post
from . import resident as _res

logger = logging.getLogger("mcevidence_amd")

__all__ = ["evidence_many_from_files", "farm_waves", "farm_layout", "read_files", "TILE", "DEFAULT_WAVE_BYTES"]

TILE = 4096                                   # csrc/chain_farm.hpp: kTileBytes
DEFAULT_WAVE_BYTES = 64 << 20                 # (docs/design/chain_farm.md: the sweep over 64 / 128 / 256 MiB)
MAX_READERS = 16                              # file reader threads: a fixed bound, never the machine's core count
FARM = "farm"

#: milliseconds per stage of the last call (file read, upload, structure, parse, prep, feed) and its counts
LAST_STATS = {}


def next_offset(off, length):
    """where the file after one of ``length`` bytes at ``off`` starts: at least one byte behind it, on a tile"""
    return (off + length + 1 + TILE - 1) // TILE * TILE


def farm_layout(file_lens):
    """(offsets, wave_bytes) of files of these lengths laid out one after the other (csrc/chain_farm.hpp: next_offset)"""
    offs, at = [], 0
    for n in file_lens:
        offs.append(at)
        at = next_offset(at, int(n))
    return offs, max(at, TILE)


def farm_waves(sizes, wave_bytes):
    """Pack roots of padded sizes ``sizes`` (bytes: ``farm_layout(lengths of the root's files)[1]``) into waves of at most
    ``wave_bytes``: lists of root indices, every root exactly once and in order.  A root larger than a wave is a wave of its own (the
    caller gives it to the per-root route).  A pure function."""
    wave_bytes = int(wave_bytes)
    if wave_bytes < TILE:
        raise ValueError("wave_bytes=%d: at least one tile of %d bytes" % (wave_bytes, TILE))
    waves, cur, used = [], [], 0
    for i, s in enumerate(sizes):
        s = int(s)
        if s < 0:
            raise ValueError("size %d of root %d" % (s, i))
        if cur and used + s > wave_bytes:
            waves.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += s
        if used > wave_bytes:                 # (a single oversized root)
            waves.append(cur)
            cur, used = [], 0
    if cur:
        waves.append(cur)
    return waves


# one reader handle per device, reused by every call (the handle owns its stream, scratch and pinned staging buffer)
_HANDLES = {}


def _handle(device, need_bytes):
    from . import _capi
    got = _HANDLES.get(device)
    if got is not None and got[2] >= need_bytes:
        return got
    if got is not None:
        _capi.chain_farm_destroy(got[0])
        del _HANDLES[device]
    cap = (int(need_bytes) + TILE - 1) // TILE * TILE
    handle, staging = _capi.chain_farm_create(cap, device)
    _HANDLES[device] = (handle, staging, cap)
    return _HANDLES[device]


def release_handles():
    """destroy the cached reader handles (their device scratch and pinned staging buffers)"""
    from . import _capi
    for dev in list(_HANDLES):
        _capi.chain_farm_destroy(_HANDLES.pop(dev)[0])


def handle_stats(device=0):
    """the cached handle's statistics (``_capi.FARM_STATS``) or None"""
    from . import _capi
    got = _HANDLES.get(device)
    return None if got is None else _capi.chain_farm_stats(got[0])


def _read_into(path, view):
    with open(path, "rb", buffering=0) as f:
        at = 0
        while at < len(view):
            n = f.readinto(view[at:])
            if not n:
                break
            at += n
        if at != len(view) or f.read(1):
            raise IOError("%s changed its size while it was read" % path)


def _per_root(value, n, name):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != n:
            raise ValueError("%s: expected %d entries, got %d" % (name, n, len(value)))
        return list(value)
    return [value] * n


# (the rules of posterior.py by the names the statistics' own tests know them by)
_per_root_summary, _per_root_marginals, _per_root_bounds = _post.SUMMARY.per_root, _post.MARGINALS.per_root, _post.per_root_bounds


def _parse_wave(pool, device, wave_bytes, paths, lens, ms):
    """one wave: the files read into the staging buffer, uploaded and parsed -> (the C array of per-file results, the device tensor
    global token k is written to, {path: exception} of the files that could not be read)"""
    import torch
    from . import _capi
    offs, wbytes = farm_layout(lens)
    handle, staging, cap = _handle(device, max(wave_bytes, wbytes))
    buf = memoryview((ctypes.c_char * cap).from_address(staging)).cast("B")
    t0 = time.perf_counter()
    nonempty = [(p, o, ln) for p, o, ln in zip(paths, offs, lens) if ln > 0]
    jobs = [pool.submit(_read_into, p, buf[o:o + ln]) for p, o, ln in nonempty]
    read_err = {}
    for (p, _, _), j in zip(nonempty, jobs):
        try:
            j.result()
        except Exception as e:
            read_err[p] = e
    ms["read"] += _res._ms(t0)
    files, ntok = _capi.chain_farm_structure(handle, offs, lens, wbytes)
    d_out = torch.empty(max(ntok, 1), dtype=torch.float64, device="cuda:%d" % device)     # (between the two steps: the protocol of the header)
    _capi.chain_farm_parse(handle, d_out.data_ptr(), files, len(paths))
    st = _capi.chain_farm_stats(handle)
    ms["upload"] += st["ms_upload"]
    ms["structure"] += st["ms_structure"]
    ms["parse"] += st["ms_parse"] + st["ms_patch"]
    del buf
    return files, d_out, read_err


def _refused(path, f):
    """the exception of a file the device reader refused (``chain_io.refused``)"""
    from . import _capi, chain_io
    return chain_io.refused(path, "ragged lines" if f.status == _capi.FARM_RAGGED else
                           "a field that is not a number at row %d, column %d" % (f.bad_row, f.bad_col))


def read_files(paths, device=0, wave_bytes=None):
    """``[chain_io.loadtxt(p) for p in paths]`` parsed on GPU ``device`` in waves of many files (the farm reader alone): one entry per
    file, the same array bit for bit, or the exception the host reader raises for a file it refuses (a ragged file, a field that is
    not a number) -- that file only."""
    import torch
    from . import _capi, chain_io
    _capi.require_device()
    device = int(device)
    wave_bytes = DEFAULT_WAVE_BYTES if wave_bytes is None else max(TILE, int(wave_bytes) // TILE * TILE)
    paths = list(paths)
    lens = [os.stat(p).st_size for p in paths]
    out = [None] * len(paths)
    ms = dict(read=0.0, upload=0.0, structure=0.0, parse=0.0)
    with torch.cuda.device(device), ThreadPoolExecutor(max_workers=MAX_READERS) as pool:
        for wave in farm_waves([farm_layout([n])[1] for n in lens], wave_bytes):
            files, d_out, read_err = _parse_wave(pool, device, wave_bytes, [paths[i] for i in wave], [lens[i] for i in wave], ms)
            host = d_out.cpu().numpy()
            for k, i in enumerate(wave):
                f = files[k]
                try:
                    if paths[i] in read_err:
                        raise read_err[paths[i]]
                    if f.status != _capi.FARM_OK:
                        raise _refused(paths[i], f)
                    a = host[int(f.tok_base):int(f.tok_base) + int(f.nrows * f.ncols)].reshape(int(f.nrows), int(f.ncols)).copy()
                    out[i] = chain_io._shape_like_numpy(a, 2)
                except Exception as e:
                    out[i] = e
    return out


class _Root(object):
    __slots__ = ("index", "files", "lens", "size", "ndim", "pvol", "burn", "thin", "parts", "ncols", "nrows", "nparam", "nd", "rc", "keep", "system", "scal", "conv", "jack")


def evidence_many_from_files(roots, *, kmax=5, ndim=None, priorvolume=1, burnlen=0, thinlen=0, covtype="all", pos_lnp=False, idchain=0,
                             idpattern="_?.txt", iw=0, ilike=1, itheta=2, device=0, backend=None, info=False, return_exceptions=False,
                             require_resident=False, wave_bytes=None, split=False, thin_corr=None, corr_min=None, corr_max_lag=None, converge=None, converge_by="auto",
                             information=None, jackknife=None, summary=None, covariance=None, marginals=None, contours=None, bounds=None):
    """``[evidence_from_files(root, ...) for root in roots]`` with the files of many roots parsed per wave and the device work of all
    of them in batched calls.  ``ndim``, ``priorvolume``, ``burnlen`` and ``thinlen`` may be sequences, one entry per root.  One result
    per root, in input order, each exactly what ``evidence_from_files(root, ...)`` returns (``MLE[1:]``; with ``info=True`` the same info keys, and
    ``info["route"]`` = ``"farm"``, ``"resident"`` or ``"host"``).

    Roots are packed into waves whose padded text fits ``wave_bytes`` (all files of a root in one wave; a larger root takes the
    per-root resident route).  A root the farm does not cover -- ``split``, a decline of ``resident.plan`` or one found on the device
    -- goes to ``evidence_from_files`` after the farm's work; ``require_resident=True`` makes a decline ``ValueError(reason)``.
    Under an initialised process group the whole call goes to ``evidence_many`` over ``MCEvidence`` objects.  A failing root raises
    what the host route raises for it (the first in input order), or sits in its slot with ``return_exceptions=True``; it never
    changes another root's result.  ``thin_corr`` (one value or one per root; with ``corr_min``, ``corr_max_lag``): such a root is thinned
    by its measured autocorrelation length on the per-root resident route.  ``converge`` (one value or one per root; with
    ``converge_by``): the Gelman-Rubin R-1 of every such root's burned, unthinned chains, in ``info["converge"]`` -- ONE
    ``mce_chain_conv_dev`` call per wave and per (columns, ndim) group covers the unthinned roots of the wave; a thinned or a
    ``thin_corr`` root is measured on its per-root route.  ``jackknife`` (one value or one per root: None, True, a number of groups or dict(groups, by)): the
    delete-a-group error bars of every such root in ``info["jackknife"]``, as ``evidence_from_files(root, jackknife=...)`` returns them --
    the group ids of all asking roots of a wave come from ONE ``mce_jack_groups_dev`` call and their leave-one-group-out blocks from ONE
    ``mce_jack_leave_out_dev`` call; the ladders (whitening, searches, ``mce_jack_dotp_dev``) run root by root after the wave's batched
    feed, and a root whose ladder raises fails alone.  The statistics of posterior.py (docs/design/posterior_stats.md has their values, the
    rule for one value or one entry per root, and who shares a call), each in ``info[<keyword>]`` as ``evidence_from_files`` returns it:
    ``information`` (one value or one per root: None or True).
    ``summary`` (a sequence of bare numbers is ONE value, so ``[(0.9,), (0.5,)]`` and not ``[0.9, 0.5]`` gives two roots one probability each).
    ``marginals`` and ``contours`` (by ``summary``'s rule; a dict is one value).
    ``bounds`` (by the same rule: None, "ranges", a mapping or one (lo, hi) per parameter): the hard prior bounds of the marginals.
    ``covariance`` (one value or one per root: None or True).
    Each is ONE library call per wave, per distinct spec and per form (plain or bounded) over the ready roots that ask, thinned and unthinned
    alike, before the feed; a root whose request does not fit its own parameters fails alone.
    Without a GPU: ``RuntimeError``."""
    from . import _capi
    _capi.require_device()
    roots = list(roots)
    n = len(roots)
    ndims = _per_root(ndim, n, "ndim")
    pvols = _per_root(priorvolume, n, "priorvolume")
    burns = _per_root(burnlen, n, "burnlen")
    thins = _per_root(thinlen, n, "thinlen")
    tcorr = _per_root(thin_corr, n, "thin_corr")
    corr_kw = {k: v for k, v in (("corr_min", corr_min), ("corr_max_lag", corr_max_lag)) if v is not None}
    convs = _per_root(converge, n, "converge")
    conv_kw = [{} if c in (None, False) else {"converge": c, "converge_by": converge_by} for c in convs]
    # one dict of values per root: the statistics' keywords (posterior.py), bounds and jackknife, each spread by its own rule and
    # validated where it always was (a summary value no route takes fails its root alone, in ``plan``)
    given = dict(information=information, jackknife=jackknife, summary=summary, marginals=marginals, bounds=bounds, contours=contours, covariance=covariance)
    rules = dict({st.key: st.per_root for st in _post.STATS}, bounds=_post.per_root_bounds, jackknife=lambda v, m: _per_root(v, m, "jackknife"))
    rnames = [r if isinstance(r, str) else None for r in roots]
    vals = [{} for _ in roots]
    for key, validated in (("information", ()), ("jackknife", ()), ("summary", ()), ("marginals", ("marginals",)), ("bounds", ()),
                           ("contours", ("bounds", "contours")), ("covariance", ("covariance",))):
        for v, x in zip(vals, rules[key](given[key], n)):
            v[key] = x
        for k in validated:
            for v, rname in zip(vals, rnames):
                _post.check(v, root=rname, keys=(k,))
    jack_kw = [{} if v["jackknife"] is None or v["jackknife"] is False else {"jackknife": v["jackknife"]} for v in vals]
    carry = [dict(_post.carry(v), **conv_kw[i], **jack_kw[i]) for i, v in enumerate(vals)]      # (what a root takes with it to another route)
    common = dict(kmax=kmax, idchain=idchain, idpattern=idpattern, iw=iw, ilike=ilike, itheta=itheta)
    if _res._distributed():
        from .evidence import MCEvidence, evidence_many
        extra = dict(common, split=split, verbose=0, **({"backend": backend} if backend else {}))
        objs = [MCEvidence(r, ndim=ndims[i], priorvolume=pvols[i], burnlen=burns[i], thinlen=thins[i], thin_corr=tcorr[i], **corr_kw, **carry[i], **extra)
                for i, r in enumerate(roots)]
        return evidence_many(objs, info=info, covtype=covtype, pos_lnp=pos_lnp)
    import torch
    from .evidence import HipBackend
    backend = backend or HipBackend()
    device = int(device)
    wave_bytes = DEFAULT_WAVE_BYTES if wave_bytes is None else max(TILE, int(wave_bytes) // TILE * TILE)
    kmax_eff = max(2, int(kmax))
    results = [None] * n
    fallback = {}                                  # index -> reason (None: not examined by the farm)
    ms = dict(read=0.0, upload=0.0, structure=0.0, parse=0.0, prep=0.0, feed=0.0)
    counts = dict(roots=n, farm=0, waves=0, files=0, fallback=0)

    def fail(i, exc):
        results[i] = exc

    # ---- planning: pure, per root ----------------------------------------------------------------------------------------------------
    todo = []
    for i, root in enumerate(roots):
        reason = _res.RESIDENT if _res._is_file_root(root) else _res.REASONS["not_files"]
        if reason == _res.RESIDENT and split:
            reason = "split: the random split is drawn per root on the host"
        if reason == _res.RESIDENT:
            try:
                reason = _res.plan(thinlen=thins[i], covtype="single" if covtype is None else covtype, ndim=ndims[i], thin_corr=tcorr[i],
                                   converge=convs[i], converge_by=converge_by, **{k: v for k, v in vals[i].items() if k != "information"})
            except ValueError as e:                # (thin_corr together with thinlen; a converge or jackknife value no route takes)
                fail(i, e)
                continue
        if reason == _res.RESIDENT and _res._chains.thin_corr_scale(tcorr[i]) is not None:
            reason = _res.REASONS["thin_corr"]
        if reason != _res.RESIDENT:
            fallback[i] = reason
            continue
        try:
            r = _Root()
            r.index, r.files = i, _res._resolve_files(root, idchain, idpattern)
            r.lens = [os.stat(p).st_size for p in r.files]
            r.size = farm_layout(r.lens)[1]
            r.ndim, r.pvol, r.burn, r.thin, r.rc, r.keep, r.system, r.scal = ndims[i], pvols[i], burns[i], thins[i], None, None, None, None
            r.conv = _res._chains.converge_spec(convs[i], converge_by)          # None, or (threshold, by); afterwards: info["converge"]
            r.jack = _res.jack_spec(vals[i]["jackknife"], len(r.files))                     # None, or dict(groups, by, G)
            todo.append(r)
        except Exception as e:                     # (no files, an unreadable path, by="chains" of one file: what the host route raises too)
            fail(i, e)
    cov = "single" if covtype is None else covtype

    with torch.cuda.device(device), ThreadPoolExecutor(max_workers=MAX_READERS) as pool:
        dev = "cuda:%d" % device
        stream = torch.cuda.current_stream(device)
        for wave in farm_waves([r.size for r in todo], wave_bytes):
            wroots = [todo[k] for k in wave]
            if len(wroots) == 1 and wroots[0].size > wave_bytes:
                fallback[wroots[0].index] = None   # larger than a wave: the per-root resident route
                continue
            counts["waves"] += 1
            paths = [p for r in wroots for p in r.files]
            lens = [x for r in wroots for x in r.lens]
            files, d_out, read_err = _parse_wave(pool, device, wave_bytes, paths, lens, ms)
            counts["files"] += len(paths)

            # ---- per root: its files' verdicts, burn-in, the decline cases known now -------------------------------------------------
            t0 = time.perf_counter()
            plain, at = [], 0
            for r in wroots:
                ff = [files[at + k] for k in range(len(r.files))]
                fp = r.files
                at += len(fp)
                try:
                    for path, f in zip(fp, ff):
                        if path in read_err:
                            raise read_err[path]
                        if f.status != _capi.FARM_OK:
                            raise _refused(path, f)      # (the host reader's ValueError with the row, column and line of the first bad field)
                    shapes = [(int(f.nrows), int(f.ncols) if f.nrows else 1) for f in ff]       # (np.loadtxt: an empty file is (0, 1))
                    reason = _res.plan(thinlen=r.thin, ncols=[c for _, c in shapes])
                    if reason != _res.RESIDENT:
                        fallback[r.index] = reason
                        continue
                    r.ncols = shapes[0][1]
                    _res.check_columns(iw, ilike, itheta, r.ncols)
                    r.nparam = r.ncols - itheta
                    r.nd = nd = _res.effective_ndim(r.ndim, r.nparam)
                    if r.thin not in (0, 1):
                        # integer or bin thinning: the per-root calls, on views of the wave's buffer
                        tensors = [d_out[int(f.tok_base):int(f.tok_base) + nr * nc].view(nr, nc) if nr else torch.empty((0, 1), dtype=torch.float64, device=dev)
                                   for f, (nr, nc) in zip(ff, shapes)]
                        r.rc = _res.ResidentChains(tensors, r.burn, r.thin, iw, ilike, itheta, device, ndim=r.ndim, **conv_kw[r.index])
                        r.nrows = r.rc.nrows
                        r.conv = r.rc.converge
                    else:
                        r.parts = []
                        for f, (nr, nc) in zip(ff, shapes):
                            start = _res.burn_start(nr, r.burn)
                            r.parts.append((d_out.data_ptr() + (int(f.tok_base) + start * nc) * 8 if nr - start > 0 else 0, nr - start))
                        r.nrows = sum(m for _, m in r.parts)
                    reason = _res.plan(covtype=cov, ndim=nd, nparam=r.nparam, nrows=r.nrows)
                    if reason != _res.RESIDENT:
                        fallback[r.index] = reason
                        r.rc = None
                        continue
                    plain.append(r)
                except _res.ResidentDecline as d:
                    fallback[r.index] = d.reason
                except Exception as e:
                    fail(r.index, e)

            # ---- converge: the unthinned roots of the wave, one call per (columns, ndim) group -----------------------------------------
            groups = {}
            for r in plain:
                if r.rc is None and r.conv is not None:
                    groups.setdefault((r.ncols, r.nd), []).append(r)
            for (nc, nd), members in sorted(groups.items()):
                systems, took = [], []
                for r in members:
                    try:
                        if nd > _res._chains.CONV_MAX_DIM:
                            raise ValueError("converge: ndim=%r (1 .. %d expected)" % (nd, _res._chains.CONV_MAX_DIM))
                        by, segs = _res.conv_device_segments(r.parts, nc, r.conv[1])
                        systems.append(segs)
                        took.append((r, by))
                    except Exception as e:
                        fail(r.index, e)
                        plain.remove(r)
                if not took:
                    continue
                for (r, by), res, segs in zip(took, _res.conv_measure_dev(systems, nc, iw, itheta, nd, device, stream.cuda_stream), systems):
                    try:
                        r.conv = _res._chains.conv_info(res, by, len(segs), r.nrows, r.conv[0])
                    except Exception as e:
                        fail(r.index, e)
                        plain.remove(r)

            # ---- preparation: one set of launches for the unthinned roots, the per-root calls for the thinned ones ---------------
            ready = []
            seg = [r for r in plain if r.rc is None]
            if seg:
                nrows = sum(r.nrows for r in seg)
                parts = [p for r in seg for p in r.parts]
                params = torch.empty(sum(r.nrows * r.nparam for r in seg), dtype=torch.float64, device=dev)
                w = torch.empty(nrows, dtype=torch.float64, device=dev)
                like = torch.empty(nrows, dtype=torch.float64, device=dev)
                fs = torch.empty(nrows, dtype=torch.float64, device=dev)
                wsb = _capi.chain_farm_prep_workspace_bytes(len(seg), len(parts), nrows)
                ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
                scal = _capi.chain_farm_prep_dev([len(r.parts) for r in seg], [r.ncols for r in seg], parts, iw, ilike, itheta, pos_lnp,
                                                 params.data_ptr(), w.data_ptr(), like.data_ptr(), fs.data_ptr(), ws.data_ptr(), wsb, stream.cuda_stream)
                row0 = par0 = 0
                for k, r in enumerate(seg):
                    r.scal = tuple(scal[k])
                    r.keep = (params, w, fs)
                    r.system = _post.System(params.data_ptr() + par0 * 8, r.nparam, r.nrows, r.nd, w.data_ptr() + row0 * 8, fs.data_ptr() + row0 * 8)
                    row0 += r.nrows
                    par0 += r.nrows * r.nparam
            for r in plain:
                try:
                    if r.rc is not None:
                        s1 = r.rc._gather(None, want=("params", "w", "like"))
                        n1 = int(s1["w"].shape[0])
                        fs1, r.scal = r.rc._reduce(s1, pos_lnp)
                        r.keep = (s1, fs1)
                        r.system = _post.System(s1["params"].data_ptr(), r.nparam, n1, r.nd, s1["w"].data_ptr(), fs1.data_ptr())
                    _res.check_reduced(*r.scal)
                    ready.append(r)
                except Exception as e:
                    fail(r.index, e)
            stream.synchronize()
            ms["prep"] += _res._ms(t0)

            # ---- feed: every root of the wave in one library call -----------------------------------------------------------------
            t0 = time.perf_counter()
            if ready:
                # the statistics of the ready roots that ask, thinned and unthinned alike, while the gathered rows are raw (the ladders
                # below whiten them): posterior.measure_wave has the rule for who shares a call and who fails alone
                names = {r.index: _post.param_names(rnames[r.index], r.nd) if _post.carry(vals[r.index]) else None for r in ready}
                found, unfit, _ = _post.measure_wave([_post.Asking(r.index, r.system, vals[r.index], names[r.index], rnames[r.index]) for r in ready],
                                                     device, stream.cuda_stream)
                for i, e in unfit.items():
                    fail(i, e)
                ready = [r for r in ready if r.index not in unfit]
                # jackknife: the group ids of the ready roots that ask for it in one call, their leave-one-group-out blocks in another
                # (src: the kept rows of a thinned root; fs only where the deleted sets' moments are wanted)
                jasked = [r for r in ready if r.jack is not None]
                jgroups, jblocks, pending = {}, {}, []
                if jasked:
                    jgroups = dict(zip((r.index for r in jasked),
                                       _res.jack_groups_dev([(r.rc._src if r.rc is not None else None, r.rc._parts if r.rc is not None else r.parts,
                                                              r.system.rows, r.jack["G"], r.jack["by"]) for r in jasked], device, stream.cuda_stream)))
                    jblocks = dict(zip((r.index for r in jasked),
                                       _res.jack_leave_out_dev([(r.system.w, r.system.fs if "information" in found[r.index] else 0, jgroups[r.index], r.system.rows,
                                                                 r.jack["G"]) for r in jasked], device, stream.cuda_stream)))
                cov_mode = 0 if cov == "all" else 1
                with backend._scoped():
                    got = _capi.evidence_feed_batch_dev([_post.feed_problem(r.system, cov_mode, kmax_eff) for r in ready], device=device, return_exceptions=True)
                    for r, g in zip(ready, got):
                        if isinstance(g, Exception):
                            # (the library words only the first failure of a batch: this problem alone, for its own message)
                            try:
                                y = r.system
                                _capi.evidence_feed_part_dev(y.params, y.rows, y.ld, 0, 0, 0, y.nd, cov_mode, kmax_eff, y.w, y.fs, 0, 1, device=device, want_checksum=False)
                                fail(r.index, g)
                            except Exception as e:
                                fail(r.index, e)
                            continue
                        dotp, jac, _ = g
                        n1 = r.system.rows
                        try:
                            out = _res.mle_from_sums(dotp, jac, r.scal[1], r.scal[0], n1, kmax_eff, math.log(r.pvol), False)[1:]
                        except Exception as e:
                            fail(r.index, e)
                            continue
                        counts["farm"] += 1
                        inf = _res.route_info(FARM, r.nparam, r.nd, n1, [n1])
                        if r.conv is not None:
                            inf["converge"] = r.conv
                        for st in _post.STATS:
                            if st.key in found[r.index]:
                                blk, req = found[r.index][st.key]
                                inf[st.key] = st.build(blk, req, names[r.index], r.scal[0], out)
                        if r.jack is not None:
                            pending.append((r, out, inf))
                            continue
                        results[r.index] = out if not info else (out, inf)
                # the ladders, root by root (a root whose ladder raises -- rows still short after the last rung -- fails alone)
                for r, out, inf in pending:
                    try:
                        y = r.system
                        run = _res.jack_run(y.params, y.rows, y.ld, y.nd, kmax_eff, y.w, y.fs, jgroups[r.index], r.jack, device, backend)
                        inf["jackknife"] = _res.jack_result(run, jblocks[r.index], r.jack, r.scal[1], r.scal[0], y.rows, kmax_eff, math.log(r.pvol))
                        if "information" in inf:
                            _res.jack_information(inf["information"], jblocks[r.index], r.scal[0], inf["jackknife"])
                        results[r.index] = out if not info else (out, inf)
                    except Exception as e:
                        fail(r.index, e)
                        counts["farm"] -= 1
            ms["feed"] += _res._ms(t0)
            for r in wroots:
                r.rc = r.keep = r.parts = None
            del d_out

    # ---- the roots the farm does not cover, after its work ----------------------------------------------------------------------------
    for i in sorted(fallback):
        counts["fallback"] += 1
        try:
            kw = dict(common, ndim=ndims[i], priorvolume=pvols[i], burnlen=burns[i], thinlen=thins[i], pos_lnp=pos_lnp, split=split, info=True, verbose=0)
            if tcorr[i] not in (None, False):
                kw.update(corr_kw, thin_corr=tcorr[i])
            kw.update(carry[i])
            if covtype != "all":
                kw["covtype"] = covtype
            if backend is not None:
                kw["backend"] = backend
            mle, inf = _res.evidence_from_files(roots[i], require_resident=require_resident, **kw)
            results[i] = (mle, inf) if info else mle
        except Exception as e:
            fail(i, e)
    LAST_STATS.clear()
    LAST_STATS.update(ms=ms, counts=counts)
    if not return_exceptions:
        for x in results:
            if isinstance(x, Exception):
                raise x
    return results
