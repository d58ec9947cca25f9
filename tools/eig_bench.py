#!/usr/bin/env python
"""The evidence feed's eigen-solve on the host (``jacobi_eig``, one core) against the batched device solver
(``eig_jacobi_kernel``, one workgroup per system), on one box, in one run:

    solver   ``_capi.eig_sym_batch`` EIG_HOST against EIG_DEVICE at d in {8, 27, 64, 100, 127} x nsys in {1, 300} (graded
             covariances; the device figure includes the upload of the matrices and the download of the results)
    feed     the whole ``_capi.evidence_feed`` call at 100 000 rows, d in {27, 64, 100, 127}: option off (the host solve between two
             waits) against ``eig_mode = EIG_DEVICE`` (one wait)
    batch    ``_capi.evidence_feed_batch`` of 300 Planck-shaped problems (7 000 x 6): off against on

Every pair is checked against each other first (which also warms both up), then timed INTERLEAVED, ``--reps`` repetitions each;
every window ends after a device synchronise (the library's own last one, and an explicit one behind it).  Reports every
repetition, medians, the CPU count and mce_source_hash().  One JSON document on stdout (and in --out).

    python tools/eig_bench.py --out profiles/device_eig/bench.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

C_FEED = 16.0
EPS = float(np.finfo(np.float64).eps)
KMAX = 4


def graded_cov(rng, d):
    """C = diag(s) Cn diag(s), s over 1e-4 .. 1e2, Cn a random correlation matrix with one near-dependence"""
    sig = np.logspace(-4, 2, d)[rng.permutation(d)]
    L = np.eye(d) + 0.8 * rng.standard_normal((d, d)) / math.sqrt(d)
    Cn = L @ L.T
    if d > 1:
        v = rng.standard_normal(d)
        Cn += 50.0 * np.outer(v, v)
    Cn = Cn / np.outer(np.sqrt(np.diag(Cn)), np.sqrt(np.diag(Cn)))
    C = Cn * np.outer(sig, sig)
    return 0.5 * (C + C.T)


def cond_cn(C):
    dg = np.sqrt(np.diag(C))
    ev = np.linalg.eigvalsh(C / np.outer(dg, dg))
    return float(ev[-1] / ev[0])


def chain_rows(rng, n, d):
    z = rng.standard_normal((n, d))
    rows = z @ np.linalg.cholesky(graded_cov(rng, d)).T
    w = rng.integers(1, 6, n).astype(np.float64)
    logl = -0.5 * np.einsum("ij,ij->i", z, z)
    return np.ascontiguousarray(rows), w, logl - logl.max()


def interleaved(fns, reps, sync):
    """fns: name -> callable; every repetition runs each once, in turn; seconds per call"""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append(time.perf_counter() - t0)
    return {k: dict(reps_ms=[1e3 * t for t in v], median_ms=1e3 * statistics.median(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=100_000, help="rows of the whole-call cases (rehearsals: fewer)")
    ap.add_argument("--nprob", type=int, default=300, help="problems of the batch case and systems of the large solver case")
    ap.add_argument("--parts", default="solver,feed,batch")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from mcevidence_amd import _capi
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(7)
    doc = dict(tool="tools/eig_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, solver=[], feed=[], batch=[])
    parts = args.parts.split(",")

    if "solver" in parts:
        for d in (8, 27, 64, 100, 127):
            for nsys in (1, args.nprob):
                C = np.stack([graded_cov(rng, d) for _ in range(nsys)])
                _, _, lam_h, st_h = _capi.eig_sym_batch(C, mode=_capi.EIG_HOST)
                _, _, lam_d, st_d = _capi.eig_sym_batch(C, mode=_capi.EIG_DEVICE)
                assert not st_h[:, 0].any() and not st_d[:, 0].any(), (d, nsys)
                worst = max(float(np.max(np.abs(lam_d[i] - lam_h[i]) / lam_h[i])) / (2.0 * C_FEED * EPS * cond_cn(C[i])) for i in range(nsys))
                assert worst <= 1.0, (d, nsys, worst)
                t = interleaved(dict(host=lambda: _capi.eig_sym_batch(C, mode=_capi.EIG_HOST), device=lambda: _capi.eig_sym_batch(C, mode=_capi.EIG_DEVICE)),
                                args.reps, sync)
                doc["solver"].append(dict(d=d, nsys=nsys, max_sweeps=int(st_d[:, 2].max()), rotations=int(st_d[:, 3].sum()),
                                          worst_share_of_twice_the_bound=worst, **t))
                print("solver d=%d nsys=%d: host %.3f ms, device %.3f ms (sweeps %d)" % (d, nsys, t["host"]["median_ms"], t["device"]["median_ms"],
                                                                                        int(st_d[:, 2].max())), file=sys.stderr)

    def feed(S, w, fs, mode):
        with _capi.options(eig_mode=mode):
            return _capi.evidence_feed(S, None, S.shape[1], 0, KMAX, w, fs)

    if "feed" in parts:
        for d in (27, 64, 100, 127):
            S, w, fs = chain_rows(rng, args.rows, d)
            off, on = feed(S, w, fs, _capi.EIG_HOST), feed(S, w, fs, _capi.EIG_DEVICE)
            stats = _capi.last_eig_stats()
            assert stats["device"] == 1 and stats["host"] == 0, stats
            tol = 2.0 * max(1e-9, d * C_FEED * EPS * cond_cn(np.cov(S.T)))
            diff = float(np.max(np.abs(np.log(on[0][1:]) - np.log(off[0][1:]))))
            assert diff <= tol, (d, diff, tol)
            t = interleaved(dict(off=lambda: feed(S, w, fs, _capi.EIG_HOST), on=lambda: feed(S, w, fs, _capi.EIG_DEVICE)), args.reps, sync)
            doc["feed"].append(dict(rows=args.rows, d=d, kmax=KMAX, max_sweeps=stats["max_sweeps"], rotations=stats["rotations"], ln_dotp_diff=diff,
                                    kernel=_capi.last_kernel(), **t))
            print("feed %d x %d: off %.3f ms, on %.3f ms" % (args.rows, d, t["off"]["median_ms"], t["on"]["median_ms"]), file=sys.stderr)

    if "batch" in parts:
        probs = []
        for _ in range(args.nprob):
            S, w, fs = chain_rows(rng, 7000, 6)
            probs.append((S, None, 6, 0, KMAX, w, fs))

        def batch(mode):
            with _capi.options(eig_mode=mode):
                return _capi.evidence_feed_batch(probs)
        off, on = batch(_capi.EIG_HOST), batch(_capi.EIG_DEVICE)
        stats = _capi.last_eig_stats()
        assert stats["device"] == args.nprob and stats["host"] == 0, stats
        diff = max(float(np.max(np.abs(np.log(a[0][1:]) - np.log(b[0][1:])))) for a, b in zip(on, off))
        assert diff <= 2e-9, diff
        t = interleaved(dict(off=lambda: batch(_capi.EIG_HOST), on=lambda: batch(_capi.EIG_DEVICE)), args.reps, sync)
        doc["batch"].append(dict(problems=args.nprob, rows=7000, d=6, kmax=KMAX, ln_dotp_diff=diff, **t))
        print("batch of %d (7000 x 6): off %.3f ms, on %.3f ms" % (args.nprob, t["off"]["median_ms"], t["on"]["median_ms"]), file=sys.stderr)

    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
