#!/usr/bin/env python
"""Convergence batches (nbatch / brange): wall time of ``MCEvidence.evidence()`` by the host loop (one whitening, upload and
search per batch; what every batched call took before ``HipBackend(batch_feed=True)`` existed, and still takes by default) and by
the batch-feed route (``mce_evidence_feed_prefix_f64``: one upload, every batch in one library call), on one box, in one run.

Two shapes, each with covtype 'all' and 'single':
    small   gaussian_chain 100 000 x 8,    kmax = 2,  nbatch = 10, brange = [3, 5]
    large   gaussian_chain 1 000 000 x 27, kmax = 10, nbatch = 8,  brange = [4, 6]
The routes are checked against each other first (|d ln E| <= 1e-9, which also warms both up), then timed INTERLEAVED, `--reps`
repetitions each; every window ends when ``evidence()`` returns, which is after the library's last device synchronise.  Reports
every repetition, medians, the CPU count and mce_source_hash().  One JSON document on stdout (and in --out).

    python tools/batch_feed_bench.py --out profiles/batch_feed/bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LNE_PARITY = 1e-9
SHAPES = {
    "small": dict(n=100_000, d=8, kmax=2, nbatch=10, brange=[3.0, 5.0]),
    "large": dict(n=1_000_000, d=27, kmax=10, nbatch=8, brange=[4.0, 6.0]),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=0, help="override the rows of every shape (rehearsals)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import mcevidence_amd as pkg
    from mcevidence_amd import _capi
    from mcevidence_amd.synth import gaussian_chain
    _capi.require_device()          # a measurement without a GPU is no measurement

    doc = dict(tool="tools/batch_feed_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, cases=[])
    for name in args.shapes.split(","):
        sh = dict(SHAPES[name])
        if args.rows:
            sh["n"] = args.rows
            sh["brange"] = [sh["brange"][0] - 2.0, float(np.log10(args.rows))]
        chain = gaussian_chain(seed=1, n=sh["n"], d=sh["d"])

        def make(batch_feed):
            return pkg.MCEvidence([chain], kmax=sh["kmax"], verbose=0, nbatch=sh["nbatch"], brange=sh["brange"], bscale="logpower",
                                  backend=pkg.HipBackend(batch_feed=batch_feed))
        host, feed = make(False), make(True)
        for covtype in ("all", "single"):
            a, b = host.evidence(covtype=covtype), feed.evidence(covtype=covtype)
            err = float(np.max(np.abs(a - b)))
            if not err <= LNE_PARITY:
                raise SystemExit("%s %s: the routes disagree, max |d ln E| = %g" % (name, covtype, err))
            t = {"host_loop": [], "batch_feed": []}
            for _ in range(args.reps):
                for key, m in (("host_loop", host), ("batch_feed", feed)):
                    t0 = time.perf_counter()
                    m.evidence(covtype=covtype)
                    t[key].append(time.perf_counter() - t0)
            case = dict(shape=name, covtype=covtype, **sh, sizes=[int(x[0]) for x in host.nchain], max_abs_dlnE=err,
                        host_loop_s=t["host_loop"], batch_feed_s=t["batch_feed"],
                        host_loop_median_s=statistics.median(t["host_loop"]), batch_feed_median_s=statistics.median(t["batch_feed"]))
            case["speedup"] = case["host_loop_median_s"] / case["batch_feed_median_s"]
            doc["cases"].append(case)
            print("%-5s %-6s host loop %.4f s   batch feed %.4f s   x%.2f   max|dlnE| %.2e" % (
                name, covtype, case["host_loop_median_s"], case["batch_feed_median_s"], case["speedup"], err), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
