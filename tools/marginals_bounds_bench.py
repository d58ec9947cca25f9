#!/usr/bin/env python
"""Marginals with hard prior bounds (``marginals=`` with ``bounds=``; docs/design/marginals_bounds.md): what the boundary kernel costs
on top of ``mce_param_marginals_dev``, on one box, in one run.

``mce_param_marginals_bounded_dev`` with HALF the columns bounded (every second column: a lower bound at its smallest sample) against
``mce_param_marginals_dev`` on the same device rows, at 1 000 000 x 27, 200 000 x 8, 5 000 x 8, and 24 systems of 27 000 x 8 in one
call, 512 grid points.  Each pair is run once first (which warms it up and checks that the open columns agree bit for bit), then timed
INTERLEAVED in one process, ``--reps`` repetitions each, with a device synchronise inside every timed window; medians are reported
next to every repetition with their min-max spread, and the ratio of the medians.  One JSON document on stdout (and in --out).

    python tools/marginals_bounds_bench.py --out profiles/marginals_bounds/bench.json
    rocprofv3 --kernel-trace --stats -- python tools/marginals_bounds_bench.py --one 1x1000000x27
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.marginals_bench import device_call                                         # noqa: E402
from tools.summary_bench import SHAPES, interleave, make_system                       # noqa: E402


def half_bounds(systems, d):
    """every second column: a lower bound at its smallest sample with a weight; the others open"""
    out = []
    for a, x, _ in systems:
        lo, hi = np.full(d, -np.inf), np.full(d, np.inf)
        lo[1::2] = x[a != 0.0][:, 1:d:2].min(axis=0)
        out.append((lo, hi))
    return out


def bounded_call(systems, d, spec, bounds):
    """-> (a function that runs ONE mce_param_marginals_bounded_dev call on device copies of the systems, what it needs kept alive)"""
    import torch
    from mcevidence_amd import _capi
    probs, grid, scale = spec
    keep = [[torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for v in (x, a)] for a, x, _ in systems]
    segs = [(t[0].data_ptr(), int(t[0].shape[1]), int(t[0].shape[0]), d, t[1].data_ptr()) for t in keep]
    wsb = _capi.param_marginals_bounded_workspace_bytes(sum(s[2] for s in segs), len(segs), d, len(probs), grid)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: _capi.param_marginals_bounded_dev(segs, bounds, probs, grid, scale, ws.data_ptr(), wsb, st)), (keep, ws), wsb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--one", default="", metavar="SYSTEMSxROWSxD", help="one warm-up and five mce_param_marginals_bounded_dev calls at this shape and "
                                                                     "nothing else: the run a kernel trace is taken of")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from mcevidence_amd import _capi, marginals
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    spec = (marginals.DEFAULT_PROBS, args.grid, 1.0)
    if args.one:
        nsys, n, d = (int(v) for v in args.one.split("x"))
        systems = [make_system(n, d, 10 + k) for k in range(nsys)]
        fn, keep, _ = bounded_call(systems, d, spec, half_bounds(systems, d))
        for _ in range(6):
            fn()
        sync()
        return
    doc = dict(tool="tools/marginals_bounds_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, grid=args.grid,
               bounded_vs_plain=[])
    for nsys, n, d in SHAPES:
        systems = [make_system(n, d, 10 + k) for k in range(nsys)]
        bounds = half_bounds(systems, d)
        plain, keep_p, wsb_p = device_call(systems, d, spec)
        bounded, keep_b, wsb_b = bounded_call(systems, d, spec, bounds)
        for b, p in zip(bounded(), plain()):
            u, v = marginals.from_block_bounded(b, d, len(spec[0]), args.grid), marginals.from_block(p, d, len(spec[0]), args.grid)
            if not (np.array_equal(u["density"][0::2], v["density"][0::2]) and np.array_equal(u["upper"][:, 0::2], v["upper"][:, 0::2])):
                raise SystemExit("%d x %d x %d: an open column of the bounded call is not mce_param_marginals_dev's" % (nsys, n, d))
            if d > 1 and not (np.all(u["at_lo"][1::2] == 1.0) and np.all(u["col_status"] == 0.0)):
                raise SystemExit("%d x %d x %d: a bounded column's grid does not end on its bound" % (nsys, n, d))
        row = dict(systems=nsys, rows=n, d=d, grid=args.grid, bounded_columns=int(d // 2), kernel_values=float(nsys) * n * d * args.grid,
                   workspace_bytes=wsb_b, plain_workspace_bytes=wsb_p, **interleave([("bounded", bounded), ("plain", plain)], args.reps, sync))
        row["bounded_over_plain"] = row["bounded_median_s"] / row["plain_median_s"]
        doc["bounded_vs_plain"].append(row)
        print("%d x %d x %d: bounded %.3f ms, plain %.3f ms (x%.3f)" % (nsys, n, d, 1e3 * row["bounded_median_s"], 1e3 * row["plain_median_s"],
                                                                       row["bounded_over_plain"]), file=sys.stderr)
        del keep_p, keep_b, plain, bounded
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
