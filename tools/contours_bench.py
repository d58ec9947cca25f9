#!/usr/bin/env python
"""2-D joint densities, modes and credible levels next to ln E (``contours=``; docs/design/contours.md): what they cost, on one box, in
one run.

``mce_param_contours_dev`` on rows that are already on the device against ``contours.measure`` (NumPy) on the same rows, at
1 x 1 000 000 x 27 with all 351 pairs, 1 x 200 000 x 8, 1 x 1 000 000 with two columns, and 24 systems of 27 000 x 8 in one call, 64 x 64
cells.  Where a shape has more than ``--numpy-flops`` multiply-adds the NumPy form is timed on the first rows that hold that many and the
time is SCALED to all rows (the row says so: ``numpy_rows``, ``numpy_scaled``); the two forms are compared on those rows.  Every pair is
run once first (which warms it up and checks that the two agree), then timed INTERLEAVED, ``--reps`` repetitions each, with a device
synchronise inside every timed window; medians are reported next to every repetition with their min-max spread.  One JSON document on
stdout (and in --out).

    python tools/contours_bench.py --out profiles/contours/bench.json
    rocprofv3 --kernel-trace --stats -- python tools/contours_bench.py --one 1x1000000x27x27
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.summary_bench import interleave, make_system          # noqa: E402

SHAPES = ((1, 1_000_000, 27, 27), (1, 200_000, 8, 8), (1, 1_000_000, 27, 2), (24, 27_000, 8, 8))      # systems, rows, d, chosen columns


def device_call(systems, d, cols, spec):
    """-> (a function that runs ONE mce_param_contours_dev call on device copies of the systems, the tensors it needs kept alive)"""
    import torch
    from mcevidence_amd import _capi
    probs, grid, scale = spec
    keep = [[torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for v in (x, a)] for a, x, _ in systems]
    segs = [(t[0].data_ptr(), int(t[0].shape[1]), int(t[0].shape[0]), d, t[1].data_ptr()) for t in keep]
    wsb = _capi.param_contours_workspace_bytes(sum(s[2] for s in segs), len(segs), d, len(cols), len(probs), grid)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: _capi.param_contours_dev(segs, cols, probs, grid, scale, ws.data_ptr(), wsb, st)), (keep, ws), wsb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--numpy-flops", type=float, default=2e9, help="multiply-adds the NumPy form is timed on at most (a shape with more: on a row subsample, scaled)")
    ap.add_argument("--one", default="", metavar="SYSTEMSxROWSxDxNC", help="one warm-up and five mce_param_contours_dev calls at this shape and nothing else: the "
                                                                         "run a kernel trace is taken of")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from mcevidence_amd import _capi, contours, marginals
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    spec = (marginals.DEFAULT_PROBS, args.grid, 1.0)
    if args.one:
        nsys, n, d, nc = (int(v) for v in args.one.split("x"))
        fn, keep, _ = device_call([make_system(n, d, 10 + k) for k in range(nsys)], d, list(range(nc)), spec)
        for _ in range(6):
            fn()
        sync()
        return
    doc = dict(tool="tools/contours_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, grid=args.grid, device_vs_numpy=[])
    G2 = args.grid * args.grid
    for nsys, n, d, nc in SHAPES:
        cols = list(range(nc))
        P = nc * (nc - 1) // 2
        systems = [make_system(n, d, 10 + k) for k in range(nsys)]
        fn, keep, wsb = device_call(systems, d, cols, spec)
        rows = int(min(n, max(1000, args.numpy_flops // (nsys * P * G2))))
        host = lambda: [contours.measure(a[:rows], x[:rows, :d], cols, *spec) for a, x, _ in systems]
        # the two forms agree on the rows the NumPy form is timed on (the tests hold them to the derived bound; here: nine digits)
        sub, _, _ = device_call([(a[:rows], x[:rows], f[:rows]) for a, x, f in systems], d, cols, spec)
        for b, v in zip(sub(), host()):
            u = contours.from_block(b, nc, len(spec[0]), args.grid)
            if not np.allclose(u["density"], v["density"], rtol=1e-9, atol=1e-300):
                raise SystemExit("%d x %d x %d: device and NumPy disagree" % (nsys, n, d))
        del sub
        row = dict(systems=nsys, rows=n, d=d, nc=nc, pairs=P, grid=args.grid, multiply_adds=float(nsys) * n * P * G2, workspace_bytes=wsb, numpy_rows=rows,
                   numpy_scaled=rows < n, **interleave([("device", fn), ("numpy", host)], args.reps, sync))
        scale = n / float(rows)
        for k in ("numpy_median_s", "numpy_min_s", "numpy_max_s"):
            row[k.replace("numpy_", "numpy_all_rows_")] = row[k] * scale
        row["numpy_over_device"] = row["numpy_all_rows_median_s"] / row["device_median_s"]
        row["device_flops"] = 2.0 * row["multiply_adds"] / row["device_median_s"]
        doc["device_vs_numpy"].append(row)
        print("%d x %d x %d, %d pairs: device %.3f ms (%.3g flop / s in the products), NumPy %.3f ms%s (x%.1f)" % (
            nsys, n, d, P, 1e3 * row["device_median_s"], row["device_flops"], 1e3 * row["numpy_all_rows_median_s"],
            " scaled from %d rows" % rows if rows < n else "", row["numpy_over_device"]), file=sys.stderr)
        del keep, fn
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
