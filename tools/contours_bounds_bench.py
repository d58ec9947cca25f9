#!/usr/bin/env python
"""2-D joint densities that honour hard prior bounds (the key ``"bounds"`` of ``contours=``; docs/design/contours_bounds.md): what the
boundary kernel costs next to the call without bounds, on one box, in one process.

``mce_param_contours_bounded_dev`` with every second chosen column bounded below at its smallest sample, INTERLEAVED with
``mce_param_contours_dev`` on the same device rows, at 1 x 1 000 000 x 27 with all 351 pairs, 1 x 200 000 x 8 and 24 systems of
27 000 x 8 in one call, 64 x 64 cells; and the bounded call with every bound open (the first-moment chains are skipped: what a call
costs that asks for bounds and has none).  Every call is run once first (which warms it up and checks that the open pairs of the bounded
call are the plain call's bit for bit), then timed ``--reps`` repetitions each with a device synchronise inside every timed window;
medians are reported next to every repetition with their min-max spread.  One JSON document on stdout (and in --out).  ``MCE_LIB`` picks
the library: the tool is run once per build of the bounded group size (MCE_CONB_JB).

    python tools/contours_bounds_bench.py --out profiles/contours_bounds/bench.json
    rocprofv3 --kernel-trace --stats -- python tools/contours_bounds_bench.py --one 1x1000000x27x27
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

SHAPES = ((1, 1_000_000, 27, 27), (1, 200_000, 8, 8), (24, 27_000, 8, 8))      # systems, rows, d, chosen columns


def device_calls(systems, d, cols, spec, bounds):
    """-> (the plain call, the bounded call with ``bounds`` = [(lo[nc], hi[nc])] per system, the bounded call with every bound open, the
    tensors they need kept alive, the two workspace sizes)"""
    import torch
    from mcevidence_amd import _capi
    probs, grid, scale = spec
    keep = [[torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for v in (x, a)] for a, x, _ in systems]
    segs = [(t[0].data_ptr(), int(t[0].shape[1]), int(t[0].shape[0]), d, t[1].data_ptr()) for t in keep]
    rows = sum(s[2] for s in segs)
    wsb = _capi.param_contours_workspace_bytes(rows, len(segs), d, len(cols), len(probs), grid)
    wsbb = _capi.param_contours_bounded_workspace_bytes(rows, len(segs), d, len(cols), len(probs), grid)
    ws = torch.empty(wsbb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    opened = [(np.full(len(cols), -np.inf), np.full(len(cols), np.inf))] * len(segs)
    return (lambda: _capi.param_contours_dev(segs, cols, probs, grid, scale, ws.data_ptr(), wsb, st),
            lambda: _capi.param_contours_bounded_dev(segs, cols, bounds, probs, grid, scale, ws.data_ptr(), wsbb, st),
            lambda: _capi.param_contours_bounded_dev(segs, cols, opened, probs, grid, scale, ws.data_ptr(), wsbb, st), (keep, ws), (wsb, wsbb))


def every_second_bounded(systems, cols):
    """every second chosen column bounded below at its smallest used sample"""
    out = []
    for a, x, _ in systems:
        lo, hi = np.full(len(cols), -np.inf), np.full(len(cols), np.inf)
        for t in range(1, len(cols), 2):
            lo[t] = float(x[a != 0.0, cols[t]].min())
        out.append((lo, hi))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--one", default="", metavar="SYSTEMSxROWSxDxNC", help="one warm-up and five mce_param_contours_bounded_dev calls at this shape and nothing "
                                                                         "else: the run a kernel trace is taken of")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from mcevidence_amd import _capi, contours, marginals
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    spec = (marginals.DEFAULT_PROBS, args.grid, 1.0)
    if args.one:
        nsys, n, d, nc = (int(v) for v in args.one.split("x"))
        systems = [make_system(n, d, 10 + k) for k in range(nsys)]
        _, fn, _, keep, _ = device_calls(systems, d, list(range(nc)), spec, every_second_bounded(systems, list(range(nc))))
        for _ in range(6):
            fn()
        sync()
        return
    doc = dict(tool="tools/contours_bounds_bench.py", source_hash=_capi.source_hash(), library=os.path.basename(_capi.LIB_PATH), cpus=len(os.sched_getaffinity(0)),
               reps=args.reps, grid=args.grid, bounded_vs_plain=[])
    G2 = args.grid * args.grid
    for nsys, n, d, nc in SHAPES:
        cols = list(range(nc))
        P = nc * (nc - 1) // 2
        systems = [make_system(n, d, 10 + k) for k in range(nsys)]
        bounds = every_second_bounded(systems, cols)
        plain, bounded, opened, keep, (wsb, wsbb) = device_calls(systems, d, cols, spec, bounds)
        # the pairs of two open columns, and the whole call with every bound open, are the plain call's bit for bit
        for b, o, v in zip(bounded(), opened(), plain()):
            u, w, v = (f(blk, nc, len(spec[0]), args.grid) for f, blk in ((contours.from_block_bounded, b), (contours.from_block_bounded, o), (contours.from_block, v)))
            same = [p for p, (s, t) in enumerate(contours.pairs(nc)) if s % 2 == 0 and t % 2 == 0]
            if not (np.array_equal(u["density"][same], v["density"][same]) and np.array_equal(w["density"], v["density"]) and np.array_equal(w["level"], v["level"])):
                raise SystemExit("%d x %d x %d: an open pair differs from the call without bounds" % (nsys, n, d))
        kinds = [(s % 2) + (t % 2) for s, t in contours.pairs(nc)]                      # bounded columns of a pair
        chains = sum(1 + k for k in kinds)                                               # MFMA chains the product phase runs
        row = dict(systems=nsys, rows=n, d=d, nc=nc, pairs=P, pairs_open_open=kinds.count(0), pairs_one_bounded=kinds.count(1), pairs_both_bounded=kinds.count(2),
                   chains_over_plain=chains / float(P), grid=args.grid, multiply_adds_plain=float(nsys) * n * P * G2, workspace_bytes_plain=wsb,
                   workspace_bytes_bounded=wsbb, **interleave([("plain", plain), ("bounded", bounded), ("all_open", opened)], args.reps, sync))
        row["bounded_over_plain"] = row["bounded_median_s"] / row["plain_median_s"]
        row["all_open_over_plain"] = row["all_open_median_s"] / row["plain_median_s"]
        doc["bounded_vs_plain"].append(row)
        print("%d x %d x %d, %d pairs: plain %.3f ms, every second column bounded %.3f ms (x%.2f; %.2f chains per pair), every bound open %.3f ms (x%.2f)" % (
            nsys, n, d, P, 1e3 * row["plain_median_s"], 1e3 * row["bounded_median_s"], row["bounded_over_plain"], row["chains_over_plain"],
            1e3 * row["all_open_median_s"], row["all_open_over_plain"]), file=sys.stderr)
        del keep, plain, bounded, opened
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
