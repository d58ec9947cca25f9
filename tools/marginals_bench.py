#!/usr/bin/env python
"""1-D marginal densities, modes and HPD regions next to ln E (``marginals=``; docs/design/marginals.md): what they cost, on one box, in
one run.

(a) ``mce_param_marginals_dev`` on rows that are already on the device against ``marginals.measure`` (NumPy) on the same rows, at
    1 000 000 x 27, 200 000 x 8, 5 000 x 8, and 24 systems of 27 000 x 8 in one call, 512 grid points.  Where a shape has more than
    ``--numpy-values`` kernel values the NumPy form is timed on the first rows that hold that many and the time is SCALED to all rows
    (the row says so: ``numpy_rows``, ``numpy_scaled``); the two forms are compared on those rows;
(b) files -> ln E on the resident route with ``marginals=True`` against the same call without it (4 files of 100 000 rows x 27, kmax 4);
(c) a farm of 24 Planck-shaped roots with and without the keyword.
Every pair is run once first (which warms it up and checks that the two agree), then timed INTERLEAVED, ``--reps`` repetitions each, with a
device synchronise inside every timed window; medians are reported next to every repetition with their min-max spread.  One JSON
document on stdout (and in --out).

    python tools/marginals_bench.py --out profiles/marginals/bench.json
    rocprofv3 --kernel-trace --stats -- python tools/marginals_bench.py --one 1x1000000x27
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.summary_bench import SHAPES, interleave, make_chains, make_system          # noqa: E402


def device_call(systems, d, spec):
    """-> (a function that runs ONE mce_param_marginals_dev call on device copies of the systems, the tensors it needs kept alive)"""
    import torch
    from mcevidence_amd import _capi
    probs, grid, scale = spec
    keep = [[torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for v in (x, a)] for a, x, _ in systems]
    segs = [(t[0].data_ptr(), int(t[0].shape[1]), int(t[0].shape[0]), d, t[1].data_ptr()) for t in keep]
    wsb = _capi.param_marginals_workspace_bytes(sum(s[2] for s in segs), len(segs), d, len(probs), grid)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: _capi.param_marginals_dev(segs, probs, grid, scale, ws.data_ptr(), wsb, st)), (keep, ws), wsb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--farm-roots", type=int, default=24)
    ap.add_argument("--numpy-values", type=float, default=5e7, help="kernel values the NumPy form is timed on at most (a shape with more: on a row subsample, scaled)")
    ap.add_argument("--one", default="", metavar="SYSTEMSxROWSxD", help="one warm-up and five mce_param_marginals_dev calls at this shape and nothing "
                                                                     "else: the run a kernel trace is taken of")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi, marginals
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    spec = (marginals.DEFAULT_PROBS, args.grid, 1.0)
    if args.one:
        nsys, n, d = (int(v) for v in args.one.split("x"))
        fn, keep, _ = device_call([make_system(n, d, 10 + k) for k in range(nsys)], d, spec)
        for _ in range(6):
            fn()
        sync()
        return
    doc = dict(tool="tools/marginals_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, grid=args.grid,
               device_vs_numpy=[])
    parts = args.parts.split(",")
    if "a" in parts:
        for nsys, n, d in SHAPES:
            systems = [make_system(n, d, 10 + k) for k in range(nsys)]
            fn, keep, wsb = device_call(systems, d, spec)
            rows = int(min(n, max(1000, args.numpy_values // (nsys * d * args.grid))))
            host = lambda: [marginals.measure(a[:rows], x[:rows, :d], *spec) for a, x, _ in systems]
            # the two forms agree on the rows the NumPy form is timed on (the tests hold them to the derived bound; here: nine digits)
            sub, _, _ = device_call([(a[:rows], x[:rows], f[:rows]) for a, x, f in systems], d, spec)
            for b, v in zip(sub(), host()):
                u = marginals.from_block(b, d, len(spec[0]), args.grid)
                if not (np.allclose(u["density"], v["density"], rtol=1e-9, atol=1e-300) and np.array_equal(u["pieces"], v["pieces"])):
                    raise SystemExit("%d x %d x %d: device and NumPy disagree" % (nsys, n, d))
            del sub
            row = dict(systems=nsys, rows=n, d=d, grid=args.grid, kernel_values=float(nsys) * n * d * args.grid, workspace_bytes=wsb, numpy_rows=rows,
                       numpy_scaled=rows < n, **interleave([("device", fn), ("numpy", host)], args.reps, sync))
            scale = n / float(rows)
            for k in ("numpy_median_s", "numpy_min_s", "numpy_max_s"):
                row[k.replace("numpy_", "numpy_all_rows_")] = row[k] * scale
            row["numpy_over_device"] = row["numpy_all_rows_median_s"] / row["device_median_s"]
            row["device_values_per_s"] = row["kernel_values"] / row["device_median_s"]
            doc["device_vs_numpy"].append(row)
            print("%d x %d x %d: device %.3f ms (%.3g kernel values / s), NumPy %.3f ms%s (x%.1f)" % (
                nsys, n, d, 1e3 * row["device_median_s"], row["device_values_per_s"], 1e3 * row["numpy_all_rows_median_s"],
                " scaled from %d rows" % rows if rows < n else "", row["numpy_over_device"]), file=sys.stderr)
            del keep, fn
    with tempfile.TemporaryDirectory() as tmp:
        if "b" in parts:
            root = os.path.join(tmp, "c3")
            write_cosmomc_chains(root, make_chains(4, 100_000, 27, seed=2), None)
            kw = dict(kmax=4, verbose=0, info=True, require_resident=True)
            without = lambda: pkg.evidence_from_files(root, **kw)
            with_ = lambda: pkg.evidence_from_files(root, marginals={"grid": args.grid}, **kw)
            a, b = with_(), without()
            if not np.array_equal(a[0], b[0]):
                raise SystemExit("resident: ln E changes with marginals=True")
            doc["resident"] = dict(files=4, rows=100_000, ndim=27, **interleave([("marginals", with_), ("plain", without)], args.reps, sync))
            doc["resident"]["cost_s"] = doc["resident"]["marginals_median_s"] - doc["resident"]["plain_median_s"]
            print("resident: plain %.4f s, with marginals %.4f s" % (doc["resident"]["plain_median_s"], doc["resident"]["marginals_median_s"]), file=sys.stderr)
        if "c" in parts:
            roots = []
            for k in range(args.farm_roots):
                roots.append(os.path.join(tmp, "p%02d" % k))
                write_cosmomc_chains(roots[-1], planck_like_chains(seed=100 + k)[0], None)
            without = lambda: pkg.evidence_many_from_files(roots, kmax=4, info=True)
            with_ = lambda: pkg.evidence_many_from_files(roots, marginals={"grid": args.grid}, kmax=4, info=True)
            a, b = with_(), without()
            if not all(np.array_equal(x[0], y[0]) for x, y in zip(a, b)):
                raise SystemExit("farm: ln E changes with marginals=True")
            doc["farm"] = dict(roots=len(roots), **interleave([("marginals", with_), ("plain", without)], args.reps, sync))
            doc["farm"]["cost_s"] = doc["farm"]["marginals_median_s"] - doc["farm"]["plain_median_s"]
            print("farm of %d: plain %.4f s, with marginals %.4f s" % (len(roots), doc["farm"]["plain_median_s"], doc["farm"]["marginals_median_s"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
