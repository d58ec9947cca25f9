#!/usr/bin/env python
"""The Gelman-Rubin R-1 of chains (``converge=``; docs/design/chain_conv.md): what measuring costs, on one box, in one run.

(a) ``mce_chain_conv_dev`` on chains that are already on the device against ``chains.gelman_rubin`` (NumPy) on the same chains, at
    4 x 250 000 x 27, 4 x 50 000 x 8, 4 x 5 000 x 8 and 2 x 50 000 x 127 (chains x rows x parameters);
(b) files -> ln E on the resident route with ``converge=True`` against the same call without it (4 files of 100 000 rows x 27);
(c) a farm of 24 Planck-shaped roots with and without the keyword.
Every pair is run once first (which warms it up and checks that the two agree), then timed INTERLEAVED, ``--reps`` repetitions
each, with a device synchronise inside every timed window; medians are reported next to every repetition.  One JSON document on
stdout (and in --out).

    python tools/chain_conv_bench.py --out profiles/chain_conv/bench.json

``--one CxRxD`` runs two device calls of that shape and nothing else: the command to put behind a kernel trace
(``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/chain_conv_bench.py --one 2x50000x127``);
``--merge-trace DIR/..._kernel_stats.csv --out FILE`` then adds the trace's per-kernel split to FILE under ``kernel_trace``."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((4, 250_000, 27), (4, 50_000, 8), (4, 5_000, 8), (2, 50_000, 127))


def make_chains(nchains, rows, d, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nchains):
        c = np.empty((rows, d + 2))
        c[:, 0] = 1.0 + rng.poisson(3.0, rows)
        c[:, 1] = rng.random(rows)
        c[:, 2:] = 0.01 * rng.standard_normal(d) + rng.standard_normal((rows, d))
        out.append(c)
    return out


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def device_call(chains, d):
    """-> (a function that runs ONE mce_chain_conv_dev call on device copies of ``chains``, the tensors it needs kept alive)"""
    import torch
    from mcevidence_amd import _capi
    tensors = [torch.from_numpy(c).to("cuda:0") for c in chains]
    segs = [(t.data_ptr(), int(t.shape[0])) for t in tensors]
    wsb = _capi.chain_conv_workspace_bytes(sum(n for _, n in segs), len(segs), 1, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: _capi.chain_conv_dev(segs, [0] * len(segs), 1, chains[0].shape[1], 0, 2, d, ws.data_ptr(), wsb, st)), (tensors, ws)


def interleave(routes, reps, sync):
    t = {k: [] for k, _ in routes}
    for _ in range(reps):
        for k, fn in routes:
            t[k].append(timed(fn, sync)[0])
    out = {}
    for k in t:
        out[k + "_s"] = t[k]
        out[k + "_median_s"] = statistics.median(t[k])
    return out


def merge_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    split = [dict(kernel=r["Name"][:120], calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3, percent=float(r["Percentage"])) for r in rows]
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernel_trace"] = dict(source=os.path.basename(path), note="two calls of --one (the first warms up); rocprofv3 --kernel-trace --stats, a run of its own",
                               kernels=split)
    with open(out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--one", default="")
    ap.add_argument("--merge-trace", default="")
    ap.add_argument("--farm-roots", type=int, default=24)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi, chains as ch
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    if args.one:
        c, r, d = (int(x) for x in args.one.split("x"))
        fn, keep = device_call(make_chains(c, r, d), d)
        fn()
        sync()
        print(float(fn()["r_minus_1"][0]))
        sync()
        return
    doc = dict(tool="tools/chain_conv_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, device_vs_numpy=[])
    parts = args.parts.split(",")
    if "a" in parts:
        for c, r, d in SHAPES:
            chains = make_chains(c, r, d)
            fn, keep = device_call(chains, d)
            host = lambda: ch.gelman_rubin(chains, by="chains")
            a, b = fn(), host()
            if not abs(a["r_minus_1"][0] - b["r_minus_1"]) <= 1e-9 * (1.0 + b["r_minus_1"]):
                raise SystemExit("%dx%dx%d: device %r and NumPy %r disagree" % (c, r, d, a["r_minus_1"][0], b["r_minus_1"]))
            row = dict(chains=c, rows=r, ndim=d, r_minus_1=b["r_minus_1"], **interleave([("device", fn), ("numpy", host)], args.reps, sync))
            row["numpy_over_device"] = row["numpy_median_s"] / row["device_median_s"]
            doc["device_vs_numpy"].append(row)
            print("%d x %d x %d: device %.3f ms, NumPy %.3f ms (x%.1f)" % (c, r, d, 1e3 * row["device_median_s"], 1e3 * row["numpy_median_s"],
                                                                         row["numpy_over_device"]), file=sys.stderr)
            del keep, chains
    with tempfile.TemporaryDirectory() as tmp:
        if "b" in parts:
            root = os.path.join(tmp, "c3")
            write_cosmomc_chains(root, make_chains(4, 100_000, 27, seed=2), None)
            kw = dict(kmax=4, verbose=0, info=True, require_resident=True)
            with_, without = (lambda: pkg.evidence_from_files(root, converge=True, **kw)), (lambda: pkg.evidence_from_files(root, **kw))
            a, b = with_(), without()
            if not np.array_equal(a[0], b[0]):
                raise SystemExit("resident: ln E changes with converge=True")
            doc["resident"] = dict(files=4, rows=100_000, ndim=27, r_minus_1=a[1]["converge"]["r_minus_1"],
                                   **interleave([("converge", with_), ("plain", without)], args.reps, sync))
            doc["resident"]["cost_s"] = doc["resident"]["converge_median_s"] - doc["resident"]["plain_median_s"]
            print("resident: %.4f s with converge, %.4f s without" % (doc["resident"]["converge_median_s"], doc["resident"]["plain_median_s"]), file=sys.stderr)
        if "c" in parts:
            roots = []
            for k in range(args.farm_roots):
                roots.append(os.path.join(tmp, "p%02d" % k))
                write_cosmomc_chains(roots[-1], planck_like_chains(seed=100 + k)[0], None)
            with_, without = (lambda: pkg.evidence_many_from_files(roots, converge=True, kmax=4, info=True)), (lambda: pkg.evidence_many_from_files(roots, kmax=4, info=True))
            a, b = with_(), without()
            if not all(np.array_equal(x[0], y[0]) for x, y in zip(a, b)):
                raise SystemExit("farm: ln E changes with converge=True")
            doc["farm"] = dict(roots=len(roots), r_minus_1_max=max(x[1]["converge"]["r_minus_1"] for x in a),
                               **interleave([("converge", with_), ("plain", without)], args.reps, sync))
            doc["farm"]["cost_s"] = doc["farm"]["converge_median_s"] - doc["farm"]["plain_median_s"]
            print("farm of %d: %.4f s with converge, %.4f s without" % (len(roots), doc["farm"]["converge_median_s"], doc["farm"]["plain_median_s"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
