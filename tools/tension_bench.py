#!/usr/bin/env python
"""The weighted parameter covariance and the tension statistics next to ln E (``covariance=``, ``tension``; docs/design/tension.md):
what they cost, on one box, in one run.

(a) ``mce_param_cov_dev`` on rows that are already on the device against ``covariance.measure`` (NumPy) on the same rows, at
    1 000 000 x 27, 50 000 x 127, 5 000 x 8, and 24 systems of 27 000 x 8 in one call;
(b) files -> ln E on the resident route with ``covariance=True`` against the same call without it (4 files of 100 000 rows x 27, kmax 4);
(c) the three-root tension call (Planck-shaped roots), the farm against the host route.
Every pair is run once first (which warms it up and checks that the two agree), then timed INTERLEAVED, ``--reps`` repetitions
each, with a device synchronise inside every timed window; medians are reported next to every repetition with their min-max spread.
A tree without the keyword (the parent commit) runs part b without it, for its own spread on the same box; ``--plain-only`` makes
this tree do the same.  One JSON document on stdout (and in --out).

    python tools/tension_bench.py --out profiles/tension/bench.json
    rocprofv3 --kernel-trace --stats -- python tools/tension_bench.py --one 1x1000000x27
"""
import argparse
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

SHAPES = ((1, 1_000_000, 27), (1, 50_000, 127), (1, 5_000, 8), (24, 27_000, 8))


def make_system(n, d, seed):
    rng = np.random.default_rng(seed)
    x = 0.01 * rng.standard_normal(d + 2) + rng.standard_normal((n, d + 2))
    return 1.0 + rng.poisson(3.0, n).astype(np.float64), x


def make_chains(nchains, rows, d, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nchains):
        c = np.empty((rows, d + 2))
        c[:, 0] = 1.0 + rng.poisson(3.0, rows)
        c[:, 2:] = 0.01 * rng.standard_normal(d) + rng.standard_normal((rows, d))
        c[:, 1] = 0.5 * np.sum(c[:, 2:] ** 2, axis=1)
        out.append(c)
    return out


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def device_call(systems, d):
    """-> (a function that runs ONE mce_param_cov_dev call on device copies of the systems, the tensors it needs kept alive, the workspace)"""
    import torch
    from mcevidence_amd import _capi
    keep = [[torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for v in (x, a)] for a, x in systems]
    segs = [(t[0].data_ptr(), int(t[0].shape[1]), int(t[0].shape[0]), d, t[1].data_ptr()) for t in keep]
    wsb = _capi.param_cov_workspace_bytes(sum(s[2] for s in segs), len(segs), d)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: _capi.param_cov_dev(segs, ws.data_ptr(), wsb, st)), (keep, ws), wsb


def interleave(routes, reps, sync):
    t = {k: [] for k, _ in routes}
    for _ in range(reps):
        for k, fn in routes:
            t[k].append(timed(fn, sync)[0])
    out = {}
    for k in t:
        out[k + "_s"] = t[k]
        out[k + "_median_s"] = statistics.median(t[k])
        out[k + "_min_s"], out[k + "_max_s"] = min(t[k]), max(t[k])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--plain-only", action="store_true", help="part b without the keyword only, as a tree without it runs it")
    ap.add_argument("--one", default="", metavar="SYSTEMSxROWSxD", help="one warm-up and five mce_param_cov_dev calls at this shape and nothing else: "
                                                                     "the run a kernel trace is taken of")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    has_keyword = hasattr(_capi, "param_cov_dev") and not args.plain_only      # (the parent commit runs part b without it, for its own spread)
    if has_keyword:
        from mcevidence_amd import covariance, tension
    if args.one:
        if not has_keyword:
            raise SystemExit("--one traces mce_param_cov_dev: this tree has no such call, or --plain-only was given")
        nsys, n, d = (int(v) for v in args.one.split("x"))
        fn, keep, _ = device_call([make_system(n, d, 10 + k) for k in range(nsys)], d)
        for _ in range(6):
            fn()
        sync()
        return
    doc = dict(tool="tools/tension_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, device_vs_numpy=[])
    parts = args.parts.split(",")
    if "a" in parts and has_keyword:
        for nsys, n, d in SHAPES:
            systems = [make_system(n, d, 10 + k) for k in range(nsys)]
            fn, keep, wsb = device_call(systems, d)
            host = lambda: [covariance.measure(a, x[:, :d]) for a, x in systems]
            dev, hst = [covariance.from_block(b, d) for b in fn()], host()
            for u, v in zip(dev, hst):
                if not (np.allclose(u["mean"], v["mean"], rtol=0, atol=1e-12) and np.allclose(u["cov"], v["cov"], rtol=0, atol=1e-11) and u["status"] == 0):
                    raise SystemExit("%d x %d x %d: device and NumPy disagree" % (nsys, n, d))
            row = dict(systems=nsys, rows=n, d=d, workspace_bytes=wsb, **interleave([("device", fn), ("numpy", host)], args.reps, sync))
            row["numpy_over_device"] = row["numpy_median_s"] / row["device_median_s"]
            doc["device_vs_numpy"].append(row)
            print("%d x %d x %d: device %.3f ms, NumPy %.3f ms (x%.2f)" % (nsys, n, d, 1e3 * row["device_median_s"], 1e3 * row["numpy_median_s"],
                                                                          row["numpy_over_device"]), file=sys.stderr)
            del keep, fn
    with tempfile.TemporaryDirectory() as tmp:
        if "b" in parts:
            root = os.path.join(tmp, "c3")
            write_cosmomc_chains(root, make_chains(4, 100_000, 27, seed=2), None)
            kw = dict(kmax=4, verbose=0, info=True, require_resident=True)
            without = lambda: pkg.evidence_from_files(root, **kw)
            routes = [("plain", without)]
            if has_keyword:
                with_ = lambda: pkg.evidence_from_files(root, covariance=True, **kw)
                a, b = with_(), without()
                if not np.array_equal(a[0], b[0]):
                    raise SystemExit("resident: ln E changes with covariance=True")
                routes.insert(0, ("covariance", with_))
            else:
                without()
            doc["resident"] = dict(files=4, rows=100_000, ndim=27, **interleave(routes, args.reps, sync))
            if has_keyword:
                doc["resident"]["cost_s"] = doc["resident"]["covariance_median_s"] - doc["resident"]["plain_median_s"]
            print("resident: plain %.4f s" % doc["resident"]["plain_median_s"], file=sys.stderr)
        if "c" in parts and has_keyword:
            roots = []
            for k in range(3):
                roots.append(os.path.join(tmp, "t%d" % k))
                write_cosmomc_chains(roots[-1], planck_like_chains(seed=100 + k)[0], None)
            nd = 6                                         # (without .paramnames files: the six leading columns are shared)
            farm = lambda: tension.evidence_tension(*roots, shared=nd, kmax=4)
            host = lambda: tension.evidence_tension(*roots, shared=nd, kmax=4, route="host")
            f, h = farm(), host()
            if not (np.allclose(f[3]["tension"]["lnR"], h[3]["tension"]["lnR"], rtol=0, atol=1e-8) and
                    abs(f[3]["tension"]["shift"]["chi2"] - h[3]["tension"]["shift"]["chi2"]) <= 1e-9 * abs(h[3]["tension"]["shift"]["chi2"])):
                raise SystemExit("tension: the farm and the host route disagree")
            doc["tension"] = dict(roots=3, **interleave([("farm", farm), ("host", host)], args.reps, sync))
            doc["tension"]["host_over_farm"] = doc["tension"]["host_median_s"] / doc["tension"]["farm_median_s"]
            print("tension: farm %.4f s, host %.4f s" % (doc["tension"]["farm_median_s"], doc["tension"]["host_median_s"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
