#!/usr/bin/env python
"""<ln L>_P, D_KL and the model dimensionality next to ln E (``information=``; docs/design/information.md): what they cost, on one
box, in one run.

(a) ``mce_like_moments_dev`` on columns that are already on the device against ``information.moments`` (NumPy) on the same columns,
    at 1 000 000 rows and at 5 000 rows;
(b) files -> ln E on the resident route with ``information=True`` against the same call without it (4 files of 100 000 rows x 27);
(c) a farm of 24 Planck-shaped roots with and without the keyword.
Every pair is run once first (which warms it up and checks that the two agree), then timed INTERLEAVED, ``--reps`` repetitions
each, with a device synchronise inside every timed window; medians are reported next to every repetition, and the min-max spread of
the runs without the keyword (to set against the same figures of the parent commit on the same box).  One JSON document on stdout
(and in --out).

    python tools/information_bench.py --out profiles/information/bench.json
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

SIZES = (1_000_000, 5_000)


def make_columns(n, seed=1):
    rng = np.random.default_rng(seed)
    f = -0.5 * rng.chisquare(27, size=n)
    return 1.0 + rng.poisson(3.0, n).astype(np.float64), f - f.max()


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


def device_call(a, f):
    """-> (a function that runs ONE mce_like_moments_dev call on device copies of the columns, the tensors it needs kept alive)"""
    import torch
    from mcevidence_amd import _capi
    da, df = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(f).to("cuda:0")
    segs = [(df.data_ptr(), da.data_ptr(), int(da.shape[0]))]
    wsb = _capi.like_moments_workspace_bytes(len(a), 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    return (lambda: _capi.like_moments_dev(segs, ws.data_ptr(), wsb, st)), (da, df, ws)


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
    ap.add_argument("--farm-roots", type=int, default=24)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    has_keyword = hasattr(_capi, "like_moments_dev")          # (the parent commit runs parts b and c without it, for its own spread)
    if has_keyword:
        from mcevidence_amd import information
    doc = dict(tool="tools/information_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, device_vs_numpy=[])
    parts = args.parts.split(",")
    if "a" in parts and has_keyword:
        for n in SIZES:
            a, f = make_columns(n)
            fn, keep = device_call(a, f)
            host = lambda: information.moments(a, f)
            d, h = information.from_block(fn()[0]), host()
            if not (abs(d["c"] - h["c"]) <= 1e-9 * abs(h["c"]) and abs(d["v"] - h["v"]) <= 1e-9 * h["v"] and d["W"] == h["W"]):
                raise SystemExit("%d rows: device %r and NumPy %r disagree" % (n, d, h))
            row = dict(rows=n, c=h["c"], v=h["v"], **interleave([("device", fn), ("numpy", host)], args.reps, sync))
            row["numpy_over_device"] = row["numpy_median_s"] / row["device_median_s"]
            doc["device_vs_numpy"].append(row)
            print("%d rows: device %.3f ms, NumPy %.3f ms (x%.1f)" % (n, 1e3 * row["device_median_s"], 1e3 * row["numpy_median_s"], row["numpy_over_device"]),
                  file=sys.stderr)
            del keep
    with tempfile.TemporaryDirectory() as tmp:
        if "b" in parts:
            root = os.path.join(tmp, "c3")
            write_cosmomc_chains(root, make_chains(4, 100_000, 27, seed=2), None)
            kw = dict(kmax=4, verbose=0, info=True, require_resident=True)
            without = lambda: pkg.evidence_from_files(root, **kw)
            routes = [("plain", without)]
            if has_keyword:
                with_ = lambda: pkg.evidence_from_files(root, information=True, **kw)
                a, b = with_(), without()
                if not np.array_equal(a[0], b[0]):
                    raise SystemExit("resident: ln E changes with information=True")
                routes.insert(0, ("information", with_))
            else:
                without()
            doc["resident"] = dict(files=4, rows=100_000, ndim=27, **interleave(routes, args.reps, sync))
            if has_keyword:
                doc["resident"]["bmd"] = a[1]["information"]["bmd"]
                doc["resident"]["cost_s"] = doc["resident"]["information_median_s"] - doc["resident"]["plain_median_s"]
            print("resident: plain %.4f s" % doc["resident"]["plain_median_s"], file=sys.stderr)
        if "c" in parts:
            roots = []
            for k in range(args.farm_roots):
                roots.append(os.path.join(tmp, "p%02d" % k))
                write_cosmomc_chains(roots[-1], planck_like_chains(seed=100 + k)[0], None)
            without = lambda: pkg.evidence_many_from_files(roots, kmax=4, info=True)
            routes = [("plain", without)]
            if has_keyword:
                with_ = lambda: pkg.evidence_many_from_files(roots, information=True, kmax=4, info=True)
                a, b = with_(), without()
                if not all(np.array_equal(x[0], y[0]) for x, y in zip(a, b)):
                    raise SystemExit("farm: ln E changes with information=True")
                routes.insert(0, ("information", with_))
            else:
                without()
            doc["farm"] = dict(roots=len(roots), **interleave(routes, args.reps, sync))
            if has_keyword:
                doc["farm"]["cost_s"] = doc["farm"]["information_median_s"] - doc["farm"]["plain_median_s"]
            print("farm of %d: plain %.4f s" % (len(roots), doc["farm"]["plain_median_s"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
