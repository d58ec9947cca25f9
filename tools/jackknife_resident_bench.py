#!/usr/bin/env python
"""Jackknife error bars on the resident route and the farm (``jackknife=``; docs/design/jackknife_resident.md): what they cost, on one
box, in one run.

(a) files -> ln E +- sigma: ``evidence_from_files(root, jackknife=16)`` on the resident route against ``MCEvidence(root,
    jackknife=16).evidence()`` on the host route, and the resident call without the keyword (4 files of 250 000 rows x 27);
(b) a farm of 24 Planck-shaped roots with and without the keyword, and the 24 per-root resident calls with it (what the batched
    group and leave-out calls are set against).
Every set is run once first (which warms it up and checks that ln E keeps its bits), then timed INTERLEAVED, ``--reps`` repetitions
each, with a device synchronise inside every timed window; medians are reported next to every repetition with their min-max spread.
On a build without the keyword (the parent commit) only the calls without it are timed, for their spread on the same box.  The chain
files are written once into ``--workdir`` and reused by a second run.  One JSON document on stdout (and in --out).

    python tools/jackknife_resident_bench.py --out profiles/jackknife_resident/bench.json
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

WRITERS = 8


def _write_chain(args):
    path, rows, d, seed = args
    if os.path.exists(path):
        return path
    rng = np.random.default_rng(seed)
    c = np.empty((rows, d + 2))
    c[:, 0] = 1.0 + rng.poisson(3.0, rows)
    c[:, 2:] = 0.01 * rng.standard_normal(d) + rng.standard_normal((rows, d))
    c[:, 1] = 0.5 * np.sum(c[:, 2:] ** 2, axis=1)
    np.savetxt(path + ".part", c, fmt="%.10e")
    os.replace(path + ".part", path)
    return path


def _write_farm_root(args):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    root, seed = args
    if not os.path.exists(root + "_4.txt"):
        write_cosmomc_chains(root, planck_like_chains(seed=seed)[0], None)
    return root


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def interleave(routes, reps, sync):
    """the routes in turn, ``reps`` times; then the call without the keyword ``reps`` times on its own (``plain_alone``: what the
    parent commit's run, which has no other route to interleave with, is set against)"""
    t = {k: [] for k, _ in routes}
    for _ in range(reps):
        for k, fn in routes:
            t[k].append(timed(fn, sync)[0])
    if len(routes) > 1:
        t["plain_alone"] = [timed(dict(routes)["plain"], sync)[0] for _ in range(reps)]
    out = {}
    for k in t:
        out[k + "_s"] = t[k]
        out[k + "_median_s"] = statistics.median(t[k])
        out[k + "_min_s"], out[k + "_max_s"] = min(t[k]), max(t[k])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--rows", type=int, default=250_000)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--ndim", type=int, default=27)
    ap.add_argument("--kmax", type=int, default=4)
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--farm-roots", type=int, default=24)
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    parts = args.parts.split(",")
    G = args.groups
    with tempfile.TemporaryDirectory() as tmp:
        # the chain files first, by worker processes that never see the device
        work = args.workdir or tmp
        os.makedirs(work, exist_ok=True)
        root = os.path.join(work, "c3")
        roots = [os.path.join(work, "p%02d" % k) for k in range(args.farm_roots)]
        with ProcessPoolExecutor(max_workers=WRITERS) as pool:
            if "a" in parts:
                list(pool.map(_write_chain, [("%s_%d.txt" % (root, i + 1), args.rows, args.ndim, 7 + i) for i in range(args.files)]))
            if "b" in parts:
                list(pool.map(_write_farm_root, [(r, 100 + k) for k, r in enumerate(roots)]))

        import torch
        import mcevidence_amd as pkg
        from mcevidence_amd import _capi, resident
        _capi.require_device()          # a measurement without a GPU is no measurement
        sync = torch.cuda.synchronize
        has_keyword = "jackknife" in inspect.signature(resident.plan).parameters      # (the parent commit times the calls without it)
        doc = dict(tool="tools/jackknife_resident_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps,
                   kmax=args.kmax, groups=args.groups, has_keyword=has_keyword)
        if "a" in parts:
            kw = dict(kmax=args.kmax, verbose=0, info=True, require_resident=True)
            plain = lambda: pkg.evidence_from_files(root, **kw)
            routes = [("plain", plain)]
            base = plain()
            if has_keyword:
                res = lambda: pkg.evidence_from_files(root, jackknife=G, **kw)
                host = lambda: pkg.MCEvidence(root, kmax=args.kmax, verbose=0, jackknife=G).evidence(info=True)
                a, h = res(), host()
                if not np.array_equal(a[0], base[0]):
                    raise SystemExit("resident: ln E changes with jackknife=%d" % G)
                ja, jh = a[1]["jackknife"], h[1]["jackknife"]
                diff = float(np.max(np.abs(ja["lnE_groups"] - jh["lnE_groups"])))
                if not diff <= 1e-9 or ja["rows_per_level"] != jh["rows_per_level"]:
                    raise SystemExit("resident and host route disagree: %r, %r against %r" % (diff, ja["rows_per_level"], jh["rows_per_level"]))
                routes = [("resident_jackknife", res), ("host_jackknife", host), ("plain", plain)]
            doc["resident"] = dict(files=args.files, rows=args.rows, ndim=args.ndim, lnE=[float(x) for x in base[0]], **interleave(routes, args.reps, sync))
            if has_keyword:
                r = doc["resident"]
                r.update(sigma=[float(x) for x in ja["sigma"]], rows_per_level={str(k): v for k, v in ja["rows_per_level"].items()},
                         max_abs_diff_lnE_groups=diff, host_over_resident=r["host_jackknife_median_s"] / r["resident_jackknife_median_s"],
                         cost_s=r["resident_jackknife_median_s"] - r["plain_median_s"])
                rc = resident.ResidentChains.from_files(root)
                rc.evidence(kmax=args.kmax, jackknife=G)
                r["stage_ms"] = {k: float(v) for k, v in rc.stats["ms"].items()}
                del rc
            print("resident: plain %.4f s" % doc["resident"]["plain_median_s"], file=sys.stderr)
        if "b" in parts:
            kw = dict(kmax=args.kmax, info=True)
            plain = lambda: pkg.evidence_many_from_files(roots, **kw)
            routes = [("plain", plain)]
            base = plain()
            if has_keyword:
                farm = lambda: pkg.evidence_many_from_files(roots, jackknife=G, **kw)
                each = lambda: [pkg.evidence_from_files(r, jackknife=G, verbose=0, require_resident=True, **kw) for r in roots]
                a, e = farm(), each()
                if not all(np.array_equal(x[0], y[0]) for x, y in zip(a, base)):
                    raise SystemExit("farm: ln E changes with jackknife=%d" % G)
                if not all(np.array_equal(x[1]["jackknife"]["lnE_groups"], y[1]["jackknife"]["lnE_groups"]) for x, y in zip(a, e)):
                    raise SystemExit("farm: a root's jackknife differs from its per-root resident run")
                routes = [("farm_jackknife", farm), ("per_root_jackknife", each), ("plain", plain)]
            doc["farm"] = dict(roots=len(roots), **interleave(routes, args.reps, sync))
            if has_keyword:
                doc["farm"]["cost_s"] = doc["farm"]["farm_jackknife_median_s"] - doc["farm"]["plain_median_s"]
                doc["farm"]["cost_per_root_s"] = doc["farm"]["cost_s"] / len(roots)
            print("farm of %d: plain %.4f s" % (len(roots), doc["farm"]["plain_median_s"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
