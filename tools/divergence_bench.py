#!/usr/bin/env python
"""The k-NN relative entropy between two chains (``divergence.estimate``; docs/design/knn_divergence.md): wall time of the estimate
on the device against the host route (scikit-learn lists and ``measure``) and against the NAIVE jackknife -- the G + 1 full problems,
every deleted-group pair of chains searched on its own, on the device -- on one box, in one run.

Shapes (K = 4, G = 8):
    small    30 000 x 6 against    30 000 x 6
    large   250 000 x 8 against 1 000 000 x 8     (the host route is left out unless --host-large: scikit-learn's brute search of that
                                                   pair takes minutes)
The routes are run once first (which warms them up and checks the naive values against the one-search values), then timed INTERLEAVED,
``--reps`` repetitions each, with a device synchronise inside every timed window.  Reports every repetition, medians, the device time
of the ``mce_knn_div_terms_dev`` calls per rung, the rows per rung, the CPU count and mce_source_hash().  One JSON document on stdout
(and in --out).  ``--once SHAPE`` runs one device estimate of a shape and nothing else: the program to put behind
``rocprofv3 --kernel-trace --stats --`` for the share of the call the terms kernel takes.

    python tools/divergence_bench.py --out profiles/divergence/bench.json
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

K, GROUPS = 4, 8
SHAPES = {
    "small": dict(nP=30_000, nQ=30_000, d=6),
    "large": dict(nP=250_000, nQ=1_000_000, d=8),
}


def chains(sh, seed=1):
    """P a correlated Gaussian, Q twice as broad and shifted by half a sigma; integer weights 1..4"""
    rng = np.random.default_rng(seed)
    d = sh["d"]
    A = np.tril(0.3 * rng.standard_normal((d, d))) + np.eye(d)
    xp = rng.standard_normal((sh["nP"], d)) @ A.T
    xq = 2.0 * rng.standard_normal((sh["nQ"], d)) @ A.T + 0.5
    return xp, rng.integers(1, 5, sh["nP"]).astype(np.float64), xq, rng.integers(1, 5, sh["nQ"]).astype(np.float64)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-large", action="store_true", help="time the host route on the large shape too")
    ap.add_argument("--no-naive", action="store_true", help="leave the naive jackknife out")
    ap.add_argument("--once", default="", metavar="SHAPE", help="one device estimate of SHAPE and nothing else (for a profiler)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from mcevidence_amd import _capi, divergence as dv
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    dev = torch.device("cuda", 0)

    if args.once:
        data = [torch.from_numpy(v).to(dev) for v in chains(SHAPES[args.once])]
        dv.estimate(*data, kmax=K, groups=GROUPS)          # (warm-up: the profile's second half is the steady call)
        out = dv.estimate(*data, kmax=K, groups=GROUPS)
        print(json.dumps(dict(shape=args.once, D=[float(x) for x in out["D"]], kernel_ms=out["kernel_ms"])))
        return

    doc = dict(tool="tools/divergence_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, groups=GROUPS, K=K,
               cases=[])
    for name in [s for s in args.shapes.split(",") if s]:
        sh = SHAPES[name]
        host = chains(sh)
        data = [torch.from_numpy(v).to(dev) for v in host]
        gP, gQ = torch.from_numpy(dv.group_ids(sh["nP"], GROUPS)).to(dev), torch.from_numpy(dv.group_ids(sh["nQ"], GROUPS)).to(dev)

        def naive():
            vals = [dv.estimate(*data, kmax=K, groups=0)["D"]]
            for b in range(GROUPS):
                kp, kq = gP != b, gQ != b
                vals.append(dv.estimate(data[0][kp], data[1][kp], data[2][kq], data[3][kq], kmax=K, groups=0)["D"])
            return np.array(vals)

        routes = [("device", lambda: dv.estimate(*data, kmax=K, groups=GROUPS))]
        if name != "large" or args.host_large:
            routes.append(("host", lambda: dv.estimate(*host, kmax=K, groups=GROUPS, native=False)))
        if not args.no_naive:
            routes.append(("naive", naive))
        first = {key: fn() for key, fn in routes}
        case = dict(shape=name, **sh, D=[float(x) for x in first["device"]["D"]], sigma=[float(x) for x in first["device"]["sigma"]],
                    rows_per_level={str(k): v for k, v in first["device"]["rows_per_level"].items()})
        if "host" in first:
            case["max_abs_dD_host"] = float(np.max(np.abs(first["host"]["D"] - first["device"]["D"])))
        if "naive" in first:
            # the naive problems whiten every deleted pair with its own metric: only the full value is the same number
            case["abs_dD_full_naive"] = float(np.max(np.abs(first["naive"][0] - first["device"]["D"])))
        t = {key: [] for key, _ in routes}
        kernel_ms = []
        for _ in range(args.reps):
            for key, fn in routes:
                dt, res = timed(fn, sync)
                t[key].append(dt)
                if key == "device":
                    kernel_ms.append(res["kernel_ms"])
        for key in t:
            case[key + "_s"] = t[key]
            case[key + "_median_s"] = statistics.median(t[key])
        case["terms_ms_per_rung"] = kernel_ms
        case["terms_ms_median"] = [statistics.median(col) for col in zip(*kernel_ms)]
        doc["cases"].append(case)
        print("%-6s device %.4f s   host %s   naive %s   rows per rung %s   terms %s ms" % (
            name, case["device_median_s"], "%.4f s" % case["host_median_s"] if "host" in t else "-",
            "%.4f s (x%.2f of the device call)" % (case["naive_median_s"], case["naive_median_s"] / case["device_median_s"]) if "naive" in t else "-",
            case["rows_per_level"], ["%.3f" % x for x in case["terms_ms_median"]]), file=sys.stderr)
        del data, host
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
