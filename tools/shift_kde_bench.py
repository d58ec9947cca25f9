#!/usr/bin/env python
"""The KDE parameter shift (``shift="kde"``, ``--shift-kde``; docs/design/shift_kde.md): what it costs, on one box, in one run.

(a) ``mce_kde_shift_dev`` on whitened-to-be rows that are already on the device, at 10 000, 100 000 and 262 144 rows x d = 2, 6, 12;
(b) ``shift_kde.measure`` (NumPy) on the same rows at 10 000 and 30 000 rows, against the device call;
(c) the three-root tension call through the farm with ``shift="both"`` against the same call without it (the cost of the second read
    of A and B and of the KDE itself), on Planck-shaped roots.
Every route is run once first (which warms it up and checks that the routes agree), then timed INTERLEAVED, ``--reps`` repetitions each,
with a device synchronise inside every timed window; medians are reported next to every repetition.  One JSON document on stdout (and
in --out).

    python tools/shift_kde_bench.py --out profiles/shift_kde/bench.json
    rocprofv3 --kernel-trace --stats -- python tools/shift_kde_bench.py --one 100000x6
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

ROWS = (10_000, 100_000, 262_144)
DIMS = (2, 6, 12)
NUMPY_ROWS = (10_000, 30_000)


def make_system(n, d, seed):
    """a Gaussian difference cloud with weights 1 .. 4, its population whitening and Silverman's c"""
    from mcevidence_amd import shift_kde
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) * np.sqrt(2.0) + 0.5
    w = rng.integers(1, 5, n).astype(np.float64)
    ess = w.sum() ** 2 / np.sum(w * w)
    return x, w, np.eye(d) / np.sqrt(2.0), np.full(d, 0.5), np.zeros(d), 1.0 / (2.0 * shift_kde.bandwidth(d, ess))


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def device_call(system):
    import torch
    from mcevidence_amd import _capi
    x, w, linv, mean, point, c = system
    n, d = x.shape
    keep = [torch.from_numpy(x).to("cuda:0"), torch.from_numpy(w).to("cuda:0")]
    wsb = _capi.kde_shift_workspace_bytes(n, 1, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    seg = [(keep[0].data_ptr(), d, n, d, keep[1].data_ptr(), linv, mean, point, c, 0, 0)]
    return (lambda: _capi.kde_shift_dev(seg, ws.data_ptr(), wsb, st)[0]), (keep, ws), wsb


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
    ap.add_argument("--one", default="", metavar="ROWSxD", help="one warm-up and five mce_kde_shift_dev calls at this shape and nothing else: the run a "
                                                                "kernel trace is taken of")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from mcevidence_amd import _capi, shift_kde, tension
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize
    if args.one:
        n, d = (int(v) for v in args.one.split("x"))
        fn, keep, _ = device_call(make_system(n, d, 7))
        for _ in range(6):
            fn()
        sync()
        return
    doc = dict(tool="tools/shift_kde_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, device=[], numpy=[])
    parts = args.parts.split(",")
    if "a" in parts:
        for n in ROWS:
            for d in DIMS:
                fn, keep, wsb = device_call(make_system(n, d, 7))
                blk = shift_kde.from_block(fn())
                if blk["status"] != 0:
                    raise SystemExit("%d x %d: status %d" % (n, d, blk["status"]))
                row = dict(rows=n, d=d, workspace_bytes=wsb, p=1.0 - blk["M"][0] / blk["W"], n_local=blk["S0"] ** 2 / blk["Q0"], **interleave([("device", fn)], args.reps, sync))
                row["pairs_per_s"] = float(n) * n / row["device_median_s"]
                doc["device"].append(row)
                print("%d x %d: device %.3f ms (%.3g pairs / s)" % (n, d, 1e3 * row["device_median_s"], row["pairs_per_s"]), file=sys.stderr)
                del keep, fn
    if "b" in parts:
        for n in NUMPY_ROWS:
            for d in DIMS:
                system = make_system(n, d, 7)
                fn, keep, _ = device_call(system)
                host = lambda: shift_kde.measure(*system, want_dens=False)       # noqa: E731
                dev, hst = shift_kde.from_block(fn()), host()
                if abs(dev["S0"] - hst["S0"]) > 1e-9 * hst["S0"] or np.max(np.abs(dev["M"] - hst["M"])) > 1e-3 * hst["W"]:
                    raise SystemExit("%d x %d: device and NumPy disagree" % (n, d))
                row = dict(rows=n, d=d, **interleave([("device", fn), ("numpy", host)], args.reps, sync))
                row["numpy_over_device"] = row["numpy_median_s"] / row["device_median_s"]
                doc["numpy"].append(row)
                print("%d x %d: device %.3f ms, NumPy %.1f ms (x%.0f)" % (n, d, 1e3 * row["device_median_s"], 1e3 * row["numpy_median_s"], row["numpy_over_device"]),
                      file=sys.stderr)
                del keep, fn
    if "c" in parts:
        with tempfile.TemporaryDirectory() as tmp:
            roots = []
            for k in range(3):
                roots.append(os.path.join(tmp, "t%d" % k))
                write_cosmomc_chains(roots[-1], planck_like_chains(seed=100 + k)[0], None)
            nd = 6                                         # (without .paramnames files: the six leading columns are shared)
            plain = lambda: tension.evidence_tension(*roots, shared=nd, kmax=4)                                   # noqa: E731
            both = lambda: tension.evidence_tension(*roots, shared=nd, kmax=4, shift="both")                      # noqa: E731
            read = lambda: [tension._farm_rows(r, nd, {}, i) for i, r in enumerate(roots[:2])]                     # noqa: E731
            p, b = plain(), both()
            read()
            if not np.array_equal(p[3]["tension"]["lnR"], b[3]["tension"]["lnR"]) or b[3]["tension"]["shift_kde"]["status"] != 0:
                raise SystemExit("tension: shift='both' moves ln R, or the KDE shift has a status")
            doc["tension"] = dict(roots=3, shift_kde={k: v for k, v in b[3]["tension"]["shift_kde"].items() if k != "names"},
                                  **interleave([("plain", plain), ("both", both), ("second_read", read)], args.reps, sync))
            doc["tension"]["cost_s"] = doc["tension"]["both_median_s"] - doc["tension"]["plain_median_s"]
            print("tension: plain %.4f s, with the KDE shift %.4f s, the second read of A and B alone %.4f s"
                  % (doc["tension"]["plain_median_s"], doc["tension"]["both_median_s"], doc["tension"]["second_read_median_s"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
