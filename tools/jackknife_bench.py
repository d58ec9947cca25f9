#!/usr/bin/env python
"""Jackknife error bars from one neighbour search (``MCEvidence.evidence_jackknife``; docs/design/jackknife.md): wall time against
plain ``evidence()`` and against the NAIVE jackknife -- the G deleted-group problems through ``mce_evidence_feed_batch_f64`` -- on
one box, in one run.  Only times are compared with the naive form: it whitens every deleted-group problem with its own eigen-system.

Shapes (auto evidence, G = 16):
    large    gaussian_chain 1 000 000 x 27, kmax = 10
    planck   gaussian_chain   100 000 x 6,  kmax = 4
and the first rung of the ladder, 16 against 32 entries at kmax = 10, whole call, on an iid chain and on an AR(1) chain (phi = 0.9) of
every shape of ``--rung-shapes``.  The routes are run once first (which warms them up and checks ln E of the jackknife against ``evidence()``), then
timed INTERLEAVED, ``--reps`` repetitions each, with a device synchronise inside every timed window.  Reports every repetition,
medians, the device time of the ``mce_jack_dotp_dev`` calls per rung, the rows per rung, the CPU count and mce_source_hash().  One
JSON document on stdout (and in --out).

    python tools/jackknife_bench.py --out profiles/jackknife/bench.json
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

LNE_PARITY = 1e-9
GROUPS = 16
SHAPES = {
    "large": dict(n=1_000_000, d=27, kmax=10),
    "planck": dict(n=100_000, d=6, kmax=4),
}


def ar1_chain(seed, n, d, phi):
    """an AR(1) walk with unit stationary variance in the chain layout (weight 1, -ln L of the stationary Gaussian, rows)"""
    rng = np.random.default_rng(seed)
    e = np.sqrt(1.0 - phi * phi) * rng.standard_normal((n, d))
    e[0] = rng.standard_normal(d)
    try:
        from scipy.signal import lfilter
        x = lfilter([1.0], [1.0, -phi], e, axis=0)
    except ImportError:
        x = e.copy()
        for i in range(1, n):
            x[i] += phi * x[i - 1]
    return np.column_stack([np.ones(n), 0.5 * np.einsum("ij,ij->i", x, x), x])


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="planck,large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=0, help="override the rows of every shape (rehearsals)")
    ap.add_argument("--rung-shapes", default="200000x6,1000000x27", help="rows x columns of the first-rung study, comma separated ('' = none)")
    ap.add_argument("--no-naive", action="store_true", help="leave the naive jackknife out")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi, jackknife as jk
    from mcevidence_amd.synth import gaussian_chain
    _capi.require_device()          # a measurement without a GPU is no measurement
    sync = torch.cuda.synchronize

    doc = dict(tool="tools/jackknife_bench.py", source_hash=_capi.source_hash(), cpus=len(os.sched_getaffinity(0)), reps=args.reps, groups=GROUPS,
               cases=[], first_rung=[])
    for name in [s for s in args.shapes.split(",") if s]:
        sh = dict(SHAPES[name])
        if args.rows:
            sh["n"] = args.rows
        chain = gaussian_chain(seed=1, n=sh["n"], d=sh["d"], cov="corr")
        m = pkg.MCEvidence([chain], kmax=sh["kmax"], verbose=0)
        gq = jk.group_ids(m.gd, "s1", GROUPS)
        s1, lnp, w = m.gd.arrays("s1")
        fs = lnp - np.max(lnp)

        def naive():
            problems = []
            for b in range(GROUPS):
                keep = gq != b
                problems.append((np.ascontiguousarray(s1[keep]), None, sh["d"], 0, sh["kmax"], np.ascontiguousarray(w[keep]), np.ascontiguousarray(fs[keep])))
            return _capi.evidence_feed_batch(problems)

        routes = [("evidence", lambda: m.evidence()), ("jackknife", lambda: m.evidence_jackknife(groups=GROUPS))]
        if not args.no_naive:
            routes.append(("naive", naive))
        first = {key: fn() for key, fn in routes}
        err = float(np.max(np.abs(first["jackknife"]["lnE"] - first["evidence"])))
        if not err <= LNE_PARITY:
            raise SystemExit("%s: ln E of the jackknife and of evidence() disagree, max |d ln E| = %g" % (name, err))
        t = {key: [] for key, _ in routes}
        kernel_ms, out = [], first["jackknife"]
        for _ in range(args.reps):
            for key, fn in routes:
                dt, res = timed(fn, sync)
                t[key].append(dt)
                if key == "jackknife":
                    out = res
                    kernel_ms.append(res["kernel_ms"])
        case = dict(shape=name, **sh, max_abs_dlnE=err, lnE=[float(x) for x in out["lnE"]], sigma=[float(x) for x in out["sigma"]],
                    rows_per_level={str(k): v for k, v in out["rows_per_level"].items()}, jack_dotp_ms_per_rung=kernel_ms,
                    jack_dotp_ms_median=[statistics.median(col) for col in zip(*kernel_ms)])
        for key in t:
            case[key + "_s"] = t[key]
            case[key + "_median_s"] = statistics.median(t[key])
        case["jackknife_over_evidence"] = case["jackknife_median_s"] / case["evidence_median_s"]
        if "naive" in t:
            case["naive_over_jackknife"] = case["naive_median_s"] / case["jackknife_median_s"]
        doc["cases"].append(case)
        print("%-7s evidence %.4f s   jackknife %.4f s (x%.2f)   naive %s   rows per rung %s   jack_dotp %s ms" % (
            name, case["evidence_median_s"], case["jackknife_median_s"], case["jackknife_over_evidence"],
            "%.4f s (x%.2f of the jackknife)" % (case["naive_median_s"], case["naive_over_jackknife"]) if "naive" in t else "-",
            case["rows_per_level"], ["%.3f" % x for x in case["jack_dotp_ms_median"]]), file=sys.stderr)
        del chain, m, s1, first

    # ---- the first rung: 16 against 32 entries at kmax = 10 ------------------------------------------------------------------------
    for shape in [x for x in args.rung_shapes.split(",") if x]:
        n, d, kmax = int(shape.split("x")[0]), int(shape.split("x")[1]), 10
        for kind, chain in (("iid", gaussian_chain(seed=2, n=n, d=d, cov="corr")), ("ar1_phi0.9", ar1_chain(3, n, d, 0.9))):
            m = pkg.MCEvidence([chain], kmax=kmax, verbose=0)
            res = {L: jk.evidence_jackknife(m, groups=GROUPS, first=L) for L in (16, 32)}
            err = float(np.max(np.abs(res[16]["lnE_groups"] - res[32]["lnE_groups"])))
            t = {16: [], 32: []}
            for _ in range(args.reps):
                for L in (16, 32):
                    t[L].append(timed(lambda: jk.evidence_jackknife(m, groups=GROUPS, first=L), sync)[0])
            row = dict(chain=kind, n=n, d=d, kmax=kmax, max_abs_dlnE_groups_16_vs_32=err,
                       rows_per_level_16={str(k): v for k, v in res[16]["rows_per_level"].items()},
                       rows_per_level_32={str(k): v for k, v in res[32]["rows_per_level"].items()},
                       first16_s=t[16], first32_s=t[32], first16_median_s=statistics.median(t[16]), first32_median_s=statistics.median(t[32]))
            doc["first_rung"].append(row)
            del m, chain
            print("rung %-11s first 16: %.4f s %s   first 32: %.4f s %s" % (kind, row["first16_median_s"], row["rows_per_level_16"],
                                                                             row["first32_median_s"], row["rows_per_level_32"]), file=sys.stderr)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
