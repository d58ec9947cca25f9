#!/usr/bin/env python
"""File -> array: the host chain reader (chain_io.loadtxt, libmcechains.so) against the device reader (chain_io.loadtxt_device,
MCE_CHAIN_READER=hip) on one box, in one run.

Writes a C3-sized root once (1 M rows x 29 columns in 4 files, %.10e) and one 1 M x 29 %.17g file, reads everything once to warm
the page cache, then times the two readers INTERLEAVED (boxes differ by a few per cent: never compare across runs), `--reps`
repetitions each, and reports medians, the device phases from the reader's own stats (upload, structure, parse, download) and the
whole `MCEvidence(root).evidence()` under both readers.  One JSON document on stdout (and in --out).

    python tools/chain_reader_bench.py --dir /tmp/crb --out profiles/r07_chain_reader/bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _write_part(args):
    path, seed, part, nparts, rows, fmt = args
    from mcevidence_amd.synth import config_chain
    chain, _ = config_chain("C3", n=rows)
    lo, hi = rows * part // nparts, rows * (part + 1) // nparts
    np.savetxt(path, chain[lo:hi], fmt=fmt)
    return path


def write_files(workdir, rows, nfiles):
    """the root's files and the %.17g file, formatted by worker processes (started before this process touches the GPU)"""
    root = os.path.join(workdir, "c3")
    jobs = [("%s_%d.txt" % (root, i + 1), 3, i, nfiles, rows, "%.10e") for i in range(nfiles)]
    g17 = [(os.path.join(workdir, "g17_%d.part" % i), 3, i, nfiles, rows, "%.17g") for i in range(nfiles)]
    with ProcessPoolExecutor(max_workers=min(2 * nfiles, 8)) as pool:
        done = list(pool.map(_write_part, jobs + g17))
    one = os.path.join(workdir, "g17.txt")
    with open(one, "wb") as out:
        for p in done[nfiles:]:
            with open(p, "rb") as f:
                out.write(f.read())
            os.remove(p)
    return root, done[:nfiles], one


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True, help="scratch directory for the text files (about 1.1 GB)")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="threads of the host reader (per file)")
    ap.add_argument("--kmax", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    t_w, (root, files, g17) = timed(lambda: write_files(a.dir, a.rows, a.files))

    from mcevidence_amd import _capi, chain_io
    import mcevidence_amd as pkg
    _capi.require_device()
    res = dict(rows=a.rows, files=a.files, reps=a.reps, host_threads=a.threads, cpus_allowed=len(os.sched_getaffinity(0)), cpus_box=os.cpu_count(),
               source_hash=_capi.source_hash(), write_s=round(t_w, 2), root_bytes=sum(os.path.getsize(f) for f in files), g17_bytes=os.path.getsize(g17))

    def host_root():
        return [chain_io.loadtxt(f, nthreads=a.threads) for f in files]

    def dev_root():
        return [chain_io.loadtxt_device(f, return_stats=True) for f in files]

    # warm: page cache, library, device context -- and the two readers must agree before anything is timed
    h, d = host_root(), dev_root()
    assert all(np.array_equal(x.view(np.uint64), y[0].view(np.uint64)) for x, y in zip(h, d)), "the readers disagree"
    hg, (dg, _) = chain_io.loadtxt(g17, nthreads=a.threads), chain_io.loadtxt_device(g17, return_stats=True)
    assert np.array_equal(hg.view(np.uint64), dg.view(np.uint64)), "the readers disagree on the %.17g file"
    del h, d, hg, dg

    t_host, t_dev, t_host17, t_dev17, phases, phases17 = [], [], [], [], [], []
    for _ in range(a.reps):
        t_host.append(timed(host_root)[0])
        t, r = timed(dev_root)
        t_dev.append(t)
        phases.append({k: sum(s[k] for _, s in r) for k in r[0][1]})
        del r
        t_host17.append(timed(lambda: chain_io.loadtxt(g17, nthreads=a.threads))[0])
        t, r = timed(lambda: chain_io.loadtxt_device(g17, return_stats=True))
        t_dev17.append(t)
        phases17.append(r[1])
        del r
    med = statistics.median

    def phase_medians(ps):
        return {k: round(med(p[k] for p in ps), 3) for k in ps[0]}

    res["root_%.10e"] = dict(host_s=round(med(t_host), 4), device_s=round(med(t_dev), 4), speedup=round(med(t_host) / med(t_dev), 3),
                             host_all=[round(t, 4) for t in t_host], device_all=[round(t, 4) for t in t_dev], device_phases_ms=phase_medians(phases))
    res["file_%.17g"] = dict(host_s=round(med(t_host17), 4), device_s=round(med(t_dev17), 4), speedup=round(med(t_host17) / med(t_dev17), 3),
                             host_all=[round(t, 4) for t in t_host17], device_all=[round(t, 4) for t in t_dev17], device_phases_ms=phase_medians(phases17))

    # the route a user takes: MCEvidence(root).evidence(), files -> lnE, under both readers (interleaved as well)
    e2e = {"native": [], "hip": []}
    lnE = {}
    for _ in range(max(3, a.reps // 2 + 1)):
        for mode in ("native", "hip"):
            os.environ["MCE_CHAIN_READER"] = mode
            t, v = timed(lambda: pkg.MCEvidence(root, kmax=a.kmax, verbose=0).evidence())
            e2e[mode].append(t)
            lnE[mode] = np.asarray(v)
    os.environ.pop("MCE_CHAIN_READER", None)
    assert np.array_equal(lnE["native"], lnE["hip"]), "evidence differs between the readers"
    res["evidence_from_files"] = dict(native_s=round(med(e2e["native"]), 4), hip_s=round(med(e2e["hip"]), 4), native_all=[round(t, 4) for t in e2e["native"]],
                                      hip_all=[round(t, 4) for t in e2e["hip"]], identical=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
