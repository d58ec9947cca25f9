#!/usr/bin/env python
"""The farm workload -- many small chain roots, files -> all ln E -- on one box, in one run, by four routes:
  (a)  MCEvidence(root).evidence() per root, native reader (libmcechains.so)
  (a2) evidence_many over host-read MCEvidence objects: every root's device work in one mce_evidence_feed_batch_f64 call
  (c)  evidence_from_files(root) per root: the per-root resident route
  (d)  evidence_many_from_files(roots): the farm -- the files parsed per wave, one batched device-source feed

Writes `--farm` Planck-shaped roots (synth.planck_like_chains, 4 files each) and a C3-sized root once, reads everything once to warm
the page cache, checks that the routes agree within 1e-9 on ln E, and times them INTERLEAVED (boxes differ by a few per cent: never
compare across runs), `--reps` repetitions each, with a device synchronise inside every window.  Also: the per-stage milliseconds of
(d) (file read, upload, structure, parse, prep, feed), a sweep of (d) over `--waves` MiB per wave, and the C3-sized root through (d)
as a one-root farm against (c).  One JSON document on stdout (and in --out).

    python tools/chain_farm_bench.py --dir /tmp/cfb --out profiles/r08_chain_farm/bench.json
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

LNE_PARITY = 1e-9


def _write_c3_part(args):
    path, part, nparts, rows = args
    from mcevidence_amd.synth import config_chain
    chain, _ = config_chain("C3", n=rows)
    np.savetxt(path, chain[rows * part // nparts:rows * (part + 1) // nparts], fmt="%.10e")
    return path


def _write_farm_root(args):
    root, seed, rows = args
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    chains, _, _ = planck_like_chains(seed=seed, rows=rows)
    write_cosmomc_chains(root, chains, None)
    return root


def write_files(workdir, rows, nfiles, nfarm, farm_rows):
    """formatted by worker processes, started before this process touches the GPU"""
    root = os.path.join(workdir, "c3")
    jobs = [("%s_%d.txt" % (root, i + 1), i, nfiles, rows) for i in range(nfiles)] if rows > 0 else []
    farm = [(os.path.join(workdir, "farm%03d" % i), 100 + i, farm_rows) for i in range(nfarm)]
    with ProcessPoolExecutor(max_workers=8) as pool:
        list(pool.map(_write_c3_part, jobs))
        roots = list(pool.map(_write_farm_root, farm))
    return root, roots


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True, help="scratch directory for the text files (about 1.4 GB at the default sizes)")
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the C3-sized root (0: skip it)")
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--farm", type=int, default=300, help="Planck-shaped roots of the farm")
    ap.add_argument("--farm-rows", type=int, nargs="+", default=[1700, 1650, 1720, 1641], help="rows of a farm root's files")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kmax", type=int, default=10, help="kmax of the C3-sized root (the farm runs kmax = 3, ndim = 6)")
    ap.add_argument("--waves", type=int, nargs="+", default=[64, 128, 256], help="MiB per wave of the sweep")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    root, farm = write_files(a.dir, a.rows, a.files, a.farm, tuple(a.farm_rows))
    t_write = time.perf_counter() - t0

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi, farm as farm_mod
    _capi.require_device()
    os.environ["MCE_CHAIN_READER"] = "native"
    res = dict(farm_roots=a.farm, farm_rows=list(a.farm_rows), reps=a.reps, c3_rows=a.rows, c3_kmax=a.kmax,
               cpus_allowed=len(os.sched_getaffinity(0)), cpus_box=os.cpu_count(), source_hash=_capi.source_hash(), write_s=round(t_write, 2),
               farm_bytes=sum(os.path.getsize("%s_%d.txt" % (r, i + 1)) for r in farm for i in range(len(a.farm_rows))))

    def farm_route(which, wave_mib=None):
        if which == "a":
            out = [pkg.MCEvidence(r, kmax=3, ndim=6, verbose=0).evidence() for r in farm]
        elif which == "a2":
            out = pkg.evidence_many([pkg.MCEvidence(r, kmax=3, ndim=6, verbose=0) for r in farm], verbose=0)
        elif which == "c":
            out = [pkg.evidence_from_files(r, kmax=3, ndim=6, verbose=0, require_resident=True) for r in farm]
        else:
            got = pkg.evidence_many_from_files(farm, kmax=3, ndim=6, info=True, wave_bytes=None if wave_mib is None else wave_mib << 20)
            assert all(g[1]["route"] == "farm" for g in got)
            out = [g[0] for g in got]
        torch.cuda.synchronize()
        return np.asarray(out)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    med = statistics.median

    def summary(v):
        return dict(median_s=round(med(v), 4), min_s=round(min(v), 4), max_s=round(max(v), 4), all_s=[round(x, 4) for x in v])

    # warm (page cache, library, device context, the reader handle) and agree before anything is timed
    for r in farm:
        for i in range(len(a.farm_rows)):
            open("%s_%d.txt" % (r, i + 1), "rb").read()
    lnE = {k: farm_route(k) for k in ("a", "a2", "c", "d")}
    worst = {k: float(np.max(np.abs(lnE[k] - lnE["a"]))) for k in lnE}
    assert max(worst.values()) <= LNE_PARITY, "ln E differs between the routes: %r" % worst
    res["agreement_max_abs_dlnE_against_a"] = worst
    res["lnE_first_root"] = [float(x) for x in lnE["d"][0]]

    names = ("a", "a2", "c", "d")
    t = {k: [] for k in names}
    stages = []
    for _ in range(a.reps):
        for k in names:
            t[k].append(timed(lambda: farm_route(k))[0])
            if k == "d":
                stages.append(dict(farm_mod.LAST_STATS["ms"], waves=farm_mod.LAST_STATS["counts"]["waves"]))
    res["farm"] = {k: summary(v) for k, v in t.items()}
    res["farm_d_stages_ms"] = {k: round(med(s[k] for s in stages), 3) for k in stages[0]}
    res["default_wave_bytes"] = farm_mod.DEFAULT_WAVE_BYTES

    # the wave size: (d) at 64 / 128 / 256 MiB per wave, interleaved
    farm_mod.release_handles()
    tw = {w: [] for w in a.waves}
    for w in a.waves:
        farm_route("d", w)                                   # (the handle of this capacity: created outside the windows)
    for _ in range(a.reps):
        for w in a.waves:
            tw[w].append(timed(lambda: farm_route("d", w))[0])
    res["wave_sweep"] = {"%d MiB" % w: summary(v) for w, v in tw.items()}
    farm_mod.release_handles()

    # the C3-sized root as a one-root farm against the per-root resident route
    if a.rows > 0:
        size = sum(os.path.getsize("%s_%d.txt" % (root, i + 1)) for i in range(a.files))
        wb = (size // (1 << 20) + 8) << 20

        def one(which):
            if which == "c":
                out, info = pkg.evidence_from_files(root, kmax=a.kmax, verbose=0, info=True, require_resident=True)
            else:
                (out, info), = pkg.evidence_many_from_files([root], kmax=a.kmax, info=True, wave_bytes=wb)
                assert info["route"] == "farm"
            torch.cuda.synchronize()
            return np.asarray(out)

        both = {k: one(k) for k in ("c", "d")}
        d = float(np.max(np.abs(both["c"] - both["d"])))
        assert d <= LNE_PARITY, "the one-root farm differs from the resident route by %g" % d
        t1 = {"c": [], "d": []}
        st1 = []
        for _ in range(a.reps):
            for k in ("c", "d"):
                t1[k].append(timed(lambda: one(k))[0])
                if k == "d":
                    st1.append(dict(farm_mod.LAST_STATS["ms"]))
        res["c3_root"] = dict(bytes=size, max_abs_dlnE=d, **{k: summary(v) for k, v in t1.items()})
        res["c3_root_d_stages_ms"] = {k: round(med(s[k] for s in st1), 3) for k in st1[0]}
        farm_mod.release_handles()

    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
