#!/usr/bin/env python
"""Chain files -> ln E on one box, in one run, by three routes:
  (a) native reader (libmcechains.so) + host route      MCEvidence(root).evidence()
  (b) MCE_CHAIN_READER=hip + host route                  the same call, the text parsed on the device and downloaded
  (c) resident                                           mcevidence_amd.evidence_from_files(root): the chain never leaves the device

Writes a C3-sized root once (1 M rows x 29 columns in 4 files, %.10e) and a farm of Planck-shaped roots (synth.planck_like_chains,
4 files each), reads everything once to warm the page cache, checks that the three routes agree -- bitwise on the thinned array
(ResidentChains.to_host() against MCEvidence(...).gd.samples), within 1e-9 on ln E -- and then times them INTERLEAVED (boxes differ by
a few per cent: never compare across runs), `--reps` repetitions each, with a device synchronise inside every window.  Reports
medians, every repetition, the per-stage milliseconds of (c), the CPU count and mce_source_hash().  One JSON document on stdout
(and in --out).

    python tools/chain_resident_bench.py --dir /tmp/crb --out profiles/r07_chain_resident/bench.json
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
    jobs = [("%s_%d.txt" % (root, i + 1), i, nfiles, rows) for i in range(nfiles)]
    farm = [(os.path.join(workdir, "farm%03d" % i), 100 + i, farm_rows) for i in range(nfarm)]
    with ProcessPoolExecutor(max_workers=8) as pool:
        list(pool.map(_write_c3_part, jobs))
        roots = list(pool.map(_write_farm_root, farm))
    return root, roots


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", required=True, help="scratch directory for the text files (about 1.4 GB at the default sizes)")
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the C3-sized root")
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--farm", type=int, default=300, help="Planck-shaped roots of the farm")
    ap.add_argument("--farm-rows", type=int, nargs="+", default=[1700, 1650, 1720, 1641], help="rows of a farm root's files")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kmax", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    root, farm = write_files(a.dir, a.rows, a.files, a.farm, tuple(a.farm_rows))
    t_write = time.perf_counter() - t0

    import torch
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi
    _capi.require_device()
    res = dict(rows=a.rows, files=a.files, farm_roots=a.farm, farm_rows=list(a.farm_rows), reps=a.reps, kmax=a.kmax,
               cpus_allowed=len(os.sched_getaffinity(0)), cpus_box=os.cpu_count(), source_hash=_capi.source_hash(), write_s=round(t_write, 2),
               root_bytes=sum(os.path.getsize("%s_%d.txt" % (root, i + 1)) for i in range(a.files)))

    def host(r, mode, kmax, **kw):
        os.environ["MCE_CHAIN_READER"] = mode
        try:
            return pkg.MCEvidence(r, kmax=kmax, verbose=0, **kw)
        finally:
            os.environ.pop("MCE_CHAIN_READER", None)

    def route(which, r, kmax, **kw):
        if which == "resident":
            out, info = pkg.evidence_from_files(r, kmax=kmax, verbose=0, info=True, require_resident=True, **kw)
            assert info["route"] == "resident"
        else:
            out = host(r, which, kmax, **kw).evidence()
        torch.cuda.synchronize()
        return np.asarray(out)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    # warm (page cache, library, device context) and agree before anything is timed
    for r, kmax, kw in ((root, a.kmax, {}), (farm[0], 3, dict(burnlen=0.3, thinlen=2, ndim=6))):
        m = {mode: host(r, mode, kmax, **kw) for mode in ("native", "hip")}
        rc = pkg.ResidentChains.from_files(r, burnlen=kw.get("burnlen", 0), thinlen=kw.get("thinlen", 0))
        th = rc.to_host()
        for mode in m:
            assert th.shape == m[mode].gd.samples.shape and np.array_equal(th.view(np.uint64), np.ascontiguousarray(m[mode].gd.samples).view(np.uint64)), \
                "to_host() differs from the %s reader's samples" % mode
        lnE = {mode: np.asarray(m[mode].evidence()) for mode in m}
        lnE["resident"] = np.asarray(rc.evidence(kmax=kmax, ndim=kw.get("ndim")))
        worst = max(float(np.max(np.abs(lnE[k] - lnE["native"]))) for k in lnE)
        assert worst <= LNE_PARITY, "ln E differs between the routes by %g" % worst
        res.setdefault("agreement", []).append(dict(root=os.path.basename(r), max_abs_dlnE=worst, to_host_bitwise=True))
        del m, rc, th
    for r in farm:                                          # (the page cache)
        for i in range(len(a.farm_rows)):
            open("%s_%d.txt" % (r, i + 1), "rb").read()

    med = statistics.median
    names = ("native", "hip", "resident")

    def series(fn_of_route):
        t = {k: [] for k in names}
        for _ in range(a.reps):
            for k in names:
                t[k].append(timed(lambda: fn_of_route(k))[0])
        return {k: dict(median_s=round(med(v), 4), min_s=round(min(v), 4), max_s=round(max(v), 4), all_s=[round(x, 4) for x in v]) for k, v in t.items()}

    res["c3_root"] = series(lambda k: route(k, root, a.kmax))
    res["farm"] = series(lambda k: [route(k, r, 3, ndim=6) for r in farm])
    # the stages of (c) on the C3 root
    stages = []
    for _ in range(a.reps):
        t, rc = timed(lambda: pkg.ResidentChains.from_files(root))
        rc.evidence(kmax=a.kmax)
        st = dict(rc.stats["ms"])
        for k in ("ms_upload", "ms_structure", "ms_parse", "ms_download"):
            st["reader_" + k] = sum(f[k] for f in rc.stats["files"])
        st["patched"] = sum(f["patched"] for f in rc.stats["files"])
        stages.append(st)
        del rc
    res["c3_resident_stages_ms"] = {k: round(med(s[k] for s in stages), 3) for k in stages[0]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
