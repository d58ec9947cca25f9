#!/usr/bin/env python3
"""GPU box: wall time per call of small fused searches (mce_knn_dotp_f64_dev, auto evidence, K = 4) from two builds of
libmcevidence_hip.so in ONE process, alternating -- what the host side of a call costs (the planner runs on every call):

    python tools/search_host_cost.py --other OTHER/libmcevidence_hip.so [--sessions 2] [--medians 5] [--windows 15] [--calls 100]

A median is taken over `windows` timed windows of `calls` calls each, the device synchronised at both ends of a window; in a session
the two libraries take turns on one workspace, `medians` medians each.  Prints every median and, per shape, whether each of this tree's lies inside the
other build's min - max of at least one session (docs/design/search_layout.md).  `--planner`: no device needed -- the planner alone, ns per
`mce_knn_workspace_bytes` call (make_plan with its sizing pass of the arena), medians of 7 rounds of 20 000 calls, the libraries taking turns."""
import argparse
import ctypes as c
import os
import statistics
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1000, 6, 4), (32000, 6, 4))


def bind(path):
    lib = c.CDLL(path)
    lib.mce_knn_workspace_bytes.restype = c.c_size_t
    lib.mce_knn_workspace_bytes.argtypes = [c.c_int64, c.c_int64, c.c_int32, c.c_int32]
    lib.mce_dotp_workspace_bytes.restype = c.c_size_t
    lib.mce_dotp_workspace_bytes.argtypes = [c.c_int64, c.c_int32]
    lib.mce_knn_dotp_f64_dev.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int32, c.c_int32, c.c_int32, c.c_int64] + [c.c_void_p] * 5 + [c.c_size_t, c.c_void_p]
    return lib


def planner(libs):
    for n, d, K in SHAPES + ((1000000, 27, 9),):
        res = {name: [] for name, _ in libs}
        for _ in range(7):
            for name, lib in libs:
                t0 = time.perf_counter()
                for _ in range(20000):
                    lib.mce_knn_workspace_bytes(n, n, d, K)
                res[name].append((time.perf_counter() - t0) / 20000 * 1e9)
        print("%d x %d, K = %d, ns per workspace query: %s" % (n, d, K, " | ".join("%s %.0f (min %.0f)" % (k, statistics.median(v), min(v)) for k, v in res.items())))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--other", required=True)
    ap.add_argument("--tree", default=os.path.join(REPO, "mcevidence_amd", "libmcevidence_hip.so"), help="the library measured against --other (a copy of --other: an A/A control)")
    ap.add_argument("--sessions", type=int, default=2)
    ap.add_argument("--medians", type=int, default=5)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--planner", action="store_true")
    a = ap.parse_args()
    libs = (("other", bind(a.other)), ("tree", bind(a.tree)))
    if a.planner:
        return planner(libs)
    import torch
    ok = True
    for n, d, K in SHAPES:
        g = torch.Generator().manual_seed(n)
        X = torch.randn(n, d, dtype=torch.float64, generator=g).cuda()
        w = torch.ones(n, dtype=torch.float64, device="cuda")
        fs = torch.zeros(n, dtype=torch.float64, device="cuda")
        out = torch.zeros(K + 1, dtype=torch.float64, device="cuda")
        calls, sums = {}, {}
        # ONE workspace for both builds (where a buffer lies moves a call by more than the host code does)
        nb = max(int(lib.mce_knn_workspace_bytes(n, n, d, K)) + int(lib.mce_dotp_workspace_bytes(n, K + 1)) for _, lib in libs)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        for name, lib in libs:

            def call(lib=lib, ws=ws, nb=nb):
                rc = lib.mce_knn_dotp_f64_dev(X.data_ptr(), n, X.data_ptr(), n, d, K + 1, 1, 0, w.data_ptr(), fs.data_ptr(), out.data_ptr(), None, ws.data_ptr(), nb, None)
                assert rc == 0, rc
            calls[name] = call
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            sums[name] = out.cpu().clone()
        assert torch.equal(sums["other"], sums["tree"]), "the two builds disagree"
        sessions = []
        for _ in range(a.sessions):
            res = {"other": [], "tree": []}
            for m in range(a.medians):
                for name, _ in (libs if m % 2 == 0 else libs[::-1]):          # (who goes first takes turns too)
                    t = []
                    for _ in range(a.windows):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(a.calls):
                            calls[name]()
                        torch.cuda.synchronize()
                        t.append((time.perf_counter() - t0) / a.calls * 1e6)
                    res[name].append(statistics.median(t))
            sessions.append(res)
            print("%d x %d, K = %d, session %d, us per call: other %s (min %.2f max %.2f) | tree %s" % (
                n, d, K, len(sessions), " ".join("%.2f" % v for v in res["other"]), min(res["other"]), max(res["other"]),
                " ".join("%.2f" % v for v in res["tree"])), flush=True)
        # every median of this tree inside the other build's min - max of at least one session
        inside = [any(min(r["other"]) <= v <= max(r["other"]) for r in sessions) for s in sessions for v in s["tree"]]
        ok = ok and all(inside)
        print("%d x %d: this tree's medians inside the other build's min - max of a session: %s" % (n, d, inside), flush=True)
    print("all inside" if ok else "NOT all inside")


if __name__ == "__main__":
    main()
