#!/usr/bin/env python3
"""Workspace sizes of the search planner for a table of shapes, from one or more builds of libmcevidence_hip.so side by side:

    python tools/search_sizes.py [--lib OTHER/libmcevidence_hip.so ...]

The first column is this tree's library.  Shapes marked * hold rocPRIM's answer for its temporary storage (the pruned walk's and the
symmetric sweep's sorts), which depends on the rocPRIM installed and on whether a device is present: they are compared between builds on
one machine (docs/design/search_layout.md), not pinned; tests/test_search_plan_sizes.py pins the others.  Exit status 1 if two
libraries disagree anywhere.  No device work: workspace queries are host arithmetic."""
import argparse
import ctypes as c
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, kind, arguments, modes (search, prune, sym), same_set (-1: unknown), rocPRIM inside
SHAPES = [
    ("long d=300", "knn", (513, 70000, 300, 4), (0, 0, 0), -1, False),
    ("generic K=40", "knn", (1000, 1000, 6, 40), (0, 0, 0), -1, False),
    ("fp64 sweep wide d=100", "knn", (5000, 5000, 100, 4), (1, 0, 0), -1, False),
    ("fp64 sweep d=6", "knn", (31, 513, 6, 17), (1, 0, 0), -1, False),
    ("deep d=100", "knn", (20000, 20000, 100, 4), (0, 0, 0), -1, False),
    ("deep d=100 two-pass", "knn", (20000, 20000, 100, 20), (0, 0, 0), -1, False),
    ("fp16 KST=1", "knn", (5000, 70000, 6, 4), (0, 0, 0), -1, False),
    ("fp16 KST=2", "knn", (5000, 70000, 27, 9), (0, 0, 0), -1, False),
    ("fp16 KST=3", "knn", (5000, 70000, 45, 9), (0, 0, 0), -1, False),
    ("fp16 KST=4", "knn", (5000, 70000, 63, 16), (0, 0, 0), -1, False),
    ("fp16 two-pass K=20", "knn", (5000, 70000, 6, 20), (0, 0, 0), -1, False),
    ("fp16 wide_ok, 489 blocks -> 490", "knn", (250001, 300000, 6, 4), (0, 1, 1), -1, False),
    ("same_set=0", "knn", (1000000, 1000000, 27, 9), (0, 0, 0), 0, False),
    ("sym off", "knn", (1000000, 1000000, 27, 9), (0, 0, 1), 1, False),
    ("same_set=1 *", "knn", (1000000, 1000000, 27, 9), (0, 0, 0), 1, True),
    ("same_set unknown *", "knn", (1000000, 1000000, 27, 9), (0, 0, 0), -1, True),
    ("sym forced, two-pass *", "knn", (70000, 70000, 6, 20), (0, 1, 2), 1, True),
    ("prune forced 100 000 x 6 *", "knn", (100000, 100000, 6, 4), (0, 2, 0), 1, True),
    ("prune forced, 20 000 queries *", "knn", (20000, 100000, 6, 4), (0, 2, 0), 0, True),
    ("prune auto 1 000 000 x 6 *", "knn", (1000000, 1000000, 6, 4), (0, 0, 0), 1, True),
    ("pairs-once 2 ranks *", "apo", (1000000, 27, 10, 2), (0, 0, 0), -1, True),
    ("pairs-once 8 ranks *", "apo", (1000000, 27, 10, 8), (0, 0, 0), -1, True),
    ("pairs-once 70 000 x 27, 2 ranks *", "apo", (70000, 27, 10, 2), (0, 0, 2), -1, True),
]


class Options(c.Structure):
    _fields_ = [("size", c.c_int32), ("search_mode", c.c_int32), ("prune_mode", c.c_int32), ("sym_mode", c.c_int32), ("same_set", c.c_int32)]


def sizes(path):
    lib = c.CDLL(path)
    lib.mce_knn_workspace_bytes_opt.restype = c.c_size_t
    lib.mce_knn_workspace_bytes_opt.argtypes = [c.c_int64, c.c_int64, c.c_int32, c.c_int32, c.c_void_p]
    lib.mce_pairs_once_workspace_bytes.restype = c.c_size_t
    lib.mce_pairs_once_workspace_bytes.argtypes = [c.c_int64, c.c_int32, c.c_int32, c.c_int32]
    out = []
    for _, kind, args, (search, prune, sym), same, _ in SHAPES:
        if kind == "knn":
            opt = Options(c.sizeof(Options), search, prune, sym, same)
            out.append(int(lib.mce_knn_workspace_bytes_opt(*args, c.addressof(opt))))
        else:
            lib.mce_set_sym_mode(sym)
            out.append(int(lib.mce_pairs_once_workspace_bytes(*args)))
            lib.mce_set_sym_mode(0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", action="append", default=[], help="another build's libmcevidence_hip.so")
    a = ap.parse_args()
    libs = [os.path.join(REPO, "mcevidence_amd", "libmcevidence_hip.so")] + a.lib
    cols = [sizes(p) for p in libs]
    bad = 0
    for i, shape in enumerate(SHAPES):
        row = [col[i] for col in cols]
        same = len(set(row)) == 1
        bad += not same
        print("| %-36s | %s | %s |" % (shape[0], " | ".join("%12d" % v for v in row), "equal" if same else "DIFFERENT"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
