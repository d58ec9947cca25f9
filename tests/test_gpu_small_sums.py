"""The fused and partitioned evidence sums at the smallest shapes: the routes of tests/test_gpu_adversarial_sums.py (its sum_oracle,
sum_certificate, run_fused, run_parts and run_kd are reused) on the inputs and edges of tests/test_gpu_small_shapes.py (its kinds,
deal, inputs and expected_kernel).  finish_dotp and dotp_final_kernel then reduce fewer rows than one 256-thread block, a ragged
last block, one row; a symmetric partition has more ranks than blocks (513 rows are two blocks: a rank without a block returns
zeros at once), a walk partition more ranks than waves that hold a query (the parts beyond the last such wave must be exact zeros),
and the distributed k-d preparation runs at the smallest sets `prune_part_applies` admits (one row fewer: refused).

As there, w and fs come from the oracle so that every row's term of one column is of order 1, and the result is held to the sum
certificate; the oracle, the equalised inputs and the blind count are computed first and alone.  The cap of 1e-5 blind rows means
NONE at these sizes.  A set of a handful of rows marks fewer than three rows with fs = -inf and with a negative weight
(helpers.equalised_inputs nspecial: a quarter of the rows each, at most three).  Needs a real MI355X: run with -m gpu."""
import json
import re
import zlib

import numpy as np
import pytest

import test_gpu_adversarial as A
import test_gpu_adversarial_sums as B
import test_gpu_small_shapes as S
from helpers import exact_distances, sum_certificate, sum_oracle
from test_gpu_small_shapes import EDGE3, KINDS7, row, sizes

pytestmark = pytest.mark.gpu

OFF, FORCE = A.OFF, A.FORCE
ROUTES = B.ROUTES
#: rank counts every route must meet (tests/test_oracle_small_shapes.py::test_small_sums_coverage)
RANKS = {"fused": (1,), "sympart": (2, 3, 4, 8), "walkpart": (2, 3, 7), "kdpart": (2, 4), "pairsonce": (2, 3)}
FUSED_SELFS = ("exclude", "asq", "asr", "shard", "cross")           # k0 = 1 on one buffer (a shard: with self_offset); k0 = 0 with separate sets


def forms(names, W=(1,)):
    """forms with rank counts ("form/W": dealt together, as in the sums matrix)"""
    return tuple("%s/W%d" % (f, w) for w in W for f in names)


FUSED_N = sizes(U=("U",), U1=("U+1",), block=(255, 256, 257), two=(513,))
FUSED_NQ = sizes(one=(1,), block=(255, 257))
SYM_N = sizes(first=(513,), two=(1025,))
WALK_N = sizes(U=("U",), wave=(63, 64, 65), two=(129,), block=(513,))
ONLY_EXCLUDE = ("exclude",)
# route -> rows of the matrix (test_gpu_small_shapes.row; dealt by its deal).  The smallest sets of the distributed k-d preparation: a
# subtree per rank needs 2^lv list chunks of 2048 rows, so (2^lv - 1) 2048 + 1 rows -- held to prune_part_applies on the GPU
MATRIX = {
    "fused": [
        row("sweep", forms(("seeded", "unseeded")), KINDS7, (1, 15, 63), (1, 4, 9, 16), FUSED_N, FUSED_NQ, FUSED_SELFS, 40),
        row("sweep", forms(("twopass",)), KINDS7, (15, 47), (17, 32), FUSED_N, FUSED_NQ, FUSED_SELFS, 12),
        row("wide", forms(("separate",)), KINDS7, (6,), (1, 4), FUSED_N, S.WIDE_NQ, ("asq", "asr"), 8),
        row("panel", forms(("default", "repair", "units")), KINDS7, (2, 27, 63), (1, 9, 16), SYM_N, S.NO_NQ, ONLY_EXCLUDE, 12),
        row("panel", forms(("twopass",)), EDGE3, (15,), (17,), SYM_N, S.NO_NQ, ONLY_EXCLUDE, 3),
        row("sym2", forms(("default",)), KINDS7, (2, 27), (1, 9, 16), SYM_N, S.NO_NQ, ONLY_EXCLUDE, 6),
        row("walk", forms(("default",)), KINDS7, (1, 2, 8, 15), (1, 4, 9, 16), FUSED_N, S.WALK_NQ, FUSED_SELFS, 30),
        row("walk", forms(("short",)), KINDS7, (2,), (9, 10), FUSED_N, S.WALK_NQ, FUSED_SELFS, 6),
        row("deep", forms(("default", "split3")), KINDS7, (64, 127), (1, 6, 16, 32), FUSED_N, FUSED_NQ, FUSED_SELFS, 24),
        row("mfma", forms(("narrow",)), KINDS7, (3, 63, 64, 127), (1, 6, 14, 30), FUSED_N, FUSED_NQ, FUSED_SELFS, 30),
        row("long", forms(("default",)), KINDS7, (128, 129), (1, 7, 30), FUSED_N, FUSED_NQ, FUSED_SELFS, 16),
        row("generic", forms(("default",)), KINDS7, (1, 33), (33, 64), FUSED_N, FUSED_NQ, FUSED_SELFS, 16),
    ],
    "sympart": [
        row("panel", forms(("default", "repair", "units"), (2, 3, 4)), KINDS7, (2, 15, 27, 63), (1, 4, 9, 16), SYM_N, S.NO_NQ, ONLY_EXCLUDE, 27),
        row("shards", forms(("default",), (8,)), KINDS7, (6, 27), (4, 9), SYM_N, S.NO_NQ, ONLY_EXCLUDE, 4),      # beyond four ranks: query shards
    ],
    "walkpart": [
        row("walk", forms(("default",), (2, 3, 7)), KINDS7, (1, 2, 8, 15), (1, 4, 9, 16), WALK_N, S.NO_NQ, ONLY_EXCLUDE, 30),
    ],
    "kdpart": [
        row("walk", forms(("default",), (2,)), EDGE3 + ("heavy_tails",), (2, 6), (4, 9), sizes(first=(2049,)), S.NO_NQ, ONLY_EXCLUDE, 4),
        row("walk", forms(("default",), (4,)), EDGE3 + ("heavy_tails",), (2, 6), (9, 4), sizes(first=(6145,)), S.NO_NQ, ONLY_EXCLUDE, 4),
    ],
    "pairsonce": [
        row("panel", forms(("default",), (2, 3)), KINDS7, (6, 27), (1, 9, 16), SYM_N, S.NO_NQ, ONLY_EXCLUDE, 8),
    ],
}

# ... and on the fused route every family meets nr == U with the three kinds whose padding rows are nearer than real rows or tie with them
MATRIX["fused"] += [dict(r, kinds=EDGE3, nr=S.U_ONLY, selfs=("asq", "asr") if r["family"] == "wide" else ("exclude", "asr"), cases=6)
                    for r in MATRIX["fused"] if r["family"] not in ("panel", "sym2") and r["forms"][0] not in ("twopass/W1", "short/W1")]

# Cases the oracle alone refused as dealt (a blind row, or an ambiguous one), and what was changed, keyed by the id as dealt: the
# other equalised column or another kind.  tests/test_oracle_small_shapes.py::test_small_sums_are_clean_on_the_oracle_alone passes
# on the matrix as adjusted and checks that every entry is used.
ADJUST = {
    # one query against 31 (29) Gaussian rows and the outlier at 1e4, d = 127: the row's columns span e^1138 (e^1148) whichever column is
    # equalised, and with one row there is nothing else in a column -- its first column's sum is 1e-552 (1e-556), which a double cannot hold
    "fused-deep-split3-one_outlier-d127-K32-asr-n32-q1-W1-last": dict(kind="huge_scale_offset", reason="a column's sum below double's normal range"),
    "fused-mfma-wide-one_outlier-d127-K30-asr-n30-q1-W1-last": dict(kind="huge_scale_offset", reason="a column's sum below double's normal range"),
}


def deal(adjust=None):
    """the cases: test_gpu_small_shapes.deal's dicts plus route, W, k0, kmax, col ("last", "last", "first" in turn) and rd (fused:
    return_dist alternating)"""
    adjust = ADJUST if adjust is None else adjust
    cases, seen = [], set()
    for route in ROUTES:
        for r in MATRIX[route]:
            for j, c in enumerate(S.deal([r], adjust={})):
                if (route, S.case_id(c)) in seen:
                    continue                                   # (dealt by an earlier row already)
                seen.add((route, S.case_id(c)))
                form, w = c["form"].split("/W")
                if c["family"] == "mfma":
                    form = S.mfma_form(c["d"])
                c.update(route=route, form=form, W=int(w), k0=1 if c["self"] in ("exclude", "shard") else 0)
                c["kmax"] = c["K"] + c["k0"]
                c["col"] = "first" if j % 3 == 2 else "last"
                c["rd"] = route == "fused" and j % 2 == 0
                c["dealt"] = sums_id(c)
                if c["dealt"] in adjust:
                    c.update({k: v for k, v in adjust[c["dealt"]].items() if k != "reason"})
                cases.append(c)
    return cases


def sums_id(c):
    return "%s-%s-W%d-%s%s" % (c["route"], S.case_id(c), c["W"], c["col"], "-dist" if c["rd"] else "")


CASES = deal()


def nspecial_of(c):
    return min(3, c["nq"] // 4)


def case_sum_oracle(c, X, Y, knn_oracle):
    """the sum's side of the oracle, as B.case_sum_oracle -- seeded with THIS matrix's id (it carries the query count too) and with
    fewer special rows where the set is a handful"""
    odl = exact_distances(X, Y, knn_oracle[1][:, :c["K"] + 1])
    rng = np.random.default_rng(zlib.crc32(sums_id(c).encode()))
    so = sum_oracle(odl, c["d"], c["k0"], c["kmax"], c["col"] == "first", rng, W=c["W"], nspecial=nspecial_of(c))
    # a column that is not exactly zero but sums to less than the smallest normal double cannot be held to a RELATIVE bound by anybody:
    # refused like a blind row (np.longdouble, the truth's format, reaches 1e-4932)
    tiny = [k for k in range(c["k0"], c["kmax"]) if 0 < so["A"][k] < np.finfo(np.float64).tiny]
    if tiny:
        raise ValueError("columns %s sum to less than the smallest normal double (A = %s): change the kind or the column" % (tiny, [float(np.log10(so["A"][k])) for k in tiny]))
    return odl, so


def modes_of(c):
    if c["family"] == "shards":
        return 0, FORCE, OFF, {}
    return S.modes_of(c)


def expected_kernel(c):
    if c["family"] == "shards":                                 # query shards: the exhaustive sweep over a row range
        return [r"^knn_f16_kernel<"], [r"symmetric|pruned|panel-kernel"]
    want, unwanted = S.expected_kernel(c)
    want, unwanted = list(want), list(unwanted)
    if c["route"] == "pairsonce":
        want.append(r" pairs-once ")
    elif c["route"] in ("sympart", "fused"):
        unwanted.append(r"pairs-once")
    return want, unwanted


def assert_kernel(c, kernel):
    want, unwanted = expected_kernel(c)
    for pat in want:
        assert re.search(pat, kernel), (pat, kernel)
    for pat in unwanted:
        assert not re.search(pat, kernel), (pat, kernel)


def searches(c):
    """r -> whether part r of the partition runs a search at all"""
    n, W = c["n"], c["W"]
    if c["route"] == "sympart" and c["family"] == "panel":      # a contiguous range of the sorted 512-row blocks
        nb = -(-n // 512)
        return lambda r: nb * (r + 1) // W > nb * r // W
    if c["route"] == "sympart":                                 # query shards: rows [n r / W, n (r + 1) / W)
        return lambda r: n * (r + 1) // W > n * r // W
    return lambda r: r < 8 * -(-n // 512)                       # the walk: every W-th wave of the dispatch order, eight waves per block


@pytest.fixture()
def lib():
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    yield _capi
    _capi.set_search_mode(_capi.MODE_AUTO)
    _capi.set_sym_mode(_capi.SYM_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


def smallest_kd_rows(lib, c):
    """the smallest n at which prune_part_applies answers yes for the case's d, kmax and W, by bisection (it is monotone in n: the
    chunk count)"""
    lo, hi = c["kmax"], 4 * c["n"]                              # (lo: no; hi: yes)
    assert not lib.prune_part_applies(lo, c["d"], c["kmax"], c["W"]) and lib.prune_part_applies(hi, c["d"], c["kmax"], c["W"])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.prune_part_applies(mid, c["d"], c["kmax"], c["W"]):
            hi = mid
        else:
            lo = mid
    return hi


def run_case(lib, c, setenv):
    X, Y, sm, off = S.case_inputs(c)
    assert len(Y) == c["n"] and len(X) == c["nq"]
    # the reference first and alone: the oracle's lists (an ambiguous row: refused), then the equalised inputs, the truth, the bound
    # and the blind rows (one: refused)
    knn_oracle = S.case_oracle(c, X, Y, sm, off)
    odl, so = case_sum_oracle(c, X, Y, knn_oracle)
    search, sym, prune, env = modes_of(c)
    lib.set_search_mode(search)
    lib.set_sym_mode(sym)
    lib.set_prune_mode(prune)
    for name, val in env.items():
        setenv(name, val)
    twin = None
    if c["route"] == "fused":
        total, kernel = B.run_fused(lib, c, X, Y, sm, off, so, knn_oracle, odl, assert_kernel=assert_kernel)
    elif c["route"] in ("sympart", "walkpart"):
        total, kernel = B.run_parts(lib, c, Y, so, assert_kernel=assert_kernel, searches=searches(c))
        if c["route"] == "walkpart":
            # the dispatch order puts the waves that hold a query first: part r starts at its r-th wave, so the parts beyond the last
            # such wave are exact zeros
            parts = [lib.knn_dotp_part(Y, so["w"], so["fs"], c["kmax"], r, c["W"]) for r in range(-(-c["n"] // 64), c["W"])]
            assert all(not p.any() for p in parts), parts
        twin = B.whole_sum(lib, c, Y, so["w"], so["fs"], OFF if c["route"] == "sympart" else sym, prune)
    elif c["route"] == "kdpart":
        assert smallest_kd_rows(lib, c) == c["n"] and not lib.prune_part_applies(c["n"] - 1, c["d"], c["kmax"], c["W"])
        total, kernel = B.run_kd(lib, c, Y, so, assert_kernel=assert_kernel)
        twin = B.whole_sum(lib, c, Y, so["w"], so["fs"], sym, prune)
    else:
        nblk = (len(Y) + 511) // 512
        assert lib.pairs_once_blocks(len(Y), c["d"], c["kmax"]) == nblk
        if nblk < c["W"]:
            # fewer blocks than ranks (513 rows are two): the partition refuses, cleanly and before any launch
            with pytest.raises(ValueError, match=r"^pairs-once partition not applicable: %d blocks, %d ranks$" % (nblk, c["W"])):
                B._emulate()(Y, so["w"], so["fs"], c["kmax"], c["W"])
            return "refused: %d blocks, %d ranks" % (nblk, c["W"]), so, 0.0
        r = B._emulate()(Y, so["w"], so["fs"], c["kmax"], c["W"])
        total, kernel = r["dotp"], r["kernel"]
        assert_kernel(c, kernel)
        assert sum(r["candidates_sent"]) == sum(r["candidates_received"])
        twin = B.whole_sum(lib, c, Y, so["w"], so["fs"], OFF, OFF)
    worst = sum_certificate(total, so["S"], so["A"], so["T"], c["k0"], what="(%s; %s)" % (sums_id(c), kernel))
    if twin is not None:
        # the parts add up to the single-rank call's sums at the tolerance the Gaussian tests of the partitions use
        assert np.allclose(total[1:], twin[1:], rtol=1e-12, atol=0), (total, twin)
    return kernel, so, worst


@pytest.mark.parametrize("case", CASES, ids=sums_id)
def test_small_sums(case, lib, monkeypatch):
    kernel, so, worst = run_case(lib, case, monkeypatch.setenv)
    print("SUMS " + json.dumps(dict(id=sums_id(case), route=case["route"], rows=so["rows"], blind=so["blind"], worst=worst, amax=so["amax"],
                                    relT=float(np.max(np.where(so["A"] > 0, so["T"] / np.where(so["A"] > 0, so["A"], 1), 0))), kernel=kernel)))
