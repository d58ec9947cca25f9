"""The fused and partitioned evidence sums on adversarial data.  MCEvidence(...).evidence() and the multi-rank routes never take
lib.knn(...), the entry point of the two every-row matrices: they call mce_knn_dotp_f64 (merge_lists_kernel with FUSE_DOTP),
mce_knn_dotp_part_f64 (the symmetric partition, query shards, every nparts-th wave of the pruned walk), the distributed k-d
preparation and the all-pairs-once partition, which return only dotp[kmax].  Here every route runs the hard inputs of
tests/helpers.py with w and fs chosen from the oracle so that EVERY row's term of one column is of order 1 (equalised_inputs), and
the result is held to the sum certificate (sum_certificate: |S_hat - S| <= T against np.longdouble, T derived from the kernel's
arithmetic; exact zeros; columns below k0).  The oracle, the equalised inputs and the blind count are computed first and alone; a
case with more than 1e-5 of its rows blind is refused.  The parts of a partition run one after the other on the one GPU and are
added on the host.  Every case asserts on last_kernel() that the route and form it is about actually ran.
tests/test_oracle_sums.py checks on the host what the matrix covers and that the certificate has power on every row.
Needs a real MI355X: run with -m gpu."""
import json
import os
import re
import sys
import zlib

import numpy as np
import pytest

import test_gpu_adversarial as A
import test_gpu_adversarial_f64 as F
from helpers import REPO, cert_bound, exact_distances, kd_partition_shares, oracle_lists, sum_bound, sum_certificate, sum_oracle
from test_gpu_adversarial import CORE, CROSS_OWN, ONE_BUFFER, case_id, expand

pytestmark = pytest.mark.gpu

ALL = A.ALL                      # the 13 one-set kinds
ALL_F64 = F.ALL                  # ... and offset_clusters, on the families of the second matrix
OFF, FORCE = A.OFF, A.FORCE
SEP = ("exclude", "asq", "asr")  # k0 = 1 on one buffer; k0 = 0 with separate sets
ROUTES = ("fused", "sympart", "walkpart", "kdpart", "pairsonce")
#: rank counts every route must meet (tests/test_oracle_sums.py::test_sums_matrix_coverage)
RANKS = {"fused": (1, 3), "sympart": (2, 3, 4, 8), "walkpart": (2, 3, 4, 7, 100), "kdpart": (2, 4), "pairsonce": (2, 3, 5)}


def row(route, family, forms, kinds, dims, K, selfs, n, W=(1,), **kw):
    """a row of the matrix.  The rank counts are dealt WITH the forms (the fastest digit of expand's counter: "form/W")"""
    return dict(route=route, family=family, forms=tuple("%s/W%d" % (f, w) for w in W for f in forms), kinds=kinds, dims=dims, K=K, selfs=selfs, n=n, **kw)


# The matrix, dealt by test_gpu_adversarial.expand: a row is the product kinds x dims; forms with rank counts, K and self modes
# are the digits of its counter, the equalised column (last, last, first) and return_dist (fused route) those of a second one over
# the row's cases (deal, below).  Sizes are the smallest at which a route still has several ranks' worth of structure: n = 6000 is
# 12 blocks of 512 rows, 94 waves of the pruned walk and three k-d chunks; n = 9000 gives the four 2048-row chunks W = 4 needs.
K16 = A.K16
MATRIX = [
    # ---------------------------------------------------------------- fused: knn_dotp(X, Y, w, fs, kmax, k0, return_dist=...)
    row("fused", "sweep", ("seeded", "unseeded"), ALL, (1, 15, 31, 63), K16, SEP, 6000),
    row("fused", "sweep", ("twopass",), CORE, (15, 47), (17, 32), SEP, 6000),
    row("fused", "sweep", ("seeded", "unseeded"), CROSS_OWN, (6,), K16, ("cross",), 6000),
    row("fused", "panel", ("default", "repair", "units"), ALL, (2, 27, 63), (9, 1, 4, 12, 16), ("exclude",), 6000),
    row("fused", "sym2", ("default",), ALL, (6,), (9, 4, 16), ("exclude",), 6000),
    row("fused", "walk", ("default",), ALL, (2, 8, 15), (4, 1, 8, 12, 16), SEP, 6000),
    row("fused", "walk", ("short",), CORE, (2,), (9, 10), SEP, 6000),
    row("fused", "walk", ("default",), CROSS_OWN, (2,), (4, 9, 16), ("cross",), 6000),
    row("fused", "walk", ("heavy",), CORE, (3,), (9,), ("exclude",), 33333),
    row("fused", "deep", ("default", "split3"), ALL, (64, 100), (6, 16, 24), SEP, 3000),
    row("fused", "mfma", ("narrow",), ALL_F64, (3, 31), F.MFMA_K, SEP, 3000),
    row("fused", "mfma", ("wide",), ALL_F64, (100,), (6, 14, 22, 30, 1, 2, 10), SEP, 3000),
    row("fused", "long", ("split",), ALL_F64, (128,), F.LONG_K, SEP, 3000),
    row("fused", "long", ("split",), F.ELSE, (255,), F.LONG_K, SEP, 3000),
    row("fused", "generic", ("default",), ALL_F64, (6, 33), (33, 40), SEP, 3001),            # (the unfused reduction behind the `dd - k0` shift)
    row("fused", "sweep", ("tail",), CORE, (6,), (9,), ("asq",), 30000, nq=135000),            # (two ranges, one reduction)
    row("fused", "sweep", ("seeded",), CORE, (6,), (9,), ("shard",), 6000),                      # (rows [n/3, n/3 + n/2) with self_offset)
    row("fused", "panel", ("default",), CORE, (6,), (9,), ("exclude",), 6001, W=(3,)),           # (devices=[0, 0, 0]: three threads, each a part)
    # ---------------------------------------------------------------- sympart: knn_dotp_part under SYM_FORCE
    row("sympart", "panel", ("default", "repair", "units"), ALL, (2, 6, 15, 27, 63), (1, 4, 9, 12, 16), ("exclude",), 6000, W=(2, 3, 4)),
    row("sympart", "panel", ("default",), CORE, (6,), (9,), ("exclude",), 6001, W=(4,)),         # ragged last block
    row("sympart", "panel", ("default",), CORE, (6,), (9,), ("exclude",), 5633, W=(4,)),
    row("sympart", "panel", ("default",), CORE, (27,), (9,), ("exclude",), 40037, W=(2,)),       # several panels
    row("sympart", "shards", ("default",), CORE, (6,), (9,), ("exclude",), 6000, W=(8,)),        # beyond four ranks: query shards under PlanCap
    # ---------------------------------------------------------------- walkpart: knn_dotp_part under PRUNE_FORCE
    row("walkpart", "walk", ("default",), ALL, (1, 2, 3, 6, 8, 9, 13, 15), (4, 1, 8, 12, 16), ("exclude",), 6000, W=(2, 3, 4, 7)),
    row("walkpart", "walk", ("default",), CORE, (3,), (9,), ("exclude",), 6000, W=(100,)),       # more ranks than waves: the extra parts are zeros
    # ---------------------------------------------------------------- kdpart: prune_part_prepare_dev + knn_dotp_part_prepared_dev
    row("kdpart", "walk", ("default",), CORE, (2, 6), (4, 9), ("exclude",), 6000, W=(2,)),
    row("kdpart", "walk", ("default",), CORE, (2, 6), (9, 4), ("exclude",), 9000, W=(4,)),
    # ---------------------------------------------------------------- pairsonce: tools/pairs_once_emulate.emulate
    row("pairsonce", "panel", ("default",), ALL, (6, 15, 27, 63), (9, 1, 4, 12, 16), ("exclude",), 6000, W=(2, 3, 5)),
    row("pairsonce", "panel", ("default",), CORE, (27,), (9,), ("exclude",), 40037, W=(3,)),
    row("pairsonce", "panel", ("repair",), CORE, (6,), (9,), ("exclude",), 6000, W=(2, 3)),      # MCE_SYM_BUCKET=1: flagged blocks > 0
]


# Cases the oracle alone refused as dealt (more than 1e-5 of the rows blind to the sum, or ambiguous to the oracle), and what was changed,
# keyed by case_id: the other equalised column, or half the rows.  tests/test_oracle_sums.py::test_sums_matrix_is_clean_on_the_oracle_alone
# passes on the matrix as adjusted.
ADJUST = {
    "sweep-seeded-fp16_cell_straddlers-d31-K9-asr-n6000": dict(col="first"),          # last column: 8 of 4505 rows blind (clusters 2^-14 wide seen from afar)
    "walk-default-subnormal_fp16_coords-d2-K4-asr-n6000": dict(n=3000, nq=2255),      # 3 (last) and 1 (first) of 4505 rows blind
    "deep-split3-fp16_cell_straddlers-d100-K24-asr-n3000": dict(n=1500, nq=1130),     # 1 (first) and 11 (last) of 2255 rows blind
    "long-split-offset_clusters-d255-K30-exclude-n3000": dict(n=1500, nq=1500),       # 2 of 3000 rows ambiguous to the oracle at S = 30
    "panel-default-jittered_lattice-d27-K9-exclude-n40037": dict(col="first"),        # (sympart, pairsonce) last column: 2 and 1 of 40037 rows blind
}


def deal(matrix=MATRIX):
    """the cases: expand's dicts plus route, W, k0, kmax, col ("last", "last", "first" in turn) and return_dist (fused: alternating)"""
    cases = []
    for r in matrix:
        nfw = len(r["forms"])
        s2 = 1 if nfw % 2 else nfw                              # the second counter's steps: past the forms' digit where that shares a factor
        s3 = 1 if nfw % 3 else nfw
        for j, c in enumerate(expand([r])):
            form, w = c["form"].split("/W")
            c.update(route=r["route"], form=form, W=int(w), k0=1 if c["self"] in ("exclude", "shard") else 0)
            c["kmax"] = c["K"] + c["k0"]
            c["col"] = "first" if (j // s3) % 3 == 2 else "last"
            c["rd"] = r["route"] == "fused" and c["W"] == 1 and (j // s2) % 2 == 0
            if case_id(c) in ADJUST:
                c.update(ADJUST[case_id(c)])
            cases.append(c)
    return cases


def sums_id(c):
    return "%s-%s-W%d-%s%s" % (c["route"], case_id(c), c["W"], c["col"], "-dist" if c["rd"] else "")


CASES = deal()


def is_f64(c):
    return c["family"] in F.FAMILIES


def case_inputs(c):
    return F.case_inputs(c) if is_f64(c) else A.inputs(c)


def case_knn_oracle(c, X, Y, sm, off):
    """oracle_lists of the case: (od, oi, ambiguous) or, on the GEMM-form families, (od, oi, ambiguous, key_ambiguous, E)"""
    return F.case_oracle(c, X, Y, sm, off) if is_f64(c) else oracle_lists(X, Y, c["K"], sm, off)


def case_sum_oracle(c, X, Y, knn_oracle):
    """the sum's side of the oracle: exact distances to the oracle's K + 1 rows, equalised (w, fs), truth, bound, blind rows"""
    K = c["K"]
    odl = exact_distances(X, Y, knn_oracle[1][:, :K + 1])
    rng = np.random.default_rng(zlib.crc32(sums_id(c).encode()))
    return odl, sum_oracle(odl, c["d"], c["k0"], c["kmax"], c["col"] == "first", rng, W=c["W"])


def modes_of(c):
    """(search mode, sym mode, prune mode, environment) that force the case's family and form"""
    if c["family"] == "shards":
        return 0, FORCE, OFF, {}
    if is_f64(c):
        return F.FAMILIES[c["family"]][0], OFF, OFF, {}
    sym, prune = A.FAMILIES[c["family"]][:2]
    return 0, sym, prune, A.FORMS[c["family"], c["form"]][0]


def expected_kernel(c):
    """(patterns last_kernel() must match, patterns it must not) after a call of the case's route"""
    if c["family"] == "shards":                                 # query shards: the exhaustive sweep over a row range
        return [r"^knn_f16_kernel<"], [r"symmetric|pruned|panel-kernel"]
    want, unwanted = F.expected_kernel(c) if is_f64(c) else A.expected_kernel(c)
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


def dist_checks(c, dist, knn_oracle):
    """the distances the fused call returned, every row: finite, ascending, a true 0 exactly 0 (C2) and within 2B of the oracle's
    (C3) -- on key-ambiguous rows of the GEMM-form families, and on every row of a WEAK pair, C3w instead"""
    od = knn_oracle[0][:, :c["K"]]
    B = cert_bound(c["d"])
    assert dist.shape == od.shape and np.all(np.isfinite(dist)) and np.all(dist >= 0)
    assert np.all(dist[:, 1:] >= dist[:, :-1]), "not ascending"
    assert np.all(dist[od == 0] == 0.0), "a zero distance is not exact"
    relaxed = np.zeros(len(od), dtype=bool)
    if len(knn_oracle) == 5:
        relaxed = np.ones(len(od), dtype=bool) if F.is_weak(c) else knn_oracle[3]
        E = knn_oracle[4]
        ok = dist ** 2 <= od * od * (1.0 + 4.0 * B) + 2.0 * E[:, None]
        assert np.all(ok | ~relaxed[:, None]), "C3w: rows %s" % np.flatnonzero(~ok.all(axis=1) & relaxed)[:5].tolist()
    ok = np.abs(dist - od) <= 2.0 * B * od
    assert np.all(ok | relaxed[:, None]), "C3: rows %s" % np.flatnonzero(~ok.all(axis=1) & ~relaxed)[:5].tolist()


@pytest.fixture()
def lib():
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    yield _capi
    _capi.set_search_mode(_capi.MODE_AUTO)
    _capi.set_sym_mode(_capi.SYM_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


def _emulate():
    tools = os.path.join(REPO, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import pairs_once_emulate
    return pairs_once_emulate.emulate


def whole_sum(lib, c, Y, w, fs, sym, prune):
    """the single-rank twin of a partition: knn_dotp of the whole set"""
    lib.set_sym_mode(sym)
    lib.set_prune_mode(prune)
    return lib.knn_dotp(Y, None, w, fs, c["kmax"], 1)


def run_fused(lib, c, X, Y, sm, off, so, knn_oracle, odl, assert_kernel=assert_kernel):
    """(assert_kernel: what the kernel string is held to -- tests/test_gpu_small_sums.py brings its own)"""
    w, fs, kmax, k0 = so["w"], so["fs"], c["kmax"], c["k0"]
    if c["W"] > 1:
        # devices=[0, 0, 0]: the library's threads each take a part (mce_knn_dotp_part_f64) and leave their kernel strings in their
        # own thread-local slots, so the route is asserted on the parts called from here: bit for bit the same sums, added in rank order
        total = lib.knn_dotp(X, Y, w, fs, kmax, k0, devices=[0] * c["W"])
        parts = []
        for r in range(c["W"]):
            parts.append(lib.knn_dotp_part(Y, w, fs, kmax, r, c["W"]))
            assert_kernel(c, lib.last_kernel())
        acc = np.zeros(kmax)
        for p in parts:
            acc = acc + p
        assert np.array_equal(total, acc), (total, acc)
        return total, lib.last_kernel()
    out = lib.knn_dotp(X, Y, w, fs, kmax, k0, self_offset=off, return_dist=c["rd"])
    kernel = lib.last_kernel()
    assert_kernel(c, kernel)
    total = out
    if c["rd"]:
        total, dist = out
        dist_checks(c, dist, knn_oracle)
    # the unfused kernel on the oracle's distance matrix, against the same truth
    full = np.zeros((len(X), kmax))
    full[:, k0:] = knn_oracle[0][:, :c["K"]]
    un = lib.dotp(full, w, fs, c["d"], k0, kmax)
    sum_certificate(un, so["S"], so["A"], sum_bound(c["d"], len(X), so["A"], so["amax"], W=1, unfused=True), k0, what="(unfused dotp)")
    return total, kernel


def run_parts(lib, c, Y, so, assert_kernel=assert_kernel, searches=lambda r: True):
    """knn_dotp_part, one part after the other.  searches(r): part r runs a search at all (a rank without a block or a wave returns
    zeros at once and leaves the kernel string of whatever ran before)"""
    parts = []
    for r in range(c["W"]):
        parts.append(lib.knn_dotp_part(Y, so["w"], so["fs"], c["kmax"], r, c["W"]))
        if searches(r):
            assert_kernel(c, lib.last_kernel())
        else:
            assert not parts[-1].any(), (r, parts[-1])
        assert parts[-1][0] == 0.0 and np.all(np.isfinite(parts[-1]))
    if c["W"] == 100:                                           # 6000 rows are 94 waves of 64 queries (96 with the padding of 12 blocks)
        assert all(not p.any() for p in parts[96:]), "a part beyond the last wave is not zero"
        assert so["A"][1] == 0 or any(p.any() for p in parts[:94])
    return np.sum(parts, axis=0), lib.last_kernel()


def run_kd(lib, c, Y, so, assert_kernel=assert_kernel):
    import torch
    n, d, kmax, W = len(Y), c["d"], c["kmax"], c["W"]
    assert lib.prune_part_applies(n, d, kmax, W)
    Yd = torch.from_numpy(Y).cuda()
    wd, fd = torch.from_numpy(so["w"]).cuda(), torch.from_numpy(so["fs"]).cuda()
    wsb = lib.knn_workspace_bytes(n, n, d, kmax - 1) + lib.dotp_workspace_bytes(n, kmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    kd = kd_partition_shares(lib, Yd, n, d, kmax, W, wd, fd, ws, wsb)
    kernel = lib.last_kernel()
    assert_kernel(c, kernel)
    cnt = kd["ranges"][0][1]
    assert cnt > 0 and all(0 <= lo < hi <= cnt for _, _, lo, hi in kd["ranges"]), kd["ranges"]     # the ranks made the order together
    assert torch.equal(kd["total"], kd["single"])
    for r in range(W):
        assert torch.equal(kd["prepared"][r], kd["replicated"][r]), r
    return np.sum([p.cpu().numpy() for p in kd["prepared"]], axis=0), kernel


@pytest.mark.parametrize("case", CASES, ids=sums_id)
def test_adversarial_sums(case, lib, monkeypatch):
    c = case
    X, Y, sm, off = case_inputs(c)
    # the reference first and alone: the oracle's lists (a case with more than 1e-5 ambiguous rows is refused), then the equalised
    # inputs, the truth, the bound and the blind rows (more than 1e-5 of them: refused)
    knn_oracle = case_knn_oracle(c, X, Y, sm, off)
    odl, so = case_sum_oracle(c, X, Y, knn_oracle)
    search, sym, prune, env = modes_of(c)
    lib.set_search_mode(search)
    lib.set_sym_mode(sym)
    lib.set_prune_mode(prune)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    twin = None
    if c["route"] == "fused":
        total, kernel = run_fused(lib, c, X, Y, sm, off, so, knn_oracle, odl)
    elif c["route"] in ("sympart", "walkpart"):
        total, kernel = run_parts(lib, c, Y, so)
        twin = whole_sum(lib, c, Y, so["w"], so["fs"], OFF if c["route"] == "sympart" else sym, prune)
    elif c["route"] == "kdpart":
        total, kernel = run_kd(lib, c, Y, so)
        twin = whole_sum(lib, c, Y, so["w"], so["fs"], sym, prune)
    else:
        assert lib.pairs_once_blocks(len(Y), c["d"], c["kmax"]) == (len(Y) + 511) // 512
        r = _emulate()(Y, so["w"], so["fs"], c["kmax"], c["W"])
        total, kernel = r["dotp"], r["kernel"]
        assert_kernel(c, kernel)
        assert sum(r["candidates_sent"]) == sum(r["candidates_received"])
        if c["form"] == "repair":
            assert r["flagged_blocks"] > 0, r["flagged_blocks"]
        twin = whole_sum(lib, c, Y, so["w"], so["fs"], OFF, OFF)
    worst = sum_certificate(total, so["S"], so["A"], so["T"], c["k0"], what="(%s; %s)" % (sums_id(c), kernel))
    print("SUMS " + json.dumps(dict(id=sums_id(c), route=c["route"], rows=so["rows"], blind=so["blind"], worst=worst, amax=so["amax"],
                                    relT=float(np.max(np.where(so["A"] > 0, so["T"] / np.where(so["A"] > 0, so["A"], 1), 0))), kernel=kernel)))
    if twin is not None:
        # the parts add up to the single-rank call's sums at the tolerance the Gaussian tests of the partitions use
        assert np.allclose(total[1:], twin[1:], rtol=1e-12, atol=0), (total, twin)
