"""Host-only checks of the smallest-shapes matrices (tests/test_gpu_small_shapes.py, tests/test_gpu_small_sums.py): they cover what they
claim, every case is clean on the oracle alone -- at these sizes the cap of 1e-5 ambiguous or blind rows admits NONE -- and the
certificate has power where a reference set fills no list: a padding row's number, a duplicate in place of the outlier and a
missing own row are all caught at nr == U and nr == U + 1.  No GPU: the lists under test are the CPU oracle's, corrupted by hand."""
import re
import zlib

import numpy as np
import pytest

import test_gpu_small_shapes as S
from helpers import ADVERSARIAL, SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE, WEAK, CertificateError, knn_certificate, oracle_lists, refine_margin

CASES = S.CASES


def fam(f, **kw):
    return [c for c in CASES if c["family"] == f and all(c[k] == v for k, v in kw.items())]


# --------------------------------------------------------------------------- what the kNN matrix covers
#: family -> (reference-row classes, query classes of separate sets, self modes, list capacities) of its table row
PINS = {
    "sweep": (("U", "U1", "U2", "tile", "chunk", "two"), ("one", "tile", "wave", "block"), S.ALL_SELFS, (4, 8, 12, 16)),
    "wide": (("U", "U1", "tile", "chunk"), ("last1", "exact", "odd"), S.SEPARATE, (4,)),
    "panel": (("first", "tile", "block", "chunk"), (), S.ONE_BUFFER, (4, 12, 16)),
    "sym2": (("first", "tile", "block", "chunk"), (), S.ONE_BUFFER, (4, 12, 16)),
    "walk": (("U", "U1", "tile", "wave", "block", "chunk", "two"), ("one", "wave"), S.ALL_SELFS, (4, 12, 16)),
    "deep": (("U", "U1", "U2", "tile", "chunk", "two"), ("one", "block"), S.ALL_SELFS, (4, 8, 16)),
    "mfma": (("U", "U1", "U2", "U3", "tile", "tile2", "chunk"), ("one", "block"), S.ALL_SELFS, (4, 8, 16, 32)),
    "long": (("U", "U1", "U2", "U3", "tile", "chunk", "two"), ("one", "block"), S.ALL_SELFS, (8, 16, 32)),
    "generic": (("U", "U1", "tile", "two"), ("one", "block"), S.ALL_SELFS, ()),
}


def _kcap(c):
    f = c["family"]
    return S.mfma_kcap(c["K"]) if f == "mfma" else S.long_kcap(c["K"]) if f == "long" else None if f == "generic" else S.f16_kcap(c["K"])


def test_small_matrix_coverage():
    ids = [S.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) and 1000 <= len(ids) <= 1600
    assert set(PINS) == {c["family"] for c in CASES} == set(S.FP16) | set(S.F64)
    assert S.A.inputs is S.case_inputs.__globals__["A"].inputs and S.knn_certificate is knn_certificate       # (reused, not copied)
    for f, (ncls, qcls, selfs, kcaps) in PINS.items():
        mine = fam(f)
        assert {c["cls"] for c in mine} == set(ncls), (f, {c["cls"] for c in mine})
        assert {c["qcls"] for c in mine if c["self"] in S.SEPARATE} == set(qcls), (f, {c["qcls"] for c in mine})
        assert {c["self"] for c in mine} == set(selfs), (f, {c["self"] for c in mine})
        assert {_kcap(c) for c in mine} - {None} == set(kcaps), (f, {_kcap(c) for c in mine})
        assert {c["kind"] for c in mine} >= set(S.KINDS7), f
        # every self mode meets the smallest legal reference set and the next; every reference-row class meets one buffer and separate sets
        for cls in ("U", "U1") if "U" in ncls else ("first",):
            assert {c["self"] for c in mine if c["cls"] == cls} >= set(selfs) - {"shard", "cross"}, (f, cls)
        for cls in ncls:
            kinds_of = {("sep" if c["self"] in S.SEPARATE else "one") for c in mine if c["cls"] == cls}
            assert kinds_of == ({"sep"} if f == "wide" else {"one"} if not qcls else {"one", "sep"}), (f, cls)
        # nr == U (the symmetric sweeps: n = 513, the smallest set the plan admits) with the three kinds whose padding rows are nearer
        # than real rows or tie with them
        small = [c for c in mine if (c["cls"] == "U" if "U" in ncls else c["n"] == 513)]
        assert {c["kind"] for c in small} >= set(S.EDGE3), (f, {c["kind"] for c in small})
        for c in mine:
            U = S.usable_min(c["K"], c["self"])
            assert c["n"] >= U and (c["cls"] != "U" or c["n"] == U) and (c["cls"] != "U1" or c["n"] == U + 1), S.case_id(c)
    # the forms of the two kNN matrices, every one that has a meaning below n = 6000 (the tail needs 264 query blocks, heavy waves 64)
    forms = {(c["family"], c["form"]) for c in CASES if c["family"] in S.FP16}
    assert forms == set(S.A.FORMS) - {("sweep", "tail"), ("wide", "onebuffer"), ("walk", "heavy")}, forms
    assert {c["form"] for c in fam("mfma")} == {"narrow", "wide"}
    # the dimensions and K of the issue's table
    want = dict(sweep=((1, 15, 31, 47, 63), (1, 4, 8, 9, 12, 16, 17, 32)), wide=((1, 6, 13), (1, 3, 4)), panel=((2, 15, 27, 63), (1, 9, 16, 17, 32)),
                walk=((1, 2, 3, 8, 9, 15), (1, 4, 9, 10, 16)), deep=((64, 80, 127), (1, 6, 16, 17, 32)),
                mfma=((1, 3, 4, 16, 31, 63, 64, 127), (1, 2, 6, 14, 30, 31, 32)), long=((128, 129, 1024), (1, 6, 7, 30, 31, 32)), generic=((1, 33, 200), (33, 64, 100)))
    for f, (dims, Ks) in want.items():
        assert {c["d"] for c in fam(f)} == set(dims), f
        assert {c["K"] for c in fam(f)} == set(Ks), (f, {c["K"] for c in fam(f)})
    # the symmetric sweep: 513 rows is two query blocks with ONE row in the second; the wide sweep: 480 blocks with one row in the last,
    # exactly 480, 481 padded to 482; one chunk, a chunk and one row, two chunks and one row on the exhaustive kernels
    assert {c["n"] for c in fam("panel")} == {513, 514, 544, 545, 1023, 1024, 1025, 1537} == {c["n"] for c in fam("sym2")}
    assert {c["nq"] for c in fam("wide")} == {245249, 245760, 245761} and {-(-c["nq"] // 512) for c in fam("wide")} == {480, 481}
    for f in ("sweep", "deep", "mfma"):
        assert {c["n"] - S.chunk_rows(c) for c in fam(f, cls="chunk")} == {-1, 0, 1}, f
    assert {c["n"] for c in fam("sweep", cls="chunk")} >= {1535, 1536, 1537, 767, 768, 769, 511, 512, 513, 383, 384, 385}
    assert {c["n"] for c in fam("deep", cls="chunk")} >= {255, 256, 257, 191, 192, 193}
    assert {S.chunk_rows(c) for c in fam("mfma")} >= {1024, 512, 256, 128, 64, 32}
    assert all(c["n"] == 2 * S.chunk_rows(c) + 1 for f in ("sweep", "deep") for c in fam(f, cls="two"))
    # usable rows below, at and above the K + m entries the fp64 sweeps keep (the merge's `nr > nsel`), own row excluded and not
    for f in ("mfma", "long"):
        for excl in (True, False):
            gaps = {c["n"] - S.usable_min(c["K"], c["self"]) - refine_margin(c["K"]) for c in fam(f)
                    if c["cls"] in ("U", "U1", "U2", "U3") and (c["self"] in ("exclude", "shard")) == excl}
            assert gaps >= {-2, -1, 0, 1}, (f, excl, gaps)
        assert {refine_margin(c["K"]) for c in fam(f)} == {2, 1, 0}
    # WEAK names only pairs the matrix holds; nothing else is let off; one_outlier stays away from K = 31, 32 on the GEMM-form families
    assert {(c["kind"], S.F.self_class(c)) for c in CASES if S.is_weak(c)} == {("lattice_ties", "one")} <= set(WEAK)
    assert all(S.margin_of(c) is None and not S.is_weak(c) for c in CASES if c["family"] in S.FP16 + ("generic",))
    assert not [c for c in CASES if c["kind"] == "one_outlier" and c["K"] >= 31 and c["family"] in ("mfma", "long")]
    src = open(S.__file__).read()
    assert "np.mean(" not in src and "0.999" not in src and "rtol" not in src and "skip" not in src and "xfail" not in src


def test_small_matrix_is_clean_on_the_oracle_alone():
    """every case passes oracle_lists with NO ambiguous and no key-ambiguous row (the WEAK pair apart, which has no cap), and every
    ADJUST entry is used"""
    dealt = {c["dealt"] for c in CASES}
    assert set(S.ADJUST) <= dealt and all("reason" in v for v in S.ADJUST.values())
    rows = 0
    for c in CASES:
        X, Y, sm, off = S.case_inputs(c)
        assert len(Y) == c["n"] and len(X) == c["nq"] and X.shape[1] == c["d"], S.case_id(c)
        o = S.case_oracle(c, X, Y, sm, off)                      # (raises above the cap: one row)
        assert not o[2].any(), S.case_id(c)
        if len(o) == 5 and not S.is_weak(c):
            assert not o[3].any(), S.case_id(c)
        assert o[0].shape[1] == min(c["K"] + (1 if S.margin_of(c) is None else S.margin_of(c) + 1), c["n"] - (sm == SELF_EXCLUDE)), S.case_id(c)
        rows += len(X)
    print("%d cases, %d rows, none ambiguous" % (len(CASES), rows))


def test_weak_pair_of_the_small_matrix_needs_it():
    """lattice_ties on one buffer is judged weakly on the GEMM-form families: somewhere in the matrix it does exceed the cap"""
    over = 0
    for c in CASES:
        if S.is_weak(c):
            X, Y, sm, off = S.case_inputs(c)
            o = oracle_lists(X, Y, c["K"], sm, off, margin=S.margin_of(c), weak=True)
            over += int((o[2] | o[3]).any())
    assert over > 0


def test_small_matrix_expected_kernel_strings():
    """the patterns a case asserts, against kernel strings of the library's documented shape"""
    def ok(c, s):
        want, unwanted = S.expected_kernel(c)
        return all(re.search(p, s) for p in want) and not any(re.search(p, s) for p in unwanted)
    c = dict(family="sweep", form="seeded", kind="one_outlier", d=15, K=9, self="exclude", n=10, nq=10)
    good = "knn_f16_kernel<KST=1,KCAP=12> grid=1 block=512 lds=157824 qt=2 ct=48 rsplit=1"
    assert ok(c, good) and not ok(c, good.replace("rsplit=1", "rsplit=2")) and not ok(c, good.replace("ct=48", "ct=24")) and not ok(dict(c, K=4), good)
    assert ok(dict(c, n=1537), good.replace("rsplit=1", "rsplit=2 seed=1x2")) and not ok(dict(c, n=1537, form="unseeded"), good.replace("rsplit=1", "rsplit=2"))
    assert not ok(dict(c, form="unseeded"), good + " seed=1x2") and not ok(c, good.replace("> grid", "> pruned grid"))
    dp = dict(c, family="deep", form="split3", d=127, K=32, n=192, nq=192)
    deep = "knn_deep_kernel<KST=8,KCAP=16> grid=1 block=512 lds=1 qt=2 ct=6 rsplit=1 two passes seed=33x0"
    assert ok(dp, deep) and not ok(dp, deep.replace(" two passes", "")) and not ok(dict(dp, n=577), deep) and ok(dict(dp, n=577), deep.replace("rsplit=1", "rsplit=3"))
    assert ok(dict(dp, n=193), deep.replace("rsplit=1", "rsplit=2")) and not ok(dict(dp, n=193), deep.replace("rsplit=1", "rsplit=3"))
    m = dict(c, family="mfma", form="narrow", d=3, K=30, n=31, nq=31)
    mf = "knn_mfma_kernel<KS=1,KCAP=32> grid=1 block=512 lds=1 qt=2 ct=32 rsplit=1"
    assert ok(m, mf) and not ok(m, mf.replace("ct=32", "ct=64")) and not ok(dict(m, K=14), mf) and ok(dict(m, K=14), mf.replace("KCAP=32", "KCAP=16").replace("ct=32", "ct=64"))
    g = dict(c, family="generic", form="default", d=200, K=33, n=34, nq=129, self="asr")
    assert ok(g, "knn_generic_kernel grid=2 block=128 lds=8192") and not ok(g, "knn_generic_kernel grid=1 block=128 lds=8192")


# --------------------------------------------------------------------------- the certificate has power where no list fills
def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def _fails(X, Y, K, dist, idx, sm, oracle, margin, check):
    with pytest.raises(CertificateError) as e:
        knn_certificate(X, Y, K, dist, idx, sm, kernel="knn_under_test<X>", oracle=oracle, margin=margin)
    assert any(f[2].startswith(check) for f in e.value.report["failures"]), e.value.report["failures"]
    return e.value.report


@pytest.mark.parametrize("margin", [None, 2])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("K,d", [(1, 1), (4, 3), (9, 15), (16, 63)])
def test_certificate_has_power_at_the_smallest_reference_sets(K, d, extra, margin):
    """on the oracle's own lists at nr == U and nr == U + 1, plain and with the fp64 sweeps' margin: all three must fail"""
    for sm in (SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE):
        nr = K + (1 if sm == SELF_EXCLUDE else 0) + extra
        Y = np.ascontiguousarray(ADVERSARIAL["one_outlier"](_rng("power", K, d, extra), nr, d))
        o = oracle_lists(Y, Y, K, sm) if margin is None else oracle_lists(Y, Y, K, sm, margin=margin)
        od, oi = o[0], o[1]
        assert not o[2].any() and od.shape[1] == K + min(extra, 1 if margin is None else margin + 1)
        knn_certificate(Y, Y, K, od[:, :K].copy(), oi[:, :K].copy(), sm, oracle=o, margin=margin)
        # (1) a padding row's number (>= nr) in the last column, at the distance a row at the centre would have
        for pad in (nr, nr + 1, 32 * ((nr + 31) // 32) - 1 + (nr % 32 == 0)):
            dist, idx = od[:, :K].copy(), oi[:, :K].copy()
            q = 0
            idx[q, K - 1] = pad
            dist[q, K - 1] = float(np.sqrt(((Y[q] - Y.mean(axis=0)) ** 2).sum()))
            rep = _fails(Y, Y, K, dist, idx, sm, o, margin, "C1 row out of range")
            assert rep["failed_rows"] == [q]
        # (2) the outlier (the last row: 1e4 in every column) replaced by a duplicate of another entry of the list (K = 1: by the own row),
        # at that row's true distance and in ascending order, on rows that must report it -- at nr == U that is every other row
        out = nr - 1
        rows = [q for q in range(nr) if q != out and out in oi[q, :K]]
        if extra == 0 and nr > 1:
            assert rows == list(range(nr - 1)), (K, d, sm, rows)
        for q in rows[:2]:
            col = int(np.flatnonzero(oi[q, :K] == out)[0])
            other = int(oi[q, col - 1]) if col > 0 else int(oi[q, col + 1]) if K > 1 else q
            dist, idx = od[:, :K].copy(), oi[:, :K].copy()
            idx[q, col] = other
            dist[q, col] = float(np.sqrt(((Y[q] - Y[other]) ** 2).sum()))
            lead = 1 if sm == SELF_INCLUDE else 0                 # (the own row stays first)
            order = np.concatenate([np.arange(lead), lead + np.lexsort((idx[q, lead:], dist[q, lead:]))])
            dist[q], idx[q] = dist[q, order], idx[q, order]
            with pytest.raises(CertificateError) as e:
                knn_certificate(Y, Y, K, dist, idx, sm, kernel="knn_under_test<X>", oracle=o, margin=margin)
            assert e.value.report["failed_rows"] == [q], e.value.report["failures"]
            assert any(f[2].startswith(("C1 duplicate row", "C1 own row reported")) for f in e.value.report["failures"]), e.value.report["failures"]
            assert any(f[2].startswith(("C3 not", "C4")) for f in e.value.report["failures"]), e.value.report["failures"]
        # (3) the own row missing under include: the others moved up, the next neighbour (or the last again) in the last column
        if sm == SELF_INCLUDE:
            q = nr // 2
            dist, idx = od[:, :K].copy(), oi[:, :K].copy()
            if od.shape[1] > K:
                dist[q], idx[q] = od[q, 1:K + 1], oi[q, 1:K + 1]
            else:                                                # nr == U: nothing to move up -- the last row twice
                dist[q, :K - 1], idx[q, :K - 1] = od[q, 1:K], oi[q, 1:K]
                if K == 1:                                       # (one row in all: an empty list, as the merge writes it)
                    idx[q, 0], dist[q, 0] = -1, np.inf
            rep = _fails(Y, Y, K, dist, idx, sm, o, margin, "C1 own row not first")
            assert rep["failed_rows"] == [q]


# --------------------------------------------------------------------------- the sums at the same edges
import test_gpu_small_sums as T  # noqa: E402
from helpers import equalised_inputs  # noqa: E402


def test_small_sums_coverage():
    cases = T.CASES
    ids = [T.sums_id(c) for c in cases]
    assert len(set(ids)) == len(ids) and 250 <= len(ids) <= 400
    assert {c["route"] for c in cases} == set(T.ROUTES)
    for route in T.ROUTES:
        mine = [c for c in cases if c["route"] == route]
        assert {c["W"] for c in mine} == set(T.RANKS[route]), (route, {c["W"] for c in mine})
        assert {c["col"] for c in mine} == {"first", "last"}, route
        assert set(S.EDGE3) <= {c["kind"] for c in mine}, route
    fused = [c for c in cases if c["route"] == "fused"]
    # every family of the table on the fused route, return_dist on and off, at n = U, U + 1, around one 256-thread block of the reduction
    # and at 513 (the symmetric sweeps: 513 and 1025 only)
    for f in S.FP16 + S.F64:
        mine = [c for c in fused if c["family"] == f]
        assert {c["rd"] for c in mine} == {True, False}, f
        if f in ("panel", "sym2"):
            assert {c["n"] for c in mine} == {513, 1025} and {c["k0"] for c in mine} == {1}, f
            continue
        assert {c["cls"] for c in mine} == {"U", "U1", "block", "two"}, (f, {c["cls"] for c in mine})
        assert {c["n"] for c in mine} >= {255, 256, 257, 513}, (f, sorted({c["n"] for c in mine}))
        assert {c["k0"] for c in mine} == ({0} if f == "wide" else {0, 1}), f
        assert set(S.EDGE3) <= {c["kind"] for c in mine if c["cls"] == "U"}, f
    assert {c["nq"] for c in fused if c["self"] in S.SEPARATE and c["family"] != "wide"} >= {1, 255, 257, 63, 64, 65}
    assert any(c["self"] == "shard" for c in fused) and any(c["self"] == "cross" for c in fused)
    assert {c["form"] for c in fused if c["family"] == "sweep"} == {"seeded", "unseeded", "twopass"}
    assert {c["form"] for c in fused if c["family"] == "deep"} == {"default", "split3"} and {c["form"] for c in fused if c["family"] == "mfma"} == {"narrow", "wide"}
    sym = [c for c in cases if c["route"] == "sympart"]
    assert {c["n"] for c in sym} == {513, 1025} and {c["form"] for c in sym if c["family"] == "panel"} == {"default", "repair", "units"}
    assert {(c["n"], c["W"]) for c in sym} == {(n, W) for n in (513, 1025) for W in (2, 3, 4, 8)}
    # ... where some ranks have no block: 513 rows are two blocks, 1025 three
    assert any(not all(T.searches(c)(r) for r in range(c["W"])) for c in sym if c["n"] == 513 and c["W"] == 3)
    assert all(sum(T.searches(c)(r) for r in range(c["W"])) == min(c["W"], -(-c["n"] // 512)) for c in sym if c["family"] == "panel")
    walk = [c for c in cases if c["route"] == "walkpart"]
    assert {c["cls"] for c in walk} == {"U", "wave", "two", "block"} and {c["n"] for c in walk} >= {63, 64, 65, 129, 513}
    for W in (2, 3, 7):
        assert {c["cls"] for c in walk if c["W"] == W} >= {"U", "wave"}, W                    # more ranks than waves that hold a query
    assert {(c["n"], c["W"]) for c in cases if c["route"] == "kdpart"} == {(2049, 2), (6145, 4)}
    po = [c for c in cases if c["route"] == "pairsonce"]
    assert {(c["n"], c["W"]) for c in po} == {(n, W) for n in (513, 1025) for W in (2, 3)}
    assert all(c["k0"] == 1 and c["self"] == "exclude" for c in cases if c["route"] != "fused")
    # a handful of rows: fewer special rows, so that some row still counts; the default leaves every existing case's w and fs unchanged
    assert [T.nspecial_of(dict(nq=n)) for n in (1, 3, 4, 7, 8, 11, 12, 513)] == [0, 0, 1, 1, 2, 2, 3, 3]
    od = np.abs(np.random.default_rng(3).standard_normal((40, 3))).cumsum(axis=1)
    a = equalised_inputs(od, 3, 2, np.random.default_rng(9))
    b = equalised_inputs(od, 3, 2, np.random.default_rng(9), nspecial=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and int(np.isneginf(a[1]).sum()) == 3 == int((a[0] < 0).sum())
    w1, f1 = equalised_inputs(od, 3, 2, np.random.default_rng(9), nspecial=1)
    assert int(np.isneginf(f1).sum()) == 1 == int((w1 < 0).sum()) and np.array_equal(np.abs(w1), np.abs(a[0]))
    src = open(T.__file__).read()
    assert "rtol=1e-12" in src and "np.mean(" not in src and "skip" not in src and "xfail" not in src


def test_small_sums_are_clean_on_the_oracle_alone():
    """every case: no ambiguous row, no blind row, every fs finite or -inf, and -- unless every term is exactly zero by the data
    (duplicates) -- some row that counts"""
    assert set(T.ADJUST) <= {c["dealt"] for c in T.CASES} and all("reason" in v for v in T.ADJUST.values())
    rows = zero = 0
    for c in T.CASES:
        X, Y, sm, off = S.case_inputs(c)
        o = S.case_oracle(c, X, Y, sm, off)
        assert not o[2].any() and (len(o) == 3 or S.is_weak(c) or not o[3].any()), T.sums_id(c)
        odl, so = T.case_sum_oracle(c, X, Y, o)
        assert so["blind"] == 0, T.sums_id(c)
        assert not np.isnan(so["fs"]).any() and not (so["fs"] == np.inf).any()
        assert int(np.isneginf(so["fs"]).sum()) == T.nspecial_of(c) == int((so["w"] < 0).sum()), T.sums_id(c)
        live = np.isfinite(so["fs"])[:, None] & (np.asarray(odl[:, :c["K"]], dtype=np.float64) > 0)
        assert (so["A"][c["k0"]:] > 0).any() == live.any(), T.sums_id(c)
        zero += int(not live.any())
        rows += so["rows"]
    assert zero < len(T.CASES) // 3
    print("%d cases, %d rows, none blind; %d cases whose sums are exactly zero (duplicates, or a single row with fs = -inf)" % (len(T.CASES), rows, zero))


def test_small_sums_adjustments_were_needed():
    """every ADJUST entry names a case that the oracle alone refuses as dealt"""
    dealt = {T.sums_id(c): c for c in T.deal(adjust={})}
    for key, change in T.ADJUST.items():
        c = dealt[key]
        X, Y, sm, off = S.case_inputs(c)
        with pytest.raises(ValueError, match="blind|ambiguous|smallest normal double"):
            T.case_sum_oracle(c, X, Y, S.case_oracle(c, X, Y, sm, off))
    for key in S.ADJUST:
        c = next(c for c in S.deal(adjust={}) if S.case_id(c) == key)
        X, Y, sm, off = S.case_inputs(c)
        with pytest.raises(ValueError, match="ambiguous"):
            S.case_oracle(c, X, Y, sm, off)
