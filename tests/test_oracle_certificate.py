"""The kNN certificate of tests/helpers.py judged on the host: it passes on the oracle's own lists for every adversarial
kind and self mode, names the row of every corruption a search could commit, and leaves a swapped AMBIGUOUS pair alone.
No GPU: the lists under test are the CPU oracle's, corrupted by hand."""
import zlib

import numpy as np
import pytest

from helpers import (ADVERSARIAL, ADVERSARIAL_EXTRA, AMBIGUOUS_CAP, CROSS, SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE, CertificateError, cert_bound, knn_certificate,
                     needs_two_columns, oracle_lists, orc)

ULP = 2.0 ** -52


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def _certify_oracle(X, Y, K, sm, off=0):
    od, oi, amb = oracle_lists(X, Y, K, sm, off)
    return knn_certificate(X, Y, K, od[:, :K].copy(), oi[:, :K].copy(), sm, off, kernel="oracle")


@pytest.mark.parametrize("kind,d", [(k, d) for k in sorted({**ADVERSARIAL, **ADVERSARIAL_EXTRA}) for d in (1, 2, 15, 27)
                                    if not (d == 1 and needs_two_columns(k))])
def test_certificate_passes_on_the_oracles_own_lists(kind, d):
    """C1 and C2 are checks of the ORACLE here (np.longdouble against its fp64 sums): it must be within B itself"""
    n, K = 1500, 5
    Y = np.ascontiguousarray({**ADVERSARIAL, **ADVERSARIAL_EXTRA}[kind](_rng(kind, d), n, d), dtype=np.float64)
    for sm in (SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE):
        rep = _certify_oracle(Y, Y, K, sm)
        assert rep["rows"] == n and rep["ambiguous"] == 0 and not rep["failures"]
    lo = 400                                      # a query shard of the set
    rep = _certify_oracle(Y[lo:lo + 300], Y, K, SELF_EXCLUDE, lo)
    assert rep["rows"] == 300 and rep["ambiguous"] == 0
    rep = _certify_oracle(Y[lo:lo + 300], Y, K, SELF_INCLUDE, lo)
    assert rep["ambiguous"] == 0


@pytest.mark.parametrize("kind", sorted(CROSS))
def test_certificate_passes_on_the_oracles_lists_of_separate_sets(kind):
    nq, K = (64, 1) if "_unit_" in kind else (700, 7)          # (a unit Gaussian against a kind of another scale: few rows, or the oracle cannot order them)
    X, Y = CROSS[kind](_rng("cross", kind), nq, 1500, 6)
    rep = _certify_oracle(np.ascontiguousarray(X), np.ascontiguousarray(Y), K, SELF_NONE)
    assert rep["rows"] == nq and rep["ambiguous"] == 0
    if kind == "queries_on_refs":
        assert np.all(oracle_lists(X, Y, 7, SELF_NONE)[0][:, 0] == 0.0)


def test_bound_is_the_derived_one():
    assert cert_bound(2) == 3.0 * 2.0 ** -53 and cert_bound(27) == 15.5 * 2.0 ** -53 and AMBIGUOUS_CAP == 1e-5


@pytest.fixture(scope="module")
def base():
    n, d, K = 2000, 6, 5
    Y = ADVERSARIAL["heavy_tails"](_rng("base"), n, d)
    od, oi, amb = oracle_lists(Y, Y, K, SELF_EXCLUDE)
    assert not amb.any()
    return Y, K, od, oi, amb


def _expect(Y, K, dist, idx, sm, row, check, oracle=None):
    with pytest.raises(CertificateError) as e:
        knn_certificate(Y, Y, K, dist, idx, sm, kernel="knn_under_test<X>", oracle=oracle)
    rep = e.value.report
    assert rep["failed_rows"] == [row], rep["failures"]
    assert any(f[2].startswith(check) for f in rep["failures"]), rep["failures"]
    assert "row %d column" % row in str(e.value) and "knn_under_test<X>" in str(e.value)
    return rep


def test_catches_a_dropped_neighbour(base):
    Y, K, od, oi, amb = base
    for row, col in ((17, 0), (1234, 2), (1999, K - 1)):
        dist, idx = od[:, :K].copy(), oi[:, :K].copy()
        dist[row, col:] = od[row, col + 1:K + 1]               # ... and the (K + 1)-th moved up
        idx[row, col:] = oi[row, col + 1:K + 1]
        rep = _expect(Y, K, dist, idx, SELF_EXCLUDE, row, "C3", oracle=(od, oi, amb))
        assert min(f[1] for f in rep["failures"] if f[2].startswith("C3")) == col


@pytest.mark.parametrize("factor", [1.0 - 1e-12, 1.0 + 1e-12])
def test_catches_a_distance_off_by_1e_12(base, factor):
    Y, K, od, oi, amb = base
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[321, 3] *= factor
    assert dist[321, 2] < dist[321, 3] < dist[321, 4]          # (still ascending: only the value is wrong)
    _expect(Y, K, dist, idx, SELF_EXCLUDE, 321, "C2 distance off", oracle=(od, oi, amb))


def test_catches_two_swapped_rows(base):
    Y, K, od, oi, amb = base
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    idx[77, [1, 2]] = idx[77, [2, 1]]                          # rows swapped under their distances
    _expect(Y, K, dist, idx, SELF_EXCLUDE, 77, "C2 distance off", oracle=(od, oi, amb))
    dist[77, [1, 2]] = dist[77, [2, 1]]                        # entries swapped whole: out of order
    rep = _expect(Y, K, dist, idx, SELF_EXCLUDE, 77, "C2 not ascending", oracle=(od, oi, amb))
    assert any(f[2].startswith("C4") for f in rep["failures"])


def test_catches_a_duplicated_row_index(base):
    Y, K, od, oi, amb = base
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    idx[900, 3], dist[900, 3] = idx[900, 2], dist[900, 2]
    _expect(Y, K, dist, idx, SELF_EXCLUDE, 900, "C1 duplicate row", oracle=(od, oi, amb))


def test_catches_the_own_row_under_self_exclude(base):
    Y, K, od, oi, amb = base
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[5, 1:], idx[5, 1:] = od[5, :K - 1], oi[5, :K - 1]
    dist[5, 0], idx[5, 0] = 0.0, 5
    _expect(Y, K, dist, idx, SELF_EXCLUDE, 5, "C1 own row reported", oracle=(od, oi, amb))
    # a query shard: the own row is self_offset + q
    lo = 1000
    sd, si, sa = oracle_lists(Y[lo:lo + 100], Y, K, SELF_EXCLUDE, lo)
    dist, idx = sd[:, :K].copy(), si[:, :K].copy()
    dist[5, 1:], idx[5, 1:] = sd[5, :K - 1], si[5, :K - 1]
    dist[5, 0], idx[5, 0] = 0.0, lo + 5
    with pytest.raises(CertificateError) as e:
        knn_certificate(Y[lo:lo + 100], Y, K, dist, idx, SELF_EXCLUDE, lo)
    assert e.value.report["failed_rows"] == [5] and any(f[2] == "C1 own row reported" for f in e.value.report["failures"])


def test_catches_the_own_row_missing_or_late_under_self_include(base):
    Y, K = base[0], base[1]
    od, oi, amb = oracle_lists(Y, Y, K, SELF_INCLUDE)
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[8, :K], idx[8, :K] = od[8, 1:K + 1], oi[8, 1:K + 1]
    _expect(Y, K, dist, idx, SELF_INCLUDE, 8, "C1 own row not first", oracle=(od, oi, amb))


def test_catches_a_tie_ordered_by_descending_row():
    n, d, K = 1500, 3, 6
    Y = ADVERSARIAL["lattice_ties"](_rng("ties"), n, d)
    od, oi, amb = oracle_lists(Y, Y, K, SELF_EXCLUDE)
    assert not amb.any()                                       # exact ties are not ambiguous
    rows, cols = np.nonzero(od[:, 1:K] == od[:, :K - 1])
    assert len(rows) > 100
    row, col = int(rows[50]), int(cols[50])
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    idx[row, [col, col + 1]] = idx[row, [col + 1, col]]
    _expect(Y, K, dist, idx, SELF_EXCLUDE, row, "C2 tie not by ascending row", oracle=(od, oi, amb))
    # a zero distance reported as a tiny positive one (duplicates)
    rows = np.flatnonzero(od[:, 0] == 0.0)
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[rows[3], 0] = 1e-300
    _expect(Y, K, dist, idx, SELF_EXCLUDE, int(rows[3]), "C2 zero distance not exact", oracle=(od, oi, amb))


def test_catches_a_row_out_of_range_and_a_non_finite_distance(base):
    Y, K, od, oi, amb = base
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    idx[1, K - 1] = len(Y)
    _expect(Y, K, dist, idx, SELF_EXCLUDE, 1, "C1 row out of range", oracle=(od, oi, amb))
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[2, K - 1] = np.inf
    _expect(Y, K, dist, idx, SELF_EXCLUDE, 2, "C2 distance not finite", oracle=(od, oi, amb))


def _speck_case(far_ulps):
    """100 000 queries (so that the cap admits ONE ambiguous row) against 500 references; query 0 sits at the origin with
    reference row 0 at 1 + far_ulps ulp and row 1 at 1 on the first axis: true distances 1 + far_ulps ulp and 1"""
    rng = _rng("speck")
    Y = rng.standard_normal((500, 2)) + 10.0
    Y[0] = (1.0 + far_ulps * ULP, 0.0)
    Y[1] = (1.0, 0.0)
    X = rng.standard_normal((100000, 2)) + 10.0
    X[0] = 0.0
    return X, Y


def test_a_swapped_ambiguous_pair_is_accepted():
    """B = 1.5 ulp at d = 2: rows 2 ulp apart may come out in either order of two correct fp64 evaluations, here both at
    1 + 1 ulp (a tie, broken by row number: row 0, the farther one, first).  The same swap of rows 16 ulp apart is an error."""
    K = 3
    X, Y = _speck_case(2)
    od, oi, amb = oracle_lists(X, Y, K, SELF_NONE)
    assert amb[0] and amb.sum() == 1 and oi[0, :2].tolist() == [1, 0] and od[0, :2].tolist() == [1.0, 1.0 + 2 * ULP]
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    assert knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=(od, oi, amb))["ambiguous"] == 1
    dist[0, :2] = 1.0 + ULP
    idx[0, :2] = (0, 1)
    rep = knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=(od, oi, amb))
    assert rep["ambiguous"] == 1 and rep["ambiguous_rows"].tolist() == [0] and not rep["failures"]
    # ... but the ambiguous row is still judged by C1 - C3: a third row in place of the pair's second is caught
    idx[0, 1], dist[0, 1] = oi[0, 2], od[0, 2]
    idx[0, 2], dist[0, 2] = oi[0, 3], od[0, 3]
    with pytest.raises(CertificateError) as e:
        knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=(od, oi, amb))
    assert e.value.report["failed_rows"] == [0] and any(f[2].startswith("C3") for f in e.value.report["failures"])

    X, Y = _speck_case(16)
    od, oi, amb = oracle_lists(X, Y, K, SELF_NONE)
    assert not amb.any()
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[0, :2] = 1.0 + 8 * ULP
    idx[0, :2] = (0, 1)
    with pytest.raises(CertificateError) as e:
        knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=(od, oi, amb))
    assert e.value.report["failed_rows"] == [0]


def test_too_many_ambiguous_rows_refuse_the_case():
    """the cap is judged on the oracle alone: one ambiguous row in 1000 is more than 1e-5 of the rows"""
    X, Y = _speck_case(2)
    with pytest.raises(ValueError, match="ambiguous on the oracle alone"):
        oracle_lists(X[:1000], Y, 3, SELF_NONE)


def test_rational_fallback_agrees_with_long_double(base, monkeypatch):
    """hosts whose long double is a double take exact rational sums: same verdicts on a sample"""
    import helpers
    Y, K, od, oi, amb = base
    rows = slice(0, 40)
    dist = od[rows, :K].copy()
    dist[3, 1] *= 1.0 + 1e-12
    a = helpers._dist_within_bound(Y[rows], Y, oi[rows, :K], dist, cert_bound(Y.shape[1]))
    monkeypatch.setattr(helpers, "_LONGDOUBLE_OK", False)
    b = helpers._dist_within_bound(Y[rows], Y, oi[rows, :K], dist, cert_bound(Y.shape[1]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not a[0][3, 1] and a[0].sum() == a[0].size - 1


# --------------------------------------------------------------------------- the GPU matrix covers what it claims (no GPU needed to see it)
def _ksteps(family, d):
    kst = (d + 1 + 15) // 16
    return 8 if family == "deep" and kst == 7 else kst


def test_gpu_matrix_coverage():
    import test_gpu_adversarial as T
    cases = T.CASES
    ids = [T.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids) and len(ids) >= 400
    assert all((c["family"], c["form"]) in T.FORMS for c in cases)
    assert {(c["family"], c["form"]) for c in cases} == set(T.FORMS)                       # every form of the table runs
    kinds = set(ADVERSARIAL) | set(ADVERSARIAL_EXTRA)
    assert len(ADVERSARIAL) == 11 and len(kinds) == 13
    one_set = [c for c in cases if c["kind"] in kinds]
    # every kind meets every family at every k-step count the family has
    for family, ksts in (("wide", (1,)), ("sweep", (1, 2, 3, 4)), ("panel", (1, 2, 3, 4)), ("sym2", (1, 2)), ("walk", (1,)), ("deep", (5, 6, 8))):
        for kst in ksts:
            seen = {c["kind"] for c in one_set if c["family"] == family and _ksteps(family, c["d"]) == kst}
            assert seen == kinds, (family, kst, kinds - seen)
    assert {c["kind"] for c in cases if c["family"] == "wide" and c["self"] == "cross"} == set(T.CROSS_OWN)
    assert {c["kind"] for c in cases if (c["family"], c["form"]) == ("wide", "onebuffer")} == set(T.CORE)     # (246 000 rows on both sides)
    # every kind meets each dimension where fewer than three norm pieces fit (d = 14, 15 mod 16), on the exhaustive sweep and the panel kernel
    for family, dims in (("sweep", (14, 15, 30, 31, 46, 47, 62, 63)), ("panel", (15, 31, 47, 63)), ("walk", (14, 15))):
        for d in dims:
            seen = {c["kind"] for c in one_set if c["family"] == family and c["d"] == d}
            assert seen == kinds, (family, d, kinds - seen)
    # every form meets the core kinds
    for fam_form in T.FORMS:
        seen = {c["kind"] for c in one_set if (c["family"], c["form"]) == fam_form}
        assert set(T.CORE) <= seen, (fam_form, seen)
    # K: every list capacity on the sweep, two passes on sweep, panel and deep filter; K <= 16 on the walk, <= 4 on the wide sweep
    assert {c["K"] for c in cases if c["family"] == "sweep"} >= {1, 4, 8, 9, 12, 16, 17, 32}
    assert {c["K"] for c in cases if c["family"] == "panel"} >= {17, 24, 32}
    assert {c["K"] for c in cases if c["family"] == "deep"} >= {6, 16, 24}
    assert max(c["K"] for c in cases if c["family"] == "walk") == 16 and {9, 10} <= {c["K"] for c in cases if c["family"] == "walk"}
    assert max(c["K"] for c in cases if c["family"] == "wide") <= 4 and min(c["nq"] for c in cases if c["family"] == "wide") >= 480 * 512
    # self modes: one buffer, shards and separate sets wherever the family takes them; the symmetric sweeps are one buffer only
    for family in ("sweep", "walk", "deep"):
        assert {c["self"] for c in cases if c["family"] == family} >= {"exclude", "include", "shard", "asq", "asr", "cross"}, family
        assert {c["kind"] for c in cases if c["family"] == family and c["self"] == "cross"} == set(T.CROSS_OWN) | set(T.UNIT_PARTNER), family
    assert {c["self"] for c in cases if c["family"] in ("panel", "sym2")} == set(T.ONE_BUFFER)
    # the dimensions of the issue's table
    assert {c["d"] for c in cases if c["family"] == "sweep"} >= {1, 13, 14, 15, 29, 30, 31, 45, 46, 47, 61, 62, 63}
    assert {c["d"] for c in cases if c["family"] == "panel"} >= {2, 6, 15, 27, 31, 47, 63}
    assert {c["d"] for c in cases if c["family"] == "walk"} >= {1, 2, 3, 6, 8, 9, 13, 14, 15}
    assert {c["d"] for c in cases if c["family"] == "deep"} == {64, 80, 100, 127}
    assert {c["d"] for c in cases if c["family"] == "wide"} == {1, 6, 13}
    # no case carries a share-based allowance: the only rows outside C4 are the oracle's ambiguous ones
    src = open(T.__file__).read()
    assert "np.mean(" not in src and "0.999" not in src


def test_gpu_matrix_expected_kernel_strings():
    """the patterns a case asserts, against kernel strings of the library's documented shape"""
    import re
    import test_gpu_adversarial as T

    def ok(c, s):
        want, unwanted = T.expected_kernel(c)
        return all(re.search(p, s) for p in want) and not any(re.search(p, s) for p in unwanted)
    c = dict(family="sweep", form="seeded", kind="heavy_tails", d=15, K=9, self="exclude", n=6000, nq=6000)
    good = "knn_f16_kernel<KST=1,KCAP=12> grid=24 block=512 lds=157824 qt=2 ct=48 rsplit=2 seed=1x2"
    assert ok(c, good)
    assert not ok(c, good.replace(" seed=1x2", "")) and not ok(c, good.replace("KST=1", "KST=2")) and not ok(c, good + " wide")
    assert not ok(c, good.replace("> grid", "> symmetric panel-kernel grid")) and not ok(dict(c, K=4), good)
    assert ok(dict(c, form="unseeded"), "knn_f16_kernel<KST=1,KCAP=12> grid=12 block=512 lds=1 qt=2 ct=48 rsplit=1")
    assert not ok(dict(c, form="unseeded"), "knn_f16_kernel<KST=1,KCAP=12> grid=12 block=512 lds=1 qt=2 ct=48 rsplit=12")
    p = dict(c, family="panel", form="default")
    sym = "knn_f16_kernel<KST=1,KCAP=12> symmetric panel-kernel grid=40 block=512 lds=162944 qt=2 ct=48 panel=96 seed=7x8/0 bucket=39936"
    assert ok(p, sym) and not ok(p, good) and not ok(dict(p, family="sym2"), sym) and ok(dict(p, family="sym2"), sym.replace(" panel-kernel", ""))
    assert ok(dict(p, form="twopass", K=24), sym.replace("KCAP=12", "KCAP=16").replace("panel-kernel", "panel-kernel two passes"))
    w = dict(c, family="walk", form="short", d=6)
    walk = "knn_f16_kernel<KST=1,KCAP=12> pruned grid=96 block=64 lds=100 qt=2 ct=64 chunks=3 heavy=0x1 lists=9"
    assert ok(w, walk) and not ok(dict(w, form="long"), walk) and ok(dict(w, form="default"), walk) and not ok(dict(w, form="heavy"), walk)
    dp = dict(c, family="deep", form="split3", d=100, K=24)
    assert ok(dp, "knn_deep_kernel<KST=8,KCAP=16> grid=18 block=512 lds=1 qt=2 ct=6 rsplit=3 two passes seed=25x3")
    assert not ok(dp, "knn_deep_kernel<KST=8,KCAP=16> grid=18 block=512 lds=1 qt=2 ct=6 rsplit=3 seed=25x3")


# --------------------------------------------------------------------------- the margin-aware mode (the fp64 sweeps: K + m selected on GEMM-form keys, refined)
import helpers as H  # noqa: E402
from helpers import WEAK, key_bound, key_bound_c, offset_clusters, refine_margin  # noqa: E402


def _emulated_keys(X, Y):
    """float64 GEMM-form keys about the reference mean, nn + nn' - 2 Z Z'^T; identical reference rows get identical keys, as on the
    device (the keys of the distinct rows, expanded)"""
    c = Y.mean(axis=0)
    Yu, inv = np.unique(Y, axis=0, return_inverse=True)
    zx, zy = X - c, Yu - c
    return ((zx * zx).sum(1)[:, None] + (zy * zy).sum(1)[None, :] - 2.0 * zx @ zy.T)[:, np.asarray(inv).reshape(-1)]


def _emulate(X, Y, K, m, sm, off=0):
    """what the fp64 sweeps compute, on the host: the K + m smallest keys (ties by row; the own row apart), direct differences of
    those, the K nearest of them (ties by row)"""
    G = _emulated_keys(X, Y)
    nq = len(X)
    own = off + np.arange(nq)
    if sm != SELF_NONE:
        G[np.arange(nq), own] = np.inf
    take = K + m - (1 if sm == SELF_INCLUDE else 0)
    sel = np.argsort(G, axis=1, kind="stable")[:, :take]
    diff = X[:, None, :] - Y[sel]
    d2 = (diff * diff).sum(-1)
    order = np.lexsort((sel, d2), axis=1)
    sel, d2 = np.take_along_axis(sel, order, 1), np.take_along_axis(d2, order, 1)
    if sm == SELF_INCLUDE:
        sel, d2 = np.column_stack([own, sel]), np.column_stack([np.zeros(nq), d2])
    return np.sqrt(d2[:, :K]), sel[:, :K].astype(np.int64)


def _f64_kind(kind, d):
    """the generator of the GPU matrix; offset_clusters one step of OFFSET_SCALES below the matrix's separation, which is the largest
    without a key-ambiguous row for the matrix's own draws -- another draw may have one"""
    import test_gpu_adversarial_f64 as F
    if kind == "offset_clusters":
        scales = sorted(H.OFFSET_SCALES)
        return offset_clusters(scales[scales.index(F.OFFSET_S[d]) - 1])
    return F.KINDS[kind]


# (K = 31 and 32 -- m = 1 and 0 -- take kinds whose ambiguous share is 0, as test_gpu_adversarial_f64.THIN does)
@pytest.mark.parametrize("kind,d,K", [(kind, d, K) for kind in ("offset_clusters", "huge_scale_offset", "heavy_tails", "few_distinct", "tight_clusters", "lattice_ties")
                                      for d, K in ((3, 9), (31, 9), (31, 31), (129, 32))
                                      if K < 31 or kind in ("huge_scale_offset", "heavy_tails", "few_distinct")])
def test_margin_certificate_passes_on_the_emulated_sweep(kind, d, K):
    """the certificate with margin = m on a host emulation of the sweeps, n = 3000 as in the GPU matrix: strictly (nothing refused,
    every row by C1 - C4 or, key-ambiguous, by C3w) except for the two WEAK kinds; and the keys stay within key_bound"""
    m = refine_margin(K)
    weak = (kind, "one") in WEAK
    n = 3000
    Y = np.ascontiguousarray(_f64_kind(kind, d)(_rng("emu", kind, d), n, d), dtype=np.float64)
    for sm in (SELF_EXCLUDE, SELF_INCLUDE):
        oracle = oracle_lists(Y, Y, K, sm, margin=m, weak=weak)
        dist, idx = _emulate(Y, Y, K, m, sm)
        rep = knn_certificate(Y, Y, K, dist, idx, sm, oracle=oracle, margin=m, weak=weak, kernel="emulation")
        assert rep["rows"] == n and not rep["failures"]
        if not weak:
            assert rep["key_ambiguous"] + rep["ambiguous"] == 0
        elif kind == "tight_clusters" or d == 3:
            assert rep["key_ambiguous"] > 0.1 * n
    # the bound against np.longdouble on a sample of the queries
    rows = np.arange(0, n, 15)
    G = _emulated_keys(Y[rows], Y)
    E = key_bound(Y[rows], Y)
    worst = 0.0
    for s in range(0, len(rows), 20):
        diff = Y[rows[s:s + 20], None, :].astype(np.longdouble) - Y[None, :, :].astype(np.longdouble)
        err = np.abs(G[s:s + 20].astype(np.longdouble) - (diff * diff).sum(-1))
        ratio = float(np.max(err / np.maximum(E[s:s + 20, None], np.finfo(float).tiny)))
        assert np.all(err <= E[s:s + 20, None]), (kind, d, ratio)
        worst = max(worst, ratio)
    print("max |key error| / E = %.3g (%s, d = %d, c(D) = %g)" % (worst, kind, d, key_bound_c(d)))


def test_key_bound_is_the_derived_one():
    assert key_bound_c(1) == 6 and key_bound_c(31) == 66 and key_bound_c(1024) == 2052
    assert [refine_margin(K) for K in (1, 9, 30, 31, 32)] == [2, 2, 2, 1, 0]
    X = np.array([[3.0, 4.0]])
    Y = np.array([[1.0, 0.0], [-1.0, 0.0]])                      # mean 0: |a| = 5, max |b| = 1
    assert key_bound(X, Y)[0] == 8.0 * 2.0 ** -53 * 36.0
    assert WEAK == {("tight_clusters", "one"), ("lattice_ties", "one")}


@pytest.fixture(scope="module")
def mbase():
    n, d, K = 2000, 6, 5
    Y = ADVERSARIAL["heavy_tails"](_rng("base"), n, d)
    o = oracle_lists(Y, Y, K, SELF_EXCLUDE, margin=2)
    assert o[0].shape[1] == K + 3 and not o[2].any() and not o[3].any()
    return Y, K, o


def _mexpect(X, Y, K, dist, idx, sm, row, check, oracle, margin=2, weak=False):
    with pytest.raises(CertificateError) as e:
        knn_certificate(X, Y, K, dist, idx, sm, kernel="knn_under_test<X>", oracle=oracle, margin=margin, weak=weak)
    rep = e.value.report
    assert rep["failed_rows"] == [row], rep["failures"]
    assert any(f[2].startswith(check) for f in rep["failures"]), rep["failures"]
    return rep


def test_margin_mode_catches_a_dropped_neighbour_and_a_swap_on_a_clean_row(mbase):
    Y, K, o = mbase
    od, oi = o[0], o[1]
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    dist[1234, 2:] = od[1234, 3:K + 1]
    idx[1234, 2:] = oi[1234, 3:K + 1]
    _mexpect(Y, Y, K, dist, idx, SELF_EXCLUDE, 1234, "C3 not", o)
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    idx[77, [1, 2]] = idx[77, [2, 1]]
    dist[77, [1, 2]] = dist[77, [2, 1]]
    rep = _mexpect(Y, Y, K, dist, idx, SELF_EXCLUDE, 77, "C2 not ascending", o)
    assert any(f[2].startswith("C4") for f in rep["failures"])


def _band_case(nq=100000):
    """_speck_case with SIX references on the first axis 4e-14 apart from 1: query 0 (at the origin, 14 from the reference mean: 2 E
    = 1e-12) has its 3rd to 6th neighbours within 2 E of each other in d^2 -- key-ambiguous at K = 3, m = 2 -- and none within 4B"""
    X, Y = _speck_case(0)
    for j in range(6):
        Y[j] = (1.0 + j * 4e-14, 0.0)
    return X[:nq], Y


def test_margin_mode_on_a_key_ambiguous_row():
    K, m = 3, 2
    X, Y = _band_case()
    o = oracle_lists(X, Y, K, SELF_NONE, margin=m)
    od, oi, amb, kamb, E = o
    assert not amb.any() and np.flatnonzero(kamb).tolist() == [0] and oi[0].tolist() == [0, 1, 2, 3, 4, 5]
    assert od[0, K + m] ** 2 - od[0, K - 1] ** 2 <= 2 * E[0] < 1e-11
    dist, idx = od[:, :K].copy(), oi[:, :K].copy()
    rep = knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=o, margin=m)
    assert rep["key_ambiguous"] == 1 and rep["key_ambiguous_rows"].tolist() == [0]
    # the K-th swapped for an outsider inside the band: accepted there (on any other row it is C3 and C4: the test above)
    idx[0, 2], dist[0, 2] = oi[0, 4], od[0, 4]
    assert not knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=o, margin=m)["failures"]
    # ... a neighbour beyond od^2 + 2 E is not
    far = int(oi[0, 5]) + 1
    idx[0, 2], dist[0, 2] = far, float(np.sqrt(((X[0] - Y[far]) ** 2).sum()))
    _mexpect(X, Y, K, dist, idx, SELF_NONE, 0, "C3w", o, margin=m)
    # ... and without the margin contract (plain mode) the swap inside the band is an error
    o3 = oracle_lists(X, Y, K, SELF_NONE)
    idx[0, 2], dist[0, 2] = oi[0, 4], od[0, 4]
    with pytest.raises(CertificateError):
        knn_certificate(X, Y, K, dist, idx, SELF_NONE, oracle=o3)
    # weak: every row by C1, C2, C3w -- the same far neighbour is caught, on a case no cap admits
    ow = oracle_lists(X[:1000], Y, K, SELF_NONE, margin=m, weak=True)
    dist, idx = ow[0][:, :K].copy(), ow[1][:, :K].copy()
    assert not knn_certificate(X[:1000], Y, K, dist, idx, SELF_NONE, oracle=ow, margin=m, weak=True)["failures"]
    idx[0, 2], dist[0, 2] = far, float(np.sqrt(((X[0] - Y[far]) ** 2).sum()))
    _mexpect(X[:1000], Y, K, dist, idx, SELF_NONE, 0, "C3w", ow, margin=m, weak=True)


def test_margin_mode_refuses_a_strict_case_above_the_cap():
    X, Y = _band_case(1000)
    with pytest.raises(ValueError, match="ambiguous on the oracle alone"):
        oracle_lists(X, Y, 3, SELF_NONE, margin=2)
    assert oracle_lists(X, Y, 3, SELF_NONE, margin=2, weak=True)[3].sum() == 1


@pytest.mark.parametrize("margin", [None, 2])
def test_catches_the_own_row_pushed_out_by_duplicates_under_self_include(margin):
    """what a sweep that keeps the earlier row on ties hands on when more than K duplicates precede the own row: rows 0 .. K - 1"""
    n, K = 200, 5
    Y = ADVERSARIAL["all_identical"](_rng("dups"), n, 4)
    o = oracle_lists(Y, Y, K, SELF_INCLUDE) if margin is None else oracle_lists(Y, Y, K, SELF_INCLUDE, margin=margin)
    assert not o[2].any() and (margin is None or not o[3].any())
    assert np.array_equal(o[1][:, 0], np.arange(n))
    dist, idx = np.zeros((n, K)), np.tile(np.arange(K), (n, 1))
    with pytest.raises(CertificateError) as e:
        knn_certificate(Y, Y, K, dist, idx, SELF_INCLUDE, oracle=o, margin=margin)
    rep = e.value.report
    assert rep["failed_rows"] == list(range(1, n)) and all(any(f[0] == q and f[2].startswith("C1 own row not first") for f in rep["failures"]) for q in (K, n - 1))
    knn_certificate(Y, Y, K, o[0][:, :K].copy(), o[1][:, :K].copy(), SELF_INCLUDE, oracle=o, margin=margin)


def test_duplicate_rows_are_not_key_ambiguous_but_distinct_ties_are():
    """identical rows get identical keys and are ordered by row on both sides; distinct rows that tie in truth do not"""
    n, K, m = 600, 9, 2
    Y = ADVERSARIAL["few_distinct"](_rng("fd"), n, 5)
    assert not oracle_lists(Y, Y, K, SELF_EXCLUDE, margin=m)[3].any()
    L = ADVERSARIAL["lattice_ties"](_rng("lt"), n, 4)
    assert oracle_lists(L, L, K, SELF_EXCLUDE, margin=m, weak=True)[3].mean() > 0.1


# --------------------------------------------------------------------------- the fp64 matrix covers what it claims, and WEAK is what the CPU says
def _f64_subsample():
    """The cases the two tests below judge on the oracle alone.  The whole matrix takes over a minute of CPU oracle, so: every case of a
    WEAK pair, every offset_clusters case, every K >= 31 case and every fifth of the others, at the matrix's own n -- but of the
    n = 40037 row only offset_clusters and tight_clusters"""
    import test_gpu_adversarial_f64 as F
    out = []
    for i, c in enumerate(F.CASES):
        special = F.is_weak(c) or c["kind"] == "offset_clusters" or c["K"] in (31, 32)
        if c["n"] > 4000 and c["kind"] not in ("offset_clusters", "tight_clusters"):
            continue
        if special or i % 5 == 0:
            out.append(c)
    return out


def test_weak_table_is_minimal_and_complete():
    """on the oracle alone: every strict case of the (subsampled) matrix is within the cap, no case is refused, and every WEAK pair
    exceeds the cap somewhere"""
    import test_gpu_adversarial_f64 as F
    over = set()
    for c in _f64_subsample():
        X, Y, sm, off = F.case_inputs(c)
        m = F.margin_of(c)
        if m is None:
            oracle_lists(X, Y, c["K"], sm, off)                     # (raises above the cap)
            continue
        od, oi, amb, kamb, E = oracle_lists(X, Y, c["K"], sm, off, margin=m, weak=True)
        share = float((amb | kamb).mean())
        if F.is_weak(c):
            if share > AMBIGUOUS_CAP:
                over.add((c["kind"], F.self_class(c)))
        else:
            assert share <= AMBIGUOUS_CAP, (F.case_id(c), int(amb.sum()), int(kamb.sum()))
    assert over == set(WEAK)


def test_offset_scales_are_the_largest_clean_ones():
    """offset_clusters per dimension: no key-ambiguous row at the chosen separation in any case of that dimension (part of the test
    above), and at the next larger one of OFFSET_SCALES some case has one"""
    import test_gpu_adversarial_f64 as F
    scales = sorted(H.OFFSET_SCALES)
    assert scales == [1, 3, 10, 30, 100]
    cases = [c for c in F.CASES if c["kind"] == "offset_clusters" and c["family"] != "generic"]
    assert {c["d"] for c in cases} >= set(F.NARROW + F.WIDE + F.LONG + F.LONGER + (27,)) and max(c["K"] for c in cases) <= 30
    saved = dict(F.OFFSET_S)
    try:
        for d in sorted({c["d"] for c in cases}):
            if saved[d] == scales[-1]:
                continue
            F.OFFSET_S[d] = scales[scales.index(saved[d]) + 1]
            hit = 0
            for c in cases:
                if c["d"] == d and not hit:
                    X, Y, sm, off = F.case_inputs(c)
                    hit += int(oracle_lists(X, Y, c["K"], sm, off, margin=F.margin_of(c), weak=True)[3].sum())
            assert hit, (d, F.OFFSET_S[d])
    finally:
        F.OFFSET_S.update(saved)


def test_gpu_f64_matrix_coverage():
    import test_gpu_adversarial as T
    import test_gpu_adversarial_f64 as F
    cases = F.CASES
    ids = [F.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids) and 300 <= len(ids) <= 700
    assert F.expand is T.expand and F.inputs is T.inputs and F.case_id is T.case_id                 # (reused, not copied)
    kinds = set(ADVERSARIAL) | set(ADVERSARIAL_EXTRA) | {"offset_clusters"}
    assert len(kinds) == 14 and set(F.KINDS) == kinds
    fam = lambda f, **kw: [c for c in cases if c["family"] == f and all(c[k] == v for k, v in kw.items())]   # noqa: E731
    ks = lambda d: (d + 4) // 4 if d <= 63 else 4 * ((d + 16) // 16)                                      # noqa: E731
    # every kind on every family; the core kinds, offset_clusters and few_distinct on every form and every k-step variant
    for f in ("mfma", "long", "generic"):
        assert {c["kind"] for c in fam(f)} >= kinds | set(T.CROSS_OWN), f
    for form in ("narrow", "wide"):
        assert {c["kind"] for c in fam("mfma", form=form)} >= set(F.ELSE) | set(T.CROSS_OWN) | set(T.UNIT_PARTNER)
    assert {ks(c["d"]) for c in fam("mfma")} == {1, 2, 3, 4, 5, 8, 9, 12, 16, 7, 20, 24, 28, 32}
    for d in F.NARROW + F.WIDE:
        assert {c["kind"] for c in fam("mfma", d=d)} >= {k for k in F.ELSE if not (d == 1 and needs_two_columns(k))}, d
    for d in F.LONG + F.LONGER:
        assert {c["kind"] for c in fam("long", d=d)} >= set(F.ELSE), d
    assert {F.long_blocks(d) for d in F.LONG + F.LONGER} == {(7, 35), (7, 35), (8, 40), (7, 42), (8, 64), (8, 72), (8, 128), (8, 264)}
    assert {F.long_blocks(d)[0] for d in F.LONG} == {7, 8} and F.long_blocks(128) == (7, 35) and F.long_blocks(160) == (7, 42) and F.long_blocks(161) == (7, 42)
    # every list capacity, and m = 2, 1 and 0, on both sweeps
    cap = lambda c: min(k for k in (4, 8, 12, 16, 24, 32) if k >= c["K"] + F.margin_of(c))                 # noqa: E731
    assert {cap(c) for c in fam("mfma", form="narrow")} == {4, 8, 12, 16, 24, 32} == {cap(c) for c in fam("mfma", form="wide")}
    assert {c["K"] for c in fam("mfma")} >= {1, 2, 6, 10, 14, 22, 30, 31, 32, 9}
    assert {c["K"] for c in fam("long")} >= {1, 6, 7, 14, 15, 30, 31, 32}
    for f in ("mfma", "long"):
        assert {F.margin_of(c) for c in fam(f)} == {2, 1, 0}
        assert {c["kind"] for c in fam(f) if c["K"] >= 31} == set(F.THIN) and not set(F.THIN) & {k for k, _ in WEAK}
        for K in (31, 32):
            assert {c["self"] for c in fam(f, K=K)} == set(F.SELFS), (f, K)
    assert {c["K"] for c in fam("generic")} == {33, 40, 64} and all(F.margin_of(c) is None and not F.is_weak(c) for c in fam("generic"))
    # every self mode on every family, the shard and separate sets included
    for f in ("mfma", "long", "generic"):
        assert {c["self"] for c in fam(f)} == set(F.SELFS) | {"cross"}, f
    for kind in F.ELSE:
        for f in ("mfma", "long"):
            assert {c["self"] for c in fam(f, kind=kind)} == set(F.SELFS), (f, kind)
    # sizes: the ragged many-chunk row, the small long-row cases, the generic kernel's odd n
    assert {c["kind"] for c in fam("mfma", n=40037)} >= set(F.ELSE) and all(c["d"] == 27 and c["K"] == 9 for c in fam("mfma", n=40037))
    assert all(c["n"] == 1500 for c in fam("long") if c["d"] >= 511) and {c["n"] for c in fam("long")} == {3000, 1500, 300, 100}
    assert all(c["nq"] == 64 for c in cases if c["kind"] in T.UNIT_PARTNER) and {c["family"] for c in cases if c["kind"] in T.UNIT_PARTNER} == {"mfma", "long"}
    assert all(c["n"] == 3001 and c["n"] % 32 and c["n"] % 128 for c in fam("generic"))
    assert {c["d"] for c in fam("generic")} == {1, 6, 31, 32, 33, 64, 200}
    # the duplicates that push the own row out of the generic kernel's list
    for kind in ("all_identical", "few_distinct"):
        assert fam("generic", kind=kind, self="include"), kind
    # WEAK names only pairs the matrix holds; nothing else is let off
    assert {(c["kind"], F.self_class(c)) for c in cases if F.is_weak(c)} == set(WEAK)
    src = open(F.__file__).read()
    assert "np.mean(" not in src and "0.999" not in src and "1e-3)" not in src


def test_gpu_f64_matrix_expected_kernel_strings():
    """the patterns a case asserts, against kernel strings of the library's documented shape"""
    import re
    import test_gpu_adversarial_f64 as F

    def ok(c, s):
        want, unwanted = F.expected_kernel(c)
        return all(re.search(p, s) for p in want) and not any(re.search(p, s) for p in unwanted)
    c = dict(family="mfma", form="narrow", kind="heavy_tails", d=31, K=10, self="exclude", n=3000, nq=3000)
    good = "knn_mfma_kernel<KS=8,KCAP=12> grid=96 block=512 lds=103424 qt=2 ct=8 rsplit=8"
    assert ok(c, good) and not ok(c, good.replace("KS=8", "KS=9")) and not ok(c, good.replace("KCAP=12", "KCAP=16")) and not ok(dict(c, K=11), good)
    assert not ok(c, good.replace("knn_mfma", "knn_f16")) and not ok(c, good.replace("qt=2", "qt=1"))
    assert ok(dict(c, K=32), good.replace("KCAP=12", "KCAP=32")) and ok(dict(c, K=30), good.replace("KCAP=12", "KCAP=32")) and ok(dict(c, K=1), good.replace("KCAP=12", "KCAP=4"))
    w = dict(c, form="wide", d=100, K=22)
    assert ok(w, "knn_mfma_kernel<KS=28,KCAP=24> grid=96 block=512 lds=1 qt=1 ct=4 rsplit=4") and not ok(w, "knn_deep_kernel<KST=8,KCAP=16> grid=18 block=512 lds=1 qt=2 ct=6 rsplit=3 two passes")
    g = dict(c, family="long", form="split", d=128, K=6)
    lng = "knn_long_kernel<KCAP=8> grid=96 block=512 lds=90112 qt=2 ct=8 rsplit=8 ksp=35"
    assert ok(g, lng) and not ok(g, lng.replace("rsplit=8", "rsplit=1")) and not ok(g, lng.replace("ksp=35", "ksp=40")) and not ok(dict(g, K=7), lng)
    assert ok(dict(g, K=7), lng.replace("KCAP=8", "KCAP=16")) and ok(dict(g, K=15), lng.replace("KCAP=8", "KCAP=32").replace("ct=8", "ct=4")) and not ok(dict(g, K=15), lng.replace("KCAP=8", "KCAP=32"))
    assert ok(dict(g, form="unsplit", n=100, nq=100), lng.replace("rsplit=8", "rsplit=1")) and not ok(dict(g, form="unsplit", n=100, nq=100), lng)
    assert ok(dict(g, form="small", n=300, nq=300), lng) and ok(dict(g, form="small", n=300, nq=300), lng.replace("rsplit=8", "rsplit=1"))
    assert ok(dict(g, d=1024), lng.replace("ksp=35", "ksp=264")) and not ok(g, "knn_generic_kernel grid=24 block=128 lds=8192")
    e = dict(c, family="generic", form="default", d=200, K=40, n=3001, nq=3001)
    assert ok(e, "knn_generic_kernel grid=24 block=128 lds=8192") and not ok(e, "knn_generic_kernel grid=23 block=128 lds=8192") and not ok(e, lng)
