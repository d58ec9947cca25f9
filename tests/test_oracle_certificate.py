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
