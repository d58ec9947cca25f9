"""Host-only checks of the sum certificate (tests/helpers.py: equalised_inputs, sum_truth, sum_bound, sum_certificate) and of the matrix
of tests/test_gpu_adversarial_sums.py: the certificate passes on the oracle's own lists reduced in float64 the way the kernel reduces
them, it FAILS when a single row takes its next neighbour instead -- at the row where that matters least, unless the blind rule
counts that row -- every case of the GPU matrix is clean on the oracle alone, and the matrix covers what it claims."""
import math

import numpy as np
import pytest

import test_gpu_adversarial_sums as S
from helpers import (_ln_terms, AMBIGUOUS_CAP, SUM_EXP_ULP, SUM_LOG_ULP, cert_bound, equalised_inputs, exact_distances, ln_unit_ball_ld, sum_bound, sum_certificate,
                     sum_truth)

N_HOST = 1500


def _pairs():
    """the first case of every (kind, d) of the GPU matrix, at N_HOST rows"""
    seen = {}
    for c in S.CASES:
        if c["n"] > 10000:
            continue
        key = (c["kind"], c["d"])
        if key not in seen:
            n = N_HOST
            nq = n if c["self"] in S.ONE_BUFFER else n // 2 if c["self"] == "shard" else 3 * n // 4 + 5
            seen[key] = dict(c, n=n, nq=nq, W=1)
    return [seen[k] for k in sorted(seen)]


PAIRS = _pairs()


def _tree256(v):
    """the sum of v in float64 the way the reduction takes it: 256-wide blocks, each a halving tree; the blocks' sums strided over 256
    accumulators, then the tree again"""
    def blocks(a):
        a = np.concatenate([a, np.zeros(-len(a) % 256)]).reshape(-1, 256)
        o = 128
        while o >= 1:
            a = a[:, :o] + a[:, o:2 * o]
            o //= 2
        return a[:, 0]
    part = blocks(np.asarray(v, dtype=np.float64))
    acc = np.zeros(256)
    for b in range(len(part)):
        acc[b % 256] += part[b]
    return float(blocks(acc)[0])


def _emulated_sums(X, Y, rows, w, fs, D, k0, kmax):
    """dotp[kmax] in float64 with the kernel's formula (reduce_kernels.hpp) on the squared direct differences to `rows`"""
    d2 = ((X[:, None, :] - Y[rows[:, :kmax - k0]]) ** 2).sum(-1)
    lnc = 0.5 * D * math.log(math.pi) - math.lgamma(1.0 + 0.5 * D)
    base = lnc - np.log(np.abs(w)) + fs
    sgn = np.where(w < 0, -1.0, 1.0)
    out = np.zeros(kmax)
    with np.errstate(divide="ignore"):
        for k in range(k0, kmax):
            out[k] = _tree256(sgn * np.exp(base + 0.5 * D * np.log(d2[:, k - k0])))
    return out


def _host_case(c):
    X, Y, sm, off = S.case_inputs(c)
    ko = S.case_knn_oracle(c, X, Y, sm, off) if not S.is_f64(c) else S.F.oracle_lists(X, Y, c["K"], sm, off, margin=S.F.margin_of(c), weak=True)
    odl, so = S.case_sum_oracle(c, X, Y, ko)
    return X, Y, ko[1], odl, so


@pytest.mark.parametrize("case", PAIRS, ids=S.sums_id)
def test_certificate_passes_on_the_emulated_sum_and_fails_on_one_swapped_row(case):
    c = case
    X, Y, oi, odl, so = _host_case(c)
    D, k0, kmax, K = c["d"], c["k0"], c["kmax"], c["K"]
    w, fs = so["w"], so["fs"]
    got = _emulated_sums(X, Y, oi, w, fs, D, k0, kmax)
    worst = sum_certificate(got, so["S"], so["A"], so["T"], k0)
    # one row takes its next neighbour at the equalised column: the row with the SMALLEST positive effect on that column
    col = so["col"]
    if odl.shape[1] <= col + 1:
        return
    kk = k0 + col
    t = np.exp(_ln_terms(odl[:, col:col + 2], w, fs, D)[0])          # the two terms of every row, np.longdouble
    t0, t1 = t[:, 0], t[:, 1]
    eff = np.abs(t1 - t0)
    if not (eff > 0).any():
        return                                                     # exact ties (or zero terms) on every row: nothing to see
    q = int(np.argmin(np.where(eff > 0, eff, np.inf)))
    rows = oi.copy()
    rows[q, col] = oi[q, col + 1]
    bad = _emulated_sums(X, Y, rows, w, fs, D, k0, kmax)
    blind = eff[q] <= 2 * so["T"][kk]
    print("emulated worst %.3g T; smallest positive effect %.3g of A (row %d), T = %.3g of A%s" % (
        worst, float(eff[q] / so["A"][kk]), q, float(so["T"][kk] / so["A"][kk]), "; BLIND" if blind else ""))
    if blind:
        assert q in so["blind_rows"]
        return
    with pytest.raises(AssertionError, match="sum certificate"):
        sum_certificate(bad, so["S"], so["A"], so["T"], k0)


def test_equalised_inputs_make_every_term_of_the_column_order_one():
    rng = np.random.default_rng(5)
    X = rng.standard_t(1.5, size=(2000, 6))
    od, oi = S.A.oracle_lists(X, X, 4, 2, 0)[:2]
    odl = exact_distances(X, X, oi)
    for col in (0, 3):
        w, fs = equalised_inputs(odl, 6, col, np.random.default_rng(1))
        assert set(np.abs(w)) <= {1.0, 2.0, 3.0, 4.0, 5.0} and int((w < 0).sum()) == 3 and int(np.isneginf(fs).sum()) == 3
        assert not (np.isneginf(fs) & (w < 0)).any()
        live = np.isfinite(fs)
        u = fs[live] + 6 * np.log(odl[live, col].astype(np.float64))
        assert np.all(u > -1.0 - 1e-9) and np.all(u <= 1e-9)
        S_, A_ = sum_truth(odl, w, fs, 6, 1, 5)
        t = float(A_[1 + col]) / live.sum()
        assert math.exp(float(ln_unit_ball_ld(6))) / 5 * math.exp(-1) < t < math.exp(float(ln_unit_ball_ld(6)))
        assert np.all(S_[:1] == 0) and np.all(A_[:1] == 0)


def test_bound_is_the_derived_one():
    u = 2.0 ** -53
    assert (SUM_LOG_ULP, SUM_EXP_ULP) == (2.0, 2.0)
    assert abs(float(ln_unit_ball_ld(6)) - math.log(math.pi ** 3 / 6)) < 1e-15 and abs(float(ln_unit_ball_ld(1)) - math.log(2.0)) < 1e-15
    A = np.array([0.0, 2.0], dtype=np.longdouble)
    D, n, amax, W = 6, 6000, 100.0, 3
    da = D * cert_bound(D) + 5 * u * amax + 5 * u * (3 * math.log(math.pi) + math.lgamma(4.0))
    want = (da * (1 + da) + 2 * u + (1 + 20 + W) * u) * (1 + 2.0 ** -20)
    T = sum_bound(D, n, A, amax, W=W)
    assert T[0] == 0 and abs(float(T[1]) / 2.0 / want - 1) < 1e-12
    assert float(sum_bound(D, 70000, A, amax, W=1)[1]) > float(sum_bound(D, 60000, A, amax, W=1)[1])           # (ceil(n / 65536))
    assert abs(float(sum_bound(D, n, A, amax, W=W, unfused=True)[1] - T[1]) / 2.0 - D * u) < 0.01 * D * u


def test_certificate_on_zero_columns_and_below_k0():
    S_ = np.array([0, 0, 3], dtype=np.longdouble)
    A_ = np.array([0, 0, 3], dtype=np.longdouble)
    T = np.array([0, 0, 1e-12], dtype=np.longdouble)
    assert sum_certificate(np.array([0.0, 0.0, 3.0]), S_, A_, T, 1) == 0.0
    for bad in ([1e-300, 0.0, 3.0], [0.0, 1e-300, 3.0], [0.0, 0.0, 3.0 + 1e-11], [0.0, 0.0, np.inf], [0.0, 0.0, np.nan]):
        with pytest.raises(AssertionError, match="sum certificate"):
            sum_certificate(np.array(bad), S_, A_, T, 1)


def test_all_duplicate_kinds_give_an_exactly_zero_sum():
    for kind, d in (("all_identical", 6), ("few_distinct", 6), ("lattice_ties", 2)):
        c = next(x for x in PAIRS if (x["kind"], x["d"]) == (kind, d) and x["self"] == "exclude")
        X, Y, oi, odl, so = _host_case(c)
        assert np.all(so["A"] == 0) and np.all(so["S"] == 0) and so["blind"] == 0
        assert not _emulated_sums(X, Y, oi, so["w"], so["fs"], d, c["k0"], c["kmax"]).any()


def test_sums_matrix_is_clean_on_the_oracle_alone():
    """on the oracle alone: at most 1e-5 of the rows ambiguous to the oracle, at most 1e-5 blind to the sum, and every fs the library
    is handed finite or -inf.  The whole matrix takes minutes of CPU oracle (and every GPU case refuses itself before the library is
    called), so here: every case of the kinds with the smallest effects, every adjusted case, every third of the others -- and of the
    rows above 10 000 rows only the jittered lattice."""
    small = ("jittered_lattice", "lattice_ties", "fp16_cell_straddlers", "subnormal_fp16_coords", "tight_clusters", "offset_clusters")
    rows = blind = 0
    fsmax = 0.0
    assert all(any(S.case_id(c) == k or S.case_id(dict(c, n=n0)) == k for c in S.CASES for n0 in (2 * c["n"],)) for k in S.ADJUST)     # (every entry is used)
    for i, c in enumerate(S.CASES):
        if c["n"] > 10000 and c["kind"] != small[0]:
            continue
        if c["kind"] not in small and i % 3:
            continue
        X, Y, sm, off = S.case_inputs(c)
        _, so = S.case_sum_oracle(c, X, Y, S.case_knn_oracle(c, X, Y, sm, off))        # (both raise above the cap)
        assert so["blind"] <= AMBIGUOUS_CAP * so["rows"], S.sums_id(c)
        rows += so["rows"]
        blind += so["blind"]
        fin = so["fs"][np.isfinite(so["fs"])]
        fsmax = max(fsmax, float(np.abs(fin).max()))
        assert not np.isnan(so["fs"]).any() and not (so["fs"] == np.inf).any()
    print("%d rows, %d blind, largest |fs| %.1f" % (rows, blind, fsmax))


def test_sums_matrix_coverage():
    cases = S.CASES
    ids = [S.sums_id(c) for c in cases]
    assert len(set(ids)) == len(ids) and 500 <= len(ids) <= 700
    assert {c["route"] for c in cases} == set(S.ROUTES)
    core = set(S.CORE)
    for route in S.ROUTES:
        mine = [c for c in cases if c["route"] == route]
        assert core <= {c["kind"] for c in mine}, route
        assert {c["W"] for c in mine} == set(S.RANKS[route]), (route, {c["W"] for c in mine})
        for W in S.RANKS[route]:                                   # every rank count meets the core kinds
            assert core <= {c["kind"] for c in mine if c["W"] == W}, (route, W)
        assert {c["col"] for c in mine} == {"first", "last"}, route
        assert {c["col"] for c in mine if c["kind"] in core} == {"first", "last"}, route
    fused = [c for c in cases if c["route"] == "fused"]
    assert {c["rd"] for c in fused} == {True, False}
    # every family of both matrices on the fused route (the wide sweep is the exhaustive sweep's kernel at 246 000 queries), return_dist on and off
    for fam in ("sweep", "panel", "sym2", "walk", "deep", "mfma", "long", "generic"):
        mine = [c for c in fused if c["family"] == fam and c["W"] == 1]
        assert {c["rd"] for c in mine} == {True, False}, fam
        assert core <= {c["kind"] for c in mine}, fam
        assert {c["k0"] for c in mine} == ({1} if fam in ("panel", "sym2") else {0, 1}), fam
    assert {c["form"] for c in fused if c["family"] == "sweep"} >= {"seeded", "unseeded", "twopass", "tail"}
    assert {c["form"] for c in fused if c["family"] == "walk"} >= {"default", "short", "heavy"}
    assert any(c["self"] == "shard" for c in fused) and any(c["self"] == "cross" for c in fused)
    assert min(c["K"] for c in fused if c["family"] == "generic") > 32
    sym = [c for c in cases if c["route"] == "sympart"]
    assert {c["form"] for c in sym} == {"default", "repair", "units"} and {c["d"] for c in sym} >= {2, 6, 15, 27, 63}
    assert {c["K"] for c in sym} >= {1, 4, 9, 12, 16} and {c["n"] for c in sym} >= {6000, 6001, 5633, 40037}
    for form in ("default", "repair", "units"):                    # every form meets every rank count of the symmetric partition
        assert {c["W"] for c in sym if c["form"] == form} >= {2, 3, 4}, form
    assert {c["d"] for c in cases if c["route"] == "walkpart"} >= {1, 2, 3, 6, 8, 9, 13, 15}
    assert {(c["W"], c["n"]) for c in cases if c["route"] == "kdpart"} == {(2, 6000), (4, 9000)}
    po = [c for c in cases if c["route"] == "pairsonce"]
    assert {c["d"] for c in po} >= {6, 15, 27, 63} and max(c["K"] for c in po) <= 16 and {c["form"] for c in po} == {"default", "repair"}
    assert all(c["k0"] == 1 and c["self"] == "exclude" for c in cases if c["route"] != "fused")
