"""Host-only checks of the certificate's own certificate (tests/verify_cases.py, tests/test_gpu_verify_power.py): the model applies
the documented rule, the sampling pattern has the properties the header promises, the table covers what it claims, and EVERY case of
the GPU file -- clean lists and every corruption -- is decided on the model alone: at these sizes the cap of 1e-5 undecided rows
admits none.  No GPU: nothing of the library runs here."""
import numpy as np
import pytest

import verify_cases as V
from helpers import SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE

NO_TIES = ("heavy_tails", "huge_scale_offset", "tiny_scale", "subnormal_fp16_coords")


# --------------------------------------------------------------------------- the rule, by hand
def test_model_applies_the_documented_rule():
    Y = np.array([[0.0], [1.0], [2.0], [3.0]])
    X = np.array([[0.0]])
    m = V.Model(X, Y, SELF_NONE)
    verdict = lambda mod, *r: mod.judge(np.array([r]))[0][0]
    assert not verdict(m, 0.0, 1.0) and not verdict(m, 0.0, 1.0, 2.0, 3.0)
    assert verdict(m, 0.0, 2.0)                            # row 1 is closer than the second entry
    assert verdict(m, 1.0, 2.0)                            # ... and row 0 than the first
    assert verdict(m, 0.0, 0.5)                            # nothing lies that close
    assert not verdict(m, 0.0, 1.0 + 1e-10) and not verdict(m, 0.0, 1.0 - 1e-10)       # 2e-10 on d^2: inside the tolerance
    assert verdict(m, 0.0, 1.0 + 1e-8) and verdict(m, 0.0, 1.0 - 1e-8)                 # 2e-8: outside
    assert verdict(m, 0.0, np.nan) and verdict(m, np.nan, 1.0) and verdict(m, 0.0, -1.0) and verdict(m, 0.0, -np.inf)
    assert not verdict(m, -0.0, 1.0)                       # (minus zero is zero)
    # +inf: accepted in column k (from 1) only if fewer than k usable rows exist
    assert verdict(m, 0.0, np.inf) and verdict(m, np.inf, np.inf) and verdict(m, 0.0, 1.0, 2.0, np.inf)
    assert not verdict(m, 0.0, 1.0, 2.0, 3.0, np.inf) and not verdict(m, 0.0, 1.0, 2.0, 3.0, np.inf, np.inf)
    assert verdict(m, 0.0, 1.0, 2.0, np.inf, np.inf)
    # the own row skipped under exclude, at self_offset + q
    e = V.Model(np.array([[1.0]]), Y, SELF_EXCLUDE, 1)
    assert not verdict(e, 1.0, 1.0, 2.0) and verdict(e, 0.0, 1.0, 1.0) and verdict(e, 1.0, 2.0)
    assert not verdict(e, 1.0, 1.0, 2.0, np.inf) and verdict(e, 1.0, 1.0, np.inf)
    wrong_own = V.Model(np.array([[1.0]]), Y, SELF_EXCLUDE, 0)
    assert verdict(wrong_own, 1.0, 1.0, 2.0)
    # undecided: an exact d2 within G of a threshold, and only then; a zero threshold never is
    d = 1.0 / np.sqrt(1.0 - 1e-9)
    assert m.judge(np.array([[0.0, d]]))[1][0] and not m.judge(np.array([[0.0, 1.0]]))[1][0] and not m.judge(np.array([[0.0, 0.0]]))[1][0]
    assert V.scan_rounding(128) == 134 * 2.0 ** -53 < 1e-3 * 2 * V.BENIGN        # (a benign factor moves d^2 by twice itself)


def test_surplus_columns_of_a_short_reference_set_pass():
    """catalogue h: lists of K' = 5 on nr = 3, the surplus columns +inf -- and one +inf too many fails"""
    Y = np.random.default_rng(5).standard_normal((3, 4))
    for sm, usable in ((SELF_NONE, 3), (SELF_INCLUDE, 3), (SELF_EXCLUDE, 2)):
        m = V.Model(Y, Y, sm)
        d = np.sort(np.sqrt(np.asarray(V.exact_d2(Y, Y), dtype=np.float64)), axis=1)[:, 3 - usable:]
        lists = np.full((3, 5), np.inf)
        lists[:, :usable] = d
        assert not m.judge(lists)[0].any()
        lists[:, usable - 1] = np.inf
        assert m.judge(lists)[0].all()


# --------------------------------------------------------------------------- the sampling pattern
@pytest.mark.parametrize("nq", [1, 2, 17, 500, 1000, 70000])
def test_sample_rows_are_distinct_and_spread(nq):
    for n in sorted({1, nq // 2 + 1, max(1, nq - 1), nq}):
        if n > nq:
            continue
        for seed in (0, nq - 1, V.U64):
            rows = V.sample_rows(n, nq, seed)
            assert len(rows) == n and rows.min() >= 0 and rows.max() < nq and len(set(rows.tolist())) == n, (nq, n, seed)
            assert rows[0] == seed % nq
            srt = np.sort(rows)
            gaps = np.diff(np.concatenate([srt, [srt[0] + nq]]))
            assert gaps.max() <= -(-nq // n) + 1, (nq, n, seed, int(gaps.max()))
    # wherever n divides nq it is the pattern of before the fix; where nq / 2 < n < nq that one was a single block
    for n in (d for d in range(1, min(nq, 60) + 1) if nq % d == 0):
        assert np.array_equal(V.sample_rows(n, nq, 12345), V.sample_rows_strided(n, nq, 12345))
    if nq >= 17:
        n = nq // 2 + 1
        assert np.array_equal(V.sample_rows_strided(n, nq, 0), np.arange(n)) and V.sample_rows(n, nq, 0)[-1] >= nq - 2


def test_more_samples_than_rows_are_all_rows():
    assert sorted(V.sample_rows(40, 17, 5).tolist()) == list(range(17))


# --------------------------------------------------------------------------- the table
def test_table_covers_what_it_claims():
    cases = V.CASES
    ids = [V.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids) == V.STEPS + 1
    dealt = cases[:-1]
    assert {c["d"] for c in dealt} == {1, 7, 8, 9, 16, 127, 128} and {c["K"] for c in dealt} == {1, 2, 9, 31, 32}
    assert {c["nq"] for c in dealt} == {1, 15, 16, 17, 257} and all(c["ns"] == c["nq"] for c in dealt)
    assert (cases[-1]["nq"], cases[-1]["ns"]) == (600, 301)
    assert {c["nr"] for c in dealt} >= {33, 513, 4097} and {c["nr"] - c["K"] for c in dealt} >= {1}
    assert {c["self"] for c in dealt} == {"none", "include", "exclude", "shard"}
    assert {c["kind"] for c in dealt} == set(V.KINDS) and len(V.KINDS) == 9
    assert all(c["self"] == "none" for c in dealt if c["kind"] == V.CROSS_KIND) and not [c for c in dealt if c["d"] == 1 and c["kind"] == "subnormal_fp16_coords"]
    # every pair (self mode, d), (self mode, K) and (d, K) comes up; duplicates of the own row under exclude
    for a, b in (("self", "d"), ("self", "K"), ("d", "K")):
        assert len({(c[a], c[b]) for c in dealt}) == len({c[a] for c in dealt}) * len({c[b] for c in dealt}), (a, b)
    assert {c["kind"] for c in dealt if c["self"] in ("exclude", "shard")} >= {"few_distinct", "all_identical", "lattice_ties"}
    # a reference split (nr > 4096 and few query blocks) and none
    assert {V.rsplit_of(c["nr"], c["ns"]) for c in dealt} == {1, 2}
    for c in cases:
        X, Y, sm, off = V.case_inputs(c)
        assert X.shape == (c["nq"], c["d"]) and Y.shape == (c["nr"], c["d"])
        assert sm == dict(none=SELF_NONE, include=SELF_INCLUDE, exclude=SELF_EXCLUDE, shard=SELF_EXCLUDE)[c["self"]] and (off > 0) == (c["self"] == "shard")
        if sm != SELF_NONE:
            assert np.array_equal(X, Y[off:off + c["nq"]])
    src = open(V.__file__.replace("verify_cases", "test_gpu_verify_power")).read()
    assert "skip" not in src and "xfail" not in src and "in (0, 1)" not in src


def test_touched_rows_hold_the_edges():
    for nq in (1, 15, 16, 17, 257, 600):
        for j in range(5):
            R = V.touched_rows(nq, j)
            assert 0 in R and nq - 1 in R and len(set(R.tolist())) == len(R) and R.max() < nq
            assert nq % 16 == 0 or (R >= 16 * (nq // 16)).any()
            assert nq <= 256 or 256 in R
            assert len(R) < max(nq, 8) and set(V.touched_rows(nq, j, spread=True).tolist()) >= set(R.tolist()) | set(range(nq - nq // 5, nq))


def test_every_case_is_decided_on_the_model_alone():
    """no undecided row in any case, the clean lists pass, the benign corruptions pass, and every kind of corruption fails where the
    data have no exact ties: all of R"""
    judged = undecided = failing = 0
    per = {}
    for c in V.CASES:
        b = V.built(c)
        assert b.undecided == 0 and not b.clean_fails.any(), V.case_id(c)
        judged += b.judged
        undecided += b.undecided
        for e in b.entries:
            assert not e.fails[np.setdiff1d(np.arange(c["nq"]), e.R)].any(), (V.case_id(c), e.name)
            failing += e.count
            per[e.name[0]] = per.get(e.name[0], 0) + e.count
            if e.name.startswith("h_"):
                assert e.count == 0 and len(e.R) == c["nq"], (V.case_id(c), e.name)
            elif c["kind"] in NO_TIES and c["self"] in ("exclude", "shard") and (e.name != "g" or c["K"] > 1):
                assert e.count == len(e.R), (V.case_id(c), e.name, e.count, len(e.R))
        names = {e.name[0] for e in b.entries}
        assert names >= set("abcfghs") and ("d" in names) == (c["K"] > 1) and ("e" in names) == (c["self"] in ("exclude", "shard"))
    assert set(per) == set("abcdefghs") and all(per[k] > 0 for k in "abcdefgs") and per["h"] == 0
    print("%d cases, %d (row, list) pairs judged, %d undecided, %d failing by the model" % (len(V.CASES), judged, undecided, failing))


def test_the_sampling_case_tells_the_two_patterns_apart():
    """nq = 600, ns = 301: the count over the mirrored sample differs from the count over one contiguous block, for every seed"""
    c = V.CASES[-1]
    b = V.built(c)
    for e in (e for e in b.entries if e.name.startswith("spread")):
        for seed in (0, c["nq"] - 1, V.U64):
            new, old = V.sample_rows(c["ns"], c["nq"], seed), V.sample_rows_strided(c["ns"], c["nq"], seed)
            assert int(e.fails[new].sum()) != int(e.fails[old].sum()), (e.name, seed)


# --------------------------------------------------------------------------- the planted neighbour
def test_planted_rows_sit_on_every_split_boundary():
    assert [V.rsplit_of(nr, V.PLANT_NQ) for nr in V.PLANT_NR] == [1, 2, 3] == [V.rsplit_of(nr, 1) for nr in V.PLANT_NR]
    for nr in V.PLANT_NR:
        J = V.plant_rows(nr)
        assert set(J) >= {0, 255, 256, nr - 1} | {nr * s // r - e for r in (2, 3, 4) for s in range(1, r) for e in (0, 1)}
    assert set(V.plant_rows(4097)) >= {2048, 2047} and set(V.plant_rows(8193)) >= {2731, 2730, 5462, 5461}


@pytest.mark.parametrize("p", V.PLANT_CASES, ids=V.plant_id)
def test_planted_rows_are_reported_and_their_loss_fails(p):
    b = V.planted(p)
    assert b.undecided == 0 and not b.clean_fails.any()
    J = V.plant_rows(p["nr"])
    assert [j for _, j, _ in b.planted][-len(J):] == J
    if p["self"] == "shard":
        assert [(q, j - b.off) for q, j, _ in b.planted[:2]] == [(2, 1), (5, 6)]
        assert {c for _, _, c in b.planted} == set(range(p["K"]))
    for q, j, c in b.planted:
        gap = np.sqrt(float(((b.X[q] - b.Y[j]) ** 2).sum()))
        assert c < p["K"] and abs(gap - b.clean[q, c]) <= 1e-12 * gap
    lost = b.entries[-1]
    assert lost.name == "lost_all" and lost.fails[lost.R].all() and lost.count == len(b.planted)
