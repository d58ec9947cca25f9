"""Every fp16-filter kernel family on adversarial data, EVERY row judged by the high-precision certificate of tests/helpers.py
(knn_certificate: C1 rows, C2 distances against np.longdouble within the derived bound B, C3 completeness against the CPU
oracle's K + 1 nearest, C4 the oracle's rows except on rows the oracle itself cannot order) and by the library's own run-time
certificate on all rows.  No share of wrong entries is tolerated.  Every case asserts on last_kernel() that the family and
form it is about actually ran.  The matrix is the one table below (MATRIX); tests/test_oracle_certificate.py checks on the
host that it covers what it claims.  Needs a real MI355X: run with -m gpu."""
import math
import re
import zlib

import numpy as np
import pytest

from helpers import ADVERSARIAL, ADVERSARIAL_EXTRA, CROSS, SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE, knn_certificate, needs_two_columns, oracle_lists

pytestmark = pytest.mark.gpu

KINDS = {**ADVERSARIAL, **ADVERSARIAL_EXTRA}
ALL = tuple(sorted(KINDS))
#: the kinds every form of every family meets
CORE = ("heavy_tails", "tight_clusters", "subnormal_fp16_coords", "lattice_ties", "jittered_lattice")
#: the generators of separate query and reference sets that are not a one-set kind against a Gaussian
#: the two kinds whose Gaussian partner had to take the kind's spread (helpers.PARTNER_SCALE), against a UNIT Gaussian after all -- the
#: partner sets the scale and the kind vanishes below fp16 resolution -- with few enough queries and K = 1 that the oracle can order every row
UNIT_PARTNER = ("tiny_scale_unit_refs", "huge_scale_offset_unit_queries")
CROSS_OWN = ("far_queries", "query_outlier_sets_scale", "refs_in_a_speck", "queries_on_refs", "lattice_queries", "lattice_refs")

# self modes of a case.  One buffer: "exclude", "include", "none" (the own row found like any other).  "shard": rows [n/3, n/3 + n/2)
# of the set as queries with self_offset.  Separate sets (SELF_NONE): "asq" / "asr" -- the kind as the queries / the references of a
# Gaussian set -- and "cross" for the CROSS_OWN generators.
ONE_BUFFER = ("exclude", "include", "none")
SEPARATE = ("asq", "asr")

OFF, FORCE = 1, 2      # set_sym_mode / set_prune_mode: never, whenever possible
# family -> (sym mode, prune mode, what last_kernel() must match, what it must not)
FAMILIES = {
    "sweep": (OFF, OFF, r"^knn_f16_kernel<", r"symmetric|pruned| wide"),
    "wide": (OFF, OFF, r"^knn_f16_kernel<KST=1,KCAP=4> .* qt=4 .* wide", r"symmetric|pruned"),
    "panel": (FORCE, OFF, r"^knn_f16_kernel<.*> symmetric panel-kernel", r"pruned"),
    "sym2": (FORCE, OFF, r"^knn_f16_kernel<.*> symmetric(?! panel-kernel)", r"pruned"),
    "walk": (OFF, FORCE, r"^knn_f16_kernel<KST=1,.*> pruned ", r"symmetric"),
    "deep": (OFF, OFF, r"^knn_deep_kernel<", r"symmetric|pruned"),
}
# (family, form) -> (environment, what last_kernel() must match on top, what it must not).  Two forms cannot be told from the string:
# MCE_PANEL_DEBUG is not part of it, so the "redo" cases rest on the variable being read (a library that stopped reading it would make
# them repeats of "default"), and " bucket=512" shows the small buckets that force the repair launch, not the launch itself.  The
# library exposes neither count; mce_last_search_stats would be the place.
FORMS = {
    ("sweep", "unseeded"): (dict(MCE_F16_SEED_ROWS="0", MCE_RSPLIT="1"), r" rsplit=1($| )", r" seed=|two passes|\+ tail"),
    ("sweep", "seeded"): ({}, r" seed=\d+x\d+", r"two passes|\+ tail"),                              # (the default: split and seeded)
    ("sweep", "seedforced"): (dict(MCE_F16_SEED_SHARE="2", MCE_F16_SEED_ROWS="4096", MCE_F16_SEED_TG="1"), r" seed=\d+x1($| )", r"two passes|\+ tail"),
    ("sweep", "tail"): ({}, r"\+ tail", r"two passes"),
    ("sweep", "twopass"): ({}, r" two passes", r"\+ tail"),
    ("wide", "separate"): ({}, r"", r"two passes"),
    ("wide", "onebuffer"): ({}, r"", r"two passes"),
    ("panel", "default"): ({}, r"", r"two passes"),
    ("panel", "repair"): (dict(MCE_SYM_BUCKET="1"), r" bucket=512($| )", r"two passes"),           # (buckets far too small: the repair launch)
    ("panel", "redo"): (dict(MCE_PANEL_DEBUG="8"), r"", r"two passes"),                              # (every candidate through the redo list)
    ("panel", "units"): (dict(MCE_SYM_PANEL="4"), r" panel=4 ", r"two passes"),                      # (many units per block)
    ("panel", "twopass"): ({}, r"panel-kernel two passes", r"^$"),
    ("sym2", "default"): (dict(MCE_SYM_KERNEL="f16"), r"", r"two passes"),
    ("walk", "default"): ({}, r" heavy=0x", r"^$"),
    ("walk", "short"): (dict(MCE_PRUNE_LISTS="short"), r" lists=(9|10)$", r"^$"),                    # (K = 9, 10: list entries in registers)
    ("walk", "long"): (dict(MCE_PRUNE_LISTS="long"), r" lists=12$", r"^$"),
    ("walk", "heavy"): (dict(MCE_PRUNE_HEAVY="64,3"), r" heavy=[1-9]\d*x3 ", r"^$"),                 # (the first waves served by three workgroups each)
    ("deep", "default"): ({}, r"", r"^$"),
    ("deep", "split3"): (dict(MCE_RSPLIT="3"), r" rsplit=3($| )", r"^$"),
}

# The matrix.  A row is the full product kinds x dims; forms, K and self modes are DEALT over that product as the digits of a
# mixed-radix counter (forms fastest), so they are spread, not multiplied in, and every combination of the three comes up where
# the product is long enough.  n: rows of the set (references); separate sets and shards take about three quarters / half as
# many queries, `nq` overrides.  HP_RHO dimensions (fewer than three norm pieces fit: d = 14, 15 mod 16) are in every dims list
# that reaches them.  Which (form, K, self mode) a kind meets at a dimension is therefore not written in the table, and it shifts for all
# later cases of a row when a kind or a dimension is inserted: tests/test_oracle_certificate.py::test_gpu_matrix_coverage pins what
# must come out (every form with the core kinds, every K, every self mode), and `pytest --collect-only -q` lists the outcome.
K16 = (1, 4, 8, 9, 12, 16)         # every list capacity: KCAP 4, 4, 8, 12, 12, 16
MATRIX = [
    # --- exhaustive sweep: one, two, three and four k-steps with their HP_RHO dimensions; smallest size at which K = 16 is seeded by default
    dict(family="sweep", forms=("seeded", "unseeded", "seedforced"), kinds=ALL, dims=(1, 13, 14, 15, 29, 30, 31, 45, 46, 47, 61, 62, 63), K=K16,
         selfs=("exclude", "include", "asq", "shard", "asr"), n=6000),
    dict(family="sweep", forms=("twopass",), kinds=CORE, dims=(15, 31, 47, 63), K=(17, 32), selfs=("exclude", "asr", "include"), n=6000),
    dict(family="sweep", forms=("seeded", "unseeded", "seedforced"), kinds=CROSS_OWN, dims=(1, 6, 15, 31, 47, 63), K=K16, selfs=("cross",), n=6000),
    dict(family="sweep", forms=("tail",), kinds=CORE, dims=(6,), K=(9,), selfs=("asq",), n=30000, nq=135000),       # (264 query blocks: a tail of 8)
    dict(family="sweep", forms=("seeded",), kinds=CORE + ("one_outlier",), dims=(27,), K=(9,), selfs=("exclude",), n=40037),   # several chunks and splits, ragged
    dict(family="sweep", forms=("seeded", "unseeded", "seedforced"), kinds=CORE, dims=(2, 6), K=(9, 4, 16), selfs=("exclude", "asr", "include"), n=30011),  # dense at low d
    dict(family="sweep", forms=("seeded", "unseeded"), kinds=UNIT_PARTNER, dims=(2, 6, 31), K=(1,), selfs=("cross",), n=3000, nq=64),   # (see UNIT_PARTNER)
    # --- wide sweep: four query tiles per wave from 480 query blocks on, K <= 4, one k-step
    #     (481 query blocks against a small reference set; the generators in which every pair is a candidate -- 1e9 pairs here -- against a smaller one)
    dict(family="wide", forms=("separate",), kinds=ALL, dims=(1, 6, 13), K=(4, 1, 3), selfs=("asq",), n=20000, nq=246000),
    dict(family="wide", forms=("separate",), kinds=CROSS_OWN, dims=(1, 6, 13), K=(3, 4, 1), selfs=("cross",), n=4000, nq=246000),
    dict(family="wide", forms=("onebuffer",), kinds=CORE, dims=(6,), K=(3, 4), selfs=("exclude", "include"), n=246000),
    # --- symmetric sweep, panel kernel
    dict(family="panel", forms=("default", "repair", "redo", "units"), kinds=ALL, dims=(2, 6, 15, 27, 31, 47, 63), K=(9, 1, 4, 12, 16),
         selfs=ONE_BUFFER, n=6000),
    dict(family="panel", forms=("twopass",), kinds=CORE, dims=(6, 15, 31, 47, 63), K=(17, 24, 32), selfs=ONE_BUFFER, n=6000),
    dict(family="panel", forms=("default",), kinds=CORE + ("one_outlier", "anisotropic"), dims=(27,), K=(9,), selfs=("exclude",), n=40037),  # several panels, ragged
    # --- symmetric sweep, round-2 kernel
    dict(family="sym2", forms=("default",), kinds=ALL, dims=(6, 27), K=(9, 4, 16), selfs=ONE_BUFFER, n=6000),
    # --- pruned walk: d = 1 .. 8 the per-query reach variants, 9 and 13 box tests only, 14 and 15 its limit (K <= 16: no second pass)
    dict(family="walk", forms=("default",), kinds=ALL, dims=(1, 2, 3, 6, 8, 9, 13, 14, 15), K=(4, 1, 8, 12, 16),
         selfs=("exclude", "asq", "include", "asr", "shard", "none"), n=6000),
    dict(family="walk", forms=("short",), kinds=CORE, dims=(2, 15), K=(9, 10), selfs=("exclude", "asr", "include", "asq"), n=6000),
    dict(family="walk", forms=("long",), kinds=CORE, dims=(6, 15), K=(10, 9), selfs=("include", "asq", "exclude", "asr"), n=6000),
    dict(family="walk", forms=("default",), kinds=CROSS_OWN, dims=(2, 8, 14), K=(4, 9, 16), selfs=("cross",), n=6000),
    dict(family="walk", forms=("default",), kinds=UNIT_PARTNER, dims=(2, 6), K=(1,), selfs=("cross",), n=3000, nq=64),
    dict(family="walk", forms=("heavy",), kinds=CORE, dims=(3,), K=(9,), selfs=("exclude",), n=33333),                 # (66 query blocks: heavy waves need 64)
    # --- deep filter: 5, 6 and 8 k-steps; K = 24 in two passes
    dict(family="deep", forms=("default", "split3"), kinds=ALL, dims=(64, 80, 100, 127), K=(6, 16, 24), selfs=("exclude", "asq", "include", "asr", "shard"), n=3000),
    dict(family="deep", forms=("default", "split3"), kinds=CROSS_OWN, dims=(64, 80, 100), K=(6, 16, 24), selfs=("cross",), n=3000),
    dict(family="deep", forms=("default", "split3"), kinds=UNIT_PARTNER, dims=(64, 100), K=(1,), selfs=("cross",), n=3000, nq=64),
]


def expand(matrix=MATRIX):
    """the cases of the matrix: dicts (family, form, kind, d, K, self, n, nq)"""
    cases = []
    for row in matrix:
        nf, nk = len(row["forms"]), len(row["K"])
        stride = len(row["kinds"])                             # counter steps per dimension: coprime to the number of forms, so that a
        while math.gcd(stride, nf) != 1:                       # kind does not meet the same form at every dimension
            stride += 1
        for idim, d in enumerate(row["dims"]):
            for ikind, kind in enumerate(row["kinds"]):
                if d == 1 and needs_two_columns(kind):
                    continue                                   # (needs at least two columns)
                i = idim * stride + ikind
                form, K, self_ = row["forms"][i % nf], row["K"][i // nf % nk], row["selfs"][i // (nf * nk) % len(row["selfs"])]
                n = row["n"]
                nq = row.get("nq") or (n if self_ in ONE_BUFFER else n // 2 if self_ == "shard" else 3 * n // 4 + 5)
                if kind == "query_outlier_sets_scale" and not row.get("nq"):      # (the filter passes nearly everything: few queries)
                    nq = min(nq, 1000)
                cases.append(dict(family=row["family"], form=form, kind=kind, d=d, K=K, self=self_, n=n, nq=nq))
    return cases


def case_id(c):
    return "%(family)s-%(form)s-%(kind)s-d%(d)d-K%(K)d-%(self)s-n%(n)d" % c


CASES = expand()


def inputs(c, KINDS=KINDS, CROSS=CROSS):
    """(X, Y, self_mode, self_offset) of a case; X is Y (the same array) for one buffer.  KINDS, CROSS: the generator tables
    (tests/test_gpu_adversarial_f64.py brings one more kind)"""
    rng = np.random.default_rng(zlib.crc32(("%(kind)s-%(d)d-%(n)d-%(self)s" % c).encode()))
    n, nq, d, kind = c["n"], c["nq"], c["d"], c["kind"]
    if c["self"] in ("asq", "asr", "cross"):
        name = kind if c["self"] == "cross" else kind + ("_as_queries" if c["self"] == "asq" else "_as_refs")
        X, Y = CROSS[name](rng, nq, n, d)
        return np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64), SELF_NONE, 0
    Y = np.ascontiguousarray(KINDS[kind](rng, n, d), dtype=np.float64)
    if c["self"] == "shard":
        lo = n // 3
        return np.ascontiguousarray(Y[lo:lo + nq]), Y, SELF_EXCLUDE, lo
    return Y, Y, dict(exclude=SELF_EXCLUDE, include=SELF_INCLUDE, none=SELF_NONE)[c["self"]], 0


def expected_kernel(c):
    """regular expressions last_kernel() must match: the family, the form, the k-step count and the list capacity"""
    d, K = c["d"], c["K"]
    kst = (d + 1 + 15) // 16                                   # 16-wide k-steps over d coordinates and at least one norm piece
    if c["family"] == "deep":
        kst = 8 if kst == 7 else kst                           # (5, 6, 8: seven would not tile the staging buffer)
    kcap = 16 if K > 12 else 12 if K > 8 else 8 if K > 4 else 4
    fam = FAMILIES[c["family"]]
    env, must, must_not = FORMS[c["family"], c["form"]]
    want = [fam[2], r"<KST=%d,KCAP=%d>" % (kst, kcap), must]
    if c["family"] in ("sweep", "deep"):
        want.append(r" two passes" if K > 16 else r"^(?!.* two passes)")
    return want, [fam[3], must_not]


@pytest.fixture()
def lib():
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    _capi.set_search_mode(_capi.MODE_AUTO)
    yield _capi
    _capi.set_sym_mode(_capi.SYM_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_adversarial_every_row(case, lib, monkeypatch):
    X, Y, sm, off = inputs(case)
    K = case["K"]
    # the reference first and alone: how many rows it cannot order (at most 1e-5 of them, or the case is refused)
    oracle = oracle_lists(X, Y, K, sm, off)
    sym, prune = FAMILIES[case["family"]][:2]
    lib.set_sym_mode(sym)
    lib.set_prune_mode(prune)
    for name, val in FORMS[case["family"], case["form"]][0].items():
        monkeypatch.setenv(name, val)
    dist, idx = lib.knn(X, Y, K, self_mode=sm, self_offset=off)
    kernel = lib.last_kernel()
    want, unwanted = expected_kernel(case)
    for pat in want:
        assert re.search(pat, kernel), (pat, kernel)
    for pat in unwanted:
        assert not re.search(pat, kernel), (pat, kernel)
    report = knn_certificate(X, Y, K, dist, idx, sm, off, kernel=kernel, oracle=oracle)
    print("certified %d rows, %d ambiguous, B = %.3g; %s" % (report["rows"], report["ambiguous"], report["B"], kernel))
    assert lib.verify_knn(X, Y, dist, self_mode=sm, self_offset=off, nsample=len(X)) == 0, kernel
