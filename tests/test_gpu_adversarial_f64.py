"""The three kernel families outside tests/test_gpu_adversarial.py on the same hard inputs, EVERY row judged: the fp64 MFMA sweep
(knn_mfma_kernel, search mode 1), the long-row sweep (knn_long_kernel, the default for 128 <= d <= 1024) and the plain exact
kernel (knn_generic_kernel, the default for K > 32).  The two sweeps select K + m entries on GEMM-form keys and refine them, so
they are judged by the margin-aware certificate of tests/helpers.py (knn_certificate(margin=m): C1 - C4 on every row that is
neither oracle- nor key-ambiguous, C1, C2 and C3w on the others; the pairs of helpers.WEAK on every row by C1, C2, C3w); the
generic kernel's keys are exact and it gets the plain C1 - C4.  Every case asserts on last_kernel() that the family and variant
it is about actually ran, and the library's run-time certificate on all rows where it supports the shape.
tests/test_oracle_certificate.py checks on the host what the matrix covers and which pairs need WEAK.  Needs a real MI355X."""
import re

import numpy as np
import pytest

from helpers import (ADVERSARIAL, ADVERSARIAL_EXTRA, CROSS, WEAK, knn_certificate, offset_clusters, oracle_lists, refine_margin)
from test_gpu_adversarial import CORE, CROSS_OWN, ONE_BUFFER, UNIT_PARTNER, case_id, expand, inputs

pytestmark = pytest.mark.gpu

#: separation of offset_clusters per dimension: the largest of helpers.OFFSET_SCALES at which no row of any of this matrix's
#: offset_clusters cases of that dimension is key-ambiguous (tests/test_oracle_certificate.py::test_offset_scales_are_the_largest_clean_ones)
OFFSET_S = {1: 3, 2: 100, 3: 100, 4: 100, 7: 100, 8: 100, 15: 100, 16: 100, 27: 30, 31: 100, 32: 100, 47: 100, 63: 30, 64: 100, 79: 100, 80: 100,
            100: 100, 127: 100, 128: 30, 129: 30, 159: 100, 160: 30, 161: 30, 255: 30, 256: 100, 511: 10, 1024: 10,
            6: 30, 33: 30, 200: 30}          # (the last three: the generic kernel only, whose keys are exact)


def _offset_clusters(r, n, d):
    return offset_clusters(OFFSET_S[d])(r, n, d)


KINDS = {**ADVERSARIAL, **ADVERSARIAL_EXTRA, "offset_clusters": _offset_clusters}
CROSS_F64 = dict(CROSS)
CROSS_F64["offset_clusters_as_queries"] = lambda r, nq, nr, d: (_offset_clusters(r, nq, d), r.standard_normal((nr, d)))
CROSS_F64["offset_clusters_as_refs"] = lambda r, nq, nr, d: (r.standard_normal((nq, d)), _offset_clusters(r, nr, d))
ALL = tuple(sorted(KINDS))
#: what every row beyond a family's first meets: few_distinct gives duplicates at a non-zero centred position (keys that can come
#: out slightly negative at the high-dword gate), as queries_on_refs does among the separate sets
ELSE = CORE + ("offset_clusters", "few_distinct")
#: the kinds of the K = 31 (m = 1) and K = 32 (m = 0) rows: no row key-ambiguous with so little margin (offset_clusters has one at
#: m = 0 even at S = 1, tight_clusters and lattice_ties are weak anyway)
THIN = ("heavy_tails", "subnormal_fp16_coords", "jittered_lattice", "few_distinct", "anisotropic", "all_identical")

SELFS = ("exclude", "include", "none", "shard", "asq", "asr")
MFMA_K = (1, 2, 6, 10, 14, 22, 30, 9)      # list capacities 4, 4, 8, 12, 16, 24, 32, 12 (K + 2 entries); eight, so that the self modes rotate over a kind's dimensions
LONG_K = (1, 6, 7, 14, 15, 30, 9, 22)      # KCAP 8, 8, 16, 16, 32, 32, 16, 32: CT = 8 and 4 (eight: as MFMA_K)
NARROW = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 47, 63)          # KS = 1, 1, 1, 2, 2, 3, 4, 5, 8, 9, 12, 16
WIDE = (64, 79, 80, 100, 127)                                 # KS = 20, 20, 24, 28, 32: one query tile per wave
LONG = (128, 129, 159, 160, 161, 255, 256)                    # 5 .. 9 blocks of 7 or 8 k-steps, padded and unpadded last steps
LONGER = (511, 1024)                                          # 16 and 33 blocks

# family -> (search mode, what last_kernel() starts with)
FAMILIES = {"mfma": (1, r"^knn_mfma_kernel<"), "long": (0, r"^knn_long_kernel<"), "generic": (0, r"^knn_generic_kernel ")}

# The matrix, dealt by test_gpu_adversarial.expand: a row is the product kinds x dims, with K and self modes spread over it.  The
# forms here only name the variant group a row is about (the k-step count and the list capacity follow from d and K: expected_kernel).
MATRIX = [
    # --- fp64 MFMA sweep, two query tiles per wave (d <= 63)
    dict(family="mfma", forms=("narrow",), kinds=ALL, dims=NARROW, K=MFMA_K, selfs=SELFS, n=3000),
    dict(family="mfma", forms=("narrow",), kinds=THIN, dims=(3, 16, 31, 63), K=(31, 32), selfs=SELFS, n=3000),
    dict(family="mfma", forms=("narrow",), kinds=CROSS_OWN, dims=(2, 7, 16, 47, 63), K=MFMA_K, selfs=("cross",), n=3000),
    dict(family="mfma", forms=("narrow",), kinds=UNIT_PARTNER, dims=(2, 31), K=(1,), selfs=("cross",), n=3000, nq=64),
    dict(family="mfma", forms=("narrow",), kinds=ELSE + ("one_outlier",), dims=(27,), K=(9,), selfs=("exclude",), n=40037),   # several chunks and splits, ragged
    # --- its wide form (64 <= d <= 127)
    dict(family="mfma", forms=("wide",), kinds=ELSE, dims=WIDE, K=(6, 14, 22, 30, 1, 2, 10), selfs=SELFS, n=3000),
    dict(family="mfma", forms=("wide",), kinds=THIN, dims=(64, 100), K=(32, 31), selfs=SELFS, n=3000),
    dict(family="mfma", forms=("wide",), kinds=CROSS_OWN, dims=(64, 100, 127), K=(6, 22, 10), selfs=("cross",), n=3000),
    dict(family="mfma", forms=("wide",), kinds=UNIT_PARTNER, dims=(100,), K=(1,), selfs=("cross",), n=3000, nq=64),
    # --- long-row sweep
    dict(family="long", forms=("split",), kinds=ALL, dims=LONG, K=LONG_K, selfs=SELFS, n=3000),
    dict(family="long", forms=("split",), kinds=ELSE, dims=LONGER, K=(6, 15, 30, 1, 7, 14), selfs=SELFS, n=1500),
    dict(family="long", forms=("split",), kinds=THIN, dims=(128, 160, 255), K=(31, 32), selfs=SELFS, n=3000),
    dict(family="long", forms=("split",), kinds=CROSS_OWN, dims=(128, 161, 256), K=(6, 15, 30), selfs=("cross",), n=3000),
    dict(family="long", forms=("split",), kinds=UNIT_PARTNER, dims=(128, 256), K=(1,), selfs=("cross",), n=3000, nq=64),
    dict(family="long", forms=("small",), kinds=CORE, dims=(129,), K=(6, 15), selfs=("exclude", "include", "asr"), n=300),
    dict(family="long", forms=("unsplit",), kinds=CORE, dims=(129,), K=(6, 14), selfs=("exclude", "include", "asr"), n=100),   # (one chunk: rsplit=1)
    # --- plain exact kernel: K > 32; n no multiple of its 32-row tile or its 128-query block; d across the 32-dimension pass
    dict(family="generic", forms=("default",), kinds=ALL, dims=(1, 6, 31, 32, 33, 64, 200), K=(33, 40, 64), selfs=SELFS, n=3001),
    dict(family="generic", forms=("default",), kinds=("all_identical", "few_distinct"), dims=(6, 33), K=(33, 40), selfs=("include",), n=3001),
    dict(family="generic", forms=("default",), kinds=CROSS_OWN, dims=(6, 64), K=(33, 64), selfs=("cross",), n=3001),
]
CASES = expand(MATRIX)


def self_class(c):
    return "one" if c["self"] in ONE_BUFFER + ("shard",) else c["self"]


def margin_of(c):
    """entries the family's lists keep beyond K; None: exact keys (plain C1 - C4)"""
    return None if c["family"] == "generic" else refine_margin(c["K"])


def is_weak(c):
    return c["family"] != "generic" and (c["kind"], self_class(c)) in WEAK


def case_inputs(c):
    return inputs(c, KINDS, CROSS_F64)


def case_oracle(c, X, Y, sm, off):
    m = margin_of(c)
    return oracle_lists(X, Y, c["K"], sm, off) if m is None else oracle_lists(X, Y, c["K"], sm, off, margin=m, weak=is_weak(c))


def long_blocks(d):
    """(k-steps per block, padded k-steps per row) of the long-row sweep (knn_long.hpp)"""
    ks = (d + 1 + 3) // 4
    nkb = (ks + 7) // 8
    ksb = (ks + nkb - 1) // nkb
    return ksb, nkb * ksb


def expected_kernel(c):
    """regular expressions last_kernel() must match, and must not: the family, its variant and rsplit"""
    d, K = c["d"], c["K"]
    ksel = K + (margin_of(c) or 0)
    want, unwanted = [FAMILIES[c["family"]][1]], []
    if c["family"] == "mfma":
        ks = (d + 1 + 3) // 4 if d <= 63 else 4 * ((d + 1 + 15) // 16)
        kcap = min(k for k in (4, 8, 12, 16, 24, 32) if k >= ksel)
        want += [r"^knn_mfma_kernel<KS=%d,KCAP=%d> " % (ks, kcap), r" qt=%d " % (2 if c["form"] == "narrow" else 1), r" rsplit=\d+$"]
    elif c["family"] == "long":
        kcap = 8 if ksel <= 8 else 16 if ksel <= 16 else 32
        want += [r"^knn_long_kernel<KCAP=%d> " % kcap, r" ct=%d " % (4 if kcap == 32 else 8), r" ksp=%d$" % long_blocks(d)[1], r" rsplit=\d+ "]
        if c["form"] == "split":
            unwanted.append(r" rsplit=1 ")
        elif c["form"] == "unsplit":
            want.append(r" rsplit=1 ")
    else:
        want.append(r"^knn_generic_kernel grid=%d block=128 " % ((c["nq"] + 127) // 128))
    return want, unwanted


@pytest.fixture()
def lib():
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    yield _capi
    _capi.set_search_mode(_capi.MODE_AUTO)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_adversarial_every_row_f64(case, lib):
    """One case of MATRIX: the family and variant asserted on last_kernel(), every row by knn_certificate, and the library's run-time
    certificate on all rows where it supports the shape.  The latter is stricter than C3w on the WEAK pairs (1e-9 relative against
    exact distances): tight_clusters at d = 1 and 2 pass it only because the merge takes an exact second look at every row whose last
    selected key does not prove the K reported complete (reduce_kernels.hpp) -- without it 139 of 3000 and 1 of 1500 rows failed there."""
    X, Y, sm, off = case_inputs(case)
    K, m, weak = case["K"], margin_of(case), is_weak(case)
    # the reference first and alone: how many rows it cannot order, how many the keys cannot (a strict case with more than 1e-5 of either is refused)
    oracle = case_oracle(case, X, Y, sm, off)
    lib.set_search_mode(FAMILIES[case["family"]][0])
    dist, idx = lib.knn(X, Y, K, self_mode=sm, self_offset=off)
    kernel = lib.last_kernel()
    want, unwanted = expected_kernel(case)
    for pat in want:
        assert re.search(pat, kernel), (pat, kernel)
    for pat in unwanted:
        assert not re.search(pat, kernel), (pat, kernel)
    report = knn_certificate(X, Y, K, dist, idx, sm, off, kernel=kernel, oracle=oracle, margin=m, weak=weak)
    print("certified %d rows%s, %d ambiguous, %d key-ambiguous, B = %.3g, max 2E = %.3g; %s" % (
        report["rows"], " weakly" if weak else "", report["ambiguous"], report["key_ambiguous"], report["B"],
        0.0 if m is None else 2.0 * float(np.max(oracle[4])), kernel))
    if case["d"] <= 128 and K <= 32:
        assert lib.verify_knn(X, Y, dist, self_mode=sm, self_offset=off, nsample=len(X)) == 0, kernel
