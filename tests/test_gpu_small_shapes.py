"""Every search family at its SMALLEST shapes, every row judged by the certificate of tests/helpers.py.  The three every-row matrices
(tests/test_gpu_adversarial.py, _f64.py, _sums.py) run at sizes chosen for the data: n = 3000, 6000 or more.  The special cases of
the code live below that: reference sets that fill no list (nr == K, the gate +inf for the whole sweep, only `j < nr` between a
padding row and the result), a last tile, chunk or query block with one row in it, a second symmetric block of one row, one chunk
(rsplit = 1 whatever is asked), fewer usable rows than the K + m entries the fp64 sweeps keep.  Here every family is forced, as in
the two kNN matrices (their FAMILIES, FORMS, inputs, case_oracle, margin_of and is_weak are reused), at reference and query counts
on both sides of every such edge, with the kinds whose padding rows are NEARER than real ones (one_outlier, huge_scale_offset: a
padding row sits at the centre) or tie with them (few_distinct, all_identical, lattice_ties).

The matrix is one table (MATRIX).  A row lists kinds, dimensions, forms, K, reference-row counts, query counts and self modes; ALL of
them are dealt from one counter (deal: attribute k of step j is j modulo m_k, the m_k pairwise coprime and each the smallest that
holds its list, so that every attribute moves from one case to the next, every pair of attributes comes up within m_k m_l steps and
the full product in the long run) over `cases` steps -- not a full product.  tests/test_oracle_small_shapes.py pins on the host what must come out (every reference-row class, query class, self
mode and list capacity per family; nr == U with the three padding kinds) and that every case is clean on the oracle alone: at these
sizes the cap of 1e-5 ambiguous rows means NONE.

Reference-row tokens: U = the smallest legal count (K, or K + 1 where the own row is excluded), C = the rows of one staged chunk of
the variant (taken from the code's constants, mirrored in chunk_rows and held to ` ct=` of last_kernel()).  A K that a size cannot
serve (U > nr) is replaced by the largest K of the row that it can.  Needs a real MI355X: run with -m gpu."""
import math
import re

import pytest

import test_gpu_adversarial as A
import test_gpu_adversarial_f64 as F
from helpers import knn_certificate, needs_two_columns, oracle_lists
from test_gpu_adversarial import ONE_BUFFER

pytestmark = pytest.mark.gpu

#: the kinds of this matrix: padding rows nearer than real rows (the first two), duplicates and ties (the next four), fp16 underflow
EDGE3 = ("one_outlier", "huge_scale_offset", "few_distinct")
KINDS7 = EDGE3 + ("all_identical", "heavy_tails", "lattice_ties", "subnormal_fp16_coords")
#: ... of the K = 31 and 32 rows of the fp64 sweeps (m = 1 and 0): one_outlier is key-ambiguous there on the oracle alone
THIN = ("huge_scale_offset", "few_distinct", "all_identical", "heavy_tails", "subnormal_fp16_coords")
CROSS_KIND = "queries_on_refs"          # the one generator of separate sets that is no one-set kind against a Gaussian
ALL_SELFS = ("exclude", "include", "none", "shard", "asq", "asr", "cross")
SEPARATE = ("asq", "asr", "cross")
FP16 = tuple(A.FAMILIES)                # sweep, wide, panel, sym2, walk, deep
F64 = tuple(F.FAMILIES)                 # mfma, long, generic


# ---- the code's geometry, mirrored (each is held to the kernel string: ` ct=`, `KST=`, `KS=`, `KCAP=`) --------------------------
def ksteps(c):
    """16-wide k-steps of the fp16 filter (knn_f16.hpp f16_ksteps, knn_deep.hpp deep_ksteps)"""
    kst = (c["d"] + 1 + 15) // 16
    return 8 if c["family"] == "deep" and kst == 7 else kst


def f16_kcap(K):
    return 16 if K > 12 else 12 if K > 8 else 8 if K > 4 else 4


def mfma_ks(d):
    return (d + 1 + 3) // 4 if d <= 63 else 4 * ((d + 1 + 15) // 16)


def mfma_kcap(K):
    return min(k for k in (4, 8, 12, 16, 24, 32) if k >= K + F.refine_margin(K))


def mfma_chunk_tiles(KS, KCAP):
    """knn_mfma.hpp chunk_tiles: A-fragments per staging buffer over the k-steps, even, at least two"""
    frag = (64 if KCAP > 16 else 128) if KS > 16 else (32 if KCAP > 16 else 64)
    return max(2, frag // KS // 2 * 2)


def long_kcap(K):
    ksel = K + F.refine_margin(K)
    return 8 if ksel <= 8 else 16 if ksel <= 16 else 32


def chunk_tiles(c, K=None):
    """reference tiles per staged chunk (` ct=` of the kernel string); None: the plain exact kernel stages no chunks"""
    K = c["K"] if K is None else K
    fam = c["family"]
    if fam in ("sweep", "wide", "panel", "sym2"):
        return 48 // ksteps(c)                                  # f16_chunk_tiles: 48 KB per buffer
    if fam == "walk":
        return 64                                               # kHPruneChunkTiles: a list entry is an aligned k-d subtree of 2048 rows
    if fam == "deep":
        return {5: 8, 6: 8, 8: 6}[ksteps(c)]                    # deep_chunk_tiles
    if fam == "mfma":
        return mfma_chunk_tiles(mfma_ks(c["d"]), mfma_kcap(K))
    if fam == "long":
        return 4 if long_kcap(K) == 32 else 8                   # long_ct
    return None


def chunk_rows(c, K=None):
    ct = chunk_tiles(c, K)
    return None if ct is None else ct * (16 if c["family"] in ("mfma", "long") else 32)


def query_block(c):
    """queries per workgroup"""
    fam = c["family"]
    if fam == "mfma":
        return 256 if c["d"] <= 63 else 128                     # queries_per_block(qt): two query tiles per wave, one for KS > 16
    return {"long": 256, "generic": 128}.get(fam, 512)


def usable_min(K, self_):
    return K + 1 if self_ in ("exclude", "shard") else K


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
def sizes(**classes):
    """reference-row tokens by class -> ((token, class), ...)"""
    return tuple((tok, cls) for cls, toks in classes.items() for tok in toks)


SWEEP_NR = sizes(U=("U",), U1=("U+1",), U2=("U+2",), tile=(31, 32, 33), chunk=("C-1", "C", "C+1"), two=("2C+1",))
SWEEP_NQ = sizes(one=(1, 2), tile=(31, 32, 33), wave=(63, 64, 65), block=(511, 512, 513))
WIDE_NR = sizes(U=("U",), U1=("U+1",), tile=(31, 32, 33), chunk=(1537,))
WIDE_NQ = sizes(last1=(245249,), exact=(245760,), odd=(245761,))           # 480 blocks with one row in the last, exactly 480, 481 padded to 482
PANEL_N = sizes(first=(513, 514), tile=(544, 545), block=(1023, 1024, 1025), chunk=(1537,))
WALK_NR = sizes(U=("U",), U1=("U+1",), tile=(31, 32, 33), wave=(63, 64, 65), block=(511, 512, 513), chunk=(2047, 2048, 2049), two=(4097,))
WALK_NQ = sizes(one=(1,), wave=(63, 64, 65))
DEEP_NQ = sizes(one=(1,), block=(511, 512, 513))
MFMA_NR = sizes(U=("U",), U1=("U+1",), U2=("U+2",), U3=("U+3",), tile=(15, 16, 17), tile2=(31, 32, 33), chunk=("C-1", "C", "C+1"))
MFMA_NQ = sizes(one=(1,), block=("Q-1", "Q", "Q+1"))
LONG_NR = sizes(U=("U",), U1=("U+1",), U2=("U+2",), U3=("U+3",), tile=(15, 16, 17), chunk=(63, 64, 65), two=(127, 128, 129))
LONG_NQ = sizes(one=(1,), block=(255, 256, 257))
GEN_NR = sizes(U=("U",), U1=("U+1",), tile=(63, 64, 65), two=(127, 128, 129))
GEN_NQ = sizes(one=(1,), block=(127, 128, 129))
NO_NQ = sizes(same=(0,))               # one buffer only


def row(family, forms, kinds, dims, K, nr, nq, selfs, cases):
    return dict(family=family, forms=forms, kinds=kinds, dims=dims, K=K, nr=nr, nq=nq, selfs=selfs, cases=cases)


SW3 = ("seeded", "unseeded", "seedforced")
U_ONLY = sizes(U=("U",))
U_U1 = sizes(U=("U",), U1=("U+1",))
NOT_CROSS = ("exclude", "include", "none", "shard", "asq", "asr")
MATRIX = [
    # --- exhaustive fp16 sweep: one to four k-steps, every list capacity; two passes apart
    row("sweep", SW3, KINDS7, (1, 15, 31, 47, 63), (1, 4, 8, 9, 12, 16), SWEEP_NR, SWEEP_NQ, ALL_SELFS, 150),
    row("sweep", ("twopass",), KINDS7, (15, 31, 47, 63), (17, 32), SWEEP_NR, SWEEP_NQ, ALL_SELFS, 60),
    row("sweep", SW3, EDGE3, (1, 15, 63), (1, 9, 16), U_U1, SWEEP_NQ, NOT_CROSS, 36),
    row("sweep", ("twopass",), EDGE3, (15, 63), (17, 32), U_U1, SWEEP_NQ, NOT_CROSS, 36),
    # --- wide sweep: 480 query blocks and more against a tiny reference set (separate sets: the queries are the many)
    row("wide", ("separate",), KINDS7, (1, 6, 13), (1, 3, 4), WIDE_NR, WIDE_NQ, SEPARATE, 30),
    row("wide", ("separate",), EDGE3, (6,), (4, 1), U_U1, WIDE_NQ, ("asr", "asq"), 12),
    # --- symmetric sweep: n = 513 is the smallest set the plan admits (two query blocks, the second with ONE row)
    row("panel", ("default", "repair", "redo", "units"), KINDS7, (2, 15, 27, 63), (1, 9, 16), PANEL_N, NO_NQ, ONE_BUFFER, 96),
    row("panel", ("twopass",), KINDS7, (15, 27, 63), (17, 32), PANEL_N, NO_NQ, ONE_BUFFER, 32),
    row("panel", ("default", "repair", "redo", "units"), EDGE3, (2, 27), (1, 16), sizes(first=(513,)), NO_NQ, ONE_BUFFER, 12),
    row("sym2", ("default",), KINDS7, (2, 15, 27), (1, 9, 16), PANEL_N, NO_NQ, ONE_BUFFER, 32),
    row("sym2", ("default",), EDGE3, (2, 27), (1, 16), sizes(first=(513,)), NO_NQ, ONE_BUFFER, 6),
    # --- pruned walk, forced: sets smaller than one 2048-row chunk, one 64-query wave, one 32-row tile
    row("walk", ("default",), KINDS7, (1, 2, 3, 8, 9, 15), (1, 4, 9, 10, 16), WALK_NR, WALK_NQ, ALL_SELFS, 150),
    row("walk", ("short", "long"), KINDS7, (2, 9, 15), (9, 10), WALK_NR, WALK_NQ, ALL_SELFS, 48),
    row("walk", ("default", "long"), EDGE3, (1, 3, 15), (1, 10, 16), U_U1, WALK_NQ, NOT_CROSS, 36),
    # --- deep filter: 5, 6 and 8 k-steps; K = 17, 32 in two passes
    row("deep", ("default", "split3"), KINDS7, (64, 80, 127), (1, 6, 16, 17, 32), SWEEP_NR, DEEP_NQ, ALL_SELFS, 120),
    row("deep", ("default", "split3"), EDGE3, (64, 127), (1, 16, 32), U_U1, DEEP_NQ, NOT_CROSS, 36),
    # --- fp64 MFMA sweep: usable rows below, at and above the K + m entries its lists keep
    row("mfma", ("narrow",), KINDS7, (1, 3, 4, 16, 31, 63), (1, 2, 6, 14, 30), MFMA_NR, MFMA_NQ, ALL_SELFS, 130),
    row("mfma", ("narrow",), THIN, (3, 16, 63), (31, 32), MFMA_NR, MFMA_NQ, ALL_SELFS, 40),
    row("mfma", ("wide",), KINDS7, (64, 127), (1, 2, 6, 14, 30), MFMA_NR, MFMA_NQ, ALL_SELFS, 60),
    row("mfma", ("wide",), THIN, (64, 127), (31, 32), MFMA_NR, MFMA_NQ, ALL_SELFS, 20),
    row("mfma", ("narrow", "wide"), EDGE3, (3, 63, 64), (1, 14, 30), U_U1, MFMA_NQ, NOT_CROSS, 36),
    # --- long-row sweep
    row("long", ("default",), KINDS7, (128, 129, 1024), (1, 6, 7, 30), LONG_NR, LONG_NQ, ALL_SELFS, 90),
    row("long", ("default",), THIN, (128, 129), (31, 32), LONG_NR, LONG_NQ, ALL_SELFS, 30),
    row("long", ("default",), EDGE3, (128, 1024), (1, 7, 30), U_U1, LONG_NQ, NOT_CROSS, 36),
    # --- plain exact kernel
    row("generic", ("default",), KINDS7, (1, 33, 200), (33, 64, 100), GEN_NR, GEN_NQ, ALL_SELFS, 70),
    row("generic", ("default",), EDGE3, (1, 200), (33, 100), U_U1, GEN_NQ, NOT_CROSS, 36),
]

# Cases the oracle alone refused as dealt (an ambiguous or key-ambiguous row: at these sizes the cap of 1e-5 admits none), and what was
# changed, keyed by the id as dealt.  tests/test_oracle_small_shapes.py::test_small_matrix_is_clean_on_the_oracle_alone passes on the
# matrix as adjusted, and checks that every entry is used.
ADJUST = {
}


def resolve(tok, U, C, Q):
    if isinstance(tok, int):
        return tok
    m = re.fullmatch(r"(\d*)([UCQ])([+-]\d+)?", tok)
    base = {"U": U, "C": C, "Q": Q}[m.group(2)]
    return int(m.group(1) or 1) * base + int(m.group(3) or 0)


def mfma_form(d):
    return "narrow" if d <= 63 else "wide"


def deal(matrix=MATRIX, adjust=None):
    """the cases: dicts (family, form, kind, d, K, self, n, nq, cls, qcls, dealt).  n: reference rows; one buffer: nq == n, shard: n // 2"""
    adjust = ADJUST if adjust is None else adjust
    cases, seen = [], set()
    for r in matrix:
        lists = [r["kinds"], r["selfs"], r["nr"], r["nq"], r["forms"], r["K"], r["dims"]]
        # pairwise coprime moduli, each the smallest that holds its list: the residues of the counter then run through every pair of
        # attributes within the product of their two moduli, and through the full product in the long run
        mods = []
        for lst in lists:
            m = len(lst)
            while any(math.gcd(m, o) != 1 for o in mods):
                m += 1
            mods.append(m)
        j = made = 0
        while made < r["cases"]:
            pick = [lst[j % m % len(lst)] for lst, m in zip(lists, mods)]
            j += 1
            assert j < 100 * r["cases"], r
            kind, self_, (ntok, cls), (qtok, qcls), form, K, d = pick
            if r["family"] == "mfma":
                form = mfma_form(d) + form[form.index("/"):] if "/" in form else mfma_form(d)      # (the sums matrix: "form/W")
            if self_ == "cross":
                kind = CROSS_KIND
            if d == 1 and needs_two_columns(kind):
                continue                                       # (needs at least two columns)
            c = dict(family=r["family"], form=form, kind=kind, d=d, K=K, self=self_, cls=cls)
            n = resolve(ntok, usable_min(K, self_), chunk_rows(c), 0)
            if self_ == "shard" and n < 6:
                c["self"] = self_ = "exclude"                  # (rows [n / 3, n / 3 + n / 2) need n >= 6; the own row stays excluded: U is the same)
            if n < usable_min(K, self_):                       # this size cannot serve the K dealt: the largest K of the row that it can
                fit = [k for k in r["K"] if usable_min(k, self_) <= n]
                if not fit:
                    continue
                c["K"] = K = max(fit)
                n = resolve(ntok, usable_min(K, self_), chunk_rows(c), 0)
            c["n"] = n
            if self_ in ONE_BUFFER:
                c["nq"], c["qcls"] = n, "same"
            elif self_ == "shard":
                c["nq"], c["qcls"] = n // 2, "shard"
            else:
                if qcls == "same":
                    continue
                c["nq"], c["qcls"] = resolve(qtok, 0, 0, query_block(c)), qcls
            c["dealt"] = case_id(c)
            if c["dealt"] in adjust:
                c.update({k: v for k, v in adjust[c["dealt"]].items() if k != "reason"})
            if case_id(c) in seen:
                continue
            seen.add(case_id(c))
            cases.append(c)
            made += 1
    return cases


def case_id(c):
    return A.case_id(c) + ("" if c["self"] in ONE_BUFFER else "-q%d" % c["nq"])


CASES = deal()


def is_f64(c):
    return c["family"] in F.FAMILIES


def margin_of(c):
    """the f64 file's margin on its families; the fp16 filter's lists hold exact distances (plain C1 - C4)"""
    return F.margin_of(c) if is_f64(c) else None


def is_weak(c):
    return is_f64(c) and F.is_weak(c)


def case_inputs(c):
    return A.inputs(c, F.KINDS, F.CROSS_F64)


def case_oracle(c, X, Y, sm, off):
    return F.case_oracle(c, X, Y, sm, off) if is_f64(c) else oracle_lists(X, Y, c["K"], sm, off)


def modes_of(c):
    """(search mode, sym mode, prune mode, environment) that force the case's family and form"""
    if is_f64(c):
        return F.FAMILIES[c["family"]][0], A.OFF, A.OFF, {}
    sym, prune = A.FAMILIES[c["family"]][:2]
    return 0, sym, prune, A.FORMS[c["family"], c["form"]][0]


def nchunks(c):
    return -(-c["n"] // chunk_rows(c))


def expected_kernel(c):
    """(patterns last_kernel() must match, patterns it must not): the family, its KST / KS / KCAP and chunk tiles, and what the form's
    knob does at this size -- or, where it cannot apply (one chunk: rsplit = 1 whatever MCE_RSPLIT says), what the plan does instead.
    The seed, rsplit and tail parts are otherwise whatever the plan takes at the size."""
    fam, form, d, K = c["family"], c["form"], c["d"], c["K"]
    if fam == "generic":
        return [F.FAMILIES[fam][1], r"^knn_generic_kernel grid=%d block=128 " % max(1, -(-c["nq"] // 128))], []
    want, unwanted = [r" ct=%d " % chunk_tiles(c)], []
    if fam == "mfma":
        want += [r"^knn_mfma_kernel<KS=%d,KCAP=%d> " % (mfma_ks(d), mfma_kcap(K)), r" qt=%d " % (2 if form == "narrow" else 1)]
    elif fam == "long":
        want += [r"^knn_long_kernel<KCAP=%d> " % long_kcap(K), r" ksp=%d$" % F.long_blocks(d)[1]]
    else:
        env, must, must_not = A.FORMS[fam, form]
        want += [A.FAMILIES[fam][2], r"<KST=%d,KCAP=%d>" % (ksteps(c), f16_kcap(K))]
        unwanted += [A.FAMILIES[fam][3]]
        if fam in ("sweep", "deep"):
            want.append(r" two passes" if K > 16 else r"^(?!.* two passes)")
        if (fam, form) == ("sweep", "unseeded"):
            want.append(must)
            unwanted.append(r" seed=")
        elif (fam, form) == ("deep", "split3"):
            # MCE_RSPLIT=3 stands where the reference set has three chunks (two passes: rmax = min(8, nchunk)); below that the plan's own
            want.append(must if nchunks(c) >= 3 else r" rsplit=[12]($| )")
        elif fam == "panel" and form in ("units", "twopass", "repair"):
            want.append(must)
        elif fam == "walk":
            # nine or ten list entries in registers where K is 9 or 10 (MCE_PRUNE_LISTS=long: the list arrays' twelve); other K: the capacity
            want.append(r" lists=%d$" % (K if K in (9, 10) and form != "long" else f16_kcap(K)))
    if fam != "walk" and fam != "wide" and fam not in ("panel", "sym2") and nchunks(c) == 1:
        want.append(r" rsplit=1($| )")                           # one chunk: one split
    return want, unwanted


@pytest.fixture()
def lib():
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    yield _capi
    _capi.set_search_mode(_capi.MODE_AUTO)
    _capi.set_sym_mode(_capi.SYM_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


def run_case(lib, c, setenv):
    """one case: the oracle first and alone, the family forced, the search, the kernel string, the certificate on EVERY row, the
    library's run-time certificate on all rows where it supports the shape -> (kernel, report)"""
    X, Y, sm, off = case_inputs(c)
    K, m, weak = c["K"], margin_of(c), is_weak(c)
    assert len(Y) == c["n"] and len(X) == c["nq"]
    oracle = case_oracle(c, X, Y, sm, off)
    search, sym, prune, env = modes_of(c)
    lib.set_search_mode(search)
    lib.set_sym_mode(sym)
    lib.set_prune_mode(prune)
    for name, val in env.items():
        setenv(name, val)
    dist, idx = lib.knn(X, Y, K, self_mode=sm, self_offset=off)
    kernel = lib.last_kernel()
    want, unwanted = expected_kernel(c)
    for pat in want:
        assert re.search(pat, kernel), (pat, kernel)
    for pat in unwanted:
        assert not re.search(pat, kernel), (pat, kernel)
    report = knn_certificate(X, Y, K, dist, idx, sm, off, kernel=kernel, oracle=oracle, margin=m, weak=weak)
    assert report["ambiguous"] == 0 and (weak or report["key_ambiguous"] == 0)
    if c["d"] <= 128 and K <= 32:
        assert lib.verify_knn(X, Y, dist, self_mode=sm, self_offset=off, nsample=len(X)) == 0, kernel
    return kernel, report


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_small_shapes_every_row(case, lib, monkeypatch):
    kernel, report = run_case(lib, case, monkeypatch.setenv)
    print("SMALL %s: certified %d rows%s, %d ambiguous; %s" % (case_id(case), report["rows"], " weakly" if report["weak"] else "", report["ambiguous"], kernel))
