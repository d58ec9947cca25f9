"""The run-time certificate of a search on trial (verify_scan_kernel, verify_check_kernel, verify_row of
mcevidence_amd/csrc/verify_kernels.hpp, through mce_verify_knn_f64 and mce_verify_knn_f64_dev): every matrix asks it
`verify_knn(...) == 0`, and a judge that is too lax says so whatever it is shown.  Here it is shown WRONG lists.  The lists are the
host oracle's, corrupted by the catalogue of tests/verify_cases.py, and the expected verdict of every row is the host model's of the
documented rule in np.longdouble -- never an expectation written down here.  One table dealt from a counter (verify_cases.deal):
d = 1 .. 128 on both sides of the scan's unroll by 8, K = 1 .. 32, samples that are no multiple of the 16 queries of a workgroup and
reach past the 256 threads of the check kernel's first block, a reference split, shards with a self offset, duplicates of the own row,
eight adversarial kinds and one cross kind.  tests/test_oracle_verify.py holds, without a GPU, that no row of any case is undecided.

Every case asserts: the count over all rows, for the clean lists and every corruption; the verdict of single rows by one-row calls
(a failure names the row); the count over a partial sample, against the mirrored sampling pattern; and the device form on a dirty
workspace, twice on one stream.  Needs a real MI355X: run with -m gpu."""
import numpy as np
import pytest

import verify_cases as V
from helpers import SELF_EXCLUDE, SELF_INCLUDE, SELF_NONE

pytestmark = pytest.mark.gpu
SEEDS = lambda nq: (0, nq - 1, V.U64)


@pytest.fixture()
def lib():
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    return _capi


def one_row(lib, b, dist, q):
    """the library's verdict on query row q alone"""
    return lib.verify_knn(b.X[q:q + 1], b.Y, dist[q:q + 1], self_mode=b.sm, self_offset=b.off + q if b.sm == SELF_EXCLUDE else 0, nsample=1)


def dealt_rows(rows, j, n=3):
    """n rows of `rows` (fewer where it has fewer) dealt from the counter j"""
    rows = np.asarray(rows)
    return sorted({int(rows[(j + 5 * i) % len(rows)]) for i in range(n)}) if len(rows) else []


def device_form(lib, b, dist, nsample, seed):
    """mce_verify_knn_f64_dev on torch buffers, the workspace filled with 0xFF, twice on the current stream -> the two results"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    dX, dY, dD = dev(b.X), dev(b.Y), dev(dist)
    nq, K = dist.shape
    wsb = lib.verify_workspace_bytes(min(nsample, nq), K)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda:0")
    res = [torch.full((2,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    for r in res:
        rc = lib.verify_knn_dev(dX.data_ptr(), nq, dY.data_ptr(), len(b.Y), b.X.shape[1], K, b.sm, b.off, dD.data_ptr(), K, nsample, seed, r.data_ptr(),
                                ws.data_ptr(), wsb, stream)
        assert rc == lib.MCE_OK, lib.last_error()
    torch.cuda.synchronize()
    return [r.cpu().tolist() for r in res]


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_certificate_gives_the_models_verdict(case, lib):
    b = V.built(case)                                          # the model first and alone (refuses a case with an undecided row)
    nq, ns, j = case["nq"], case["ns"], case["step"]
    kw = dict(self_mode=b.sm, self_offset=b.off)
    what = V.case_id(case)
    # ---- all rows sampled: the clean lists, then every corruption
    assert not b.clean_fails.any()
    assert lib.verify_knn(b.X, b.Y, b.clean, nsample=nq, **kw) == 0, what
    outside = dealt_rows(np.setdiff1d(np.arange(nq), V.touched_rows(nq, j)), j)
    for q in outside:
        assert one_row(lib, b, b.clean, q) == 0, (what, "clean", q)
    counts = []
    for i, e in enumerate(b.entries):
        got = lib.verify_knn(b.X, b.Y, e.dist, nsample=nq, seed=(0, 1, nq - 1)[i % 3], **kw)
        counts.append((e.name, got, e.count))
        assert got == e.count, (what, e.name, "failing rows: got %d, the model %d" % (got, e.count))
        # ---- single rows of R (rows outside it hold the clean lists: judged above)
        for q in dealt_rows(e.R, j + i):
            assert one_row(lib, b, e.dist, q) == int(e.fails[q]), (what, e.name, "row %d" % q, e.dist[q].tolist())
    # ---- a partial sample: nq / 2 < n < nq, where a stride of nq / n would look at one contiguous block
    part = ns if ns < nq else nq // 2 + 1
    if part < nq:
        for e in (e for e in b.entries if e.name.startswith("spread")):
            for seed in SEEDS(nq):
                want = int(e.fails[V.sample_rows(part, nq, seed)].sum())
                assert lib.verify_knn(b.X, b.Y, e.dist, nsample=part, seed=seed, **kw) == want, (what, e.name, part, seed)
    # ---- the device form: one dealt corruption and the clean lists
    e = b.entries[j % len(b.entries)]
    for dist, fails in ((e.dist, e.fails), (b.clean, b.clean_fails)):
        for nsample, seed in ((nq, 0), (part, nq - 1), (nq + 3, V.U64)):
            n = min(nsample, nq)
            want = [n, int(fails[V.sample_rows(n, nq, seed)].sum())]
            assert device_form(lib, b, dist, nsample, seed) == [want, want], (what, e.name, nsample, seed)
            assert lib.verify_knn(b.X, b.Y, dist, nsample=nsample, seed=seed, **kw) == want[1]
    print("VERIFY %s: %d rows, %d lists; failing rows (got = model): %s" % (what, nq, 1 + len(b.entries), " ".join("%s=%d" % (n, g) for n, g, _ in counts)))


@pytest.mark.parametrize("p", V.PLANT_CASES, ids=V.plant_id)
def test_a_planted_neighbour_is_seen_at_every_split_boundary(p, lib):
    """reference rows planted as neighbours on both sides of every boundary a split of the scan can have, at the ends and around the
    first 256 rows; under exclude also next to the own row in memory.  The correct lists pass; with the planted row deleted, exactly
    the planted queries fail -- in the call on all rows (the launch's split count for 4 workgroups) and in one-row calls"""
    b = V.planted(p)
    kw = dict(self_mode=b.sm, self_offset=b.off)
    nq = len(b.X)
    assert lib.verify_knn(b.X, b.Y, b.clean, nsample=nq, **kw) == 0
    lost = b.entries[-1]
    assert lib.verify_knn(b.X, b.Y, lost.dist, nsample=nq, **kw) == lost.count == len(b.planted)
    for q, j, c in b.planted:
        assert one_row(lib, b, b.clean, q) == 0, ("planted row %d of query %d: the correct list" % (j, q))
        assert one_row(lib, b, lost.dist, q) == 1, ("planted row %d of query %d, column %d: its loss was not seen" % (j, q, c))
    for q in np.setdiff1d(np.arange(nq), lost.R)[::7]:
        assert one_row(lib, b, lost.dist, int(q)) == 0, q


def test_surplus_columns_of_a_short_reference_set_pass(lib):
    """catalogue h: K' = 5 columns on nr = 3 rows, the surplus +inf, pass; one +inf too many fails on every row"""
    Y = np.random.default_rng(5).standard_normal((3, 4))
    for sm, usable in ((SELF_NONE, 3), (SELF_INCLUDE, 3), (SELF_EXCLUDE, 2)):
        m = V.Model(Y, Y, sm)
        d = np.sort(np.sqrt(np.asarray(V.exact_d2(Y, Y), dtype=np.float64)), axis=1)[:, 3 - usable:]
        lists = np.full((3, 5), np.inf)
        lists[:, :usable] = d
        assert not m.judge(lists)[0].any() and lib.verify_knn(Y, Y, lists, self_mode=sm, nsample=3) == 0
        lists[:, usable - 1] = np.inf
        assert m.judge(lists)[0].all() and lib.verify_knn(Y, Y, lists, self_mode=sm, nsample=3) == 3


def test_refusals_launch_nothing(lib):
    import torch
    rng = np.random.default_rng(1)
    nq, nr = 20, 40
    res = torch.full((2,), -7, dtype=torch.int32, device="cuda:0")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")

    def call(d, K, ld, ws_bytes):
        dX, dY = (torch.from_numpy(rng.standard_normal((n, d))).to("cuda:0") for n in (nq, nr))
        dD = torch.ones((nq, max(ld, 1)), dtype=torch.float64, device="cuda:0")
        rc = lib.verify_knn_dev(dX.data_ptr(), nq, dY.data_ptr(), nr, d, K, lib.SELF_NONE, 0, dD.data_ptr(), ld, nq, 0, res.data_ptr(), ws.data_ptr(), ws_bytes, 0)
        torch.cuda.synchronize()
        return rc

    need = lib.verify_workspace_bytes(nq, 4)
    assert 0 < need <= ws.numel()
    assert call(129, 4, 4, need) == lib.MCE_ERR_DIM_RANGE
    assert call(5, 33, 33, ws.numel()) == lib.MCE_ERR_K_RANGE
    assert call(5, 4, 3, need) == lib.MCE_ERR_INVALID
    assert call(5, 4, 4, need - 1) == lib.MCE_ERR_WORKSPACE
    assert res.cpu().tolist() == [-7, -7] and int(ws.max()) == 0         # nothing was written
    assert call(5, 4, 4, need) == lib.MCE_OK and res.cpu().tolist()[0] == nq
