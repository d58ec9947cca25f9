"""The two byte offsets into the search workspace that are public: ``mce_prune_part_prepare_dev`` returns where the k-d permutation
lies and ``mce_pairs_once_prepare_dev`` where the rows' bounds lie, and parallel.py all-reduces the memory at those addresses over the
ranks.  They are now read off the typed arena (csrc/search_layout.hpp: ``A.prune.perm_r``, ``A.sym.thr``) and must be what the planner
counted by hand at 3aad787 ("One table of posterior statistics for host, resident and farm routes"), the last commit that did.
Neither array lies behind a block sized by rocPRIM."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d))


@pytest.fixture
def capi():
    from mcevidence_amd import _capi
    yield _capi
    _capi.set_sym_mode(_capi.SYM_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


def test_perm_offset_is_where_the_hand_counted_planner_put_it(capi):
    """the pruned walk's distributed k-d preparation: 70 000 x 6, K = 4, rank 1 of two"""
    import torch
    capi.set_prune_mode(capi.PRUNE_FORCE)
    n, d, kmax = 70000, 6, 5
    Y = torch.from_numpy(_rows(n, d, 1)).cuda()
    wsb = capi.knn_workspace_bytes(n, n, d, kmax - 1) + capi.dotp_workspace_bytes(n, kmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    off, cnt, lo, hi = capi.prune_part_prepare_dev(Y.data_ptr(), n, d, kmax, 1, 2, ws.data_ptr(), wsb, 0, want_range=True)
    torch.cuda.synchronize()
    assert (off, cnt) == (9422592, 71680) and 0 < lo < hi == cnt
    own = ws[off:off + 4 * cnt].view(torch.int32)[lo:hi]
    rows = own[own >= 0].tolist()
    assert bool((ws[off:off + 4 * lo] == 0).all()) and len(rows) == len(set(rows)) > 0 and max(rows) < n


def test_bounds_offset_is_where_the_hand_counted_planner_put_it(capi):
    """the all-pairs-once partition: 70 000 x 27, kmax = 10, rank 0 of two"""
    import torch
    capi.set_sym_mode(capi.SYM_FORCE)
    capi.set_prune_mode(capi.PRUNE_OFF)
    n, d, kmax = 70000, 27, 10
    Y = torch.from_numpy(_rows(n, d, 2)).cuda()
    wsb = capi.pairs_once_workspace_bytes(n, d, kmax, 2)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    off, cnt = capi.pairs_once_prepare_dev(Y.data_ptr(), n, d, kmax, 0, 2, ws.data_ptr(), wsb, 0)
    torch.cuda.synchronize()
    assert (off, cnt) == (36871680, 70144)
    bounds = ws[off:off + 8 * cnt].view(torch.float64)
    assert bool(torch.isfinite(bounds[:512]).all()) and bool(torch.isinf(bounds[512:1024]).all())        # rank 0 owns block 0, not block 1
