"""A pruned search in a workspace that was sized before MCE_PRUNE_HEAVY was set (``plan_for_workspace``'s third fallback, capi_plan.hpp): the
plan it falls back to has no heavy waves at all -- their count lives in the plan's ``SearchSizes`` and is recomputed by every ``plan_sizes`` --
so the walk runs unsplit, inside the workspace, with the same bits.  (When the planner still counted offsets by hand, ``Plan::heavy_max`` and
``off_heavy`` kept the first plan's values and the side lists were written behind the workspace.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d))


@pytest.fixture
def capi():
    from mcevidence_amd import _capi
    yield _capi
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


def test_a_workspace_sized_before_the_heavy_waves_were_asked_for_runs_unsplit_inside_it(capi, monkeypatch):
    """plan_for_workspace's third fallback: the plan it falls back to has no heavy waves at all (the count lives in the plan's sizes), so
    nothing is written behind the workspace -- a guard band behind it stays untouched -- and the sums are those of the unsplit walk, bit
    for bit; a workspace sized with the variable set does split."""
    import torch
    monkeypatch.delenv("MCE_PRUNE_HEAVY", raising=False)
    capi.set_prune_mode(capi.PRUNE_FORCE)
    n, d, kmax = 40000, 6, 5          # 79 query blocks: from 64 blocks a same-set pruned plan may reserve side lists
    Y = torch.from_numpy(_rows(n, d, 3)).cuda()
    w = torch.ones(n, dtype=torch.float64, device="cuda")
    fs = torch.zeros(n, dtype=torch.float64, device="cuda")
    small = capi.knn_workspace_bytes(n, n, d, kmax - 1) + capi.dotp_workspace_bytes(n, kmax)
    guard = 1 << 20

    def run(wsb):
        buf = torch.full((wsb + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        out = torch.zeros(kmax, dtype=torch.float64, device="cuda")
        capi.knn_dotp_dev(Y.data_ptr(), n, Y.data_ptr(), n, d, kmax, 1, 0, w.data_ptr(), fs.data_ptr(), out.data_ptr(), 0, buf.data_ptr(), wsb, 0)
        torch.cuda.synchronize()
        assert "pruned" in capi.last_kernel() and bool((buf[wsb:] == 0x5A).all())
        return out.cpu().numpy(), capi.last_kernel()

    plain, k0 = run(small)
    monkeypatch.setenv("MCE_PRUNE_HEAVY", "100,4")
    large = capi.knn_workspace_bytes(n, n, d, kmax - 1) + capi.dotp_workspace_bytes(n, kmax)
    assert large > small
    fallback, k1 = run(small)
    split, k2 = run(large)
    assert "heavy=0x1" in k0 and "heavy=0x1" in k1 and "heavy=39x4" in k2          # (room for max(79 * 8 / 16, 32) = 39 waves)
    assert np.array_equal(plain, fallback) and np.all(np.isfinite(plain))
    assert np.allclose(split, plain, rtol=1e-12, atol=0)          # (the split walk folds the same exact lists: the sums agree to rounding of their order)
