"""summary, cov, marginals and contours plan the head of their workspaces in ONE text (csrc/capi_sum_front.hpp: ``SumFrontWs``): what
must not have moved when the four copies were merged.  The sizes are those that the library built at 6d7f905 ("Marginals: one set of
kernels and drivers for bounds on and off") planned, the last commit with a workspace head per family.  (The marginals' sizes are
pinned in test_param_marginals_one.py; summary's hold rocPRIM's answer for its sort and are compared old against new instead:
docs/design/seg_tiles.md.)"""
import pytest

from mcevidence_amd import _capi

# (nrows_total, nseg, dmax) -> workspace bytes, block doubles
COV_PLANNED = {(0, 1, 1): (4096, 10),
               (513, 1, 3): (6144, 17),
               (40000, 3, 27): (588544, 413)}

# (nrows_total, nseg, dmax, nc, np, grid) -> workspace bytes, block doubles
CONTOURS_PLANNED = {(0, 1, 1, 2, 1, 32): (27904, 1061),
                    (513, 1, 3, 2, 2, 64): (109824, 4140),
                    (40000, 3, 27, 27, 2, 64): (586850304, 1444265)}


@pytest.mark.parametrize("shape", sorted(COV_PLANNED))
def test_cov_plans_the_sizes_of_its_own_workspace_head(shape):
    ws, block = COV_PLANNED[shape]
    assert _capi.param_cov_workspace_bytes(*shape) == ws
    assert _capi.param_cov_out_doubles(shape[2]) == block == _capi.cov_block_doubles(shape[2])


@pytest.mark.parametrize("shape", sorted(CONTOURS_PLANNED))
def test_contours_plans_the_sizes_of_its_own_workspace_head(shape):
    ws, block = CONTOURS_PLANNED[shape]
    assert _capi.param_contours_workspace_bytes(*shape) == ws
    assert _capi.param_contours_out_doubles(*shape[3:]) == block == _capi.contours_block_doubles(*shape[3:])
