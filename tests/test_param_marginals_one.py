"""marginals without and with bounds are ONE text on every layer (csrc/param_marginals_kernels.hpp, csrc/capi_marginals.hpp,
``marginals._measure``): what must not have moved when the two families were merged.  The sizes the library plans are those of the last
commit that had two texts; the rule without bounds and the rule with open bounds decide and measure the same bytes."""
import numpy as np
import pytest

from mcevidence_amd import _capi, marginals

# (nrows_total, nseg, dmax, np, grid) -> workspace bytes, bounded workspace bytes, block doubles, bounded block doubles: read from the
# library built at fed3099 ("Add bounds=: 1-D marginals that honour hard prior bounds"), which had a workspace struct per family
PLANNED = {(0, 1, 1, 1, 64): (4096, 4864, 86, 90),
           (513, 1, 3, 2, 512): (40192, 65536, 1598, 1610),
           (40000, 3, 27, 2, 1024): (18695936, 36618496, 28142, 28250)}


@pytest.mark.parametrize("shape", sorted(PLANNED))
def test_planned_sizes_are_the_two_families(shape):
    ws, ws_bounded, block, block_bounded = PLANNED[shape]
    assert _capi.param_marginals_workspace_bytes(*shape) == ws
    assert _capi.param_marginals_bounded_workspace_bytes(*shape) == ws_bounded
    assert _capi.param_marginals_out_doubles(*shape[2:]) == block == _capi.marginals_block_doubles(*shape[2:])
    assert _capi.param_marginals_bounded_out_doubles(*shape[2:]) == block_bounded == _capi.marginals_bounded_block_doubles(*shape[2:])


def _same_bytes(u, v):
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return u.shape == v.shape and u.tobytes() == v.tobytes()


def _densities():
    G = 64
    k = np.arange(G, dtype=np.float64)
    ties = np.round(8.0 * np.exp(-((k - 20.0) / 9.0) ** 2) + 5.0 * np.exp(-((k - 47.0) / 5.0) ** 2)) / 8.0     # few values, each many times
    plateau = np.exp(-((k - 30.0) / 11.0) ** 2)
    plateau[:9] = plateau[9]                                     # flat from k = 0 on: the lower end is selected with its neighbours
    return {"ties": ties, "plateau_at_an_end": plateau}


@pytest.mark.parametrize("name", sorted(_densities()))
def test_decide_is_decide_bounded_without_ends(name):
    rho = _densities()[name]
    assert np.unique(rho).size < rho.size
    probs = (0.3, 0.68, 0.95, 0.999)
    plain = marginals.decide(rho, -1.25, 0.0625, probs)
    open_ends = marginals.decide_bounded(rho, -1.25, 0.0625, probs, False, False)
    assert len(plain) == len(open_ends) == 6 and all(_same_bytes(u, v) for u, v in zip(plain, open_ends))
    order, masks = marginals.hpd_selection(rho, probs)
    order_b, masks_b = marginals.hpd_selection_bounded(rho, probs, False, False)
    assert np.array_equal(order, order_b) and all(np.array_equal(u, v) for u, v in zip(masks, masks_b))


def test_measure_is_measure_bounded_with_open_bounds():
    rng = np.random.default_rng(11)
    x = np.round(rng.standard_normal((40, 2)) * 64) / 64
    x[:, 1] = np.abs(x[:, 1])
    a = rng.integers(0, 5, 40).astype(np.float64)                # (some rows without a weight)
    inf = np.full(2, np.inf)
    plain = marginals.measure(a, x, (0.68, 0.95), grid=64)
    bounded = marginals.measure_bounded(a, x, (-inf, inf), (0.68, 0.95), grid=64)
    assert plain["status"] == 0 and np.all(plain["col_status"] == 0) and set(bounded) - set(plain) == set(marginals.BOUND_KEYS)
    for k in plain:
        assert _same_bytes(plain[k], bounded[k]), k
    assert np.all(bounded["at_lo"] == 0.0) and np.all(bounded["at_hi"] == 0.0)
