"""The panel sweep with FOUR query tiles per wave (knn_panel.hpp, QT = 4: a workgroup serves two of the plan's blocks, the
owner lanes' lists live in memory between drains) against the two-tile form, the exhaustive sweep and the CPU oracle: same
distances, same neighbour rows, same order -- bit for bit.  Needs a real MI355X: run with -m gpu."""
import functools
import logging

import numpy as np
import pytest

from helpers import orc

pytestmark = pytest.mark.gpu
logging.disable(logging.CRITICAL)


@pytest.fixture()
def wide(monkeypatch):
    from mcevidence_amd import _capi
    assert _capi.device_count() >= 1, "no GPU visible: the HIP path cannot be tested"
    _capi.set_search_mode(_capi.MODE_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_OFF)          # the pruned walk has priority where it applies
    yield _capi
    _capi.set_sym_mode(_capi.SYM_AUTO)
    _capi.set_prune_mode(_capi.PRUNE_AUTO)


@functools.lru_cache(maxsize=None)
def _data(n, d):
    rng = np.random.default_rng(1000 * d + n)
    Y = rng.standard_normal((n, d)) @ (np.eye(d) + 0.3 * rng.standard_normal((d, d))) + 3.0
    Y.setflags(write=False)
    return Y


_EXH = {}


def _exhaustive(capi, Y, key, K, sm):
    """the exhaustive sweep's lists (SYM_OFF), computed once per case and shared"""
    k = (key, K, sm)
    if k not in _EXH:
        capi.set_sym_mode(capi.SYM_OFF)
        d0, i0 = capi.knn(Y, Y, K, self_mode=sm)
        assert "symmetric" not in capi.last_kernel(), capi.last_kernel()
        d0.setflags(write=False)
        i0.setflags(write=False)
        _EXH[k] = (d0, i0)
    return _EXH[k]


def _sym(capi, monkeypatch, Y, K, sm, qt):
    monkeypatch.setenv("MCE_PANEL_QT", str(qt))
    capi.set_sym_mode(capi.SYM_FORCE)
    d1, i1 = capi.knn(Y, Y, K, self_mode=sm)
    kern = capi.last_kernel()
    assert "symmetric panel-kernel" in kern and " qt=%d " % qt in kern, kern
    return d1, i1


def _oracle(Y, K, d4, i4, m=600):
    """The last m rows against the brute-force oracle: the same ROWS, bit for bit.  The oracle adds the D squared differences one after
    the other, the library's exact refine (every sweep of it: the lists compared above are identical) in eight interleaved fma chains
    and a tree -- two correctly rounded evaluations of one sum of D non-negative terms, each within (D + 1) 2^-53 of it, relative;
    so the two DISTANCES differ by at most 2 (D + 1) 2^-53, plus one rounding each where a square root follows."""
    n, D = Y.shape
    m = min(n, m)
    od, oi = orc.knn_brute(Y[-m:], Y, K, self_mode=2, self_offset=n - m)
    rel = float(np.max(np.abs(d4[-m:] - od) / np.maximum(od, np.finfo(float).tiny)))
    bound = (2 * (D + 1) + 2) * 2.0 ** -53
    print("oracle: rows equal %s, max relative distance difference %.3e (bound %.3e)" % (np.array_equal(i4[-m:], oi), rel, bound))
    assert np.array_equal(i4[-m:], oi)
    assert rel <= bound, (rel, bound)


SHAPES = [(513, 27, 9, None),        # one wide block, its second half mostly padding
          (1025, 27, 9, None),       # three plan blocks: the last workgroup has no second one
          (2048, 27, 1, None),
          (3000, 16, 12, None),
          (7777, 27, 9, None),
          (20000, 27, 9, 4),         # MCE_SYM_PANEL=4: seven units per block -- the lists go through memory at every drain and hand-over
          (20000, 27, 16, None)]     # lists of 16


@pytest.mark.parametrize("n,d,K,panel", SHAPES)
def test_four_tiles_per_wave_are_bit_identical(wide, monkeypatch, n, d, K, panel):
    """all three self modes: QT = 4 against QT = 2, against the exhaustive sweep, and the last rows against the oracle"""
    capi = wide
    Y = _data(n, d)
    if panel:
        monkeypatch.setenv("MCE_SYM_PANEL", str(panel))
    for sm in (capi.SELF_EXCLUDE, capi.SELF_INCLUDE, capi.SELF_NONE):
        d0, i0 = _exhaustive(capi, Y, (n, d), K, sm)
        d2, i2 = _sym(capi, monkeypatch, Y, K, sm, 2)
        d4, i4 = _sym(capi, monkeypatch, Y, K, sm, 4)
        assert np.array_equal(d4, d2) and np.array_equal(i4, i2), (sm, np.argwhere(d4 != d2)[:5], np.argwhere(i4 != i2)[:5])
        assert np.array_equal(d4, d0) and np.array_equal(i4, i0), (sm, np.argwhere(d4 != d0)[:5], np.argwhere(i4 != i0)[:5])
        if sm == capi.SELF_EXCLUDE:
            _oracle(Y, K, d4, i4)


def test_ties_break_by_caller_row(wide, monkeypatch):
    """a 4-D lattice of 10 000 points (massive ties at the K-th distance) and a set with duplicated rows"""
    capi = wide
    sm = capi.SELF_EXCLUDE
    grid = np.stack(np.meshgrid(*[np.arange(10.0)] * 4), -1).reshape(-1, 4)
    rng = np.random.default_rng(9)
    base = rng.standard_normal((3000, 4))
    dup = np.concatenate([base, base, base[:1500], rng.standard_normal((2000, 4)) * 1e-3 + 50.0, base[::-1]])
    dup = np.ascontiguousarray(dup[rng.permutation(len(dup))])
    for name, Y, K in (("lattice", grid, 9), ("duplicates", dup, 4)):
        d0, i0 = _exhaustive(capi, Y, name, K, sm)
        d2, i2 = _sym(capi, monkeypatch, Y, K, sm, 2)
        d4, i4 = _sym(capi, monkeypatch, Y, K, sm, 4)
        assert np.array_equal(d4, d2) and np.array_equal(i4, i2), name
        assert np.array_equal(d4, d0) and np.array_equal(i4, i0), name
        _oracle(Y, K, d4, i4)


@pytest.mark.parametrize("env", [dict(MCE_PANEL_DEBUG="8"),                                        # every candidate through the redo list
                                 dict(MCE_PANEL_DEBUG="16"),                                       # the odd waves of every block's second unit give up
                                 dict(MCE_SYM_SPIN_LIMIT="0", MCE_SYM_PANEL="4"),                  # every unit after a block's first gives up
                                 dict(MCE_SYM_BUCKET="2")],                                        # buckets overflow: the repair launch
                         ids=["redo", "some-waves-give-up", "all-give-up", "repair"])
def test_redo_give_up_and_repair(wide, monkeypatch, env):
    capi = wide
    n, d, K = 20000, 27, 9
    sm = capi.SELF_EXCLUDE
    Y = _data(n, d)
    d0, i0 = _exhaustive(capi, Y, (n, d), K, sm)
    d2, i2 = _sym(capi, monkeypatch, Y, K, sm, 2)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    d4, i4 = _sym(capi, monkeypatch, Y, K, sm, 4)
    assert np.array_equal(d4, d2) and np.array_equal(i4, i2), (np.argwhere(d4 != d2)[:5], np.argwhere(i4 != i2)[:5])
    assert np.array_equal(d4, d0) and np.array_equal(i4, i0)
    _oracle(Y, K, d4, i4)


def test_fused_reduction(wide, monkeypatch):
    """knn_dotp: the distances that enter the sums are the exhaustive sweep's, bit for bit; the sums agree to rounding and are
    reproducible run to run"""
    capi = wide
    n, d, kmax = 20000, 27, 10
    X = _data(n, d)
    w = np.random.default_rng(1).integers(1, 5, n).astype(float)
    fs = -np.random.default_rng(2).random(n)
    capi.set_sym_mode(capi.SYM_OFF)
    p0, q0 = capi.knn_dotp(X, None, w, fs, kmax, 1, return_dist=True)
    assert "symmetric" not in capi.last_kernel()
    capi.set_sym_mode(capi.SYM_FORCE)
    res = {}
    for qt in (2, 4):
        monkeypatch.setenv("MCE_PANEL_QT", str(qt))
        res[qt] = capi.knn_dotp(X, None, w, fs, kmax, 1, return_dist=True)
        assert " qt=%d " % qt in capi.last_kernel(), capi.last_kernel()
    assert np.array_equal(res[4][1], res[2][1]) and np.array_equal(res[4][1], q0)
    assert np.array_equal(res[4][0], res[2][0])             # same lists, same column order: the same sums
    assert np.allclose(res[4][0], p0, rtol=1e-13, atol=0)
    assert np.array_equal(res[4][0], capi.knn_dotp(X, None, w, fs, kmax, 1))


def test_under_graph_capture(wide, monkeypatch):
    """the call only enqueues: captured into a HIP graph and replayed on new data in the same buffers"""
    import torch
    capi = wide
    monkeypatch.setenv("MCE_PANEL_QT", "4")
    capi.set_sym_mode(capi.SYM_FORCE)
    rng = np.random.default_rng(21)
    n, d, kmax = 20000, 27, 10
    K = kmax - 1
    X = torch.empty((n, d), dtype=torch.float64, device="cuda")
    w = torch.ones(n, dtype=torch.float64, device="cuda")
    fs = torch.zeros(n, dtype=torch.float64, device="cuda")
    wsb = capi.knn_workspace_bytes(n, n, d, K) + capi.dotp_workspace_bytes(n, kmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(kmax, dtype=torch.float64, device="cuda")
    dd = torch.zeros((n, K), dtype=torch.float64, device="cuda")

    def call(stream):
        capi.knn_dotp_dev(X.data_ptr(), n, X.data_ptr(), n, d, kmax, 1, 0, w.data_ptr(), fs.data_ptr(), out.data_ptr(),
                          dd.data_ptr(), ws.data_ptr(), wsb, stream)
    data = [rng.standard_normal((n, d)) for _ in range(3)]
    X.copy_(torch.from_numpy(data[0]))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                       # warm-up outside capture (one-time kernel attributes)
        call(side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(torch.cuda.current_stream().cuda_stream)
    assert " qt=4 " in capi.last_kernel(), capi.last_kernel()
    capi.set_sym_mode(capi.SYM_OFF)
    for h in data[1:]:
        X.copy_(torch.from_numpy(h))
        graph.replay()
        torch.cuda.synchronize()
        want_dotp, want_dist = capi.knn_dotp(h, None, np.ones(n), np.zeros(n), kmax, 1, return_dist=True)
        assert "symmetric" not in capi.last_kernel()
        assert np.array_equal(dd.cpu().numpy(), want_dist)
        assert np.allclose(out.cpu().numpy(), want_dotp, rtol=1e-13, atol=0)
