"""The jackknife on the GPU (docs/design/jackknife.md): mce_knn_f64_dev + mce_jack_dotp_dev through jackknife.HipSession and the ladder,
against brute-force DELETION (tests/jack_cases.py: delete the group, search again).  Bounds: n eps relative on the sums (sums of n
same-signed terms), LNE_TOL on ln E per group.  Shapes are small on purpose; every case takes a second or two."""
import numpy as np
import pytest

import jack_cases as jc
from helpers import LNE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from mcevidence_amd import _capi
    _capi.require_device()
    return _capi


def _session(c):
    from mcevidence_amd.jackknife import HipSession
    return HipSession(c["X"], c["Y"], c["d"], c["kmax"], c["w"], c["fs"], c["gq"], c["gr"], c["G"], whitened=True)


_MODEL = {}


def _model(name, make):
    """the case and its deletion sums, computed once"""
    if name not in _MODEL:
        c = make()
        _MODEL[name] = (c, jc.deletion_model(c["X"], c["Y"], c["gq"], c["gr"], c["G"], c["k0"], c["kmax"], c["w"], c["fs"]))
    return _MODEL[name]


def _model_short(c, L):
    """the rows the model's own lists of L entries leave short"""
    n = len(c["X"])
    if c["Y"] is None:
        _, idx = jc.exact_lists(c["X"], c["X"], min(L, n - 1), own=np.arange(n))
    else:
        _, idx = jc.exact_lists(c["X"], c["Y"], min(L, len(c["Y"])))
    return jc.short_rows(idx, c["gq"], c["gr"], c["G"], c["kmax"] - c["k0"])


def _ladder_against_model(name, make):
    from mcevidence_amd.jackknife import run_ladder
    c, (want_g, want_f) = _model(name, make)
    n = len(c["X"])
    g, f, per_level = run_ladder(_session(c), n, c["G"], c["k0"], c["kmax"])
    jc.assert_sums(g, f, want_g, want_f, n, c["k0"], what=name)
    lf, lg = jc.lnE_groups(g, f, c["gq"], c["G"], c["k0"], c["kmax"], c["w"])
    wf, wg = jc.lnE_groups(want_g, want_f, c["gq"], c["G"], c["k0"], c["kmax"], c["w"])
    err = max(np.max(np.abs(lf - wf)), np.max(np.abs(lg - wg)))
    print("%s: max |d ln E| over the groups %.3e, rows per level %s" % (name, err, per_level))
    assert err <= LNE_TOL
    return c, per_level


def _full_sum_is_dotp(capi, c):
    """no short row: the full-sample sum of the jackknife kernel == mce_dotp_f64_dev on the same distances, bit for bit; two runs equal"""
    import torch
    s = _session(c)
    n, k0, kmax = len(c["X"]), c["k0"], c["kmax"]
    dist, idx, sel = s.lists(16, None)
    g1, f1, short1 = s.sums(dist, idx, sel)
    g2, f2, short2 = s.sums(dist, idx, sel)
    assert len(short1) == 0 and len(short2) == 0
    assert np.array_equal(g1, g2) and np.array_equal(f1, f2)
    out = torch.zeros(kmax, dtype=torch.float64, device=dist.device)
    wsb = capi.dotp_workspace_bytes(n, kmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dist.device)
    # column k of the reduction is list entry k - k0: the base pointer is shifted as the library's own unfused path shifts it
    capi.dotp_dev(dist.data_ptr() - 8 * k0, n, dist.shape[1], k0, kmax, c["d"], s.w.data_ptr(), s.fs.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    assert np.array_equal(f1, out.cpu().numpy()), (f1, out.cpu().numpy())
    return g1, f1


def test_A_iid_no_short_rows(capi):
    c, (want_g, want_f) = _model("A", jc.case_iid)
    assert len(_model_short(c, 16)) == 0
    g, f = _full_sum_is_dotp(capi, c)
    jc.assert_sums(g, f, want_g, want_f, len(c["X"]), 1, what="A")
    _, per_level = _ladder_against_model("A", jc.case_iid)
    assert per_level == {16: 600}


def test_B_walk_takes_the_second_rung():
    c, _ = _model("B", jc.case_walk)
    s16, s32 = _model_short(c, 16), _model_short(c, 32)
    assert len(s16) > 0 and len(s32) == 0
    _, per_level = _ladder_against_model("B", jc.case_walk)
    assert per_level == {16: 600, 32: len(s16)}


def test_C_planted_overflow_short_rows_ascending():
    c, _ = _model("C", jc.case_planted)
    s = _session(c)
    for L in (16, 32):
        rows = None if L == 16 else np.array([10, 330, 500])
        _, _, short = s.level(L, rows)
        assert short.tolist() == [10, 330, 500] == _model_short(c, L).tolist()
    assert len(_model_short(c, 64)) == 0
    _, per_level = _ladder_against_model("C", jc.case_planted)
    assert per_level == {16: 640, 32: 3, 128: 3}


@pytest.mark.parametrize("n,G", [(257, 2), (300, 64)])
def test_D_sizes_off_the_block(n, G):
    _ladder_against_model("D%d" % n, lambda: jc.case_iid(n=n, G=G, seed=20 + G))


def test_E_group_without_query_rows():
    c, _ = _ladder_against_model("E", lambda: jc.case_cross(empty_group=3))
    assert not (c["gq"] == 3).any() and (c["gr"] == 3).any()


def test_F_fp16_filter_family_at_16(capi):
    mode = capi.get_search_mode()
    capi.set_search_mode(2)
    try:
        make = lambda: jc.case_iid(n=2048, d=27, G=16, kmax=10, seed=27)          # noqa: E731
        c, _ = _model("F", make)
        s = _session(c)
        dist, _, _ = s.lists(16, None)
        assert dist.shape == (2048, 16) and "f16" in capi.last_kernel(), capi.last_kernel()
        _ladder_against_model("F", make)
    finally:
        capi.set_search_mode(mode)


def test_G_cross_shuffled(capi):
    c, per_level = _ladder_against_model("G", jc.case_cross)
    assert c["k0"] == 0 and not np.array_equal(c["rows"][0], np.sort(c["rows"][0])) and per_level[16] == 500


def test_H_negative_weight(capi):
    def make():
        c = jc.case_iid(seed=31)
        c["w"] = c["w"].copy()
        c["w"][123] = -2.0
        return c
    c, (want_g, want_f) = _model("H", make)
    g, f = _full_sum_is_dotp(capi, c)
    jc.assert_sums(g, f, want_g, want_f, len(c["X"]), 1, what="H")


def test_I_capacity_is_an_ordinary_error():
    from mcevidence_amd.jackknife import run_ladder
    c = jc.case_capacity()
    with pytest.raises(ValueError, match=r"1 row still short after lists of 1024"):
        run_ladder(_session(c), 3000, 2, 1, 5)


def test_J_evidence_jackknife_on_a_file_root(capi, tmp_path):
    import mcevidence_amd as pkg
    from helpers import OracleFeedBackend
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    from test_jackknife_shared import _model_lnE
    chains, _, ranges = planck_like_chains(seed=1, rows=(700, 650, 720, 680))
    root = str(tmp_path / "planck")
    write_cosmomc_chains(root, chains, ranges=ranges, fmt="%.17g")
    m = pkg.MCEvidence(root, kmax=3, ndim=6, verbose=0)
    problem, ctx = m._feed_problem("all", False)
    dotp, jac, _ = capi.evidence_feed(*problem)
    before = m._feed_finish(ctx, dotp, jac, 0.0)[1:]
    assert m.jackknife is None
    plain = m.evidence()
    assert np.array_equal(plain, before) and "jackknife" not in m.info
    out = m.evidence_jackknife()
    assert out["groups"] == 16 and out["by"] == "blocks" and np.max(np.abs(out["lnE"] - plain)) <= LNE_TOL
    host = pkg.MCEvidence(root, kmax=3, ndim=6, verbose=0, backend=OracleFeedBackend()).evidence_jackknife()
    assert np.max(np.abs(out["lnE_groups"] - host["lnE_groups"])) <= LNE_TOL and np.max(np.abs(out["sigma"] - host["sigma"])) <= LNE_TOL
    assert out["rows_per_level"] == host["rows_per_level"]
    by = m.evidence_jackknife(by="chains")
    assert by["groups"] == 4 and np.max(np.abs(by["lnE_groups"] - _model_lnE(m, 4, "chains"))) <= LNE_TOL
    with_bars = pkg.MCEvidence(root, kmax=3, ndim=6, verbose=0, jackknife=16)
    assert np.array_equal(with_bars.evidence(), plain) and np.array_equal(with_bars.info["jackknife"]["lnE_groups"], out["lnE_groups"])
