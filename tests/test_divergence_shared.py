"""The k-NN relative entropy's shared rule on the CPU (docs/design/knn_divergence.md): csrc/knn_div.hpp through its stand-alone program
(AddressSanitizer + UBSan) and divergence.measure against brute-force DELETION (tests/div_cases.py: delete the group from both chains,
search again) and the mpmath oracle, the group ids, every status and argument error, the ladder on a planted cluster, ``estimate`` and
the tension route without a device, both command-line forms, and the statistical and calibration checks on Gaussians with a known
answer.  CPU only."""
import logging
import os
import subprocess

import numpy as np
import pytest

import div_cases as dc
from helpers import REPO, OracleBackend
from mcevidence_amd import _capi, divergence as dv, tension as tn

# nP, nQ, d, K, G: odd sizes, one block and more, one column, no groups and 64 of them, the widest rank count
CASES = {
    "257x300_d3_K4_G8": (257, 300, 3, 4, 8),
    "513x700_d27_K4_G2": (513, 700, 27, 4, 2),
    "33x32_d1_K1_G2": (33, 32, 1, 1, 2),
    "255x300_d3_K2_G64": (255, 300, 3, 2, 64),
    "256x300_d3_K16_G0": (256, 300, 3, 16, 0),
    "300x257_d3_K8_G8_frac": (300, 257, 3, 8, 8),
}
GAP = 1e-9


@pytest.fixture(scope="module")
def div_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("div") / "div_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"), os.path.join(REPO, "tests", "native", "div_check.cpp"), "-o", exe])
    return exe


def test_native_unit_checks(div_check):
    assert subprocess.check_output([div_check]).decode().startswith("ok ")


def _groups(c, G):
    return (dc.blocks(len(c["zp"]), G), dc.blocks(len(c["zq"]), G)) if G > 0 else (None, None)


def _native(div_check, tmp_path):
    def run(dP, iP, dQ, iQ, gq, gP, gQ, G, K, d, aq, aP, bQ, qid=None):
        dc.write_case(str(tmp_path / "case.bin"), dP, iP, dQ, iQ, gq, gP, gQ, G, K, d, aq, aP, bQ, qid=qid)
        subprocess.check_call([div_check, str(tmp_path / "case.bin"), str(tmp_path / "out.txt")])
        return dc.read_result(str(tmp_path / "out.txt"), G, K)
    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_measure_and_native_driver_against_deletion_and_the_oracle(name, div_check, tmp_path):
    nP, nQ, d, K, G = CASES[name]
    c = dc.make_case(nP, nQ, d, seed=1, weights="frac" if name.endswith("frac") else "int")
    gP, gQ = _groups(c, G)
    model = dc.deletion_model(c, G, K)
    wp, wq = dv.masses(c["a"], gP, G), dv.masses(c["b"], gQ, G)
    levels, oracle = {}, {}
    for what, fn in (("measure", dv.measure), ("div_serial", _native(div_check, tmp_path))):
        sums, levels[what] = dv.run_ladder(dc.ladder_session(fn, c, gP, gQ, G, K), nP, G, K)
        L = max(levels[what])                            # (a row that is not short at a rung has the same K kept entries at every longer one)
        if L not in oracle:
            dP, iP, dQ, iQ = dc.lists(c["zp"], c["zq"], L)
            gap = dc.min_relative_gap(dP, dQ)
            print("%s: smallest relative gap %.3g, rows per level %s" % (name, gap, levels[what]))
            assert gap >= GAP
            oracle[L] = dc.oracle_sums(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, c["a"], c["a"], c["b"])
        N, X, B = oracle[L]
        assert sums.shape == (G + 1, K, 2)
        dc.assert_sums(sums, N, X, B, what="%s %s" % (name, what))
        dc.assert_values(dv.values(sums, wp, wq), sums, model, B, what="%s %s" % (name, what))
    assert levels["measure"] == levels["div_serial"]
    if name == "257x300_d3_K4_G8":
        assert levels["measure"] == {16: 257}
    if name == "513x700_d27_K4_G2":
        assert set(levels["measure"]) >= {16, 32} and levels["measure"][32] > 0          # half the rows are a group: lists of 16 run out


def test_tie_case_counts_coincident_rows(div_check, tmp_path):
    c = dc.tie_case()
    G, K, d = 4, 3, 3
    gP, gQ = _groups(c, G)
    dP, iP, dQ, iQ = dc.lists(c["zp"], c["zq"], 16)
    N, X, B = dc.oracle_sums(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, c["a"], c["a"], c["b"])
    # rank 1: P rows 40, 41, 42 (weight 2 each) coincide with one another, 100 and 200 with rows of Q
    assert X[0, 0] == 6.0 + c["a"][100] + c["a"][200] and X[0, 1] == 6.0 + c["a"][200] and X[0, 2] == 0.0
    model = dc.deletion_model(c, G, K)
    for what, fn in (("measure", dv.measure), ("div_serial", _native(div_check, tmp_path))):
        sums, short = fn(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, c["a"], c["a"], c["b"])
        assert len(short) == 0
        dc.assert_sums(sums, N, X, B, what="tie " + what)
        dc.assert_values(dv.values(sums, dv.masses(c["a"], gP, G), dv.masses(c["b"], gQ, G)), sums, model, B, what="tie " + what)
    out = dv.summarise(sums, dv.masses(c["a"], gP, G), dv.masses(c["b"], gQ, G))
    assert np.array_equal(out["excluded"], X[0] / c["a"].sum()) and out["D_groups"].shape == (G, K)


def test_group_ids_masses_and_summarise():
    for n in (2, 7, 257, 300, 1000003):
        for G in (2, 8, 64):
            g = dv.group_ids(n, G)
            assert g.dtype == np.int32 and np.array_equal(g, np.arange(n, dtype=np.int64) * G // n) and g.min() == 0 and g.max() <= G - 1
            cnt = np.bincount(g, minlength=G)
            assert cnt.max() - cnt.min() <= 1
    m = dv.masses(np.array([1.0, 2.0, 4.0, 8.0, 16.0]), np.array([0, 1, 0, 2, 1]), 3)
    assert m.tolist() == [31.0, 5.0, 18.0, 8.0] and dv.masses(np.array([1.0, 2.0]), None, 0).tolist() == [3.0]
    assert dv.ladder(4) == (16, 32, 128) == dv.ladder(8) and dv.ladder(9) == (32, 128) == dv.ladder(16)
    # D = N / (WP_b - X) + log WQ_b; sigma and the bias-corrected value are jackknife.summarise's
    sums = np.zeros((3, 1, 2))
    sums[:, 0, 0] = [6.0, 2.0, 8.0]
    sums[:, 0, 1] = [1.0, 0.0, 1.0]
    out = dv.summarise(sums, np.array([4.0, 1.0, 2.0]), np.array([np.e, 0.0, 0.0]))
    assert np.allclose(out["D"], [3.0]) and np.allclose(out["D_groups"][:, 0], [2.0 / 3.0 + 1.0, 8.0 + 1.0]) and np.allclose(out["excluded"], [0.25])
    v = out["D_groups"][:, 0]
    assert np.allclose(out["sigma"], [np.sqrt(0.5 * ((v - v.mean()) ** 2).sum())]) and np.allclose(out["D_bias_corrected"], [2 * 3.0 - v.mean()])
    none = dv.summarise(sums[:1], np.array([4.0]), np.array([np.e]))
    assert np.allclose(none["D"], [3.0]) and np.isnan(none["sigma"]).all() and none["D_groups"].shape == (0, 1)


def test_the_ladder_on_the_planted_cluster(div_check, tmp_path):
    c = dc.planted_case()
    G, K, d = 8, 4, 3
    gP, gQ = _groups(c, G)
    native = _native(div_check, tmp_path)
    model = dc.deletion_model(c, G, K)
    wp, wq = dv.masses(c["a"], gP, G), dv.masses(c["b"], gQ, G)
    for what, fn in (("measure", dv.measure), ("div_serial", native)):
        seen = {}
        sums, per_level = dv.run_ladder(dc.ladder_session(fn, c, gP, gQ, G, K, seen), 640, G, K)
        assert seen == {16: [10, 330, 500], 32: [10, 330, 500], 128: []} and per_level == {16: 640, 32: 3, 128: 3}, (what, seen)
        # the level sums add up to the deletion model (the bound of the first rung's lists covers the three rows of the last)
        dP, iP, dQ, iQ = dc.lists(c["zp"], c["zq"], 128)
        N, X, B = dc.oracle_sums(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, c["a"], c["a"], c["b"])
        dc.assert_sums(sums, N, X, B, what="planted " + what)
        dc.assert_values(dv.values(sums, wp, wq), sums, model, B, what="planted " + what)

    class Never(object):
        def level(self, L, rows):
            return np.zeros((G + 1, K, 2)), np.array([3, 5])
    with pytest.raises(ValueError, match="2 rows still short after lists of 128"):
        dv.run_ladder(Never(), 640, G, K)


def test_statuses(caplog):
    c = dc.make_case(120, 130, 3, seed=3)
    xp, a, xq, b = c["zp"], c["a"], c["zq"], c["b"]
    good = dv.estimate(xp, a, xq, b, kmax=2, groups=4, native=False)
    assert good["status"] == 0 and np.isfinite(good["D"]).all() and good["chain"] is None and good["rows_per_level"] == {16: 120}

    def run(xp=xp, a=a, xq=xq, b=b, **kw):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            out = dv.estimate(xp, a, xq, b, native=False, **dict(dict(kmax=2, groups=4), **kw))
        assert len([r for r in caplog.records if "knn divergence: status" in r.getMessage()]) == (1 if out["status"] else 0)
        if out["status"]:
            assert all(np.isnan(out[k]).all() for k in ("D", "sigma", "D_bias_corrected", "D_groups", "excluded"))
        return out["status"], out["column"], out["chain"]

    def edit(v, i, x):
        v = v.copy()
        v[i] = x
        return v
    assert run(a=edit(a, 5, -1.0)) == (3, -1, "P") and run(a=edit(a, 5, np.nan)) == (3, -1, "P") and run(b=edit(b, 7, np.inf)) == (3, -1, "Q")
    assert run(xp=edit(edit(xp, (4, 2), np.nan), (9, 1), np.inf)) == (4, 1, "P") and run(xq=edit(xq, (0, 2), np.nan)) == (4, 2, "Q")
    # precedence: P's weights, P's values, the row counts, the factorisation, Q's weights, Q's values
    assert run(a=edit(a, 5, np.nan), xp=edit(xp, (4, 2), np.nan), b=edit(b, 7, -2.0)) == (3, -1, "P")
    assert run(xp=edit(xp, (4, 2), np.nan), b=edit(b, 7, -2.0)) == (4, 2, "P")
    assert run(b=edit(b, 7, -2.0), xq=edit(xq, (0, 2), np.nan)) == (3, -1, "Q")
    # a weight of 0 drops its row before anything else, whatever the row holds
    z = dv.estimate(edit(xp, (4, 2), np.nan), edit(a, 4, 0.0), xq, b, kmax=2, groups=4, native=False)
    assert z["status"] == 0 and z["rows_p"] == 119
    # 6: K + 1 rows of P and K of Q must be left for every deleted group
    assert run(xp=xp[:6], a=a[:6], kmax=3, groups=2)[0] == 6 and run(xp=xp[:8], a=a[:8], kmax=3, groups=2)[0] == 0
    assert run(xq=xq[:5], b=b[:5], kmax=3, groups=2)[0] == 6 and run(xq=xq[:6], b=b[:6], kmax=3, groups=2)[0] == 0
    assert run(xp=xp[:3], a=a[:3], kmax=3, groups=0)[0] == 6 and run(xp=xp[:4], a=a[:4], xq=xq[:3], b=b[:3], kmax=3, groups=0)[0] == 0
    # 7: a column that repeats another
    flat = xp.copy()
    flat[:, 2] = flat[:, 0]
    assert run(xp=flat)[0] == 7 and run(xp=flat, xq=edit(xq, (0, 2), np.nan))[0] == 7


def test_new_symbols_and_argument_errors():
    lib = _capi.load()
    for s in ("mce_div_whiten_workspace_bytes", "mce_div_whiten_dev", "mce_div_whiten_f64", "mce_knn_div_workspace_bytes", "mce_knn_div_terms_dev",
              "mce_knn_div_terms_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_DIV_MAX_K == dv.MAX_K == 16 and _capi.MCE_DIV_MAX_DIM == dv.MAX_DIM == 64
    assert _capi.knn_div_workspace_bytes(1000, 1200, 8, 4) >= 4 * 9 * 4 * 2 * 8 and _capi.div_whiten_workspace_bytes(1000, 64) >= (64 * 65 + 12) * 8
    for bad in ((0, 10, 8, 4), (10, 0, 8, 4), (10, 10, 1, 4), (10, 10, 65, 4), (10, 10, 8, 0), (10, 10, 8, 17)):
        with pytest.raises(ValueError):
            _capi.knn_div_workspace_bytes(*bad)
    for bad in ((0, 3), (10, 0), (10, 65)):
        with pytest.raises(ValueError):
            _capi.div_whiten_workspace_bytes(*bad)
    # argument errors come before any device call: here there may be no device at all
    c = dc.make_case(40, 50, 3, seed=2)
    gP, gQ = dc.blocks(40, 4), dc.blocks(50, 4)
    dP, iP, dQ, iQ = dc.lists(c["zp"], c["zq"], 16)
    w = (c["a"], c["a"], c["b"])
    for fn in (dv.measure, _capi.knn_div_terms):
        for G in (1, 65, -1):
            with pytest.raises(ValueError, match="groups"):
                fn(dP, iP, dQ, iQ, gP, gP, gQ, G, 4, 3, *w)
        with pytest.raises(ValueError, match="ranks"):
            fn(dP, iP, dQ, iQ, gP, gP, gQ, 4, 17, 3, *w)
        with pytest.raises(ValueError, match="ranks"):
            fn(dP, iP, dQ, iQ, gP, gP, gQ, 4, 0, 3, *w)
        with pytest.raises(ValueError, match="shorter"):
            fn(dP[:, :3], iP[:, :3], dQ[:, :3], iQ[:, :3], gP, gP, gQ, 4, 4, 3, *w)
        for k in range(3):
            bad = [gP.copy(), gP.copy(), gQ.copy()]
            bad[k][7] = 4
            with pytest.raises(ValueError, match="group id"):
                fn(dP, iP, dQ, iQ, *bad, 4, 4, 3, *w)
    assert _capi.load().mce_knn_div_terms_f64(dP.ctypes.data, iP.ctypes.data, dQ.ctypes.data, iQ.ctypes.data, 40, 16, None, gP.ctypes.data, gP.ctypes.data, 40,
                                              gQ.ctypes.data, 50, 4, 17, 3, c["a"].ctypes.data, c["a"].ctypes.data, c["b"].ctypes.data, dP.ctypes.data,
                                              iP.ctypes.data, iP.ctypes.data, 0) == _capi.MCE_ERR_K_RANGE
    with pytest.raises(ValueError, match="null pointer"):
        _capi.knn_div_terms_dev(8, 8, 8, 8, 40, 16, 0, 0, 8, 40, 8, 50, 4, 4, 3, 8, 8, 8, 8, 8, 8, 8, 1 << 30)
    with pytest.raises(ValueError, match="workspace"):
        _capi.knn_div_terms_dev(8, 8, 8, 8, 40, 16, 0, 8, 8, 40, 8, 50, 4, 4, 3, 8, 8, 8, 8, 8, 8, 8, 16)
    for bad, words in (((8, 2, 5, 3), "stride"), ((8, 3, 0, 3), "rows"), ((8, 65, 5, 65), "columns"), ((8, 3, 5, 0), "columns")):
        with pytest.raises(ValueError, match=words):
            _capi.div_whiten_dev(bad[0], bad[1], bad[2], bad[3], np.eye(max(bad[3], 1)), np.zeros(max(bad[3], 1)), 8, 8, 8, 1 << 30)
    with pytest.raises(ValueError, match="linv"):
        _capi.div_whiten_dev(8, 3, 5, 3, np.eye(2), np.zeros(3), 8, 8, 8, 1 << 30)
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.knn_div_terms(dP, iP, dQ, iQ, gP, gP, gQ, 4, 4, 3, *w)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.div_whiten(c["zp"], 3, np.eye(3), np.zeros(3), c["a"])
        with pytest.raises(RuntimeError, match="no HIP device"):
            dv.estimate(c["zp"], c["a"], c["zq"], c["b"], native=True)
    for kw, words in ((dict(kmax=17), "ranks"), (dict(kmax=0), "ranks"), (dict(groups=1), "groups"), (dict(groups=65), "groups")):
        with pytest.raises(ValueError, match=words):
            dv.estimate(c["zp"], c["a"], c["zq"], c["b"], native=False, **kw)
    with pytest.raises(ValueError, match="shared parameters"):
        dv.estimate(np.zeros((3, 65)), np.ones(3), np.zeros((3, 65)), np.ones(3), native=False)
    with pytest.raises(ValueError, match="weights"):
        dv.estimate(c["zp"], c["a"][:-1], c["zq"], c["b"], native=False)


def test_estimate_end_to_end_on_the_cpu():
    """raw rows with a metric that is not the identity: the estimate is the deletion model on the rows whitened with P's system"""
    rng = np.random.default_rng(8)
    nP, nQ, d, K, G = 257, 300, 3, 4, 8
    A = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.2, 1.5]])
    xp = rng.standard_normal((nP, d)) @ A.T + np.array([1.0, -2.0, 0.5])
    xq = 1.4 * rng.standard_normal((nQ, d)) @ A.T + np.array([1.2, -1.8, 0.4])
    a, b = rng.integers(1, 5, nP).astype(float), rng.integers(1, 5, nQ).astype(float)
    out = dv.estimate(xp, a, xq, b, kmax=K, groups=G, native=False, names=["x", "y", "z"])
    assert out["status"] == 0 and out["names"] == ["x", "y", "z"] and out["rows_per_level"] == {16: nP} and (out["rows_p"], out["rows_q"], out["dof"]) == (nP, nQ, d)
    from mcevidence_amd import covariance as cv
    cov = cv.measure(a, xp)
    linv = np.tril(np.linalg.solve(np.linalg.cholesky(cov["cov"]), np.eye(d)))
    c = dict(zp=dv.whiten(xp, linv, cov["mean"]), zq=dv.whiten(xq, linv, cov["mean"]), a=a, b=b, d=d)
    dP, iP, dQ, iQ = dc.lists(c["zp"], c["zq"], 16)
    assert dc.min_relative_gap(dP, dQ) >= GAP
    gP, gQ = _groups(c, G)
    _, _, B = dc.oracle_sums(dP, iP, dQ, iQ, gP, gP, gQ, G, K, d, a, a, b)
    D = np.vstack([out["D"][None, :], out["D_groups"]])
    dc.assert_values(D, out["sums"], dc.deletion_model(c, G, K), B, what="estimate")
    s = dv.summarise(out["sums"], dv.masses(a, gP, G), dv.masses(b, gQ, G))
    assert all(np.array_equal(s[k], out[k]) for k in s) and (out["sigma"] > 0).all() and np.array_equal(out["excluded"], np.zeros(K))
    # a linear map of both chains leaves the estimate where it is, up to the rounding of the two whitenings
    M = np.array([[2.0, 0.3, 0.0], [0.0, 0.5, -0.2], [0.1, 0.0, 3.0]])
    again = dv.estimate(xp @ M.T, a, xq @ M.T, b, kmax=K, groups=G, native=False)
    assert np.max(np.abs(again["D"] - out["D"])) < 1e-9
    assert len(dv.lines(out)) == K and dv.lines(out)[0].startswith("   D_KL(P || Q)[k=1] = %s ± %s" % (out["D"][0], out["sigma"][0]))


# ---- the tension route and the command line -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_roots(tmp_path_factory):
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    d = tmp_path_factory.mktemp("gain_roots")
    out = []
    for name, seed, npar, pnames in (("A", 1, 3, ["om", "h", "a_x"]), ("B", 2, 3, ["om", "h", "b_y"]), ("AB", 3, 4, ["om", "h", "a_x", "b_y"])):
        root = str(d / name)
        chains = [gaussian_chain(seed=10 * seed + i, n=400, d=npar, weights="int") for i in range(2)]
        write_cosmomc_chains(root, chains, [(p, -6.0, 6.0) for p in pnames], fmt="%.17g")
        with open(root + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (p, p) for p in pnames))
        out.append(root)
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif k == "names":
            assert a[k] == b[k]
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _rows(root, cols):
    rows = np.concatenate([np.loadtxt(root + "_%d.txt" % i) for i in (1, 2)])
    return rows[:, [2 + j for j in cols]], rows[:, 0]


def test_evidence_tension_gain_on_the_host_route(three_roots, monkeypatch):
    plain = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend())
    off = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), gain=None, gain_k=7, gain_groups=3)
    assert set(plain[3]["tension"]) == {"lnR", "lnI", "lnS", "d", "p", "sigma_equiv", "status", "shift"}
    _same(plain[3]["tension"], off[3]["tension"])
    assert tn.lines(plain[3]["tension"]) == tn.lines(off[3]["tension"]) and len(tn.lines(plain[3]["tension"])) == 2 + 4
    outs = [(e, i) for e, i in zip(plain[:3], plain[3]["roots"])]
    _same(tn.combine(*outs), tn.combine(*outs, gain=None))
    with pytest.raises(ValueError, match="gain="):
        tn.evidence_tension(*three_roots, route="host", gain="kde")
    monkeypatch.setattr(tn, "knn_divergence", lambda xp, wp, xq, wq, device=None, **k: dv.estimate(xp, wp, xq, wq, native=False, **k))
    got = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), gain="knn", gain_k=3, gain_groups=4)
    t = dict(got[3]["tension"])
    g = t.pop("gain")
    _same(plain[3]["tension"], t)                            # every number that exists today, bit for bit
    assert all(np.array_equal(x, y) for x, y in zip(plain[:3], got[:3]))
    assert tuple(g) == tn.GAIN_KEYS == ("AB|A", "AB|B", "A|B", "B|A")
    ra, rb, rab = three_roots
    # the rows are the files' own: the pairs over the parameters they share, by name
    want = {"AB|A": (_rows(rab, [0, 1, 2]), _rows(ra, [0, 1, 2]), ["om", "h", "a_x"]), "AB|B": (_rows(rab, [0, 1, 3]), _rows(rb, [0, 1, 2]), ["om", "h", "b_y"]),
            "A|B": (_rows(ra, [0, 1]), _rows(rb, [0, 1]), ["om", "h"]), "B|A": (_rows(rb, [0, 1]), _rows(ra, [0, 1]), ["om", "h"])}
    for key, ((xp, wp), (xq, wq), names) in want.items():
        ref = dv.estimate(xp, wp, xq, wq, kmax=3, groups=4, native=False, names=names)
        assert g[key]["names"] == names and g[key]["status"] == 0 and g[key]["groups"] == 4
        assert np.array_equal(g[key]["D"], ref["D"]) and np.array_equal(g[key]["sigma"], ref["sigma"]), key
    lines = tn.lines(got[3]["tension"])
    assert lines[:-4] == tn.lines(plain[3]["tension"]) and len(lines) == 2 + 4 + 4
    for line, key in zip(lines[-4:], tn.GAIN_KEYS):
        p, q = key.split("|")
        assert line.startswith("   gain D_KL(%s || %s) (%s): [k=1] %s ± %s" % (p, q, ", ".join(g[key]["names"]), g[key]["D"][0], g[key]["sigma"][0]))
    # the refusals, in information.refuse's words
    for kw, words in ((dict(nbatch=2, brange=[2.0, 2.5]), "gain with batched runs"), (dict(isfunc=lambda x: x), "gain with isfunc is not supported")):
        with pytest.raises(ValueError, match=words):
            tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), gain="knn", **kw)
    from mcevidence_amd import parallel
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    with pytest.raises(ValueError, match="gain under an initialised process group"):
        tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), gain="knn")


def test_both_command_line_forms(three_roots, capsys, monkeypatch):
    from mcevidence_amd import cli, evidence
    ra, rb, rab = three_roots
    p = cli.build_parser()
    assert p.parse_args([rab]).gain_knn is None and p.parse_args([rab, "--tension", ra, rb, "--gain-knn"]).gain_knn == 4 and cli._gain_kw(p.parse_args([rab])) == {}
    assert cli._gain_kw(p.parse_args([rab, "--tension", ra, rb, "--gain-knn", "6", "--gain-groups", "16"])) == {"gain": "knn", "gain_k": 6, "gain_groups": 16}
    for argv, words in (([rab, "--gain-knn"], "belongs to --tension"), ([rab, "--gain-groups", "4"], "belongs to --gain-knn or --divergence"),
                        ([rab, "--tension", ra, rb, "--gain-knn", "17"], "1 .. 16"), ([rab, "--tension", ra, rb, "--gain-knn", "--gain-groups", "1"], "2 .. 64"),
                        ([rab, "--divergence", ra, "0"], "K in 1 .. 16"), ([rab, "--divergence", ra, "--tension", ra, rb], "does not combine")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and words in capsys.readouterr().err, argv
    real = tn.evidence_tension
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    monkeypatch.setattr(tn, "evidence_tension", lambda *a, **k: real(*a, **dict(k, route="host")))          # (no device here: the host route)
    monkeypatch.setattr(tn, "knn_divergence", lambda xp, wp, xq, wq, device=None, **k: dv.estimate(xp, wp, xq, wq, native=False, **k))
    capsys.readouterr()
    got = cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0", "--gain-knn", "2", "--gain-groups", "4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    want = [ln.strip() for ln in tn.lines(got[3]["tension"])]
    at = [out.index(ln) for ln in want]
    assert at == sorted(at) and [w[:17] for w in want[-4:]] == ["gain D_KL(AB || A", "gain D_KL(AB || B", "gain D_KL(A || B)", "gain D_KL(B || A)"]
    assert out.index(tn.FOOTNOTE_GAIN.strip()) == out.index(tn.FOOTNOTE) + 1 and got[3]["tension"]["gain"]["A|B"]["kmax"] == 2
    cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0"])
    plain_out = capsys.readouterr().out
    assert "gain D_KL" not in plain_out and tn.FOOTNOTE_GAIN not in plain_out and tn.FOOTNOTE in plain_out
    # --divergence ROOT_Q [K]: D_KL(root_name || ROOT_Q)[k] = x ± sigma over the shared parameters, from the two roots' host rows
    res = cli.main([ra, "--divergence", rb, "3", "--allparams", "-vb", "0", "--gain-groups", "4"])
    text = capsys.readouterr().out
    ref = dv.estimate(*_rows(ra, [0, 1]), *_rows(rb, [0, 1]), kmax=3, groups=4, native=False)
    assert res["names"] == ["om", "h"] and np.array_equal(res["D"], ref["D"]) and np.array_equal(res["sigma"], ref["sigma"])
    for k in range(3):
        assert "D_KL(%s ‖ %s)[k=%d] = %s ± %s" % (ra, rb, k + 1, ref["D"][k], ref["sigma"][k]) in text
    assert tn.FOOTNOTE_GAIN in text and cli.main([ra, "--divergence", rb, "--allparams", "-vb", "0"])["kmax"] == 4


# ---- Gaussians with a known answer ----------------------------------------------------------------------------------------------------
MU = np.array([0.5, -0.5, 1.0])
CP = np.diag([1.0, 0.5, 2.0])
CQ = 4.0 * np.array([[1.0, 0.3, 0.0], [0.3, 1.0, 0.2], [0.0, 0.2, 1.5]])


def _truth():
    iq = np.linalg.inv(CQ)
    return 0.5 * (np.trace(iq @ CP) + MU @ iq @ MU - 3.0 + np.log(np.linalg.det(CQ) / np.linalg.det(CP)))


_RUNS = {}


def _run(seed):
    """4 000 rows of P against 6 000 of Q, integer weights 1..4, K = 4, G = 8: computed once per seed"""
    if seed not in _RUNS:
        rng = np.random.default_rng(seed)
        xp, xq = rng.multivariate_normal(MU, CP, 4000), rng.multivariate_normal(np.zeros(3), CQ, 6000)
        a, b = rng.integers(1, 5, 4000).astype(float), rng.integers(1, 5, 6000).astype(float)
        out = dv.estimate(xp, a, xq, b, kmax=4, groups=8, native=False)
        _RUNS[seed] = (out["D"], out["sigma"])
    return _RUNS[seed]


def test_the_estimate_is_within_5_sigma_of_the_truth():
    """P = N(mu, diag(1, 0.5, 2)), Q = N(0, 4 [[1, .3, 0], [.3, 1, .2], [0, .2, 1.5]]), mu = (0.5, -0.5, 1): truth 1.3018 nat.  Seeds 0-4:
    |D[k] - truth| <= 5 sigma[k] for k = 1, 2, 3; k = 4 is recorded and not asserted."""
    truth = _truth()
    assert abs(truth - 1.3018) < 5e-5
    for seed in range(5):
        D, sigma = _run(seed)
        pull = (D - truth) / sigma
        print("seed %d: D = %s  sigma = %s  (D - truth) / sigma = %s" % (seed, D, sigma, np.array2string(pull, precision=2)))
        assert (np.abs(pull[:3]) <= 5.0).all(), (seed, pull)


def test_sigma_is_calibrated():
    """the mean jackknife sigma over the empirical standard deviation of D[k] over seeds 0-15 lies in [0.7, 2.0]"""
    runs = [_run(seed) for seed in range(16)]
    ratio = np.mean([s for _, s in runs], axis=0) / np.std([D for D, _ in runs], axis=0, ddof=1)
    print("mean sigma / empirical sd of D, k = 1..4: %s" % np.array2string(ratio, precision=3))
    assert ratio.shape == (4,) and (ratio >= 0.7).all() and (ratio <= 2.0).all(), ratio
