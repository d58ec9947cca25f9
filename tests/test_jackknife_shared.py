"""The jackknife's shared rule on the CPU (docs/design/jackknife.md): csrc/jack.hpp through its stand-alone program (AddressSanitizer +
UBSan) and jackknife.jackknife_host against brute-force DELETION (tests/jack_cases.py: delete the group, search again), the group
ids, the error cases, ``evidence_jackknife`` on a backend without a device, and the calibration of sigma.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import jack_cases as jc
from helpers import LNE_TOL, REPO, OracleBackend, OracleFeedBackend
from mcevidence_amd import _capi, jackknife as jk
from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains

CASES = {
    "A_iid": lambda: jc.case_iid(),
    "B_walk": lambda: jc.case_walk(),
    "C_planted": lambda: jc.case_planted(),
    "D_257_G2": lambda: jc.case_iid(n=257, G=2, seed=21),
    "D_300_G64": lambda: jc.case_iid(n=300, G=64, seed=22),
    "E_empty_group": lambda: jc.case_cross(empty_group=3),
    "G_cross": lambda: jc.case_cross(),
}


@pytest.fixture(scope="module")
def jack_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jack") / "jack_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"), os.path.join(REPO, "tests", "native", "jack_check.cpp"), "-o", exe])
    return exe


def test_native_unit_checks(jack_check):
    assert subprocess.check_output([jack_check]).decode().startswith("ok ")


def _ladder_with(level, c):
    """run_ladder over a level function (L, qid or None) -> sums; lists come from the exact search of jack_cases"""
    X, Y = c["X"], c["Y"]

    class Session(object):
        def level(self, L, rows):
            sel = np.arange(len(X)) if rows is None else rows
            if Y is None:
                dist, idx = jc.exact_lists(X[sel], X, min(L, len(X) - 1), own=sel)
            else:
                dist, idx = jc.exact_lists(X[sel], Y, min(L, len(Y)))
            return level(dist, idx, None if rows is None else rows)

        def share(self, L, rows):
            return 1.0
    return jk.run_ladder(Session(), len(X), c["G"], c["k0"], c["kmax"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_model_and_native_driver_against_deletion(name, jack_check, tmp_path):
    c = CASES[name]()
    want_g, want_f = jc.deletion_model(c["X"], c["Y"], c["gq"], c["gr"], c["G"], c["k0"], c["kmax"], c["w"], c["fs"])
    n = len(c["X"])

    def host(dist, idx, qid):
        sel = slice(None) if qid is None else qid
        return jk.jackknife_host(dist, idx, c["gq"][sel], c["gr"], c["G"], c["k0"], c["kmax"], c["d"], c["w"][sel], c["fs"][sel], qid=qid)

    def native(dist, idx, qid):
        jc.write_case(str(tmp_path / "case.bin"), dist, idx, c, qid=qid)
        subprocess.check_call([jack_check, str(tmp_path / "case.bin"), str(tmp_path / "out.txt")])
        return jc.read_result(str(tmp_path / "out.txt"), c["G"], c["kmax"])

    levels = {}
    for what, fn in (("jackknife_host", host), ("jack_serial", native)):
        g, f, per_level = _ladder_with(fn, c)
        jc.assert_sums(g, f, want_g, want_f, n, c["k0"], what="%s %s" % (name, what))
        lf, lg = jc.lnE_groups(g, f, c["gq"], c["G"], c["k0"], c["kmax"], c["w"])
        wf, wg = jc.lnE_groups(want_g, want_f, c["gq"], c["G"], c["k0"], c["kmax"], c["w"])
        assert np.max(np.abs(lf - wf)) <= LNE_TOL and np.max(np.abs(lg - wg)) <= LNE_TOL
        levels[what] = per_level
    assert levels["jackknife_host"] == levels["jack_serial"]
    if name == "A_iid":
        assert levels["jackknife_host"] == {16: n}
    if name == "B_walk":
        assert set(levels["jackknife_host"]) == {16, 32} and levels["jackknife_host"][32] > 0
    if name == "C_planted":
        assert levels["jackknife_host"] == {16: n, 32: 3, 128: 3}


def test_planted_case_short_rows_ascending_and_exact():
    c = jc.case_planted()
    for L in (16, 32):
        dist, idx = jc.exact_lists(c["X"], c["X"], L, own=np.arange(640))
        _, _, short = jk.jackknife_host(dist, idx, c["gq"], c["gr"], c["G"], 1, c["kmax"], 3, c["w"], c["fs"])
        assert short.tolist() == [10, 330, 500] == jc.short_rows(idx, c["gq"], c["gr"], c["G"], 4).tolist()
    dist, idx = jc.exact_lists(c["X"], c["X"], 64, own=np.arange(640))
    assert len(jc.short_rows(idx, c["gq"], c["gr"], c["G"], 4)) == 0


def test_summarise():
    v = np.array([[1.0, 0.0], [2.0, 0.0], [4.0, 0.0], [5.0, 0.0]])
    sigma, bc = jk.summarise(np.array([3.5, 1.0]), v)
    assert np.allclose(sigma, [np.sqrt(7.5), 0.0], rtol=1e-15) and np.allclose(bc, [5.0, 4.0], rtol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- group ids
def _chain(n, seed, d=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    return np.column_stack([rng.integers(1, 4, n).astype(float), 0.5 * (x * x).sum(axis=1), x])


def test_group_ids_under_split_shuffle_and_set_split():
    import mcevidence_amd as pkg
    ch = _chain(1000, 1)
    m = pkg.MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend())
    assert np.array_equal(jk.group_ids(m.gd, "s1", 16), np.arange(1000) * 16 // 1000)
    np.random.seed(3)
    m = pkg.MCEvidence([ch], kmax=3, verbose=0, split=True, backend=OracleBackend())
    r1, r2 = np.asarray(m.gd.data["s1"].ichain), np.asarray(m.gd.data["s2"].ichain)
    assert sorted(np.concatenate([r1, r2]).tolist()) == list(range(1000)) and not np.array_equal(r1, np.sort(r1))
    assert np.array_equal(jk.group_ids(m.gd, "s1", 8), r1 * 8 // 1000) and np.array_equal(jk.group_ids(m.gd, "s2", 8), r2 * 8 // 1000)
    # the rows themselves say which stretch of chain they are: the group of a row of s1 is the group of the chain row it copies
    g = np.arange(1000) * 8 // 1000
    assert np.array_equal(m.gd.data["s1"].samples, ch[r1, 2:]) and np.array_equal(jk.group_ids(m.gd, "s1", 8), g[r1])
    m = pkg.MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).set_split(np.arange(0, 400), np.arange(400, 1000))
    assert jk.group_ids(m.gd, "s1", 10).max() == 3 and jk.group_ids(m.gd, "s2", 10).min() == 4       # s1 holds no row of groups 4..9
    # two input arrays: by="chains" labels them
    m = pkg.MCEvidence([ch[:300], ch[300:]], kmax=3, verbose=0, backend=OracleBackend())
    assert np.array_equal(jk.group_ids(m.gd, "s1", 2, by="chains"), (np.arange(1000) >= 300).astype(int))
    with pytest.raises(ValueError, match="by="):
        jk.group_ids(m.gd, "s1", 2, by="files")


def test_chain_labels_survive_thinning(tmp_path):
    from mcevidence_amd.chains import MCSamples, thin_rows
    parts = [_chain(400, 5), _chain(300, 6), _chain(500, 7)]
    root = str(tmp_path / "c")
    write_cosmomc_chains(root, parts, fmt="%.17g")
    plain = MCSamples(root)
    assert np.array_equal(plain.row_chain, np.repeat([0, 1, 2], [400, 300, 500]))
    gd = MCSamples(root, burnlen=50, thinlen=3.0)
    burned = np.concatenate([p[50:] for p in parts])
    keep, _ = thin_rows(burned[:, 0], 3.0)
    assert np.array_equal(gd.row_chain, np.repeat([0, 1, 2], [350, 250, 450])[keep]) and len(gd.row_chain) == gd.samples.shape[0]
    assert np.array_equal(gd.samples[:, 2:], burned[keep, 2:])          # thinning itself is what it was
    g = jk.group_ids(gd, "s1", 3, by="chains")
    assert np.array_equal(g, gd.row_chain) and g.dtype == np.int32


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_cases():
    import mcevidence_amd as pkg
    c = jc.case_iid(n=100, G=4)
    dist, idx = jc.exact_lists(c["X"], c["X"], 16, own=np.arange(100))
    args = (c["gq"], c["gr"])
    for G in (1, 65):
        with pytest.raises(ValueError, match="groups"):
            jk.jackknife_host(dist, idx, *args, G, 1, 5, 3, c["w"], c["fs"])
        with pytest.raises(ValueError, match="groups"):
            _capi.jack_dotp(dist, idx, *args, G, 1, 5, 3, c["w"], c["fs"])
    bad = c["gq"].copy()
    bad[7] = 4
    with pytest.raises(ValueError, match="group id"):
        jk.jackknife_host(dist, idx, bad, c["gr"], 4, 1, 5, 3, c["w"], c["fs"])
    with pytest.raises(ValueError, match="group id"):
        _capi.jack_dotp(dist, idx, bad, c["gr"], 4, 1, 5, 3, c["w"], c["fs"])
    with pytest.raises(ValueError, match="group id"):
        _capi.jack_dotp(dist, idx, c["gq"], bad, 4, 1, 5, 3, c["w"], c["fs"])
    with pytest.raises(ValueError, match="shorter"):
        jk.jackknife_host(dist[:, :3], idx[:, :3], *args, 4, 1, 5, 3, c["w"], c["fs"])
    with pytest.raises(ValueError, match="shorter"):
        _capi.jack_dotp(dist[:, :3], idx[:, :3], *args, 4, 1, 5, 3, c["w"], c["fs"])
    assert _capi.jack_workspace_bytes(1000, 16, 5) >= 4 * 17 * 5 * 8
    with pytest.raises(ValueError):
        _capi.jack_workspace_bytes(1000, 65, 5)
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.jack_dotp(dist, idx, *args, 4, 1, 5, 3, c["w"], c["fs"])
    ch = _chain(400, 9)
    with pytest.raises(ValueError, match="brange"):
        pkg.MCEvidence([ch], kmax=3, verbose=0, nbatch=2, brange=[2.0, 2.5], bscale="logpower", backend=OracleBackend()).evidence_jackknife()
    np.random.seed(1)
    with pytest.raises(ValueError, match="split=True and covtype='single'"):
        pkg.MCEvidence([ch], kmax=3, verbose=0, split=True, backend=OracleBackend()).evidence_jackknife(covtype="single")
    with pytest.raises(ValueError, match="at least 2 chains"):
        pkg.MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence_jackknife(by="chains")
    with pytest.raises(ValueError, match="groups"):
        pkg.MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence_jackknife(groups=65)


def test_refused_under_a_process_group(monkeypatch):
    import mcevidence_amd as pkg
    from mcevidence_amd import parallel
    m = pkg.MCEvidence([_chain(400, 9)], kmax=3, verbose=0, backend=OracleBackend())
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        jk.evidence_jackknife(m)


def test_capacity_error_names_the_short_rows():
    c = jc.case_capacity()

    def host(dist, idx, qid):
        sel = slice(None) if qid is None else qid
        return jk.jackknife_host(dist, idx, c["gq"][sel], c["gr"], c["G"], 1, c["kmax"], 3, c["w"][sel], c["fs"][sel], qid=qid)
    with pytest.raises(ValueError, match=r"1 row still short after lists of 1024"):
        _ladder_with(host, c)


# ---------------------------------------------------------------------------------------------------------------- MCEvidence
def _whitened(m):
    cs = m.get_covariance()
    s1 = m.gd.arrays("s1")[0][:, :m.ndim]
    X = m.diagonalise_chain(s1, cs["eVec"], cs["eVal"])
    Y = m.diagonalise_chain(m.gd.arrays("s2")[0][:, :m.ndim], cs["eVec"], cs["eVal"]) if m.split else None
    return X, Y, cs["J"]


def _model_lnE(m, G, by):
    """ln E of every deleted group by brute-force deletion on the whitened rows of ``m``, finished as evidence() finishes"""
    from mcevidence_amd.resident import mle_from_sums
    X, Y, J = _whitened(m)
    _, lnp, w = m.gd.arrays("s1")
    logLmax = float(np.max(lnp))
    gq = jk.group_ids(m.gd, "s1", G, by)
    gr = jk.group_ids(m.gd, "s2", G, by) if m.split else gq
    k0 = 0 if m.split else 1
    dg, df = jc.deletion_model(X, Y, gq, gr, G, k0, m.kmax, np.asarray(w), lnp - logLmax)
    aw = m.gd.data["s1"].adjusted_weights
    return np.stack([mle_from_sums(dg[b], J, np.sum(aw[gq != b]), logLmax, int((gq != b).sum()), m.kmax, 0.0, m.split)[1:] for b in range(G)])


@pytest.mark.parametrize("split", [False, True])
def test_evidence_jackknife_on_the_cpu_backend(split):
    import mcevidence_amd as pkg
    ch = _chain(900, 31)
    np.random.seed(5)
    m = pkg.MCEvidence([ch], kmax=4, verbose=0, split=split, backend=OracleFeedBackend())
    plain = m.evidence(covtype="all")
    assert "jackknife" not in m.info
    out = m.evidence_jackknife(groups=8)
    assert sorted(out) == ["by", "groups", "lnE", "lnE_bias_corrected", "lnE_groups", "rows_per_level", "sigma"]
    assert np.max(np.abs(out["lnE"] - plain)) <= LNE_TOL
    assert np.max(np.abs(out["lnE_groups"] - _model_lnE(m, 8, "blocks"))) <= LNE_TOL
    sigma, bc = jk.summarise(out["lnE"], out["lnE_groups"])
    assert np.array_equal(sigma, out["sigma"]) and np.array_equal(bc, out["lnE_bias_corrected"]) and (sigma > 0).all()
    assert out["groups"] == 8 and out["by"] == "blocks" and out["rows_per_level"][16] == m.nsample[0]
    m.jackknife = 8
    again = m.evidence(covtype="all")
    assert np.array_equal(again, plain) and np.array_equal(m.info["jackknife"]["lnE_groups"], out["lnE_groups"])


def test_evidence_jackknife_by_chains_and_cli(tmp_path, capsys):
    import mcevidence_amd as pkg
    from mcevidence_amd import cli, evidence
    chains, _, ranges = planck_like_chains(seed=1, rows=(300, 260, 320, 280))
    root = str(tmp_path / "planck")
    write_cosmomc_chains(root, chains, ranges=ranges, fmt="%.17g")
    m = pkg.MCEvidence(root, kmax=3, ndim=6, verbose=0, backend=OracleFeedBackend())
    out = m.evidence_jackknife(by="chains")
    assert out["groups"] == 4 and out["lnE_groups"].shape == (4, 2)
    assert np.max(np.abs(out["lnE_groups"] - _model_lnE(m, 4, "chains"))) <= LNE_TOL
    # the command line prints x +- sigma per k
    real = evidence.HipBackend
    evidence.HipBackend = OracleFeedBackend
    try:
        cli.main([root, "-k", "3", "-np", "6", "-vb", "0", "--jackknife=4", "--jackknife-by", "chains"])
    finally:
        evidence.HipBackend = real
    text = capsys.readouterr().out
    assert "ln(B)[k=1] = " in text and "ln(B)[k=2] = " in text and text.count("±") >= 3


# ---------------------------------------------------------------------------------------------------------------- calibration
def test_sigma_is_conservative_on_iid_gaussians():
    """N = 2000, d = 3, G = 16, K = 3, 40 seeded iid Gaussian realisations, unit weights, logL = -|x|^2 / 2: the mean jackknife sigma
    over the empirical standard deviation of ln E lies in [1.0, 2.5] for k = 1..3 (a jackknife variance is conservative in
    expectation: Efron-Stein)."""
    import mcevidence_amd as pkg
    lnE, sig = [], []
    for seed in range(40):
        x = np.random.default_rng(1000 + seed).standard_normal((2000, 3))
        ch = np.column_stack([np.ones(2000), 0.5 * (x * x).sum(axis=1), x])
        out = pkg.MCEvidence([ch], kmax=4, verbose=0, backend=OracleBackend()).evidence_jackknife(groups=16)
        lnE.append(out["lnE"])
        sig.append(out["sigma"])
    ratio = np.mean(sig, axis=0) / np.std(lnE, axis=0, ddof=1)
    print("mean sigma / empirical sd of ln E, k = 1..3: %s" % np.array2string(ratio, precision=3))
    assert ratio.shape == (3,) and (ratio >= 1.0).all() and (ratio <= 2.5).all(), ratio
