"""covariance without a GPU: the serial driver of mcevidence_amd/csrc/param_cov.hpp (tests/native/param_cov_check.cpp, built with
-fsanitize=address,undefined as a stand-alone program) and its NumPy form ``covariance.measure`` against the exact integer model of
tests/cov_cases.py within the bounds of docs/design/tension.md; the keyword through ``MCEvidence`` (auto and cross, the host loop and the
device-feeder hook, ``evidence_many``), the refusals, ``resident.plan``, every status, the names, the new symbols and their argument
errors."""
import logging
import os
import struct
import subprocess

import numpy as np
import pytest

import cov_cases as cc
from helpers import REPO, OracleBackend, OracleFeedBackend
from mcevidence_amd import covariance as cv
from mcevidence_amd.evidence import MCEvidence, evidence_many
from mcevidence_amd.synth import gaussian_chain


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("param_cov") / "param_cov_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "param_cov_check.cpp"), "-o", exe])
    return exe


def run_native(exe, tmp_path, systems):
    """[(a, x[n, ld], d)] through the sanitized program -> one block dict per system"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        for a, x, d in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            x = x if x.ndim == 2 else x.reshape(len(a), -1)
            fh.write(struct.pack("<qqq", len(a), d, x.shape[1]))
            fh.write(x.tobytes())
            fh.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    out = subprocess.run([exe, "cov", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(systems)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = np.frombuffer(open(fout, "rb").read(), dtype="<f8")
    blocks, at = [], 0
    for a, x, d in systems:
        size = cv.HEAD + d + d * (d + 1) // 2
        blocks.append(cv.from_block(raw[at:at + size], d))
        at += size
    assert at == raw.size
    return blocks


def test_blocks_cover_the_upper_triangle_once(checker):
    out = subprocess.run([checker, "blocks"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok records=127", out.stdout + out.stderr


def test_serial_driver_and_numpy_form_equal_the_exact_model(checker, tmp_path):
    cases = cc.cpu_cases()
    assert len(cases) == 12 * 4 + 3 and max(c.exact["rows"] for c in cases if c.d == 127) == 65
    native = run_native(checker, tmp_path, [(c.a, c.x, c.d) for c in cases])
    for c, nat in zip(cases, native):
        cc.check(c, nat, "native")
        num = cv.measure(c.a, c.x[:, :c.d])
        cc.check(c, num, "numpy ")
        cc.check_info(c, cv.build(num), "numpy ")


def test_the_device_cases_on_the_host(checker, tmp_path):
    # what the device is asked (tests/test_gpu_param_cov.py), asked of the two host forms: the centring, zero weights over NaN and inf,
    # identical / negated / constant columns, +-1e150 beside +-1e-150, denormals, d = 127 with ld > d
    names = ["B_centring", "C_skipped", "D_structure", "D_denormal", "A_513_127", "A_65_127", "A_1025_17", "F_c"]
    g = cc.gpu_cases()
    native = run_native(checker, tmp_path, [(g[n].a, g[n].x, g[n].d) for n in names])
    for n, nat in zip(names, native):
        cc.check(g[n], nat, "native")
        cc.check_info(g[n], cv.build(cv.measure(g[n].a, g[n].x[:, :g[n].d])), "numpy ")
    C = cv.measure(g["D_structure"].a, g["D_structure"].x)["cov"]
    assert C[0, 0] == C[0, 1] == C[1, 1] == -C[0, 2] == C[2, 2] and np.all(C[3] == 0.0) and np.array_equal(C, C.T)
    # the oracle's two integer paths agree
    c = g["A_65_127"]
    big = cc.exact(c.a, c.x[:, :5] * (1.0 + 2.0 ** -40))          # (53-bit values: Python integers)
    small = cc.exact(c.a, c.x[:, :5])
    assert np.allclose(big["cov"], small["cov"], rtol=1e-10, atol=0) and np.array_equal(small["cov"], small["cov"].T)


def test_status_cases_of_both_forms(checker, tmp_path, caplog):
    cases = cc.status_cases()
    native = run_native(checker, tmp_path, [(a, x, x.shape[1]) for _, a, x, _, _ in cases])
    for (name, a, x, status, column), nat in zip(cases, native):
        for got in (nat, cv.measure(a, x)):
            assert (got["status"], got["column"]) == (status, column), (name, got["status"], got["column"])
            assert got["rows"] == int(np.count_nonzero(a != 0)), (name, got)
            assert all(np.isnan(got[k]).all() for k in ("W", "A2", "mean", "cov")), (name, got)
    # the dict: every value NaN, the status kept, one WARNING in the route-independent words, nothing raised
    for status in (3, 5):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            d = cv.build(cv._nan_block(3, 7, status, -1))
        warned = [r for r in caplog.records if r.levelno == logging.WARNING]
        assert len(warned) == 1 and "covariance: status %d" % status in warned[0].getMessage() and cv.STATUS_WORDS[status] in warned[0].getMessage()
        assert d["status"] == status and d["rows"] == 7 and d["names"] == ["p0", "p1", "p2"] and d["cov"].shape == d["corr"].shape == (3, 3)
        assert all(np.isnan(d[k]).all() for k in ("sum_w", "ess", "mean", "sd", "cov", "corr"))


def test_keyword_values_sd_and_corr():
    assert cv.spec(None) is None and cv.spec(False) is None and cv.spec(True) is True
    for bad in (1, 0.5, "yes", (True,), {}):
        with pytest.raises(ValueError, match="covariance="):
            cv.spec(bad)
    x = np.array([[1.0, 5.0, 2.0], [2.0, 5.0, 1.0], [4.0, 5.0, 0.5]])
    d = cv.build(cv.measure(np.array([1.0, 2.0, 1.0]), x))
    assert d["sd"][1] == 0.0 and np.isnan(d["corr"][1]).all() and np.isnan(d["corr"][:, 1]).all() and d["corr"][0, 0] == 1.0 == d["corr"][2, 2]
    assert np.array_equal(d["cov"], d["cov"].T) and np.array_equal(d["corr"], d["corr"].T, equal_nan=True) and d["corr"][0, 2] < 0
    assert np.array_equal(cv.unpack([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 3), [[1, 2, 3], [2, 4, 5], [3, 5, 6]])


def _inputs(m):
    """(a, x) of the rule for an MCEvidence object, formed apart from the package's code path"""
    part = m.gd.data["s1"]
    return np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)[:, :m.ndim]


KEYS = {"names", "rows", "sum_w", "ess", "mean", "cov", "sd", "corr", "status", "column"}


def _check_dict(d, a, x, what):
    assert set(d) == KEYS, (what, set(d) ^ KEYS)
    cc.check_info(cc.Case(what, a, x), d, what)
    assert d["cov"].shape == d["corr"].shape == (x.shape[1], x.shape[1]) and len(d["names"]) == x.shape[1]


def test_mcevidence_auto_and_cross_forms():
    ch = gaussian_chain(seed=3, n=1500, d=4, weights="int")
    for split, backend in ((False, OracleBackend), (True, OracleBackend), (False, OracleFeedBackend), (True, OracleFeedBackend)):
        np.random.seed(5)
        m = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend(), covariance=True)
        lnE, info = m.evidence(info=True)
        a, x = _inputs(m)
        assert len(a) == (750 if split else 1500) and m.param_cov is info["covariance"]
        _check_dict(info["covariance"], a, x, "split=%s %s" % (split, backend.__name__))
        np.random.seed(5)
        plain, pinfo = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend()).evidence(info=True)
        assert np.array_equal(lnE, plain) and "covariance" not in pinfo
    # the rows are the chain's own: raw, not whitened; C_jj is summary's var within the two bounds
    both = MCEvidence([ch], kmax=4, verbose=0, backend=OracleBackend(), covariance=True, summary=True).evidence(info=True)[1]
    case = cc.Case("with summary", ch[:, 0], ch[:, 2:])
    bvar = 2.0 * (1500 + 1) * cc.EPS * np.diagonal(case.exact["cov"]) + case.bound["mean"] ** 2
    assert np.all(np.abs(np.diagonal(both["covariance"]["cov"]) - both["summary"]["var"]) <= bvar + np.diagonal(case.bound["cov"]))
    assert np.all(np.abs(both["covariance"]["mean"] - both["summary"]["mean"]) <= 2 * case.bound["mean"])
    # ndim below the sampled parameters
    m = MCEvidence([ch], kmax=3, verbose=0, ndim=2, backend=OracleBackend(), covariance=True)
    lnE, info = m.evidence(info=True)
    assert info["covariance"]["mean"].shape == (2,) and info["covariance"]["cov"].shape == (2, 2)
    _check_dict(info["covariance"], *_inputs(m), "ndim=2")
    # with the jackknife set the covariance is what it is without it
    with_jk = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=True, jackknife=4).evidence(info=True)[1]["covariance"]
    without = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=True).evidence(info=True)[1]["covariance"]
    assert all(np.array_equal(np.asarray(with_jk[k]), np.asarray(without[k])) for k in KEYS - {"names"}) and "sigma" not in with_jk
    # evidence_many fills it too
    ms = [MCEvidence([gaussian_chain(seed=s, n=401, d=3, weights="int")], kmax=3, verbose=0, backend=OracleBackend(), covariance=True) for s in (1, 2)]
    for m, (lnE, info) in zip(ms, evidence_many(ms, info=True)):
        _check_dict(info["covariance"], *_inputs(m), "evidence_many")


def test_without_the_keyword_nothing_changes():
    ch = gaussian_chain(seed=8, n=900, d=3, weights="int")
    a, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence(info=True)
    assert "covariance" not in info
    for off in (None, False):
        b, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=off).evidence(info=True)
        assert "covariance" not in info and np.array_equal(a, b)
    c, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=True).evidence(info=True)
    assert np.array_equal(a, c) and "covariance" in info


def test_refused_combinations_and_the_plan():
    ch = gaussian_chain(seed=2, n=2000, d=3)
    with pytest.raises(ValueError, match="covariance with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=3, brange=[2.5, 3.2], bscale="logpower", backend=OracleBackend(), covariance=True)
    with pytest.raises(ValueError, match="covariance with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=2, backend=OracleBackend(), covariance=True)
    with pytest.raises(ValueError, match="covariance with isfunc"):
        MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend(), covariance=True)
    with pytest.raises(ValueError, match="covariance="):
        MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=1.5)
    MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend())      # neither refusal without the keyword
    # the words are information.refuse's
    from mcevidence_amd import information
    for kw in (dict(nbatch=2), dict(brange=[2.5, 3.2]), dict(isfunc=abs)):
        with pytest.raises(ValueError) as e_cov:
            cv.refuse(True, **kw)
        with pytest.raises(ValueError) as e_inf:
            information.refuse(True, **kw)
        assert str(e_cov.value) == str(e_inf.value).replace("information", "covariance", 1)
    from mcevidence_amd import resident
    assert resident.plan(covariance=True) == resident.RESIDENT == resident.plan()
    with pytest.raises(ValueError, match="covariance="):
        resident.plan(covariance=2.0)
    assert not any("covariance" in k or "covariance=" in v for k, v in resident.REASONS.items())
    # every existing reason, in its order
    for kw, key in ((dict(ischain=False), "ischain"), (dict(thinlen=-1), "negative_thinlen"), (dict(thinlen=0.5), "poisson"), (dict(isfunc=abs), "isfunc"),
                    (dict(nbatch=2), "batches"), (dict(verbose=2), "verbose"), (dict(covtype="diag"), "covtype"), (dict(split=True, covtype="single"), "split_single"),
                    (dict(split=True, jackknife=4), "jackknife_cross"), (dict(ndim=128), "ndim"), (dict(distributed=True), "distributed"),
                    (dict(ncols=[5, 6]), "columns"), (dict(nrows=1), "rows")):
        assert resident.plan(**kw) == resident.plan(covariance=True, **kw) == resident.REASONS[key], key
    assert resident.plan(thinlen=0.5, isfunc=abs, covariance=True) == resident.REASONS["poisson"]


def test_status_through_mcevidence(caplog):
    ch = gaussian_chain(seed=6, n=800, d=3, weights="int")
    bad = ch.copy()
    bad[123, 3] = np.inf                                   # a value that is not finite in the second measured column
    plain = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend()).evidence()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        lnE, info = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend(), covariance=True).evidence(info=True)
        assert info["covariance"]["status"] == 0           # (the column is not measured)
        caplog.clear()
        m = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend(), covariance=True)
        m.ndim = 2                                         # (measure it without sending the row through a search)
        m._fill_covariance()
    d = m.info["covariance"]
    assert np.array_equal(lnE, plain)
    assert d["status"] == 3 and d["column"] == 1 and d["rows"] == 800
    assert all(np.isnan(d[k]).all() for k in ("sum_w", "ess", "mean", "sd", "cov", "corr"))
    assert sum("covariance: status 3" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING) == 1


def test_parameter_names(tmp_path):
    from mcevidence_amd.synth import write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=400, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    with open(root + ".paramnames", "w") as fh:
        fh.write("om0\t\\Omega_0\nom1   \\Omega_1\n\nom2\n")
    m = MCEvidence(root, kmax=3, verbose=0, backend=OracleBackend(), covariance=True)
    m.evidence()
    assert m.param_cov["names"] == ["om0", "om1", "om2"]
    assert MCEvidence([gaussian_chain(seed=1, n=300, d=2)], kmax=3, verbose=0, backend=OracleBackend(), covariance=True).evidence(info=True)[1]["covariance"]["names"] == ["p0", "p1"]


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    lib = _capi.load()
    for s in ("mce_param_cov_out_doubles", "mce_param_cov_workspace_bytes", "mce_param_cov_dev", "mce_param_cov_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_COV_HEAD == cv.HEAD == 8
    assert _capi.param_cov_out_doubles(27) == 8 + 27 + 27 * 28 // 2 == _capi.cov_block_doubles(27)
    assert _capi.param_cov_out_doubles(0) == 0 == _capi.param_cov_out_doubles(128) and _capi.param_cov_out_doubles(127) == 8 + 127 + 8128
    small, wide = _capi.param_cov_workspace_bytes(1000, 1, 8), _capi.param_cov_workspace_bytes(1000, 1, 127)
    assert 0 < small < 2 ** 16 and small < wide < 2 ** 20
    # the tiles' blocks dominate: 2 KB per tile and 16 x 16 block
    assert 1954 * 3 * 2048 < _capi.param_cov_workspace_bytes(10 ** 6, 1, 27) < 2 * 1954 * 3 * 2048
    for bad in ((-1, 1, 4), (10, 0, 4), (10, 1, 0), (10, 1, 128), (10, (1 << 16) + 1, 4)):
        assert _capi.param_cov_workspace_bytes(*bad) == 0, bad
    # argument errors come before any device call
    ok = (1, 4, 5, 4, 1)
    for segs, words in (([], "segments"), ([(1, 3, 5, 4, 1)], "segment 0"), ([(1, 4, 5, 0, 1)], "segment 0"), ([ok, (1, 200, 5, 128, 1)], "segment 1"),
                        ([(1, 4, -1, 4, 1)], "segment 0"), ([(0, 4, 5, 4, 1)], "segment 0"), ([(1, 4, 5, 4, 0)], "segment 0")):
        with pytest.raises(ValueError, match=words):
            _capi.param_cov_dev(segs, 1, 1 << 30)
    with pytest.raises(ValueError, match="null pointer"):
        _capi.param_cov_dev([ok], 0, 1 << 30)
    with pytest.raises(ValueError):
        _capi.param_cov([(np.zeros((3, 2)), 2, np.zeros(4))])


def test_no_device_is_its_own_error():
    from mcevidence_amd import _capi
    c = cc.cpu_cases()[20]
    if _capi.device_count() > 0:                           # (a device is visible: the same call answers)
        assert cv.from_block(_capi.param_cov([c.system])[0], c.d)["status"] == 0
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_cov([c.system])
    # the device form: valid arguments, so the refusal is the missing device's (argument errors come first and need none)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_cov_dev([(8, 4, 5, 4, 8)], 8, 1 << 30)


def test_under_a_process_group_every_rank_computes_its_own_on_the_host(monkeypatch):
    import torch.distributed as dist
    from mcevidence_amd import parallel
    ch = gaussian_chain(seed=12, n=700, d=3, weights="int")
    want = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=True).evidence(info=True)[1]["covariance"]
    m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), covariance=True)

    def refuse(*a, **k):
        raise AssertionError("a collective was called")
    monkeypatch.setattr(parallel, "is_distributed", lambda *a, **k: True)
    for name in ("all_reduce", "all_gather", "all_gather_object", "broadcast", "broadcast_object_list", "barrier", "reduce", "gather", "all_to_all_single"):
        monkeypatch.setattr(dist, name, refuse)
    m._fill_covariance()
    got = m.info["covariance"]
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True) for k in KEYS - {"names"}) and got["names"] == want["names"]
    from mcevidence_amd import resident
    assert resident.plan(distributed=True, covariance=True) == resident.REASONS["distributed"]
