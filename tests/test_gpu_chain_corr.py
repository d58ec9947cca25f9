"""thin_corr on the device: ``mce_chain_corr_dev`` (csrc/chain_corr_kernels.hpp) on every case of tests/corr_cases.py against the
longdouble oracle, with the rho table; two runs bit for bit; a chain alone and beside a copy of itself; the resident route and the
farm with ``thin_corr``; the status cases in the host's words."""
import numpy as np
import pytest

import corr_cases as cc

pytestmark = pytest.mark.gpu

LNE_PARITY = 1e-9           # tests/test_gpu_resident.py: the resident route against the host route


def measure_dev(parts, ndim=None, max_lag=cc.MAX_LAG, min_corr=cc.MIN_CORR):
    """mce_chain_corr_dev on device copies of ``parts``"""
    import torch
    from mcevidence_amd import _capi
    tensors = [torch.from_numpy(np.array(p, dtype=np.float64)).to("cuda:0") for p in parts]
    table = [(t.data_ptr() if t.shape[0] else 0, int(t.shape[0])) for t in tensors]
    ncols = int(parts[0].shape[1])
    nd = ncols - 2 if ndim is None else ndim
    wsb = _capi.chain_corr_workspace_bytes(sum(n for _, n in table), len(table), nd, max_lag)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.chain_corr_dev(table, ncols, 0, 2, nd, min_corr, max_lag, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream, want_rho=True)
    torch.cuda.synchronize()
    return got


def measure_case(name):
    parts, kw, want = cc.case(name)
    return measure_dev(parts, kw.get("ndim"), kw.get("max_lag", cc.MAX_LAG)), want


@pytest.mark.parametrize("name", cc.NUMERIC)
def test_device_equals_the_oracle(name):
    got, want = measure_case(name)
    cc.check(name, got, want)
    # the windows double: 128, 256, 512, .. lags, up to the cap; none after the one with the last cut
    assert got["rho_rows"] == cc.lags_summed(want)
    assert np.all(got["rho"][0] == 1.0)


def test_windows_stop_after_the_last_cut():
    """one, two and three waits: T1 ends in the first window, T3 in the second, T5_far in the third (tests/corr_cases.py asserts where
    their cuts lie), and the whole table up to there is the oracle's"""
    for name, rows in (("T1", 128), ("T3", 384), ("T5_far", 896)):
        got, want = measure_case(name)
        assert got["rho_rows"] == rows == cc.lags_summed(want), name
        table = cc.oracle(cc.case(name)[0], min_corr=-2.0, max_lag=rows - 1)["rho"]          # (never cut: every lag up to rows - 1)
        assert got["rho"].shape == table.shape == (rows, want["rho"].shape[1]), name
        worst = float(np.max(np.abs(got["rho"] - table.astype(np.float64))))
        print("%s: %d lags, max|drho| over the whole table %.2e (tol %.2e)" % (name, rows, worst, cc.tolerances(want)[0]))
        assert worst <= cc.tolerances(want)[0], name


@pytest.mark.parametrize("name", ["T3", "T4_127", "T5", "T5_far", "T6"])
def test_two_runs_give_the_same_bits(name):
    a, _ = measure_case(name)
    b, _ = measure_case(name)
    assert a["rho"].tobytes() == b["rho"].tobytes() and a["per_param"].tobytes() == b["per_param"].tobytes() and np.array_equal(a["cut"], b["cut"])


def test_host_pointer_form_equals_the_device_form():
    from mcevidence_amd import _capi
    parts, _, _ = cc.case("T2")
    a = _capi.chain_corr(parts, 0, 2, 3)
    b = measure_dev(parts)
    assert a["rho"].tobytes() == b["rho"].tobytes() and np.array_equal(a["cut"], b["cut"]) and a["units"] == b["units"]


@pytest.mark.parametrize("name", cc.SINGLE)
def test_a_chain_alone_and_beside_itself(name):
    """rho of [A, A] and of [A, nothing, A] is rho of [A]: every sum and every count doubles, unless a pair spans two parts"""
    parts, kw, want = cc.case(name)
    alone = measure_dev(parts)
    tol_rho, tol_len = cc.tolerances(dict(want, units=2 * want["units"]))
    empty = np.zeros((0, parts[0].shape[1]))
    for table in ([parts[0], parts[0]], [parts[0], empty, parts[0]]):
        got = measure_dev(table)
        assert got["units"] == 2 * want["units"] and got["cap"] == want["cap"] and np.array_equal(got["cut"], want["cut"])
        last = int(want["cut"].max())
        assert np.max(np.abs(got["rho"][:last + 1] - want["rho"][:last + 1].astype(np.float64))) <= tol_rho
        assert np.max(np.abs(got["rho"][:last + 1] - alone["rho"][:last + 1])) <= 2 * tol_rho
        assert np.all(np.abs(got["per_param"] - want["per_param"].astype(np.float64)) <= tol_len)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    d = tmp_path_factory.mktemp("corr_roots")
    out = {}
    for name in ("T2", "T6", "T4") + tuple(cc.STATUS):
        out[name] = str(d / name)
        cc.write_files(out[name], cc.case(name)[0])
    return out


@pytest.mark.parametrize("name", ["T2", "T6"])
def test_resident_route_with_thin_corr(name, roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import chains
    parts, _, want = cc.case(name)
    rc = pkg.ResidentChains.from_files(roots[name], thin_corr=True)
    host = pkg.MCEvidence(roots[name], thin_corr=True, kmax=3, verbose=0)
    tc = rc.thin_corr
    assert tc["factor"] == want["factor"] == host.info["thin_corr"]["factor"] and tc["cut"] == [int(c) for c in want["cut"]]
    assert tc["units"] == ("weight" if name == "T2" else "rows") and tc["cap"] == want["cap"]
    assert np.all(np.abs(np.asarray(tc["per_param"]) - want["per_param"].astype(np.float64)) <= cc.tolerances(want)[1])
    # the same rows and weights as the host route
    w = np.concatenate([p[:, 0] for p in parts])
    keep, new_w = chains.thin_rows(w, float(want["factor"]))
    assert np.array_equal(rc.keep(), keep) and np.array_equal(rc.weights(), np.asarray(new_w, dtype=np.float64))
    assert np.array_equal(rc.to_host(), host.gd.samples)
    lnE, info = rc.evidence(kmax=3, info=True)
    assert info["thin_corr"] == tc and info["route"] == "resident"
    assert np.max(np.abs(lnE - host.evidence())) <= LNE_PARITY
    # bit for bit its own thinlen = factor run
    own = pkg.ResidentChains.from_files(roots[name], thinlen=want["factor"])
    assert np.array_equal(own.keep(), rc.keep()) and np.array_equal(own.evidence(kmax=3), lnE)
    # and through evidence_from_files, and from arrays
    lnE2, info2 = pkg.evidence_from_files(roots[name], thin_corr=True, kmax=3, verbose=0, info=True, require_resident=True)
    assert np.array_equal(lnE2, lnE) and info2["thin_corr"]["factor"] == want["factor"]
    assert np.array_equal(pkg.ResidentChains.from_arrays([np.array(p) for p in parts], thin_corr=True).keep(), keep)
    with pytest.raises(ValueError, match="thin_corr.*thinlen"):
        pkg.ResidentChains.from_files(roots[name], thin_corr=True, thinlen=2)


def test_farm_sends_a_thin_corr_root_to_the_per_root_route(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    outs = pkg.evidence_many_from_files([roots["T2"], roots["T4"]], thin_corr=[True, None], kmax=3, info=True)
    one = pkg.evidence_from_files(roots["T2"], thin_corr=True, kmax=3, verbose=0, info=True)
    assert outs[0][1]["route"] == "resident" and outs[1][1]["route"] == "farm" and "thin_corr" not in outs[1][1]
    assert np.array_equal(outs[0][0], one[0]) and outs[0][1]["thin_corr"] == one[1]["thin_corr"]
    assert farm.LAST_STATS["counts"]["fallback"] == 1 and farm.LAST_STATS["counts"]["farm"] == 1
    plain = pkg.evidence_many_from_files([roots["T4"]], kmax=3)
    assert np.array_equal(plain[0], outs[1][0])


@pytest.mark.parametrize("name", cc.STATUS)
def test_status_cases_raise_the_hosts_words(name, roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import chains
    _, kw, want = cc.case(name)
    got, _ = measure_case(name)
    assert (got["status"], got["column"], got["cap"]) == (want["status"], want["column"], want["cap"])
    words = str(chains.corr_status_error(want["status"], want["column"], want["cap"], cc.MIN_CORR))
    extra = {"corr_max_lag": kw["max_lag"]} if "max_lag" in kw else {}
    with pytest.raises(ValueError) as e:
        pkg.ResidentChains.from_files(roots[name], thin_corr=True, **extra)
    assert str(e.value) == words
    with pytest.raises(ValueError) as e:
        pkg.evidence_from_files(roots[name], thin_corr=True, verbose=0, **extra)
    assert str(e.value) == words
    with pytest.raises(ValueError) as e:
        pkg.MCEvidence(roots[name], thin_corr=True, verbose=0, **extra)
    assert str(e.value) == words
