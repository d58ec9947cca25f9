"""thin_corr on the CPU: the rule the host check and the device kernels share (mcevidence_amd/csrc/chain_corr.hpp: its serial driver,
built with -fsanitize=address,undefined as a stand-alone program) and its NumPy form ``chains.correlation_length`` against the
longdouble oracle of tests/corr_cases.py; the unit -> row map against ``np.repeat``; the status cases; ``MCEvidence(files,
thin_corr=True)`` against its own ``thinlen=factor`` run; the keyword in ``resident.plan`` and on the command line; the new C symbols."""
import os
import struct
import subprocess

import numpy as np
import pytest

import corr_cases as cc
from helpers import REPO, OracleBackend
from prep_cases import LENGTHS, int_weights

from mcevidence_amd import _capi, chains, cli, resident
from mcevidence_amd.evidence import MCEvidence


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_corr") / "chain_corr_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "chain_corr_check.cpp"), "-o", exe])
    return exe


def run_corr(exe, tmp_path, jobs):
    """jobs: [(parts, ndim, min_corr, max_lag)] -> the serial driver's results as dicts"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for parts, ndim, min_corr, max_lag in jobs:
            f.write(struct.pack("<qqqqqdq", len(parts), parts[0].shape[1], 0, 2, ndim, min_corr, max_lag))
            for p in parts:
                f.write(struct.pack("<q", p.shape[0]))
                f.write(np.ascontiguousarray(p, dtype="<f8").tobytes())
    out = subprocess.run([exe, "corr", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(jobs)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = open(fout, "rb").read()
    got, at = [], 0
    for parts, ndim, _, _ in jobs:
        rule, = struct.unpack_from("<q", raw, at)
        at += 8
        if rule < 0:
            got.append(dict(rule=rule))
            continue
        status, column, units, max_units, cap, rows = struct.unpack_from("<6q", raw, at)
        at += 48
        r = dict(rule=rule, status=status, column=column, units=units, max_units=max_units, cap=cap, rho_rows=rows)
        r["L"], = struct.unpack_from("<d", raw, at)
        at += 8
        if status in (0, 1):
            r["per_param"] = np.frombuffer(raw, dtype="<f8", count=ndim, offset=at)
            at += 8 * ndim
            r["cut"] = np.frombuffer(raw, dtype="<i8", count=ndim, offset=at)
            at += 8 * ndim
            r["rho"] = np.frombuffer(raw, dtype="<f8", count=rows * ndim, offset=at).reshape(rows, ndim)
            at += 8 * rows * ndim
        got.append(r)
    assert at == len(raw)
    return got


def measure_numpy(name):
    parts, kw, want = cc.case(name)
    return chains.correlation_length(parts, 0, 2, kw.get("ndim"), cc.MIN_CORR, kw.get("max_lag", cc.MAX_LAG)), want


@pytest.mark.parametrize("name", cc.NUMERIC)
def test_correlation_length_equals_the_oracle(name):
    got, want = measure_numpy(name)
    cc.check(name, got, want)
    assert got["rho_rows"] == int(want["cut"].max()) + 1          # it stops at the last cut


def test_serial_driver_equals_the_oracle(checker, tmp_path):
    jobs, wants = [], []
    for name in cc.NUMERIC:
        parts, kw, want = cc.case(name)
        jobs.append((parts, want["rho"].shape[1], cc.MIN_CORR, kw.get("max_lag", cc.MAX_LAG)))
        wants.append(want)
    for name, got, want in zip(cc.NUMERIC, run_corr(checker, tmp_path, jobs), wants):
        cc.check(name, got, want)
        assert got["max_units"] == want["max_units"] and got["rho_rows"] == int(want["cut"].max()) + 1
        assert abs(got["L"] - float(want["length"])) <= float(cc.tolerances(want)[1].max())


@pytest.mark.parametrize("name", cc.STATUS)
def test_status_cases(name, checker, tmp_path):
    got, want = measure_numpy(name)
    parts, kw, _ = cc.case(name)
    ser, = run_corr(checker, tmp_path, [(parts, parts[0].shape[1] - 2, cc.MIN_CORR, kw.get("max_lag", cc.MAX_LAG))])
    for g in (got, ser):
        assert (g["status"], g["column"], g["cap"]) == (want["status"], want["column"], want["cap"])
    err = chains.corr_status_error(want["status"], want["column"], want["cap"], cc.MIN_CORR)
    assert isinstance(err, ValueError) and "column %d" % want["column"] in str(err)
    if want["status"] == 1:
        assert "cap=%d" % want["cap"] in str(err) and "corr_max_lag" in str(err) and "burn" in str(err)
    if want["status"] == 2:
        assert "ndim" in str(err)
    with pytest.raises(ValueError, match="column %d" % want["column"]):
        chains.corr_info(got, 1.0)


def test_rule_choice_and_declines(checker, tmp_path):
    parts, _, _ = cc.case("T2")
    near = [p.copy() for p in parts]
    near[1][3, 0] += 1e-4 + 4e-7                      # fractional sum within 1e-6 of the threshold
    neg = [p.copy() for p in parts]
    neg[2][7, 0] = -1.0
    rules = [r["rule"] for r in run_corr(checker, tmp_path, [(parts, 3, 0.05, 64), (near, 3, 0.05, 64), (neg, 3, 0.05, 64), (cc.case("T6")[0], 2, 0.05, 64)])]
    assert rules == [1, -2, -1, 2]
    with pytest.raises(ValueError, match="weight"):
        chains.correlation_length(neg)


def test_unit_row_map_equals_repeat(checker, tmp_path):
    """the row of every unit, for a part at the head of the prefix sums and for one behind another part"""
    ws = [int_weights(n, hi, seed=11 * hi + n) for n in LENGTHS for hi in (1, 3, 50)]
    ws.append(np.asarray([0.0, 0.0, 5000.0, 0.0, 1.0, 0.0]))
    fin, fout = tmp_path / "map.bin", tmp_path / "map.out"
    with open(fin, "wb") as f:
        for w in ws:
            f.write(struct.pack("<q", len(w)))
            f.write(np.ascontiguousarray(w, dtype="<f8").tobytes())
    out = subprocess.run([checker, "map", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(ws)), out.stdout[-2000:] + out.stderr[-2000:]
    raw, at = open(fout, "rb").read(), 0
    for w in ws:
        units, = struct.unpack_from("<q", raw, at)
        at += 8
        want = np.repeat(np.arange(len(w)), w.astype(np.int64))
        assert units == len(want)
        for _ in range(2):
            assert np.array_equal(np.frombuffer(raw, dtype="<i8", count=units, offset=at), want)
            at += 8 * units
    assert at == len(raw)


def test_factor_rule(checker):
    for scale, length in ((1.0, 2.53), (1.0, 0.2), (2.0, 18.25), (0.5, 18.25), (1.0, 171.0), (1.0, 1.0)):
        got = int(subprocess.check_output([checker, "factor", repr(scale), repr(length)]).decode())
        assert got == chains.corr_factor(scale, length) == max(1, int(np.ceil(scale * length)))


@pytest.fixture(scope="module")
def t2_root(tmp_path_factory):
    parts, _, want = cc.case("T2")
    root = str(tmp_path_factory.mktemp("t2") / "t2")
    cc.write_files(root, parts)
    return root, want


def test_mcevidence_thin_corr_equals_its_thinlen_run(t2_root):
    root, want = t2_root
    a = MCEvidence(root, thin_corr=True, kmax=3, verbose=0, backend=OracleBackend())
    b = MCEvidence(root, thinlen=want["factor"], kmax=3, verbose=0, backend=OracleBackend())
    assert a.gd.samples.shape == b.gd.samples.shape and a.gd.samples.shape[0] < want["units"] // want["factor"] + 2
    assert np.array_equal(a.gd.samples, b.gd.samples)
    lnE_a, info = a.evidence(info=True)
    assert np.array_equal(lnE_a, b.evidence())
    tc = info["thin_corr"]
    tol_rho, tol_len = cc.tolerances(want)
    assert tc["factor"] == want["factor"] and tc["cut"] == [int(c) for c in want["cut"]] and tc["units"] == "weight" and tc["cap"] == want["cap"]
    assert np.all(np.abs(np.asarray(tc["per_param"]) - want["per_param"].astype(np.float64)) <= tol_len)
    assert abs(tc["length"] - float(want["length"])) <= tol_len.max()
    assert "thin_corr" not in b.evidence(info=True)[1]
    # ndim: the columns the estimator uses are the columns measured; a scale multiplies the length
    one = MCEvidence(root, thin_corr=2.0, ndim=1, kmax=3, verbose=0, backend=OracleBackend()).info["thin_corr"]
    want1 = cc.oracle(cc.case("T2")[0], ndim=1, scale=2.0)
    assert one["factor"] == want1["factor"] and one["cut"] == [int(want1["cut"][0])]
    # a list of file names is thinned like the root; arrays ignore the keyword, as they ignore thinlen
    files = sorted(p for p in (root + "_%d.txt" % i for i in (1, 2, 3)))
    assert np.array_equal(MCEvidence(files, thin_corr=True, kmax=3, verbose=0, backend=OracleBackend()).gd.samples, a.gd.samples)
    arr = MCEvidence(list(cc.case("T2")[0]), thin_corr=True, kmax=3, verbose=0, backend=OracleBackend())
    assert arr.gd.samples.shape[0] == sum(len(p) for p in cc.case("T2")[0]) and "thin_corr" not in arr.info


def test_thin_corr_with_thinlen_raises_and_negative_thinlen_still_does(t2_root):
    root, _ = t2_root
    with pytest.raises(ValueError, match="thin_corr.*thinlen"):
        MCEvidence(root, thin_corr=True, thinlen=3, verbose=0, backend=OracleBackend())
    with pytest.raises(ValueError, match="thin_corr.*thinlen"):
        resident.plan(thin_corr=1.5, thinlen=2)
    with pytest.raises(ValueError, match="thin_corr"):
        MCEvidence(root, thin_corr=-1.0, verbose=0, backend=OracleBackend())
    with pytest.raises(ValueError, match="negative thinlen"):
        MCEvidence(root, thinlen=-2, verbose=0, backend=OracleBackend())
    assert resident.plan(thinlen=-2) == resident.REASONS["negative_thinlen"]
    for off in (None, False):
        m = MCEvidence(root, thin_corr=off, thinlen=3, kmax=3, verbose=0, backend=OracleBackend())
        assert "thin_corr" not in m.info


def test_status_is_a_value_error_on_the_host_route(tmp_path):
    for name in cc.STATUS:
        parts, kw, want = cc.case(name)
        root = str(tmp_path / name)
        cc.write_files(root, parts)
        extra = {"corr_max_lag": kw["max_lag"]} if "max_lag" in kw else {}
        with pytest.raises(ValueError) as e:
            MCEvidence(root, thin_corr=True, verbose=0, backend=OracleBackend(), **extra)
        assert str(e.value) == str(chains.corr_status_error(want["status"], want["column"], want["cap"], cc.MIN_CORR))


def test_plan_and_cli_carry_the_keyword(monkeypatch):
    assert resident.plan(thin_corr=True) == "resident" and resident.plan(thin_corr=2.5, covtype="single") == "resident"
    assert resident.plan(thin_corr=True, isfunc=lambda s: 0.0) == resident.REASONS["isfunc"]
    assert "thin_corr" in resident.REASONS and len(set(resident.REASONS.values())) == len(resident.REASONS)
    parse = cli.build_parser().parse_args
    assert parse(["root"]).thin_corr is None
    assert parse(["root", "--thin-corr"]).thin_corr is True
    assert parse(["root", "--thin-corr", "2.5"]).thin_corr == 2.5
    seen = {}

    class Spy(object):
        def __init__(self, root, **kw):
            seen.update(kw, root=root)

        def evidence(self):
            return np.zeros(1)
    monkeypatch.setattr(cli, "MCEvidence", Spy)
    monkeypatch.setattr(cli.prior, "get_prior_volume", lambda args, cosmo=True: 1.0)
    cli.main(["root", "--thin-corr", "2"])
    assert seen["thin_corr"] == 2.0 and seen["thinlen"] == 0
    seen.clear()
    cli.main(["root"])
    assert "thin_corr" not in seen


def test_new_symbols_validate_without_a_device():
    lib = _capi.load()
    for name in ("mce_chain_corr_workspace_bytes", "mce_chain_corr_dev", "mce_chain_corr_f64"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert lib.mce_abi_version() == 3
    assert _capi.chain_corr_workspace_bytes(1000, 2, 3, 1024) >= _capi.chain_select_workspace_bytes(1000, 2) + 1025 * 3 * 16
    for bad in ((-1, 2, 3, 1024), (1000, 0, 3, 1024), (1000, 2, 0, 1024), (1000, 2, 128, 1024), (1000, 2, 3, 0)):
        assert _capi.chain_corr_workspace_bytes(*bad) == 0
    P = 0x1000          # never dereferenced: every call below fails in its argument checks
    ok = dict(parts=[(P, 100)], ncols=5, iw=0, itheta=2, ndim=3, min_corr=0.05, max_lag=64, ws=P, ws_bytes=1 << 30)
    for change in (dict(ws=0), dict(parts=[(0, 100)]), dict(parts=[(P, -1)]), dict(parts=[(P, 0)]), dict(ndim=0), dict(ndim=4), dict(ndim=128, ncols=200),
                   dict(iw=5), dict(itheta=5), dict(min_corr=1.0), dict(min_corr=-0.1), dict(min_corr=float("nan")), dict(max_lag=0), dict(max_lag=1 << 20),
                   dict(ws_bytes=64)):
        with pytest.raises(ValueError):
            _capi.chain_corr_dev(**dict(ok, **change))
    with pytest.raises(ValueError):
        _capi.chain_corr([np.zeros((10, 5))], 0, 2, 4)
    with pytest.raises(ValueError):
        _capi.chain_corr([np.zeros((10, 5)), np.zeros((10, 4))], 0, 2, 2)
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_corr_dev(**ok)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_corr([np.ones((10, 5))], 0, 2, 3)
