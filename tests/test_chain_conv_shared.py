"""converge on the CPU: the rule the host check and the device kernels share (mcevidence_amd/csrc/chain_conv.hpp: its serial driver,
built with -fsanitize=address,undefined as a stand-alone program) and its NumPy form ``chains.gelman_rubin`` against the extended
precision model of tests/conv_cases.py, within the bound derived in docs/design/chain_conv.md; the status cases and their
precedence; the invariances; ``MCEvidence(..., converge=...)`` on files and arrays, under burn-in and thinning; the warning; the
keyword in ``resident.plan`` and on the command line; the new C symbols."""
import logging
import os
import struct
import subprocess

import numpy as np
import pytest

import conv_cases as cv
from corr_cases import write_files
from helpers import REPO, OracleBackend

from mcevidence_amd import _capi, chains, cli, resident
from mcevidence_amd.evidence import MCEvidence


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_conv") / "chain_conv_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "chain_conv_check.cpp"), "-o", exe])
    return exe


def run_conv(exe, tmp_path, jobs):
    """jobs: [(segments, ndim)] -> the serial driver's results as dicts"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for segs, ndim in jobs:
            f.write(struct.pack("<qqqqq", len(segs), segs[0].shape[1], 0, 2, ndim))
            for s in segs:
                f.write(struct.pack("<q", s.shape[0]))
                f.write(np.ascontiguousarray(s, dtype="<f8").tobytes())
    out = subprocess.run([exe, "conv", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(jobs)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = open(fout, "rb").read()
    got, at = [], 0
    for segs, ndim in jobs:
        status, column, used, skipped = struct.unpack_from("<4q", raw, at)
        at += 32
        r = dict(status=status, column=column, used=used, skipped=skipped)
        r["r_minus_1"], = struct.unpack_from("<d", raw, at)
        at += 8
        if status in (0, 4):
            r["per_param"] = np.frombuffer(raw, dtype="<f8", count=ndim, offset=at)
            at += 8 * ndim
        got.append(r)
    assert at == len(raw)
    return got


@pytest.mark.parametrize("by", cv.BY)
@pytest.mark.parametrize("name", cv.NUMERIC)
def test_gelman_rubin_equals_the_model(name, by):
    got = chains.gelman_rubin(list(cv.parts(name)), by=by)
    cv.check(got, cv.model(name, by), "%s/%s" % (name, by))
    assert got["by"] == by and got["status"] == 0 and got["threshold"] is None and got["converged"] is None
    assert got["worst_param"] == int(np.argmax(got["per_param"])) and got["rows"] == sum(len(p) for p in cv.parts(name))
    assert got["r_minus_1"] >= max(got["per_param"]) * (1.0 - 1e-12)          # the worst direction is at least as bad as the worst axis


def test_serial_driver_equals_the_model(checker, tmp_path):
    labels = [(name, by) for name in cv.NUMERIC for by in cv.BY]
    jobs = [(cv.segments(cv.parts(name), by), cv.parts(name)[0].shape[1] - 2) for name, by in labels]
    for (name, by), got in zip(labels, run_conv(checker, tmp_path, jobs)):
        want = cv.model(name, by)
        assert got["status"] == 0 and got["skipped"] == want["skipped"]
        cv.check(got, want, "serial %s/%s" % (name, by))


def test_the_cases_are_what_they_claim():
    assert cv.model("B", "chains")["skipped"] == 1 and cv.model("B", "halves")["skipped"] == 3          # the empty chain; the halves of 1 and 0 rows
    assert cv.model("I", "chains")["skipped"] == 1 and cv.model("I", "halves")["skipped"] == 2          # the chain whose weights are all 0
    assert cv.model("F", "halves")["used"] == chains.CONV_MAX_SEGMENTS == _capi.CONV_MAX_SEGMENTS
    d = cv.model("D", "chains")
    assert 50 < d["kappa"] < 150 and d["r_minus_1"] > 5 * d["per_param"].max()          # per_param alone would miss the worst direction
    assert cv.model("G", "chains")["r_minus_1"] > 0.2                                   # unconverged by any threshold in use
    assert chains.gelman_rubin(list(cv.parts("A")))["by"] == "chains" and chains.gelman_rubin([cv.parts("A")[0]])["by"] == "halves"


@pytest.mark.parametrize("name", cv.STATUS)
def test_status_cases(name, checker, tmp_path):
    parts = list(cv.parts(name))
    status, column = cv.STATUS_WANT[name]
    ser, = run_conv(checker, tmp_path, [(parts, parts[0].shape[1] - 2)])
    assert ser["status"] == status and (column is None or ser["column"] == column)
    if status == 4:
        got = chains.gelman_rubin(parts)
        assert got["status"] == 4 and np.isnan(got["r_minus_1"]) and np.all(np.isfinite(got["per_param"])) and len(got["per_param"]) == 6
        assert np.allclose(got["per_param"], ser["per_param"], rtol=1e-12) and np.isnan(ser["r_minus_1"])
        assert chains.gelman_rubin(parts, threshold=0.1)["converged"] is False
        return
    with pytest.raises(ValueError) as e:
        chains.gelman_rubin(parts)
    assert str(e.value) == str(chains.conv_status_error(status, column))
    if column >= 0:
        assert "column %d" % column in str(e.value)
    if status == 2:
        assert "ndim" in str(e.value)


def test_segment_rules_and_their_errors():
    assert chains.conv_segments([10, 7], "auto") == ("chains", [(0, 0, 10), (1, 0, 7)])
    assert chains.conv_segments([10, 0], "auto") == ("halves", [(0, 0, 5), (0, 5, 5), (1, 0, 0), (1, 0, 0)])
    assert chains.conv_segments([7], "halves") == ("halves", [(0, 0, 3), (0, 3, 4)])
    with pytest.raises(ValueError, match='converge_by="halves"'):
        chains.conv_segments([10, 0], "chains")
    with pytest.raises(ValueError, match="more rows"):
        chains.conv_segments([1], "auto")
    with pytest.raises(ValueError, match="at most 128"):
        chains.conv_segments([10] * 65, "halves")
    with pytest.raises(ValueError, match="at most 128"):
        chains.conv_segments([10] * 129, "chains")
    with pytest.raises(ValueError, match="converge_by"):
        chains.conv_segments([10, 10], "quarters")
    assert chains.converge_spec(None) is None and chains.converge_spec(False) is None
    assert chains.converge_spec(True) == (None, "auto") and chains.converge_spec(0.01, "halves") == (0.01, "halves")
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="converge"):
            chains.converge_spec(bad)
    with pytest.raises(ValueError, match="127"):
        chains.gelman_rubin([np.ones((10, 130)), np.ones((10, 130))])


def test_invariances():
    parts = list(cv.parts("D"))
    want = cv.model("D", "chains")
    base = chains.gelman_rubin(parts, by="chains")
    scaled = [p.copy() for p in parts]
    for p in scaled:
        p[:, 2 + 3] *= 2.0 ** 20
        p[:, 2 + 5] *= 2.0 ** -33
    perm = [parts[k] for k in (5, 2, 7, 0, 1, 6, 3, 4)]
    for other in (chains.gelman_rubin(scaled, by="chains"), chains.gelman_rubin(perm, by="chains")):
        assert abs(other["r_minus_1"] - base["r_minus_1"]) <= 2 * want["bound_r"]
        assert np.all(np.abs(np.asarray(other["per_param"]) - base["per_param"]) <= 2 * want["bound_per"])
    a, b = cv.parts("A")[0], cv.parts("A")[1]
    doubled = [a, a, b, b]
    cv.check(chains.gelman_rubin(doubled, by="chains"), cv.model_segments(doubled, 3), "[A, A, B, B]")


@pytest.fixture(scope="module")
def g_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("g") / "g")
    write_files(root, cv.parts("G"))
    return root


def test_mcevidence_measures_the_burned_unthinned_chains(g_root):
    parts = list(cv.parts("G"))
    want = cv.model("G", "chains")
    m = MCEvidence(g_root, converge=True, kmax=3, verbose=0, backend=OracleBackend())
    lnE, info = m.evidence(info=True)
    cv.check(info["converge"], want, "files")
    assert info["converge"]["converged"] is None and info["converge"]["rows"] == 8000
    # converge=None: info and the returned bits exactly as they are without the keyword
    for off in (None, False):
        plain = MCEvidence(g_root, converge=off, kmax=3, verbose=0, backend=OracleBackend())
        lnE0, info0 = plain.evidence(info=True)
        assert np.array_equal(lnE, lnE0) and "converge" not in info0
        assert {k: v for k, v in info.items() if k != "converge"} == info0
    bare = MCEvidence(g_root, kmax=3, verbose=0, backend=OracleBackend()).evidence(info=True)
    assert np.array_equal(bare[0], lnE) and bare[1] == info0
    # burn-in comes first; thinning of either kind does not change what is measured
    burned = [p[int(0.25 * len(p)):] for p in parts]
    wantb = cv.model_segments(burned, 6)
    for extra in (dict(), dict(thinlen=3), dict(thin_corr=True)):
        mb = MCEvidence(g_root, converge=True, burnlen=0.25, kmax=3, verbose=0, backend=OracleBackend(), **extra)
        cv.check(mb.info["converge"], wantb, "burned %r" % (extra,))
        assert mb.info["converge"] == MCEvidence(g_root, converge=True, burnlen=0.25, kmax=3, verbose=0, backend=OracleBackend()).info["converge"]
        assert mb.info["converge"]["rows"] == 6000
    # ndim: the columns the estimator uses are the columns measured; halves on request
    two = MCEvidence(g_root, converge=True, converge_by="halves", ndim=2, kmax=3, verbose=0, backend=OracleBackend()).info["converge"]
    cv.check(two, cv.model_segments(cv.segments(parts, "halves"), 2), "ndim 2 by halves")
    assert two["by"] == "halves" and len(two["per_param"]) == 2
    # a list of file names, a list / tuple / dict of arrays, a single array by halves
    files = [g_root + "_%d.txt" % i for i in (1, 2, 3, 4)]
    for method in (files, parts, tuple(parts), {"a%d" % i: p for i, p in enumerate(parts)}):
        cv.check(MCEvidence(method, converge=True, kmax=3, verbose=0, backend=OracleBackend()).info["converge"], want, type(method).__name__)
    one = MCEvidence([parts[0]], converge=True, kmax=3, verbose=0, backend=OracleBackend()).info["converge"]
    cv.check(one, cv.model_segments(cv.segments(parts[:1], "halves"), 6), "one array")
    assert one["by"] == "halves"


def test_threshold_warns_and_raises_nothing(g_root, caplog):
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        m = MCEvidence(g_root, converge=0.01, kmax=3, verbose=0, backend=OracleBackend())
        lnE = m.evidence()
    c = m.info["converge"]
    assert c["converged"] is False and c["threshold"] == 0.01 and c["r_minus_1"] > 0.2
    text = " ".join(r.getMessage() for r in caplog.records if r.levelno == logging.WARNING)
    assert "R-1 = %.4g" % c["r_minus_1"] in text and "0.01" in text and "worst parameter %d" % c["worst_param"] in text
    assert np.array_equal(lnE, MCEvidence(g_root, kmax=3, verbose=0, backend=OracleBackend()).evidence())
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        ok = MCEvidence(g_root, converge=10.0, kmax=3, verbose=0, backend=OracleBackend()).info["converge"]
    assert ok["converged"] is True and not [r for r in caplog.records if "converge" in r.getMessage()]
    with pytest.raises(ValueError, match="converge"):
        MCEvidence(g_root, converge=-1, verbose=0, backend=OracleBackend())
    with pytest.raises(ValueError, match="converge_by"):
        MCEvidence(g_root, converge=True, converge_by="thirds", verbose=0, backend=OracleBackend())


def test_status_is_a_value_error_on_the_host_route(tmp_path, caplog):
    for name in cv.STATUS:
        root = str(tmp_path / name)
        write_files(root, cv.parts(name))
        status, column = cv.STATUS_WANT[name]
        if status == 4:
            with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
                c = MCEvidence(root, converge=0.05, kmax=2, verbose=0, backend=OracleBackend()).info["converge"]
            assert c["status"] == 4 and np.isnan(c["r_minus_1"]) and c["converged"] is False
            assert any("not positive definite" in r.getMessage() for r in caplog.records)
            continue
        with pytest.raises(ValueError) as e:
            MCEvidence(root, converge=True, verbose=0, backend=OracleBackend())
        assert str(e.value) == str(chains.conv_status_error(status, column))


def test_plan_and_cli_carry_the_keyword(monkeypatch, capsys):
    assert resident.plan(converge=True) == "resident" and resident.plan(converge=0.01, converge_by="halves", covtype="single") == "resident"
    assert resident.plan(converge=True, isfunc=lambda s: 0.0) == resident.REASONS["isfunc"]          # it declines nothing by itself
    assert resident.plan(converge=True, thinlen=3) == resident.plan(thinlen=3) == "resident"
    with pytest.raises(ValueError, match="converge"):
        resident.plan(converge=-0.5)
    with pytest.raises(ValueError, match="converge_by"):
        resident.plan(converge=True, converge_by="x")
    parse = cli.build_parser().parse_args
    assert parse(["root"]).converge is None and parse(["root"]).converge_by == "auto"
    assert parse(["root", "--converge"]).converge is True
    assert parse(["root", "--converge", "0.02", "--converge-by", "halves"]).converge == 0.02
    assert parse(["root", "--converge=0.02", "--converge-by", "halves"]).converge_by == "halves"
    with pytest.raises(SystemExit):
        parse(["root", "--converge-by", "thirds"])
    seen = {}

    class Spy(object):
        def __init__(self, root, **kw):
            seen.update(kw, root=root)
            if "converge" in kw:
                self.info = {"converge": chains.gelman_rubin(list(cv.parts("A")), threshold=None if kw["converge"] is True else kw["converge"])}

        def evidence(self):
            print("   ln(B) lines")
            return np.zeros(1)
    monkeypatch.setattr(cli, "MCEvidence", Spy)
    monkeypatch.setattr(cli.prior, "get_prior_volume", lambda args, cosmo=True: 1.0)
    cli.main(["root", "--converge", "0.01", "--converge-by", "chains"])
    assert seen["converge"] == 0.01 and seen["converge_by"] == "chains"
    out = capsys.readouterr().out
    want = cv.model("A", "chains")
    assert "R-1 = %.6g (worst parameter %d: " % (want["r_minus_1"], int(np.argmax(want["per_param"]))) in out and "NOT converged" in out
    assert out.index("R-1 = ") < out.index("ln(B) lines")
    seen.clear()
    cli.main(["root"])
    assert "converge" not in seen and "converge_by" not in seen and "R-1" not in capsys.readouterr().out


def test_new_symbols_validate_without_a_device():
    lib = _capi.load()
    for name in ("mce_chain_conv_workspace_bytes", "mce_chain_conv_dev", "mce_chain_conv_f64"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert lib.mce_abi_version() == 3
    assert _capi.chain_conv_workspace_bytes(100000, 8, 2, 27) >= (100000 // 1024) * 378 * 8
    for bad in ((-1, 2, 1, 3), (1000, 0, 1, 3), (1000, 2, 0, 3), (1000, 2, 1, 0), (1000, 2, 1, 128)):
        assert _capi.chain_conv_workspace_bytes(*bad) == 0
    P = 0x1000          # never dereferenced: every call below fails in its argument checks
    ok = dict(segs=[(P, 100), (P, 100)], seg_sys=[0, 0], nsys=1, ncols=5, iw=0, itheta=2, ndim=3, ws=P, ws_bytes=1 << 30)
    changes = (dict(ws=0), dict(segs=[(0, 100), (P, 100)]), dict(segs=[(P, -1), (P, 100)]), dict(ndim=0), dict(ndim=4), dict(ndim=128, ncols=200), dict(iw=5),
               dict(itheta=5), dict(ws_bytes=64), dict(seg_sys=[0, 1]), dict(seg_sys=[1, 0], nsys=2), dict(seg_sys=[0, -1]), dict(nsys=0),
               dict(segs=[(P, 100), (P, 0)]),                                   # one usable segment
               dict(segs=[(P, 100)] * 4, seg_sys=[0, 0, 0, 1], nsys=2),       # the second system has one
               dict(segs=[(P, 10)] * 129, seg_sys=[0] * 129))                  # 129 segments
    for change in changes:
        with pytest.raises(ValueError):
            _capi.chain_conv_dev(**dict(ok, **change))
    with pytest.raises(ValueError, match="more than 128 segments"):
        _capi.chain_conv_dev(**dict(ok, segs=[(P, 10)] * 129, seg_sys=[0] * 129))
    with pytest.raises(ValueError, match="ndim=128"):
        _capi.chain_conv_dev(**dict(ok, ndim=128, ncols=200))
    with pytest.raises(ValueError, match="halves"):
        _capi.chain_conv_dev(**dict(ok, segs=[(P, 100), (P, 0)]))
    with pytest.raises(ValueError):
        _capi.chain_conv([np.zeros((10, 5)), np.zeros((10, 4))], [0, 0], 1, 0, 2, 2)
    with pytest.raises(ValueError):
        _capi.chain_conv([np.zeros((10, 5))], [0], 1, 0, 2, 3)
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_conv_dev(**ok)
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.chain_conv([np.ones((10, 5)), np.ones((10, 5))], [0, 0], 1, 0, 2, 3)
