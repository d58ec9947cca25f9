"""information on the CPU: the rule the host check and the device kernels share (mcevidence_amd/csrc/like_moments.hpp: its serial
driver, built with -fsanitize=address,undefined as a stand-alone program) and its NumPy form ``information.moments`` against the exact
rational model of tests/moments_cases.py, within the bound derived in docs/design/information.md; ``MCEvidence(..., information=True)``
for the auto and the cross form with the D_KL identity; the jackknife part; the refusals; the status cases; the untouched default; the
command line; a statistical check on Gaussian samples; the new C symbols."""
import logging
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import moments_cases as mc
from helpers import REPO, OracleBackend, OracleFeedBackend
from mcevidence_amd import information as inf_mod
from mcevidence_amd.evidence import MCEvidence, evidence_many
from mcevidence_amd.synth import gaussian_chain


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("like_moments") / "like_moments_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "like_moments_check.cpp"), "-o", exe])
    return exe


def run_native(exe, tmp_path, systems):
    """[(a, f)] through the sanitized program -> one dict per system"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        for a, f in systems:
            fh.write(struct.pack("<q", len(a)))
            fh.write(np.ascontiguousarray(f, dtype="<f8").tobytes())
            fh.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    out = subprocess.run([exe, "moments", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(systems)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = np.frombuffer(open(fout, "rb").read(), dtype="<f8").reshape(len(systems), 6)
    return [inf_mod.from_block(b) for b in raw]


def test_serial_driver_and_numpy_form_equal_the_exact_model(checker, tmp_path):
    native = run_native(checker, tmp_path, [(c.a, c.f) for c in mc.CASES])
    for c, got in zip(mc.CASES, native):
        mc.check(c, got, "native")
        mc.check(c, inf_mod.moments(c.a, c.f), "numpy ")


def test_status_cases_of_both_forms(checker, tmp_path, caplog):
    cases = mc.status_cases()
    native = run_native(checker, tmp_path, [(a, f) for _, a, f, _ in cases])
    for (name, a, f, status), nat in zip(cases, native):
        for got in (nat, inf_mod.moments(a, f)):
            assert got["status"] == status, (name, got)
            assert all(math.isnan(got[k]) for k in ("W", "c", "v", "A2")), (name, got)
        assert nat["rows"] == inf_mod.moments(a, f)["rows"] == int(np.count_nonzero(a != 0)), name
    # the dict: every value NaN, the status kept, one WARNING in the route-independent words, nothing raised
    for status in (3, 5):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            d = inf_mod.build(dict(W=float("nan"), c=float("nan"), v=float("nan"), A2=float("nan"), rows=7, status=status), -3.0, np.array([1.0, 2.0]))
        warned = [r for r in caplog.records if r.levelno == logging.WARNING]
        assert len(warned) == 1 and "information: status %d" % status in warned[0].getMessage() and inf_mod.STATUS_WORDS[status] in warned[0].getMessage()
        assert d["status"] == status and d["rows"] == 7 and np.isnan(d["D_KL"]).all()
        assert all(math.isnan(d[k]) for k in ("mean_logL", "var_logL", "bmd", "ess", "sum_w"))


def _inputs(m, pos_lnp=False):
    """(a, f, logLmax) of the rule for an MCEvidence object, formed apart from the package's code path"""
    part = m.gd.data["s1"]
    logL = np.asarray(part.loglikes if pos_lnp else -part.loglikes, dtype=np.float64)
    return np.asarray(part.adjusted_weights, dtype=np.float64), logL - logL.max(), float(logL.max())


def _check_dict(d, a, f, logLmax, lnE, what):
    ex = mc.exact(a, f)
    b = mc.bounds(ex)
    err = {"mean_logL": abs(d["mean_logL"] - (logLmax + ex["c"])) / (b["c"] + mc.EPS * abs(logLmax + ex["c"])), "var_logL": abs(d["var_logL"] - ex["v"]) / b["v"],
           "bmd": abs(d["bmd"] - 2 * ex["v"]) / (2 * b["v"]), "ess": abs(d["ess"] - ex["ess"]) / b["ess"], "sum_w": abs(d["sum_w"] - ex["W"]) / max(b["W"], 5e-324)}
    print("%s n=%d error/bound: %s" % (what, ex["rows"], "  ".join("%s %.3g" % kv for kv in err.items())))
    assert all(v <= 1.0 for v in err.values()), (what, err)
    assert d["rows"] == ex["rows"] and d["status"] == 0
    # D_KL is an identity between this result's mean_logL and this result's ln E
    c = d["mean_logL"] - logLmax
    assert d["D_KL"].shape == np.shape(lnE)
    assert np.all(np.abs(d["D_KL"] - (d["mean_logL"] - lnE)) <= 4 * mc.EPS * (abs(logLmax) + abs(c) + np.abs(lnE)))


def test_mcevidence_auto_and_cross_forms():
    ch = gaussian_chain(seed=3, n=1500, d=4, weights="int")
    # auto and cross, through the host loop and through the device-feeder hook of a backend that offers it
    for split, backend in ((False, OracleBackend), (True, OracleBackend), (False, OracleFeedBackend), (True, OracleFeedBackend)):
        np.random.seed(5)
        m = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend(), information=True)
        lnE, info = m.evidence(info=True)
        d = info["information"]
        assert set(d) == {"mean_logL", "var_logL", "bmd", "ess", "D_KL", "rows", "sum_w", "status"} and d["D_KL"].shape == (3,)
        a, f, logLmax = _inputs(m)
        assert len(a) == (750 if split else 1500)
        _check_dict(d, a, f, logLmax, lnE, "split=%s %s" % (split, backend.__name__))
        np.random.seed(5)
        plain = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend()).evidence()
        assert np.array_equal(lnE, plain)
    # pos_lnp: the column is +ln L
    pos = ch.copy()
    pos[:, 1] = -pos[:, 1]
    m = MCEvidence([pos], kmax=3, verbose=0, backend=OracleBackend(), information=True)
    lnE, info = m.evidence(info=True, pos_lnp=True)
    _check_dict(info["information"], *_inputs(m, pos_lnp=True), lnE, "pos_lnp")
    # evidence_many fills it too
    ms = [MCEvidence([gaussian_chain(seed=s, n=400, d=3)], kmax=3, verbose=0, backend=OracleBackend(), information=True) for s in (1, 2)]
    for m, (lnE, info) in zip(ms, evidence_many(ms, info=True)):
        _check_dict(info["information"], *_inputs(m), lnE, "evidence_many")


def test_without_the_keyword_nothing_changes():
    ch = gaussian_chain(seed=8, n=900, d=3, weights="int")
    a, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence(info=True)
    assert "information" not in info
    for off in (None, False):
        b, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), information=off).evidence(info=True)
        assert "information" not in info and np.array_equal(a, b)
    c, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), information=True).evidence(info=True)
    assert np.array_equal(a, c) and "information" in info


@pytest.mark.parametrize("by", ["blocks", "chains"])
def test_jackknife_part(by):
    from mcevidence_amd.jackknife import group_ids, summarise
    chains = [gaussian_chain(seed=20 + i, n=500, d=3, weights="int") for i in range(4)]
    G = 4 if by == "chains" else 6
    m = MCEvidence(chains, kmax=3, verbose=0, backend=OracleBackend(), information=True, jackknife={"groups": G, "by": by})
    lnE, info = m.evidence(info=True)
    d, jk = info["information"], info["jackknife"]
    assert d["groups"] == G and d["by"] == by and set(d["sigma"]) == {"mean_logL", "bmd", "D_KL"}
    a, f, logLmax = _inputs(m)
    gq = group_ids(m.gd, "s1", G, by)
    # every group's values against the rule applied to the deleted set, within the bound at that set's n
    got = inf_mod.leave_one_out(a, f, gq, G)
    mean_b, bmd_b, dkl_b = [], [], []
    for b in range(G):
        rest = gq != b
        ex = mc.exact(a[rest], f[rest])
        bd = mc.bounds(ex)
        assert ex["rows"] == int(rest.sum()) == got[b]["rows"] and 0 < ex["rows"] < len(a)
        r = {k: abs(got[b][k] - ex[k]) / bd[k] for k in ("W", "c", "v")}
        print("group %d n=%d error/bound: %s" % (b, ex["rows"], r))
        assert all(x <= 1.0 for x in r.values()), (b, r)
        mean_b.append([logLmax + ex["c"]])
        bmd_b.append([2 * ex["v"]])
        dkl_b.append(logLmax + ex["c"] - jk["lnE_groups"][b])
    # sigma: jackknife.summarise's formula on the exact leave-one-out values
    for key, full, vals in (("mean_logL", [d["mean_logL"]], mean_b), ("bmd", [d["bmd"]], bmd_b), ("D_KL", d["D_KL"], dkl_b)):
        want = summarise(np.asarray(full), np.asarray(vals))[0]
        assert np.allclose(np.atleast_1d(d["sigma"][key]), want, rtol=1e-9, atol=0), (key, d["sigma"][key], want)
        assert np.all(want > 0)


def test_refused_combinations():
    ch = gaussian_chain(seed=2, n=2000, d=3)
    with pytest.raises(ValueError, match="information with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=3, brange=[2.5, 3.2], bscale="logpower", backend=OracleBackend(), information=True)
    with pytest.raises(ValueError, match="information with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=2, backend=OracleBackend(), information=True)
    with pytest.raises(ValueError, match="information with isfunc"):
        MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend(), information=True)
    # neither refusal without the keyword
    MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend())
    # resident.plan declines nothing for the keyword and has no reason for it
    from mcevidence_amd import resident
    assert not any("information" in k or "information" in v for k, v in resident.REASONS.items())


def test_status_through_mcevidence(caplog):
    ch = gaussian_chain(seed=6, n=800, d=3, weights="int")
    bad = ch.copy()
    bad[123, 1] = np.inf                                   # -ln L = +inf: fs = -inf on a row with weight; the estimator adds exp(-inf) = 0
    plain = MCEvidence([bad], kmax=3, verbose=0, backend=OracleBackend()).evidence()
    assert np.all(np.isfinite(plain))
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        lnE, info = MCEvidence([bad], kmax=3, verbose=0, backend=OracleBackend(), information=True).evidence(info=True)
    d = info["information"]
    assert np.array_equal(lnE, plain)
    assert d["status"] == 3 and d["rows"] == 800 and np.isnan(d["D_KL"]).all() and all(math.isnan(d[k]) for k in ("mean_logL", "var_logL", "bmd", "ess", "sum_w"))
    assert sum("information: status 3" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING) == 1


def test_command_line(tmp_path, monkeypatch, capsys, caplog):
    from mcevidence_amd import cli, evidence
    from mcevidence_amd.synth import write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=400, d=3, weights="int") for i in range(3)], [("p%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    args = [root, "-k", "3", "--allparams"]
    # with --jackknife the lines are printed before the ln(B) lines and carry +- sigma
    cli.main(args + ["-vb", "0", "--information", "--jackknife=4"])
    out = capsys.readouterr().out.splitlines()
    at = {key: [i for i, ln in enumerate(out) if ln.strip().startswith(key)] for key in ("<ln L> =", "d =", "N_eff =", "D_KL[k=1] =", "D_KL[k=2] =", "ln(B)[k=1] =")}
    assert all(len(v) == 1 for v in at.values()), at
    assert at["<ln L> ="][0] < at["d ="][0] < at["N_eff ="][0] < at["D_KL[k=1] ="][0] < at["D_KL[k=2] ="][0] < at["ln(B)[k=1] ="][0]
    assert all("±" in out[at[k][0]] for k in ("<ln L> =", "d =", "D_KL[k=1] =", "D_KL[k=2] =")) and "±" not in out[at["N_eff ="][0]]
    # without it they come where the ln(B) lines come from, before them, without +-
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1", "--information"])
    msgs = [r.getMessage().strip() for r in caplog.records]
    first = {key: min(i for i, m in enumerate(msgs) if m.startswith(key)) for key in ("<ln L> =", "d =", "N_eff =", "D_KL[k=1] =", "ln(B)[k=1] =")}
    assert first["<ln L> ="] < first["d ="] < first["N_eff ="] < first["D_KL[k=1] ="] < first["ln(B)[k=1] ="]
    assert not any("±" in m for m in msgs)
    # and without the flag there is no such line
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1"])
    assert not any(r.getMessage().strip().startswith(("<ln L>", "D_KL", "N_eff")) for r in caplog.records)
    assert cli.build_parser().parse_args([root, "--information", "--resident"]).information is True
    assert cli.build_parser().parse_args([root, "--farm"]).information is False


@pytest.mark.parametrize("seed", range(5))
def test_gaussian_samples_give_their_dimension(seed):
    """iid N(0, I_4), logL = -|x|^2 / 2: <ln L> = -2 and d = 4; 5 sigma of the sampling error at n = 20 000 (sqrt(d/2/n) = 0.01 and
    2 sqrt((24 - 4)/n) = 0.063)"""
    n = 20000
    x = np.random.default_rng(seed).standard_normal((n, 4))
    logL = -0.5 * np.sum(x * x, axis=1)
    mom = inf_mod.moments(np.ones(n), logL - logL.max())
    d = inf_mod.build(mom, logL.max(), np.zeros(1))
    print("seed %d: mean_logL + 2 = %.4f, bmd - 4 = %.4f" % (seed, d["mean_logL"] + 2, d["bmd"] - 4))
    assert abs(d["mean_logL"] + 2) <= 0.05
    assert abs(d["bmd"] - 4) <= 0.32
    assert d["ess"] == n


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    lib = _capi.load()
    for s in ("mce_like_moments_workspace_bytes", "mce_like_moments_dev", "mce_like_moments_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_MOMENTS_OUT == 6 == len(_capi.MOMENTS_FIELDS)
    assert _capi.like_moments_workspace_bytes(1000, 3) > 0 and _capi.like_moments_workspace_bytes(0, 1) > 0
    assert _capi.like_moments_workspace_bytes(10, 0) == 0 and _capi.like_moments_workspace_bytes(-1, 1) == 0
    # argument errors come before any device call
    with pytest.raises(ValueError):
        _capi.like_moments_dev([], 1, 1024)
    with pytest.raises(ValueError, match="segment 0"):
        _capi.like_moments_dev([(0, 0, 5)], 1, 1 << 20)
    with pytest.raises(ValueError):
        _capi.like_moments([(np.zeros(3), np.zeros(4))])
