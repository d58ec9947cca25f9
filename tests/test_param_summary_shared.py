"""summary on the CPU: the rule the host check and the device kernels share (mcevidence_amd/csrc/param_summary.hpp: its serial driver,
built with -fsanitize=address,undefined as a stand-alone program) and its NumPy form ``summary.measure`` against the exact rational
model of tests/summary_cases.py, within the bounds derived in docs/design/summary.md and with every kept quantile exact;
``MCEvidence(..., summary=...)`` for the auto and the cross form through the host loop and the device-feeder hook; ``evidence_many``; the
refusals; ``resident.plan``; the status cases; the untouched default; the command line and the names of a .paramnames file; a statistical
check on Gaussian samples; the new C symbols."""
import logging
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import summary_cases as sc
from helpers import REPO, OracleBackend, OracleFeedBackend
from mcevidence_amd import summary as sm
from mcevidence_amd.evidence import MCEvidence, evidence_many
from mcevidence_amd.synth import gaussian_chain


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("param_summary") / "param_summary_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "param_summary_check.cpp"), "-o", exe])
    return exe


def run_native(exe, tmp_path, systems, q):
    """[(a, x[n, ld], d, f or None)] through the sanitized program -> one block dict per system"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    q = np.ascontiguousarray(q, dtype="<f8")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", q.size))
        fh.write(q.tobytes())
        for a, x, d, f in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            x = x if x.ndim == 2 else x.reshape(len(a), -1)
            fh.write(struct.pack("<qqqq", len(a), d, x.shape[1], 0 if f is None else 1))
            fh.write(x.tobytes())
            fh.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
            if f is not None:
                fh.write(np.ascontiguousarray(f, dtype="<f8").tobytes())
    out = subprocess.run([exe, "summary", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(systems)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = np.frombuffer(open(fout, "rb").read(), dtype="<f8")
    blocks, at = [], 0
    for a, x, d, f in systems:
        size = sm.HEAD + d * (sm.PER_COL + q.size)
        blocks.append(sm.from_block(raw[at:at + size], d, q.size))
        at += size
    assert at == raw.size
    return blocks


def test_keys_keep_the_order_of_the_doubles(checker):
    out = subprocess.run([checker, "keys"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().startswith("ok records="), out.stdout + out.stderr


def test_serial_driver_and_numpy_form_equal_the_exact_model(checker, tmp_path):
    cases = sc.cpu_cases()
    assert len(cases) == 44 and sum(c.exact["keep"].size for c in cases) == 220
    native = run_native(checker, tmp_path, [(c.a, c.x, c.d, c.f) for c in cases], sc.TARGETS)
    counts = [0, 0]
    for c, nat in zip(cases, native):
        sc.check(c, nat, "native", counts)
        sc.check(c, sm.measure(c.a, c.x[:, :c.d], c.f, c.q), "numpy ")
    print("kept %d, dropped %d of %d triples" % (counts[0], counts[1], sum(counts)))
    assert 10 * counts[1] <= sum(counts)


def test_the_wide_and_the_adversarial_cases_on_the_host(checker, tmp_path):
    # what the device is asked (tests/test_gpu_param_summary.py), asked of the two host forms: zero weights over NaN, the keys'
    # adversaries, best-fit ties, d = 127 with ld > d, no fs
    names = ["D_zeros", "E_keys_1", "E_keys_2", "E_keys_1000", "B_513_127", "C_narrow", "K_ties", "K_last", "K_minus_inf"]
    g = sc.gpu_cases()
    native = run_native(checker, tmp_path, [(g[n].a, g[n].x, g[n].d, g[n].f) for n in names], sc.TARGETS)
    for n, nat in zip(names, native):
        sc.check(g[n], nat, "native")
        sc.check(g[n], sm.measure(g[n].a, g[n].x[:, :g[n].d], g[n].f, g[n].q), "numpy ")
    e = sm.measure(g["E_keys_1000"].a, g["E_keys_1000"].x, g["E_keys_1000"].f, sc.TARGETS)
    assert e["var"][6] == 0.0 and np.all(e["quant"][:, 6] == 2.5) and e["min"][6] == e["max"][6] == 2.5      # the constant column
    assert g["K_ties"].exact["bestfit_row"] == 33 and g["K_last"].exact["bestfit_row"] == 1024 and g["K_minus_inf"].exact["bestfit_row"] == 3
    t = g["T_tie"]
    tie, = run_native(checker, tmp_path, [(t.a, t.x, 1, None)], t.q)
    for got in (tie, sm.measure(t.a, t.x, None, t.q)):
        assert got["quant"][0, 0] == np.sort(t.x[:, 0])[499] and got["bestfit_row"] == -1 and np.isnan(got["bestfit"]).all()


def test_status_cases_of_both_forms(checker, tmp_path, caplog):
    cases = sc.status_cases()
    native = run_native(checker, tmp_path, [(a, x, x.shape[1], f) for _, a, x, f, _, _ in cases], sc.TARGETS)
    for (name, a, x, f, status, column), nat in zip(cases, native):
        for got in (nat, sm.measure(a, x, f, sc.TARGETS)):
            assert (got["status"], got["column"]) == (status, column), (name, got["status"], got["column"])
            assert got["rows"] == int(np.count_nonzero(a != 0)) and got["bestfit_row"] == -1, (name, got)
            assert all(np.isnan(got[k]).all() for k in ("W", "A2", "bestfit_f", "mean", "var", "min", "max", "bestfit", "quant")), (name, got)
    # the dict: every value NaN, the status kept, one WARNING in the route-independent words, nothing raised
    for status in (3, 5):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            d = sm.build(sm._nan_block(3, 5, 7, status, -1), (0.68, 0.95), -3.0)
        warned = [r for r in caplog.records if r.levelno == logging.WARNING]
        assert len(warned) == 1 and "summary: status %d" % status in warned[0].getMessage() and sm.STATUS_WORDS[status] in warned[0].getMessage()
        assert d["status"] == status and d["rows"] == 7 and d["bestfit_row"] == -1 and d["names"] == ["p0", "p1", "p2"]
        assert all(np.isnan(d[k]).all() for k in ("sum_w", "ess", "mean", "sd", "var", "min", "max", "median", "lower", "upper", "bestfit", "bestfit_loglike"))


def test_keyword_values():
    assert sm.spec(None) is None and sm.spec(False) is None and sm.spec(True) == (0.68, 0.95) and sm.spec(0.9) == (0.9,) and sm.spec([0.5, 0.99]) == (0.5, 0.99)
    assert np.array_equal(sm.targets((0.68, 0.95)), sc.TARGETS)
    for bad in (0.0, 1.0, -0.5, (0.5, 1.5), (), tuple([0.5] * 8), "0.68", float("nan")):
        with pytest.raises(ValueError, match="summary="):
            sm.spec(bad)
    assert len(sm.spec(tuple([0.5] * 7))) == 7


def _inputs(m, pos_lnp=False):
    """(a, x, f, logLmax) of the rule for an MCEvidence object, formed apart from the package's code path"""
    part = m.gd.data["s1"]
    logL = np.asarray(part.loglikes if pos_lnp else -part.loglikes, dtype=np.float64)
    return np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)[:, :m.ndim], logL - logL.max(), float(logL.max())


KEYS = {"probs", "q", "rows", "sum_w", "ess", "names", "mean", "sd", "var", "min", "max", "median", "lower", "upper", "bestfit", "bestfit_row", "bestfit_loglike",
        "status", "column"}


def _check_dict(d, a, x, f, logLmax, what, probs=(0.68, 0.95)):
    assert set(d) == KEYS and d["probs"] == tuple(probs) and np.array_equal(d["q"], sm.targets(probs)), (what, set(d) ^ KEYS)
    case = sc.Case(what, a, x, f, q=sm.targets(probs))
    blk = dict(W=d["sum_w"], A2=d["sum_w"] ** 2 / d["ess"], rows=d["rows"], status=d["status"], column=d["column"], mean=d["mean"], var=d["var"], min=d["min"],
               max=d["max"], bestfit=d["bestfit"], bestfit_row=d["bestfit_row"], bestfit_f=case.exact["bestfit_f"],
               quant=np.concatenate([d["median"][None, :]] + [r[None, :] for lo, hi in zip(d["lower"], d["upper"]) for r in (lo, hi)]))
    sc.check(case, blk, what)
    assert d["lower"].shape == d["upper"].shape == (len(probs), x.shape[1])
    assert np.all(np.abs(d["sd"] - np.sqrt(d["var"])) <= 2 * sc.EPS * d["sd"])
    assert d["bestfit_loglike"] == logLmax + case.exact["bestfit_f"] and len(d["names"]) == x.shape[1]


def test_mcevidence_auto_and_cross_forms():
    ch = gaussian_chain(seed=3, n=1500, d=4, weights="int")
    for split, backend in ((False, OracleBackend), (True, OracleBackend), (False, OracleFeedBackend), (True, OracleFeedBackend)):
        np.random.seed(5)
        m = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend(), summary=True)
        lnE, info = m.evidence(info=True)
        a, x, f, logLmax = _inputs(m)
        assert len(a) == (750 if split else 1500) and m.param_summary is info["summary"]
        _check_dict(info["summary"], a, x, f, logLmax, "split=%s %s" % (split, backend.__name__))
        if not split:                                      # the rows are the chain's own: raw, not whitened
            assert np.array_equal(info["summary"]["min"], ch[:, 2:].min(axis=0)) and info["summary"]["bestfit_row"] == int(np.argmin(ch[:, 1]))
        np.random.seed(5)
        plain, pinfo = MCEvidence([ch], kmax=4, verbose=0, split=split, backend=backend()).evidence(info=True)
        assert np.array_equal(lnE, plain) and "summary" not in pinfo
    # ndim below the sampled parameters, other probabilities, pos_lnp
    pos = ch.copy()
    pos[:, 1] = -pos[:, 1]
    m = MCEvidence([pos], kmax=3, verbose=0, ndim=2, backend=OracleBackend(), summary=(0.5, 0.9, 0.99))
    lnE, info = m.evidence(info=True, pos_lnp=True)
    assert info["summary"]["mean"].shape == (2,)
    _check_dict(info["summary"], *_inputs(m, pos_lnp=True), "pos_lnp", probs=(0.5, 0.9, 0.99))
    # with the jackknife set the summary is what it is without it
    with_jk = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=True, jackknife=4).evidence(info=True)[1]["summary"]
    without = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=True).evidence(info=True)[1]["summary"]
    assert all(np.array_equal(np.asarray(with_jk[k]), np.asarray(without[k])) for k in KEYS - {"names", "probs"}) and "sigma" not in with_jk
    # evidence_many fills it too
    ms = [MCEvidence([gaussian_chain(seed=s, n=401, d=3, weights="int")], kmax=3, verbose=0, backend=OracleBackend(), summary=True) for s in (1, 2)]
    for m, (lnE, info) in zip(ms, evidence_many(ms, info=True)):
        _check_dict(info["summary"], *_inputs(m), "evidence_many")


def test_without_the_keyword_nothing_changes():
    ch = gaussian_chain(seed=8, n=900, d=3, weights="int")
    a, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend()).evidence(info=True)
    assert "summary" not in info
    for off in (None, False):
        b, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=off).evidence(info=True)
        assert "summary" not in info and np.array_equal(a, b)
    c, info = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=True).evidence(info=True)
    assert np.array_equal(a, c) and "summary" in info


def test_refused_combinations_and_the_plan():
    ch = gaussian_chain(seed=2, n=2000, d=3)
    with pytest.raises(ValueError, match="summary with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=3, brange=[2.5, 3.2], bscale="logpower", backend=OracleBackend(), summary=True)
    with pytest.raises(ValueError, match="summary with batched runs"):
        MCEvidence([ch], kmax=3, verbose=0, nbatch=2, backend=OracleBackend(), summary=True)
    with pytest.raises(ValueError, match="summary with isfunc"):
        MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend(), summary=True)
    with pytest.raises(ValueError, match="summary="):
        MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=1.5)
    with pytest.raises(ValueError, match="summary="):
        MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=tuple([0.5] * 8))
    MCEvidence([ch], kmax=3, verbose=0, isfunc=lambda s: 0.1 * s[:, 0] ** 2, backend=OracleBackend())      # neither refusal without the keyword
    from mcevidence_amd import resident
    assert resident.plan(summary=True) == resident.RESIDENT == resident.plan(summary=(0.5, 0.9)) == resident.plan()
    with pytest.raises(ValueError, match="summary="):
        resident.plan(summary=2.0)
    assert not any("summary" in k or "summary" in v for k, v in resident.REASONS.items())
    # every existing reason, in its order
    for kw, key in ((dict(ischain=False), "ischain"), (dict(thinlen=-1), "negative_thinlen"), (dict(thinlen=0.5), "poisson"), (dict(isfunc=abs), "isfunc"),
                    (dict(nbatch=2), "batches"), (dict(verbose=2), "verbose"), (dict(covtype="diag"), "covtype"), (dict(split=True, covtype="single"), "split_single"),
                    (dict(split=True, jackknife=4), "jackknife_cross"), (dict(ndim=128), "ndim"), (dict(distributed=True), "distributed"),
                    (dict(ncols=[5, 6]), "columns"), (dict(nrows=1), "rows")):
        assert resident.plan(**kw) == resident.plan(summary=True, **kw) == resident.REASONS[key], key
    assert resident.plan(thinlen=0.5, isfunc=abs, summary=True) == resident.REASONS["poisson"]


def test_status_through_mcevidence(caplog):
    ch = gaussian_chain(seed=6, n=800, d=3, weights="int")
    bad = ch.copy()
    bad[123, 3] = np.inf                                   # a value that is not finite in the second measured column
    plain = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend()).evidence()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        lnE, info = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend(), summary=True).evidence(info=True)
        assert info["summary"]["status"] == 0              # (the column is not measured)
        caplog.clear()
        m = MCEvidence([bad], kmax=3, verbose=0, ndim=1, backend=OracleBackend(), summary=True)
        m.ndim = 2                                         # (measure it without sending the row through a search)
        m._fill_summary(False)
    d = m.info["summary"]
    assert np.array_equal(lnE, plain)
    assert d["status"] == 3 and d["column"] == 1 and d["rows"] == 800 and d["bestfit_row"] == -1
    assert all(np.isnan(d[k]).all() for k in ("sum_w", "ess", "mean", "sd", "var", "min", "max", "median", "lower", "upper", "bestfit", "bestfit_loglike"))
    assert sum("summary: status 3" in r.getMessage() for r in caplog.records if r.levelno == logging.WARNING) == 1


def test_command_line_and_parameter_names(tmp_path, monkeypatch, capsys, caplog):
    from mcevidence_amd import cli, evidence
    from mcevidence_amd.synth import write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=400, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    with open(root + ".paramnames", "w") as fh:
        fh.write("om0\t\\Omega_0\nom1   \\Omega_1\n\nom2\n")
    monkeypatch.setattr(evidence, "HipBackend", lambda *a, **k: OracleBackend())
    args = [root, "-k", "3", "--allparams"]
    # with --jackknife the lines are printed, before the ln(B) lines
    cli.main(args + ["-vb", "0", "--summary", "--jackknife=4"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    at = {key: [i for i, ln in enumerate(out) if ln.startswith(key)] for key in ("summary: parameter", "summary: om0", "summary: om1", "summary: om2", "ln(B)[k=1] =")}
    assert all(len(v) == 1 for v in at.values()), at
    assert at["summary: parameter"][0] < at["summary: om0"][0] < at["summary: om1"][0] < at["summary: om2"][0] < at["ln(B)[k=1] ="][0]
    assert len(out[at["summary: om0"][0]].split()) == 2 + 2 + 4 + 1 and "lower68" in out[at["summary: parameter"][0]] and "upper95" in out[at["summary: parameter"][0]]
    # -vb 1 with --jackknife: the class logs them (after the information lines), so the CLI does not print them a second time
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1", "--summary", "--information", "--jackknife=4"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    msgs = [r.getMessage().strip() for r in caplog.records]
    assert not any(ln.startswith("summary:") for ln in printed) and sum(m.startswith("summary: parameter") for m in msgs) == 1
    assert max(i for i, m in enumerate(msgs) if m.startswith(("<ln L>", "D_KL"))) < min(i for i, m in enumerate(msgs) if m.startswith("summary:"))
    # -vb 0: printed once, after the information lines
    cli.main(args + ["-vb", "0", "--summary", "--information", "--jackknife=4"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert sum(ln.startswith("summary: parameter") for ln in printed) == 1
    assert max(i for i, m in enumerate(printed) if m.startswith(("<ln L>", "D_KL"))) < min(i for i, m in enumerate(printed) if m.startswith("summary:"))
    caplog.clear()
    # without it they come where the ln(B) lines come from, before them; the probabilities of the flag are the limits' columns
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1", "--summary", "0.9"])
    msgs = [r.getMessage().strip() for r in caplog.records]
    first = {key: min(i for i, m in enumerate(msgs) if m.startswith(key)) for key in ("summary: parameter", "summary: om0", "summary: om2", "ln(B)[k=1] =")}
    assert first["summary: parameter"] < first["summary: om0"] < first["summary: om2"] < first["ln(B)[k=1] ="]
    assert "lower90" in msgs[first["summary: parameter"]] and len(msgs[first["summary: om0"]].split()) == 2 + 2 + 2 + 1
    # the lines are summary.lines' of the object's dict; the names come from the .paramnames file
    m = MCEvidence(root, kmax=3, verbose=0, backend=OracleBackend(), summary=True)
    m.evidence()
    assert m.param_summary["names"] == ["om0", "om1", "om2"] and [ln.strip() for ln in sm.lines(m.param_summary)][1].startswith("summary: om0")
    assert sm.param_names(str(tmp_path / "none"), 2) == ["p0", "p1"] and sm.param_names(root, 5) == ["om0", "om1", "om2", "p3", "p4"]
    # and without the flag there is no such line
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1"])
    assert not any(r.getMessage().strip().startswith("summary:") for r in caplog.records)
    p = cli.build_parser()
    assert p.parse_args([root, "--summary", "--resident"]).summary == [] and p.parse_args([root, "--farm", "--summary", "0.5", "0.9"]).summary == [0.5, 0.9]
    assert p.parse_args([root, "--farm"]).summary is None
    assert cli._summary_kw(p.parse_args([root, "--summary"])) == {"summary": True} and cli._summary_kw(p.parse_args([root])) == {}


@pytest.mark.parametrize("seed", range(5))
def test_gaussian_samples_give_their_moments(seed):
    """iid N(0, I_4), unit weights, n = 20 000: 5 sigma of the sampling error of a mean (1 / sqrt(n)), of an sd (1 / sqrt(2 n)) and of a
    normal quantile at the 16 % / 84 % level (sqrt(q (1 - q)) / phi(z) / sqrt(n) = 1.37 / sqrt(n) at z = 0.9945)"""
    n = 20000
    x = np.random.default_rng(seed).standard_normal((n, 4))
    logL = -0.5 * np.sum(x * x, axis=1)
    d = sm.build(sm.measure(np.ones(n), x, logL - logL.max(), sm.targets(sm.DEFAULT_PROBS)), sm.DEFAULT_PROBS, logL.max())
    z = 0.9944578832097535
    worst = (np.abs(d["mean"]).max() * math.sqrt(n), np.abs(d["sd"] - 1).max() * math.sqrt(2 * n),
             max(np.abs(d["lower"][0] + z).max(), np.abs(d["upper"][0] - z).max()) * math.sqrt(n) / 1.37)
    print("seed %d: |mean| %.2f sigma, |sd - 1| %.2f sigma, 68 %% limits %.2f sigma" % ((seed,) + worst))
    assert all(w <= 5.0 for w in worst)
    assert d["ess"] == n and d["bestfit_row"] == int(np.argmax(logL)) and d["bestfit_loglike"] == logL.max()


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    lib = _capi.load()
    for s in ("mce_param_summary_out_doubles", "mce_param_summary_workspace_bytes", "mce_param_summary_dev", "mce_param_summary_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_SUMMARY_HEAD == sm.HEAD == 8 and _capi.MCE_SUMMARY_MAX_Q == 16
    assert _capi.param_summary_out_doubles(27, 5) == 8 + 27 * 10 == _capi.summary_block_doubles(27, 5)
    assert _capi.param_summary_out_doubles(0, 5) == 0 == _capi.param_summary_out_doubles(128, 5) == _capi.param_summary_out_doubles(4, 17)
    small, big = _capi.param_summary_workspace_bytes(1000, 1000, 1, 8, 5), _capi.param_summary_workspace_bytes(2 * 10 ** 6, 2 * 10 ** 6, 1, 27, 5)
    assert 0 < small < 2 ** 21 and 32 * 2 ** 25 < big < 32 * 2 ** 25 + 2 ** 26      # the sort's buffers stop growing at the size of a pass
    assert _capi.param_summary_workspace_bytes(10 ** 6, 10 ** 6, 1, 27, 5, 1 << 22) < 2 ** 28
    for bad in ((-1, 0, 1, 4, 5), (10, 20, 1, 4, 5), (10, 10, 0, 4, 5), (10, 10, 1, 128, 5), (10, 10, 1, 4, 0), (10, 10, 1, 4, 17), (10, 10, 1, 4, 5, -1)):
        assert _capi.param_summary_workspace_bytes(*bad) == 0, bad
    # argument errors come before any device call
    ok = (1, 4, 5, 4, 1, 0)
    for segs, q, words in (([], [0.5], "segments"), ([ok], [], "targets"), ([ok], [0.5] * 17, "targets"), ([ok], [0.0], "target 0"), ([ok], [0.5, 1.0], "target 1"),
                           ([(1, 3, 5, 4, 1, 0)], [0.5], "segment 0"), ([(1, 4, 5, 0, 1, 0)], [0.5], "segment 0"), ([ok, (1, 200, 5, 128, 1, 0)], [0.5], "segment 1"),
                           ([(1, 4, -1, 4, 1, 0)], [0.5], "segment 0"), ([(0, 4, 5, 4, 1, 0)], [0.5], "segment 0")):
        with pytest.raises(ValueError, match=words):
            _capi.param_summary_dev(segs, q, 1, 1 << 30)
    with pytest.raises(ValueError, match="pass_elems"):
        _capi.param_summary_dev([ok], [0.5], 1, 1 << 30, pass_elems=-1)
    with pytest.raises(ValueError):
        _capi.param_summary([(np.zeros((3, 2)), 2, np.zeros(4), None)], [0.5])


def test_the_summary_method_of_the_class_still_prints(capsys):
    """``MCEvidence.summary()`` is the reference's method: the keyword's result is kept as ``param_summary`` so that it stays callable"""
    ch = gaussian_chain(seed=4, n=500, d=3, weights="int")
    for kw in ({}, {"summary": True}, {"summary": (0.9,)}):
        m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), **kw)
        for after_evidence in (False, True):
            if after_evidence:
                m.evidence()
            capsys.readouterr()
            assert m.summary() is None
            out = capsys.readouterr().out
            assert all("%s=" % k in out for k in ("ndim", "nsample", "kmax", "brange", "bsize", "powers", "nchain")) and "ndim=3" in out, (kw, out)
        assert (m.param_summary is None) == (not kw) and callable(m.summary)


def test_no_device_is_its_own_error():
    from mcevidence_amd import _capi
    c = sc.cpu_cases()[20]
    if _capi.device_count() > 0:                           # (a device is visible: the same call answers)
        assert sm.from_block(_capi.param_summary([c.system], sc.TARGETS)[0], c.d, len(sc.TARGETS))["status"] == 0
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_summary([c.system], sc.TARGETS)
    # the device form: valid arguments, so the refusal is the missing device's (argument errors come first and need none)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.param_summary_dev([(8, 4, 5, 4, 8, 8)], [0.5], 8, 1 << 30)


def test_under_a_process_group_every_rank_computes_its_own_on_the_host(monkeypatch):
    import torch.distributed as dist
    from mcevidence_amd import parallel
    ch = gaussian_chain(seed=12, n=700, d=3, weights="int")
    want = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=True).evidence(info=True)[1]["summary"]
    m = MCEvidence([ch], kmax=3, verbose=0, backend=OracleBackend(), summary=True)

    def refuse(*a, **k):
        raise AssertionError("a collective was called")
    monkeypatch.setattr(parallel, "is_distributed", lambda *a, **k: True)
    for name in ("all_reduce", "all_gather", "all_gather_object", "broadcast", "broadcast_object_list", "barrier", "reduce", "gather", "all_to_all_single"):
        monkeypatch.setattr(dist, name, refuse)
    m._fill_summary(False)
    got = m.info["summary"]
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in KEYS - {"names", "probs"}) and got["names"] == want["names"]
    # and the device routes decline to the host route there
    from mcevidence_amd import resident
    assert resident.plan(distributed=True, summary=True) == resident.REASONS["distributed"]


def test_the_farm_rule_for_one_value_or_one_per_root():
    from mcevidence_amd.farm import _per_root_summary
    assert _per_root_summary(None, 3) == [None] * 3 and _per_root_summary(True, 2) == [True, True]
    assert _per_root_summary((0.68, 0.95), 2) == [(0.68, 0.95)] * 2 and _per_root_summary([0.9, 0.5], 2) == [[0.9, 0.5]] * 2      # bare numbers: ONE value
    assert _per_root_summary([(0.9,), None], 2) == [(0.9,), None] and _per_root_summary([True, False, (0.5, 0.9)], 3) == [True, False, (0.5, 0.9)]
    with pytest.raises(ValueError, match="summary: expected 2 entries, got 3"):
        _per_root_summary([True, None, None], 2)
    with pytest.raises(ValueError, match="not a mixture"):
        _per_root_summary([0.5, None], 2)
