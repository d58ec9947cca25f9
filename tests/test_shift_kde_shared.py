"""The KDE shift without a GPU: the serial driver of mcevidence_amd/csrc/kde_shift.hpp (tests/native/kde_shift_check.cpp, built with
-fsanitize=address,undefined as a stand-alone program) and its NumPy form ``shift_kde.measure`` against the oracle of tests/kde_cases.py
within the derived bound, the decision intervals, every status, the difference chain, the statistical check on Gaussian differences, the
new symbols and their argument errors, and that nothing moves without the keyword or the flag."""
import logging
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import kde_cases as kc
from helpers import REPO, OracleBackend
from mcevidence_amd import shift_kde as sk
from mcevidence_amd import tension as tn


@pytest.fixture
def oracle():
    """only the tests that hold a value to the oracle need mpmath"""
    return pytest.importorskip("mpmath")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kde_shift") / "kde_shift_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "kde_shift_check.cpp"), "-o", exe])
    return exe


def run_native(exe, tmp_path, systems):
    """[(x[n, ld], d, w, linv, mean, point, c)] through the sanitized program -> one block dict (with dens and z) per system"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        for x, d, w, linv, mean, point, c in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            fh.write(struct.pack("<qqq", len(w), d, x.shape[1]))
            for a in (x, w, linv, mean, point):
                fh.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
            fh.write(struct.pack("<d", c))
    out = subprocess.run([exe, "kde", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(systems)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = np.frombuffer(open(fout, "rb").read(), dtype="<f8")
    blocks, at = [], 0
    for x, d, w, linv, mean, point, c in systems:
        n = len(w)
        blk = sk.from_block(raw[at:at + sk.OUT], raw[at + sk.OUT:at + sk.OUT + n + 1].copy())
        blk["z"] = raw[at + sk.OUT + n + 1:at + sk.OUT + n + 1 + n * d].reshape(n, d)
        blocks.append(blk)
        at += sk.OUT + n + 1 + n * d
    assert at == raw.size
    return blocks


def test_parts_tile_the_reference_range(checker):
    out = subprocess.run([checker, "parts"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().startswith("ok records="), out.stdout + out.stderr
    for n in kc.SIZES:
        assert all(0 < b < n for b in kc.boundaries(n)) and len(kc.queries(n, 64)) <= 64


@pytest.mark.parametrize("group", ["ACDE"] + ["B_d%d" % d for d in kc.DIMS])
def test_serial_driver_and_numpy_form_within_the_bound_of_the_oracle(checker, tmp_path, oracle, group):
    assert len(kc.cases()) == 4 + len(kc.SIZES) * len(kc.DIMS) and sum(len(v) for v in kc.groups().values()) == len(kc.cases())
    cases = [kc.cases()[n] for n in kc.groups()[group]]
    native = run_native(checker, tmp_path, [c.system for c in cases])
    for c, nat in zip(cases, native):
        num = sk.measure(c.x[:, :c.d], c.w, c.linv, c.mean, c.point, c.c)
        kc.check(c, nat, "native")
        kc.check(c, num, "numpy ")
        kc.check_two(c, nat, num, "native / numpy")
        # the whitened rows: within their bound of each other, zeros where the row is not used
        y = np.abs(c.x[c.used][:, :c.d] - c.mean[None, :])
        assert np.all(np.abs(nat["z"][c.used] - num["z"][c.used]) <= 2.0 * kc.gamma(c.d + 2) * (y @ np.abs(c.linv).T)), c.name
        unused = np.setdiff1d(np.arange(c.n), c.used)
        assert not nat["z"][unused].any() and not num["z"][unused].any()


def test_decision_intervals_of_both_forms(checker, tmp_path, oracle):
    cases = [c for c in kc.cases().values() if c.decide]
    assert {c.name for c in cases} >= {"A", "C", "D", "E"} and len(cases) == 8
    native = run_native(checker, tmp_path, [c.system for c in cases])
    for c, nat in zip(cases, native):
        kc.check_all_rows_model(c)
        kc.check_masses(c, nat, "native")
        kc.check_masses(c, sk.measure(c.x[:, :c.d], c.w, c.linv, c.mean, c.point, c.c), "numpy ")
    # D reaches the subnormal range and the underflow; E has exact zeros of the distance
    D = kc.cases()["D"]
    t = sk.measure(D.x, D.w, D.linv, D.mean, D.point, D.c)
    z = D.x
    arg = D.c * ((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2)
    assert ((arg > 708.4) & (arg < 744.4)).sum() > 100 and (arg > 746.0).sum() > 10000 and np.isfinite(t["dens"]).all()


def test_status_cases_of_both_forms(checker, tmp_path, caplog):
    cases = kc.status_cases()
    assert sorted({s for _, _, s, _ in cases}) == [3, 4, 5, 6]
    native = run_native(checker, tmp_path, [s for _, s, _, _ in cases])
    for (name, (x, d, w, linv, mean, point, c), status, column), nat in zip(cases, native):
        for got in (nat, sk.measure(x, w, linv, mean, point, c)):
            assert (got["status"], got["column"]) == (status, column), (name, got["status"], got["column"])
            assert got["rows"] == int(np.count_nonzero(w != 0)), (name, got["rows"])
            assert all(np.isnan(got[k]).all() for k in ("W", "A2", "c", "S0", "Q0", "M", "M_eq", "dens")), (name, got)
    # the dict: every value NaN, one WARNING in the route-independent words, nothing raised; status 7 from a constant column
    rng = np.random.default_rng(0)
    xa, xb = rng.standard_normal((300, 3)), rng.standard_normal((300, 3))
    xa[:, 1] = 2.0
    xb[:, 1] = 1.0
    for bad, status in (((xa, np.ones(300), xb, np.ones(300)), 7), ((xa, -np.ones(300), xb, np.ones(300)), 3), ((xa, np.zeros(300), xb, np.ones(300)), 5)):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
            d = sk.estimate(*bad, native=False)
        warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
        assert len(warned) == 1 and "shift kde: status %d" % status in warned[0] and sk.STATUS_WORDS[status] in warned[0], warned
        assert d["status"] == status and all(math.isnan(d[k]) for k in ("p", "p_lo", "p_hi", "sigma_p", "sigma_equiv", "n_local", "ess_eff", "h"))
    # the second WARNING leaves the values as they are
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        d = sk.estimate(rng.standard_normal((400, 6)), np.ones(400), rng.standard_normal((400, 6)) + 3.0, np.ones(400), native=False)
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "n_local" in warned[0] and "raise bandwidth_scale or the number of rows" in warned[0]
    assert d["status"] == 0 and d["n_local"] < 10 and 0.0 <= d["p_lo"] <= d["p"] <= d["p_hi"] <= 1.0


def test_difference_chain():
    rng = np.random.default_rng(1)
    xa, a, xb, b = rng.standard_normal((10, 2)), rng.integers(1, 4, 10) * 1.0, rng.standard_normal((7, 2)), rng.integers(1, 4, 7) * 1.0
    ch = sk.difference_chain(xa, a, xb, b)
    ia = [i * 10 // 7 for i in range(7)]
    assert np.array_equal(ch["x"], xa[ia] - xb) and np.array_equal(ch["w"], a[ia] * b) and np.array_equal(ch["a"], a[ia]) and np.array_equal(ch["b"], b)
    ch = sk.difference_chain(xb, b, xa, a, boost=3)           # the longer chain second
    want_x, want_w = [], []
    for s in range(3):
        for i in range(7):
            j = ((i + s * 7 // 3) % 7) * 10 // 7
            want_x.append(xb[i] - xa[j])
            want_w.append(b[i] * a[j])
    assert np.array_equal(ch["x"], np.array(want_x)) and np.array_equal(ch["w"], np.array(want_w)) and ch["x"].shape == (21, 2)
    thin = sk.difference_chain(xb, b, xa, a, boost=3, max_rows=8)        # stride ceil(21 / 8) = 3
    assert np.array_equal(thin["x"], ch["x"][::3]) and np.array_equal(thin["w"], ch["w"][::3]) and thin["w"].size == 7
    assert sk.difference_chain(xb, b, xa, a, boost=3, max_rows=21)["w"].size == 21
    for bad in (dict(boost=0), dict(max_rows=1)):
        with pytest.raises(ValueError, match="shift kde"):
            sk.difference_chain(xa, a, xb, b, **bad)
    with pytest.raises(ValueError, match="shift kde"):
        sk.difference_chain(xa, a, xb[:, :1], b)
    assert sk.bandwidth(4, 1000.0, 2.0) == 4.0 * (4.0 / 6000.0) ** 0.25


@pytest.mark.parametrize("d,scale", [(2, 1.0), (4, 2.0)])
def test_gaussian_differences_give_the_gaussian_p(d, scale):
    """a Gaussian difference has no smoothing bias (the smoothed density is still spherical about the mean after whitening): p is
    Q(d / 2, chi^2 / 2), here 0.05 exactly; |p - 0.05| <= 5 sigma_p, and the Gaussian shift of the same rows agrees with it"""
    import scipy.stats
    chi2 = float(scipy.stats.chi2.isf(0.05, d))
    for seed in range(5):
        rng = np.random.default_rng(seed)
        n = 8000
        delta = np.zeros(d)
        delta[0] = math.sqrt(2.0 * chi2)                    # the difference has covariance 2 I
        xa, xb = rng.standard_normal((n, d)) + delta, rng.standard_normal((n, d))
        a, b = rng.integers(1, 5, n).astype(np.float64), rng.integers(1, 5, n).astype(np.float64)
        s = sk.estimate(xa, a, xb, b, bandwidth_scale=scale, native=False)
        print("d=%d scale=%g seed=%d: p=%.4f [%.4f, %.4f] sigma_p=%.4f n_local=%.1f  (p - 0.05) / sigma_p = %.2f"
              % (d, scale, seed, s["p"], s["p_lo"], s["p_hi"], s["sigma_p"], s["n_local"], (s["p"] - 0.05) / s["sigma_p"]))
        assert s["status"] == 0 and abs(s["p"] - 0.05) <= 5.0 * s["sigma_p"] and s["sigma_p"] < 0.05
        assert s["rows"] == n and s["dof"] == d and not s["limit"] and s["sigma_equiv"] == tn.sigma_equivalent(s["p"])
        from mcevidence_amd import covariance as cv
        ca, cb = cv.build(cv.measure(a, xa)), cv.build(cv.measure(b, xb))
        g = tn._shift(ca, cb, d)
        se = math.sqrt(2.0 * chi2 / (n / 2.5))               # chi^2's own sampling error: 2 sqrt(chi2) sd / sqrt(ess), ess > n / 2.5 for weights 1..4
        assert abs(g["chi2"] - chi2) <= 5.0 * 2.0 * se and abs(g["p"] - 0.05) < 0.03


def test_new_symbols_and_argument_errors():
    from mcevidence_amd import _capi
    lib = _capi.load()
    for s in ("mce_kde_shift_out_doubles", "mce_kde_shift_workspace_bytes", "mce_kde_shift_dev", "mce_kde_shift_f64"):
        assert hasattr(lib, s) and s in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3 and _capi.MCE_KDE_OUT == sk.OUT == 16 == _capi.kde_shift_out_doubles() and _capi.MCE_KDE_MAX_DIM == sk.MAX_DIM == 64
    small, wide = _capi.kde_shift_workspace_bytes(1000, 1, 3), _capi.kde_shift_workspace_bytes(1000, 1, 64)
    assert 0 < small < wide < 2 ** 20
    # the whitened rows and the parts' sums dominate: (dpad + 1 + 8) doubles per row
    assert 262144 * 21 * 8 < _capi.kde_shift_workspace_bytes(262144, 1, 12) < 262144 * 22 * 8
    for bad in ((-1, 1, 4), (10, 0, 4), (10, 1, 0), (10, 1, 65), (10, (1 << 16) + 1, 4)):
        assert _capi.kde_shift_workspace_bytes(*bad) == 0, bad
    # argument errors come before any device call
    L, m = np.eye(4), np.zeros(4)
    ok = (8, 4, 5, 4, 8, L, m, m, 0.5, 0, 0)
    edit = lambda k, v: tuple(v if i == k else a for i, a in enumerate(ok))          # noqa: E731
    for segs, words in (([], "segments"), ([edit(1, 3)], "segment 0"), ([edit(3, 0)], "segment 0"), ([ok, (8, 70, 5, 65, 8, None, None, None, 0.5, 0, 0)], "segment 1"),
                        ([edit(2, -1)], "segment 0"), ([edit(0, 0)], "segment 0"), ([edit(4, 0)], "segment 0"), ([edit(5, None)], "segment 0"),
                        ([edit(6, None)], "segment 0"), ([edit(7, None)], "segment 0"), ([edit(8, 0.0)], "segment 0"), ([edit(8, float("nan"))], "segment 0"),
                        ([edit(8, float("inf"))], "segment 0"), ([edit(5, np.eye(3))], "segment 0")):
        with pytest.raises(ValueError, match=words):
            _capi.kde_shift_dev(segs, 1, 1 << 30)
    with pytest.raises(ValueError, match="null pointer"):
        _capi.kde_shift_dev([ok], 0, 1 << 30)
    with pytest.raises(ValueError):
        _capi.kde_shift([(np.zeros((3, 2)), 2, np.zeros(4), np.eye(2), np.zeros(2), np.zeros(2), 1.0)])
    with pytest.raises(ValueError, match="bandwidth_scale"):
        sk.estimate(np.zeros((3, 2)), np.ones(3), np.zeros((3, 2)), np.ones(3), bandwidth_scale=0.0)
    with pytest.raises(ValueError, match="shared parameters"):
        sk.estimate(np.zeros((3, 65)), np.ones(3), np.zeros((3, 65)), np.ones(3))


def test_no_device_is_its_own_error():
    from mcevidence_amd import _capi
    c = kc.cases()["B_17_3"]
    if _capi.device_count() > 0:                           # (a device is visible: the same call answers)
        assert sk.from_block(_capi.kde_shift([c.system])[0][0])["status"] == 0
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.kde_shift([c.system])
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.kde_shift_dev([(8, 4, 5, 4, 8, np.eye(4), np.zeros(4), np.zeros(4), 0.5, 0, 0)], 8, 1 << 30)
    # the public function is the native one: no quiet NumPy route
    with pytest.raises(RuntimeError, match="no HIP device"):
        tn.parameter_shift_kde(c.x[:, :3], c.w, c.x[::-1, :3], c.w)


# ---- nothing moves without the keyword or the flag ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_roots(tmp_path_factory):
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    d = tmp_path_factory.mktemp("shift_kde_roots")
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


def test_the_default_gives_todays_dict_and_lines(three_roots, monkeypatch):
    plain = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend())
    gauss = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), shift="gaussian", boost=3, bandwidth_scale=2.0)
    assert set(plain[3]["tension"]) == {"lnR", "lnI", "lnS", "d", "p", "sigma_equiv", "status", "shift"}
    _same(plain[3]["tension"], gauss[3]["tension"])
    assert tn.lines(plain[3]["tension"]) == tn.lines(gauss[3]["tension"]) and len(tn.lines(plain[3]["tension"])) == 2 + 4
    assert all(np.array_equal(a, b) for a, b in zip(plain[:3], gauss[:3]))
    outs = [(e, i) for e, i in zip(plain[:3], plain[3]["roots"])]
    _same(tn.combine(*outs), tn.combine(*outs, shift_kde=None))
    with pytest.raises(ValueError, match="shift="):
        tn.evidence_tension(*three_roots, route="host", shift="flow")
    # with the keyword, the host route's rows go through ``parameter_shift_kde``; here its NumPy form stands in for the library
    monkeypatch.setattr(tn, "parameter_shift_kde", lambda xa, wa, xb, wb, device=None, **k: sk.estimate(xa, wa, xb, wb, native=False, **k))
    both = tn.evidence_tension(*three_roots, route="host", kmax=3, backend=OracleBackend(), shift="both", bandwidth_scale=1.5)
    t = dict(both[3]["tension"])
    s = t.pop("shift_kde")
    _same(plain[3]["tension"], t)
    assert s["names"] == ["om", "h"] and s["status"] == 0 and s["rows"] == 800 and s["bandwidth_scale"] == 1.5 and 0.0 <= s["p_lo"] <= s["p"] <= s["p_hi"] <= 1.0
    lines = tn.lines(both[3]["tension"])
    assert lines[:-1] == tn.lines(plain[3]["tension"]) and lines[-1].startswith("   shift kde (om, h): p = %s [%s, %s]" % (s["p"], s["p_lo"], s["p_hi"]))
    assert all(("%s = %s" % (k, s[v])) in lines[-1] for k, v in (("n_local", "n_local"), ("rows", "rows"), ("h", "h"), ("sigma", "sigma_equiv")))


def test_parser_errors(three_roots, capsys):
    from mcevidence_amd import cli
    ra, rb, rab = three_roots
    p = cli.build_parser()
    assert p.parse_args([rab]).shift_kde is None and p.parse_args([rab, "--tension", ra, rb, "--shift-kde"]).shift_kde == 1
    args = p.parse_args([rab, "--tension", ra, rb, "--shift-kde", "3", "--shift-bandwidth", "2"])
    assert cli._shift_kw(args) == {"shift": "both", "boost": 3, "bandwidth_scale": 2.0} and cli._shift_kw(p.parse_args([rab])) == {}
    for argv, words in (([rab, "--shift-kde"], "belong to --tension"), ([rab, "--shift-bandwidth", "2"], "belong to --tension"),
                        ([rab, "--tension", ra, rb, "--shift-bandwidth", "2"], "belongs to --shift-kde"), ([rab, "--tension", ra, rb, "--shift-kde", "0"], "positive"),
                        ([rab, "--tension", ra, rb, "--shift-kde", "--shift-bandwidth", "0"], "positive")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and words in capsys.readouterr().err, argv
    assert "Gaussian" in tn.FOOTNOTE and "--thin-corr" in tn.FOOTNOTE_KDE and "independent data sets" in tn.FOOTNOTE_KDE
