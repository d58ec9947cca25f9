"""The KDE shift on the device: ``mce_kde_shift_dev`` / ``mce_kde_shift_f64`` on the cases of tests/kde_cases.py against the mpmath oracle
within the derived bound and against ``shift_kde.measure`` within two bounds, the decision intervals of the masses, every status between
two good systems, mixed shapes in several orders around an empty segment, two runs and the host-pointer twin bit for bit; then
``evidence_tension(shift="both")`` through the farm and on the host route, and the command line."""
import functools
import math

import numpy as np
import pytest

import kde_cases as kc
from mcevidence_amd import shift_kde as sk

pytestmark = pytest.mark.gpu


@pytest.fixture
def oracle():
    """only the tests that hold a value to the oracle need mpmath"""
    return pytest.importorskip("mpmath")


def _blocks(systems):
    """one ``mce_kde_shift_f64`` call -> one dict per system, with the densities and the whitened rows"""
    from mcevidence_amd import _capi
    out = []
    for blk, dens, z in _capi.kde_shift(systems, want_dens=True, want_z=True):
        b = sk.from_block(blk, dens)
        b["z"], b["raw"] = z, np.array(blk)
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def all_cases_in_one_call():
    cases = list(kc.cases().values())
    return cases, _blocks([c.system for c in cases])


@functools.lru_cache(maxsize=None)
def single(name):
    """the case alone in its call"""
    return _blocks([kc.cases()[name].system])[0]


def _same_bits(a, b, what):
    assert np.array_equal(a["raw"], b["raw"], equal_nan=True), (what, a["raw"], b["raw"])
    assert np.array_equal(a["dens"], b["dens"], equal_nan=True) and np.array_equal(a["z"], b["z"]), what


@pytest.mark.parametrize("group", ["ACDE"] + ["B_d%d" % d for d in kc.DIMS])
def test_cases_against_the_oracle_and_the_numpy_form(oracle, group):
    cases, got = all_cases_in_one_call()
    assert len(cases) == 4 + len(kc.SIZES) * len(kc.DIMS)
    worst = two = 0.0
    for c, g in zip(cases, got):
        if c.name not in kc.groups()[group]:
            continue
        worst = max(worst, kc.check(c, g, "device", verbose=c.n >= 511 or not c.name.startswith("B")))
        num = sk.measure(c.x[:, :c.d], c.w, c.linv, c.mean, c.point, c.c)
        two = max(two, kc.check_two(c, g, num, "device / numpy"))
        y = np.abs(c.x[c.used][:, :c.d] - c.mean[None, :])
        assert np.all(np.abs(g["z"][c.used] - num["z"][c.used]) <= 2.0 * kc.gamma(c.d + 2) * (y @ np.abs(c.linv).T)), c.name
        assert not g["z"][np.setdiff1d(np.arange(c.n), c.used)].any(), c.name
        assert g["A2"] == float(np.sum(c.w[c.used] ** 2)) and g["c"] == c.c and not g["raw"][12:].any()
    print("device %s: worst error / bound over %d cases = %.3g; device against numpy / two bounds = %.3g" % (group, len(kc.groups()[group]), worst, two))


def test_decision_intervals(oracle):
    cases, got = all_cases_in_one_call()
    used = 0
    for c, g in zip(cases, got):
        if c.decide:
            kc.check_all_rows_model(c)
            kc.check_masses(c, g, "device")
            used += 1
    assert used == 8


def test_every_status_between_two_good_systems():
    good = ("B_513_4", "B_65_27")
    for name, system, status, column in kc.status_cases():
        a, bad, b = _blocks([kc.cases()[good[0]].system, system, kc.cases()[good[1]].system])
        _same_bits(a, single(good[0]), name)
        _same_bits(b, single(good[1]), name)
        assert (bad["status"], bad["column"]) == (status, column) and bad["rows"] == int(np.count_nonzero(system[2] != 0)), (name, bad["raw"])
        assert all(np.isnan(bad[k]).all() for k in ("W", "A2", "c", "S0", "Q0", "M", "M_eq", "dens")), (name, bad["raw"])


def test_mixed_shapes_in_three_orders_around_an_empty_segment():
    names = ["B_1025_3", "B_129_27", "B_513_64", "B_17_3", "B_511_27"]
    empty = (np.zeros((0, 5)), 3, np.zeros(0), np.eye(3), np.zeros(3), np.zeros(3), 1.0)
    for order in ((0, 1, 2, 3, 4), (4, 2, 0, 3, 1), (3, 1, 4, 2, 0)):
        systems = [kc.cases()[names[k]].system for k in order]
        got = _blocks(systems[:2] + [empty] + systems[2:])
        assert got[2]["status"] == 5 and got[2]["rows"] == 0
        for k, g in zip(order, got[:2] + got[3:]):
            _same_bits(g, single(names[k]), (order, names[k]))
    # and the one call of every case gave each its own bits too
    cases, got = all_cases_in_one_call()
    for n in names:
        _same_bits(got[[c.name for c in cases].index(n)], single(n), n)


def test_two_runs_and_the_twin_give_the_same_bits():
    import torch
    from mcevidence_amd import _capi
    for name in ("A", "D", "B_1025_5"):
        c = kc.cases()[name]
        _same_bits(_blocks([c.system])[0], single(name), name)
        x, w = torch.from_numpy(c.x).cuda(), torch.from_numpy(c.w).cuda()
        dens = torch.empty(c.n + 1, dtype=torch.float64, device="cuda")
        z = torch.empty((c.n, c.d), dtype=torch.float64, device="cuda")
        wsb = _capi.kde_shift_workspace_bytes(c.n, 1, c.d)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        blk = _capi.kde_shift_dev([(x.data_ptr(), c.x.shape[1], c.n, c.d, w.data_ptr(), c.linv, c.mean, c.point, c.c, dens.data_ptr(), z.data_ptr())],
                                  ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)[0]
        dev = sk.from_block(blk, dens.cpu().numpy())
        dev["z"], dev["raw"] = z.cpu().numpy(), np.array(blk)
        _same_bits(dev, single(name), name + " device form")
        m = sk.measure_dev(x[:, :c.d], w, c.linv, c.mean, c.point, c.c, want_dens=True)
        assert np.array_equal(m["dens"], dev["dens"], equal_nan=True) and np.array_equal(m["M"], dev["M"])


# ---- evidence_tension on both routes and the command line ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_roots(tmp_path_factory):
    """A: 6 parameters, B: 5, AB: 8; the first three are shared; three chains each; A and B of different lengths"""
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    d = tmp_path_factory.mktemp("shift_kde_roots")
    names = {"A": ["om", "h", "tau", "a1", "a2", "a3"], "B": ["om", "h", "tau", "b1", "b2"], "AB": ["om", "h", "tau", "a1", "a2", "a3", "b1", "b2"]}
    out = []
    for k, (name, pn) in enumerate(names.items()):
        root = str(d / name)
        chains = []
        for i, n in enumerate((500 - 60 * k, 450, 400)):
            ch = gaussian_chain(seed=100 * k + i, n=n, d=len(pn), weights="int")
            ch[:, 2:5] += 0.9 * k                          # the shared parameters sit elsewhere in every run
            chains.append(ch)
        write_cosmomc_chains(root, chains, [(p, -9.0, 9.0) for p in pn], fmt="%.17g")
        with open(root + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (p, p) for p in pn))
        out.append(root)
    return out


def _same_dict(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], dict):
            _same_dict(a[k], b[k])
        elif k == "names":
            assert a[k] == b[k]
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_evidence_tension_on_both_routes_and_the_command_line(three_roots, capsys, oracle):
    from mcevidence_amd import _capi, cli
    from mcevidence_amd import covariance as cv
    from mcevidence_amd import tension as tn
    res = {}
    for route in ("farm", "host"):
        plain = tn.evidence_tension(*three_roots, route=route, kmax=3)
        both = tn.evidence_tension(*three_roots, route=route, kmax=3, shift="both", boost=2, bandwidth_scale=1.5)
        t = dict(both[3]["tension"])
        res[route] = t.pop("shift_kde")
        _same_dict(plain[3]["tension"], t)                       # every number that exists today, bit for bit
        assert all(np.array_equal(a, b) for a, b in zip(plain[:3], both[:3]))
    f, h = res["farm"], res["host"]
    assert f["names"] == h["names"] == ["om", "h", "tau"] and f["status"] == h["status"] == 0 and f["boost"] == 2 and f["bandwidth_scale"] == 1.5
    # the model of the difference chain, from the files themselves
    rows = [np.concatenate([np.loadtxt(r + "_%d.txt" % i) for i in (1, 2, 3)]) for r in three_roots[:2]]
    ch = sk.difference_chain(rows[0][:, 2:5], rows[0][:, 0], rows[1][:, 2:5], rows[1][:, 0], boost=2)
    assert f["rows"] == h["rows"] == 2 * min(len(rows[0]), len(rows[1])) == ch["w"].size
    white = sk.whitening(cv.from_block(_capi.param_cov([(ch["x"], 3, ch["w"])])[0], 3), 1.5)
    case = kc.Case("difference chain", ch["x"], 3, ch["w"], white["linv"], white["mean"], np.zeros(3), white["c"], cap=2)
    iv, undecided = case.decision()
    assert undecided <= 1e-3 * float(case.all_rows["W"])
    W = float(case.all_rows["W"])
    for name, s in res.items():
        err = abs(s["t0"] - float(case.exact["t0"]))
        print("%s: t0 error / bound = %.3g, p = %r in [%r, %r]" % (name, err / case.bound["t0"], s["p"], 1.0 - iv[0][1] / W, 1.0 - iv[0][0] / W))
        assert err <= case.bound["t0"] and s["h"] == white["h"]
        for key, (lo, hi) in zip(("p", "p_lo", "p_hi"), iv):
            assert 1.0 - hi / W - 2.0 ** -52 <= s[key] <= 1.0 - lo / W + 2.0 ** -52, (name, key)
    assert abs(f["t0"] - h["t0"]) <= 2.0 * case.bound["t0"] and 0.0 < f["p_lo"] <= f["p"] <= f["p_hi"] < 1.0
    # the command line prints evidence_tension's own numbers, the line after the Gaussian shift and the second footnote sentence
    ra, rb, rab = three_roots
    capsys.readouterr()
    got = cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0", "--shift-kde", "2", "--shift-bandwidth", "1.5"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    want = [ln.strip() for ln in tn.lines(got[3]["tension"])]
    at = [out.index(ln) for ln in want]
    assert at == sorted(at) and want[-1].startswith("shift kde (om, h, tau): p = ") and want[-2].startswith("shift (om, h, tau): chi2 = ")
    assert out.index(tn.FOOTNOTE_KDE.strip()) == out.index(tn.FOOTNOTE) + 1
    _same_dict(got[3]["tension"]["shift_kde"], f)
    cli.main([rab, "--tension", ra, rb, "-k", "3", "--allparams", "-vb", "0"])
    plain_out = capsys.readouterr().out
    assert "shift kde" not in plain_out and tn.FOOTNOTE_KDE not in plain_out and tn.FOOTNOTE in plain_out
    assert math.isfinite(f["sigma_p"]) and f["ess_eff"] > 100
