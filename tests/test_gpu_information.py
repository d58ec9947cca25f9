"""information on the device: ``mce_like_moments_dev`` (csrc/like_moments_kernels.hpp) on every case of tests/moments_cases.py against
the exact rational model, within the bound derived in docs/design/information.md; the status cases, each next to a good system; many
systems in one call, each bit for bit its own single call whatever its neighbours and its place; two runs bit for bit; the
host-pointer form; the resident route and the farm with ``information``.

Measured on one MI355X (error / bound): see docs/design/information.md."""
import math

import numpy as np
import pytest

import moments_cases as mc

pytestmark = pytest.mark.gpu


def measure(systems):
    """ONE mce_like_moments_dev call on device copies of ``systems`` = [(a, f)] -> float64 [nseg, 6]"""
    import torch
    from mcevidence_amd import _capi
    keep = [(torch.from_numpy(np.array(f, dtype=np.float64)).to("cuda:0"), torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda:0")) for a, f in systems]
    segs = [(f.data_ptr() if f.shape[0] else 0, w.data_ptr() if w.shape[0] else 0, int(f.shape[0])) for f, w in keep]
    wsb = _capi.like_moments_workspace_bytes(sum(n for _, _, n in segs), len(segs))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.like_moments_dev(segs, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {c.name: measure([(c.a, c.f)])[0] for c in mc.CASES}


def as_dict(block):
    from mcevidence_amd import information
    return information.from_block(block)


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_device_equals_the_exact_model(name, singles):
    # A: unit weights; B: the tile edges; C: a second pass that must be centred; D: zero weights over -inf and NaN; E: a negative weight
    mc.check(mc.BY_NAME[name], as_dict(singles[name]), "device")


def test_status_cases_fail_alone(singles):
    good = mc.BY_NAME["B_513"]
    for name, a, f, status in mc.status_cases():
        got = measure([(good.a, good.f), (a, f), (good.a, good.f)])
        assert got[0].tobytes() == singles["B_513"].tobytes() == got[2].tobytes(), name
        bad = as_dict(got[1])
        assert bad["status"] == status and bad["rows"] == int(np.count_nonzero(a != 0)), (name, bad)
        assert all(math.isnan(bad[k]) for k in ("W", "c", "v", "A2")), (name, bad)
        assert measure([(a, f)])[0].tobytes() == got[1].tobytes(), name


def test_five_systems_in_three_orders(singles):
    names = ["A_unit", "B_1025", "D_zeros", "E_negative", "L_4100"]
    empty = (np.zeros(0), np.zeros(0))
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        systems = [(mc.BY_NAME[names[i]].a, mc.BY_NAME[names[i]].f) for i in order]
        systems.insert(2, empty)
        got = np.delete(measure(systems), 2, axis=0)
        for i, block in zip(order, got):
            assert block.tobytes() == singles[names[i]].tobytes(), (order, names[i])


def test_two_runs_and_the_host_pointer_form(singles):
    from mcevidence_amd import _capi
    for name in ("B_512", "C_narrow", "L_4100"):
        c = mc.BY_NAME[name]
        assert measure([(c.a, c.f)])[0].tobytes() == singles[name].tobytes(), name
    cases = [mc.BY_NAME[n] for n in ("A_unit", "B_513", "D_zeros")]
    host = _capi.like_moments([(c.f, c.a) for c in cases] + [(np.zeros(0), np.zeros(0))])
    for c, block in zip(cases, host):
        assert block.tobytes() == singles[c.name].tobytes(), c.name
    assert as_dict(host[3])["status"] == 5


def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("information_roots")
    out = {}
    for name, seed, rows, nnuis in (("p21", 41, (1500, 1400, 1450, 1300), 15), ("p21b", 42, (1200, 1250, 1100, 1300), 15), ("p9", 43, (900, 1000, 950), 3),
                                    ("bad", 44, (700, 650, 720), 3)):
        out[name] = str(d / name)
        chains = planck_like_chains(seed=seed, rows=rows, nnuis=nnuis)[0]
        if name == "bad":
            chains = [np.array(c) for c in chains]
            chains[1][100, 1] = np.inf                     # -ln L = +inf on a row with weight: status 3; the estimator adds exp(-inf) = 0
        write_cosmomc_chains(out[name], chains, None, fmt="%.17g")
    return out


def test_resident_route_with_information(roots):
    import mcevidence_amd as pkg
    root = roots["p21"]
    rows = np.concatenate([np.loadtxt(root + "_%d.txt" % i) for i in (1, 2, 3, 4)])
    lnE, info = pkg.evidence_from_files(root, information=True, kmax=3, verbose=0, info=True, require_resident=True)
    hostE, hinfo = pkg.MCEvidence(root, information=True, kmax=3, verbose=0).evidence(info=True)
    a, logL = rows[:, 0], -rows[:, 1]
    ex = mc.exact(a, logL - logL.max())
    b = mc.bounds(ex)
    for what, d, E in (("resident", info["information"], lnE), ("host", hinfo["information"], hostE)):
        err = {"mean_logL": abs(d["mean_logL"] - (logL.max() + ex["c"])) / (b["c"] + mc.EPS * abs(logL.max() + ex["c"])), "var_logL": abs(d["var_logL"] - ex["v"]) / b["v"],
               "bmd": abs(d["bmd"] - 2 * ex["v"]) / (2 * b["v"]), "ess": abs(d["ess"] - ex["ess"]) / b["ess"]}
        print("%s n=%d error/bound: %s" % (what, ex["rows"], "  ".join("%s %.3g" % kv for kv in err.items())))
        assert all(v <= 1.0 for v in err.values()), (what, err)
        assert d["status"] == 0 and d["rows"] == ex["rows"] == len(rows) and d["sum_w"] == ex["W"]
        c = d["mean_logL"] - logL.max()
        assert np.all(np.abs(d["D_KL"] - (d["mean_logL"] - E)) <= 4 * mc.EPS * (abs(logL.max()) + abs(c) + np.abs(E)))
    assert info["route"] == "resident" and info["information"]["D_KL"].shape == (2,)
    # ln E is bit for bit what the route returns without the keyword
    lnE0, info0 = pkg.evidence_from_files(root, kmax=3, verbose=0, info=True, require_resident=True)
    assert np.array_equal(lnE, lnE0) and "information" not in info0 and {k: v for k, v in info.items() if k != "information"} == info0


def test_farm_measures_every_root_as_its_own_resident_run(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p21", "p9", "bad", "p21b", "p21"]           # two (ncols, ndim) shapes, a root whose status is 3, a thinned root
    thins = [0, 0, 0, 0, 3]
    outs = pkg.evidence_many_from_files([roots[n] for n in names], information=True, thinlen=thins, kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 5 and farm.LAST_STATS["counts"]["farm"] == 5
    for n, t, (lnE, info) in zip(names, thins, outs):
        own = pkg.evidence_from_files(roots[n], information=True, thinlen=t, kmax=3, verbose=0, info=True, require_resident=True)
        assert same_dict(info["information"], own[1]["information"]), (n, info["information"], own[1]["information"])
        assert np.array_equal(lnE, own[0]), n
        assert info["information"]["status"] == (3 if n == "bad" else 0), n
    bad = outs[2][1]["information"]
    assert np.isnan(bad["D_KL"]).all() and math.isnan(bad["bmd"]) and np.all(np.isfinite(outs[2][0]))
    # the other roots are unaffected by the failing one; without the keyword ln E keeps its bits
    rest = [i for i in range(5) if i != 2]
    without = pkg.evidence_many_from_files([roots[names[i]] for i in rest], information=True, thinlen=[thins[i] for i in rest], kmax=3, info=True)
    for i, o in zip(rest, without):
        assert same_dict(outs[i][1]["information"], o[1]["information"]) and np.array_equal(outs[i][0], o[0]), names[i]
    plain = pkg.evidence_many_from_files([roots[n] for n in names], thinlen=thins, kmax=3, info=True)
    for a, p in zip(outs, plain):
        assert np.array_equal(a[0], p[0]) and "information" not in p[1]
    mixed = pkg.evidence_many_from_files([roots["p21"], roots["p9"]], information=[True, None], kmax=3, info=True)
    assert "information" in mixed[0][1] and "information" not in mixed[1][1]
