"""marginals on the device: ``mce_param_marginals_dev`` (csrc/param_marginals_kernels.hpp) on the cases of tests/marginals_cases.py: the
moments and h within their bounds, every density within its bound of the exact kernel estimate at the reported h, c, lo and step (mpmath
on the query points, the extended format on all), every density within two bounds of ``marginals.measure``'s, every decision bit for bit
the serial rule's on the device's own densities (NumPy and the sanitized native program) and the oracle's on every decided grid point;
the status cases, each between two good systems; many systems of several shapes in one call, each bit for bit its own single call whatever
its neighbours and its place; two runs bit for bit; the host-pointer form; the resident route, the farm and the command line.

Measured on one MI355X (error / bound): see docs/design/marginals.md."""
import numpy as np
import pytest

import marginals_cases as mc

pytestmark = pytest.mark.gpu


def measure(systems, probs=mc.PROBS, grid=512, scale=1.0):
    """ONE mce_param_marginals_dev call on device copies of ``systems`` = [(a, x[n, ld], d)] -> one float64 block per system"""
    import torch
    from mcevidence_amd import _capi
    keep, segs = [], []
    for a, x, d in systems:
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x if x.ndim == 2 else x.reshape(len(a), -1)
        t = [torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0") for v in (x, a)]
        keep.append(t)
        n = len(a)
        segs.append((t[0].data_ptr() if n else 0, x.shape[1], n, d, t[1].data_ptr() if n else 0))
    wsb = _capi.param_marginals_workspace_bytes(sum(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(probs), grid)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_marginals_dev(segs, probs, grid, scale, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def sys_of(c):
    return (c.a, c.x, c.d)


def as_dict(block, c):
    from mcevidence_amd import marginals
    return marginals.from_block(block, c.d, len(c.probs), c.grid)


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {name: measure([sys_of(c)], c.probs, c.grid, c.scale)[0] for name, c in mc.cases().items()}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return mc.build_checker(tmp_path_factory.mktemp("param_marginals_gpu"))


@pytest.mark.parametrize("name", list(mc.cases()))
def test_device_against_the_oracle(name, singles, checker, tmp_path):
    from mcevidence_amd import marginals
    c = mc.cases()[name]
    got = as_dict(singles[name], c)
    good = mc.check_moments(c, got, "device")
    stats = {}
    for j in mc.oracle_columns(c):
        if j in good:
            mc.check_column(c, got, j, "device", stats=stats)
    for j in sorted(set(range(c.d)) - set(good)):
        mc.assert_failed_column(got, j, name)
    # ALL densities against the NumPy form's, within two bounds; ALL decisions bit for bit the serial rule's on the device's own densities
    mc.check_against_numpy(c, got, "device")
    for j in good:
        mode, md, lower, upper, pieces, edge = marginals.decide(got["density"][j], got["lo"][j], got["step"][j], c.probs)
        assert (got["mode"][j], got["mode_density"][j]) == (mode, md), (name, j)
        for k, v in (("lower", lower), ("upper", upper), ("pieces", pieces), ("edge", edge)):
            assert np.array_equal(got[k][:, j], v), (name, j, k)
    assert mc.check_decisions_native(checker, tmp_path, [got], c.probs, c.grid) == len(good)
    if c.d == 8 and c.n >= 400:
        assert sorted(set(range(c.d)) - set(good)) == [2, 3]
    if name == "n4100_d8_G512_fractional":
        assert np.count_nonzero(got["density"][5] == 0.0) > c.grid // 2      # exact zeros by the 746 rule, ties by the lowest k
    assert stats["undecided"] <= mc.MAX_UNDECIDED


def test_status_cases_fail_alone(singles):
    from mcevidence_amd import marginals
    good = mc.cases()["n513_d127_G512_fractional"]
    for name, a, x, status, column in mc.status_cases():
        got = measure([sys_of(good), (a, x, x.shape[1]), sys_of(good)], good.probs, good.grid)
        assert got[0].tobytes() == singles[good.name].tobytes() == got[2].tobytes(), name
        bad = marginals.from_block(got[1], x.shape[1], len(good.probs), good.grid)
        mc.assert_failed_system(bad, x.shape[1], status, column, int(np.count_nonzero(a != 0)), name)
        assert measure([(a, x, x.shape[1])], good.probs, good.grid)[0].tobytes() == got[1].tobytes(), name


def test_five_systems_of_three_shapes_in_three_orders(singles):
    # one grid per call: the cases with G = 512; (d, ld): (8, 10), (1, 3), (127, 129), (8, 10), (1, 3)
    names = ["n3_d8_G512_fractional", "n65_d1_G512_fractional", "n513_d127_G512_fractional", "n4100_d8_G512_fractional", "n512_d1_G512_integer"]
    g = mc.cases()
    assert all(g[n].grid == 512 and g[n].scale == 1.0 for n in names)
    empty = (np.zeros(0), np.zeros((0, 3)), 3)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        systems = [sys_of(g[names[i]]) for i in order]
        systems.insert(2, empty)
        got = measure(systems)
        assert got[2][3] == 5 and got[2][2] == 0           # the empty segment: status 5, no rows
        del got[2]
        for i, block in zip(order, got):
            assert block.tobytes() == singles[names[i]].tobytes(), (order, names[i])


def test_two_runs_and_the_host_pointer_form(singles):
    from mcevidence_amd import _capi
    g = mc.cases()
    for name in ("n512_d1_G512_integer", "n4100_d27_G64_unit", "n33300_d1_G64_integer", "scale_quarter"):
        c = g[name]
        assert measure([sys_of(c)], c.probs, c.grid, c.scale)[0].tobytes() == singles[name].tobytes(), name
    cases = [g[n] for n in ("n511_d8_G1024_unit", "n1025_d27_G1024_integer", "n63_d1_G1024_unit")]
    host = _capi.param_marginals([c.system for c in cases] + [(np.zeros((0, 2)), 2, np.zeros(0))], mc.PROBS, 1024, 1.0)
    for c, block in zip(cases, host):
        assert np.array(block).tobytes() == singles[c.name].tobytes(), c.name
    assert host[3][3] == 5
    # other probabilities leave the densities alone
    c = g["n64_d8_G64_integer"]
    seven = as_dict(measure([sys_of(c)], (0.1, 0.3, 0.5, 0.68, 0.9, 0.95, 0.99), c.grid)[0], mc.Case(c.name, c.a, c.x, c.d, c.grid, probs=(0.1,) * 7))
    ref = as_dict(singles[c.name], c)
    assert np.array_equal(seven["density"], ref["density"]) and np.array_equal(seven["lower"][3], ref["lower"][0]) and np.array_equal(seven["pieces"][5], ref["pieces"][1])
    assert np.all(np.diff(seven["upper"] - seven["lower"], axis=0) >= 0.0)


def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, tuple, str)))
        for k in a)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("marginals_roots")
    out = {}
    for name, seed, rows, nnuis in (("p21", 41, (1500, 1400, 1450, 1300), 15), ("p21b", 42, (1200, 1250, 1100, 1300), 15), ("p9", 43, (900, 1000, 950), 3),
                                    ("bad", 44, (700, 650, 720), 3)):
        out[name] = str(d / name)
        chains, names, _ = planck_like_chains(seed=seed, rows=rows, nnuis=nnuis)
        if name == "bad":
            chains = [np.array(c) for c in chains]
            chains[1][100, 0] = -2.0                       # a negative weight: allowed in the estimator, status 3 here
        write_cosmomc_chains(out[name], chains, None, fmt="%.17g")
        if name == "p21":
            with open(out[name] + ".paramnames", "w") as fh:
                fh.write("".join("%s\t%s\n" % (n, n.upper()) for n in names))
    return out


@pytest.mark.parametrize("thin", [0, 3])
@pytest.mark.parametrize("jackknife", [None, 4])
def test_resident_route_with_marginals(roots, thin, jackknife):
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import PLANCK_PARAMS
    root = roots["p21"]
    kw = dict(kmax=3, verbose=0, thinlen=thin, **({} if jackknife is None else {"jackknife": jackknife}))
    spec = {"probs": (0.68, 0.95), "grid": 128}
    lnE, info = pkg.evidence_from_files(root, marginals=spec, info=True, require_resident=True, **kw)
    host = pkg.MCEvidence(root, marginals=spec, **kw)          # (the HIP backend: its marginals are mce_param_marginals_f64's)
    hostE, hinfo = host.evidence(info=True)
    part = host.gd.data["s1"]
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)
    case = mc.Case("resident thin=%s jackknife=%s" % (thin, jackknife), a, x, grid=128)
    d, h = info["marginals"], hinfo["marginals"]
    for what, m in (("resident", d), ("host    ", h)):
        blk = dict(m, W=m["sum_w"], A2=m["sum_w"] ** 2 / m["ess"], lo=m["grid_lo"], step=m["grid_step"], var=m["sd"] ** 2)
        assert m["status"] == 0 and np.all(m["col_status"] == 0) and (m["probs"], m["grid"], m["scale"]) == ((0.68, 0.95), 128, 1.0)
        for j in (0, x.shape[1] - 1):
            mc.check_column(case, blk, j, what)
        assert m["names"][:3] == [p[0] for p in PLANCK_PARAMS][:3] and len(m["names"]) == x.shape[1] and not any("sigma" in k for k in m)
    # the two device forms see the same rows: bit for bit one another
    assert same_dict(d, h)
    mc.check_against_numpy(case, dict(d, lo=d["grid_lo"], step=d["grid_step"]), "resident")
    assert info["route"] == "resident" and ("jackknife" in info) == (jackknife is not None)
    # ln E is bit for bit what the route returns without the keyword
    lnE0, info0 = pkg.evidence_from_files(root, info=True, require_resident=True, **kw)
    untimed = lambda inf: {k: ({j: u for j, u in v.items() if j != "kernel_ms"} if isinstance(v, dict) else v) for k, v in inf.items() if k != "marginals"}      # noqa: E731
    assert np.array_equal(lnE, lnE0) and "marginals" not in info0 and same_dict(untimed(info), untimed(info0))


def test_farm_measures_every_root_as_its_own_resident_run(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p21", "p9", "bad", "p21b", "p21"]           # two (ncols, ndim) shapes, a root whose status is 3, a thinned root
    thins = [0, 0, 0, 0, 3]
    outs = pkg.evidence_many_from_files([roots[n] for n in names], marginals={"grid": 64}, thinlen=thins, kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 5 and farm.LAST_STATS["counts"]["farm"] == 5
    for n, t, (lnE, info) in zip(names, thins, outs):
        own = pkg.evidence_from_files(roots[n], marginals={"grid": 64}, thinlen=t, kmax=3, verbose=0, info=True, require_resident=True)
        assert same_dict(info["marginals"], own[1]["marginals"]), n
        assert np.array_equal(lnE, own[0]), n
        assert info["marginals"]["status"] == (3 if n == "bad" else 0), n
    bad = outs[2][1]["marginals"]
    assert np.isnan(bad["density"]).all() and np.isnan(bad["upper"]).all() and bad["column"] == -1 and np.all(np.isfinite(outs[2][0]))
    plain = pkg.evidence_many_from_files([roots[n] for n in names], thinlen=thins, kmax=3, info=True)
    for a, p in zip(outs, plain):
        assert np.array_equal(a[0], p[0]) and "marginals" not in p[1]
    # one entry per root: two specs are two calls, a root that does not ask is left alone; together with summary
    mixed = pkg.evidence_many_from_files([roots["p21"], roots["p9"], roots["p21b"]], marginals=[(0.9,), None, {"grid": 64}], summary=True, kmax=3, info=True)
    assert mixed[0][1]["marginals"]["probs"] == (0.9,) and mixed[0][1]["marginals"]["density"].shape == (21, 512) and "marginals" not in mixed[1][1]
    assert same_dict(mixed[2][1]["marginals"], outs[3][1]["marginals"]) and all("summary" in m[1] for m in mixed)


def test_command_line_on_the_resident_route_and_the_farm(tmp_path, capsys, caplog):
    import logging

    from mcevidence_amd import cli
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=600, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    npz = str(tmp_path / "res.npz")
    args = [root, "-k", "3", "--allparams", "--resident", "--summary", "--marginals", "--marginals-grid", "64", "--marginals-out", npz, "--jackknife=4"]
    # -vb 0: the CLI prints the lines once, after the summary lines and before the ln(B) lines it prints
    cli.main(args + ["-vb", "0"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    at = {key: [i for i, ln in enumerate(out) if ln.startswith(key)] for key in ("summary: p2", "marginals: parameter", "marginals: p0", "marginals: p2", "ln(B)[k=1] =")}
    assert all(len(v) == 1 for v in at.values()), (at, out)
    assert at["summary: p2"][0] < at["marginals: parameter"][0] < at["marginals: p0"][0] < at["marginals: p2"][0] < at["ln(B)[k=1] ="][0]
    z = np.load(npz)
    assert list(z["roots"]) == [root] and z["density_0"].shape == z["grid_0"].shape == (3, 64) and np.all(z["density_0"] >= 0.0)
    assert np.all(np.abs(z["density_0"].sum(axis=1) * (z["grid_0"][:, 1] - z["grid_0"][:, 0]) - 1.0) < 5e-3)
    # -vb 1: the route logs them, the CLI does not print them a second time
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    msgs = [r.getMessage().strip() for r in caplog.records]
    assert not any(ln.startswith("marginals:") for ln in printed) and sum(m.startswith("marginals: parameter") for m in msgs) == 1
    assert max(i for i, m in enumerate(msgs) if m.startswith("summary:")) < min(i for i, m in enumerate(msgs) if m.startswith("marginals:"))
    # the farm prints them for every root and writes one set per root
    lst = tmp_path / "roots.txt"
    lst.write_text("%s\n%s   # twice\n" % (root, root))
    npz2 = str(tmp_path / "farm.npz")
    cli.main([str(lst), "-k", "3", "--allparams", "--farm", "--marginals", "0.9", "--marginals-out", npz2, "-vb", "0"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert sum(ln.startswith("marginals: parameter") for ln in out) == 2 and sum(ln.startswith("ln(B)[k=1] =") for ln in out) == 2
    assert all("lower90" in ln for ln in out if ln.startswith("marginals: parameter"))
    assert max(i for i, ln in enumerate(out) if ln.startswith("marginals:")) < max(i for i, ln in enumerate(out) if ln.startswith("ln(B)[k=1] ="))
    z2 = np.load(npz2)
    assert list(z2["roots"]) == [root, root] and z2["density_1"].shape == (3, 512) and np.array_equal(z2["density_0"], z2["density_1"])
