"""contours on the device: ``mce_param_contours_dev`` (csrc/param_contours_kernels.hpp) on the cases of tests/contours_cases.py: the
moments and h within their bounds, every density within its bound of the exact product-kernel estimate at the reported h, c, lo and step
(mpmath on the query cells, the extended format on all), every density within two bounds of ``contours.measure``'s, every decision bit
for bit the serial rule's on the device's own densities (NumPy and the sanitized native program) and the oracle's on every decided cell;
the status cases, each between two good systems; a pair asked alone against the same pair among all columns; many systems of several
shapes in one call, each bit for bit its own single call; two runs bit for bit; the host-pointer form; MCEvidence on host arrays; the
resident route, the farm (two distinct specs in one wave) and the command line end to end on small chain files, ln E byte-equal with and
without the keyword.

Measured on one MI355X (error / bound): see docs/design/contours.md."""
import numpy as np
import pytest

import contours_cases as cc

pytestmark = pytest.mark.gpu


def measure(systems, cols, probs=cc.PROBS, grid=64, scale=1.0):
    """ONE mce_param_contours_dev call on device copies of ``systems`` = [(a, x[n, ld], d)] -> one float64 block per system"""
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
    wsb = _capi.param_contours_workspace_bytes(sum(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(cols), len(probs), grid)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_contours_dev(segs, cols, probs, grid, scale, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def sys_of(c):
    return (c.a, c.x, c.d)


def as_dict(block, c):
    from mcevidence_amd import contours
    return contours.from_block(block, c.nc, len(c.probs), c.grid)


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {name: measure([sys_of(c)], c.cols, c.probs, c.grid, c.scale)[0] for name, c in cc.cases().items()}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cc.build_checker(tmp_path_factory.mktemp("param_contours_gpu"))


@pytest.mark.parametrize("name", list(cc.cases()))
def test_device_against_the_oracle(name, singles, checker, tmp_path):
    c = cc.cases()[name]
    got = as_dict(singles[name], c)
    good = cc.check_moments(c, got, "device")
    assert len(good) == c.nc
    stats = {}
    for p, s, t in cc.oracle_pairs(c):
        cc.check_pair(c, got, p, s, t, "device", stats=stats)
    # ALL densities against the NumPy form's, within two bounds; ALL decisions bit for bit the serial rule's on the device's own densities
    cc.check_against_numpy(c, got, "device")
    assert cc.check_decisions_native(checker, tmp_path, [got], c.probs, c.grid) == c.nc * (c.nc - 1) // 2
    assert stats["undecided"] <= cc.MAX_UNDECIDED


def test_status_cases_fail_alone(singles):
    from mcevidence_amd import contours
    good = cc.cases()["n16_nc2_G32_unit"]
    for name, a, x, status, column in cc.status_cases():
        got = measure([sys_of(good), (a, x, x.shape[1]), sys_of(good)], good.cols, good.probs, good.grid)
        assert got[0].tobytes() == singles[good.name].tobytes() == got[2].tobytes(), name
        bad = contours.from_block(got[1], 2, len(good.probs), good.grid)
        cc.assert_failed_system(bad, status, column, int(np.count_nonzero(a != 0)), name)
        assert np.array_equal(bad["col"], [0.0, 1.0])
        assert measure([(a, x, x.shape[1])], good.cols, good.probs, good.grid)[0].tobytes() == got[1].tobytes(), name


def test_a_constant_column_fails_its_pairs_alone():
    from mcevidence_amd import contours
    c = cc.constant_column_case()
    good = cc.cases()["n5_nc3_G32_integer"]
    first, mid, last = measure([sys_of(good), sys_of(c), sys_of(good)], c.cols, c.probs, c.grid)
    assert first.tobytes() == last.tobytes() == measure([sys_of(good)], good.cols, good.probs, good.grid)[0].tobytes()
    got = contours.from_block(mid, 3, len(c.probs), c.grid)
    assert list(got["col_status"]) == [0.0, 7.0, 0.0] and list(got["pair_status"]) == [7.0, 0.0, 7.0]
    cc.assert_failed_pair(got, 0)
    cc.assert_failed_pair(got, 2)
    alone = contours.from_block(measure([sys_of(c)], (0, 2), c.probs, c.grid)[0], 2, len(c.probs), c.grid)
    assert got["density"][1].tobytes() == alone["density"][0].tobytes() and np.array_equal(got["level"][:, 1], alone["level"][:, 0])


def test_a_pair_alone_among_all_columns_and_in_another_probs(singles):
    from mcevidence_amd import contours
    g = cc.cases()
    for name, pair in (("n15_nc6_G64_fractional", (0, 5)), ("n1025_nc6_G64_fractional", (1, 4)), ("n513_nc27_G64_integer", (7, 22)), ("n511_nc6_G32_unit", (2, 3))):
        c = g[name]
        whole = as_dict(singles[name], c)
        probs = (0.1, 0.3, 0.5, 0.68, 0.9, 0.95, 0.99)
        alone = contours.from_block(measure([sys_of(c)], pair, probs, c.grid)[0], 2, 7, c.grid)
        p = contours.pairs(c.nc).index(pair)
        assert whole["density"][p].tobytes() == alone["density"][0].tobytes(), name
        assert (whole["mode_x"][p], whole["mode_y"][p], whole["mode_density"][p]) == (alone["mode_x"][0], alone["mode_y"][0], alone["mode_density"][0])
        for k in contours.P_KEYS:
            assert whole[k][0][p] == alone[k][3][0] and whole[k][1][p] == alone[k][5][0], (name, k)
        assert np.all(np.diff(alone["cells"][:, 0]) >= 0.0) and np.all(np.diff(alone["level"][:, 0]) <= 0.0)


def test_many_systems_of_several_shapes_in_three_orders():
    # cols (0, 1) of systems with (n, d, ld): (3, 3, 5), (17, 3, 5), (513, 127, 129), (1025, 6, 8), (8705, 3, 5) and an empty one
    g = cc.cases()
    names = ["n3_nc3_G64_fractional", "n17_nc3_G64_integer", "n513_d127_last_two", "n1025_nc6_G64_fractional", "n8705_nc3_G32_fractional"]
    own = [measure([sys_of(g[n])], (0, 1))[0] for n in names]
    empty = (np.zeros(0), np.zeros((0, 3)), 3)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        systems = [sys_of(g[names[i]]) for i in order]
        systems.insert(2, empty)
        got = measure(systems, (0, 1))
        assert got[2][3] == 5 and got[2][2] == 0           # the empty segment: status 5, no rows
        del got[2]
        for i, block in zip(order, got):
            assert block.tobytes() == own[i].tobytes(), (order, names[i])


def test_two_runs_and_the_host_pointer_form(singles):
    from mcevidence_amd import _capi
    g = cc.cases()
    for name in ("n2_nc2_G32_integer", "n513_nc27_G64_integer", "n8193_nc2_G64_unit", "scale_half"):
        c = g[name]
        assert measure([sys_of(c)], c.cols, c.probs, c.grid, c.scale)[0].tobytes() == singles[name].tobytes(), name
    cases = [g[n] for n in ("n3_nc3_G64_fractional", "n17_nc3_G64_integer", "n512_nc3_G64_fractional")]
    host = _capi.param_contours([(c.x, c.d, c.a) for c in cases] + [(np.zeros((0, 3)), 3, np.zeros(0))], (0, 1, 2), cc.PROBS, 64, 1.0)
    for c, block in zip(cases, host):
        assert np.array(block).tobytes() == singles[c.name].tobytes(), c.name
    assert host[3][3] == 5


def test_mcevidence_on_host_arrays_uses_the_library():
    import mcevidence_amd as pkg
    from mcevidence_amd import contours
    from mcevidence_amd.synth import gaussian_chain
    chain = gaussian_chain(seed=7, n=3000, d=4, weights="int")
    kw = dict(kmax=2, verbose=0, ndim=4)
    spec = {"probs": (0.68,), "grid": 32, "params": [0, 2, 3]}
    obj = pkg.MCEvidence([chain], contours=spec, **kw)
    lnE, info = obj.evidence(info=True)
    m = info["contours"]
    assert obj.param_contours is m and m["cols"] == [0, 2, 3] and m["pairs"] == [(0, 2), (0, 3), (2, 3)] and m["density"].shape == (3, 32, 32)
    assert m["status"] == 0 and np.all(m["pair_status"] == 0) and np.all(m["cells"] > 0)
    part = obj.gd.data["s1"]
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)
    blk = contours.measure_native(a, x, (0, 2, 3), (0.68,), 32)
    assert np.array_equal(blk["density"], m["density"]) and np.array_equal(blk["level"], m["level"])
    lnE0, info0 = pkg.MCEvidence([chain], **kw).evidence(info=True)
    assert np.array_equal(lnE, lnE0) and "contours" not in info0


def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, tuple, str)))
        for k in a)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("contours_roots")
    out = {}
    for name, seed, rows, nnuis in (("p9", 43, (900, 1000, 950), 3), ("p9b", 45, (800, 850, 700), 3), ("bad", 44, (700, 650, 720), 3)):
        out[name] = str(d / name)
        chains, names, _ = planck_like_chains(seed=seed, rows=rows, nnuis=nnuis)
        if name == "bad":
            chains = [np.array(c) for c in chains]
            chains[1][100, 0] = -2.0                       # a negative weight: allowed in the estimator, status 3 here
        write_cosmomc_chains(out[name], chains, None, fmt="%.17g")
        if name == "p9":
            with open(out[name] + ".paramnames", "w") as fh:
                fh.write("".join("%s\t%s\n" % (n, n.upper()) for n in names))
    return out


@pytest.mark.parametrize("thin", [0, 3])
def test_resident_route_with_contours(roots, thin):
    import mcevidence_amd as pkg
    root = roots["p9"]
    kw = dict(kmax=3, verbose=0, thinlen=thin)
    spec = {"probs": (0.68, 0.95), "grid": 32, "params": [0, 1, 4]}
    lnE, info = pkg.evidence_from_files(root, contours=spec, info=True, require_resident=True, **kw)
    host = pkg.MCEvidence(root, contours=spec, **kw)          # (the HIP backend: its contours are mce_param_contours_f64's)
    hostE, hinfo = host.evidence(info=True)
    part = host.gd.data["s1"]
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)
    case = cc.Case("resident thin=%s" % thin, a, x, x.shape[1], (0, 1, 4), grid=32)
    d, h = info["contours"], hinfo["contours"]
    for what, m in (("resident", d), ("host    ", h)):
        blk = dict(m, W=m["sum_w"], A2=m["sum_w"] ** 2 / m["ess"], lo=m["grid_lo"], step=m["grid_step"], var=m["sd"] ** 2, nc=3, col=np.array(m["cols"], dtype=np.float64))
        assert m["status"] == 0 and np.all(m["pair_status"] == 0) and (m["probs"], m["grid"], m["scale"], m["cols"]) == ((0.68, 0.95), 32, 1.0, [0, 1, 4])
        cc.check_pair(case, blk, 1, 0, 2, what)
        cc.check_against_numpy(case, blk, what)
        assert len(m["names"]) == 3 and not any("sigma" in k for k in m)
    # the two device forms see the same rows: bit for bit one another
    assert same_dict(d, h)
    assert info["route"] == "resident"
    # ln E is bit for bit what the route returns without the keyword
    lnE0, info0 = pkg.evidence_from_files(root, info=True, require_resident=True, **kw)
    untimed = lambda inf: {k: ({j: u for j, u in v.items() if j != "kernel_ms"} if isinstance(v, dict) else v) for k, v in inf.items() if k != "contours"}      # noqa: E731
    assert np.array_equal(lnE, lnE0) and "contours" not in info0 and same_dict(untimed(info), untimed(info0))
    # names choose the same columns
    names = d["names"]
    byname = pkg.evidence_from_files(root, contours=dict(spec, params=[names[2], names[0], names[1]]), info=True, require_resident=True, **kw)[1]["contours"]
    assert same_dict(byname, d)


def test_farm_measures_every_root_as_its_own_resident_run(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p9", "bad", "p9b", "p9"]
    thins = [0, 0, 0, 3]
    # two distinct specs in one wave, a root whose status is 3, a thinned root
    specs = [{"grid": 32, "params": [0, 1, 2]}, {"grid": 32, "params": [0, 1, 2]}, {"probs": (0.9,), "params": [1, 3]}, {"grid": 32, "params": [0, 1, 2]}]
    outs = pkg.evidence_many_from_files([roots[n] for n in names], contours=specs, thinlen=thins, kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 4 and farm.LAST_STATS["counts"]["farm"] == 4
    for n, t, sp, (lnE, info) in zip(names, thins, specs, outs):
        own = pkg.evidence_from_files(roots[n], contours=sp, thinlen=t, kmax=3, verbose=0, info=True, require_resident=True)
        assert same_dict(info["contours"], own[1]["contours"]), n
        assert np.array_equal(lnE, own[0]), n
        assert info["contours"]["status"] == (3 if n == "bad" else 0), n
    bad = outs[1][1]["contours"]
    assert np.isnan(bad["density"]).all() and np.isnan(bad["level"]).all() and bad["column"] == -1 and np.all(np.isfinite(outs[1][0]))
    assert outs[2][1]["contours"]["density"].shape == (1, 64, 64) and outs[2][1]["contours"]["probs"] == (0.9,)
    plain = pkg.evidence_many_from_files([roots[n] for n in names], thinlen=thins, kmax=3, info=True)
    for a, p in zip(outs, plain):
        assert np.array_equal(a[0], p[0]) and "contours" not in p[1]
    # a root whose params do not fit fails alone, with the ValueError of contours.spec; a root that does not ask is left alone
    mixed = pkg.evidence_many_from_files([roots["p9"], roots["p9b"], roots["p9"]], contours=[{"params": [0, 99]}, None, True], marginals={"grid": 64}, kmax=3, info=True,
                                         return_exceptions=True)
    assert isinstance(mixed[0], ValueError) and "contours=" in str(mixed[0]) and "contours" not in mixed[1][1] and "marginals" in mixed[1][1]
    assert mixed[2][1]["contours"]["density"].shape == (36, 64, 64) and "marginals" in mixed[2][1]


def test_command_line_on_the_resident_route_and_the_farm(tmp_path, capsys, caplog):
    import logging

    from mcevidence_amd import cli
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=600, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    npz = str(tmp_path / "res.npz")
    args = [root, "-k", "3", "--allparams", "--resident", "--marginals", "--marginals-grid", "64", "--contours", "--contours-grid", "32", "--contours-out", npz, "--jackknife=4"]
    # -vb 0: the CLI prints the lines once, after the marginals lines and before the ln(B) lines it prints
    cli.main(args + ["-vb", "0"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    keys = {"mar": ["marginals:", "p2"], "head": ["contours:", "x", "y"], "first": ["contours:", "p0", "p1"], "last": ["contours:", "p1", "p2"], "lnb": ["ln(B)[k=1]", "="]}
    at = {k: [i for i, ln in enumerate(out) if ln.split()[:len(v)] == v] for k, v in keys.items()}
    assert all(len(v) == 1 for v in at.values()), (at, out)
    assert at["mar"][0] < at["head"][0] < at["first"][0] < at["last"][0] < at["lnb"][0]
    z = np.load(npz)
    assert list(z["roots"]) == [root] and z["density_0"].shape == (3, 32, 32) and z["grid_x_0"].shape == z["grid_y_0"].shape == (3, 32) and np.all(z["density_0"] >= 0.0)
    cell = (z["grid_x_0"][:, 1] - z["grid_x_0"][:, 0]) * (z["grid_y_0"][:, 1] - z["grid_y_0"][:, 0])
    assert np.all(np.abs(z["density_0"].sum(axis=(1, 2)) * cell - 1.0) < 1e-2) and z["levels_0"].shape == (2, 3) and z["pairs_0"].tolist() == [[0, 1], [0, 2], [1, 2]]
    # -vb 1: the route logs them, the CLI does not print them a second time
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    msgs = [r.getMessage().strip() for r in caplog.records]
    assert not any(ln.startswith("contours:") for ln in printed) and sum(m.startswith("contours: x") for m in msgs) == 1
    assert max(i for i, m in enumerate(msgs) if m.startswith("marginals:")) < min(i for i, m in enumerate(msgs) if m.startswith("contours:"))
    # the farm prints them for every root and writes one set per root
    lst = tmp_path / "roots.txt"
    lst.write_text("%s\n%s   # twice\n" % (root, root))
    npz2 = str(tmp_path / "farm.npz")
    cli.main([str(lst), "-k", "3", "--allparams", "--farm", "--contours", "0.9", "--contours-params", "0", "2", "--contours-out", npz2, "-vb", "0"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert sum(ln.startswith("contours: x") for ln in out) == 2 and sum(ln.startswith("contours: p0") for ln in out) == 2 and sum(ln.startswith("ln(B)[k=1] =") for ln in out) == 2
    assert all("level90" in ln for ln in out if ln.startswith("contours: x"))
    assert max(i for i, ln in enumerate(out) if ln.startswith("contours:")) < max(i for i, ln in enumerate(out) if ln.startswith("ln(B)[k=1] ="))
    z2 = np.load(npz2)
    assert list(z2["roots"]) == [root, root] and z2["density_1"].shape == (1, 64, 64) and np.array_equal(z2["density_0"], z2["density_1"]) and z2["pairs_0"].tolist() == [[0, 2]]
