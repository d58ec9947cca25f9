"""marginals with bounds on the device: ``mce_param_marginals_bounded_dev`` (csrc/param_marginals_kernels.hpp, <true>) on the cases of
tests/marginals_bounds_cases.py: the moments and h within their bounds, every density within its bound of the exact boundary-kernel
estimate at the reported h, c, lo and step (mpmath on the query points, the extended format on all), every density within two bounds of
``marginals.measure_bounded``'s, every decision bit for bit the serial rule's with the end weights on the device's own densities (NumPy and
the sanitized native program) and the oracle's on every decided grid point; a call whose columns are all open, and an open column next to
bounded ones, are ``mce_param_marginals_dev``'s bits; a sample outside its bounds fails its column alone, between two good columns and two
good systems; many systems of several shapes and bounds in one call, each bit for bit its own single call; two runs; the host-pointer
form; the host route, the resident route, the farm, --tension and the command line with ``bounds="ranges"``; without ``bounds`` nothing
moves and the bounded entry points are not called.

Measured on one MI355X (error / bound): see docs/design/marginals_bounds.md."""
import numpy as np
import pytest

import marginals_bounds_cases as bc
import marginals_cases as mc

pytestmark = pytest.mark.gpu
INF = float("inf")


def _device_segs(systems):
    import torch
    keep, segs = [], []
    for s in systems:
        a, x, d = s[0], s[1], s[2]
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x if x.ndim == 2 else x.reshape(len(a), -1)
        t = [torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0") for v in (x, a)]
        keep.append(t)
        n = len(a)
        segs.append((t[0].data_ptr() if n else 0, x.shape[1], n, d, t[1].data_ptr() if n else 0))
    return keep, segs


def measure(systems, probs=bc.PROBS, grid=512, scale=1.0):
    """ONE mce_param_marginals_bounded_dev call on device copies of ``systems`` = [(a, x[n, ld], d, (lo[d], hi[d]))] -> one block each"""
    import torch
    from mcevidence_amd import _capi
    keep, segs = _device_segs(systems)
    wsb = _capi.param_marginals_bounded_workspace_bytes(sum(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(probs), grid)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_marginals_bounded_dev(segs, [s[3] for s in systems], probs, grid, scale, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def measure_plain(systems, probs=bc.PROBS, grid=512, scale=1.0):
    """ONE mce_param_marginals_dev call on the same systems (their bounds are not read)"""
    import torch
    from mcevidence_amd import _capi
    keep, segs = _device_segs(systems)
    wsb = _capi.param_marginals_workspace_bytes(sum(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(probs), grid)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_marginals_dev(segs, probs, grid, scale, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def sys_of(c):
    return (c.a, c.x, c.d, c.bounds)


def as_dict(block, c):
    from mcevidence_amd import marginals
    return marginals.from_block_bounded(block, c.d, len(c.probs), c.grid)


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {name: measure([sys_of(c)], c.probs, c.grid, c.scale)[0] for name, c in bc.cases().items()}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return bc.build_checker(tmp_path_factory.mktemp("param_marginals_bounds_gpu"))


def moments(c, got, what):
    ex = c.exact
    clipped = dict(got)
    clipped["lo"] = np.array([ex["min"][j] - 3.0 * got["h"][j] for j in range(c.d)])
    clipped["step"] = np.array([((ex["max"][j] + 3.0 * got["h"][j]) - clipped["lo"][j]) / float(c.grid - 1) for j in range(c.d)])
    return mc.check_moments(c, clipped, what)


@pytest.mark.parametrize("name", list(bc.cases()))
def test_device_against_the_oracle(name, singles, checker, tmp_path):
    from mcevidence_amd import marginals
    c = bc.cases()[name]
    got = as_dict(singles[name], c)
    assert singles[name][7] == 1.0                              # the head's reserved slot
    good = moments(c, got, "device")
    assert list(good) == list(range(c.d)), (name, got["col_status"])
    stats = {}
    for j in bc.oracle_columns(c):
        bc.check_column(c, got, j, "device", stats=stats)
    bc.check_against_numpy(c, got, "device")
    for j in range(c.d):
        bc.check_grid(c, got, j)
        mode, md, lower, upper, pieces, edge = marginals.decide_bounded(got["density"][j], got["lo"][j], got["step"][j], c.probs, got["at_lo"][j] == 1.0,
                                                                        got["at_hi"][j] == 1.0)
        assert (got["mode"][j], got["mode_density"][j]) == (mode, md), (name, j)
        for k, v in (("lower", lower), ("upper", upper), ("pieces", pieces), ("edge", edge)):
            assert np.array_equal(got[k][:, j], v), (name, j, k)
    assert bc.check_decisions_native(checker, tmp_path, [got], c.probs, c.grid) == c.d
    assert stats["undecided"] <= bc.MAX_UNDECIDED
    print("device %s largest error/bound of a density: %.3g" % (name, stats["density"]))


@pytest.mark.parametrize("name", list(bc.cases()))
def test_open_columns_are_todays_bits(name, singles):
    from mcevidence_amd import marginals
    c = bc.cases()[name]
    o = bc.open_case(c)
    plain = marginals.from_block(measure_plain([sys_of(o)], o.probs, o.grid, o.scale)[0], o.d, len(o.probs), o.grid)
    opened = as_dict(measure([sys_of(o)], o.probs, o.grid, o.scale)[0], o)
    assert bc.equal_common(opened, plain), name
    assert np.all(opened["at_lo"] == 0.0) and np.all(opened["at_hi"] == 0.0) and np.all(opened["bound_lo"] == -INF) and np.all(opened["bound_hi"] == INF)
    open_cols = [j for j in range(c.d) if c.lo[j] == -INF and c.hi[j] == INF]
    if open_cols:
        assert bc.equal_common(as_dict(singles[name], c), plain, cols=open_cols), name


def test_a_sample_outside_fails_its_column_alone_and_the_status_cases(singles):
    from mcevidence_amd import marginals
    c = bc.cases()["n511_d8_G1024_unit"]
    good = bc.cases()["n1025_d8_G1024_integer"]
    lo = c.lo.copy()
    lo[3] = float(np.sort(c.x[c.use, 3])[1])                     # the smallest sample of column 3 lies below its bound
    got = measure([sys_of(good), (c.a, c.x, c.d, (lo, c.hi)), sys_of(good)], c.probs, c.grid)
    assert got[0].tobytes() == singles[good.name].tobytes() == got[2].tobytes()
    bad, ref = as_dict(got[1], c), as_dict(singles[c.name], c)
    assert bad["status"] == 0 and list(bad["col_status"]) == [0, 0, 0, 8, 0, 0, 0, 0] and (bad["bound_lo"][3], bad["bound_hi"][3]) == (lo[3], c.hi[3])
    bc.assert_outside_column(bad, 3)
    assert bc.equal_common(bad, ref, cols=[j for j in range(c.d) if j != 3])
    for k in marginals.BOUND_KEYS:
        assert np.array_equal(np.delete(bad[k], 3), np.delete(ref[k], 3)), k
    # today's 3 / 5 / 6 and 7, each between two good systems
    g512 = bc.cases()["n513_d127_G512_fractional"]
    two = (np.array([-1e9, -INF]), np.array([INF, 1e9]))
    for name, a, x, status, column in mc.status_cases():
        out = measure([sys_of(g512), (a, x, x.shape[1], two), sys_of(g512)], g512.probs, g512.grid)
        assert out[0].tobytes() == singles[g512.name].tobytes() == out[2].tobytes(), name
        failed = marginals.from_block_bounded(out[1], x.shape[1], len(g512.probs), g512.grid)
        mc.assert_failed_system(failed, x.shape[1], status, column, int(np.count_nonzero(a != 0)), name)
        assert all(np.isnan(failed[k]).all() for k in marginals.BOUND_KEYS), name
    x7 = c.x.copy()
    x7[:, 2] = 2.5
    seven = as_dict(measure([(c.a, x7, c.d, (np.where(np.arange(c.d) == 2, -INF, c.lo), np.where(np.arange(c.d) == 2, INF, c.hi)))], c.probs, c.grid)[0], c)
    assert list(seven["col_status"]) == [0, 0, 7, 0, 0, 0, 0, 0] and np.all(seven["pieces"][:, 2] == -1.0) and np.isnan(seven["density"][2]).all()
    assert bc.equal_common(seven, ref, cols=[j for j in range(c.d) if j != 2])


def test_many_systems_two_runs_and_the_host_pointer_form(singles):
    from mcevidence_amd import _capi
    g = bc.cases()
    names = ["n3_d8_G512_fractional", "n512_d1_G512_integer", "n513_d127_G512_fractional", "n1025_d1_G512_unit"]
    assert all(g[n].grid == 512 for n in names)
    empty = (np.zeros(0), np.zeros((0, 3)), 3, (np.array([0.0, -INF, -INF]), np.array([INF, INF, 1.0])))
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        systems = [sys_of(g[names[i]]) for i in order]
        systems.insert(2, empty)
        got = measure(systems)
        assert got[2][3] == 5 and got[2][2] == 0           # the empty segment: status 5, no rows
        del got[2]
        for i, block in zip(order, got):
            assert block.tobytes() == singles[names[i]].tobytes(), (order, names[i])
    for name, c in g.items():                              # two runs
        assert measure([sys_of(c)], c.probs, c.grid, c.scale)[0].tobytes() == singles[name].tobytes(), name
    cases = [g[n] for n in ("n511_d8_G1024_unit", "n1025_d8_G1024_integer")]
    host = _capi.param_marginals_bounded([c.system for c in cases], [c.bounds for c in cases], bc.PROBS, 1024, 1.0)
    for c, block in zip(cases, host):
        assert np.array(block).tobytes() == singles[c.name].tobytes(), c.name
    big = g["n33300_d1_G64_integer"]
    assert np.array(_capi.param_marginals_bounded([big.system], [big.bounds], bc.PROBS, 64, 1.0)[0]).tobytes() == singles[big.name].tobytes()


def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, tuple, str)))
        for k in a)


RANGES = {"p21": {"omegabh2": (0.005, 0.1), "tau": (0.01, 0.8), "ns": (None, None)}}


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """three roots with .ranges and .paramnames: a bound on the second column that cuts its samples' range (the rows below it are
    dropped from the chains first), an upper bound at the third column's largest sample, open sides"""
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("marginals_bounds_roots")
    out = {}
    for name, seed, rows, nnuis in (("a", 61, (1300, 1200, 1250), 3), ("b", 62, (1100, 1150, 1000), 3), ("ab", 63, (1200, 1250, 1100), 3)):
        out[name] = str(d / name)
        chains, names, _ = planck_like_chains(seed=seed, rows=rows, nnuis=nnuis)
        chains = [np.array(c) for c in chains]
        cut = float(np.median(np.concatenate([c[:, 3] for c in chains])))
        chains = [c[c[:, 3] >= cut] for c in chains]           # the second parameter: its posterior is cut at its prior edge
        top = float(max(c[:, 4].max() for c in chains))
        ranges = [(n, -INF, None) for n in names]
        ranges[1] = (names[1], cut, None)
        ranges[2] = (names[2], -INF, top)
        write_cosmomc_chains(out[name], chains, ranges, fmt="%.17g")
        with open(out[name] + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (n, n.upper()) for n in names))
        out[name + "_bounds"] = (names, cut, top)
    return out


def direct_block(host, bounds, spec):
    """the block of a direct bounded call on the rows of a host object"""
    from mcevidence_amd import _capi, marginals
    part = host.gd.data["s1"]
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.ascontiguousarray(np.asarray(part.samples, dtype=np.float64)[:, :host.ndim])
    probs, grid, scale = spec
    blk, = _capi.param_marginals_bounded([(x, x.shape[1], a)], [bounds], probs, grid, scale)
    return marginals.from_block_bounded(blk, x.shape[1], len(probs), grid)


def test_routes_with_bounds_from_the_ranges_file(roots, tmp_path, capsys):
    import mcevidence_amd as pkg
    from mcevidence_amd import cli, marginals, tension
    root = roots["a"]
    names, cut, top = roots["a_bounds"]
    nd = len(names)
    spec = {"probs": (0.68, 0.95), "grid": 128}
    sp = marginals.spec(spec)
    kw = dict(kmax=3, verbose=0)
    host = pkg.MCEvidence(root, marginals=spec, bounds="ranges", **kw)
    hostE, hinfo = host.evidence(info=True)
    lo, hi = marginals.bounds_spec("ranges", names=names[:host.ndim], root=root)
    assert lo[1] == cut and hi[2] == top and np.isinf(lo[0]) and np.isinf(hi[1])
    want = marginals.build(direct_block(host, (lo, hi), sp), sp, names[:host.ndim])
    h = hinfo["marginals"]
    assert same_dict(h, want) and h["at_lo"][1] == 1.0 and h["grid_lo"][1] == cut and h["lower"][0][1] >= cut and h["at_hi"][2] == 1.0
    lnE, info = pkg.evidence_from_files(root, marginals=spec, bounds="ranges", info=True, require_resident=True, **kw)
    assert info["route"] == "resident" and same_dict(info["marginals"], want)
    # the mapping and the sequence
    for form in ({names[1]: (cut, None), names[2]: (None, top)}, [(None, None), (cut, "N"), (-INF, top)] + [None] * (host.ndim - 3)):
        assert same_dict(pkg.evidence_from_files(root, marginals=spec, bounds=form, info=True, require_resident=True, **kw)[1]["marginals"], want)
    # the farm: each root with its own bounds; a root that does not ask for bounds goes through mce_param_marginals_dev
    three = [roots[n] for n in ("a", "b", "ab")]
    outs = pkg.evidence_many_from_files(three, marginals=spec, bounds=["ranges", None, "ranges"], kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 3 and same_dict(outs[0][1]["marginals"], want)
    own_b = pkg.evidence_from_files(roots["b"], marginals=spec, info=True, require_resident=True, **kw)[1]["marginals"]
    own_ab = pkg.evidence_from_files(roots["ab"], marginals=spec, bounds="ranges", info=True, require_resident=True, **kw)[1]["marginals"]
    assert same_dict(outs[1][1]["marginals"], own_b) and "at_lo" not in own_b and same_dict(outs[2][1]["marginals"], own_ab)
    assert own_ab["grid_lo"][1] == roots["ab_bounds"][1]
    # --tension's three runs
    ta, tb, tab, tinfo = tension.evidence_tension(roots["a"], roots["b"], roots["ab"], marginals=spec, bounds="ranges", kmax=3)
    assert same_dict(tinfo["roots"][0]["marginals"], want) and same_dict(tinfo["roots"][2]["marginals"], own_ab)
    # the command line
    npz = str(tmp_path / "res.npz")
    cli.main([root, "-k", "3", "--resident", "--marginals", "--marginals-grid", "128", "--bounds", "--marginals-out", npz, "-vb", "0"])
    z = np.load(npz)
    k = z["density_0"].shape[0]                                  # (the command line counts the parameters by the .ranges file; a column's density is its own)
    assert k >= 3 and np.array_equal(z["density_0"], want["density"][:k]) and np.array_equal(z["bound_lo_0"], lo[:k]) and z["at_lo_0"][1] == 1.0
    cli.main([root, "-k", "3", "--resident", "--marginals", "--marginals-grid", "128", "--bounds", "%s=%r:" % (names[1], cut), "%s=:%r" % (names[2], top),
              "--marginals-out", npz, "-vb", "0"])
    assert np.array_equal(np.load(npz)["density_0"], want["density"][:k])
    capsys.readouterr()
    # a name that is not a parameter: the ValueError of every route
    with pytest.raises(ValueError, match="^bounds=.*not among"):
        pkg.evidence_from_files(root, marginals=spec, bounds={"zz": (0, 1)}, info=True, require_resident=True, **kw)
    with pytest.raises(ValueError, match="^bounds=.*not among"):
        pkg.evidence_many_from_files([root], marginals=spec, bounds={"zz": (0, 1)}, kmax=3, info=True)
    failed = pkg.evidence_many_from_files([root, roots["b"]], marginals=spec, bounds=[{"zz": (0, 1)}, None], kmax=3, info=True, return_exceptions=True)
    assert isinstance(failed[0], ValueError) and same_dict(failed[1][1]["marginals"], own_b)     # the root fails alone


def test_without_bounds_nothing_moves_and_no_bounded_call_is_made(roots, monkeypatch):
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi, marginals
    root = roots["a"]
    spec = {"probs": (0.68, 0.95), "grid": 128}
    sp = marginals.spec(spec)
    kw = dict(kmax=3, verbose=0)
    calls = []

    def refuse(*a, **k):
        calls.append(1)
        raise AssertionError("a bounded call without bounds")
    for sym in ("param_marginals_bounded_dev", "param_marginals_bounded"):
        monkeypatch.setattr(_capi, sym, refuse)
    plain_dev = []
    real = _capi.param_marginals_dev
    monkeypatch.setattr(_capi, "param_marginals_dev", lambda *a, **k: plain_dev.append(1) or real(*a, **k))
    host = pkg.MCEvidence(root, marginals=spec, **kw)
    hostE, hinfo = host.evidence(info=True)
    part = host.gd.data["s1"]
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.ascontiguousarray(np.asarray(part.samples, dtype=np.float64)[:, :host.ndim])
    blk, = _capi.param_marginals([(x, x.shape[1], a)], sp[0], sp[1], sp[2])
    want = marginals.build(marginals.from_block(blk, x.shape[1], 2, 128), sp, roots["a_bounds"][0][:host.ndim])
    assert same_dict(hinfo["marginals"], want) and not set(marginals.BOUND_KEYS) & set(want)
    n0 = len(plain_dev)
    for extra in ({}, {"bounds": None}):
        lnE, info = pkg.evidence_from_files(root, marginals=spec, info=True, require_resident=True, **extra, **kw)
        assert same_dict(info["marginals"], want) and np.array_equal(lnE, pkg.evidence_from_files(root, info=True, require_resident=True, **kw)[0])
    assert len(plain_dev) == n0 + 2                              # one mce_param_marginals_dev call each, as before
    outs = pkg.evidence_many_from_files([root, roots["b"]], marginals=spec, kmax=3, info=True)
    assert same_dict(outs[0][1]["marginals"], want) and len(plain_dev) == n0 + 3 and not calls
