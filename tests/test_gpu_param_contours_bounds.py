"""contours with hard prior bounds on the device: ``mce_param_contours_bounded_dev`` (the <true> instances of
csrc/param_contours_kernels.hpp) on the cases of tests/contours_bounds_cases.py: the grid that ends on a bound, every density within its
derived bound of the exact three-term boundary-kernel estimate at the reported h, c, lo and step (mpmath on the query cells, the extended
format on all), every density within two bounds of ``contours.measure_bounded``'s, every decision bit for bit the serial rule's on the
device's own densities (NumPy and the sanitized native program) and the oracle's on every decided cell; every pair of two open columns
byte-equal to ``mce_param_contours_dev`` on the same rows, and a call whose bounds are all open equal to it on every shared key; a pair
asked alone against the same pair among all columns, and in other probabilities; status 8, 7 before 8, the refused systems;
systems with bounds of their own in one call; the host-pointer form; and the Exponential corner of
tests/test_param_contours_bounds_shared.py on the device.

Measured on one MI355X (error / bound): see docs/design/contours_bounds.md."""
import numpy as np
import pytest

import contours_bounds_cases as cb
import contours_cases as cc

pytestmark = pytest.mark.gpu
INF = float("inf")


def measure(systems, cols, probs=cb.PROBS, grid=64, scale=1.0):
    """ONE mce_param_contours_bounded_dev call on device copies of ``systems`` = [(a, x[n, ld], d, (lo[nc], hi[nc]))] -> one float64
    block per system"""
    import torch
    from mcevidence_amd import _capi
    keep, segs = [], []
    for a, x, d, _ in systems:
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x if x.ndim == 2 else x.reshape(len(a), -1)
        t = [torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0") for v in (x, a)]
        keep.append(t)
        n = len(a)
        segs.append((t[0].data_ptr() if n else 0, x.shape[1], n, d, t[1].data_ptr() if n else 0))
    wsb = _capi.param_contours_bounded_workspace_bytes(sum(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(cols), len(probs), grid)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_contours_bounded_dev(segs, cols, [b for _, _, _, b in systems], probs, grid, scale, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def measure_plain(c):
    """ONE mce_param_contours_dev call on a device copy of the case's rows -> what ``contours.measure`` returns"""
    import torch
    from mcevidence_amd import _capi, contours
    x, a = (torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0") for v in (c.x, c.a))
    wsb = _capi.param_contours_workspace_bytes(len(c.a), 1, c.d, c.nc, len(c.probs), c.grid)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    blk, = _capi.param_contours_dev([(x.data_ptr(), c.x.shape[1], len(c.a), c.d, a.data_ptr())], c.cols, c.probs, c.grid, c.scale, ws.data_ptr(), wsb,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return contours.from_block(np.array(blk), c.nc, len(c.probs), c.grid)


def sys_of(c):
    return (c.a, c.x, c.d, c.bounds)


def as_dict(block, c):
    from mcevidence_amd import contours
    return contours.from_block_bounded(block, c.nc, len(c.probs), c.grid)


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {name: measure([sys_of(c)], c.cols, c.probs, c.grid, c.scale)[0] for name, c in cb.cases().items()}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cb.build_checker(tmp_path_factory.mktemp("param_contours_bounds_gpu"))


@pytest.mark.parametrize("name", list(cb.cases()))
def test_device_against_the_oracle(name, singles, checker, tmp_path):
    c = cb.cases()[name]
    got = as_dict(singles[name], c)
    assert (got["status"], got["column"], got["rows"], got["grid"], got["nc"]) == (0, -1, c.n, c.grid, c.nc)
    assert np.all(got["col_status"] == 0.0) and np.array_equal(got["col"], np.array(c.cols, dtype=np.float64))
    stats = {}
    for p, s, t in cb.oracle_pairs(c):
        cb.check_pair(c, got, p, s, t, "device", stats=stats)
    # ALL densities against the NumPy form's, within two bounds; ALL decisions bit for bit the serial rule's on the device's own densities
    cb.check_against_numpy(c, got, "device")
    assert cb.check_decisions_native(checker, tmp_path, [got], c.probs, c.grid) == c.nc * (c.nc - 1) // 2
    assert stats["undecided"] <= cb.MAX_UNDECIDED


@pytest.mark.parametrize("name", list(cb.cases()))
def test_open_pairs_are_the_call_without_bounds_bit_for_bit(name, singles):
    from mcevidence_amd import contours
    c = cb.cases()[name]
    got = as_dict(singles[name], c)
    plain = measure_plain(c)
    assert cb.assert_open_pairs_equal(c, got, plain, (name, "device")) == sum(1 for s, t in contours.pairs(c.nc) if c.open_t(s) and c.open_t(t))
    o = cb.open_case(c)
    all_open = as_dict(measure([sys_of(o)], o.cols, o.probs, o.grid, o.scale)[0], o)
    assert cb.equal_common(all_open, plain), name
    assert np.all(all_open["at_lo"] == 0.0) and np.all(all_open["at_hi"] == 0.0) and np.all(all_open["bound_lo"] == -INF) and np.all(all_open["bound_hi"] == INF)


def test_a_pair_alone_among_all_columns_and_in_other_probabilities(singles):
    from mcevidence_amd import contours
    g = cb.cases()
    probs = (0.1, 0.3, 0.5, 0.68, 0.9, 0.95, 0.99)
    for name, pairs in (("n513_nc6_G64_fractional", ((1, 4), (0, 5), (3, 5), (0, 1))), ("n1025_nc6_G32_integer", ((1, 3), (0, 2), (2, 5))), ("n8705_nc3_G64_unit", ((0, 2),))):
        c = g[name]
        whole = as_dict(singles[name], c)
        for s, t in pairs:
            sub = cb.sub_case(c, (s, t))
            p = contours.pairs(c.nc).index((s, t))
            alone = as_dict(measure([sys_of(sub)], sub.cols, sub.probs, sub.grid, sub.scale)[0], sub)
            assert cb.pair_values(whole, p).tobytes() == cb.pair_values(alone, 0).tobytes(), (name, s, t)
            other = contours.from_block_bounded(measure([sys_of(sub)], sub.cols, probs, sub.grid, sub.scale)[0], 2, 7, sub.grid)
            assert whole["density"][p].tobytes() == other["density"][0].tobytes(), (name, s, t)
            for k in contours.P_KEYS:
                assert whole[k][0][p] == other[k][3][0] and whole[k][1][p] == other[k][5][0], (name, s, t, k)


def test_a_value_outside_its_bounds_fails_its_pairs_alone(singles):
    from mcevidence_amd import contours
    c = cb.cases()["n513_nc6_G64_fractional"]
    lo = c.lo.copy()
    lo[2] = float(np.sort(c.x[c.use, c.cols[2]])[3]) + 1.0 / 1024.0
    bad = cb.Case("outside", c.a, c.x, c.d, c.cols, lo, c.hi, c.kinds, grid=c.grid)
    first, mid, last = measure([sys_of(c), sys_of(bad), sys_of(c)], c.cols, c.probs, c.grid)
    assert first.tobytes() == last.tobytes() == singles[c.name].tobytes()
    got = as_dict(mid, bad)
    assert list(got["col_status"]) == [0.0, 0.0, 8.0, 0.0, 0.0, 0.0] and got["bound_lo"][2] == lo[2] and np.isnan(got["at_lo"][2]) and np.isnan(got["h"][2])
    rest = cb.sub_case(c, (0, 1, 3, 4, 5))
    without = as_dict(measure([sys_of(rest)], rest.cols, rest.probs, rest.grid)[0], rest)
    q = 0
    for p, (s, t) in enumerate(contours.pairs(6)):
        if 2 in (s, t):
            cb.assert_failed_pair(got, p, 8.0, "outside")
        else:
            assert cb.pair_values(got, p).tobytes() == cb.pair_values(without, q).tobytes(), (s, t)
            q += 1
    cb.check_against_numpy(bad, got, "device")


def test_status_7_comes_before_8_and_refused_systems_are_unchanged(singles):
    from mcevidence_amd import contours
    c = cc.constant_column_case()
    bad = cb.Case("seven_first", c.a, c.x, c.d, c.cols, [-INF, 3.0, 2.0], [INF, 4.0, INF], ("open", "both", "gamma_at_0"), grid=c.grid)
    got = as_dict(measure([sys_of(bad)], bad.cols, bad.probs, bad.grid)[0], bad)
    assert list(got["col_status"]) == [0.0, 7.0, 8.0] and list(got["pair_status"]) == [7.0, 8.0, 7.0]
    for p, st in enumerate((7.0, 8.0, 7.0)):
        cb.assert_failed_pair(got, p, st, "seven_first")
    good = cb.cases()["n16_nc2_G32_unit"]
    for name, a, x, status, column in cc.status_cases():
        blocks = measure([sys_of(good), (a, x, x.shape[1], ([-INF, 0.0], [INF, INF])), sys_of(good)], good.cols, good.probs, good.grid)
        assert blocks[0].tobytes() == singles[good.name].tobytes() == blocks[2].tobytes(), name
        failed = contours.from_block_bounded(blocks[1], 2, len(good.probs), good.grid)
        cc.assert_failed_system({k: failed[k] for k in failed if k not in contours.BOUND_KEYS}, status, column, int(np.count_nonzero(a != 0)), name)
        for k in contours.BOUND_KEYS:
            assert np.isnan(failed[k]).all(), (name, k)


def test_systems_with_their_own_bounds_and_the_host_pointer_form(singles):
    from mcevidence_amd import _capi
    g = cb.cases()
    a, b = g["n17_nc3_G64_integer"], g["n8705_nc3_G64_unit"]
    empty = (np.zeros(0), np.zeros((0, 3)), 3, ([-INF] * 3, [INF] * 3))
    for order in ([a, b], [b, a]):
        systems = [sys_of(c) for c in order]
        systems.insert(1, empty)
        got = measure(systems, (0, 1, 2))
        assert got[1][3] == 5 and got[1][2] == 0           # the empty segment: status 5, no rows
        assert got[0].tobytes() == singles[order[0].name].tobytes() and got[2].tobytes() == singles[order[1].name].tobytes()
    assert measure([sys_of(b)], b.cols, b.probs, b.grid)[0].tobytes() == singles[b.name].tobytes()      # two runs
    host = _capi.param_contours_bounded([(c.x, c.d, c.a) for c in (a, b)], (0, 1, 2), [a.bounds, b.bounds], cb.PROBS, 64, 1.0)
    assert np.array(host[0]).tobytes() == singles[a.name].tobytes() and np.array(host[1]).tobytes() == singles[b.name].tobytes()


@pytest.mark.parametrize("seed", range(5))
def test_the_exponential_corner(seed):
    c = cb.exponential_case(seed)
    got = as_dict(measure([sys_of(c)], c.cols, c.probs, c.grid)[0], c)
    cb.assert_exponential_corner(c, got, "device")


# ---- the routes ------------------------------------------------------------------------------------------------------------------------
def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, tuple, str)))
        for k in a)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """three small Planck-shaped roots with .ranges and .paramnames: a lower bound on the second column that cuts its samples' range (the
    rows below it are dropped from the chains first), an upper bound at the third column's largest sample, open sides"""
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("contours_bounds_roots")
    out = {}
    for name, seed, rows in (("a", 71, (700, 650, 600)), ("b", 72, (600, 640, 620)), ("ab", 73, (650, 600, 610))):
        out[name] = str(d / name)
        chains, names, _ = planck_like_chains(seed=seed, rows=rows, nnuis=3)
        chains = [np.array(c) for c in chains]
        cut = float(np.median(np.concatenate([c[:, 3] for c in chains])))
        chains = [c[c[:, 3] >= cut] for c in chains]
        top = float(max(c[:, 4].max() for c in chains))
        ranges = [(n, -INF, None) for n in names]
        ranges[1] = (names[1], cut, None)
        ranges[2] = (names[2], -INF, top)
        write_cosmomc_chains(out[name], chains, ranges, fmt="%.17g")
        with open(out[name] + ".paramnames", "w") as fh:
            fh.write("".join("%s\t%s\n" % (n, n.upper()) for n in names))
        out[name + "_bounds"] = (names, cut, top)
    return out


def host_rows(host):
    part = host.gd.data["s1"]
    return np.asarray(part.adjusted_weights, dtype=np.float64), np.ascontiguousarray(np.asarray(part.samples, dtype=np.float64)[:, :host.ndim])


def test_routes_with_bounds_from_the_ranges_file(roots, tmp_path, capsys, caplog):
    import logging
    import mcevidence_amd as pkg
    from mcevidence_amd import _capi, cli, contours, tension
    root = roots["a"]
    names, cut, top = roots["a_bounds"]
    spec = {"probs": (0.68, 0.95), "grid": 32, "params": list(names[:3]), "bounds": "ranges"}
    plain_spec = {k: v for k, v in spec.items() if k != "bounds"}
    kw = dict(kmax=3, verbose=0)
    host = pkg.MCEvidence(root, contours=spec, **kw)
    hostE, hinfo = host.evidence(info=True)
    sp = contours.spec(spec, ndim=host.ndim, names=names[:host.ndim])
    lo, hi = contours.bounds_spec(spec, names=names[:host.ndim], ndim=host.ndim, root=root)
    assert list(lo) == [-INF, cut, -INF] and list(hi) == [INF, INF, top] and sp[3] == (0, 1, 2)
    a, x = host_rows(host)
    blk, = _capi.param_contours_bounded([(x, x.shape[1], a)], sp[3], [(lo, hi)], sp[0], sp[1], sp[2])
    direct = contours.from_block_bounded(blk, 3, 2, 32)
    want = contours.build(direct, sp, names[:host.ndim])
    h = hinfo["contours"]
    assert same_dict(h, want) and h["at_lo"][1] == 1.0 and h["grid_lo"][1] == cut and h["at_hi"][2] == 1.0 and np.all(h["lower_y"][:, 0] >= cut)
    # the device's block against the NumPy form's on the same rows: within two bounds, every decision bit for bit
    case = cb.Case("route_a", a, x, x.shape[1], sp[3], lo, hi, ("open", "lower_at_min", "upper"), grid=32)
    assert cb.check_against_numpy(case, direct, "route") <= 1.0
    # ln E does not move, and without the key the dict keeps exactly its keys and the INFO line is logged
    assert np.array_equal(hostE, pkg.MCEvidence(root, **kw).evidence())
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        caplog.clear()
        loud = dict(kw, verbose=1)
        lnE, info = pkg.evidence_from_files(root, contours=spec, marginals=True, bounds="ranges", info=True, require_resident=True, **loud)
        assert not [r for r in caplog.records if "not boundary-corrected" in r.getMessage()]
        caplog.clear()
        lnE0, info0 = pkg.evidence_from_files(root, contours=plain_spec, marginals=True, bounds="ranges", info=True, require_resident=True, **loud)
        assert len([r for r in caplog.records if "not boundary-corrected" in r.getMessage()]) == 1
    assert info["route"] == "resident" and same_dict(info["contours"], want) and np.array_equal(lnE, lnE0) and np.array_equal(lnE, hostE)
    assert set(info["contours"]) - set(info0["contours"]) == set(contours.BOUND_KEYS) and not set(info0["contours"]) - set(info["contours"])
    own_plain = pkg.evidence_from_files(root, contours=plain_spec, info=True, require_resident=True, **kw)[1]["contours"]
    assert same_dict(info0["contours"], own_plain)
    # "bounds": True takes the call's bounds=, with no marginals=; the mapping and the sequence
    forms = ({names[1]: (cut, None), names[2]: (None, top)}, [(None, None), (cut, "N"), (-INF, top)] + [None] * (host.ndim - 3))
    for form in forms:
        assert same_dict(pkg.evidence_from_files(root, contours=dict(plain_spec, bounds=form), info=True, require_resident=True, **kw)[1]["contours"], want)
    assert same_dict(pkg.evidence_from_files(root, contours=dict(plain_spec, bounds=True), bounds=forms[0], info=True, require_resident=True, **kw)[1]["contours"], want)
    with pytest.raises(ValueError, match="^contours="):
        pkg.evidence_from_files(root, contours=dict(plain_spec, bounds=True), info=True, require_resident=True, **kw)
    # the farm: a bounded and an unbounded root in one wave, each through its own call
    three = [roots[n] for n in ("a", "b", "ab")]
    outs = pkg.evidence_many_from_files(three, contours=[spec, plain_spec, spec], kmax=3, info=True)
    own_b = pkg.evidence_from_files(roots["b"], contours=plain_spec, info=True, require_resident=True, **kw)[1]["contours"]
    own_ab = pkg.evidence_from_files(roots["ab"], contours=spec, info=True, require_resident=True, **kw)[1]["contours"]
    assert [o[1]["route"] for o in outs] == ["farm"] * 3 and same_dict(outs[0][1]["contours"], want)
    assert same_dict(outs[1][1]["contours"], own_b) and "at_lo" not in own_b and same_dict(outs[2][1]["contours"], own_ab)
    assert own_ab["grid_lo"][1] == roots["ab_bounds"][1] and np.array_equal(outs[0][0], lnE)
    failed = pkg.evidence_many_from_files([root, roots["b"]], contours=[dict(plain_spec, bounds={"zz": (0, 1)}), plain_spec], kmax=3, info=True, return_exceptions=True)
    assert isinstance(failed[0], ValueError) and str(failed[0]).startswith("contours=") and same_dict(failed[1][1]["contours"], own_b)
    # --tension's three runs
    ta, tb, tab, tinfo = tension.evidence_tension(roots["a"], roots["b"], roots["ab"], contours=spec, kmax=3)
    assert same_dict(tinfo["roots"][0]["contours"], want) and same_dict(tinfo["roots"][2]["contours"], own_ab)
    # the command line
    npz = str(tmp_path / "res.npz")
    cli.main([root, "-k", "3", "--resident", "--contours", "--contours-grid", "32", "--contours-params", *names[:3], "--contours-bounds", "--contours-out", npz, "-vb", "0"])
    z = np.load(npz)
    assert np.array_equal(z["density_0"], want["density"]) and np.array_equal(z["bound_lo_0"], lo) and z["at_lo_0"][1] == 1.0 and z["at_hi_0"][2] == 1.0
    cli.main([root, "-k", "3", "--resident", "--contours", "--contours-grid", "32", "--contours-params", *names[:3], "--contours-bounds", "%s=%r:" % (names[1], cut),
              "%s=:%r" % (names[2], top), "--contours-out", npz, "-vb", "0"])
    assert np.array_equal(np.load(npz)["density_0"], want["density"])
    capsys.readouterr()
    args = cli.build_parser().parse_args([root, "--contours", "--contours-bounds"])
    assert cli._contours_kw(args) == {"contours": {"probs": True, "bounds": "ranges"}}
    args = cli.build_parser().parse_args([root, "--contours", "0.5", "--contours-bounds", "a=0:", "b=N:2"])
    assert cli._contours_kw(args) == {"contours": {"probs": (0.5,), "bounds": {"a": ("0", None), "b": (None, "2")}}}
    assert cli._contours_kw(cli.build_parser().parse_args([root, "--contours"])) == {"contours": True}


def test_a_value_outside_logs_one_warning_and_leaves_ln_e_alone(roots, caplog):
    import logging
    import mcevidence_amd as pkg
    root = roots["a"]
    names, cut, top = roots["a_bounds"]
    kw = dict(kmax=3, verbose=0)
    spec = {"grid": 32, "params": list(names[:3]), "bounds": {names[0]: (None, None), names[2]: (None, top - 1e-3)}}
    with caplog.at_level(logging.WARNING, logger="mcevidence_amd"):
        lnE, info = pkg.evidence_from_files(root, contours=spec, info=True, require_resident=True, **kw)
    assert len([r for r in caplog.records if r.levelno == logging.WARNING and "contours" in r.getMessage()]) == 1
    c = info["contours"]
    assert list(c["col_status"]) == [0.0, 0.0, 8.0] and list(c["pair_status"]) == [0.0, 8.0, 8.0] and np.isfinite(c["density"][0]).all()
    assert np.array_equal(lnE, pkg.evidence_from_files(root, require_resident=True, **kw))
