"""converge on the device: ``mce_chain_conv_dev`` (csrc/chain_conv_kernels.hpp) on every case of tests/conv_cases.py against the
extended precision model, within the bound derived in docs/design/chain_conv.md; two runs bit for bit; the host-pointer form; many
systems in one call, each bit for bit its own single call whatever its neighbours and its place; the status cases per system; the
resident route and the farm with ``converge``; the argument errors.

Measured on one MI355X (error / bound, worst over both ``by`` forms; the bound is conv_cases.model's): see docs/design/chain_conv.md."""
import numpy as np
import pytest

import conv_cases as cv

pytestmark = pytest.mark.gpu


def measure_systems(systems, nd):
    """ONE mce_chain_conv_dev call on device copies of ``systems`` (a list of segment lists, host arrays) -> the binding's dict of arrays"""
    import torch
    from mcevidence_amd import _capi
    tensors = [[torch.from_numpy(np.array(s, dtype=np.float64)).to("cuda:0") for s in sy] for sy in systems]
    segs = [(t.data_ptr() if t.shape[0] else 0, int(t.shape[0])) for sy in tensors for t in sy]
    seg_sys = [y for y, sy in enumerate(tensors) for _ in sy]
    ncols = int(systems[0][0].shape[1])
    wsb = _capi.chain_conv_workspace_bytes(sum(n for _, n in segs), len(segs), len(systems), nd)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.chain_conv_dev(segs, seg_sys, len(systems), ncols, 0, 2, nd, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return got


def one(got, y=0):
    return dict(r_minus_1=got["r_minus_1"][y], per_param=got["per_param"][y], status=int(got["status"][y]), column=int(got["column"][y]),
                used=int(got["used"][y]))


def bits(got, y=0):
    return got["r_minus_1"][y].tobytes() + got["per_param"][y].tobytes() + bytes([int(got["status"][y]), int(got["used"][y])])


def measure_case(name, by):
    chains = cv.parts(name)
    return measure_systems([cv.segments(chains, by)], chains[0].shape[1] - 2)


@pytest.mark.parametrize("by", cv.BY)
@pytest.mark.parametrize("name", cv.NUMERIC)
def test_device_equals_the_model(name, by):
    got = one(measure_case(name, by))
    assert got["status"] == 0
    cv.check(got, cv.model(name, by), "device %s/%s" % (name, by))


@pytest.mark.parametrize("name", ["B", "C", "E", "F", "J"])
def test_two_runs_give_the_same_bits(name):
    assert bits(measure_case(name, "halves")) == bits(measure_case(name, "halves"))


def test_host_pointer_form_equals_the_device_form():
    from mcevidence_amd import _capi
    for name in ("C", "I"):
        segs = cv.segments(cv.parts(name), "halves")
        a = _capi.chain_conv(segs, [0] * len(segs), 1, 0, 2, segs[0].shape[1] - 2)
        assert bits(a) == bits(measure_case(name, "halves"))


def test_many_systems_in_one_call():
    """A, C, D, G and J have 3, 4, 8, 6 and 27 parameters: one call takes one (ncols, ndim), so every system is measured on its first 3
    parameter columns of rows cut to 5 columns -- still five different shapes of segments and tiles"""
    names = ("A", "C", "D", "G", "J")
    systems = {n: [np.ascontiguousarray(s[:, :5]) for s in cv.segments(cv.parts(n), "chains")] for n in names}
    alone = {n: bits(measure_systems([systems[n]], 3)) for n in names}
    for n in names:
        cv.check(one(measure_systems([systems[n]], 3)), cv.model_segments(systems[n], 3), "alone %s" % n)
    empty = np.zeros((0, 5))
    for order in (names, names[::-1], ("G", "A", "J", "C", "D")):
        got = measure_systems([systems[n] for n in order], 3)
        for y, n in enumerate(order):
            assert bits(got, y) == alone[n], (order, n)
        # the same with segments without rows in between: a system's worth of padding, spread over its neighbours
        padded = [[empty, empty] + systems[n][:1] + [empty] + systems[n][1:] + [empty] for n in order]
        got = measure_systems(padded, 3)
        for y, n in enumerate(order):
            assert got["r_minus_1"][y].tobytes() == measure_systems([systems[n]], 3)["r_minus_1"][0].tobytes(), (order, n)
            assert got["per_param"][y].tobytes() == measure_systems([systems[n]], 3)["per_param"][0].tobytes() and got["used"][y] == len(systems[n])


def test_status_cases_per_system_and_a_failing_system_fails_alone():
    from mcevidence_amd import chains
    good = [np.array(s) for s in cv.parts("A")]
    alone = bits(measure_systems([good], 3))
    for name in ("S2", "S3nan", "S3inf", "S3neg", "S3both"):
        bad = [np.array(s) for s in cv.parts(name)]
        status, column = cv.STATUS_WANT[name]
        for systems, yb, yg in (([bad, good], 0, 1), ([good, bad], 1, 0), ([good, bad, good], 1, 2)):
            got = measure_systems(systems, 3)
            assert (int(got["status"][yb]), int(got["column"][yb])) == (status, column), name
            assert np.isnan(got["r_minus_1"][yb]) and np.all(np.isnan(got["per_param"][yb]))
            assert bits(got, yg) == alone, name
            with pytest.raises(ValueError) as e:
                chains.conv_info(one(got, yb), "chains", 3, 150)
            assert str(e.value) == str(chains.conv_status_error(status, column))
    # status 4 keeps per_param; a segment of weight 0 is skipped, and with one segment left the status is 5
    s4 = [np.array(s) for s in cv.parts("S4")]
    got = one(measure_systems([s4], 6))
    assert got["status"] == 4 and np.isnan(got["r_minus_1"]) and np.all(np.isfinite(got["per_param"]))
    assert np.allclose(got["per_param"], chains.gelman_rubin(s4)["per_param"], rtol=1e-12)
    zero = np.array(cv.parts("A")[1])
    zero[:, 0] = 0.0
    got = one(measure_systems([[good[0], zero]], 3))
    assert (got["status"], got["used"]) == (5, 1)
    with pytest.raises(ValueError, match="halves"):
        chains.conv_info(got, "chains", 2, 514)


def test_argument_errors_need_no_device():
    from mcevidence_amd import _capi
    P = 0x1000
    ok = dict(segs=[(P, 100), (P, 100)], seg_sys=[0, 0], nsys=1, ncols=5, iw=0, itheta=2, ndim=3, ws=P, ws_bytes=1 << 30)
    with pytest.raises(ValueError, match="more than 128 segments"):
        _capi.chain_conv_dev(**dict(ok, segs=[(P, 10)] * 129, seg_sys=[0] * 129))
    with pytest.raises(ValueError, match="ndim=128"):
        _capi.chain_conv_dev(**dict(ok, ndim=128, ncols=200))
    with pytest.raises(ValueError, match="1 segments with rows"):
        _capi.chain_conv_dev(**dict(ok, segs=[(P, 100), (P, 0)]))
    with pytest.raises(ValueError, match="seg_sys"):
        _capi.chain_conv_dev(**dict(ok, seg_sys=[1, 0], nsys=2))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("conv_roots")
    out = {}
    for name, seed, rows, nnuis in (("p21", 11, (1500, 1400, 1450, 1300), 15), ("p21b", 12, (1200, 1250, 1100, 1300), 15), ("p9", 13, (900, 1000, 950), 3)):
        out[name] = str(d / name)
        write_cosmomc_chains(out[name], planck_like_chains(seed=seed, rows=rows, nnuis=nnuis)[0], None, fmt="%.17g")
    return out


def test_resident_route_with_converge(roots):
    import mcevidence_amd as pkg
    root = roots["p21"]
    parts = [np.loadtxt(root + "_%d.txt" % i) for i in (1, 2, 3, 4)]
    lnE, info = pkg.evidence_from_files(root, converge=True, kmax=3, verbose=0, info=True, require_resident=True)
    host = pkg.MCEvidence(root, converge=True, kmax=3, verbose=0)
    want = cv.model_segments(parts, 21)
    cv.check(info["converge"], want, "resident")
    cv.check(host.info["converge"], want, "host")
    c, h = info["converge"], host.info["converge"]
    assert abs(c["r_minus_1"] - h["r_minus_1"]) <= 2 * want["bound_r"] and np.all(np.abs(np.subtract(c["per_param"], h["per_param"])) <= 2 * want["bound_per"])
    assert {k: c[k] for k in c if k not in ("r_minus_1", "per_param")} == {k: h[k] for k in h if k not in ("r_minus_1", "per_param")}
    assert info["route"] == "resident" and c["by"] == "chains" and c["segments"] == 4 and c["rows"] == sum(len(p) for p in parts)
    # ln E is bit for bit what the route returns without the keyword
    lnE0, info0 = pkg.evidence_from_files(root, kmax=3, verbose=0, info=True, require_resident=True)
    assert np.array_equal(lnE, lnE0) and "converge" not in info0 and {k: v for k, v in info.items() if k != "converge"} == info0
    # burn-in, halves, ndim and a threshold; thinning does not change what is measured
    burned = [p[int(0.3 * len(p)):] for p in parts]
    wantb = cv.model_segments(cv.segments(burned, "halves"), 6)
    for extra in (dict(), dict(thinlen=2), dict(thin_corr=True)):
        rc = pkg.ResidentChains.from_files(root, burnlen=0.3, ndim=6, converge=1e-6, converge_by="halves", **extra)
        cv.check(rc.converge, wantb, "resident burned %r" % (extra,))
        assert rc.converge["converged"] is False and rc.converge["segments"] == 8 and rc.converge["by"] == "halves"
    arr = pkg.ResidentChains.from_arrays(parts, converge=True, ndim=21)
    assert arr.converge["r_minus_1"] == c["r_minus_1"] and arr.converge["per_param"] == c["per_param"]


def test_farm_measures_every_root_as_its_own_resident_run(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p21", "p9", "p21b", "p21"]
    thins = [0, 0, 0, 3]
    outs = pkg.evidence_many_from_files([roots[n] for n in names], converge=0.5, thinlen=thins, kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 4 and farm.LAST_STATS["counts"]["farm"] == 4
    for n, t, (lnE, info) in zip(names, thins, outs):
        own = pkg.evidence_from_files(roots[n], converge=0.5, thinlen=t, kmax=3, verbose=0, info=True, require_resident=True)
        assert info["converge"] == own[1]["converge"], n
        assert info["converge"]["converged"] is True and info["converge"]["segments"] == (3 if n == "p9" else 4)
    plain = pkg.evidence_many_from_files([roots[n] for n in names], thinlen=thins, kmax=3, info=True)
    for a, b in zip(outs, plain):
        assert np.array_equal(a[0], b[0]) and "converge" not in b[1]
    mixed = pkg.evidence_many_from_files([roots["p21"], roots["p9"]], converge=[True, None], kmax=3, info=True)
    assert mixed[0][1]["converge"]["threshold"] is None and "converge" not in mixed[1][1]
