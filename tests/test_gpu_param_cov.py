"""covariance on the device: ``mce_param_cov_dev`` (csrc/param_cov_kernels.hpp) on the cases of tests/cov_cases.py against the exact
model, within the bounds derived in docs/design/tension.md: the k-step, LDS-chunk, tile and column-block edges; a Gram pass that must be
centred; zero weights over NaN and inf; structured columns; the status cases, each between two good systems; many systems of several
shapes in one call, each bit for bit its own single call whatever its neighbours and its place; two runs bit for bit; the host-pointer
form; the means bit for bit ``mce_param_summary_dev``'s; the resident route and the farm with ``covariance``.

Measured on one MI355X (error / bound): see docs/design/tension.md."""
import numpy as np
import pytest

import cov_cases as cc
import summary_cases as sc

pytestmark = pytest.mark.gpu


def _upload(cases):
    import torch
    keep, segs = [], []
    for a, x, d in cases:
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x if x.ndim == 2 else x.reshape(len(a), -1)
        t = [torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0") for v in (x, a)]
        keep.append(t)
        n = len(a)
        segs.append((t[0].data_ptr() if n else 0, x.shape[1], n, d, t[1].data_ptr() if n else 0))
    return keep, segs


def measure(cases):
    """ONE mce_param_cov_dev call on device copies of ``cases`` = [(a, x[n, ld], d)] -> one float64 block per system"""
    import torch
    from mcevidence_amd import _capi
    keep, segs = _upload(cases)
    wsb = _capi.param_cov_workspace_bytes(sum(s[2] for s in segs), len(segs), max(s[3] for s in segs))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_cov_dev(segs, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def sys_of(c):
    return (c.a, c.x, c.d)


def as_dict(block, d):
    from mcevidence_amd import covariance
    return covariance.from_block(block, d)


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {name: measure([sys_of(c)])[0] for name, c in cc.gpu_cases().items()}


EDGES = ["A_%d_%d" % (n, d) for d in (17, 127) for n in cc.GPU_EDGE_N] + ["A_513_%d" % d for d in cc.GPU_EDGE_D if d not in (17, 127)]


@pytest.mark.parametrize("name", EDGES + ["B_centring", "C_skipped", "D_structure", "D_denormal"])
def test_device_equals_the_exact_model(name, singles):
    # A: the k-step of 4, the LDS chunk of 64, the tile of 512 and the column blocks of 16 (ld = d + 2); B: a Gram pass that must be
    # centred; C: zero weights over NaN and inf; D: identical, negated and constant columns, +-1e150 beside +-1e-150, denormals
    from mcevidence_amd import covariance
    c = cc.gpu_cases()[name]
    got = as_dict(singles[name], c.d)
    cc.check(c, got, "device")
    cc.check_info(c, covariance.build(got), "device")
    if name == "B_centring":
        assert np.all(np.abs(np.diagonal(got["cov"]) - 1e-12) < 1e-14)         # (an uncentred pass is left with 2500 eps = 5e-13 of noise)
    if name == "D_structure":
        C = got["cov"]
        assert C[0, 0] == C[0, 1] == C[1, 1] == -C[0, 2] == C[2, 2] and np.all(C[3] == 0.0)      # identical, negated, constant
        corr = covariance.build(got)["corr"]
        assert abs(corr[0, 1] - 1.0) <= 4 * cc.EPS and abs(corr[0, 2] + 1.0) <= 4 * cc.EPS and np.isnan(corr[3]).all()


def test_status_cases_fail_alone(singles):
    good = cc.gpu_cases()["F_a"]
    for name, a, x, status, column in cc.status_cases():
        got = measure([sys_of(good), (a, x, x.shape[1]), sys_of(good)])
        assert got[0].tobytes() == singles["F_a"].tobytes() == got[2].tobytes(), name
        bad = as_dict(got[1], x.shape[1])
        assert (bad["status"], bad["column"]) == (status, column) and bad["rows"] == int(np.count_nonzero(a != 0)), (name, bad)
        assert all(np.isnan(bad[k]).all() for k in ("W", "A2", "mean", "cov")), (name, bad)
        assert measure([(a, x, x.shape[1])])[0].tobytes() == got[1].tobytes(), name


def test_five_systems_of_three_shapes_in_three_orders(singles):
    names = ["F_a", "F_c", "F_b", "F_e", "F_d"]            # (d, ld): (8, 8), (27, 30), (8, 8), (40, 41), (27, 30)
    g = cc.gpu_cases()
    empty = (np.zeros(0), np.zeros((0, 3)), 3)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        systems = [sys_of(g[names[i]]) for i in order]
        systems.insert(2, empty)
        got = measure(systems)
        assert got[2][3] == 5 and got[2][2] == 0           # the empty segment: status 5, no rows
        del got[2]
        for i, block in zip(order, got):
            assert block.tobytes() == singles[names[i]].tobytes(), (order, names[i])
    for name in names:
        cc.check(g[name], as_dict(singles[name], g[name].d), "device")


def test_two_runs_and_the_host_pointer_form(singles):
    from mcevidence_amd import _capi
    g = cc.gpu_cases()
    for name in ("A_513_127", "B_centring", "F_b"):
        assert measure([sys_of(g[name])])[0].tobytes() == singles[name].tobytes(), name
    cases = [g[n] for n in ("F_a", "A_513_27", "C_skipped", "F_c")]
    host = _capi.param_cov([c.system for c in cases] + [(np.zeros((0, 2)), 2, np.zeros(0))])
    for c, block in zip(cases, host):
        assert np.array(block).tobytes() == singles[c.name].tobytes(), c.name
    assert host[4][3] == 5


def test_means_are_the_summary_calls_bits(singles):
    """G: ``mean`` is bit for bit ``mce_param_summary_dev``'s on the same segments; C_jj lies within the sum of the two bounds of its var"""
    import torch
    from mcevidence_amd import _capi, summary
    g = cc.gpu_cases()
    names = ["A_1025_17", "A_513_127", "B_centring", "C_skipped", "F_c", "F_e"]
    keep, segs = _upload([sys_of(g[n]) for n in names])
    q = sc.TARGETS
    wsb = _capi.param_summary_workspace_bytes(sum(s[2] for s in segs), max(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(q))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    blocks = _capi.param_summary_dev([s + (0,) for s in segs], q, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    for n, b in zip(names, blocks):
        c = g[n]
        s, v = summary.from_block(np.array(b), c.d, len(q)), as_dict(singles[n], c.d)
        assert s["mean"].tobytes() == v["mean"].tobytes() and s["W"] == v["W"] and s["A2"] == v["A2"] and s["rows"] == v["rows"], n
        ex = c.exact
        bvar = 2.0 * (ex["rows"] + 1) * cc.EPS * np.diagonal(ex["cov"]) + c.bound["mean"] ** 2      # summary.md's bound of var
        r = np.abs(np.diagonal(v["cov"]) - s["var"]) / (bvar + np.diagonal(c.bound["cov"]))
        print("%-12s |C_jj - var_j| / (sum of the two bounds) %.3g" % (n, r.max()))
        assert np.all(r <= 1.0), n


def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, tuple, str)))
        for k in a)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("cov_roots")
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
def test_resident_route_with_covariance(roots, thin, jackknife):
    # H: with the jackknife the ladder whitens the gathered rows in place after the call: a read behind it would fail the bounds
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import PLANCK_PARAMS
    root = roots["p21"]
    kw = dict(kmax=3, verbose=0, thinlen=thin, **({} if jackknife is None else {"jackknife": jackknife}))
    lnE, info = pkg.evidence_from_files(root, covariance=True, summary=True, info=True, require_resident=True, **kw)
    host = pkg.MCEvidence(root, covariance=True, **kw)
    hostE, hinfo = host.evidence(info=True)
    part = host.gd.data["s1"]
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)
    if thin == 0:                                          # the rows are the files' own: raw, not whitened
        rows = np.concatenate([np.loadtxt(root + "_%d.txt" % i) for i in (1, 2, 3, 4)])
        assert np.array_equal(x, rows[:, 2:]) and np.array_equal(a, rows[:, 0])
    case = cc.Case("resident thin=%s jackknife=%s" % (thin, jackknife), a, x)
    d, h = info["covariance"], hinfo["covariance"]
    assert set(d) == set(h) == {"names", "rows", "sum_w", "ess", "mean", "cov", "sd", "corr", "status", "column"}
    for what, s in (("resident", d), ("host    ", h)):
        cc.check_info(case, s, what)
        assert s["names"][:3] == [p[0] for p in PLANCK_PARAMS][:3] and len(s["names"]) == x.shape[1] and "sigma" not in s
    assert d["mean"].tobytes() == info["summary"]["mean"].tobytes()          # with summary also set: the same bits
    assert info["route"] == "resident" and ("jackknife" in info) == (jackknife is not None)
    # ln E is bit for bit what the route returns without the keyword
    lnE0, info0 = pkg.evidence_from_files(root, summary=True, info=True, require_resident=True, **kw)
    untimed = lambda inf: {k: ({j: u for j, u in v.items() if j != "kernel_ms"} if isinstance(v, dict) else v) for k, v in inf.items() if k != "covariance"}      # noqa: E731
    assert np.array_equal(lnE, lnE0) and "covariance" not in info0 and same_dict(untimed(info), untimed(info0))


def test_farm_measures_every_root_as_its_own_resident_run(roots):
    # I: five roots, two shapes, one thinned, one of status 3
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p21", "p9", "bad", "p21b", "p21"]
    thins = [0, 0, 0, 0, 3]
    outs = pkg.evidence_many_from_files([roots[n] for n in names], covariance=True, thinlen=thins, kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 5 and farm.LAST_STATS["counts"]["farm"] == 5
    for n, t, (lnE, info) in zip(names, thins, outs):
        own = pkg.evidence_from_files(roots[n], covariance=True, thinlen=t, kmax=3, verbose=0, info=True, require_resident=True)
        assert same_dict(info["covariance"], own[1]["covariance"]), (n, info["covariance"], own[1]["covariance"])
        assert np.array_equal(lnE, own[0]), n
        assert info["covariance"]["status"] == (3 if n == "bad" else 0), n
    bad = outs[2][1]["covariance"]
    assert np.isnan(bad["mean"]).all() and np.isnan(bad["cov"]).all() and np.isnan(bad["corr"]).all() and bad["column"] == -1 and np.all(np.isfinite(outs[2][0]))
    # the other roots are unaffected by the failing one; without the keyword ln E keeps its bits
    rest = [i for i in range(5) if i != 2]
    without = pkg.evidence_many_from_files([roots[names[i]] for i in rest], covariance=True, thinlen=[thins[i] for i in rest], kmax=3, info=True)
    for i, o in zip(rest, without):
        assert same_dict(outs[i][1]["covariance"], o[1]["covariance"]) and np.array_equal(outs[i][0], o[0]), names[i]
    plain = pkg.evidence_many_from_files([roots[n] for n in names], thinlen=thins, kmax=3, info=True)
    for a, p in zip(outs, plain):
        assert np.array_equal(a[0], p[0]) and "covariance" not in p[1]
    mixed = pkg.evidence_many_from_files([roots["p21"], roots["p9"]], covariance=[True, None], kmax=3, info=True)
    assert mixed[0][1]["covariance"]["cov"].shape == (21, 21) and "covariance" not in mixed[1][1]
