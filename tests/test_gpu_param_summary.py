"""summary on the device: ``mce_param_summary_dev`` (csrc/param_summary_kernels.hpp) on the cases of tests/summary_cases.py against the
exact rational model, within the bounds derived in docs/design/summary.md and with every kept quantile exact; with integer weights
every quantile equal to ``summary.measure``'s; the status cases, each between two good systems; many systems of several shapes in one
call, each bit for bit its own single call whatever its neighbours and its place; two runs bit for bit; the host-pointer form; small
sort passes; no fs; the resident route and the farm with ``summary``.

Measured on one MI355X (error / bound): see docs/design/summary.md."""
import math

import numpy as np
import pytest

import summary_cases as sc

pytestmark = pytest.mark.gpu


def measure(cases, q=sc.TARGETS, pass_elems=0):
    """ONE mce_param_summary_dev call on device copies of ``cases`` = [(a, x[n, ld], d, f or None)] -> one float64 block per system"""
    import torch
    from mcevidence_amd import _capi
    keep, segs = [], []
    for a, x, d, f in cases:
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x if x.ndim == 2 else x.reshape(len(a), -1)
        t = [torch.from_numpy(np.array(v, dtype=np.float64)).to("cuda:0") if v is not None else None for v in (x, a, f)]
        keep.append(t)
        n = len(a)
        segs.append((t[0].data_ptr() if n else 0, x.shape[1], n, d, t[1].data_ptr() if n else 0, t[2].data_ptr() if f is not None and n else 0))
    wsb = _capi.param_summary_workspace_bytes(sum(s[2] for s in segs), max(s[2] for s in segs), len(segs), max(s[3] for s in segs), len(q), pass_elems)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    got = _capi.param_summary_dev(segs, q, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream, pass_elems)
    torch.cuda.synchronize()
    return [np.array(b) for b in got]


def sys_of(c):
    return (c.a, c.x, c.d, c.f)


def as_dict(block, c):
    from mcevidence_amd import summary
    return summary.from_block(block, c.d, len(c.q))


@pytest.fixture(scope="module")
def singles():
    """every case's own single call: the block the other tests compare bits with"""
    return {name: measure([sys_of(c)], c.q)[0] for name, c in sc.gpu_cases().items()}


NAMES = ["A_unit"] + ["B_%d_%d" % (n, d) for n in (511, 512, 513, 1025) for d in (1, 8, 27, 127)] + [
    "C_narrow", "D_zeros", "E_keys_1", "E_keys_2", "E_keys_1000", "L_4100", "T_tie", "K_ties", "K_last", "K_minus_inf"]


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_exact_model(name, singles):
    # A: unit weights; B: the tile edges at every width (ld = d + 2); C: a second pass that must be centred; D: zero weights over NaN and
    # inf; E: the keys' adversaries, n = 1 and 2; T: the designed exact tie; K: the best fit's ties, last row and all f = -inf
    from mcevidence_amd import summary
    c = sc.gpu_cases()[name]
    got = as_dict(singles[name], c)
    sc.check(c, got, "device")
    host = summary.measure(c.a, c.x[:, :c.d], c.f, c.q)
    if np.all(c.a == np.floor(c.a)):
        # integer weights: every sum is exact in every order, so every quantile is the NumPy rule's, dropped triples included
        assert np.array_equal(got["quant"], host["quant"]) and got["W"] == host["W"] and got["A2"] == host["A2"], name
    if name == "E_keys_1000":
        assert got["var"][6] == 0.0 and np.all(got["quant"][:, 6] == 2.5) and got["min"][6] == got["max"][6] == 2.5      # the constant column
    if name == "T_tie":
        assert got["quant"][0, 0] == np.sort(c.x[:, 0])[499]
    if name.startswith("K_"):
        assert got["bestfit_row"] == {"K_ties": 33, "K_last": 1024, "K_minus_inf": 3}[name]


def test_status_cases_fail_alone(singles):
    good = sc.gpu_cases()["B_513_8"]
    for name, a, x, f, status, column in sc.status_cases():
        got = measure([sys_of(good), (a, x, x.shape[1], f), sys_of(good)])
        assert got[0].tobytes() == singles["B_513_8"].tobytes() == got[2].tobytes(), name
        from mcevidence_amd import summary
        bad = summary.from_block(got[1], x.shape[1], len(sc.TARGETS))
        assert (bad["status"], bad["column"]) == (status, column) and bad["rows"] == int(np.count_nonzero(a != 0)) and bad["bestfit_row"] == -1, (name, bad)
        assert all(np.isnan(bad[k]).all() for k in ("W", "A2", "bestfit_f", "mean", "var", "min", "max", "bestfit", "quant")), (name, bad)
        assert measure([(a, x, x.shape[1], f)])[0].tobytes() == got[1].tobytes(), name


def test_five_systems_of_three_shapes_in_three_orders(singles):
    names = ["A_unit", "B_1025_27", "D_zeros", "B_513_127", "L_4100"]          # (d, ld): (8, 8), (27, 29), (5, 5), (127, 129), (8, 8)
    g = sc.gpu_cases()
    empty = (np.zeros(0), np.zeros((0, 3)), 3, np.zeros(0))
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        systems = [sys_of(g[names[i]]) for i in order]
        systems.insert(2, empty)
        got = measure(systems)
        assert got[2][3] == 5 and got[2][2] == 0           # the empty segment: status 5, no rows
        del got[2]
        for i, block in zip(order, got):
            assert block.tobytes() == singles[names[i]].tobytes(), (order, names[i])


def test_two_runs_the_host_pointer_form_small_passes_and_no_fs(singles):
    from mcevidence_amd import _capi, summary
    g = sc.gpu_cases()
    for name in ("B_512_8", "C_narrow", "L_4100"):
        assert measure([sys_of(g[name])])[0].tobytes() == singles[name].tobytes(), name
    cases = [g[n] for n in ("A_unit", "B_513_27", "D_zeros")]
    host = _capi.param_summary([c.system for c in cases] + [(np.zeros((0, 2)), 2, np.zeros(0), None)], sc.TARGETS)
    for c, block in zip(cases, host):
        assert np.array(block).tobytes() == singles[c.name].tobytes(), c.name
    assert host[3][3] == 5
    # passes of 1024 elements on a 4100 x 8 system: every column a pass of its own; and passes that hold several runs and end inside
    # a system
    for pe in (1024, 4100 * 3, 5000):
        got = measure([sys_of(g["L_4100"]), sys_of(g["B_511_8"])], pass_elems=pe)
        assert got[0].tobytes() == singles["L_4100"].tobytes() and got[1].tobytes() == singles["B_511_8"].tobytes(), pe
    # fs = NULL: the best-fit entries are NaN / -1 and nothing else changes
    c = g["B_1025_8"]
    got = as_dict(measure([(c.a, c.x, c.d, None)])[0], c)
    ref = as_dict(singles["B_1025_8"], c)
    assert got["bestfit_row"] == -1 and math.isnan(got["bestfit_f"]) and np.isnan(got["bestfit"]).all()
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(ref[k])) for k in ("W", "A2", "rows", "status", "column", "mean", "var", "min", "max", "quant"))
    assert summary.build(got, (0.68, 0.95), 0.0)["bestfit_row"] == -1


def same_dict(a, b):
    return set(a) == set(b) and all(
        same_dict(a[k], b[k]) if isinstance(a[k], dict) else np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=not isinstance(a[k], (list, tuple, str)))
        for k in a)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("summary_roots")
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
def test_resident_route_with_summary(roots, thin, jackknife):
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import PLANCK_PARAMS
    root = roots["p21"]
    kw = dict(kmax=3, verbose=0, thinlen=thin, **({} if jackknife is None else {"jackknife": jackknife}))
    lnE, info = pkg.evidence_from_files(root, summary=True, info=True, require_resident=True, **kw)
    host = pkg.MCEvidence(root, summary=True, **kw)
    hostE, hinfo = host.evidence(info=True)
    part = host.gd.data["s1"]
    logL = -np.asarray(part.loglikes, dtype=np.float64)
    a, x = np.asarray(part.adjusted_weights, dtype=np.float64), np.asarray(part.samples, dtype=np.float64)
    if thin == 0:                                          # the rows are the files' own: raw, not whitened
        rows = np.concatenate([np.loadtxt(root + "_%d.txt" % i) for i in (1, 2, 3, 4)])
        assert np.array_equal(x, rows[:, 2:]) and np.array_equal(a, rows[:, 0])
    case = sc.Case("resident thin=%s jackknife=%s" % (thin, jackknife), a, x, logL - logL.max())
    d, h = info["summary"], hinfo["summary"]
    for what, s in (("resident", d), ("host    ", h)):
        sc.check(case, sc.block_of(s, case.exact["bestfit_f"]), what)
        assert s["bestfit_loglike"] == logL.max() + case.exact["bestfit_f"] and np.all(np.abs(s["sd"] - np.sqrt(s["var"])) <= 2 * sc.EPS * s["sd"])
        assert s["names"][:3] == [p[0] for p in PLANCK_PARAMS][:3] and len(s["names"]) == x.shape[1] and "sigma" not in s
    # quantiles, min, max and the best fit are the host route's (the weights are integers: every sum is exact)
    assert np.all(a == np.floor(a))
    for k in ("median", "lower", "upper", "min", "max", "bestfit", "bestfit_row", "rows", "sum_w", "status", "column"):
        assert np.array_equal(np.asarray(d[k]), np.asarray(h[k])), k
    assert info["route"] == "resident" and ("jackknife" in info) == (jackknife is not None)
    # ln E is bit for bit what the route returns without the keyword
    lnE0, info0 = pkg.evidence_from_files(root, info=True, require_resident=True, **kw)
    untimed = lambda inf: {k: ({j: u for j, u in v.items() if j != "kernel_ms"} if isinstance(v, dict) else v) for k, v in inf.items() if k != "summary"}      # noqa: E731
    assert np.array_equal(lnE, lnE0) and "summary" not in info0 and same_dict(untimed(info), untimed(info0))


def test_farm_measures_every_root_as_its_own_resident_run(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p21", "p9", "bad", "p21b", "p21"]           # two (ncols, ndim) shapes, a root whose status is 3, a thinned root
    thins = [0, 0, 0, 0, 3]
    outs = pkg.evidence_many_from_files([roots[n] for n in names], summary=True, thinlen=thins, kmax=3, info=True)
    assert [o[1]["route"] for o in outs] == ["farm"] * 5 and farm.LAST_STATS["counts"]["farm"] == 5
    for n, t, (lnE, info) in zip(names, thins, outs):
        own = pkg.evidence_from_files(roots[n], summary=True, thinlen=t, kmax=3, verbose=0, info=True, require_resident=True)
        assert same_dict(info["summary"], own[1]["summary"]), (n, info["summary"], own[1]["summary"])
        assert np.array_equal(lnE, own[0]), n
        assert info["summary"]["status"] == (3 if n == "bad" else 0), n
    bad = outs[2][1]["summary"]
    assert np.isnan(bad["mean"]).all() and np.isnan(bad["upper"]).all() and bad["column"] == -1 and np.all(np.isfinite(outs[2][0]))
    # the other roots are unaffected by the failing one; without the keyword ln E keeps its bits
    rest = [i for i in range(5) if i != 2]
    without = pkg.evidence_many_from_files([roots[names[i]] for i in rest], summary=True, thinlen=[thins[i] for i in rest], kmax=3, info=True)
    for i, o in zip(rest, without):
        assert same_dict(outs[i][1]["summary"], o[1]["summary"]) and np.array_equal(outs[i][0], o[0]), names[i]
    plain = pkg.evidence_many_from_files([roots[n] for n in names], thinlen=thins, kmax=3, info=True)
    for a, p in zip(outs, plain):
        assert np.array_equal(a[0], p[0]) and "summary" not in p[1]
    mixed = pkg.evidence_many_from_files([roots["p21"], roots["p9"]], summary=[(0.9,), None], kmax=3, info=True)
    assert mixed[0][1]["summary"]["probs"] == (0.9,) and mixed[0][1]["summary"]["lower"].shape == (1, 21) and "summary" not in mixed[1][1]


def test_command_line_on_the_resident_route_and_the_farm(tmp_path, capsys, caplog):
    import logging

    from mcevidence_amd import cli
    from mcevidence_amd.synth import gaussian_chain, write_cosmomc_chains
    root = str(tmp_path / "run")
    write_cosmomc_chains(root, [gaussian_chain(seed=30 + i, n=600, d=3, weights="int") for i in range(3)], [("om%d" % j, -6.0, 6.0) for j in range(3)], fmt="%.17g")
    args = [root, "-k", "3", "--allparams", "--resident", "--summary", "--jackknife=4"]
    # -vb 0: the CLI prints the lines once, before the ln(B) lines it prints
    cli.main(args + ["-vb", "0"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    at = {key: [i for i, ln in enumerate(out) if ln.startswith(key)] for key in ("summary: parameter", "summary: p0", "summary: p2", "ln(B)[k=1] =")}
    assert all(len(v) == 1 for v in at.values()), (at, out)
    assert at["summary: parameter"][0] < at["summary: p0"][0] < at["summary: p2"][0] < at["ln(B)[k=1] ="][0]
    # -vb 1: the route logs them, the CLI does not print them a second time
    with caplog.at_level(logging.INFO, logger="mcevidence_amd"):
        cli.main(args + ["-vb", "1"])
    printed = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    msgs = [r.getMessage().strip() for r in caplog.records]
    assert not any(ln.startswith("summary:") for ln in printed) and sum(m.startswith("summary: parameter") for m in msgs) == 1
    # the farm prints them for every root
    lst = tmp_path / "roots.txt"
    lst.write_text("%s\n%s   # twice\n" % (root, root))
    cli.main([str(lst), "-k", "3", "--allparams", "--farm", "--summary", "0.9", "-vb", "0"])
    out = [ln.strip() for ln in capsys.readouterr().out.splitlines()]
    assert sum(ln.startswith("summary: parameter") for ln in out) == 2 and sum(ln.startswith("ln(B)[k=1] =") for ln in out) == 2
    assert all("lower90" in ln for ln in out if ln.startswith("summary: parameter"))
    assert max(i for i, ln in enumerate(out) if ln.startswith("summary:")) < max(i for i, ln in enumerate(out) if ln.startswith("ln(B)[k=1] ="))
