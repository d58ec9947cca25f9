"""The jackknife of the resident route and the farm on the GPU (docs/design/jackknife_resident.md): mce_jack_groups_dev against NumPy,
exactly; mce_jack_leave_out_dev against the exact rational model of tests/moments_cases.py applied to every deleted set, within the
bound of docs/design/information.md at that set's own n; ``evidence_from_files(root, jackknife=...)`` against the host route's
``MCEvidence(root, jackknife=...)`` within LNE_TOL (the tolerance docs/design/jackknife.md uses for ln E per group); the farm against the
per-root resident run, bit for bit.  Shapes are small on purpose; every test takes a few seconds."""
import numpy as np
import pytest

import jack_cases as jc
import moments_cases as mc
from helpers import LNE_TOL
from test_jackknife_resident_shared import check_slot, leave_out_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from mcevidence_amd import _capi
    _capi.require_device()
    return _capi


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def groups_on_device(capi, systems):
    """[(rows or None, src or None, part_first or None, n, N, G, by)] in ONE call -> one int32 array per system"""
    import torch
    keep, segs = [], []
    for rows, src, first, n, N, G, by in systems:
        t = (None if rows is None else _dev(rows, np.int64), None if src is None else _dev(src, np.int64), torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda:0"))
        keep.append(t)
        segs.append((0 if t[0] is None else t[0].data_ptr(), 0 if t[1] is None else t[1].data_ptr(), first, n, N, G, by, t[2].data_ptr()))
    torch.cuda.synchronize()
    capi.jack_groups_dev(segs)
    return [t[2][:s[3]].cpu().numpy() for t, s in zip(keep, systems)]


def measure(capi, systems):
    """[(w, fs or None, g, G)] in ONE mce_jack_leave_out_dev call -> one [G + 1, 8] block per system"""
    import torch
    keep, segs = [], []
    for w, f, g, G in systems:
        n = len(w)
        t = (_dev(w, np.float64), None if f is None else _dev(f, np.float64), _dev(g, np.int32))
        keep.append(t)
        segs.append((t[0].data_ptr() if n else 0, t[1].data_ptr() if n and f is not None else 0, t[2].data_ptr() if n else 0, n, G))
    wsb = capi.jack_leave_out_workspace_bytes(sum(len(s[0]) for s in systems), len(systems), max(s[3] for s in systems))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return capi.jack_leave_out_dev(segs, ws.data_ptr(), wsb)


# ------------------------------------------------------------------------------------------------------------------------ group ids
def test_group_ids_are_numpys(capi):
    rng = np.random.default_rng(5)
    systems, want = [], []
    for n in (1, 255, 256, 257, 513):
        for G in (2, 16, 64):
            perm = rng.permutation(n)
            systems.append((None, None, None, n, n, G, "blocks"))
            want.append((np.arange(n, dtype=np.int64) * G // n).astype(np.int32))
            systems.append((perm, None, None, n, n, G, "blocks"))
            want.append((perm.astype(np.int64) * G // n).astype(np.int32))
    lens = [300, 0, 57, 401]                                         # four parts of unequal length, one of them empty
    first = np.concatenate([[0], np.cumsum(lens)])[:4]
    chain = np.repeat(np.arange(4), lens)
    nb = sum(lens)
    systems.append((None, None, first, nb, nb, 4, "chains"))
    want.append(chain.astype(np.int32))
    src = np.sort(rng.permutation(nb)[:333])                         # a thinned sample: the kept rows in the burned, concatenated numbering
    systems.append((None, src, first, 333, 333, 4, "chains"))
    want.append(chain[src].astype(np.int32))
    got = groups_on_device(capi, systems)                            # every system in one launch
    for s, g, w in zip(systems, got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), s[3:]
    # each system alone gives the same ids; a row outside the sample has no group
    for s, w in zip(systems[::7], want[::7]):
        assert np.array_equal(groups_on_device(capi, [s])[0], w)
    bad, = groups_on_device(capi, [(np.array([0, 7, -1, 3]), None, None, 4, 7, 2, "blocks")])
    assert list(bad) == [0, -1, -1, 0]


# -------------------------------------------------------------------------------------------------------------------- leave-out blocks
@pytest.fixture(scope="module")
def singles(capi):
    """every case's block from a call of its own, computed once"""
    return {name: measure(capi, [(a, f, g, G)])[0] for name, a, f, g, G in leave_out_cases()}


def test_leave_out_blocks_within_the_bound_of_the_exact_model(singles):
    worst = 0.0
    for name, a, f, g, G in leave_out_cases():
        block = singles[name]
        assert block.shape == (G + 1, 8)
        err = max(check_slot(name, b, block[b + 1], a, f, g != b) for b in range(-1, G))
        print("%-20s n=%-5d G=%-2d largest error / bound over the slots %.3g" % (name, len(a), G, err))
        worst = max(worst, err)
    print("largest error / bound: %.3g" % worst)
    # a group without rows: its slot equals the full slot bit for bit
    assert singles["B_1025_empty_group"][1 + 3].tobytes() == singles["B_1025_empty_group"][0].tobytes()


def test_leave_out_slots_fail_alone(capi):
    c = mc.BY_NAME["A_unit"]
    n, G = len(c.a), 4
    g = (np.arange(n) * G // n).astype(np.int32)
    # group 1 holds every used row; the zero weights lie over -inf and NaN, which are never read into a sum
    a = np.where(g == 1, c.a, 0.0)
    f = np.where(g == 1, c.f, np.where(np.arange(n) % 2 == 0, -np.inf, np.nan))
    block, = measure(capi, [(a, f, g, G)])
    assert block[2, 7] == 5 and np.isnan(block[2, 2:6]).all() and block[2, 6] == 0 and block[2, 0] == (g != 1).sum() and block[2, 1] == 0.0
    for b in (-1, 0, 2, 3):
        check_slot("all_in_one_group", b, block[b + 1], a, f, g != b)
    # a -inf likelihood on a used row of group 2: every slot that keeps the row has status 3, the slot that deletes it is good
    f3 = c.f.copy()
    f3[int(np.flatnonzero(g == 2)[5])] = -np.inf
    block, = measure(capi, [(c.a, f3, g, G)])
    assert [int(s) for s in block[:, 7]] == [3, 3, 3, 0, 3] and np.isnan(block[[0, 1, 2, 4], 2:6]).all()
    check_slot("minus_inf", 2, block[3], c.a, f3, g != 2)
    # without an fs column: rows and SumW, the same bits, and no moments
    with_f, = measure(capi, [(c.a, c.f, g, G)])
    without, = measure(capi, [(c.a, None, g, G)])
    assert without[:, :2].tobytes() == with_f[:, :2].tobytes() and np.isnan(without[:, 2:7]).all() and (without[:, 7] == -1).all()
    # a group id outside [0, G) is an argument error, as in mce_jack_dotp_dev
    gbad = g.copy()
    gbad[n - 1] = G
    with pytest.raises(ValueError, match="a group id outside"):
        measure(capi, [(c.a, c.f, gbad, G)])
    gbad[n - 1] = -1
    with pytest.raises(ValueError, match="a group id outside"):
        measure(capi, [(c.a, c.f, g, G), (c.a, None, gbad, G)])


def test_systems_do_not_depend_on_their_neighbours(capi, singles):
    cases = {c[0]: c for c in leave_out_cases()}
    names = ["B_511_blocks", "B_1025_permuted", "D_zeros_blocks", "E_negative_blocks", "B_513_blocks"]
    empty = (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32), 3)
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        systems = [cases[names[i]][1:] for i in order]
        systems.insert(2, empty)
        got = measure(capi, systems)
        assert got[2].shape == (4, 8) and (got[2][:, 0] == 0).all() and (got[2][:, 1] == 0).all()
        del got[2]
        for i, block in zip(order, got):
            assert block.tobytes() == singles[names[i]].tobytes(), (order, names[i])


def test_two_runs_and_the_host_pointer_form(capi, singles):
    cases = {c[0]: c for c in leave_out_cases()}
    for name in ("B_512_blocks", "C_narrow_blocks", "B_1025_permuted"):
        assert measure(capi, [cases[name][1:]])[0].tobytes() == singles[name].tobytes(), name
    names = ["B_513_blocks", "D_zeros_blocks", "B_1025_empty_group"]
    host = capi.jack_leave_out([cases[n][1:] for n in names] + [(np.zeros(0), None, np.zeros(0, dtype=np.int32), 2)])
    for n, block in zip(names, host):
        assert block.tobytes() == singles[n].tobytes(), n
    assert host[3].shape == (3, 8) and (host[3][:, 0] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------- the resident route
@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    d = tmp_path_factory.mktemp("jackknife_roots")
    out = {}
    for name, seed, rows, nnuis in (("p9", 51, (300, 260, 320, 280), 3), ("p7", 52, (250, 270, 240), 1)):
        out[name] = str(d / name)
        write_cosmomc_chains(out[name], planck_like_chains(seed=seed, rows=rows, nnuis=nnuis)[0], None, fmt="%.17g")
    # jack_cases' capacity case as two files, one per group: with by="chains" the row at the centre of the other chain's 1100
    # near-identical rows stays short after the last rung
    c = jc.case_capacity()
    out["capacity"] = str(d / "capacity")
    write_cosmomc_chains(out["capacity"], [np.column_stack([c["w"], -c["fs"], c["X"]])[c["gq"] == b] for b in (0, 1)], None, fmt="%.17g")
    return out


NUMERIC = ("lnE", "sigma", "lnE_groups", "lnE_bias_corrected")


def same_jackknife(a, b):
    """bit for bit, apart from the device times"""
    return (set(a) - {"kernel_ms"} == set(b) - {"kernel_ms"} and all(np.array_equal(a[k], b[k]) for k in NUMERIC)
            and all(a[k] == b[k] for k in ("groups", "by", "rows_per_level")))


@pytest.mark.parametrize("jack, thin", [(8, 0), ({"by": "chains"}, 0), (8, 2), ({"by": "chains"}, 2)])
def test_resident_route_against_the_host_route(roots, jack, thin):
    import mcevidence_amd as pkg
    from mcevidence_amd.jackknife import summarise
    root = roots["p9"]
    kw = dict(kmax=3, ndim=6, verbose=0, thinlen=thin)
    lnE, info = pkg.evidence_from_files(root, jackknife=jack, info=True, require_resident=True, **kw)
    host = pkg.MCEvidence(root, jackknife=jack, **kw)
    hostE, hinfo = host.evidence(info=True)
    got, want = info["jackknife"], hinfo["jackknife"]
    assert info["route"] == "resident" and set(got) == set(want)
    G = 4 if isinstance(jack, dict) else 8
    assert got["groups"] == want["groups"] == G and got["by"] == want["by"] and got["lnE_groups"].shape == (G, 2)
    for k in ("lnE_groups", "lnE"):
        err = float(np.max(np.abs(got[k] - want[k])))
        print("%s thin=%s %-10s max difference from the host route %.3e" % (jack, thin, k, err))
        assert err <= LNE_TOL, (k, err)
    assert np.max(np.abs(got["lnE"] - lnE)) <= LNE_TOL
    sigma, bc = summarise(got["lnE"], got["lnE_groups"])
    assert np.array_equal(got["sigma"], sigma) and np.array_equal(got["lnE_bias_corrected"], bc) and np.all(sigma > 0)
    assert got["rows_per_level"] == want["rows_per_level"]
    # the returned ln E is bit for bit what the route returns without the keyword, and nothing else in the info dict moves
    lnE0, info0 = pkg.evidence_from_files(root, info=True, require_resident=True, **kw)
    assert np.array_equal(lnE, lnE0) and "jackknife" not in info0 and {k: v for k, v in info.items() if k != "jackknife"} == info0


def test_resident_route_with_information(roots):
    from mcevidence_amd.jackknife import summarise
    from mcevidence_amd.resident import ResidentChains
    root, G = roots["p9"], 8
    rows = np.concatenate([np.loadtxt(root + "_%d.txt" % i) for i in (1, 2, 3, 4)])
    rc = ResidentChains.from_files(root)
    lnE, info = rc.evidence(kmax=3, ndim=6, information=True, jackknife=G, info=True)
    d, jk = info["information"], info["jackknife"]
    assert d["groups"] == G and d["by"] == "blocks" and set(d["sigma"]) == {"mean_logL", "bmd", "D_KL"}
    a, logL = rows[:, 0], -rows[:, 1]
    f, n = logL - logL.max(), len(rows)
    gq = (np.arange(n, dtype=np.int64) * G // n).astype(np.int32)
    block = rc.jackknife_block
    assert block.shape == (G + 1, 8)
    mean_b, bmd_b, dkl_b = [], [], []
    for b in range(-1, G):
        err = check_slot("resident", b, block[b + 1], a, f, gq != b)
        print("slot %2d n=%d error / bound %.3g" % (b, int(block[b + 1, 0]), err))
        if b >= 0:
            ex = mc.exact(a[gq != b], f[gq != b])
            mean_b.append([logL.max() + ex["c"]])
            bmd_b.append([2 * ex["v"]])
            dkl_b.append(logL.max() + ex["c"] - jk["lnE_groups"][b])
    for key, full, vals in (("mean_logL", [d["mean_logL"]], mean_b), ("bmd", [d["bmd"]], bmd_b), ("D_KL", d["D_KL"], dkl_b)):
        want = summarise(np.asarray(full), np.asarray(vals))[0]
        assert np.allclose(np.atleast_1d(d["sigma"][key]), want, rtol=1e-9, atol=0), (key, d["sigma"][key], want)
        assert np.all(want > 0)
    # without the jackknife the information dict keeps its bits, and ln E keeps them in any case
    lnE1, info1 = ResidentChains.from_files(root).evidence(kmax=3, ndim=6, information=True, info=True)
    assert np.array_equal(lnE, lnE1) and {k: v for k, v in d.items() if k not in ("sigma", "groups", "by")}.keys() == info1["information"].keys()
    assert all(np.array_equal(d[k], info1["information"][k]) for k in info1["information"])


def test_declines_and_errors_on_the_device_routes(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd.resident import REASONS
    np.random.seed(3)
    lnE, info = pkg.evidence_from_files(roots["p9"], jackknife=4, split=True, kmax=3, ndim=6, verbose=0, info=True)
    assert info["route"] == "host" and info["declined"] == REASONS["jackknife_cross"] and info["jackknife"]["lnE_groups"].shape[0] == 4
    with pytest.raises(ValueError, match=REASONS["jackknife_cross"]):
        pkg.evidence_from_files(roots["p9"], jackknife=4, split=True, kmax=3, ndim=6, verbose=0, require_resident=True)
    with pytest.raises(ValueError, match=r"jackknife: G=65 groups \(2 \.\. 64 expected\)"):
        pkg.evidence_from_files(roots["p9"], jackknife=65, kmax=3, ndim=6, verbose=0)
    with pytest.raises(ValueError, match=r"jackknife by='chains' needs at least 2 chains \(got 1\)"):
        pkg.evidence_from_files(roots["p9"] + "_1.txt", jackknife={"by": "chains"}, kmax=3, ndim=6, verbose=0)
    with pytest.raises(ValueError, match=r"1 row still short after lists of 1024"):
        pkg.evidence_from_files(roots["capacity"], jackknife={"by": "chains"}, kmax=5, verbose=0, require_resident=True)


# ------------------------------------------------------------------------------------------------------------------------------ the farm
def test_farm_gives_every_root_its_own_resident_run(roots):
    import mcevidence_amd as pkg
    from mcevidence_amd import farm
    names = ["p9", "p7", "p9", "p7", "capacity"]          # two (ncols, ndim) shapes, a thinned root, one asking for nothing, one whose ladder raises
    thins = [0, 0, 2, 0, 0]
    jacks = [8, {"groups": 4}, 8, None, {"by": "chains"}]
    ndims = [6, None, 6, None, None]
    kw = dict(kmax=5, info=True)
    outs = pkg.evidence_many_from_files([roots[n] for n in names], jackknife=jacks, thinlen=thins, ndim=ndims, information=[True, None, None, None, None],
                                        return_exceptions=True, **kw)
    assert isinstance(outs[4], ValueError) and "1 row still short after lists of 1024" in str(outs[4])
    assert [o[1]["route"] for o in outs[:4]] == ["farm"] * 4 and farm.LAST_STATS["counts"]["farm"] == 4
    assert "jackknife" not in outs[3][1]
    for i in (0, 1, 2):
        own = pkg.evidence_from_files(roots[names[i]], jackknife=jacks[i], thinlen=thins[i], ndim=ndims[i], information=True if i == 0 else None, verbose=0,
                                      require_resident=True, **kw)
        assert np.array_equal(outs[i][0], own[0]), names[i]
        assert same_jackknife(outs[i][1]["jackknife"], own[1]["jackknife"]), (names[i], outs[i][1]["jackknife"], own[1]["jackknife"])
    a, b = outs[0][1]["information"], pkg.evidence_from_files(roots["p9"], jackknife=8, ndim=6, information=True, verbose=0, **kw)[1]["information"]
    assert a["groups"] == 8 and all(np.array_equal(a["sigma"][k], b["sigma"][k]) for k in ("mean_logL", "bmd", "D_KL"))
    # the failing root raises where exceptions are not collected, and without the keyword ln E keeps its bits
    with pytest.raises(ValueError, match="still short"):
        pkg.evidence_many_from_files([roots["p7"], roots["capacity"]], jackknife=[None, {"by": "chains"}], **kw)
    plain = pkg.evidence_many_from_files([roots[n] for n in names[:4]], thinlen=thins[:4], ndim=ndims[:4], **kw)
    for i in range(4):
        assert np.array_equal(outs[i][0], plain[i][0]) and "jackknife" not in plain[i][1]
