"""The resident farm (mcevidence_amd/farm.py: the files of many roots parsed per wave -> segmented preparation -> one batched
device-source feed) against the host reader, the per-root resident route, the host route and the reference's own pins.  Every
comparison of a result asserts ``route == "farm"`` first, so a fallback cannot pass for the feature.

Spans: the reader's tile is 4 096 bytes and its single-block scans run 1 024 threads (more than 1 024 tiles: a thread owns two);
the preparation's tile is 512 rows, counted from each root's first row."""
import os

import numpy as np
import pytest

import mcevidence_amd as pkg
from mcevidence_amd import _capi, chain_io, farm, resident
from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
from helpers import host_pins
from farm_cases import TILE, boundary_files

pytestmark = pytest.mark.gpu

PINS = host_pins()
LNE_PARITY = 1e-9           # the project's stated parity bound on ln E (tests/helpers.py: LNE_TOL)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def wave_bytes_for(sizes, k):
    """the smallest multiple of a tile for which ``farm_waves`` makes exactly ``k`` waves"""
    for wb in range(TILE, sum(sizes) + 2 * TILE, TILE):
        if len(farm.farm_waves(sizes, wb)) == k:
            return wb
    raise AssertionError("no wave size gives %d waves" % k)


# ---------------------------------------------------------------------------------------------------------------- 1. reader boundaries
@pytest.fixture(scope="module")
def boundary(tmp_path_factory):
    td = tmp_path_factory.mktemp("boundary")
    paths = []
    for name, data in boundary_files():
        p = os.path.join(str(td), name + ".txt")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    want = [chain_io.loadtxt(p) for p in paths]          # computed once, shared, never modified
    return paths, want


def test_reader_boundaries_one_wave(boundary):
    paths, want = boundary
    sizes = [farm.farm_layout([os.path.getsize(p)])[1] for p in paths]
    assert sum(sizes) // TILE > 1024                      # a scan thread owns more than one tile
    assert sorted({w.shape[1] for w in want if w.shape[0]} & {3, 5, 23}) == [3, 5, 23]
    got = farm.read_files(paths, wave_bytes=sum(sizes))
    st = farm.handle_stats()
    assert st["files"] >= len(paths) and st["patched"] > 0          # (the TOKENS files: inf, nan, long tails are patched on the host)
    for p, g, w in zip(paths, got, want):
        assert not isinstance(g, Exception), (p, g)
        assert same(g, w), p


@pytest.mark.parametrize("nwaves", [1, 2, 5])
def test_reader_boundaries_any_order_any_wave_split(boundary, nwaves):
    paths, want = boundary
    order = np.random.default_rng(nwaves).permutation(len(paths))
    sizes = [farm.farm_layout([os.path.getsize(paths[i])])[1] for i in order]
    wb = wave_bytes_for(sizes, nwaves)
    got = farm.read_files([paths[i] for i in order], wave_bytes=wb)
    for i, g in zip(order, got):
        assert not isinstance(g, Exception), (paths[i], g)
        assert same(g, want[i]), paths[i]


# ---------------------------------------------------------------------------------------------------------------- shared roots
@pytest.fixture(scope="module")
def small_roots(tmp_path_factory):
    """six small roots of 1-4 files (300-3 000 rows each), a negated copy of the first, and the C1 stand-in"""
    td = str(tmp_path_factory.mktemp("farm"))
    roots = []
    for k, rows in enumerate([(900, 700), (1500,), (600, 500, 400, 300), (1200, 1100, 900), (2000, 1000), (800, 800)]):
        chs, _, ranges = planck_like_chains(seed=20 + k, rows=rows, nnuis=3 + k)
        root = os.path.join(td, "r%d" % k)
        write_cosmomc_chains(root, chs, ranges)
        roots.append(root)
    neg = [c.copy() for c in planck_like_chains(seed=20, rows=(900, 700), nnuis=3)[0]]
    for c in neg:
        c[:, 1] = -c[:, 1]
    rootn = os.path.join(td, "neg")
    write_cosmomc_chains(rootn, neg, None)
    chs, _, ranges = planck_like_chains(seed=1)
    c1 = os.path.join(td, "base_plikHM_TT_lowTEB")
    write_cosmomc_chains(c1, chs, ranges)
    return dict(roots=roots, negated=rootn, c1=c1, dir=td)


def routes(out):
    return [o[1]["route"] for o in out]


# ---------------------------------------------------------------------------------------------------------------- 2. per-file failure
def test_a_ragged_file_and_a_junk_field_fail_their_roots_only(small_roots, tmp_path):
    good = small_roots["roots"][:4]
    bad = []
    for name in ("ragged", "junk"):
        chs = planck_like_chains(seed=31, rows=(400, 300), nnuis=2)[0]
        root = str(tmp_path / name)
        write_cosmomc_chains(root, chs, None)
        with open(root + "_2.txt", "ab") as f:            # the second file of the root goes wrong near its end
            f.write(b"1 2 3\n" if name == "ragged" else b"1 2 3 4 abc 6 7 8 9 10\n")       # (the files have 10 columns)
        bad.append(root)
    alone = pkg.evidence_many_from_files(good, kmax=3, ndim=6, info=True)
    assert routes(alone) == ["farm"] * 4
    mixed = pkg.evidence_many_from_files([good[0], bad[0], good[1], good[2], bad[1], good[3]], kmax=3, ndim=6, info=True, return_exceptions=True)
    for slot, root in ((1, bad[0]), (4, bad[1])):
        with pytest.raises(ValueError) as host:
            chain_io.loadtxt(root + "_2.txt")
        assert isinstance(mixed[slot], ValueError) and str(mixed[slot]) == str(host.value)
    for a, m in zip(alone, [mixed[0], mixed[2], mixed[3], mixed[5]]):
        assert m[1]["route"] == "farm" and same(a[0], m[0])
    with pytest.raises(ValueError) as first:              # the first failing root in input order raises
        pkg.evidence_many_from_files([good[0], bad[1], bad[0]], kmax=3, ndim=6)
    assert str(first.value) == str(mixed[4])


# ---------------------------------------------------------------------------------------------------------------- 3. preparation
PREP_ROOTS = [       # (columns, rows per file, burn-in, rows left)
    (5, (1011,), 500, 511),
    (7, (700, 812), 500, 512),
    (9, (600, 300, 913), 500, 513),                  # the burn-in lies beyond the end of the second file
    (12, (800, 800, 800, 625), 500, 1025),
    (6, (730,), 0.3, 511),
    (8, (400, 331), 0.3, 512),
    (10, (513,), 0, 513),
    (5, (512, 513), 0, 1025),
    (23, (300, 211), 0, 511),
]


def per_root_reference(rc, ncols):
    """what the per-root calls (gather, mce_chain_reduce_dev) prepare for the resident chain ``rc``"""
    import torch
    n = rc.nrows
    s1 = rc._gather(None, want=("params", "w", "like"))
    fs = torch.empty(n, dtype=torch.float64, device="cuda:0")
    wsb = _capi.chain_reduce_workspace_bytes(n)
    ws = rc._ws(wsb)
    scal = _capi.chain_reduce_dev(s1["like"].data_ptr(), s1["w"].data_ptr(), n, False, fs.data_ptr(), ws.data_ptr(), wsb, rc._stream())
    return dict(rc=rc, ncols=ncols, n=n, params=s1["params"].cpu().numpy(), w=s1["w"].cpu().numpy(), fs=fs.cpu().numpy(), scal=scal)


@pytest.fixture(scope="module")
def prep_reference(tmp_path_factory):
    """per root: the resident chain and what ResidentChains prepares for it (parameters, weights, fs, max(logL), SumW), once"""
    td = str(tmp_path_factory.mktemp("prep"))
    rng = np.random.default_rng(5)
    ref = []
    for k, (ncols, rows, burn, left) in enumerate(PREP_ROOTS):
        chs = [np.column_stack([1.0 + rng.poisson(3.0, n), 50.0 + rng.random(n) * 20.0, rng.standard_normal((n, ncols - 2))]) for n in rows]
        root = os.path.join(td, "p%d" % k)
        write_cosmomc_chains(root, chs, None, fmt="%.17g")
        rc = pkg.ResidentChains.from_files(root, burnlen=burn)
        assert rc.nrows == left
        ref.append(per_root_reference(rc, ncols))
    return ref


def farm_prep(ref, order):
    import torch
    sel = [ref[i] for i in order]
    parts = [p for r in sel for p in r["rc"]._parts]
    n = sum(r["n"] for r in sel)
    dev = "cuda:0"
    params = torch.full((sum(r["n"] * (r["ncols"] - 2) for r in sel),), -7.0, dtype=torch.float64, device=dev)
    w, like, fs = (torch.full((n,), -7.0, dtype=torch.float64, device=dev) for _ in range(3))
    wsb = _capi.chain_farm_prep_workspace_bytes(len(sel), len(parts), n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    scal = _capi.chain_farm_prep_dev([len(r["rc"]._parts) for r in sel], [r["ncols"] for r in sel], parts, 0, 1, 2, False, params.data_ptr(),
                                     w.data_ptr(), like.data_ptr(), fs.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    params, w, fs = params.cpu().numpy(), w.cpu().numpy(), fs.cpu().numpy()
    out, r0, p0 = {}, 0, 0
    for k, (i, r) in enumerate(zip(order, sel)):
        npar = r["n"] * (r["ncols"] - 2)
        out[i] = dict(params=params[p0:p0 + npar].reshape(r["n"], -1), w=w[r0:r0 + r["n"]], fs=fs[r0:r0 + r["n"]], scal=tuple(scal[k]))
        r0 += r["n"]
        p0 += npar
    return out


@pytest.mark.parametrize("order", [list(range(9)), list(range(8, -1, -1)), [4, 0, 8, 2], [3], [7, 1, 5, 6, 3]])
def test_segmented_preparation_equals_the_per_root_calls_bitwise(prep_reference, order):
    """9 roots of 1-4 files and 3-21 parameters, 511 / 512 / 513 / 1 025 rows after a fractional or absolute burn-in: parameters,
    weights, fs, max(logL) and SumW bitwise what the per-root calls give, whatever the order and the subset (the wave) a root is in"""
    got = farm_prep(prep_reference, order)
    for i in order:
        r, g = prep_reference[i], got[i]
        assert same(g["params"], r["params"]) and same(g["w"], r["w"]) and same(g["fs"], r["fs"]), i
        assert same(np.array(g["scal"][:2]), np.array(r["scal"][:2])) and g["scal"][2:] == (0.0, 0.0) and tuple(r["scal"][2:]) == (0, 0), i


def test_segmented_preparation_counts_bad_rows_per_root_bitwise():
    """three roots of 511 / 513 / 1 025 rows after a burn-in of 100 (a partial tile, a tile and a row, two tiles and a row), uploaded
    as arrays so that no reader is involved: a NaN likelihood in the last row of the second, an infinite weight in row 512 of the
    third.  Per root max(logL), SumW, both bad counts, fs, weights and parameters are bitwise what mce_chain_reduce_dev gives the
    root alone, and the clean root is bitwise what it is in a wave of its own"""
    rng = np.random.default_rng(11)
    burn, ncols = 100, 6
    chs = [np.column_stack([1.0 + rng.poisson(3.0, n), 50.0 + rng.random(n) * 20.0, rng.standard_normal((n, ncols - 2))]) for n in (611, 613, 1125)]
    chs[1][-1, 1] = np.nan
    chs[2][burn + 512, 0] = np.inf
    ref = [per_root_reference(pkg.ResidentChains.from_arrays([a], burnlen=burn), ncols) for a in chs]
    assert [r["n"] for r in ref] == [511, 513, 1025]
    assert np.isnan(ref[1]["fs"][-1]) and np.isinf(ref[2]["w"][512])          # the planted rows are where the text says
    got = farm_prep(ref, [0, 1, 2])
    for i, bad in enumerate([(0, 0), (1, 0), (0, 1)]):
        r, g = ref[i], got[i]
        assert same(g["params"], r["params"]) and same(g["w"], r["w"]) and same(g["fs"], r["fs"]), i
        assert same(np.array(g["scal"][:2]), np.array(r["scal"][:2])), i
        assert g["scal"][2:] == bad and tuple(r["scal"][2:]) == bad, (i, g["scal"], r["scal"])
    alone = farm_prep(ref, [0])[0]
    assert all(same(alone[k], got[0][k]) for k in ("params", "w", "fs")) and same(np.array(alone["scal"]), np.array(got[0]["scal"]))
    assert np.isinf(got[2]["scal"][1]) and np.isfinite(got[1]["scal"][0])     # SumW with the infinite weight; the max skips the NaN


# ---------------------------------------------------------------------------------------------------------------- 4. host route and pins
def test_against_the_host_route_and_the_per_root_resident_route(small_roots, monkeypatch):
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    roots = small_roots["roots"] + [small_roots["c1"]]
    ndims = [6, 5, None, 6, 4, 6, 6]
    pvols = [1.0, 2.5, 1.0, 0.5, 1.0, 3.0, 1.0]
    burns = [0, 0.3, 0, 100, 0, 0.2, 0]
    thins = [0, 0, 2, 0, 3, 0, 0]                          # thinned roots in the same call as unthinned ones
    want = [pkg.MCEvidence(r, kmax=4, verbose=0, ndim=ndims[i], priorvolume=pvols[i], burnlen=burns[i], thinlen=thins[i]).evidence(info=True)
            for i, r in enumerate(roots)]
    got = pkg.evidence_many_from_files(roots, kmax=4, ndim=ndims, priorvolume=pvols, burnlen=burns, thinlen=thins, info=True)
    assert routes(got) == ["farm"] * len(roots)
    per_root = [pkg.evidence_from_files(r, kmax=4, verbose=0, ndim=ndims[i], priorvolume=pvols[i], burnlen=burns[i], thinlen=thins[i], info=True)
                for i, r in enumerate(roots)]
    assert routes(per_root) == ["resident"] * len(roots)
    err_host = max(float(np.max(np.abs(g[0] - w[0]))) for g, w in zip(got, want))
    err_res = max(float(np.max(np.abs(g[0] - p[0]))) for g, p in zip(got, per_root))
    print("farm: max |lnE - lnE(host)| = %.3e, max |lnE - lnE(resident)| = %.3e (0 expected)" % (err_host, err_res))
    for g, w, p in zip(got, want, per_root):
        assert g[0].shape == w[0].shape
        for k in ("NparamsMC", "Nsamples_read", "Nparams_read", "NparamsCosmo", "Nsamples"):
            assert g[1][k] == w[1][k] == p[1][k], k
    assert err_host <= LNE_PARITY and err_res <= LNE_PARITY
    plain = pkg.evidence_many_from_files(roots[:2], kmax=4, ndim=ndims[:2], priorvolume=pvols[:2], burnlen=burns[:2])
    assert isinstance(plain[0], np.ndarray) and same(plain[0], got[0][0]) and same(plain[1], got[1][0])


@pytest.mark.parametrize("name", ["single", "pos_lnp", "recheck"])
def test_host_route_cases(small_roots, monkeypatch, name):
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    pos = name == "pos_lnp"
    roots = [small_roots["negated"]] if pos else small_roots["roots"][:3]
    covtype = "single" if name == "single" else "all"
    backend = pkg.HipBackend(recheck_rows=64) if name == "recheck" else None
    kw = {"backend": backend} if backend else {}
    want = [pkg.MCEvidence(r, kmax=3, verbose=0, ndim=6, **kw).evidence(covtype=covtype, pos_lnp=pos) for r in roots]
    got = pkg.evidence_many_from_files(roots, kmax=3, ndim=6, covtype=covtype, pos_lnp=pos, info=True, **kw)
    assert routes(got) == ["farm"] * len(roots)
    err = max(float(np.max(np.abs(g[0] - w))) for g, w in zip(got, want))
    print("%s: max |lnE(farm) - lnE(host)| = %.3e" % (name, err))
    assert err <= LNE_PARITY


def test_reference_pins(small_roots):
    root = small_roots["c1"]
    pi = pkg.params_info(root, cosmo=True)
    (lnE, info), = pkg.evidence_many_from_files([root], ndim=pi["ndim"], priorvolume=pi["volume"], kmax=2, info=True)
    assert info["route"] == "farm"
    assert info["Nsamples"] == "26862" and info["NparamsMC"] == 21 and info["NparamsCosmo"] == 6
    worst = float(np.max(np.abs(lnE - np.asarray(PINS["C1_all"]["lnE"]))))
    assert np.allclose(lnE, PINS["C1_all"]["lnE"], rtol=0, atol=1e-8)
    for ic in (1, 2, 3, 4):
        (lnE, info), = pkg.evidence_many_from_files([root], ndim=6, priorvolume=pi["volume"], kmax=2, idchain=ic, info=True)
        assert info["route"] == "farm" and info["Nsamples"] == str(PINS["C1_chain%d" % ic]["N"])
        worst = max(worst, float(np.max(np.abs(lnE - np.asarray(PINS["C1_chain%d" % ic]["lnE"])))))
        assert np.allclose(lnE, PINS["C1_chain%d" % ic]["lnE"], rtol=0, atol=1e-8)
    tags = ["burn0.3", "thin2", "burn0.2_thin3"]
    kws = [PINS["file_" + t]["kw"] for t in tags]
    got = pkg.evidence_many_from_files([root] * 3, ndim=6, priorvolume=1.0, kmax=3, burnlen=[k.get("burnlen", 0) for k in kws],
                                       thinlen=[k.get("thinlen", 0) for k in kws], info=True)
    assert routes(got) == ["farm"] * 3
    for t, (lnE, info) in zip(tags, got):
        p = PINS["file_" + t]
        assert info["Nsamples"] == str(p["N"])
        worst = max(worst, float(np.max(np.abs(lnE - np.asarray(p["lnE"])))))
        assert np.allclose(lnE, p["lnE"], rtol=0, atol=1e-8), t
    print("farm: max |dlnE| against the reference's pins = %.3e" % worst)


# ---------------------------------------------------------------------------------------------------------------- 5. declines and fallbacks
def test_declines_and_fallbacks(small_roots, monkeypatch, capsys, tmp_path):
    monkeypatch.setenv("MCE_CHAIN_READER", "native")
    roots = small_roots["roots"][:3]
    np.random.seed(3)
    want = pkg.MCEvidence(roots[1], kmax=3, verbose=0, ndim=6, thinlen=0.5).evidence()
    np.random.seed(3)
    got = pkg.evidence_many_from_files(roots, kmax=3, ndim=6, thinlen=[0, 0.5, 0], info=True)
    assert routes(got) == ["farm", "host", "farm"] and got[1][1]["declined"] == resident.REASONS["poisson"] and same(got[1][0], want)
    np.random.seed(5)
    split = pkg.evidence_many_from_files(roots[:2], kmax=3, ndim=6, split=True, info=True)
    assert routes(split) == ["resident", "resident"]
    with pytest.raises(ValueError, match="Poisson"):
        pkg.evidence_many_from_files(roots, kmax=3, ndim=6, thinlen=[0, 0.5, 0], require_resident=True)
    slots = pkg.evidence_many_from_files(roots, kmax=3, ndim=6, thinlen=[0, 0.5, 0], require_resident=True, return_exceptions=True, info=True)
    assert isinstance(slots[1], ValueError) and str(slots[1]) == resident.REASONS["poisson"]
    assert same(slots[0][0], got[0][0]) and same(slots[2][0], got[2][0])
    # a root larger than a wave takes the per-root resident route; the others stay on the farm
    sizes = [farm.farm_layout([os.path.getsize(p) for p in resident._resolve_files(r)])[1] for r in roots]
    small = pkg.evidence_many_from_files(roots, kmax=3, ndim=6, info=True, wave_bytes=max(sizes) - TILE)
    assert routes(small)[int(np.argmax(sizes))] == "resident" and sorted(set(routes(small))) == ["farm", "resident"]
    for s, g in zip(small, pkg.evidence_many_from_files(roots, kmax=3, ndim=6, info=True)):
        assert float(np.max(np.abs(s[0] - g[0]))) <= LNE_PARITY
    # the CLI: one root per line, '#' comments
    lst = tmp_path / "roots.txt"
    lst.write_text("# the grid\n%s\n\n%s   # second\n" % (roots[0], roots[1]))
    from mcevidence_amd import cli
    outs = cli.main([str(lst), "--farm", "-k", "3", "-vb", "0"])
    text = capsys.readouterr().out
    for r, o in zip(roots[:2], outs):
        host = cli.main([r, "-k", "3", "-vb", "0"])
        assert float(np.max(np.abs(o - host))) <= LNE_PARITY
        assert r in text and all(str(v) in text for v in o)


# ---------------------------------------------------------------------------------------------------------------- 6. the device-source batch call
def test_feed_batch_dev_equals_feed_batch_bitwise():
    import torch
    rng = np.random.default_rng(12)
    shapes = [(3, 200, 0, 3), (4, 3000, 0, 6), (5, 777, 400, 5), (6, 1500, 0, 9), (7, 513, 0, 7), (8, 2048, 1000, 8), (3, 300, 300, 4), (5, 1000, 0, 5),
              (6, 2500, 0, 6), (8, 900, 0, 11), (4, 1200, 650, 4), (7, 2000, 0, 10)]       # (d, n1, n2 -- 0: auto --, ld)
    host, dev, keep = [], [], []
    for k, (d, n1, n2, ld) in enumerate(shapes):
        S1 = rng.standard_normal((n1, ld)) * (1.0 + np.arange(ld))
        S2 = rng.standard_normal((n2, ld)) * (1.0 + np.arange(ld)) if n2 else None
        if k == 5:
            S1[:, 2] = 0.0                                   # a column of zeros: mean and covariance exactly 0, a singular matrix
            S2[:, 2] = 0.0
        w = 1.0 + rng.poisson(3.0, n1).astype(np.float64)
        fs = -rng.random(n1) * 5.0
        kmax = 3 + k % 3
        cov_mode = 1 if k == 9 else 0
        host.append((S1[:, :d] if ld == d else S1, None if S2 is None else S2, d, cov_mode, kmax, w, fs))
        t = [torch.from_numpy(a).to("cuda:0") if a is not None else None for a in (S1, S2, w, fs)]
        keep.append(t)
        dev.append((t[0].data_ptr(), n1, ld, t[1].data_ptr() if n2 else 0, n2, ld, d, cov_mode, kmax, t[2].data_ptr(), t[3].data_ptr()))
    torch.cuda.synchronize()
    a = _capi.evidence_feed_batch(host, return_exceptions=True)
    msg_host = _capi.last_error()
    b = _capi.evidence_feed_batch_dev(dev, return_exceptions=True)
    msg_dev = _capi.last_error()
    worst = 0.0
    for k, (x, y) in enumerate(zip(a, b)):
        if k == 5:
            assert isinstance(x, ValueError) and isinstance(y, ValueError) and str(x) == str(y) and "eigenvalue" in str(y), (x, y)
            continue
        assert not isinstance(x, Exception) and not isinstance(y, Exception), (k, x, y)
        worst = max(worst, float(np.max(np.abs(x[0] - y[0]))))
        assert same(x[0], y[0]) and x[1] == y[1] and same(x[2], y[2]), k
    assert msg_host == msg_dev
    print("feed_batch_dev against feed_batch over 12 problems: max |d dotp| = %.3e" % worst)
    with pytest.raises(ValueError, match="eigenvalue"):
        _capi.evidence_feed_batch_dev(dev)


# ---------------------------------------------------------------------------------------------------------------- 7. handle reuse
def test_one_handle_serves_every_call(small_roots):
    roots = small_roots["roots"]
    first = pkg.evidence_many_from_files(roots, kmax=3, ndim=6)
    h0 = farm._HANDLES[0][0].value
    st1 = farm.handle_stats()
    second = pkg.evidence_many_from_files(roots, kmax=3, ndim=6)
    st2 = farm.handle_stats()
    _capi.release_device_memory()
    third = pkg.evidence_many_from_files(roots, kmax=3, ndim=6)
    st3 = farm.handle_stats()
    assert farm._HANDLES[0][0].value == h0
    for a, b, c in zip(first, second, third):
        assert same(a, b) and same(a, c)
    nfiles = sum(len(resident._resolve_files(r)) for r in roots)
    assert st2["waves"] == st1["waves"] + 1 and st3["waves"] == st1["waves"] + 2 and st3["files"] == st1["files"] + 2 * nfiles
    # no allocation per file or per wave: nothing since the first wave of this size
    assert st2["allocs"] == st1["allocs"] == st3["allocs"] and st2["allocs_wave"] == 0 and st3["allocs_wave"] == 0 and st3["grows"] == st1["grows"]


# ------------------------------------------------------------------------------------------- 9. every statistic at once, mixed per root
def mixed_roots(td):
    """four roots of two files each, three parameters, 400 rows per file (integer weights); the second root has a .ranges file.  Returns
    (roots, the farm's keywords: one entry per root for every statistic of posterior.py, the jackknife and the thinning)"""
    from mcevidence_amd.synth import gaussian_chain
    roots = []
    for r in range(4):
        chains = [gaussian_chain(seed=900 + 2 * r + c, n=400, d=3, weights="int", cov="corr") for c in range(2)]
        lo = min(float(ch[:, 2].min()) for ch in chains) - 0.5
        roots.append(os.path.join(str(td), "mixed%d" % r))
        write_cosmomc_chains(roots[-1], chains, [("p0", lo, None), ("p1", -50.0, 50.0), ("p2", -50.0, None)] if r == 1 else None, fmt="%.17g")
    m1 = {"probs": (0.9,), "grid": 64}
    kw = dict(information=[True, True, None, True], summary=[(0.9,), True, None, None], marginals=[m1, {"grid": 128}, None, m1],
              bounds=[None, "ranges", None, None], contours=[{"grid": 32}, None, None, {"grid": 32, "probs": (0.5,), "bounds": {"p1": (-40.0, None)}}],
              covariance=[True, None, None, True], jackknife=[4, None, None, 4], thinlen=[0, 0, 0, 2])
    return roots, kw


def same_info(a, b):
    """two info entries, bit for bit in every float (the route's name and the ladder's timings left out)"""
    if isinstance(a, dict):
        keys = set(a) - {"route", "kernel_ms"}
        return isinstance(b, dict) and keys == set(b) - {"route", "kernel_ms"} and all(same_info(a[k], b[k]) for k in keys)
    if isinstance(a, (str, bool, int, type(None))) or (isinstance(a, (list, tuple)) and any(isinstance(x, (str, tuple, list)) for x in a)):
        return type(a) is type(b) and a == b
    return same(a, b)


def test_every_statistic_at_once_mixed_per_root_equals_the_per_root_resident_route(tmp_path):
    roots, kw = mixed_roots(tmp_path)
    got = farm.evidence_many_from_files(roots, kmax=3, info=True, **kw)
    assert farm.LAST_STATS["counts"]["farm"] == len(roots) and farm.LAST_STATS["counts"]["fallback"] == 0
    for i, (root, (lnE, info)) in enumerate(zip(roots, got)):
        assert info["route"] == "farm"
        one = {k: v[i] for k, v in kw.items() if v[i] is not None}
        want_lnE, want = pkg.evidence_from_files(root, kmax=3, info=True, verbose=0, require_resident=True, **one)
        assert want["route"] == "resident" and same(lnE, want_lnE)
        assert set(info) & set(kw) == set(one) - {"bounds", "thinlen"} == set(want) & set(kw), (i, sorted(info))
        assert same_info(info, want), (i, [k for k in info if k in want and not same_info(info[k], want[k])])
        for key in ("marginals", "contours"):
            if key in info:                              # (every column and pair measured: the comparison is of numbers, not of NaN)
                assert info[key]["status"] == 0 and not np.any(info[key]["col_status"]) and not np.any(info[key].get("pair_status", 0))
    assert got[1][1]["marginals"]["at_lo"][0] == 1.0 and got[1][1]["marginals"]["grid"] == 128 and "bound_lo" not in got[0][1]["marginals"]
    assert got[3][1]["contours"]["bound_lo"][1] == -40.0 and "bound_lo" not in got[0][1]["contours"] and got[3][1]["Nsamples_read"] != 800
    assert set(got[2][1]) & set(kw) == set() and "sigma" in got[0][1]["information"] and "sigma" not in got[1][1]["information"]
