"""The jackknife of the resident route and the farm on the CPU (docs/design/jackknife_resident.md): the rule the host check and the
device kernels share (mcevidence_amd/csrc/jack_groups.hpp: its serial drivers, built with -fsanitize=address,undefined as a stand-alone
program) -- group ids against ``jackknife.group_ids``, leave-one-group-out blocks against the exact rational model of
tests/moments_cases.py applied to every deleted set, within the bound of docs/design/information.md at that set's own n -- and the
plumbing that needs no device: the decline table of ``plan(jackknife=...)``, the three ValueErrors, the command line, the new C symbols."""
import os
import struct
import subprocess

import numpy as np
import pytest

import moments_cases as mc
from helpers import REPO
from mcevidence_amd import _capi, jackknife as jk, resident


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jack_groups") / "jack_groups_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "jack_groups_check.cpp"), "-o", exe])
    return exe


def _run(exe, mode, tmp_path, payload, nrec):
    fin, fout = tmp_path / (mode + "_in.bin"), tmp_path / (mode + "_out.bin")
    with open(fin, "wb") as fh:
        fh.write(payload)
    out = subprocess.run([exe, mode, str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % nrec), out.stdout[-2000:] + out.stderr[-2000:]
    return open(fout, "rb").read()


def native_groups(exe, tmp_path, systems):
    """[(rows or None, src or None, part_first or None, n, N, G, by)] through the sanitized program -> one int32 array per system"""
    payload = b""
    for rows, src, first, n, N, G, by in systems:
        first = [] if first is None else list(first)
        payload += struct.pack("<7q", n, N, G, _capi.JACK_BY[by], rows is not None, src is not None, len(first))
        for a in (rows, src, first):
            if a is not None:
                payload += np.ascontiguousarray(a, dtype="<i8").tobytes()
    raw = np.frombuffer(_run(exe, "groups", tmp_path, payload, len(systems)), dtype="<i4")
    at = np.concatenate([[0], np.cumsum([s[3] for s in systems])])
    return [raw[at[i]:at[i + 1]] for i in range(len(systems))]


def native_leave_out(exe, tmp_path, systems):
    """[(w, fs or None, g, G)] through the sanitized program -> [(ok, block [G + 1, 8])]"""
    payload = b""
    for w, fs, g, G in systems:
        payload += struct.pack("<3q", len(w), G, fs is not None) + np.ascontiguousarray(w, dtype="<f8").tobytes()
        if fs is not None:
            payload += np.ascontiguousarray(fs, dtype="<f8").tobytes()
        payload += np.ascontiguousarray(g, dtype="<i4").tobytes()
    raw = _run(exe, "leave_out", tmp_path, payload, len(systems))
    out, at = [], 0
    for _, _, _, G in systems:
        ok = struct.unpack_from("<q", raw, at)[0]
        out.append((ok, np.frombuffer(raw, dtype="<f8", count=(G + 1) * 8, offset=at + 8).reshape(G + 1, 8)))
        at += 8 + (G + 1) * 64
    assert at == len(raw)
    return out


class FakeSamples(object):
    """what ``jackknife.group_ids`` reads of an MCSamples: the sample, the partition's rows, the chain of every row"""

    def __init__(self, N, rows, row_chain):
        part = type("Part", (), {})()
        part.ichain = np.asarray(rows, dtype=np.int64)
        self.data = {"s1": part}
        self.samples = np.zeros((N, 1))
        self.row_chain = row_chain


def test_group_ids_equal_the_host_rule(checker, tmp_path):
    rng = np.random.default_rng(5)
    systems, want = [], []
    for n in (1, 255, 256, 257, 513):
        for G in (2, 16, 64):
            perm = rng.permutation(n)
            for rows in (None, perm):
                systems.append((rows, None, None, n, n, G, "blocks"))
                want.append(jk.group_ids(FakeSamples(n, np.arange(n) if rows is None else rows, None), "s1", G, "blocks"))
    # a row list that takes part of a longer sample (a split): N is the sample's length
    pick = np.sort(rng.permutation(1000)[:300])
    systems.append((pick, None, None, 300, 1000, 16, "blocks"))
    want.append(jk.group_ids(FakeSamples(1000, pick, None), "s1", 16, "blocks"))
    # chains: four parts of unequal length, one of them empty; unthinned, through a thinned src, and both under a row list
    lens = [300, 0, 57, 401]
    first = np.concatenate([[0], np.cumsum(lens)])[:4]
    chain = np.repeat(np.arange(4), lens)
    nb = sum(lens)
    systems.append((None, None, first, nb, nb, 4, "chains"))
    want.append(jk.group_ids(FakeSamples(nb, np.arange(nb), chain), "s1", 4, "chains"))
    src = np.sort(rng.permutation(nb)[:333])
    systems.append((None, src, first, 333, 333, 4, "chains"))
    want.append(jk.group_ids(FakeSamples(333, np.arange(333), chain[src]), "s1", 4, "chains"))
    rows = rng.permutation(333)[:100]
    systems.append((rows, src, first, 100, 333, 4, "chains"))
    want.append(jk.group_ids(FakeSamples(333, rows, chain[src]), "s1", 4, "chains"))
    # empty parts at both ends
    first2 = [0, 0, 10, 10, 25, 25]
    chain2 = np.repeat(np.arange(6), [0, 10, 0, 15, 0, 0])
    systems.append((None, None, first2, 25, 25, 6, "chains"))
    want.append(jk.group_ids(FakeSamples(25, np.arange(25), chain2), "s1", 6, "chains"))
    got = native_groups(checker, tmp_path, systems)
    for s, g, w in zip(systems, got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), s[3:]
    # a row outside the sample has no group
    bad, = native_groups(checker, tmp_path, [(np.array([0, 7, -1, 3]), None, None, 4, 7, 2, "blocks")])
    assert list(bad) == [0, -1, -1, 0]


def check_slot(name, b, block, a, f, keep, with_moments=True):
    """one slot against the exact model of the deleted set, within the bound at that set's n"""
    a, f = a[keep], f[keep]
    assert block[0] == keep.sum(), (name, b)
    ex = mc.exact(a, f)
    bound = mc.bounds(ex)
    assert abs(block[1] - ex["W"]) <= bound["W"], (name, b, "SumW")
    if not with_moments:
        assert np.isnan(block[2:7]).all() and block[7] == -1
        return 0.0
    got = dict(W=block[2], c=block[3], v=block[4], A2=block[5], rows=int(block[6]), status=int(block[7]))
    assert got["status"] == 0 and got["rows"] == ex["rows"], (name, b, got)
    r = mc.ratios(type("C", (), {"exact": ex, "bound": bound})(), got)
    assert all(x <= 1.0 for x in r.values()), (name, b, r)
    return max(r.values())


def leave_out_cases():
    """(name, a, f, g, G): the cases of moments_cases cut into groups -- blocks, a permuted assignment, a group without rows"""
    rng = np.random.default_rng(77)
    out = []
    for name, G in (("B_511", 2), ("B_512", 16), ("B_513", 64), ("B_1025", 8), ("C_narrow", 8), ("D_zeros", 5), ("E_negative", 4)):
        c = mc.BY_NAME[name]
        n = len(c.a)
        out.append((name + "_blocks", c.a, c.f, (np.arange(n) * G // n).astype(np.int32), G))
    c = mc.BY_NAME["B_1025"]
    out.append(("B_1025_permuted", c.a, c.f, rng.integers(0, 16, size=1025).astype(np.int32), 16))
    g = rng.integers(0, 7, size=1025).astype(np.int32)
    g[g == 3] = 4
    out.append(("B_1025_empty_group", c.a, c.f, g, 7))
    return out


def test_leave_out_blocks_against_the_exact_model_of_every_deleted_set(checker, tmp_path):
    cases = leave_out_cases()
    got = native_leave_out(checker, tmp_path, [(a, f, g, G) for _, a, f, g, G in cases])
    worst = 0.0
    for (name, a, f, g, G), (ok, block) in zip(cases, got):
        assert ok == 1
        for b in range(-1, G):
            worst = max(worst, check_slot(name, b, block[b + 1], a, f, g != b))
    print("serial driver: largest error / bound over every slot: %.3g" % worst)
    # a group without rows: its slot is the full slot, bit for bit
    name, a, f, g, G = cases[-1]
    assert got[-1][1][1 + 3].tobytes() == got[-1][1][0].tobytes()
    # without an fs column: rows and SumW only
    (ok, block), = native_leave_out(checker, tmp_path, [(a, None, g, G)])
    assert ok == 1
    for b in range(-1, G):
        check_slot(name, b, block[b + 1], a, f, g != b, with_moments=False)


def test_leave_out_statuses_fail_alone(checker, tmp_path):
    c = mc.BY_NAME["A_unit"]
    n, G = len(c.a), 4
    g = (np.arange(n) * G // n).astype(np.int32)
    # group 1 holds every used row: with it deleted nothing is left (status 5); every other slot is that of the good data
    a = np.where(g == 1, c.a, 0.0)
    f = np.where(g == 1, c.f, np.where(np.arange(n) % 2 == 0, -np.inf, np.nan))          # zero weights over -inf and NaN: never read
    (ok, block), = native_leave_out(checker, tmp_path, [(a, f, g, G)])
    assert ok == 1
    assert block[2, 7] == 5 and np.isnan(block[2, 2:6]).all() and block[2, 6] == 0 and block[2, 0] == (g != 1).sum() and block[2, 1] == 0.0
    for b in (-1, 0, 2, 3):
        check_slot("all_in_one_group", b, block[b + 1], a, f, g != b)
    # a -inf likelihood on a used row of group 2: every slot that keeps the row has status 3, the slot that deletes it is good
    f3 = c.f.copy()
    row = int(np.flatnonzero(g == 2)[5])
    f3[row] = -np.inf
    (ok, block), = native_leave_out(checker, tmp_path, [(c.a, f3, g, G)])
    assert [int(s) for s in block[:, 7]] == [3, 3, 3, 0, 3]
    assert np.isnan(block[[0, 1, 2, 4], 2:6]).all()
    check_slot("minus_inf", 2, block[3], c.a, f3, g != 2)
    # a group id outside [0, G): refused
    gbad = g.copy()
    gbad[17] = G
    assert native_leave_out(checker, tmp_path, [(c.a, c.f, gbad, G)])[0][0] == 0


def test_plan_decline_table_and_value_errors():
    R = resident.REASONS
    assert R["jackknife_cross"] == "jackknife of a cross evidence whitens on the host"
    for jack in (True, 8, {"groups": 8}, {"by": "chains"}, {"groups": 4, "by": "blocks"}):
        assert resident.plan(jackknife=jack) == resident.RESIDENT
        assert resident.plan(jackknife=jack, split=True) == R["jackknife_cross"]
        assert resident.plan(jackknife=jack, nchains=4, covtype="all", ndim=6, nparam=9, nrows=100) == resident.RESIDENT
    for off in (None, False):
        assert resident.plan(jackknife=off, split=True) == resident.RESIDENT
        assert resident.jack_spec(off) is None
    # what declines anyway keeps its reason and its precedence
    assert resident.plan(jackknife=8, thinlen=0.5) == R["poisson"]
    assert resident.plan(jackknife=8, split=True, covtype="single") == R["split_single"]
    assert resident.plan(jackknife=8, brange=[1, 2]) == R["batches"]
    assert resident.plan(jackknife=8, ndim=200) == R["ndim"]
    # the ValueErrors of the host route, in its words
    for G in (1, 65, 0):
        with pytest.raises(ValueError, match=r"jackknife: G=%d groups \(2 \.\. 64 expected\)" % G):
            resident.plan(jackknife=G)
    with pytest.raises(ValueError, match=r"jackknife by='chains' needs at least 2 chains \(got 1\)"):
        resident.plan(jackknife={"by": "chains"}, nchains=1)
    with pytest.raises(ValueError, match=r"jackknife: by='files' \('blocks' or 'chains' expected\)"):
        resident.plan(jackknife={"by": "files"})
    with pytest.raises(ValueError, match="jackknife: unknown key"):
        resident.plan(jackknife={"group": 4})
    assert resident.jack_spec({"by": "chains"}, 5) == {"groups": 16, "by": "chains", "G": 5}
    assert resident.jack_spec(True)["G"] == 16 and resident.jack_spec({"by": "chains"})["G"] is None


def test_host_route_raises_the_same_words():
    from helpers import OracleBackend
    from mcevidence_amd.evidence import MCEvidence
    from mcevidence_amd.synth import gaussian_chain
    m = MCEvidence([gaussian_chain(seed=1, n=300, d=3)], kmax=3, verbose=0, backend=OracleBackend())
    for kw, words in (({"groups": 1}, r"jackknife: G=1 groups \(2 \.\. 64 expected\)"), ({"by": "chains"}, r"needs at least 2 chains \(got 1\)"),
                      ({"by": "files"}, r"jackknife: by='files' \('blocks' or 'chains' expected\)")):
        with pytest.raises(ValueError, match=words):
            m.evidence_jackknife(**kw)


def test_cli_takes_jackknife_with_resident_and_farm(tmp_path, capsys):
    from mcevidence_amd import cli
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    root = str(tmp_path / "planck")
    chains, _, ranges = planck_like_chains(seed=3, rows=(260, 250, 240, 255), nnuis=3)
    write_cosmomc_chains(root, chains, ranges=ranges, fmt="%.17g")
    listing = tmp_path / "roots.txt"
    listing.write_text(root + "\n")
    for argv in ([root, "--resident"], [str(listing), "--farm"]):
        argv = argv + ["-k", "3", "-np", "6", "-vb", "0", "--jackknife=4", "--jackknife-by", "chains"]
        if _capi.device_count() < 1:
            with pytest.raises(RuntimeError, match="no HIP device"):          # (accepted: only the device is missing)
                cli.main(argv)
            continue
        capsys.readouterr()
        cli.main(argv)
        out = capsys.readouterr().out
        assert out.count("±") == 3 and "   ln(B)[k=1] = " in out and "   ln(B)[k=2] = " in out
        assert "* ±: delete-a-group jackknife over 4 chains (conservative, not a calibrated 1 sigma)." in out


def test_new_symbols_validate_without_a_device():
    lib = _capi.load()
    for name in ("mce_jack_groups_dev", "mce_jack_leave_out_workspace_bytes", "mce_jack_leave_out_dev", "mce_jack_leave_out_f64"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert lib.mce_abi_version() == 3
    small, big = _capi.jack_leave_out_workspace_bytes(1000, 1, 2), _capi.jack_leave_out_workspace_bytes(100000, 5, 64)
    assert 0 < small < big
    assert _capi.jack_leave_out_workspace_bytes(1000, 1, 1) == 0 and _capi.jack_leave_out_workspace_bytes(1000, 1, 65) == 0
    w = np.ones(10)
    with pytest.raises(ValueError, match=r"jackknife: G=1 groups \(2 \.\. 64 expected\)"):
        _capi.jack_leave_out([(w, None, np.zeros(10, dtype=np.int32), 1)])
    with pytest.raises(ValueError, match="by=7"):
        arr = (_capi.JackGroupsSeg * 1)()
        arr[0].n, arr[0].N, arr[0].G, arr[0].by = 0, 0, 4, 7
        _capi.check(lib.mce_jack_groups_dev(arr, 1, None))
    with pytest.raises(ValueError, match="parts for G=4 chains"):
        _capi.jack_groups_dev([(0, 0, [0, 5], 0, 0, 4, "chains", 0)])
