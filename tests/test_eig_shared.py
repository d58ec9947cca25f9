"""The rules the host check and the batched device eigen-solver share (mcevidence_amd/csrc/eig_jacobi.hpp), on the CPU: the
round-robin pair schedule is exact; the header's serial driver -- the device's schedule, phases and finalisation on one thread --
meets the bound family of tests/test_gpu_feeders.py against the high-precision oracle (orc.eig_hp), converges well below the
sweep cap, leaves the canonical form and reports the status rule; and the option travels through the Python layers without a
GPU.  The stand-alone program is built with AddressSanitizer and UBSan.  CPU only.

Bounds (test_gpu_feeders.py): with C = diag(s) Cn diag(s), every eigenvalue within C_FEED eps cond(Cn) relative of eig_hp of
the SAME fp64 matrix, ln J within d/2 of that."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import REPO, graded_chain, graded_cov, orc, singular_chain

from mcevidence_amd import _capi
from mcevidence_amd.evidence import HipBackend

C_FEED = 16.0
EPS = float(np.finfo(np.float64).eps)
SWEEP_CAP = 100
DIMS = (1, 2, 3, 5, 27, 63, 64, 65, 127)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eig_jacobi") / "eig_jacobi_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "eig_jacobi_check.cpp"), "-o", exe])
    return exe


def solve(exe, tmp_path, mats, solver=0):
    """[d x d fp64] -> [(status[4], lam, scale, evec)] from the header's serial driver (solver 1: the host solver)"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for a in mats:
            a = np.ascontiguousarray(a, dtype="<f8")
            f.write(struct.pack("<qq", a.shape[0], solver))
            f.write(a.tobytes())
    out = subprocess.run([exe, "solve", str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % len(mats)), out.stdout[-2000:] + out.stderr[-2000:]
    raw = open(fout, "rb").read()
    got, at = [], 0
    for a in mats:
        d = np.asarray(a).shape[0]
        st = np.frombuffer(raw, dtype="<i8", count=4, offset=at)
        at += 32
        lam = np.frombuffer(raw, dtype="<f8", count=d, offset=at)
        at += 8 * d
        scale = np.frombuffer(raw, dtype="<f8", count=d, offset=at)
        at += 8 * d
        evec = np.frombuffer(raw, dtype="<f8", count=d * d, offset=at).reshape(d, d)
        at += 8 * d * d
        got.append((st, lam, scale, evec))
    assert at == len(raw)
    return got


def cond_cn(M):
    dg = np.sqrt(np.diag(M))
    ev = np.linalg.eigvalsh(M / np.outer(dg, dg))
    return float(ev[-1] / ev[0])


def matrices():
    """name -> fp64 symmetric matrix: the two graded covariances, and the rounded longdouble covariance of a graded chain per d"""
    out = {"graded_cov4_d40": graded_cov(4), "graded_cov5_d64": graded_cov(5)}
    for d in DIMS:
        n = 255 if d == 127 else 2 * d + 33
        out["graded_chain_d%d_n%d" % (d, n)] = orc.covariance_hp(graded_chain(100 + d, n, d)[:, 2:]).astype(np.float64)
    return out


@pytest.fixture(scope="module")
def solved(checker, tmp_path_factory):
    mats = matrices()
    got = solve(checker, tmp_path_factory.mktemp("solved"), list(mats.values()))
    return {name: (M, g) for (name, M), g in zip(mats.items(), got)}


def assert_canonical(lam, evec):
    d = lam.size
    assert np.all(np.diff(lam) <= 0), "eigenvalues not descending"
    big = np.argmax(np.abs(evec), axis=0)            # (argmax: the FIRST largest)
    assert np.all(evec[big, np.arange(d)] > 0), "an eigenvector's first largest-magnitude component is not positive"


def test_schedule_is_a_round_robin_tournament(checker):
    """d = 1 .. 128: each unordered pair of real indices exactly once per sweep, the pairs of a step disjoint -- exact"""
    out = subprocess.run([checker, "schedule"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "ok schedule", (out.returncode, out.stdout[-500:], out.stderr[-2000:])


@pytest.mark.parametrize("name", list(matrices()))
def test_serial_driver_against_the_oracle(solved, name):
    """eigenvalues within C_FEED eps cond(Cn) of eig_hp, ln J within d/2 of it; sweeps below the cap; canonical form; the
    eigenvectors orthonormal and the scales 1 / sqrt(lam)"""
    M, (st, lam, scale, evec) = solved[name]
    d = M.shape[0]
    assert tuple(st[:2]) == (0, 0), st
    assert 1 <= st[2] < SWEEP_CAP, "sweeps: %d" % st[2]
    assert st[3] <= st[2] * d * (d - 1) // 2
    truth, _ = orc.eig_hp(M)
    bound = C_FEED * EPS * cond_cn(M)
    rel = np.abs(lam - truth.astype(np.float64)) / truth.astype(np.float64)
    print("%s: sweeps %d rotations %d max rel err %.3e bound %.3e" % (name, st[2], st[3], rel.max(), bound))
    assert rel.max() <= bound, (name, int(rel.argmax()), rel.max(), bound)
    lnj = 0.5 * float(np.sum(np.log(truth)))
    assert abs(0.5 * float(np.sum(np.log(lam))) - lnj) <= 0.5 * d * bound
    assert_canonical(lam, evec)
    assert np.array_equal(scale, 1.0 / np.sqrt(lam))
    assert np.max(np.abs(evec.T @ evec - np.eye(d))) <= 64 * d * EPS


def test_multiple_of_identity_returns_identity_after_one_sweep(checker, tmp_path):
    mats = [c * np.eye(d) for c in (1.0, 3.5e-7) for d in (1, 2, 5, 64)]
    for M, (st, lam, scale, evec) in zip(mats, solve(checker, tmp_path, mats)):
        assert tuple(st) == (0, 0, 1, 0), st
        assert np.array_equal(evec, np.eye(M.shape[0])) and np.array_equal(lam, np.diag(M))


def test_status_rule(checker, tmp_path):
    """a NaN (or an infinity) gives status 1 with zero sweeps; a singular covariance status 2 or a tiny smallest eigenvalue; a
    negative-definite 2 x 2 status 2 at index 0, an indefinite one at index 1 -- and a system that fails still gets the identity
    and unit scales"""
    nan = graded_cov(0).copy()
    nan[2, 4] = nan[4, 2] = np.nan
    inf = graded_cov(0).copy()
    inf[0, 0] = np.inf
    sing = orc.covariance_hp(singular_chain(8, 3000)[:, 2:]).astype(np.float64)
    negdef = np.array([[-2.0, 0.5], [0.5, -1.0]])
    indef = np.array([[1.0, 2.0], [2.0, 1.0]])
    got = solve(checker, tmp_path, [nan, inf, sing, negdef, indef])
    for st, lam, scale, evec in got[:2]:
        assert tuple(st) == (1, 0, 0, 0), st
        assert np.array_equal(evec, np.eye(6)) and np.array_equal(scale, np.ones(6))
    st, lam, scale, evec = got[2]
    assert st[0] in (0, 2) and st[2] < SWEEP_CAP
    assert st[0] == 2 or lam.min() < 1e-9 * lam.max(), (st, lam)
    st, lam, scale, evec = got[3]
    assert tuple(st[:2]) == (2, 0) and np.all(lam < 0) and lam[0] >= lam[1], (st, lam)
    assert np.array_equal(evec, np.eye(2)) and np.array_equal(scale, np.ones(2))
    st, lam, scale, evec = got[4]
    assert tuple(st[:2]) == (2, 1) and np.allclose(lam, [3.0, -1.0], rtol=1e-15, atol=0), (st, lam)
    assert np.array_equal(evec, np.eye(2)) and np.array_equal(scale, np.ones(2))


def test_host_solver_moved_unchanged(checker, tmp_path):
    """jacobi_eig lives in the shared header now: through the library's door (eig_sym_batch, EIG_HOST; no GPU needed) it gives
    what the stand-alone build of the header gives, in canonical form, with the shared status rule"""
    mats = [graded_cov(0), graded_cov(1), np.array([[1.0, 2.0], [2.0, 1.0]])]
    got = solve(checker, tmp_path, mats, solver=1)
    for M, (st, lam, scale, evec) in zip(mats, got):
        e2, s2, l2, st2 = _capi.eig_sym_batch(M, mode=_capi.EIG_HOST)
        assert tuple(st2[0][:2]) == tuple(st[:2])
        assert np.allclose(l2[0], lam, rtol=1e-13, atol=0)
        if st[0] == 0:
            assert_canonical(l2[0], e2[0])
            assert np.allclose(e2[0], evec, rtol=0, atol=1e-12) and np.allclose(s2[0], scale, rtol=1e-13, atol=0)
        else:
            assert np.array_equal(e2[0], np.eye(M.shape[0])) and np.array_equal(s2[0], np.ones(M.shape[0]))


# ---------------------------------------------------------------------------------------------------- plumbing, without a GPU
def test_options_carry_eig_mode():
    assert (_capi.EIG_DEFAULT, _capi.EIG_HOST, _capi.EIG_DEVICE) == (0, 1, 2)
    o = _capi.Options()
    assert o.eig_mode == 0 and o.size == ctypes.sizeof(_capi.Options) == 32            # the struct did not grow: reserved[0] became eig_mode
    o = _capi.Options(eig_mode=_capi.EIG_DEVICE, verify=7)
    assert (o.eig_mode, o.verify, o.search_mode) == (2, 7, -1)
    for m in (_capi.EIG_DEFAULT, _capi.EIG_HOST, _capi.EIG_DEVICE):
        with _capi.options(eig_mode=m):
            with _capi.options(eig_mode=_capi.EIG_HOST):
                pass
    with pytest.raises(ValueError, match="eig_mode"):
        with _capi.options(eig_mode=3):
            pass
    with pytest.raises(ValueError, match="eig_mode"):
        with _capi.options(eig_mode=-1):
            pass


def test_backend_and_environment_set_it(monkeypatch):
    monkeypatch.delenv("MCE_FEED_EIG", raising=False)
    b = HipBackend()
    assert b.device_eig is None and not b.uses_device_eig()
    assert not hasattr(b._scoped(), "opt")                              # nothing pushed: the library's default, as before
    on, off = HipBackend(device_eig=True), HipBackend(device_eig=False)
    assert on.uses_device_eig() and on._scoped().opt.eig_mode == _capi.EIG_DEVICE
    assert not off.uses_device_eig() and off._scoped().opt.eig_mode == _capi.EIG_HOST
    both = HipBackend(device_eig=True, recheck_rows=64)._scoped().opt
    assert (both.eig_mode, both.verify) == (_capi.EIG_DEVICE, 64)
    monkeypatch.setenv("MCE_FEED_EIG", "hip")
    assert HipBackend().uses_device_eig() and not HipBackend(device_eig=False).uses_device_eig()
    monkeypatch.setenv("MCE_FEED_EIG", "host")
    assert not HipBackend().uses_device_eig()
    from mcevidence_amd.cli import build_parser
    assert build_parser().parse_args(["root", "--device-eig"]).device_eig is True
    assert build_parser().parse_args(["root"]).device_eig is False


def test_new_symbols_are_exported_and_validate():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("mce_eig_sym_batch_dev_f64", "mce_eig_sym_batch_f64", "mce_last_eig_stats"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES, name
    assert _capi.load().mce_abi_version() == 3
    assert sorted(_capi.last_eig_stats()) == ["device", "host", "max_sweeps", "rotations"]
    with pytest.raises(ValueError):
        _capi.eig_sym_batch(np.eye(128), mode=_capi.EIG_HOST)           # d > 127
    with pytest.raises(ValueError):
        _capi.eig_sym_batch(np.eye(3), mode=0)
    with pytest.raises(ValueError):
        _capi.eig_sym_batch(np.zeros((2, 3, 4)))
    if _capi.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            _capi.eig_sym_batch(np.eye(3), mode=_capi.EIG_DEVICE)
