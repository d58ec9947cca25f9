"""The batched Jacobi eigen-solver on the device (mcevidence_amd/csrc/eig_kernels.hpp) and the evidence feed with it switched on
(mce_options.eig_mode = EIG_DEVICE; docs/design/device_eig.md): the solver itself, a batch with bad systems planted in it, every
feed route, the failure path, the class and the farm, and the guard that the option OFF is what it was.  Needs a real MI355X:
run with -m gpu.

Bounds: those of tests/test_gpu_feeders.py, whose chains and high-precision truths (computed once per session, in that module's
cache) this file shares.  With C = diag(s) Cn diag(s):
  eigenvalue        |lam - lam_hp| / lam_hp                 <= C_FEED eps cond(Cn)          (two solvers against each other: twice)
  Jacobian          |ln J - ln J_hp|                         <= d/2 * C_FEED eps cond(Cn)
  whitened column   max_i |X_ic - X_hp,ic|                   <= C_FEED eps cond(Cn) (spread_c + max_i |X_hp,ic|) / min(1, gap_c)
  pair distance     | |x_i - x_j| - |x_i - x_j|_hp |         <= C_FEED eps (cond(Cn) |x_i - x_j|_hp + |x_i|_hp + |x_j|_hp)
  device vs host    |ln dotp_device - ln dotp_host|          <= 2 max(LNE_TOL, d C_FEED eps cond(Cn))
"""
import logging
import math
import os

import numpy as np
import pytest

import test_gpu_feeders as tf
from helpers import LNE_TOL, graded_chain, orc, singular_chain

pytestmark = pytest.mark.gpu
logging.disable(logging.CRITICAL)

C_FEED = 16.0
EPS = float(np.finfo(np.float64).eps)
KMAX = 4
SWEEP_CAP = 100

CASES = {"graded27_n20000": "graded27_n20000_condC1.9e16_condCn2.3e4", "issue64_n20000": "issue64_n20000_condC2.4e15_condCn2.1e5",
         "offset12_n20000": "offset12_n20000_condC1.2e8_condCn5.6"}
SHAPES = [(1, 33), (2, 33), (63, 65), (64, 66), (127, 255)]
KEYS = list(CASES.values()) + SHAPES
IDS = list(CASES) + ["d%d_n%d" % s for s in SHAPES]


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def cond_cn(M):
    M = np.asarray(M, dtype=np.longdouble)
    dg = np.sqrt(np.diag(M))
    ev = np.linalg.eigvalsh((M / np.outer(dg, dg)).astype(np.float64))
    return float(ev[-1] / ev[0])


def assert_canonical(lam, evec):
    d = lam.size
    assert np.all(np.diff(lam) <= 0), "eigenvalues not descending"
    big = np.argmax(np.abs(evec), axis=0)
    assert np.all(evec[big, np.arange(d)] > 0), "an eigenvector's first largest-magnitude component is not positive"


def check_eigs(ev, J, f, what=""):
    lam = f["lam"].astype(np.float64)
    bound = C_FEED * EPS * f["condCn"]
    rel = np.abs(ev - lam) / lam
    assert np.all(np.isfinite(ev)) and rel.max() <= bound, (
        "%s eigenvalue %d: relative error %.3e > bound %.3e (cond(Cn) = %.3g)" % (what, int(rel.argmax()), rel.max(), bound, f["condCn"]))
    lnj = 0.5 * float(np.sum(np.log(f["lam"])))
    assert abs(math.log(J) - lnj) <= 0.5 * len(lam) * bound, (what, math.log(J) - lnj)
    return rel.max() / bound


def check_rows(X, S, f, nsample=4000, seed=0):
    """whitened rows X [n, d] from the device against whiten_hp of S with the true eigen-system: per column where the eigenvalue
    is separated, and the distances of sampled row pairs everywhere (a rotation inside a near-degenerate eigen-space keeps them)"""
    Xt = orc.whiten_hp(S, f["U"], f["lam"])
    Xf = Xt.astype(np.float64)
    lam = f["lam"].astype(np.float64)
    d = lam.size
    cond = f["condCn"]
    gap = np.full(d, np.inf)
    for c in range(d):
        o = np.delete(lam, c)
        if o.size:
            gap[c] = np.min(np.abs(o - lam[c]) / np.sqrt(o * lam[c]))
    n = S.shape[0]
    if n > 2:
        err = np.max(np.abs(X - Xf), axis=0)
        bound = C_FEED * EPS * cond * (Xf.std(axis=0) + np.max(np.abs(Xf), axis=0)) / np.minimum(1.0, np.maximum(gap, 1e-300))
        bad = np.nonzero((gap > 1e-6) & ~(err <= bound))[0]
        assert bad.size == 0, ("whitened column", bad[:5], err[bad[:5]], bound[bad[:5]])
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, n, nsample), rng.integers(0, n, nsample)
    dt = np.sqrt(np.sum((Xt[i] - Xt[j]) ** 2, axis=1)).astype(np.float64)
    dd = np.sqrt(np.sum((X[i] - X[j]) ** 2, axis=1))
    nrm = np.sqrt(np.sum(Xf ** 2, axis=1))
    bound = C_FEED * EPS * (cond * dt + nrm[i] + nrm[j])
    bad = np.nonzero(~(np.abs(dd - dt) <= bound))[0]
    assert bad.size == 0, ("pair distance", bad[:5], dd[bad[:5]], dt[bad[:5]], bound[bad[:5]])


def device_eig():
    from mcevidence_amd import _capi
    return _capi.options(eig_mode=_capi.EIG_DEVICE)


def host_eig():
    from mcevidence_amd import _capi
    return _capi.options(eig_mode=_capi.EIG_HOST)


def assert_stats(device, host=0):
    from mcevidence_amd import _capi
    st = _capi.last_eig_stats()
    assert st["device"] == device and st["host"] == host, st
    if device:
        assert 1 <= st["max_sweeps"] < SWEEP_CAP and st["rotations"] >= 0, st
    return st


# ---------------------------------------------------------------------------------------------------------------- 1. the solver
SOLVER_DIMS = (1, 2, 3, 5, 16, 63, 64, 65, 100, 127)


def solver_matrix(d):
    """(fp64 matrix, cond(Cn) of the longdouble covariance it was rounded from)"""
    n = 255 if d == 127 else 2 * d + 33
    cov = orc.covariance_hp(graded_chain(100 + d, n, d)[:, 2:])
    return cov.astype(np.float64), cond_cn(cov)


@pytest.mark.parametrize("d", SOLVER_DIMS)
def test_solver_against_truth_and_host(d):
    """no pair (d = 1), one pair, a bye (odd d), a half wave of pairs, 64 pairs, the LDS maximum: d <= 65 against eig_hp of the same
    matrix within the bound, d = 100 / 127 against the host solver within twice the bound (each is within the bound of the
    truth: the triangle inequality); canonical form, orthonormal vectors, scale = 1 / sqrt(lam), a small residual"""
    from mcevidence_amd import _capi
    M, cond = solver_matrix(d)
    evec, scale, lam, st = _capi.eig_sym_batch(M, mode=_capi.EIG_DEVICE)
    evec, scale, lam, st = evec[0], scale[0], lam[0], st[0]
    assert tuple(st[:2]) == (0, 0) and 1 <= st[2] < SWEEP_CAP and st[3] <= st[2] * d * (d - 1) // 2, st
    bound = C_FEED * EPS * cond
    if d <= 65:
        want = orc.eig_hp(M)[0].astype(np.float64)
        factor = 1.0
    else:
        _, _, want, hst = _capi.eig_sym_batch(M, mode=_capi.EIG_HOST)
        assert tuple(hst[0][:2]) == (0, 0)
        want, factor = want[0], 2.0
    rel = np.abs(lam - want) / want
    print("d=%d: sweeps %d rotations %d, max relative error %.3e, bound %.3e x %g" % (d, st[2], st[3], rel.max(), bound, factor))
    assert rel.max() <= factor * bound, (d, int(rel.argmax()), rel.max(), bound)
    assert_canonical(lam, evec)
    assert np.array_equal(scale, 1.0 / np.sqrt(lam))
    assert np.max(np.abs(evec.T @ evec - np.eye(d))) <= 64 * d * EPS
    assert np.max(np.abs(M @ evec - evec * lam)) <= 64 * d * EPS * np.max(np.abs(M))


# ---------------------------------------------------------------------------------------------------------------- 2. a batch
def test_batch_bad_systems_fail_alone_and_good_ones_are_bitwise_their_own():
    """300 systems at d = 8 in one call, one exactly singular, one with a NaN and one negative definite among them: each bad system
    has its own status and the identity / unit scales; every good one is bit for bit its own nsys = 1 solve, and a second run"""
    from mcevidence_amd import _capi
    rng = np.random.default_rng(5)
    d, nsys = 8, 300
    A = rng.standard_normal((nsys, d, 2 * d)) * np.logspace(-3, 2, d)[None, :, None]
    C = A @ A.transpose(0, 2, 1) / (2 * d - 1)
    C = 0.5 * (C + C.transpose(0, 2, 1))
    bad = {17: 2, 150: 1, 299: 2}
    C[17, 3, :] = 0.0
    C[17, :, 3] = 0.0                                # a zero row and column: an eigenvalue exactly 0, the smallest
    C[150, 2, 5] = C[150, 5, 2] = np.nan
    C[299] = -C[299]
    evec, scale, lam, st = _capi.eig_sym_batch(C, mode=_capi.EIG_DEVICE)
    evec2, scale2, lam2, st2 = _capi.eig_sym_batch(C, mode=_capi.EIG_DEVICE)
    _, _, lam_h, st_h = _capi.eig_sym_batch(C, mode=_capi.EIG_HOST)          # (each solver within the bound of the truth: twice the bound apart)
    assert np.array_equal(st_h[:, :2], st[:, :2])
    for i in range(nsys):
        if i in bad:
            assert st[i][0] == bad[i], (i, st[i])
            assert np.array_equal(evec[i], np.eye(d)) and np.array_equal(scale[i], np.ones(d)), i
            continue
        assert tuple(st[i][:2]) == (0, 0) and 1 <= st[i][2] < SWEEP_CAP, (i, st[i])
        e1, s1, l1, t1 = _capi.eig_sym_batch(C[i], mode=_capi.EIG_DEVICE)
        assert same(e1[0], evec[i]) and same(s1[0], scale[i]) and same(l1[0], lam[i]) and np.array_equal(t1[0], st[i]), i
        assert same(evec2[i], evec[i]) and same(scale2[i], scale[i]) and same(lam2[i], lam[i]) and np.array_equal(st2[i], st[i]), i
        assert_canonical(lam[i], evec[i])
        assert np.max(np.abs(lam[i] - lam_h[i]) / lam_h[i]) <= 2.0 * C_FEED * EPS * cond_cn(C[i]), i
    assert (st[17][1], st[150][2], st[299][1]) == (d - 1, 0, 0), (st[17], st[150], st[299])
    assert lam[17][-1] == 0.0 and np.all(lam[299] < 0)


# ---------------------------------------------------------------------------------------------------------------- 3. the feed routes
def _prefix_sizes(n, d):
    """two prefixes -- two systems in one launch -- where half the rows still give a well-conditioned covariance; else one"""
    return [n] if n < 2 * d + 12 else [n // 2, n]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_feed_routes_with_the_device_solver(key):
    """every feed route under eig_mode = EIG_DEVICE: eigenvalues, J and whitened rows against the truth, the sums against the
    option-off call within the device-vs-host bound, the routes against each other bit for bit (one covariance, one solver),
    and last_eig_stats: every system on the device, none on the host"""
    import torch
    from mcevidence_amd import _capi
    chain = tf._chain(key)
    S, w, fs = tf._inputs(chain)
    f = tf._truth(key)
    n, d = S.shape
    kmax = min(KMAX, n - 1)
    tol = 2.0 * max(LNE_TOL, d * C_FEED * EPS * f["condCn"])
    with host_eig():
        dotp_h, J_h, ev_h = _capi.evidence_feed(S, None, d, 0, kmax, w, fs)
    assert_stats(0, 1)
    dS, dw, df = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S, w, fs))
    logl = -chain[:, 1]
    dl = torch.from_numpy(np.ascontiguousarray(logl)).cuda()
    torch.cuda.synchronize()
    with device_eig():
        # evidence_feed
        dotp, J, ev = _capi.evidence_feed(S, None, d, 0, kmax, w, fs)
        st = assert_stats(1)
        used = check_eigs(ev, J, f, "evidence_feed")
        assert np.all(np.isfinite(dotp[1:])) and np.all(dotp[1:] > 0)
        diff = np.max(np.abs(np.log(dotp[1:]) - np.log(dotp_h[1:])))
        print("%s: sweeps %d rotations %d, eigenvalue error %.2f of the bound, |ln dotp_dev - ln dotp_host| = %.3e (tol %.3e)"
              % (key, st["max_sweeps"], st["rotations"], used, diff, tol))
        assert diff <= tol, (diff, tol)
        # evidence_feed_whiten / _dev
        for dev_inputs in (False, True):
            X = torch.empty((n, d), dtype=torch.float64, device="cuda")
            wo, fo = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            if dev_inputs:
                Jw, evw, _ = _capi.evidence_feed_whiten_dev(dS.data_ptr(), n, d, d, kmax, dw.data_ptr(), df.data_ptr(), X.data_ptr(), wo.data_ptr(),
                                                            fo.data_ptr())
            else:
                Jw, evw, _ = _capi.evidence_feed_whiten(S, d, kmax, w, fs, X.data_ptr(), wo.data_ptr(), fo.data_ptr())
            assert_stats(1)
            torch.cuda.synchronize()
            assert Jw == J and same(evw, ev), dev_inputs
            assert np.array_equal(wo.cpu().numpy(), w) and np.array_equal(fo.cpu().numpy(), fs)
            check_rows(X.cpu().numpy(), S, f)
        # evidence_feed_batch / _dev: three problems (piped), each the single call bit for bit
        out = _capi.evidence_feed_batch([(S, None, d, 0, kmax, w, fs)] * 3)
        assert_stats(3)
        out += _capi.evidence_feed_batch_dev([(dS.data_ptr(), n, d, 0, 0, 0, d, 0, kmax, dw.data_ptr(), df.data_ptr())] * 3)
        assert_stats(3)
        for dotp_b, J_b, ev_b in out:
            assert same(dotp_b, dotp) and J_b == J and same(ev_b, ev)
        # evidence_feed_part
        for nparts in (2, 3):
            tot = np.zeros(kmax)
            for r in range(nparts):
                part, Jp, evp, _ = _capi.evidence_feed_part(S, None, d, 0, kmax, w, fs, r, nparts)
                assert_stats(1)
                assert Jp == J and same(evp, ev), (nparts, r)
                tot += part
            assert np.allclose(tot[1:], dotp[1:], rtol=1e-12, atol=0), (nparts, tot, dotp)
        # evidence_feed_prefix: cov_mode 0 (one system of all rows), cov_mode 1 (every prefix's own, all in ONE launch), and the
        # device-pointer twin
        sizes = _prefix_sizes(n, d)
        p0 = sizes[0]
        dp0, lm0, jc0 = _capi.evidence_feed_prefix(S, None, d, 0, kmax, w, logl, sizes)
        assert_stats(1)
        assert np.all(jc0 == J) and lm0[-1] == logl.max()
        assert np.max(np.abs(np.log(dp0[-1][1:]) - np.log(dotp[1:]))) <= tol
        dp1, lm1, jc1 = _capi.evidence_feed_prefix(S, None, d, 1, kmax, w, logl, sizes)
        assert_stats(len(sizes))
        dp1d, lm1d, jc1d = _capi.evidence_feed_prefix_dev(dS.data_ptr(), n, d, 0, 0, 0, d, 1, kmax, dw.data_ptr(), dl.data_ptr(), sizes)
        assert_stats(len(sizes))
        assert same(dp1d, dp1) and same(jc1d, jc1) and same(lm1d, lm1)
        assert jc1[-1] == J and np.max(np.abs(np.log(dp1[-1][1:]) - np.log(dotp[1:]))) <= tol
        if len(sizes) > 1:          # the shorter prefix's own system: that of the feed of those rows alone
            own, J_own, _ = _capi.evidence_feed(S[:p0], None, d, 0, kmax, w[:p0], logl[:p0] - logl[:p0].max())
            assert jc1[0] == J_own and np.max(np.abs(np.log(dp1[0][1:]) - np.log(own[1:]))) <= tol
    with host_eig():
        dph, lmh, jch = _capi.evidence_feed_prefix(S, None, d, 1, kmax, w, logl, sizes)
    assert_stats(0, len(sizes))
    assert np.max(np.abs(np.log(dph[-1][1:]) - np.log(dp1[-1][1:]))) <= tol and same(lmh, lm1)


@pytest.mark.parametrize("key", ["graded27_n20000", "issue64_n20000"])
def test_two_eigen_systems_in_one_launch_against_their_own_truths(key):
    """cov_mode 1 with S2 (covtype 'single', cross evidence): both systems solved in one launch; s1's eigenvalues and J against
    s1's truth, the sums -- which see s2's system through every reference row -- against evidence_truth"""
    from mcevidence_amd import _capi
    chain = tf._chain(CASES[key])
    r1, r2 = tf._split(chain)
    tr = orc.evidence_truth(chain, kmax=KMAX, covtype="single", s1_idx=r1, s2_idx=r2)
    S, w, _ = tf._inputs(chain)
    d = S.shape[1]
    logL = -chain[r1, 1]
    with device_eig():
        dotp, J, ev = _capi.evidence_feed(S[r1], S[r2], d, 1, KMAX, w[r1], logL - logL.max())
    assert_stats(2)
    check_eigs(ev, J, tr["feed"], key + " s1")
    tol = max(LNE_TOL, d * C_FEED * EPS * max(tr["feed"]["condCn"], tr["feed2"]["condCn"]))
    assert np.max(np.abs(np.log(dotp) - np.log(tr["dotp"]))) <= tol, (np.log(dotp) - np.log(tr["dotp"]), tol)


# ---------------------------------------------------------------------------------------------------------------- 4. failures
def _nan_chain(n, d, seed):
    ch = graded_chain(seed, n, d, lo=1e-2, hi=1e1)
    ch[n // 3, 2 + d // 2] = np.nan
    return ch


def _zero_column_chain(n, d, seed):
    ch = graded_chain(seed, n, d, lo=1e-2, hi=1e1)
    ch[:, 3] = 0.0
    return ch


BAD = {"singular8_n3000": lambda: singular_chain(8, 3000), "zero_column_n3000x5": lambda: _zero_column_chain(3000, 5, 31),
       "nan_n3000x5": lambda: _nan_chain(3000, 5, 32), "nan_n70000x6": lambda: _nan_chain(70000, 6, 33)}


def _outcome(fn):
    try:
        return fn()
    except Exception as exc:          # noqa: BLE001 -- the outcome IS the exception
        return exc


def _masked(exc):
    """an exception's text with the eigenvalue a 'math domain error' quotes left out.  Where a covariance is singular by
    construction but not exactly (singular_chain, fewer rows than parameters), the eigenvalues that should be 0 are rounding
    noise of whichever solver ran -- 'eigenvalue 19 is -2.0e-11' from one, 'eigenvalue 20 is -4.9e-11' from the other -- so
    which of them is the first not > 0, and its value, are not the solvers' to agree on; everything else in the text is."""
    import re
    return re.sub(r"covariance eigenvalue \d+ is \S+ ", "covariance eigenvalue # is # ", str(exc))


def _same_failure(on, off, name):
    """the same exception type and message (the noise eigenvalue of a rounded singular matrix left out: _masked); for
    singular_chain, as in test_gpu_feeders, either solver may instead return a tiny eigenvalue"""
    if name.startswith("singular"):
        for r in (on, off):
            if isinstance(r, Exception):
                assert isinstance(r, ValueError) and "math domain error: covariance eigenvalue" in str(r), r
            else:
                assert r[2].min() < 1e-9 * r[2].max(), r[2]
        if isinstance(on, Exception) and isinstance(off, Exception):
            assert _masked(on) == _masked(off), (on, off)
        return
    assert isinstance(on, Exception) and type(on) is type(off) and str(on) == str(off), (name, on, off)


@pytest.mark.parametrize("name", list(BAD))
def test_a_failed_solve_is_reported_like_the_host_solvers(name):
    """alone and inside a batch of good problems: the exception of the option-off call, the good problems keep their results bit
    for bit, and the next call on the same process is correct.  (The 70 000-row chain is above the run-time certificate's
    65 536-row threshold: the certificate runs on the placeholder rows, and the solve's status takes precedence over it.)"""
    from mcevidence_amd import _capi
    S, w, fs = tf._inputs(BAD[name]())
    d = S.shape[1]
    gS, gw, gfs = tf._inputs(graded_chain(41, 2500, d, lo=1e-2, hi=1e1))
    good = (gS, None, d, 0, KMAX, gw, gfs)
    bad = (S, None, d, 0, KMAX, w, fs)
    with host_eig():
        off = _outcome(lambda: _capi.evidence_feed(*bad))
        off_batch = _capi.evidence_feed_batch([good, bad, good], return_exceptions=True)
    with device_eig():
        want = _capi.evidence_feed(*good)
        on = _outcome(lambda: _capi.evidence_feed(*bad))
        _same_failure(on, off, name)
        after = _capi.evidence_feed(*good)
        assert same(after[0], want[0]) and after[1] == want[1] and same(after[2], want[2])
        on_batch = _capi.evidence_feed_batch([good, bad, good], return_exceptions=True)
        _same_failure(on_batch[1], off_batch[1], name)
        for k in (0, 2):
            assert not isinstance(on_batch[k], Exception), on_batch[k]
            assert same(on_batch[k][0], want[0]) and on_batch[k][1] == want[1] and same(on_batch[k][2], want[2]), k
        if isinstance(on, Exception):
            with pytest.raises(type(on)):
                _capi.evidence_feed_batch([good, bad, good])
            pre = _outcome(lambda: _capi.evidence_feed_prefix(S, None, d, 0, KMAX, w, fs, [S.shape[0]]))
            with host_eig():
                pre_off = _outcome(lambda: _capi.evidence_feed_prefix(S, None, d, 0, KMAX, w, fs, [S.shape[0]]))
            _same_failure(pre, pre_off, name)
        again = _capi.evidence_feed(*good)
        assert same(again[0], want[0]) and again[1] == want[1]


# ---------------------------------------------------------------------------------------------------------------- 5. class and farm
@pytest.mark.parametrize("covtype", ["all", "single"])
@pytest.mark.parametrize("name", list(tf.CLASS_CASES))
def test_class_route_with_device_eig_against_truth(name, covtype):
    import mcevidence_amd as pkg
    chain = tf.CLASS_CASES[name]()
    tr = orc.evidence_truth(chain, kmax=KMAX, covtype=covtype)
    backend = pkg.HipBackend(device_eig=True)
    dev = pkg.MCEvidence([chain], kmax=KMAX, verbose=0, backend=backend).evidence(covtype=covtype)
    assert_stats(1)
    assert np.max(np.abs(dev - tr["lnE"])) < LNE_TOL, (dev - tr["lnE"])


def _lnE_tol(rows):
    d = rows.shape[1]
    return 2.0 * max(LNE_TOL, d * C_FEED * EPS * cond_cn(orc.covariance_hp(rows)))


def test_evidence_many_with_device_eig():
    """five small chains through evidence_many: one batched call, every system on the device, the option-off results within the
    device-vs-host bound"""
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import gaussian_chain
    chains = [gaussian_chain(seed=50 + k, n=2000 + 300 * k, d=4 + k, weights="int", cov="corr") for k in range(5)]
    host = pkg.HipBackend(device_eig=False)          # (one backend: evidence_many batches per backend)
    off = pkg.evidence_many([pkg.MCEvidence([c], kmax=KMAX, verbose=0, backend=host) for c in chains])
    assert_stats(0, 5)
    backend = pkg.HipBackend(device_eig=True)
    on = pkg.evidence_many([pkg.MCEvidence([c], kmax=KMAX, verbose=0, backend=backend) for c in chains])
    assert_stats(5)
    for c, a, b in zip(chains, on, off):
        assert np.max(np.abs(a - b)) <= _lnE_tol(c[:, 2:]), (a - b)


def test_farm_with_device_eig(tmp_path):
    """evidence_many_from_files(backend=HipBackend(device_eig=True)): chain roots through the farm route (every system on the
    device), and the reader's boundary files of tests/farm_cases.py as roots of their own -- most of which are no chain at all:
    whatever the option-off call makes of a root (a result or an exception), the option-on call makes the same of it"""
    import mcevidence_amd as pkg
    from mcevidence_amd.synth import planck_like_chains, write_cosmomc_chains
    from farm_cases import boundary_files
    roots, ndims = [], []
    for k, rows in enumerate([(900, 700), (1500,), (600, 500, 400)]):
        chs, _, ranges = planck_like_chains(seed=20 + k, rows=rows, nnuis=3 + k)
        root = os.path.join(str(tmp_path), "r%d" % k)
        write_cosmomc_chains(root, chs, ranges)
        roots.append(root)
        ndims.append(6)
    off = pkg.evidence_many_from_files(roots, kmax=3, ndim=ndims, info=True, backend=pkg.HipBackend(device_eig=False))
    on = pkg.evidence_many_from_files(roots, kmax=3, ndim=ndims, info=True, backend=pkg.HipBackend(device_eig=True))
    assert_stats(len(roots))
    for root, (a, ia), (b, ib) in zip(roots, on, off):
        assert ia["route"] == "farm" and ib["route"] == "farm"
        rows = np.vstack([np.loadtxt(root + "_%d.txt" % (i + 1)) for i in range(9) if os.path.exists(root + "_%d.txt" % (i + 1))])[:, 2:8]
        assert np.max(np.abs(a - b)) <= _lnE_tol(rows), (a - b)
    broots, bdims = [], []
    for name, data in boundary_files(big_rows=1500):
        with open(os.path.join(str(tmp_path), name + "_1.txt"), "wb") as fh:
            fh.write(data)
        ncols = len(data.split(b"\n", 1)[0].split()) if data.strip() else 3
        broots.append(os.path.join(str(tmp_path), name))
        bdims.append(max(ncols - 2, 1))
    off = pkg.evidence_many_from_files(broots, kmax=3, ndim=bdims, return_exceptions=True, backend=pkg.HipBackend(device_eig=False))
    on = pkg.evidence_many_from_files(broots, kmax=3, ndim=bdims, return_exceptions=True, backend=pkg.HipBackend(device_eig=True))
    results = 0
    for root, a, b in zip(broots, on, off):
        if isinstance(b, Exception):
            assert type(a) is type(b) and _masked(a) == _masked(b), (root, a, b)
        else:
            assert not isinstance(a, Exception), (root, a)
            results += 1
            assert np.allclose(a, b, rtol=0, atol=2.0 * LNE_TOL, equal_nan=True), (root, a, b)
    print("boundary files as roots: %d of %d gave a result, the rest the same exception either way" % (results, len(broots)))


# ---------------------------------------------------------------------------------------------------------------- 6. the guard
def test_option_off_is_the_host_solver_bit_for_bit():
    """without the option (and without MCE_FEED_EIG) the call solves on the host: every system counted there, none on the device,
    and the bits are those of an explicit EIG_HOST call and of a second call"""
    from mcevidence_amd import _capi
    assert os.environ.get("MCE_FEED_EIG") in (None, "host")
    S, w, fs = tf._inputs(tf._chain(CASES["graded27_n20000"]))
    d = S.shape[1]
    a = _capi.evidence_feed(S, None, d, 0, KMAX, w, fs)
    assert_stats(0, 1)
    b = _capi.evidence_feed(S, None, d, 0, KMAX, w, fs)
    with host_eig():
        c = _capi.evidence_feed(S, None, d, 0, KMAX, w, fs)
    assert_stats(0, 1)
    for x in (b, c):
        assert same(x[0], a[0]) and x[1] == a[1] and same(x[2], a[2])
    with device_eig():
        e = _capi.evidence_feed(S, None, d, 0, KMAX, w, fs)
    assert_stats(1)
    after = _capi.evidence_feed(S, None, d, 0, KMAX, w, fs)
    assert_stats(0, 1)
    assert same(after[0], a[0]) and after[1] == a[1] and same(after[2], a[2])
