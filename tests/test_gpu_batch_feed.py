"""Convergence batches on the device (mce_evidence_feed_prefix_f64, ``HipBackend(batch_feed=True)``): entry b must be what a
separate call on the first prefix[b] rows gives -- |d ln E| <= LNE_TOL for every batch and every k -- at the sizes where a prefix
ends inside a wave, at a workgroup edge and before the first full wave, for likelihood profiles that move the shift from
prefix to prefix, and through the class (reference MCEvidence.py:1034-1131 with nbatch / brange)."""
import numpy as np
import pytest

from helpers import LNE_TOL, gaussian_chain, host_pins

pytestmark = pytest.mark.gpu

N, D, KMAX, N2 = 1100, 5, 4, 700
#: wave edge (63, 64, 65), workgroup edges (255 .. 257, 511 .. 513), a duplicate, the full set, the smallest legal prefix (kmax + 1)
PREFIXES = [5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 513, 1100]


@pytest.fixture()
def capi():
    from mcevidence_amd import _capi
    _capi.require_device()
    return _capi


def _canonical_eig(rows):
    """eigen-system of the unweighted covariance in the library's documented form (descending, largest component positive)"""
    ev, U = np.linalg.eigh(np.atleast_2d(np.cov(rows.T)))
    ev, U = ev[::-1], U[:, ::-1]
    return ev, U * np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])


@pytest.fixture(scope="module")
def data():
    """one seeded shape for the ABI tests; the rows whitened on the host with the FULL sets' systems (the reference of
    cov_mode 0), computed once and never written to"""
    rng = np.random.default_rng(7)
    mix = np.eye(D) + 0.3 * rng.standard_normal((D, D))
    S1 = rng.standard_normal((N, D)) @ mix + rng.standard_normal(D)
    S2 = rng.standard_normal((N2, D)) @ mix
    ev, U = _canonical_eig(S1)
    evx, Ux = _canonical_eig(np.concatenate([S1, S2]))
    out = dict(S1=S1, S2=S2, w=np.ones(N), auto=((S1 @ U) / np.sqrt(ev), np.sqrt(np.prod(ev))),
               cross=((S1 @ Ux) / np.sqrt(evx), (S2 @ Ux) / np.sqrt(evx), np.sqrt(np.prod(evx))))
    base = -0.5 * np.einsum("ij,ij->i", out["auto"][0], out["auto"][0])
    step = 0.01 * base.copy()
    step[:300] -= 2000.0
    out["logl"] = {
        "increasing": np.sort(base),                              # every prefix has its own maximum
        "max_first": np.concatenate([[1.0], base[1:]]),           # the maximum at row 0
        "step": step,                                             # rows < 300 at -2000, the rest near 0
        "plain": base,
    }
    arrays = [S1, S2, out["w"], out["auto"][0], out["cross"][0], out["cross"][1]] + list(out["logl"].values())
    for a in arrays:
        a.setflags(write=False)
    return out


def _ln_terms(dotp, jac, lmax, k0):
    """what ln E_k of a batch is made of, up to terms that do not come from the library: ln(dotp_k J) + logLmax"""
    with np.errstate(all="ignore"):
        return np.log(np.asarray(dotp)[..., k0:] * np.asarray(jac)[..., None]) + np.asarray(lmax)[..., None]


def _assert_same(got, ref, what):
    err = np.abs(got - ref)
    print(what, "max |d ln E| =", np.nanmax(np.where(np.isfinite(err), err, 0.0)))
    # (identical non-finite values -- a prefix of d rows has a singular covariance, both sides then compute the same thing -- agree)
    assert np.array_equal(got, ref, equal_nan=True) or (np.isfinite(got).all() and np.isfinite(ref).all() and err.max() <= LNE_TOL), what


def _reference(capi, data, mode, w, logl, prefixes):
    """B separate calls: (dotp[B, kmax], jac[B], lmax[B]) and the prefixes whose call raised ValueError"""
    dotp, jac, lmax, failed = [], [], [], []
    for b, p in enumerate(prefixes):
        m = np.amax(logl[:p])
        fs = logl[:p] - m
        try:
            if mode == "single":                    # the feed of the first p rows, as it is
                dp, j, _ = capi.evidence_feed(data["S1"][:p], None, D, 1, KMAX, w[:p], fs)
            elif mode == "all":                     # rows pre-whitened on the host with the full set's system
                dp, j = capi.knn_dotp(data["auto"][0][:p], None, w[:p], fs, KMAX, 1), data["auto"][1]
            else:                                   # cross: ... of s1 U s2; every batch searches all of s2
                dp, j = capi.knn_dotp(data["cross"][0][:p], data["cross"][1], w[:p], fs, KMAX, 0), data["cross"][2]
        except ValueError:
            failed.append(b)
            dp, j = np.full(KMAX, np.nan), np.nan
        dotp.append(dp)
        jac.append(j)
        lmax.append(m)
    return np.array(dotp), np.array(jac), np.array(lmax), failed


def _prefix_call(capi, data, mode, w, logl, prefixes):
    return capi.evidence_feed_prefix(data["S1"], data["S2"] if mode == "cross" else None, D, 1 if mode == "single" else 0, KMAX, w, logl, prefixes)


def _check(capi, data, mode, w, logl, prefixes=PREFIXES):
    k0 = 0 if mode == "cross" else 1
    rd, rj, rl, failed = _reference(capi, data, mode, w, logl, prefixes)
    if failed:
        # a prefix whose own covariance is not positive definite fails the separate call, and the whole batched call, which names it
        with pytest.raises(ValueError, match="prefix %d " % failed[0]):
            _prefix_call(capi, data, mode, w, logl, prefixes)
        keep = [b for b in range(len(prefixes)) if b not in failed]
        prefixes, rd, rj, rl = [prefixes[b] for b in keep], rd[keep], rj[keep], rl[keep]
    dotp, lmax, jac = _prefix_call(capi, data, mode, w, logl, prefixes)
    assert dotp.shape == (len(prefixes), KMAX) and np.array_equal(lmax, rl)          # the shift is an exact maximum
    if k0 == 1:
        assert (dotp[:, 0] == 0).all()
    _assert_same(_ln_terms(dotp, jac, lmax, k0), _ln_terms(rd, rj, rl, k0), "%s" % mode)
    if mode == "single":
        assert np.array_equal(jac, rj)          # the same covariance kernels and solver on the same rows
    else:
        assert np.allclose(jac, rj, rtol=1e-12) and (jac == jac[0]).all()          # ONE system of all rows, the same for every b
    return prefixes, dotp, lmax, jac


@pytest.mark.parametrize("mode", ["all", "single", "cross"])
@pytest.mark.parametrize("profile", ["increasing", "max_first", "step"])
def test_abi_prefixes_equal_separate_calls(capi, data, mode, profile):
    logl = data["logl"][profile]
    prefixes, dotp, lmax, _ = _check(capi, data, mode, data["w"], logl)
    dup = prefixes.index(513)
    assert prefixes[dup + 1] == 513 and np.array_equal(dotp[dup], dotp[dup + 1])                # the duplicate prefix
    if profile == "increasing":
        assert len(set(lmax.tolist())) == len(set(prefixes))
    if profile == "step":
        # the short prefixes lie 2000 below the chain's maximum: a globally shifted sum would be exp(-2000) = 0
        # (under its own system the prefix of d rows is singular: its sum is compared above, but need not be positive)
        short = [b for b, p in enumerate(prefixes) if p <= 257 and not (mode == "single" and p <= D)]
        k0 = 0 if mode == "cross" else 1
        assert len(short) >= 6 and (lmax[short] < -1990).all() and np.isfinite(dotp[short]).all() and (dotp[short][:, k0:] > 0).all()


@pytest.mark.parametrize("mode", ["all", "single", "cross"])
def test_weights_and_a_row_of_zero_likelihood(capi, data, mode):
    rng = np.random.default_rng(11)
    w = rng.uniform(0.25, 7.5, N)
    w[100] = -1.75                                          # the reference keeps a negative weight's signed term
    logl = data["logl"]["plain"].copy()
    logl[50] = -np.inf                                      # exp(-inf) = 0: a harmless zero term
    _check(capi, data, mode, w, logl)


@pytest.mark.parametrize("mode", ["all", "single", "cross"])
def test_nan_likelihood_poisons_the_prefixes_that_hold_it(capi, data, mode):
    logl = data["logl"]["plain"].copy()
    logl[400] = np.nan
    # (under its own system the prefix of d rows is singular; it is covered where the whole call is compared with separate calls)
    prefixes = PREFIXES[1:] if mode == "single" else PREFIXES
    nb = sum(1 for p in prefixes if p <= 400)
    dotp, lmax, jac = _prefix_call(capi, data, mode, data["w"], logl, prefixes)
    k0 = 0 if mode == "cross" else 1
    for b, p in enumerate(prefixes):
        if p > 400:
            assert np.isnan(lmax[b]) and np.isnan(dotp[b, k0:]).all(), (p, lmax[b], dotp[b])
    # ... and the values below are finite, and what the same call without the NaN gives
    rd, rl, rj = _prefix_call(capi, data, mode, data["w"], data["logl"]["plain"], prefixes)
    assert nb >= 6 and np.array_equal(lmax[:nb], rl[:nb]) and np.isfinite(lmax[:nb]).all() and np.isfinite(dotp[:nb]).all()
    _assert_same(_ln_terms(dotp[:nb], jac[:nb], lmax[:nb], k0), _ln_terms(rd[:nb], rj[:nb], rl[:nb], k0), "below the NaN, %s" % mode)


def test_device_pointer_twin(capi, data):
    import torch
    dev = torch.device("cuda", 0)
    S1, S2 = torch.from_numpy(data["S1"].copy()).to(dev), torch.from_numpy(data["S2"].copy()).to(dev)
    w, logl = torch.from_numpy(data["w"].copy()).to(dev), torch.from_numpy(data["logl"]["step"].copy()).to(dev)
    torch.cuda.synchronize()
    for mode in ("all", "single", "cross"):
        prefixes = PREFIXES[1:]                 # (without the prefix of d rows, singular under its own system)
        a = _prefix_call(capi, data, mode, data["w"], data["logl"]["step"], prefixes)
        b = capi.evidence_feed_prefix_dev(S1.data_ptr(), N, D, S2.data_ptr() if mode == "cross" else 0, N2, D, D, 1 if mode == "single" else 0, KMAX,
                                          w.data_ptr(), logl.data_ptr(), prefixes)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), mode
    assert np.array_equal(S1.cpu().numpy(), data["S1"])          # the inputs are copied, not modified


def test_medium_prefixes_with_different_plans_and_the_default_certificate(capi):
    """20 000 x 6, kmax = 3, prefixes 300 / 3000 / 20 000: the three searches take different plans out of one workspace.  The
    library's default certificate stays on.  Below 65 536 query rows it samples one search in eight (a per-thread counter:
    tests/test_gpu_verify.py pins that rule), so eight calls hold at least one certified search whatever the counter was; mce_last_verify_rows() counts the rows of all searches of a call."""
    n, d, kmax, prefixes = 20000, 6, 3, [300, 3000, 20000]
    chain = gaussian_chain(seed=2, n=n, d=d, weights="int", cov="corr")
    w, logl, S = np.ascontiguousarray(chain[:, 0]), -np.ascontiguousarray(chain[:, 1]), np.ascontiguousarray(chain[:, 2:])
    ev, U = _canonical_eig(S)
    Xw = (S @ U) / np.sqrt(ev)
    for mode in ("all", "single"):
        dotp, lmax, jac = capi.evidence_feed_prefix(S, None, d, 1 if mode == "single" else 0, kmax, w, logl, prefixes)
        ref = []
        for p in prefixes:
            fs = logl[:p] - np.amax(logl[:p])
            if mode == "single":
                dp, j, _ = capi.evidence_feed(S[:p], None, d, 1, kmax, w[:p], fs)
            else:
                dp, j = capi.knn_dotp(Xw[:p], None, w[:p], fs, kmax, 1), np.sqrt(np.prod(ev))
            ref.append(np.log(dp[1:] * j) + np.amax(logl[:p]))
        _assert_same(_ln_terms(dotp, jac, lmax, 1), np.array(ref), "medium %s" % mode)
    ran = []
    for _ in range(8):
        capi.evidence_feed_prefix(S, None, d, 0, kmax, w, logl, prefixes)
        ran.append(capi.last_verify_rows())
    print("rows certified per call:", ran)
    assert max(ran) > 0 and all(r % 256 == 0 for r in ran)
    with capi.options(verify=100):                  # asked for: every search of the call
        capi.evidence_feed_prefix(S, None, d, 0, kmax, w, logl, prefixes)
    assert capi.last_verify_rows() == 300
    with capi.options(verify=0):
        capi.evidence_feed_prefix(S, None, d, 0, kmax, w, logl, prefixes)
    assert capi.last_verify_rows() == 0


# ---------------------------------------------------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------------------------------------------------
def _mce(chain, batch_feed, kmax=3, nbatch=3, brange=(2.5, 3.5), split_rows=None):
    import mcevidence_amd as pkg
    m = pkg.MCEvidence([chain], kmax=kmax, verbose=0, nbatch=nbatch, brange=list(brange), bscale="logpower",
                       backend=pkg.HipBackend(batch_feed=batch_feed))
    if split_rows is not None:
        m.set_split(*split_rows)
    return m


def test_pin_against_the_reference(capi):
    p = host_pins()["batch_logpower"]
    ch = gaussian_chain(seed=0, n=4000, d=4)
    new = _mce(ch, True)
    assert new.nchain.tolist() == p["nchain"]
    lnE = new.evidence()
    print("pin: max |d ln E| =", np.max(np.abs(lnE - np.array(p["lnE"]))))
    assert np.max(np.abs(lnE - np.array(p["lnE"]))) <= LNE_TOL
    assert np.max(np.abs(lnE - _mce(ch, False).evidence())) <= LNE_TOL


@pytest.mark.parametrize("case", ["auto_all", "auto_single", "split_all"])
def test_class_route_equals_the_host_loop(capi, case, monkeypatch):
    ch = gaussian_chain(seed=3, n=3000, d=5, weights="int", cov="corr")
    split = case == "split_all"
    rows = (np.arange(0, 1800), np.arange(1800, 3000)) if split else None
    brange = (2.3, np.log10(1800.5 if split else 3000.5))
    covtype = "single" if case == "auto_single" else "all"
    new = _mce(ch, True, kmax=4, nbatch=4, brange=brange, split_rows=rows)
    calls = []
    real = new.backend.evidence_feed_prefix
    monkeypatch.setattr(new.backend, "evidence_feed_prefix", lambda *a: calls.append(1) or real(*a))
    a = new.evidence(covtype=covtype)
    b = _mce(ch, False, kmax=4, nbatch=4, brange=brange, split_rows=rows).evidence(covtype=covtype)
    assert calls == [1] and a.shape == b.shape == (4, 3)
    print(case, "max |d ln E| =", np.max(np.abs(a - b)))
    assert np.max(np.abs(a - b)) <= LNE_TOL


def test_evidence_many_with_batched_and_plain_objects(capi):
    import mcevidence_amd as pkg
    chains = [gaussian_chain(seed=s, n=2500, d=4) for s in range(4)]
    be = pkg.HipBackend(batch_feed=True)

    def objects():
        return [pkg.MCEvidence([chains[0]], kmax=3, verbose=0, nbatch=3, brange=[2.3, 3.3], bscale="logpower", backend=be),
                pkg.MCEvidence([chains[1]], kmax=3, verbose=0, backend=be),
                pkg.MCEvidence([chains[2]], kmax=3, verbose=0, nbatch=2, brange=[2.5, 3.0], bscale="logpower", backend=be),
                pkg.MCEvidence([chains[3]], kmax=3, verbose=0, backend=be)]
    many = pkg.evidence_many(objects())
    for got, m in zip(many, objects()):
        one = m.evidence()
        assert got.shape == one.shape and np.array_equal(got, one)
    assert many[0].shape == (3, 2) and many[1].shape == (2,)
