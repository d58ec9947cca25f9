"""Convergence batches (nbatch / brange) through ``backend.evidence_feed_prefix``: argument validation of the C entry point
without a GPU, and the routing of ``MCEvidence.evidence()`` pinned on a NumPy backend that gives every prefix exact
brute-force neighbours.  CPU only."""
import numpy as np
import pytest

import mcevidence_amd as pkg
from helpers import LNE_TOL, OracleBackend, OracleFeedBackend, gaussian_chain, host_pins
from mcevidence_amd import _capi

PINS = host_pins()


# ---------------------------------------------------------------------------------------------------------------------
# the C entry point: argument errors need no device
# ---------------------------------------------------------------------------------------------------------------------
def _raw_call(n1=40, d=3, kmax=3, prefix=(10, 20, 40), cov_mode=0, n2=0, null=None, nprefix=None, dev_variant=False):
    """mce_evidence_feed_prefix_f64 through the bare ctypes symbol -> its return code"""
    lib = _capi.load()
    rng = np.random.default_rng(0)
    S1 = rng.standard_normal((n1, d))
    S2 = rng.standard_normal((n2, d)) if n2 else None
    w, logl = np.ones(n1), -rng.random(n1)
    pre = np.asarray(prefix, dtype=np.int64)
    B = len(pre) if nprefix is None else nprefix
    out, lmax, jac = np.zeros((max(B, 1), kmax)), np.zeros(max(B, 1)), np.zeros(max(B, 1))
    args = dict(S1=S1.ctypes.data, w=w.ctypes.data, logl=logl.ctypes.data, prefix=pre.ctypes.data if len(pre) else None, dotp=out.ctypes.data,
                loglmax=lmax.ctypes.data, jacobian=jac.ctypes.data)
    if null:
        args[null] = None
    fn = lib.mce_evidence_feed_prefix_dev_f64 if dev_variant else lib.mce_evidence_feed_prefix_f64
    return fn(args["S1"], n1, d, S2.ctypes.data if n2 else None, n2, d if n2 else 0, d, cov_mode, kmax, args["w"], args["logl"], args["prefix"], B,
              args["dotp"], args["loglmax"], args["jacobian"], 0)


@pytest.mark.parametrize("null", ["S1", "w", "logl", "prefix", "dotp", "loglmax", "jacobian"])
def test_null_pointers_are_invalid(null):
    assert _raw_call(null=null) == _capi.MCE_ERR_INVALID
    assert _raw_call(null=null, dev_variant=True) == _capi.MCE_ERR_INVALID
    assert "null pointer" in _capi.last_error()


def test_prefix_list_errors():
    assert _capi.MCE_MAX_PREFIX == 256
    assert _raw_call(nprefix=0) == _capi.MCE_ERR_INVALID                                  # nprefix < 1
    assert _raw_call(n1=400, prefix=[100] * 257) == _capi.MCE_ERR_INVALID                 # nprefix > MCE_MAX_PREFIX
    assert "256" in _capi.last_error()
    assert _raw_call(prefix=(10, 30, 20)) == _capi.MCE_ERR_INVALID                        # not non-decreasing
    assert "prefix 2" in _capi.last_error()
    assert _raw_call(prefix=(10, 20, 41)) == _capi.MCE_ERR_INVALID                        # prefix[b] > n1
    assert "prefix 2" in _capi.last_error() and "n1=40" in _capi.last_error()
    assert _raw_call(kmax=3, prefix=(3, 20, 40)) == _capi.MCE_ERR_INVALID                 # prefix[b] < kmax + 1
    assert "prefix 0" in _capi.last_error()
    assert _raw_call(cov_mode=1, n2=30) == _capi.MCE_ERR_INVALID                          # cov_mode 1 with S2
    assert "cov_mode 1" in _capi.last_error()
    assert _raw_call(cov_mode=2) == _capi.MCE_ERR_INVALID
    assert _raw_call(n1=200, d=128, prefix=(150, 200)) == _capi.MCE_ERR_DIM_RANGE         # d > 127
    with pytest.raises(ValueError, match="exceeds n1"):
        _capi.evidence_feed_prefix(np.zeros((40, 3)), None, 3, 0, 3, np.ones(40), np.zeros(40), [10, 50])
    with pytest.raises(ValueError, match="one entry per s1 row"):
        _capi.evidence_feed_prefix(np.zeros((40, 3)), None, 3, 0, 3, np.ones(39), np.zeros(40), [10, 40])
    with pytest.raises(ValueError):
        _capi.evidence_feed_prefix_dev(0, 40, 3, 0, 0, 0, 3, 0, 3, 0, 0, [10, 40])        # null device pointers


def test_a_valid_call_fails_loudly_without_a_device():
    if _capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _raw_call() == _capi.MCE_ERR_NO_DEVICE                                         # the smallest legal prefix is kmax + 1:
    assert _raw_call(kmax=3, prefix=(4, 4, 40)) == _capi.MCE_ERR_NO_DEVICE                # passes the checks, then needs the GPU
    assert _raw_call(n2=30) == _capi.MCE_ERR_NO_DEVICE
    assert _raw_call(cov_mode=1) == _capi.MCE_ERR_NO_DEVICE
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.evidence_feed_prefix(np.random.default_rng(1).standard_normal((40, 3)), None, 3, 0, 3, np.ones(40), np.zeros(40), [10, 40])
    ch = gaussian_chain(seed=0, n=400, d=3)
    with pytest.raises(RuntimeError):                                                     # the class: no quiet fall-back either
        pkg.MCEvidence([ch], kmax=3, verbose=0, nbatch=2, brange=[2.0, 2.5], bscale="logpower", backend=pkg.HipBackend(batch_feed=True)).evidence()


def test_backend_switch(monkeypatch):
    monkeypatch.delenv("MCE_BATCH_FEED", raising=False)
    assert pkg.HipBackend().batch_feed is False                                           # opt-in
    assert pkg.HipBackend(batch_feed=True).batch_feed is True
    monkeypatch.setenv("MCE_BATCH_FEED", "1")
    assert pkg.HipBackend().batch_feed is True and pkg.HipBackend(batch_feed=False).batch_feed is False
    monkeypatch.setenv("MCE_BATCH_FEED", "0")
    assert pkg.HipBackend().batch_feed is False
    # declines (None: the caller falls back) before it touches the library: off, > 127 parameters, a multi-device selection
    X, w = np.zeros((40, 3)), np.ones(40)
    assert pkg.HipBackend(batch_feed=False).evidence_feed_prefix(X, None, 3, 0, 3, w, w, [10, 40]) is None
    assert pkg.HipBackend(batch_feed=True).evidence_feed_prefix(np.zeros((300, 128)), None, 128, 0, 3, np.ones(300), np.ones(300), [200, 300]) is None
    assert pkg.HipBackend(batch_feed=True, devices=[0, 1]).evidence_feed_prefix(X, None, 3, 0, 3, w, w, [10, 40]) is None
    assert pkg.HipBackend(batch_feed=True, devices=[1]).evidence_feed_prefix(X, None, 3, 0, 3, w, w, [10, 40]) is None


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
class OraclePrefixBackend(OracleFeedBackend):
    """``evidence_feed_prefix`` with the contract of mce_evidence_feed_prefix_f64 in NumPy: cov_mode 0 whitens with the
    eigen-system of ALL rows of s1 (and s2), cov_mode 1 with each prefix's own; every prefix gets exact brute-force neighbours."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.prefix_calls = []

    @staticmethod
    def _eig(rows):
        ev, U = np.linalg.eigh(np.atleast_2d(np.cov(rows.T)))
        if (ev <= 0).any():
            raise ValueError("math domain error")
        ev, U = ev[::-1], U[:, ::-1]
        return ev, U * np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])

    def evidence_feed_prefix(self, S1, S2, ndim, cov_mode, kmax, weight, logL, sizes):
        s1 = np.asarray(S1)[:, :ndim]
        s2 = None if S2 is None else np.asarray(S2)[:, :ndim]
        assert not (cov_mode == 1 and s2 is not None)
        self.prefix_calls.append(list(sizes))
        dotp, lmax, jac = np.zeros((len(sizes), kmax)), np.zeros(len(sizes)), np.zeros(len(sizes))
        if cov_mode == 0:
            ev, U = self._eig(s1 if s2 is None else np.concatenate([s1, s2]))
        for b, p in enumerate(sizes):
            if cov_mode == 1:
                ev, U = self._eig(s1[:p])
            X = (s1[:p] @ U) / np.sqrt(ev)
            Y = None if s2 is None else (s2 @ U) / np.sqrt(ev)
            lmax[b] = np.amax(logL[:p])
            dotp[b], _ = self.knn_dotp(X, Y, weight[:p], logL[:p] - lmax[b], kmax, 0 if s2 is not None else 1)
            jac[b] = np.sqrt(np.prod(ev))
        return dotp, lmax, jac


def _batched(chain, backend, kmax=3, nbatch=3, brange=(2.5, 3.5), split_rows=None, **kw):
    m = pkg.MCEvidence([chain], kmax=kmax, verbose=0, nbatch=nbatch, brange=list(brange), bscale="logpower", backend=backend, **kw)
    if split_rows is not None:
        m.set_split(*split_rows)
    return m


def test_pin_through_the_new_route():
    ch = gaussian_chain(seed=0, n=4000, d=4)
    p = PINS["batch_logpower"]
    be = OraclePrefixBackend()
    m = _batched(ch, be)
    assert m.nchain.tolist() == p["nchain"]
    lnE = m.evidence()
    assert be.prefix_calls == [[row[0] for row in p["nchain"]]]
    print("pin: max |dlnE| =", np.max(np.abs(lnE - np.array(p["lnE"]))))
    assert np.allclose(lnE, np.array(p["lnE"]), atol=LNE_TOL)


ROUTE_CASES = {
    "auto_all": dict(covtype="all"),
    "auto_single": dict(covtype="single"),
    "split_all": dict(covtype="all", split=True),
}


@pytest.mark.parametrize("case", sorted(ROUTE_CASES))
def test_route_equals_the_host_loop(case):
    cfg = ROUTE_CASES[case]
    ch = gaussian_chain(seed=3, n=3000, d=5, weights="int", cov="corr")
    rows = (np.arange(0, 1800), np.arange(1800, 3000)) if cfg.get("split") else None
    brange = (2.3, np.log10(1800.5)) if cfg.get("split") else (2.3, np.log10(3000.5))      # up to ALL of s1
    host_be, new_be = OracleBackend(), OraclePrefixBackend()
    host = _batched(ch, host_be, kmax=4, nbatch=4, brange=brange, split_rows=rows)
    new = _batched(ch, new_be, kmax=4, nbatch=4, brange=brange, split_rows=rows)
    a = host.evidence(covtype=cfg["covtype"])
    b = new.evidence(covtype=cfg["covtype"])
    assert len(host_be.calls) == 4 and new_be.prefix_calls == [[int(x[0]) for x in new.nchain]]
    assert new.nchain[-1][0] == (1800 if cfg.get("split") else 3000)
    assert a.shape == b.shape == (4, 3)
    print(case, "max |dlnE| =", np.max(np.abs(a - b)))
    assert np.max(np.abs(a - b)) <= LNE_TOL
    # info=True and pvolume travel as in the host loop
    c, info = new.evidence(covtype=cfg["covtype"], info=True, pvolume=2.0)
    assert info is new.info and np.allclose(c, b - np.log(2.0), atol=1e-12)


def test_pos_lnp_and_verbose_one():
    ch = gaussian_chain(seed=5, n=1500, d=3)
    host = _batched(ch, OracleBackend(), brange=(2.2, 3.1))
    be = OraclePrefixBackend()
    new = _batched(ch, be, brange=(2.2, 3.1))
    assert np.max(np.abs(host.evidence(pos_lnp=True) - new.evidence(pos_lnp=True))) <= LNE_TOL
    assert np.max(np.abs(host.evidence(verbose=1) - new.evidence(verbose=1))) <= LNE_TOL
    assert len(be.prefix_calls) == 2


def test_what_keeps_the_host_loop():
    ch = gaussian_chain(seed=0, n=2000, d=3)
    # rand=True
    be = OraclePrefixBackend()
    np.random.seed(1)
    _batched(ch, be, brange=(2.5, 3.2)).evidence(rand=True)
    assert be.prefix_calls == [] and len(be.calls) == 3
    # verbose=2 (the per-neighbour debug output wants the distances)
    be = OraclePrefixBackend()
    _batched(ch, be, brange=(2.5, 3.2)).evidence(verbose=2)
    assert be.prefix_calls == [] and len(be.calls) == 3
    # split + 'single': two eigen-systems whose conventions are np.linalg.eig's
    be = OraclePrefixBackend()
    _batched(ch, be, brange=(2.5, 2.9), split_rows=(np.arange(0, 1000), np.arange(1000, 2000))).evidence(covtype="single")
    assert be.prefix_calls == [] and len(be.calls) == 3
    # a covtype the routes do not know: the host loop's own error
    be = OraclePrefixBackend()
    with pytest.raises(Exception):
        _batched(ch, be, brange=(2.5, 3.2)).evidence(covtype="none")
    assert be.prefix_calls == []
    # a batch larger than n1: the host loop raises what it always raised
    be, host_be = OraclePrefixBackend(), OracleBackend()
    with pytest.raises(Exception) as new_exc:
        _batched(ch, be, brange=(2.5, 3.5)).evidence()
    with pytest.raises(Exception) as host_exc:
        _batched(ch, host_be, brange=(2.5, 3.5)).evidence()
    assert be.prefix_calls == [] and type(new_exc.value) is type(host_exc.value) and str(new_exc.value) == str(host_exc.value)
    # a batch smaller than kmax + 1
    be = OraclePrefixBackend()
    with pytest.raises(Exception):
        _batched(ch, be, kmax=5, brange=(0.5, 3.0)).evidence()
    assert be.prefix_calls == []
    # a backend without the method; and one that declines
    be = OracleFeedBackend()
    a = _batched(ch, be, brange=(2.5, 3.2)).evidence()
    assert len(be.calls) == 3

    class Declines(OraclePrefixBackend):
        def evidence_feed_prefix(self, *args):
            self.prefix_calls.append("asked")
            return None
    be = Declines()
    b = _batched(ch, be, brange=(2.5, 3.2)).evidence()
    assert be.prefix_calls == ["asked"] and len(be.calls) == 3 and np.array_equal(a, b)
    # no batches: the plain feed route, as before
    be = OraclePrefixBackend()
    pkg.MCEvidence([ch], kmax=3, verbose=0, backend=be).evidence()
    assert be.prefix_calls == [] and len(be.calls) == 1


def test_evidence_many_reaches_the_route_by_itself():
    chains = [gaussian_chain(seed=s, n=1500, d=3) for s in range(4)]
    be = OraclePrefixBackend()
    ms = [_batched(chains[0], be, brange=(2.2, 3.1)), pkg.MCEvidence([chains[1]], kmax=3, verbose=0, backend=be),
          _batched(chains[2], be, brange=(2.4, 3.0), nbatch=2), pkg.MCEvidence([chains[3]], kmax=3, verbose=0, backend=be)]
    many = pkg.evidence_many(ms)
    assert len(be.prefix_calls) == 2 and be.batches == [2]
    for m, got in zip(ms, many):
        assert np.array_equal(got, m.evidence())
