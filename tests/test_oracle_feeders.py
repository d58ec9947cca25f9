"""Pins the high-precision feeder oracle (oracle/oracle_np.py: covariance_hp, eig_hp, jacobi_eig_ld, whiten_hp,
evidence_truth) that tests/test_gpu_feeders.py measures the device feeders against.  CPU only."""
import math
import sys
from fractions import Fraction

import numpy as np
import pytest

from helpers import LNE_TOL, chain_of, graded_cov, isotropic_chain, load_golden, orc, planck_allparams_chain, singular_chain

G = load_golden()
# the goldens that carry a chain recipe of their own (not the big, C4 and C5 configs: their mpmath solves are too slow)
PLAIN = sorted(n for n, c in G.items() if c["tag"] in ("small", "medium", "sym", "sym2") and not c.get("config"))
EPS_LD = float(np.finfo(np.longdouble).eps)


def _cond_n(C):
    C = np.asarray(C, dtype=np.float64)
    dg = np.sqrt(np.diag(C))
    e = np.linalg.eigvalsh(C / np.outer(dg, dg))
    return e[-1] / e[0]


def test_eig_hp_agrees_with_numpy_on_well_conditioned_input():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((12, 12))
    C = A @ A.T + 12 * np.eye(12)
    lam, U = orc.eig_hp(C)
    ev, V = orc.canonical_eig(*np.linalg.eigh(C))
    assert np.allclose(lam.astype(np.float64), ev, rtol=1e-14, atol=0)
    assert np.allclose(U.astype(np.float64), V, rtol=0, atol=1e-13)
    assert np.all(np.diff(lam.astype(np.float64)) < 0)
    big = np.argmax(np.abs(U.astype(np.float64)), axis=0)
    assert np.all(U[big, np.arange(12)] > 0)


def test_eig_hp_residuals_in_multiple_precision():
    """graded covariance (d = 27, cond(C) 3e14, cond(Cn) 8.4e4): ||A q_j - lam_j q_j|| / lam_j and ||Q^T Q - I|| in mpmath,
    for the pairs before rounding; and the longdouble pairs it returns are those, rounded"""
    import mpmath
    C = graded_cov(2)
    d = C.shape[0]
    lam, U, (E, Q) = orc.eig_hp(C, return_mp=True)
    with mpmath.workdps(34):
        A = mpmath.matrix(C.tolist())
        R = A * Q - Q * mpmath.diag(E)
        O = Q.T * Q - mpmath.eye(d)
        res = max(max(abs(R[i, j]) for i in range(d)) / abs(E[j]) for j in range(d))
        orth = max(abs(O[i, j]) for i in range(d) for j in range(d))
        assert res < 1e-25 and orth < 1e-25, (res, orth)
        assert all(abs(E[j] - mpmath.mpf(float(lam[j]))) <= 1e-15 * abs(E[j]) for j in range(d))
    assert float(lam[0] / lam[-1]) > 1e14


def test_longdouble_jacobi_matches_mpmath_on_a_graded_covariance():
    """the fallback (no mpmath): per-element Jacobi in longdouble, eigenvalues within eps_ld * cond(Cn) relative of mpmath's
    on the d = 40 graded covariance where a stopping rule relative to the largest eigenvalues loses 2e-9"""
    C = graded_cov(4)
    lam, U = orc.eig_hp(C)
    l2, U2 = orc.jacobi_eig_ld(C)
    rel = np.abs((l2 - lam) / lam).astype(np.float64)
    assert rel.max() < 16 * EPS_LD * _cond_n(C), rel.max()
    assert np.max(np.abs(U2 - U).astype(np.float64)) < 1e-12


def test_eig_hp_falls_back_without_mpmath(monkeypatch):
    C = graded_cov(1)
    want = orc.eig_hp(C)
    monkeypatch.setitem(sys.modules, "mpmath", None)            # `import mpmath` now raises ImportError
    lam, U = orc.eig_hp(C)
    assert np.max(np.abs((lam - want[0]) / want[0]).astype(np.float64)) < 16 * EPS_LD * _cond_n(C)
    with pytest.raises(ImportError):
        orc.eig_hp(C, return_mp=True)


def test_covariance_hp_is_exact_where_fp64_is_not():
    """rows far from the origin: covariance_hp against exact rational arithmetic; np.cov loses digits there"""
    rng = np.random.default_rng(4)
    rows = 1e8 + rng.integers(-1000, 1000, (301, 3)).astype(np.float64) / 64.0
    n = rows.shape[0]
    fr = [[Fraction(float(x)) for x in r] for r in rows]
    mean = [sum(r[c] for r in fr) / n for c in range(3)]
    exact = np.array([[float(sum((r[i] - mean[i]) * (r[j] - mean[j]) for r in fr) / (n - 1)) for j in range(3)] for i in range(3)])
    got = orc.covariance_hp(rows).astype(np.float64)
    assert np.allclose(got, exact, rtol=1e-15, atol=0)
    assert np.allclose(np.cov(rows.T), exact, rtol=1e-6)


def test_whiten_hp_matches_the_reference_whitening_on_well_conditioned_input():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((500, 6)) @ (np.eye(6) + 0.3 * rng.standard_normal((6, 6)))
    lam, U = orc.eig_hp(orc.covariance_hp(rows))
    X = orc.whiten_hp(rows, U, lam).astype(np.float64)
    assert np.allclose(X, orc.whiten(rows, U.astype(np.float64), lam.astype(np.float64)), rtol=0, atol=1e-13)
    assert np.allclose(np.cov(X.T), np.eye(6), atol=1e-13)


def test_chain_families_have_their_stated_shape():
    """what tests/test_gpu_feeders.py relies on: the Planck stand-in is ill-conditioned through near-functions, the
    isotropic chain has exactly repeated eigenvalues (up to rounding), the singular one a null direction"""
    ch = planck_allparams_chain(4, 5000)
    f = orc.feed_hp(ch[:, 2:])
    assert ch.shape[1] == 2 + 27 and f["condCn"] > 1e6 and 1e10 < f["condC"] < 1e17
    lam = orc.feed_hp(isotropic_chain(6, 3000)[:, 2:])["lam"].astype(np.float64)
    assert np.allclose(lam, np.repeat([10.0, 1.0, 0.1, 0.01], (4, 5, 3, 6)), rtol=1e-12)
    lam = orc.feed_hp(singular_chain(8, 3000)[:, 2:])["lam"].astype(np.float64)
    assert abs(lam[-1]) < 1e-14 * lam[0]


@pytest.mark.parametrize("name", PLAIN)
def test_evidence_truth_reproduces_the_reference_on_the_goldens(name):
    """on the goldens' well-conditioned chains the truth and the reference (np.cov + np.linalg.eig + sklearn) agree to
    LNE_TOL: the oracle computes the same estimator"""
    case = G[name]
    mk, ek = case["mce"], case["ev"]
    kw = dict(ndim=mk.get("ndim"), kmax=mk.get("kmax", 5), priorvolume=ek.get("pvolume") or mk.get("priorvolume", 1.0),
              pos_lnp=ek.get("pos_lnp", False))
    cov = ek.get("covtype", "all")
    kw["covtype"] = mk.get("covtype", "single") if cov is None else cov
    if mk.get("split"):
        kw["s1_idx"], kw["s2_idx"] = case["arrays"]["s1_idx"], case["arrays"]["s2_idx"]
    out = orc.evidence_truth(chain_of(case), **kw)
    assert np.max(np.abs(out["lnE"] - np.array(case["lnE"]))) <= LNE_TOL, out["lnE"] - np.array(case["lnE"])
    assert math.isclose(out["J"], case["J"], rel_tol=1e-12)
