"""The cases and the oracle of the Gelman-Rubin R-1 (converge=): docs/design/chain_conv.md states the rule and derives the bound.

The MODEL evaluates the rule with the moments in ``np.longdouble`` after subtracting a pivot row IN longdouble (without the pivot the
longdouble model itself is only good to about 2e-8 on the offset case C), and steps 7 and 8 in ``mpmath`` at 50 digits: Cholesky
``Wn = L L^T``, then the largest eigenvalue of ``L^-1 Bn L^-T`` by ``mp.eigsy`` -- on ``Z^T Z / (M - 1)``, ``Z = L^-1 D^T`` with D the
M rows ``delta_s / sigma``, where M < d: the two products have the same non-zero eigenvalues and the smaller one is solved.
``kappa = cond(Wn)`` only scales the bound; fp64 gives it.

The BOUND (U = the rows of the largest segment, d = ndim, eps = 2^-52):
    |d r_minus_1|    <= (4 d (U + 1) eps + 32 eps) kappa (1 + r_minus_1) + 16 eps (1 + r_minus_1)^2
    |d per_param[j]| <= 16 U eps (per_j + sqrt(per_j))
A case is accepted only if its bound is below 1e-3 of its own r_minus_1."""
import functools

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble

NUMERIC = ("A", "B", "C", "D", "E", "F", "G", "H", "I", "J")
STATUS = ("S2", "S3nan", "S3inf", "S3neg", "S3both", "S4")
BY = ("chains", "halves")


def _chain(rng, n, d, mean=0.0, scale=1.0, weights=None):
    """rows [w, lnlike, d parameters]"""
    out = np.empty((n, d + 2))
    out[:, 0] = 1.0 if weights is None else weights
    out[:, 1] = rng.random(n)
    out[:, 2:] = mean + scale * rng.standard_normal((n, d))
    return out


@functools.lru_cache(maxsize=None)
def parts(name):
    """the chains of a case (a tuple of read-only arrays)"""
    rng = np.random.default_rng([ord(c) for c in name] + [2026])
    if name == "A":
        out = [_chain(rng, 257, 3, mean=0.1 * rng.standard_normal(3)) for _ in range(4)]
    elif name == "B":
        out = [_chain(rng, n, 2, mean=0.05 * rng.standard_normal(2)) for n in (300, 2, 1, 0, 300)]
    elif name == "C":
        out = [_chain(rng, 1025, 4, mean=1e8 + 1e-3 * rng.standard_normal(4), scale=1e-2, weights=rng.integers(1, 4, 1025).astype(float)) for _ in range(3)]
    elif name == "D":
        mix = np.eye(8) + 0.999 * np.ones((8, 8))
        out = []
        for _ in range(8):
            c = _chain(rng, 1023, 8, mean=0.08 * rng.standard_normal(8))
            c[:, 2:] = c[:, 2:] @ mix.T
            out.append(c)
    elif name == "E":
        out = [_chain(rng, 600, 127, mean=0.02 * rng.standard_normal(127)) for _ in range(2)]
    elif name == "F":
        out = [_chain(rng, 300, 5, mean=0.05 * rng.standard_normal(5), weights=rng.integers(1, 5, 300).astype(float)) for _ in range(64)]
    elif name == "G":
        out = []
        for k in range(4):
            e = rng.standard_normal((2000, 6)) * np.sqrt(1.0 - 0.9 ** 2)
            x = np.empty((2000, 6))
            x[0] = rng.standard_normal(6)
            for i in range(1, 2000):
                x[i] = 0.9 * x[i - 1] + e[i]
            c = _chain(rng, 2000, 6)
            c[:, 2:] = x + (0.5 if k == 2 else 0.0)
            out.append(c)
    elif name == "H":
        scales = 10.0 ** np.array([-6.0, -3.0, 0.0, 3.0, 6.0])
        out = [_chain(rng, 500, 5, mean=0.1 * rng.standard_normal(5) * scales, scale=scales) for _ in range(4)]
    elif name == "I":
        out = []
        for k in range(4):
            w = rng.random(400) * 3.0
            w[rng.random(400) < 0.2] = 0.0
            if k == 1:
                w[:] = 0.0
            out.append(_chain(rng, 400, 3, mean=0.1 * rng.standard_normal(3), weights=w))
    elif name == "J":
        out = [_chain(rng, n, 27, mean=0.05 * rng.standard_normal(27)) for n in (1023, 1024, 1025, 2049)]
    elif name == "S2":
        out = [_chain(rng, 50, 3) for _ in range(3)]
        for c in out:
            c[:, 3] = 7.0
    elif name.startswith("S3"):
        out = [_chain(rng, 50, 3) for _ in range(3)]
        if name in ("S3nan", "S3both"):
            out[1][7, 4] = np.nan
        if name == "S3inf":
            out[2][3, 0] = np.inf
        if name == "S3neg":
            out[0][9, 0] = -1.0
        if name == "S3both":                               # a constant column as well: 3 comes before 2
            for c in out:
                c[:, 2] = 1.0
    elif name == "S4":
        out = [_chain(rng, 3, 6) for _ in range(2)]
    else:
        raise KeyError(name)
    for c in out:
        c.setflags(write=False)
    return tuple(out)


# what the status cases give on every route: (status, column)
STATUS_WANT = {"S2": (2, 1), "S3nan": (3, 2), "S3inf": (3, -1), "S3neg": (3, -1), "S3both": (3, 2), "S4": (4, None)}


def segments(chains, by):
    """the segments of ``chains`` as arrays (views), by the rule of chains.conv_segments, restated"""
    if by == "chains":
        return [c for c in chains]
    return [h for c in chains for h in (c[:c.shape[0] // 2], c[c.shape[0] // 2:])]


def model_segments(segs, nd, iw=0, itheta=2):
    """the rule on segments in extended precision -> dict(r_minus_1, per_param, kappa, used, skipped, U, bound_r, bound_per)"""
    use = [s for s in segs if s.shape[0] > 0 and float(np.sum(s[:, iw])) > 0.0]
    M = len(use)
    assert M >= 2
    pivot = use[0][0, itheta:itheta + nd].astype(LD)
    W, mean, cov = [], [], []
    for s in use:
        w = s[:, iw].astype(LD)
        x = s[:, itheta:itheta + nd].astype(LD) - pivot
        Ws = np.sum(w)
        m = (w @ x) / Ws
        y = x - m
        W.append(Ws)
        mean.append(m)
        cov.append(((y * w[:, None]).T @ y) / Ws)
    W, mean = np.array(W), np.array(mean)
    o = (W @ mean) / np.sum(W)
    delta = mean - o
    Wc = np.sum(cov, axis=0) / M
    diag = np.diag(Wc)
    sigma = np.sqrt(diag)
    per = np.sum(delta * delta, axis=0) / (M - 1) / diag
    Wn = Wc / np.outer(sigma, sigma)
    D = delta / sigma
    mp.mp.dps = 50
    to_mp = lambda a: mp.matrix([[mp.mpf(float(v)) + mp.mpf(float(v - LD(float(v)))) for v in row] for row in a])
    L = mp.cholesky(to_mp(Wn))
    Dm = to_mp(D)
    Z = mp.matrix(nd, M)                                       # Z = L^-1 D^T by forward substitution
    for k in range(M):
        for i in range(nd):
            acc = Dm[k, i]
            for j in range(i):
                acc -= L[i, j] * Z[j, k]
            Z[i, k] = acc / L[i, i]
    G = (Z.T * Z if M < nd else Z * Z.T) / (M - 1)
    r = float(max(mp.eigsy(G, eigvals_only=True)))
    lam = np.linalg.eigvalsh(Wn.astype(np.float64))
    kappa = float(lam[-1] / lam[0])
    U = max(s.shape[0] for s in use)
    per = per.astype(np.float64)
    out = dict(r_minus_1=r, per_param=per, kappa=kappa, used=M, skipped=len(segs) - M, U=U,
               bound_r=(4.0 * nd * (U + 1) * EPS + 32.0 * EPS) * kappa * (1.0 + r) + 16.0 * EPS * (1.0 + r) ** 2,
               bound_per=16.0 * U * EPS * (per + np.sqrt(per)))
    assert out["bound_r"] < 1e-3 * r, "the case is not accepted: bound %.3e against R-1 = %.3e" % (out["bound_r"], r)
    return out


@functools.lru_cache(maxsize=None)
def model(name, by):
    chains = parts(name)
    return model_segments(segments(chains, by), chains[0].shape[1] - 2)


def check(got, want, label="", ratios=None):
    """``got``: r_minus_1, per_param, and (optionally) segments / segments_skipped or used, against the model ``want``"""
    err = abs(float(got["r_minus_1"]) - want["r_minus_1"])
    perr = np.abs(np.asarray(got["per_param"], dtype=np.float64) - want["per_param"])
    ratio = err / want["bound_r"], float(np.max(perr / want["bound_per"]))
    if ratios is not None:
        ratios[label] = ratio
    print("conv %-12s R-1 = %.6e  err / bound = %.3e  per_param err / bound = %.3e  kappa = %.3g" % (label, want["r_minus_1"], ratio[0], ratio[1], want["kappa"]))
    assert err <= want["bound_r"], (label, err, want["bound_r"])
    assert np.all(perr <= want["bound_per"]), (label, perr, want["bound_per"])
    if "segments" in got:
        assert (got["segments"], got["segments_skipped"]) == (want["used"], want["skipped"]), label
    if "used" in got:
        assert int(got["used"]) == want["used"], label
