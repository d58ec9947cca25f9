"""Seeded chains for the thin_corr tests (tests/test_chain_corr_shared.py on the CPU, tests/test_gpu_chain_corr.py on the device) and
the oracle they are held against; no test in here.

A case is AR(1) columns ``y_t = phi y_{t-1} + eps`` (chain c drawn from ``default_rng(100 + c)``), integer weights from
``default_rng(5).integers(lo, hi + 1)``, columns (weight, -ln L, parameters).  The oracle is the rule of docs/design/chain_corr.md
evaluated in ``np.longdouble``.  A numeric case is accepted only if, IN THE ORACLE, every rho_j(t) for t <= cut_j lies at least 1e-6
from min_corr and scale * L lies at least 1e-3 from an integer: then cut and factor are decided far outside fp64's error, and the
tests may ask for them exactly.  A case that does not is rejected by an assert here, never skipped."""
import functools

import numpy as np

MIN_CORR = 0.05
MAX_LAG = 1024
TILE = 256              # csrc/chain_corr_kernels.hpp: kCorrTile (units per tile)
WINDOW = 128            # kCorrWin (lags of the first window)
EPS = float(np.finfo(np.float64).eps)
RHO_MARGIN = 1e-6
FACTOR_MARGIN = 1e-3


def ar1(rows, phi, d, chain):
    rng = np.random.default_rng(100 + chain)
    e = rng.standard_normal((rows, d))
    y = np.empty((rows, d))
    y[0] = e[0]
    for t in range(1, rows):
        y[t] = phi * y[t - 1] + e[t]
    return y


def chain_of(y, w):
    return np.column_stack([w, 0.5 * np.sum(y * y, axis=1), y])


def build(rows, phi, d, lo, hi):
    wrng = np.random.default_rng(5)
    parts = []
    for c, n in enumerate(rows):
        w = wrng.integers(lo, hi + 1, n).astype(np.float64) if hi > lo else np.full(n, float(lo))
        parts.append(chain_of(ar1(n, phi, d, c), w))
    return parts


def _t5():
    p = build((2000,), 0.5, 2, 1, 1)
    p[0][1000, 0] = 300.0                      # one row across several tiles
    return p


def _t5_far():
    p = build((4000,), 0.5, 2, 1, 1)
    p[0][2000, 0] = 1000.0                     # a stretch of 1000 equal units at 2.5: rho falls off over hundreds of lags
    p[0][2000, 2] = 2.5
    return p


def _t6():
    wrng = np.random.default_rng(5)
    return [chain_of(ar1(n, 0.9, 2, c), wrng.uniform(0.1, 9.0, n)) for c, n in enumerate((5000, 777))]


def _t7():
    y = np.cumsum(np.random.default_rng(100).standard_normal((4000, 1)), axis=0)
    return [chain_of(y, np.ones(4000))]


def _t8():
    p = build((1000,), 0.5, 1, 1, 1)
    return [np.column_stack([p[0], np.full(1000, 0.3)])]


def _t9():
    p = build((1000,), 0.5, 1, 1, 1)
    p[0][500, 2] = np.nan
    return p


def _zeros():
    p = build((6000,), 0.9, 2, 1, 1)
    w = np.zeros(6000)
    w[3::8] = np.random.default_rng(5).integers(1, 3, len(w[3::8]))
    p[0][:, 0] = w                             # a strip of 384 units crosses some 2000 rows: beyond the prefix sums kept in LDS
    return p


#: name -> (builder, keywords of the measurement, expected status)
CASES = {
    "T1": (lambda: build((1000,), 0.5, 1, 1, 1), {}, 0),
    "T2": (lambda: build((700, 4099, 65), 0.8, 3, 1, 3), {}, 0),
    "T2b": (lambda: build((700, 4099, 65), 0.8, 3, 0, 3), {}, 0),
    "T3": (lambda: build((6000, 9001), 0.98, 2, 1, 3), {}, 0),
    "T4": (lambda: build((3000, 2500), 0.5, 27, 1, 2), {}, 0),
    "T4_127": (lambda: build((3000, 2500), 0.5, 127, 1, 2), {}, 0),
    "T4_ndim5": (lambda: build((3000, 2500), 0.5, 27, 1, 2), {"ndim": 5}, 0),
    "T5": (_t5, {}, 0),
    "T5_far": (_t5_far, {}, 0),                                         # cuts in the third window: two waits carried over
    "T6": (_t6, {}, 0),
    "T7": (_t7, {"max_lag": 256}, 1),
    "T8": (_t8, {}, 2),
    "T9": (_t9, {}, 3),
    "tile-1": (lambda: build((TILE - 1,), 0.5, 1, 1, 1), {}, 0),
    "tile": (lambda: build((TILE,), 0.5, 1, 1, 1), {}, 0),
    "tile+1": (lambda: build((TILE + 1,), 0.5, 1, 1, 1), {}, 0),
    "short_part": (lambda: build((600, 40), 0.5, 2, 1, 1), {}, 0),      # a part shorter than the first lag window
    "zeros": (_zeros, {}, 0),
}
NUMERIC = [k for k, v in CASES.items() if v[2] == 0]
STATUS = [k for k, v in CASES.items() if v[2] != 0]
SINGLE = ["T1", "T5", "tile-1", "tile", "tile+1", "zeros"]          # one chain each
WINDOW_ENDS = [WINDOW * (2 ** k - 1) for k in range(1, 12)]          # the device sums windows of 128, 256, 512, .. lags: 128, 384, 896, ..
#: which window (0-based) every cut of a case must lie in, and what else a case is there for: asserted by case()
IN_WINDOW = {"T3": 1, "T5_far": 2}


def lags_summed(want):
    """rows of the device's rho table: up to the end of the window that holds the last cut, or the cap"""
    last = int(want["cut"].max())
    return min(next(e for e in WINDOW_ENDS if e > last), want["cap"] + 1)


def series_of(parts, iw=0, itheta=2, ndim=None):
    """(rule, [series of each non-empty part]) as the rule defines them: weight units for integer weights, row units otherwise"""
    parts = [p for p in parts if len(p)]
    w = np.concatenate([p[:, iw] for p in parts])
    frac = float(np.sum(w - np.trunc(w)))
    assert abs(frac - 1e-4) > 1e-6
    rule = 1 if frac <= 1e-4 else 2
    nd = parts[0].shape[1] - itheta if ndim is None else ndim
    out = []
    for p in parts:
        y = p[:, itheta:itheta + nd]
        out.append(np.repeat(y, p[:, iw].astype(np.int64), axis=0) if rule == 1 else y)
    return rule, out


def oracle(parts, iw=0, itheta=2, ndim=None, min_corr=MIN_CORR, max_lag=MAX_LAG, scale=1.0):
    """the rule in np.longdouble: dict(rule, status, column, units, max_units, cap, rho [lags, ndim], cut, per_param, length, factor)"""
    rule, series = series_of(parts, iw, itheta, ndim)
    L = np.longdouble
    nd = series[0].shape[1]
    units = [len(y) for y in series]
    cap = min(max_lag, max(units) // 4)
    out = dict(rule=rule, status=0, column=-1, units=sum(units), max_units=max(units), cap=cap)
    cen = []
    for y in series:
        y = y.astype(L)
        if len(y):
            lo, hi = y.min(axis=0), y.max(axis=0)
            y = y - np.where(lo == hi, lo, y.sum(axis=0) / L(len(y)))
        cen.append(y)

    def lagged(t):
        s = np.zeros(nd, dtype=L)
        for y in cen:
            if len(y) > t:
                s += np.sum(y[:len(y) - t] * y[t:], axis=0)
        return s, L(sum(max(u - t, 0) for u in units))

    with np.errstate(invalid="ignore"):
        s0, n0 = lagged(0)
    bad = np.nonzero(~np.isfinite(s0.astype(np.float64)))[0]
    if len(bad):
        return dict(out, status=3, column=int(bad[0]))
    flat = np.nonzero(~(s0 > 0))[0]
    if len(flat):
        return dict(out, status=2, column=int(flat[0]))
    cut, acc, rows = np.zeros(nd, dtype=np.int64), np.zeros(nd, dtype=L), [np.ones(nd, dtype=L)]
    for t in range(1, cap + 1):
        s, nt = lagged(t)
        rho = (s / nt) / (s0 / n0)
        rows.append(rho)
        found = (cut == 0) & (rho <= min_corr)
        acc += np.where((cut == 0) & ~found, rho, L(0))
        cut[found] = t
        if np.all(cut > 0):
            break
    rho = np.asarray(rows)
    per = 1 + 2 * acc
    out.update(rho=rho, cut=cut, per_param=per)
    missing = np.nonzero(cut == 0)[0]
    if len(missing):
        return dict(out, status=1, column=int(missing[0]))
    length = per.max()
    out.update(length=length, factor=max(1, int(np.ceil(scale * length))))
    # the conditions under which cut and factor may be asked for exactly
    for j in range(nd):
        margin = float(np.min(np.abs(rho[1:cut[j] + 1, j] - min_corr)))
        assert margin >= RHO_MARGIN, "rho of column %d comes within %.2e of min_corr" % (j, margin)
    assert abs(float(scale * length) - round(float(scale * length))) >= FACTOR_MARGIN, "scale * L = %r" % (float(scale * length),)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(parts, keywords, oracle) of a case, built once per process; callers must not write into the arrays"""
    make, kw, status = CASES[name]
    parts = make()
    for p in parts:
        p.setflags(write=False)
    want = oracle(parts, **kw)
    assert want["status"] == status, (name, want["status"])
    if name in IN_WINDOW:
        k = IN_WINDOW[name]
        assert WINDOW_ENDS[k - 1] <= int(want["cut"].min()) and int(want["cut"].max()) < WINDOW_ENDS[k], (name, want["cut"])
    if name == "short_part":
        assert min(len(p) for p in parts) < WINDOW
    if name == "T3":
        assert max(want["max_units"], 0) > 64 * TILE          # more than one tile per chunk
    return parts, dict(kw), want


def tolerances(want):
    """(|rho - oracle|, |L_j - oracle| per column): every term of S_j(t) is bounded in sum by S_j(0) (Cauchy-Schwarz), so a U-term
    fp64 sum in any order, its denominator and the centring each err by at most U eps S_j(0) to first order: 4 U eps on rho,
    8 cut_j U eps on L_j"""
    U = want["units"]
    return 4.0 * U * EPS, 8.0 * want["cut"].astype(np.float64) * U * EPS


def check(name, got, want):
    """a measurement (dict: rule, status, units, cap, cut, per_param, rho) against the oracle: rho and L_j within the derived tolerances;
    cut, units, cap and the factor exactly.  Prints the figures before it asserts."""
    tol_rho, tol_len = tolerances(want)
    assert got["status"] == 0 and got["rule"] == want["rule"], name
    assert got["units"] == want["units"] and got["cap"] == want["cap"], name
    assert np.array_equal(got["cut"], want["cut"]), (name, got["cut"], want["cut"])
    last = int(want["cut"].max())
    assert got["rho"].shape[0] > last, name
    drho = float(np.max(np.abs(got["rho"][:last + 1] - want["rho"][:last + 1].astype(np.float64))))
    dlen = np.abs(got["per_param"] - want["per_param"].astype(np.float64))
    print("%s: units=%d max|drho|=%.2e (tol %.2e) max|dL_j|=%.2e (tol %.2e)" % (name, want["units"], drho, tol_rho, float(dlen.max()), float(tol_len.min())))
    assert drho <= tol_rho, name
    assert np.all(dlen <= tol_len), name
    assert max(1, int(np.ceil(float(np.max(got["per_param"]))))) == want["factor"], name


def write_files(root, parts):
    """root_1.txt .. in CosmoMC layout, every value with 17 significant digits (read back bit for bit)"""
    paths = []
    for i, p in enumerate(parts):
        path = "%s_%d.txt" % (root, i + 1)
        np.savetxt(path, p, fmt="%.17g")
        paths.append(path)
    return paths
