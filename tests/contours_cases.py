"""The oracle, the derived bounds and the cases of ``contours=`` (mcevidence_amd/csrc/param_contours.hpp, docs/design/contours.md),
shared by tests/test_param_contours_shared.py (the serial driver and ``contours.measure`` on the CPU) and
tests/test_gpu_param_contours.py (the device).  The manner is tests/marginals_cases.py's, whose helpers are used where they fit.

THE ORACLE.  W, ess, m and v are summary's exact rational model.  A density is held against the exact product-kernel estimate AT THE
REPORTED h, c, lo and step of the block under test: exp and the sums by mpmath at 60 digits on at most 64 cells of at most three pairs
per case -- always the four corners, the mode and cells on either side of every 16-cell block boundary in both axes, off the diagonal, so
that a transposed or mis-rowed write of a 16 x 16 block fails.  ``dense`` evaluates every cell in the x87 extended format and is itself
held to the mpmath values on the query cells within a hundredth of the bound.

THE BOUNDS (u = 2^-53, gamma(k) = k u / (1 - k u)); nothing in them is fitted to an output:
  * W, ess, m, v: summary's;  h = (s sd) (1 / ess)^(1/6), relative: marginals' with the exponent 1/6 and 1 / ess under the power (one
    division instead of a product and a division: u less)
  * a kernel value E = K(arg): marginals' darg (grid point, subtraction, square and product, the cancellation term included) becomes the
    relative factor expm1(darg), then exp's stated 2 EXP_ULPS u: rel_E = expm1(darg) (1 + q) + q
  * a term (a E_x) E_y: (1 + rel_x)(1 + rel_y)(1 + u)^2 - 1 relative (the weight product's rounding and the MFMA product's), and
    (2 a + 3) 2^-1074 absolute for the subnormal range: each kernel value, the weight product and the final product may round there, the
    other factor being at most a or 1
  * a sum of n non-negative terms in any order: gamma(n + 2) relative -- a k-step of the matrix instruction adds its four products in an
    order that is not stated, and is taken to round each partial sum at least as well as fp64 (docs/design/tension.md)
  * the normalisation ((W h_i) h_j) 2 pi: W's bound, three products, the constant's rounding and the division: (n - 1) 2 u + 6 u, and
    2^-1074 absolute

THE DECISIONS have no tolerance on the block's OWN densities.  Against the oracle a cell is UNDECIDED for p where its exact density lies
within its bound plus the threshold cell's bound of the exact threshold, or where the exact running sum at the cut lies within
4 G^2 u Z of p Z; at most MAX_UNDECIDED cells per (pair, p), the threshold cell always one of them.
"""
import functools

import mpmath
import numpy as np

import marginals_cases as mc
import summary_cases as sc
from mcevidence_amd import contours as ct

U, TINY, LD, EXP_ULPS, POW_ULPS, gamma = mc.U, mc.TINY, mc.LD, mc.EXP_ULPS, mc.POW_ULPS, mc.gamma
TILE, MAX_PARTS = 512, 16
MAX_UNDECIDED = 2
PROBS = (0.68, 0.95)
MP_BUDGET = 60000                                      # rows x cells by mpmath per pair
TWO_PI = LD("6.283185307179586476925286766559005768")

mpmath.mp.dps = 60


def nparts(n):
    return min(MAX_PARTS, -(-n // TILE))


def query_cells(G, n, mode_k):
    """the four corners, the mode, cells on either side of every 16-cell block boundary in both axes (off the diagonal), then cells
    spread over the grid: at most 64, and at most MP_BUDGET rows x cells (the mandatory cells always)"""
    bounds = list(range(16, G, 16))
    must = [(0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1), (int(mode_k) // G, int(mode_k) % G)]
    for i, b in enumerate(bounds):
        b2 = bounds[(i + 1) % len(bounds)] if len(bounds) > 1 else b
        must += [(b - 1, b2), (b, b2 - 1), (b2 - 1, b - 1) if len(bounds) == 1 else (b - 1, b2 - 1)]
    out = []
    rng = np.random.default_rng(G)
    spread = [(int(p), int(q)) for p, q in zip(rng.integers(1, G - 1, 64), rng.integers(1, G - 1, 64))]
    cap = max(len(set(must)), min(64, MP_BUDGET // max(n, 1)))
    for cell in must + spread:
        if cell not in out and len(out) < cap:
            out.append(cell)
    return out


def oracle_cells(a, xs, xt, W_exact, prm_s, prm_t, cells):
    """the exact densities at ``cells`` = [(kx, ky)] (mpmath); prm = (h, c, lo, step)"""
    A = [mpmath.mpf(float(v)) for v in a]

    def axis(x, prm, ks):
        h, c, lo, step = (mpmath.mpf(float(v)) for v in prm)
        X = [mpmath.mpf(float(v)) for v in x]
        return {k: [mpmath.exp(-c * (lo + int(k) * step - xi) ** 2) for xi in X] for k in ks}
    Ex = axis(xs, prm_s, sorted(set(k for k, _ in cells)))
    Ey = axis(xt, prm_t, sorted(set(k for _, k in cells)))
    norm = mpmath.mpf(W_exact) * mpmath.mpf(float(prm_s[0])) * mpmath.mpf(float(prm_t[0])) * 2 * mpmath.pi
    return [mpmath.fsum(ai * ex * ey for ai, ex, ey in zip(A, Ex[kx], Ey[ky])) / norm for kx, ky in cells]


def _axis(x, prm, G, T):
    """E[r][k] and its relative error bound in the type T"""
    h, c, lo, step = (T(v) for v in prm)
    x = np.asarray(x, dtype=T)
    k = np.arange(G, dtype=T)
    g = lo + k * step
    dg = U * np.abs(k * step) + U * np.abs(g)
    e = g[None, :] - x[:, None]
    de = dg[None, :] + U * np.abs(e)
    arg = c * e * e
    darg = c * (2 * np.abs(e) * de + de * de) * (1 + 3 * U) + 3 * U * arg
    q = 2 * EXP_ULPS * U
    D = np.expm1(darg)
    return np.exp(-arg), D * (1 + q) + q


def bound_of(a, xs, xt, W_exact, prm_s, prm_t, G):
    """the bound of every cell, in fp64 (it needs no more than a few digits) -> bound[G, G]"""
    a = np.asarray(a, dtype=np.float64)
    n = a.size
    with np.errstate(all="ignore"):
        Ex, rx = _axis(xs, prm_s, G, np.float64)
        Ey, ry = _axis(xt, prm_t, G, np.float64)
        aE = a[:, None] * Ex
        S = aE.T @ Ey
        B = (aE * rx).T @ Ey + aE.T @ (Ey * ry) + (aE * rx).T @ (Ey * ry) + (2 * U + U * U) * ((aE * (1 + rx)).T @ (Ey * (1 + ry)))
        B = B * (1 + 1e-9) + float(np.sum(2 * a + 3)) * TINY + n * TINY
        B = B + gamma(n + 2) * (S + B)
        norm = float(W_exact) * float(prm_s[0]) * float(prm_t[0]) * float(TWO_PI)
        rho = S / norm
        return B / norm + (rho + B / norm) * ((n - 1) * 2 * U + 6 * U) + 3 * TINY


def dense(a, xs, xt, W_exact, prm_s, prm_t, G):
    """every cell in the extended format -> rho[G, G]"""
    with np.errstate(all="ignore"):
        Ex, _ = _axis(xs, prm_s, G, LD)
        Ey, _ = _axis(xt, prm_t, G, LD)
        S = np.dot((np.asarray(a, dtype=LD)[:, None] * Ex).T, Ey)
        return S / (LD(W_exact) * LD(prm_s[0]) * LD(prm_t[0]) * TWO_PI)


class Case(object):
    """one system: a (weights), x ([n, ld] with d measured columns), the chosen columns, the grid, the scale"""

    def __init__(self, name, a, x, d, cols, grid=64, scale=1.0, probs=PROBS):
        self.name = name
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.a.size, -1)
        self.d, self.cols = int(d), tuple(int(j) for j in cols)
        self.nc = len(self.cols)
        self.grid, self.scale, self.probs = int(grid), float(scale), tuple(probs)
        self.use = self.a != 0.0
        self.n = int(self.use.sum())

    @functools.cached_property
    def exact(self):
        """summary's exact moments of the CHOSEN columns (index t, not j)"""
        return sc.exact(self.a, self.x[:, list(self.cols)], None, [0.5])

    @functools.cached_property
    def bound(self):
        return sc.bounds(self.exact)

    @property
    def spec(self):
        return (self.cols, self.probs, self.grid, self.scale)


def check_moments(case, got, what=""):
    """W, ess, m, v within summary's bounds and h within the bound that follows; -> the chosen columns (t) with status 0"""
    ex, b, n = case.exact, case.bound, case.n
    assert (got["status"], got["column"], got["rows"], got["grid"], got["nc"]) == (0, -1, n, case.grid, case.nc), (case.name, got["status"], got["column"], got["rows"])
    assert np.array_equal(got["col"], np.array(case.cols, dtype=np.float64)), case.name
    good = np.flatnonzero(np.asarray(got["col_status"]) == 0)
    ess = got["W"] * got["W"] / got["A2"]
    r = {"W": abs(got["W"] - ex["W"]) / max(b["W"], 5e-324), "ess": abs(ess - ex["ess"]) / b["ess"], "mean": 0.0, "var": 0.0, "h": 0.0}
    for t in good:
        r["mean"] = max(r["mean"], abs(got["mean"][t] - ex["mean"][t]) / max(b["mean"][t], 5e-324))
        r["var"] = max(r["var"], abs(got["var"][t] - ex["var"][t]) / max(b["var"][t], 5e-324))
        h_exact = case.scale * mpmath.sqrt(mpmath.mpf(ex["var"][t])) * (1 / mpmath.mpf(ex["ess"])) ** (mpmath.mpf(1) / 6)
        # (ex holds the exact values rounded to fp64: one more u each; the exponent 1/6 is itself rounded: |ln t| u / 6 relative)
        lnt = abs(float(mpmath.log(mpmath.mpf(ex["ess"]))))
        rel = 0.5 * (b["var"][t] / ex["var"][t] + U) + U + (b["ess"] / ex["ess"] + U + U) / 6.0 + lnt * U / 6.0 + 2 * POW_ULPS * U + 2 * U + 2 * U
        r["h"] = max(r["h"], float(abs(mpmath.mpf(float(got["h"][t])) - h_exact) / (h_exact * rel)))
        h = got["h"][t]
        lo = ex["min"][t] - 3.0 * h
        assert got["lo"][t] == lo and mc.within_ulps(got["sd"][t], np.sqrt(got["var"][t]), 1) and mc.within_ulps(got["c"][t], 1.0 / ((2.0 * h) * h), 1), (case.name, t)
        assert mc.within_ulps(got["step"][t], ((ex["max"][t] + 3.0 * h) - lo) / float(case.grid - 1), 1), (case.name, t)
    print("%s %-24s n=%-5d nc=%-3d G=%-3d error/bound: W %.3g  ess %.3g  mean %.3g  var %.3g  h %.3g" % (
        what, case.name, n, case.nc, case.grid, r["W"], r["ess"], r["mean"], r["var"], r["h"]))
    assert all(v <= 1.0 for v in r.values()), (case.name, r)
    return good


def _prm(got, t):
    return tuple(float(got[k][t]) for k in ("h", "c", "lo", "step"))


_CACHE = {}


def _cached(kind, case, s, t, got, fn):
    key = (kind, case.name, s, t, _prm(got, s), _prm(got, t))
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def pair_data(case, s, t):
    return case.a[case.use], case.x[case.use, case.cols[s]], case.x[case.use, case.cols[t]]


def bound_cached(case, s, t, got):
    a, xs, xt = pair_data(case, s, t)
    return _cached("bound", case, s, t, got, lambda: bound_of(a, xs, xt, case.exact["W"], _prm(got, s), _prm(got, t), case.grid))


def assert_decisions(got, p, s, t, probs, who=""):
    """the block's decisions of pair p are the serial rule's on the block's own densities, bit for bit (``contours.decide``)"""
    mx, my, md, per = ct.decide(got["density"][p], got["lo"][s], got["step"][s], got["lo"][t], got["step"][t], probs)
    assert (got["mode_x"][p], got["mode_y"][p], got["mode_density"][p]) == (mx, my, md) and md == np.max(got["density"][p]), (who, p, "mode")
    for i, k in enumerate(ct.P_KEYS):
        assert np.array_equal(np.asarray(got[k])[:, p], per[:, i]), (who, p, k, np.asarray(got[k])[:, p], per[:, i])


def check_pair(case, got, p, s, t, what="", stats=None):
    """pair p of a block: every density against ``dense`` within the bound (the query cells against mpmath), the decisions redone bit
    for bit on the block's own densities, and the selection against the oracle on every decided cell"""
    a, xs, xt = pair_data(case, s, t)
    G = case.grid
    bound = bound_cached(case, s, t, got).astype(LD)
    rho = _cached("dense", case, s, t, got, lambda: dense(a, xs, xt, case.exact["W"], _prm(got, s), _prm(got, t), G))
    dev = np.asarray(got["density"][p], dtype=np.float64)
    worst = float(np.max(np.abs(dev.astype(LD) - rho) / bound))
    cells = query_cells(G, a.size, int(np.argmax(dev)))
    W = sc.Fraction(case.exact["W"])
    exact = _cached("mp", case, s, t, got, lambda: oracle_cells(a, xs, xt, mpmath.mpf(W.numerator) / W.denominator, _prm(got, s), _prm(got, t), cells))
    worst_mp = worst_ld = 0.0
    for (kx, ky), ex in zip(cells, exact):
        bk = mc._mp(bound[kx, ky])
        worst_ld = max(worst_ld, float(abs(mc._mp(rho[kx, ky]) - ex) / (bk / 100)))
        worst_mp = max(worst_mp, float(abs(mpmath.mpf(float(dev[kx, ky])) - ex) / bk))
    assert_decisions(got, p, s, t, case.probs, (case.name, what))
    undecided = decisions(rho.reshape(-1), bound.reshape(-1), case.probs, dev, (case.name, p))
    assert decisions(rho.reshape(-1), bound.reshape(-1), case.probs, rho.astype(np.float64), (case.name, p, "oracle")) == undecided
    if stats is not None:
        stats["density"] = max(stats.get("density", 0.0), worst, worst_mp)
        stats["undecided"] = max(stats.get("undecided", 0), max(undecided))
    print("%s %-24s pair %-3d (%d, %d) error/bound: all %.3g  mpmath %.3g on %d cells  (extended format / mpmath: %.3g of a hundredth)  undecided %s" % (
        what, case.name, p, case.cols[s], case.cols[t], worst, worst_mp, len(cells), worst_ld, undecided))
    assert worst <= 1.0 and worst_mp <= 1.0 and worst_ld <= 1.0, (case.name, p, worst, worst_mp, worst_ld)
    assert max(undecided) <= MAX_UNDECIDED, (case.name, p, undecided)


def decisions(rho, bound, probs, dens, who=""):
    """the selection of the densities ``dens`` against the exact densities ``rho`` (flat, extended): asserts agreement on every decided
    cell; -> the undecided cells per p"""
    N = rho.size
    G = int(round(N ** 0.5))
    order = np.lexsort((np.arange(N), -rho))
    cum = np.cumsum(rho[order])
    Z = cum[-1]
    got_order, got_cuts = ct.selection(dens, probs)
    out = []
    for p, gcut in zip(probs, got_cuts):
        target = LD(p) * Z
        cut = min(int(np.searchsorted(cum, target, side="left")), N - 1)
        kc = order[cut]
        und = np.abs(rho - rho[kc]) <= bound + bound[kc]
        near = 4 * G * G * U * Z
        if abs(cum[cut] - target) <= near or (cut > 0 and abs(cum[cut - 1] - target) <= near):
            und[order[max(cut - 1, 0):cut + 2]] = True
        want = np.zeros(N, dtype=bool)
        want[order[:cut + 1]] = True
        sel = np.zeros(N, dtype=bool)
        sel[got_order[:gcut + 1]] = True
        wrong = np.flatnonzero(~und & (want != sel))
        assert wrong.size == 0, (who, p, wrong[:8], "decided cells selected differently")
        assert und[kc]
        out.append(int(und.sum()))
    return out


def check_against_numpy(case, got, what=""):
    """ALL densities of a block against the NumPy form's at the block's reported h, c, lo and step: within two bounds; all decisions bit
    for bit on the block's own densities; -> the largest ratio"""
    host = ct.measure(case.a, case.x[:, :case.d], case.cols, case.probs, case.grid, case.scale, at=got)
    assert np.array_equal(host["col_status"], got["col_status"]) and np.array_equal(host["pair_status"], got["pair_status"]), case.name
    worst = 0.0
    for p, (s, t) in enumerate(ct.pairs(case.nc)):
        if got["pair_status"][p] != 0:
            assert_failed_pair(got, p, case.name)
            continue
        b = bound_cached(case, s, t, got)
        ratio = float(np.max(np.abs(np.asarray(got["density"][p]) - host["density"][p]) / (2 * b)))
        assert ratio <= 1.0, (case.name, p, ratio)
        worst = max(worst, ratio)
        assert_decisions(got, p, s, t, case.probs, (case.name, what))
    print("%s %-24s every density against the NumPy form's at the reported parameters: %.3g of the two bounds" % (what, case.name, worst))
    return worst


def assert_failed_pair(got, p, who=""):
    assert got["pair_status"][p] == 7 and np.all(np.asarray(got["cells"])[:, p] == -1.0), (who, p)
    for k in ("mode_x", "mode_y", "mode_density"):
        assert np.isnan(got[k][p]), (who, p, k)
    for k in ("level", "lower_x", "upper_x", "lower_y", "upper_y", "edge"):
        assert np.isnan(np.asarray(got[k])[:, p]).all(), (who, p, k)
    assert np.isnan(got["density"][p]).all(), (who, p)


def assert_failed_system(got, status, column, rows, who=""):
    assert (got["status"], got["column"], got["rows"]) == (status, column, rows), (who, got["status"], got["column"], got["rows"])
    for k in ("W", "A2") + ct.COL_KEYS[1:] + ct.PAIR_KEYS + ct.P_KEYS + ("density",):
        assert np.isnan(got[k]).all(), (who, k)


def equal_blocks(a, b):
    """bit for bit, NaN equal to NaN"""
    return all(np.array_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), equal_nan=True) for k in a)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def column(rng, n, j):
    """column j's OWN asymmetric shape: gamma-like with its own shape parameter, scale and shift, integers / 64; no two columns are
    alike or mirror images, so no cell ties with its transpose"""
    return np.round((rng.gamma(1.5 + 0.75 * (j % 11), 1.0, n) * (0.5 + 0.25 * (j % 7)) + float(j % 5) - 2.0) * 64.0) / 64.0


def narrow(rng, n):
    """50 +- 2^-20: fails unless g - x is bounded honestly"""
    return 50.0 + rng.choice([-1.0, 0.0, 0.0, 1.0, 1.0, 1.0], n) * 2.0 ** -20


def weights(rng, n, kind):
    if n == 2:                                         # (two rows of one weight are mirror images)
        return np.array([3.0, 1.0]) / (1.0 if kind != "fractional" else 16.0), np.zeros(0, dtype=int)
    if kind == "unit":
        return np.ones(n), np.zeros(0, dtype=int)
    if kind == "integer":
        return rng.integers(1, 5, n).astype(np.float64), np.zeros(0, dtype=int)
    a = rng.integers(1, 64, n) / 16.0
    zero = np.arange(1, n, 5) if n > 3 else np.zeros(0, dtype=int)
    a[zero] = 0.0
    return a, zero


def make(name, n, d, cols, grid, kind, seed, with_narrow=False, scale=1.0):
    rng = np.random.default_rng(seed)
    a, zero = weights(rng, n, kind)
    x = np.stack([column(rng, n, j) for j in range(d + 2)], axis=1)
    if with_narrow:
        x[:, cols[1]] = narrow(rng, n)
    if zero.size:
        x[zero] = np.tile([np.nan, np.inf, -np.inf], -(-x.shape[1] // 3))[:x.shape[1]]
    return Case(name, a, x, d, cols, grid=grid, scale=scale)


# (n, nc, G, weights): the k-step tail (2 .. 5), the chunk (15 .. 17), the tile (511 .. 513), three parts (1025), 17 tiles: the part
# cap and uneven parts (8193, 8705); nc = 6: a full group and a one-column group; ld = d + 2
PLAN = [(2, 2, 32, "integer"), (3, 3, 64, "fractional"), (4, 2, 64, "unit"), (5, 3, 32, "integer"), (15, 6, 64, "fractional"), (16, 2, 32, "unit"),
        (17, 3, 64, "integer"), (511, 6, 32, "unit"), (512, 3, 64, "fractional"), (513, 27, 64, "integer"), (1025, 6, 64, "fractional"),
        (8193, 2, 64, "unit"), (8705, 3, 32, "fractional")]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for i, (n, nc, G, kind) in enumerate(PLAN):
        name = "n%d_nc%d_G%d_%s" % (n, nc, G, kind)
        out[name] = make(name, n, nc, tuple(range(nc)), G, kind, 300 + i, with_narrow=nc == 6 and n >= 500)
    out["n513_d127_last_two"] = make("n513_d127_last_two", 513, 127, (125, 126), 64, "fractional", 400)
    out["scale_half"] = make("scale_half", 1025, 3, (0, 2), 32, "unit", 401, scale=0.5)
    return out


def oracle_pairs(case):
    """the pairs the oracle is asked about: at most three -- the first, the last and one in the middle (with the narrow column where
    there is one); ``check_against_numpy`` covers every pair"""
    P = case.nc * (case.nc - 1) // 2
    allp = ct.pairs(case.nc)
    return [(p, allp[p][0], allp[p][1]) for p in sorted(set([0, P // 2, P - 1]))]


def constant_column_case():
    """a system whose chosen column 1 is constant: col_status 7 there, pair_status 7 in its pairs, the pair (0, 2) untouched"""
    c = make("constant_column", 65, 3, (0, 1, 2), 32, "integer", 402)
    c.x[:, 1] = 2.5
    return c


def status_cases():
    """marginals' refusals on two columns"""
    return mc.status_cases()


# ---- the native program (tests/native/param_contours_check.cpp), a stand-alone sanitized build ------------------------------------
def build_checker(directory):
    import os
    import subprocess
    from helpers import REPO
    exe = os.path.join(str(directory), "param_contours_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "mcevidence_amd", "csrc"),
                           os.path.join(REPO, "tests", "native", "param_contours_check.cpp"), "-o", exe])
    return exe


def _run(exe, mode, fin, fout, count):
    import subprocess
    out = subprocess.run([exe, mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok records=%d" % count), out.stdout[-2000:] + out.stderr[-2000:]
    return np.frombuffer(open(fout, "rb").read(), dtype="<f8")


def run_native(exe, tmp_path, systems, cols, probs, grid, scale):
    """[(a, x[n, ld], d)] through the serial driver -> one block dict per system"""
    import struct
    fin, fout = tmp_path / "con_in.bin", tmp_path / "con_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<qdq", grid, scale, len(cols)) + np.asarray(cols, dtype="<i8").tobytes())
        for a, x, d in systems:
            x = np.ascontiguousarray(x, dtype="<f8")
            x = x if x.ndim == 2 else x.reshape(len(a), -1)
            fh.write(struct.pack("<qqq", len(a), d, x.shape[1]) + x.tobytes() + np.ascontiguousarray(a, dtype="<f8").tobytes())
    raw = _run(exe, "contours", fin, fout, len(systems))
    nc = len(cols)
    size = ct.HEAD + ct.PER_COL * nc + (nc * (nc - 1) // 2) * (ct.PER_PAIR + ct.PER_P * probs.size + grid * grid)
    assert raw.size == size * len(systems)
    return [ct.from_block(raw[i * size:(i + 1) * size], nc, probs.size, grid) for i in range(len(systems))]


def check_decisions_native(exe, tmp_path, blocks, probs, grid):
    """the serial rule (steps 5 and 6) applied to each block's OWN density arrays equals the block's decisions bit for bit"""
    import struct
    fin, fout = tmp_path / "dec_in.bin", tmp_path / "dec_out.bin"
    probs = np.ascontiguousarray(probs, dtype="<f8")
    recs = [(b, p, s, t) for b in blocks if b["status"] == 0 for p, (s, t) in enumerate(ct.pairs(b["nc"])) if b["pair_status"][p] == 0]
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<q", probs.size) + probs.tobytes() + struct.pack("<q", grid))
        for b, p, s, t in recs:
            fh.write(struct.pack("<dddd", b["lo"][s], b["step"][s], b["lo"][t], b["step"][t]) + np.ascontiguousarray(b["density"][p], dtype="<f8").tobytes())
    raw = _run(exe, "decide", fin, fout, len(recs)).reshape(len(recs), 3 + ct.PER_P * probs.size)
    for (b, p, s, t), rec in zip(recs, raw):
        got = [b["mode_x"][p], b["mode_y"][p], b["mode_density"][p]] + [b[k][q][p] for q in range(probs.size) for k in ct.P_KEYS]
        assert np.array_equal(np.array(got), rec), (p, got, rec)
    return len(recs)
