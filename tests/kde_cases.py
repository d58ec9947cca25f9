"""The oracle, the derived bound and the cases of the KDE shift (mcevidence_amd/csrc/kde_shift.hpp, docs/design/shift_kde.md), shared by
tests/test_shift_kde_shared.py (the serial driver and ``shift_kde.measure`` on the CPU) and tests/test_gpu_shift_kde.py (the device).

THE ORACLE takes the fp64 inputs (x, w, linv, mean, point, c) as the exact numbers they are.  The whitened rows are exact: every input
is an integer times a power of two, so z = linv (x - mean) is integer arithmetic (Python integers), and so is |z_i - z_j|^2.  exp and
the sums over j are mpmath's at 60 digits.  It is evaluated on at most 64 QUERY rows per case (the first and the last row, the rows on
either side of every tile, part, 16-row and chunk boundary: 36 rows at n = 1025, so the cap never cuts a boundary of these cases) and at the
point.  For the decision check, which needs every row, ``all_rows`` evaluates the
same formulas in the x87 extended format (64-bit mantissa) and is itself held to the oracle on the query rows within a thousandth of
the bound.

THE BOUND (u = 2^-53, gamma(k) = k u / (1 - k u)); nothing in it is fitted to an output:
  * a whitened coordinate: one subtraction, one product and at most d sums per entry:  |dz_k| <= gamma(d + 2) sum_j |linv_kj| |x_j - m_j|
  * a squared distance in the Gram form |q|^2 + |z|^2 - 2 q.z: gamma(d + 3) (|z_i| + |z_j|)^2 (the direct form of the point's distances
    errs by less), plus what the whitening error propagates: 2 |z_i - z_j| e + e^2 with e = |dz_i| + |dz_j|
  * a term w_j exp(-c D): the argument c D is off by c dD (1 + u) + c D u (its one rounding), which exp turns into the relative factor
    expm1(.); the exp routine's stated error of 1 ulp = 2 u relative; one rounding for the weight; and, where the result is subnormal,
    2^-1074 absolute for exp and for the product each
  * a sum of n positive terms in any order: gamma(n + 2) relative
  * t_i = S_i / (W - w_i): W is such a sum of the weights, then one subtraction and one division; t_0 = S_0 / W; s_0 = sqrt(Q_0) / W.
A row whose exact t_i lies within its bound (plus the threshold's) of an exact threshold is UNDECIDED; a computed mass M(tau) must lie in
the interval got by counting the undecided rows both ways.
"""
import functools
import math

import numpy as np

from mcevidence_amd import shift_kde as sk

U = 2.0 ** -53
EXP_ULPS = 1.0                                         # the stated error of the fp64 exp of the device library, of glibc and of NumPy
TINY = 2.0 ** -1074
TILE, CHUNK, MAX_PARTS = 512, 64, 8                    # seg_tiles.hpp, kde_shift.hpp
SIZES = (2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)
DIMS = (1, 3, 4, 5, 8, 27, 64)


def gamma(k):
    return k * U / (1.0 - k * U)


def nparts(n):
    c = -(-n // CHUNK)
    return max(1, min(c, MAX_PARTS))


def boundaries(n):
    """the first rows of the tiles, the chunks (= the workgroups' query rows), the 16-row groups of a wave and the parts of n rows"""
    c = -(-n // CHUNK)
    b = set(range(0, n, TILE)) | set(range(0, n, CHUNK)) | {16} | {CHUNK * (c * p // nparts(n)) for p in range(nparts(n))}
    return sorted(r for r in b if 0 < r < n)


def queries(n, cap):
    """the first and the last row and the rows on either side of every boundary; at most ``cap``, the tile and part boundaries first"""
    if n == 0:
        return []
    c = -(-n // CHUNK)
    first = [0, n - 1]
    for b in sorted(set(range(0, n, TILE)) | {CHUNK * (c * p // nparts(n)) for p in range(nparts(n))}) + [16] + boundaries(n):
        if 0 < b < n:
            first += [b - 1, b]
    out = []
    for r in first:
        if r not in out:
            out.append(r)
    return out[:cap]


def _ints(a):
    """fp64 array -> (object array of Python integers, e) with a = integers * 2^e exactly"""
    a = np.asarray(a, dtype=np.float64)
    m, ex = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)
    e = ex.astype(np.int64) - 53
    nz = mi != 0
    emin = int(e[nz].min()) if nz.any() else 0
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for k, (v, ek) in enumerate(zip(mi.reshape(-1).tolist(), e.reshape(-1).tolist())):
        flat[k] = (v << (ek - emin)) if v else 0
    return out, emin


class Case(object):
    """one system: x[n, ld] (the first d columns are measured), w, linv, mean, point, c"""

    def __init__(self, name, x, d, w, linv, mean, point, c, cap=64, decide=False):
        self.name, self.d, self.cap, self.decide = name, int(d), cap, decide
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.linv = np.tril(np.asarray(linv, dtype=np.float64)).reshape(d, d)
        self.mean, self.point, self.c = np.asarray(mean, dtype=np.float64), np.asarray(point, dtype=np.float64), float(c)
        self.n = self.w.size
        self.used = np.flatnonzero(self.w != 0.0)

    @property
    def system(self):
        return (self.x, self.d, self.w, self.linv, self.mean, self.point, self.c)

    # ---- the exact model -------------------------------------------------------------------------------------------------------
    @functools.cached_property
    def _exact_z(self):
        """(Z[m, d], Z0[d], scale): the whitened used rows and the point as integers times 2^scale"""
        xu = self.x[self.used][:, :self.d]
        vals, e = _ints(np.concatenate([xu.reshape(-1), self.mean, self.point]))
        m = self.used.size
        X = vals[:m * self.d].reshape(m, self.d)
        M, P = vals[m * self.d:m * self.d + self.d], vals[m * self.d + self.d:]
        L, el = _ints(self.linv)
        return (X - M[None, :]) @ L.T, (P - M) @ L.T, e + el

    @functools.cached_property
    def exact(self):
        """dict(W, S[q], t[q] for the query rows q (indices into the rows), S0, Q0, t0, s0) as mpmath numbers"""
        import mpmath
        mp = mpmath.mp
        mp.dps = 60
        Z, Z0, e = self._exact_z
        wu = [mp.mpf(float(v)) for v in self.w[self.used]]
        W = mp.fsum(wu)
        cm = mp.mpf(self.c)

        def kernels(row):
            diff = Z - row[None, :]
            D = (diff * diff).sum(axis=1)
            return [mp.exp(-mp.ldexp(cm * mp.mpf(int(v)), 2 * e)) for v in D]

        pos = {int(r): k for k, r in enumerate(self.used)}
        out = {"W": W, "S": {}, "t": {}}
        for q in queries(self.n, self.cap):
            if q not in pos:
                continue
            K = kernels(Z[pos[q]])
            S = mp.fsum(wk * Kk for k, (wk, Kk) in enumerate(zip(wu, K)) if k != pos[q])
            out["S"][q], out["t"][q] = S, S / (W - wu[pos[q]])
        K0 = kernels(Z0)
        out["S0"] = mp.fsum(wk * Kk for wk, Kk in zip(wu, K0))
        out["Q0"] = mp.fsum((wk * Kk) ** 2 for wk, Kk in zip(wu, K0))
        out["t0"], out["s0"] = out["S0"] / W, mp.sqrt(out["Q0"]) / W
        return out

    # ---- the bound -------------------------------------------------------------------------------------------------------------
    @functools.cached_property
    def bound(self):
        """dict(S[n], t[n] (NaN for rows that are not used), S0, Q0, t0, s0): the bound of every computed value"""
        d, n = self.d, self.used.size
        a = self.w[self.used]
        with np.errstate(all="ignore"):
            y = self.x[self.used][:, :d] - self.mean[None, :]
            z = y @ self.linv.T
            dz = gamma(d + 2) * (np.abs(y) @ np.abs(self.linv).T)
            y0 = (self.point - self.mean)[None, :]
            z0, dz0 = (y0 @ self.linv.T)[0], gamma(d + 2) * (np.abs(y0) @ np.abs(self.linv).T)[0]
            zn, en = np.sqrt(np.sum(z * z, axis=1)), np.sqrt(np.sum(dz * dz, axis=1))

            def rows(q, qn, qe, leave):
                """(sum of w K rho + floors, S, the largest rho) of the query rows q against every used row"""
                D = np.maximum((qn ** 2)[:, None] + (zn ** 2)[None, :] - 2.0 * (q @ z.T), 0.0)
                e = qe[:, None] + en[None, :]
                dD = gamma(d + 3) * (qn[:, None] + zn[None, :]) ** 2 + 2.0 * np.sqrt(D) * e + e * e
                rho = (1.0 + np.expm1(self.c * dD * (1.0 + U) + self.c * D * U)) * (1.0 + 2.0 * EXP_ULPS * U) * (1.0 + U) - 1.0
                K = np.exp(-self.c * D) * a[None, :]
                if leave is not None:
                    K[np.arange(q.shape[0]), leave] = 0.0
                return K, rho

            K, rho = rows(z, zn, en, np.arange(n))
            S = K.sum(axis=1)
            floor = float(np.sum(a + 1.0)) * TINY
            bS = (K * rho).sum(axis=1) + gamma(n + 2) * (S + (K * rho).sum(axis=1)) + floor
            t = S / (a.sum() - a)
            bt = bS / (a.sum() - a) + t * (gamma(n + 2) * a.sum() / (a.sum() - a) + 3.0 * U) * (1.0 + 1e-6)
            K0, rho0 = rows(z0[None, :], np.sqrt(np.sum(z0 * z0))[None], np.sqrt(np.sum(dz0 * dz0))[None], None)
            S0, Q0 = float(K0.sum()), float((K0 * K0).sum())
            bS0 = float((K0 * rho0).sum()) * (1.0 + gamma(n + 2)) + gamma(n + 2) * S0 + floor
            rq = (1.0 + rho0) ** 2 * (1.0 + U) - 1.0
            bQ0 = float((K0 * K0 * rq).sum()) * (1.0 + gamma(n + 2)) + gamma(n + 2) * Q0 + floor
            W = a.sum()
            bt0 = bS0 / W + S0 / W * (gamma(n + 2) + 2.0 * U) * (1.0 + 1e-6)
            bs0 = (0.5 * bQ0 / math.sqrt(Q0) if Q0 > 0.0 else math.sqrt(bQ0)) / W + math.sqrt(Q0) / W * (gamma(n + 2) + 3.0 * U) * (1.0 + 1e-6)
        full = lambda v: _scatter(v, self.used, self.n)      # noqa: E731
        return {"S": full(bS), "t": full(bt), "S0": bS0, "Q0": bQ0, "t0": bt0, "s0": bs0, "W": gamma(n + 2) * W}

    # ---- every row, in the extended format -------------------------------------------------------------------------------------
    @functools.cached_property
    def all_rows(self):
        """dict(t[n] (NaN where not used), t0, s0, W) in the extended format: what the decision check takes for exact"""
        ld = np.longdouble
        assert np.finfo(ld).nmant >= 63, "the extended format is needed"
        a = self.w[self.used].astype(ld)
        y = self.x[self.used][:, :self.d].astype(ld) - self.mean.astype(ld)[None, :]
        L = self.linv.astype(ld)
        z = y @ L.T
        z0 = (self.point.astype(ld) - self.mean.astype(ld)) @ L.T
        c = ld(self.c)
        n = a.size
        t = np.empty(n, dtype=ld)
        W = a.sum()
        for i in range(n):
            diff = z - z[i][None, :]
            K = np.exp(-c * (diff * diff).sum(axis=1)) * a
            K[i] = 0
            t[i] = K.sum() / (W - a[i])
        K0 = np.exp(-c * ((z - z0[None, :]) ** 2).sum(axis=1)) * a
        return {"t": _scatter(t, self.used, self.n, ld), "t0": K0.sum() / W, "s0": np.sqrt((K0 * K0).sum()) / W, "W": W}

    def decision(self):
        """[(lo, hi)] for M(t0), M(t0 - s0), M(t0 + s0): the masses with the undecided rows counted both ways, and the undecided weight"""
        ex, b = self.all_rows, self.bound
        out, undecided = [], 0.0
        for tau, btau in ((ex["t0"], b["t0"]), (ex["t0"] - ex["s0"], b["t0"] + b["s0"]), (ex["t0"] + ex["s0"], b["t0"] + b["s0"])):
            btau = btau + 2.0 * U * abs(float(tau))
            sure = lo = 0.0
            for i in self.used:
                margin = (b["t"][i] + btau) * 1.001
                if ex["t"][i] - tau > margin:
                    sure += self.w[i]
                elif ex["t"][i] - tau >= -margin:
                    lo += self.w[i]
            out.append((sure, sure + lo))
            undecided = max(undecided, lo)
        return out, undecided


def _scatter(v, used, n, dtype=np.float64):
    out = np.full(n, np.nan, dtype=dtype)
    out[used] = v
    return out


def check(case, got, what, verbose=True):
    """a computed block (``shift_kde.measure`` / ``from_block`` with dens) against the oracle on the query rows and the point, within the
    bound; prints error over bound; returns the largest ratio"""
    import mpmath
    ex, b = case.exact, case.bound
    assert got["status"] == 0 and got["rows"] == case.used.size, (what, case.name, got["status"], got["rows"])
    worst = 0.0

    def one(label, value, exact, bound):
        nonlocal worst
        err = float(abs(mpmath.mpf(float(value)) - exact))
        ratio = err / bound if bound > 0.0 else (0.0 if err == 0.0 else math.inf)
        worst = max(worst, ratio)
        assert err <= bound, "%s %s %s: error %.3e > bound %.3e (value %r)" % (what, case.name, label, err, bound, value)

    one("W", got["W"], ex["W"], b["W"] + U * float(ex["W"]))
    one("S0", got["S0"], ex["S0"], b["S0"])
    one("Q0", got["Q0"], ex["Q0"], b["Q0"])
    one("t0", got["dens"][case.n], ex["t0"], b["t0"])
    for q, t in ex["t"].items():
        one("t[%d]" % q, got["dens"][q], t, b["t"][q])
    unused = np.setdiff1d(np.arange(case.n), case.used)
    assert np.isnan(got["dens"][unused]).all(), (what, case.name)
    if verbose:
        print("%s %-16s n=%d d=%d queries=%d: worst error / bound = %.3g" % (what, case.name, case.n, case.d, len(ex["t"]), worst))
    return worst


def check_all_rows_model(case):
    """the extended-format evaluation against the oracle on the query rows: within a thousandth of the bound"""
    import mpmath
    ex, al, b = case.exact, case.all_rows, case.bound
    for q, t in ex["t"].items():
        assert abs(mpmath.mpf(float(al["t"][q])) - t) <= 1e-3 * b["t"][q] + float(t) * 2.0 * U, (case.name, q)
    assert abs(mpmath.mpf(float(al["t0"])) - ex["t0"]) <= 1e-3 * b["t0"] + float(ex["t0"]) * 2.0 * U, case.name


def check_two(case, one, two, what):
    """ALL densities of two computed forms: each within the bound of the exact value, hence within two bounds of each other"""
    b = case.bound
    u = case.used
    err = np.abs(one["dens"][:case.n][u] - two["dens"][:case.n][u])
    assert np.all(err <= 2.0 * b["t"][u]), (what, case.name, float(np.max(err / b["t"][u])))
    assert abs(one["dens"][case.n] - two["dens"][case.n]) <= 2.0 * b["t0"], (what, case.name)
    return float(np.max(err / (2.0 * b["t"][u]))) if u.size else 0.0


def check_masses(case, got, what):
    """the decision check, without a tolerance: the computed masses lie in the interval of the undecided rows; with integer weights they
    are also the exact selection sums over the computed densities themselves, bit for bit"""
    iv, undecided = case.decision()
    assert undecided <= 1e-3 * float(case.all_rows["W"]), (case.name, undecided)
    for k, (lo, hi) in enumerate(iv):
        assert lo <= got["M"][k] <= hi, (what, case.name, k, lo, got["M"][k], hi)
    a, t = case.w[case.used], got["dens"][:case.n][case.used]
    if np.all(a == np.round(a)) and a.sum() < 2.0 ** 53:
        t0 = got["dens"][case.n]
        s0 = math.sqrt(got["Q0"]) / got["W"]
        want = [a[t > tau].sum() for tau in (t0, t0 - s0, t0 + s0)]
        assert list(got["M"]) == want and got["M_eq"] == a[t == t0].sum(), (what, case.name, list(got["M"]), want)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _cloud(seed, n, d, ld=None, weights="1..4", offset=0.3):
    """rows of a correlated Gaussian cloud with its POPULATION whitening (so that any n >= 1 has one) and Silverman's c for its ess"""
    rng = np.random.default_rng(seed)
    ld = d if ld is None else ld
    A = rng.standard_normal((d, d)) / math.sqrt(d) + np.eye(d)
    Lp = np.linalg.cholesky(A @ A.T)
    mu = offset * rng.standard_normal(d)
    x = np.full((n, ld), 1e300)
    x[:, :d] = rng.standard_normal((n, d)) @ Lp.T + mu[None, :] + 0.4
    w = np.ones(n) if weights == "unit" else rng.integers(1, 5, n).astype(np.float64)
    ess = max(w.sum() ** 2 / np.sum(w * w), 2.0) if n else 2.0
    return x, w, np.linalg.solve(Lp, np.eye(d)), mu + 0.4, np.zeros(d), 1.0 / (2.0 * sk.bandwidth(d, ess))


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    out["A"] = Case("A", *_splice(_cloud(1, 600, 3, weights="unit"), 3), cap=64, decide=True)
    for n in SIZES:
        for d in DIMS:
            out["B_%d_%d" % (n, d)] = Case("B_%d_%d" % (n, d), *_splice(_cloud(1000 * d + n, n, d, ld=d + 2), d), cap=64,
                                           decide=(n, d) in ((17, 3), (129, 5), (513, 4), (65, 27)))
    # C: a fifth of the rows has weight 0 over NaN / inf values
    x, w, linv, mean, point, c = _cloud(3, 700, 4)
    rng = np.random.default_rng(33)
    off = rng.permutation(700)[:140]
    w[off] = 0.0
    x[off] = rng.choice([np.nan, np.inf, -np.inf], size=(140, 4))
    out["C"] = Case("C", x, 4, w, linv, mean, point, c, cap=64, decide=True)
    # D: two clusters 60 whitened units apart and a group whose kernel values towards the first cluster are subnormal (c D near 708 .. 745)
    rng = np.random.default_rng(4)
    c = 3.0
    z = np.concatenate([0.3 * rng.standard_normal((140, 2)), 0.3 * rng.standard_normal((140, 2)) + [60.0, 0.0],
                        0.02 * rng.standard_normal((20, 2)) + [0.0, math.sqrt(727.0 / c)]])
    out["D"] = Case("D", z, 2, rng.integers(1, 5, 300).astype(np.float64), np.eye(2), np.zeros(2), np.array([0.1, -0.2]), c, cap=64, decide=True)
    # E: duplicated rows (distance exactly 0: the Gram form goes slightly negative) and the point on a sample
    x, w, linv, mean, point, c = _cloud(5, 200, 3)
    x[1::2] = x[::2]
    out["E"] = Case("E", x, 3, w, linv, mean, x[6, :3].copy(), c, cap=64, decide=True)
    return out


def groups():
    """the cases in groups that a test serves in a few seconds each: A and C..E, then the B cases of one d"""
    names = list(cases())
    return dict([("ACDE", [n for n in names if not n.startswith("B_")])] + [("B_d%d" % d, [n for n in names if n.startswith("B_") and n.endswith("_%d" % d)]) for d in DIMS])


def _splice(cloud, d):
    x, w, linv, mean, point, c = cloud
    return x, d, w, linv, mean, point, c


def status_cases():
    """[(name, system, status, column)]"""
    x, w, linv, mean, point, c = _cloud(6, 90, 3)
    out = []
    for name, edit, status, column in (("negative weight", lambda x, w: w.__setitem__(7, -1.0), 3, -1), ("nan weight", lambda x, w: w.__setitem__(80, np.nan), 3, -1),
                                       ("inf weight and a bad value", lambda x, w: (w.__setitem__(3, np.inf), x.__setitem__((4, 1), np.nan)), 3, -1),
                                       ("inf value", lambda x, w: (x.__setitem__((70, 2), np.inf), x.__setitem__((12, 1), -np.inf)), 4, 1),
                                       ("nan value", lambda x, w: x.__setitem__((89, 0), np.nan), 4, 0),
                                       ("no weight", lambda x, w: w.__setitem__(slice(None), 0.0), 5, -1),
                                       ("one row", lambda x, w: (w.__setitem__(slice(None), 0.0), w.__setitem__(40, 2.0)), 6, -1)):
        xs, ws = x.copy(), w.copy()
        edit(xs, ws)
        out.append((name, (xs, 3, ws, linv, mean, point, c), status, column))
    # two bad rows of ONE thread of a tile (rows i and i + 256), the higher column in the later row: the lowest column is reported
    x6, w6, linv, mean, point, c = _cloud(7, 600, 3)
    for name, cells, column in (("two rows of a thread, lower column first", ((10, 0), (266, 2)), 0), ("two rows of a thread, lower column last", ((44, 2), (300, 1)), 1),
                                ("two rows of the second tile", ((515, 2), (599, 1)), 1)):
        xs = x6.copy()
        for k, (r, col) in enumerate(cells):
            xs[r, col] = (np.inf, np.nan, -np.inf)[k % 3]
        out.append((name, (xs, 3, w6.copy(), linv, mean, point, c), 4, column))
    out.append(("no rows", (np.zeros((0, 3)), 3, np.zeros(0), linv, mean, point, c), 5, -1))
    return out
