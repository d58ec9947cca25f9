"""Seeded weight vectors and thinning factors for the chain-preparation tests (tests/test_chain_prep_shared.py on the CPU,
tests/test_gpu_resident.py on the device); no test in here.  Every case is (name, weights, thinlen); the expected result is
always ``chains.thin_rows`` / ``chains.max_weight_bin_thin`` on the same weights."""
import numpy as np

LENGTHS = (1, 2, 3, 255, 256, 257, 4097, 70001)
INT_HIGHS = (1, 2, 6, 50)
INT_FACTORS = (1, 2, 3, 5, 6, 10, 49, 50, 51, 1000)          # both branches of the integer rule, factor == max included
BIN_UNITS = (0.5, 1, 2, 3, 4, 7.5, 10, "n", "n+1")
BURNS = (0, 0.3, 0.999, 1, 500, "n", "n+7")


def int_weights(n, hi, seed, lo=0):
    """integer weights drawn from [lo, hi]; the maximum is present whenever there is room for it"""
    rng = np.random.default_rng(seed)
    w = rng.integers(lo, hi + 1, n).astype(np.float64)
    if n > 1:
        w[rng.integers(0, n)] = hi
    return w


def tied_float_weights(n, seed):
    """weights that are not integers, a third of them tied at one of four values"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.05, 9.0, n)
    tied = rng.random(n) < 1.0 / 3.0
    w[tied] = np.asarray([0.25, 1.5, 2.75, 8.125])[rng.integers(0, 4, n)][tied]
    return w


def unit_of(u, n):
    if isinstance(u, str):                                   # "n", "n+1", "n+7"
        return float(n + int(u[2:] or 0))
    return float(u)


def integer_cases(lengths=LENGTHS):
    for n in lengths:
        for hi in INT_HIGHS:
            w = int_weights(n, hi, seed=1000 * hi + n)
            for f in INT_FACTORS:
                yield "int n=%d hi=%d f=%d" % (n, hi, f), w, float(f)
    if 70001 in lengths:                                      # the prefix sum passes 2^32
        w = int_weights(70001, 100000, seed=7, lo=30000)       # (drawn from [30 000, 100 000]: from [0, 100 000] the sum stays at 3.5e9)
        assert w.sum() > 2 ** 32
        for f in (20000, 50000, 99999, 100000, 100001):            # (a small factor would repeat rows millions of times)
            yield "int n=70001 hi=100000 f=%d" % f, w, float(f)


def bin_cases(lengths=LENGTHS, units=BIN_UNITS):
    for n in lengths:
        w = tied_float_weights(n, seed=31 + n)
        for u in units:
            yield "bin n=%d unit=%s" % (n, u), w, unit_of(u, n)
