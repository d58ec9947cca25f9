// f16_gate_check.cpp -- CPU check of the fp16 filter's bound (mcevidence_amd/csrc/f16_filter.hpp), the arithmetic every
// filter kernel calls.  Over seeded draws of (thr, e_x, |x^|^2, max e_y, max |y^|, rho, scale = a power of two, KST = 1..8):
//   * f16_gate >= (s sqrt(thr) + e_x + e_y)^2 - |x^|^2 + 32 KST 2^-24 (|x^| + max |y^|)^2 + rho, evaluated in long double;
//   * it does not decrease when thr grows; a padding query gives -inf, thr = +inf gives +inf;
//   * f16_gate(f16_seed_bound(A)) >= A: the row behind a seed minimum passes its own gate;
//   * f16_row_gate(thr) + ru(c) >= f16_gate(thr) as real numbers (rows of the reference set: |x^| <= max |y^|).
// Every assertion is an inequality that holds by the derivation: no tolerance.
// Build + run: g++ -std=c++17 -O1 -I mcevidence_amd/csrc tests/native/f16_gate_check.cpp -o /tmp/f16_gate_check && /tmp/f16_gate_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "f16_filter.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next_u64() >> 11) * 0x1p-53; }                                     // [0, 1)
static double logu(double lo, double hi) { return lo * std::exp(uni() * std::log(hi / lo)); }          // log-uniform

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("  (draw %ld)\n", n); return 1; } while (0)

int main()
{
    using namespace mce;
    const double INF = __builtin_huge_val();
    long n = 0, rows = 0;
    for (; n < 400000; ++n) {
        const int KST = 1 + (int)(next_u64() % 8);
        const double s = std::ldexp(1.0, (int)(next_u64() % 41) - 20), s2 = s * s;
        const double ymax = uni() < 0.05 ? 0.0 : 200.0 * uni();
        // |x^|: mostly a row of the reference set (<= max |y^|), sometimes a foreign query
        const double xr = uni() < 0.8 ? ymax * uni() : 200.0 * uni();
        const double xn = uni() < 0.02 ? 0.0 : xr * xr;
        const double ex = uni() < 0.1 ? 0.0 : uni(), ey = uni() < 0.1 ? 0.0 : uni();
        const double rho = uni() < 0.5 ? 0.0 : 0x1p-11 * ymax * ymax * uni();
        // s sqrt(thr): from far below the conversion errors to beyond the diameter of the scaled cloud
        const double u = uni() < 0.02 ? 0.0 : logu(1e-9, 1e3);
        const double thr = (u / s) * (u / s);

        const F16GateTerms t = f16_gate_terms(ex, xn, ey, ymax, rho, KST);
        const float G = f16_gate(thr, s2, t.a, t.c);
        {
            const long double r = sqrtl((long double)xn) + ymax;
            const long double reach = (long double)s * sqrtl((long double)thr) + ex + ey;
            const long double ref = reach * reach - xn + 32.0L * KST * 0x1p-24L * r * r + rho;
            if (!((long double)G >= ref)) FAIL("gate below the bound: %.9g < %.20Lg", (double)G, ref);
        }
        // monotone in thr: the next double up, and a larger step
        for (const double thr2 : {std::nextafter(thr, INF), thr * (1.0 + uni()) + 1e-300}) {
            if (!(f16_gate(thr2, s2, t.a, t.c) >= G)) FAIL("gate decreases from thr = %.17g to %.17g", thr, thr2);
            if (!(f16_row_gate(thr2, s2, t.a, f16_row_const(ymax)) >= f16_row_gate(thr, s2, t.a, f16_row_const(ymax)))) FAIL("row gate decreases at thr = %.17g", thr);
        }
        // padding query; no bound yet
        const F16GateTerms pad = f16_gate_terms(ex, xn, ey, ymax, rho, KST, false);
        if (!(pad.c == -INF && f16_gate(thr, s2, pad.a, pad.c) == -__builtin_huge_valf() && f16_gate(INF, s2, pad.a, pad.c) == -__builtin_huge_valf()))
            FAIL("a padding query passes");
        if (!(f16_gate(INF, s2, t.a, t.c) == __builtin_huge_valf() && f16_row_gate(INF, s2, t.a, f16_row_const(ymax)) == __builtin_huge_valf()))
            FAIL("thr = inf does not open the gate");
        // the seed phases: an accumulator value A (what a row at scaled distance v from the query yields, give or take; or anything
        // below -|x^|^2, which only rounding could produce), turned into a bound and back into a gate
        {
            const double v = logu(1e-6, 1e3);
            const float A = uni() < 0.1 ? (float)(-xn - 100.0 * uni()) : (float)(v * v - xn + (uni() - 0.5) * t.eps);
            const double sb = f16_seed_bound((double)A, xn, t.eps, t.a, s2);
            if (!(f16_gate(sb, s2, t.a, t.c) >= A)) FAIL("seed minimum %.9g fails its own gate %.9g", (double)A, (double)f16_gate(sb, s2, t.a, t.c));
        }
        // the row side, for rows of the reference set: R + c >= G before the fp32 addition
        if (xn <= ymax * ymax) {
            const float R = f16_row_gate(thr, s2, t.a, f16_row_const(ymax)), cf = f16_round_up(t.c);
            if (!((long double)R + (long double)cf >= (long double)G)) FAIL("row gate %.9g + c %.9g below the column gate %.9g", (double)R, (double)cf, (double)G);
            rows += 1;
        }
        // the convenience form reads the same scalars from the parameter block
        {
            double params[HP_COUNT] = {};
            params[HP_SCALE] = s; params[HP_EY] = ey; params[HP_YHATMAX] = ymax; params[HP_RHO] = rho;
            if (f16_row_gate_of(thr, ex, params, KST) != f16_row_gate(thr, s2, t.a, f16_row_const(ymax))) FAIL("f16_row_gate_of differs");
        }
    }
    std::printf("ok %ld draws, %ld with the row side\n", n, rows);
    return 0;
}
