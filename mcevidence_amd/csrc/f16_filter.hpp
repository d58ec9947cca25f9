// f16_filter.hpp -- what the fp16-filter kernel families share (knn_f16.hpp: exhaustive / seeded / wide / pruned / round-2
// symmetric / repair; knn_panel.hpp; knn_deep.hpp; the merge of reduce_kernels.hpp): the gate's bound, the 16-accumulator
// minimum, the sorted-list insertion, the row side's slots, the wave-wide resolution of a candidate tile and chunk staging.
// ONE copy of each: a change to the bound is a change to f16_gate_terms / f16_gate_a.
//
// The bound (derivation: docs/design/sweep_f16_exhaustive.md, "The bound"; the header of knn_f16.hpp).  With
//      a = e_x + max_j e_y + slack            c = eps_q - |x^|^2
// a pair can be among the query's K nearest only if its accumulator is at most
//      G = (s sqrt(thr) + a)^2 + c            rounded up to fp32.
// Every family evaluates it as  rr = sqrt(thr s^2) (1 + 1e-12) + a;  G = ru(rr^2 (1 + 1e-12) + c)  with c = eps - xn formed
// first.  (The exhaustive kernel used to add  (rr^2 (1 + 1e-12) - xn) + eps: the same real number.)  Forming c costs one
// fp64 rounding, at most 2^-53 max(eps, xn); eps carries (1 + 2^-9) on a term >= 2^-19 xn, i.e. >= 2^-28 xn of headroom, and
// rr^2 carries (1 + 1e-12): either exceeds that rounding, and the two of the final sum, by many orders of magnitude.
//
// The arithmetic is __host__ __device__ and plain C++, so tests/native/f16_gate_check.cpp checks it with g++.
//
// The kernels' register peaks sit in this arithmetic (the gate refresh at the end of a drain, the row gate inside
// sym_slot_insert), so its SHAPE is pinned by the resource table of docs/design/filter_common.md: list_insert is handed
// pointers by the exhaustive kernel (arrays: +4 VGPRs in its k-step 3 / 4 forms) and arrays by everybody else, the row gate adds its
// 1e-30 last and reads max |y^| last (added first: +2 VGPRs in every panel kernel), and the exhaustive kernel tests thr and
// the padding itself and calls f16_gate_finite (f16_gate's two selects: +2 VGPRs there), and f16_gate_terms forms a before eps
// (after: one more spilled SGPR in two kernels).  Re-run the table after a change.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "sym_types.hpp"

namespace mce {

#if defined(__HIPCC__)
#define MCE_HDI __host__ __device__ __forceinline__
#else
#define MCE_HDI inline
#endif

// device-side scalars shared by the f16 kernels (doubles; maxima kept as bit patterns)
enum { HP_RMAX = 0, HP_SCALE = 1, HP_EY = 2, HP_YHATMAX = 3, HP_RHO = 4, HP_STAT_CHUNKS = 5, HP_STAT_TILES = 6, HP_COUNT = 16 };   // STAT_*: pruned walk, totals over the launch

constexpr int kHWaves = 8;      // waves per workgroup (two per SIMD)
constexpr int kHThreads = kHWaves * 64;
constexpr int kHRelBits = 26;   // queue entry = query-local (6|7 bits) << kHRelBits | row - first row of the split
constexpr int kHSymRowBits = kHRelBits - 1;            // symmetric sweep: the row field's top bit says "this lane passed the ROW gate"

// ---- the gate ---------------------------------------------------------------------------------------------------------
MCE_HDI float f16_round_up(double g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2float_ru(g);
#else
    float f = (float)g;
    if ((double)f < g) f = nextafterf(f, __builtin_huge_valf());
    return f;
#endif
}
struct F16GateTerms { double a, c, eps; };
// a of a query or row with conversion error ex.  + 2 sqrt(16 KST) 2^-14: even if the matrix unit flushed fp16 subnormal
// inputs (it does not on gfx950) the bound would hold
MCE_HDI double f16_gate_a(double ex, double ey, int KST) { return (ex + ey) * (1.0 + 1e-9) + 2.0 * sqrt(16.0 * KST) * 0x1p-14; }
// a, c and eps of a query from its qinfo pair (ex, xn = |x^|^2) and the launch's HP_EY, HP_YHATMAX, HP_RHO; live = false
// (padding query; an ablation build): c = -inf, the gate never passes
MCE_HDI F16GateTerms f16_gate_terms(double ex, double xn, double ey, double ymax, double rho, int KST, bool live = true)
{
    const double r = sqrt(xn) + ymax;
    const double a = f16_gate_a(ex, ey, KST);          // (r, a, eps in this order: see the note on register peaks above)
    const double eps = (32.0 * KST) * 0x1p-24 * r * r * (1.0 + 0x1p-9) + rho + 1e-30;
    return {a, live ? eps - xn : -__builtin_huge_val(), eps};
}
// (s sqrt(thr) + a)^2, never below its real value; thr: a bound on the K-th squared distance (input units), s2 = scale^2
MCE_HDI double f16_reach2(double thr, double s2, double a)
{
    const double rr = sqrt(thr * s2) * (1.0 + 1e-12) + a;
    return rr * rr * (1.0 + 1e-12);
}
// the column gate of a query: finite thr and c; any (padding query: c = -inf, never passes; no bound yet: always)
MCE_HDI float f16_gate_finite(double thr, double s2, double a, double c) { return f16_round_up(f16_reach2(thr, s2, a) + c); }
MCE_HDI float f16_gate(double thr, double s2, double a, double c)
{
    if (!(c > -__builtin_huge_val())) return -__builtin_huge_valf();
    if (!(thr < __builtin_huge_val())) return __builtin_huge_valf();
    return f16_gate_finite(thr, s2, a, c);
}
// Row side of the symmetric sweep: R_j = (s sqrt(thr_j) + a_j)^2 of row j, tested as  A[i,j] <= R_j + c_i  in fp32; inflated
// by what that fp32 addition can lose (rowc, from the launch's largest |y^|)
MCE_HDI double f16_row_const(double ymax) { return 0x1p-22 * (ymax * ymax + 1.0); }
MCE_HDI float f16_row_round(double g, double rowc) { return f16_round_up(g * (1.0 + 0x1p-22) + rowc + 1e-30); }
MCE_HDI float f16_row_gate(double thr, double s2, double a, double rowc)
{
    if (!(thr < __builtin_huge_val())) return __builtin_huge_valf();
    return f16_row_round(f16_reach2(thr, s2, a), rowc);
}
// ... of a row known by its conversion error alone (params: the HP_* scalars, each read where it is used)
template <class P>
MCE_HDI float f16_row_gate_of(double thr, double ex, P params, int KST)
{
    if (!(thr < __builtin_huge_val())) return __builtin_huge_valf();
    const double s2 = params[HP_SCALE] * params[HP_SCALE];
    const double g = f16_reach2(thr, s2, f16_gate_a(ex, params[HP_EY], KST));
    return f16_row_round(g, f16_row_const(params[HP_YHATMAX]));
}
// The gate read the other way (seed phases, prepass): a row whose accumulator is a_up lies within this squared distance
// (input units) of the query -- true <= sqrt(A + |x^|^2 + eps) + e_x + max e_y.  f16_gate of the result is >= a_up.
MCE_HDI double f16_seed_bound(double a_up, double xn, double eps, double a, double s2)
{
    const double dd = sqrt(fmax(a_up + xn + eps, 0.0)) * (1.0 + 1e-12) + a;
    return dd * dd * (1.0 + 1e-12) / s2 * (1.0 + 1e-12);
}

// ---- sorted top-N list: one candidate (d2, j) through a static compare/select network --------------------------------------
// ascending distance, ties by row; d2 = +inf (idle lane) changes nothing
// (own_d, own_i: arrays, or pointers to their first entries)
template <int N, class D, class I>
MCE_HD inline void list_insert(D&& own_d, I&& own_i, double d2, int j)
{
    const double INF = __builtin_huge_val();
    bool c_hi = (d2 < own_d[N - 1]) || (d2 == own_d[N - 1] && j < own_i[N - 1] && d2 < INF);
#pragma unroll
    for (int k = N - 1; k >= 1; --k) {
        const bool c_lo = (d2 < own_d[k - 1]) || (d2 == own_d[k - 1] && j < own_i[k - 1] && d2 < INF);
        own_d[k] = c_lo ? own_d[k - 1] : (c_hi ? d2 : own_d[k]);
        own_i[k] = c_lo ? own_i[k - 1] : (c_hi ? j : own_i[k]);
        c_hi = c_lo;
    }
    own_d[0] = c_hi ? d2 : own_d[0];
    own_i[0] = c_hi ? j : own_i[0];
}

#if defined(__HIPCC__)
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// v_min3_f32 without the NaN-canonicalising v_max the compiler adds around fminf()
__device__ __forceinline__ float min3f(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// ---- min of the lane's 16 accumulators (8 v_min3_f32); l1: the five first-level minima -- of the accumulators 3i .. 3i + 2 --
// which f16_event looks at first.  With `run`: min(run, the 16), in the same eight instructions.
__device__ __forceinline__ void f16_min16_halves(const v16f& c, float (&l1)[5], float& m0, float& m3)
{
    l1[0] = min3f(c[0], c[1], c[2]);
    l1[1] = min3f(c[3], c[4], c[5]);
    l1[2] = min3f(c[6], c[7], c[8]);
    l1[3] = min3f(c[9], c[10], c[11]);
    l1[4] = min3f(c[12], c[13], c[14]);
    m0 = min3f(l1[0], l1[1], l1[2]);
    m3 = min3f(l1[3], l1[4], c[15]);
}
__device__ __forceinline__ float f16_min16(const v16f& c, float (&l1)[5])
{
    float m0, m3;
    f16_min16_halves(c, l1, m0, m3);
    return min3f(m0, m3, m3);
}
__device__ __forceinline__ float f16_min16(const v16f& c, float (&l1)[5], float run)
{
    float m0, m3;
    f16_min16_halves(c, l1, m0, m3);
    return min3f(run, m0, m3);
}

// ---- row side of the symmetric sweep: one candidate distance d2 for sorted row `row` ---------------------------------------
// Replace the largest of the row's K slots if d2 is smaller (compare-and-swap; lock-free, any number of writers) and publish
// the new K-th as the row's bound thr, its gate constant rrow (row_gate(bound, row)) and the tile's largest, rtile.  Returns
// false if K slots hold strictly smaller distances (the candidate cannot be among the K).  The pointers are SymParams's.
template <int KCAP, class PS, class PT, class PR, class PF, class RG>
__device__ __forceinline__ bool sym_slot_insert(PS slots, PT thr, PR rrow, PF rtile, int ksel, int row, double d2, RG row_gate)
{
    const auto sl = slots + (int64_t)row * KCAP;
    for (;;) {
        double vmax = -1.0, v2 = -1.0;
        int imax = 0;
#pragma unroll
        for (int k = 0; k < KCAP; ++k) {
            if (k < ksel) {
                const double v = __longlong_as_double((long long)__hip_atomic_load(sl + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (v > vmax) { v2 = vmax; vmax = v; imax = k; }
                else if (v > v2) v2 = v;
            }
        }
        if (d2 > vmax) return false;
        if (d2 == vmax) return true;                     // a tie: the merge decides by row number
        unsigned long long expect = (unsigned long long)__double_as_longlong(vmax);
        if (__hip_atomic_compare_exchange_strong(sl + imax, &expect, (unsigned long long)__double_as_longlong(d2), __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            const double nk = fmax(v2, d2);              // the K-th smallest after the replacement, from a snapshot: an upper bound
            if (nk < __builtin_huge_val()) {
                const unsigned long long nb = (unsigned long long)__double_as_longlong(nk);
                const unsigned long long ob = __hip_atomic_fetch_min(thr + row, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (nb < ob) {
                    const unsigned rb = __float_as_uint(row_gate(nk, row));
                    const unsigned orb = __hip_atomic_fetch_min(rrow + row, rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (rb < orb) {
                        // the tile's largest R_j, from a snapshot (each value >= its current one): safe to store
                        const auto rt = rrow + (int64_t)(row >> 5) * 32;
                        unsigned m = 0;
                        for (int k = 0; k < 32; ++k) {
                            const unsigned v = __hip_atomic_load(rt + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            m = v > m ? v : m;
                        }
                        __hip_atomic_store(rtile + (row >> 5), __uint_as_float(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            return true;
        }
    }
}

// ---- a tile with a candidate (panel and deep kernels) ------------------------------------------------------------------------
// c: the 16 accumulators of one query tile (C layout of 32x32 f32: lane l -> query column l & 31, rows (r & 3) + 8 (r >> 2) +
// 4 (l >> 5)); l1: f16_min16's; lanew: query-local << kHRelBits | 4 (lane >> 5); g: the lane's gate; ROWFLAG / rowflag: the
// lane passed the ROW gate (the entry's kHSymRowBits bit); jb0: first reference row of the tile; todo: the accumulators still
// to be looked at (a redo passes what is left).  Wave-wide compares, scalar branches over the empty ones; the lanes under the
// gate append (query, row) to the wave's queue wq / qcount (wave-uniform).  A hit is queued while at most qlimit entries are
// waiting; returns the accumulators NOT handled because the queue was full.
// The gate's own first-level minima say which triples of accumulators hold something: 6 wave-wide compares, then 3 for each
// triple that does (usually one) -- 9 instead of 16.
// (ROWBIT: where the row flag sits -- the panel sweep's four-tile form keeps 7 query-local bits above a 24-bit row field)
template <bool ROWFLAG, int ROWBIT = kHSymRowBits>
__device__ __forceinline__ unsigned f16_event(const v16f& c, const float (&l1)[5], const unsigned lanew, const float g, const bool rowflag, const int jb0,
                                              const unsigned todo, const int qlimit, int* const wq, int& qcount)
{
    const unsigned wbase = (lanew + (unsigned)jb0) | (ROWFLAG && rowflag ? (1u << ROWBIT) : 0u);
    unsigned rem = 0;
#define MCE_HIT(R_, P_, S_)                                                                                               \
    if ((S_) != 0 && (todo & (1u << (R_)))) {                                                                             \
        if (qcount > qlimit) rem |= 1u << (R_);                                                                           \
        else {                                                                                                            \
            if (P_) wq[__builtin_amdgcn_mbcnt_hi((unsigned)((S_) >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)(S_), (unsigned)qcount))] = \
                        (int)(wbase + (unsigned)(((R_) & 3) + 8 * ((R_) >> 2)));                                          \
            qcount += __builtin_popcountll(S_);                                                                           \
        }                                                                                                                 \
    }
#define MCE_TRIPLE(I_, U_)                                                                                                \
    if ((U_) != 0) {                                                                                                      \
        const bool p0 = c[3 * (I_) + 0] <= g, p1 = c[3 * (I_) + 1] <= g, p2 = c[3 * (I_) + 2] <= g;                     \
        const unsigned long long s0 = __ballot(p0), s1 = __ballot(p1), s2 = __ballot(p2);                                \
        MCE_HIT(3 * (I_) + 0, p0, s0)                                                                                     \
        MCE_HIT(3 * (I_) + 1, p1, s1)                                                                                     \
        MCE_HIT(3 * (I_) + 2, p2, s2)                                                                                     \
    }
    const bool q0 = l1[0] <= g, q1 = l1[1] <= g, q2 = l1[2] <= g, q3 = l1[3] <= g, q4 = l1[4] <= g, p15 = c[15] <= g;
    const unsigned long long u0 = __ballot(q0), u1 = __ballot(q1), u2 = __ballot(q2), u3 = __ballot(q3), u4 = __ballot(q4), s15 = __ballot(p15);
    MCE_TRIPLE(0, u0) MCE_TRIPLE(1, u1) MCE_TRIPLE(2, u2) MCE_TRIPLE(3, u3) MCE_TRIPLE(4, u4)
    MCE_HIT(15, p15, s15)
#undef MCE_TRIPLE
#undef MCE_HIT
    return rem;
}

// ---- staging: one chunk (VPT 16-byte vectors per thread) from global memory into an LDS buffer by LDS-DMA, linear image -----
template <int VPT, class P>
__device__ __forceinline__ void f16_stage_chunk(P src, char* dst, int tid, int wave)
{
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int e = tid + i * kHThreads;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(src + (size_t)e * 16),
            (__attribute__((address_space(3))) void*)(dst + (size_t)(wave * 64 + i * kHThreads) * 16),
            16, 0, 0);
    }
}
// A fragments of one 32-row tile: KST 16-byte LDS reads per lane
template <int KST>
__device__ __forceinline__ void f16_load_a(const char* lp, v8h (&a)[KST])
{
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) a[ks] = *reinterpret_cast<const v8h*>(lp + ks * 1024);
}

// (Phase A of the drains -- the exact fp64 evaluation of the queued pairs, 8 lanes per pair -- stays written out in the three
//  kernels: as a shared function it moved their register counts, docs/design/filter_common.md.)
#endif   // __HIPCC__

}  // namespace mce
