// knn_deep.hpp -- the fp16-MFMA filter + exact fp64 refine of knn_f16.hpp (same bound, same lists, same results: reference
// MCEvidence.py:1093-1104, which puts no limit on ndim; :1405 `--allparams` hands it every derived column) for 64 <= d <= 127:
// FIVE to EIGHT sixteen-wide k-steps per 32-row tile (round 6; VERDICT round 5, missing #4 -- d = 64 fell to the fp64 sweep,
// 31.5 ms against 2.4 ms at d = 63 for 100 k x 100 k).
//
// Why a kernel of its own.  knn_f16_kernel<4, 12> holds 245 VGPRs: B fragments for more k-steps do not fit its body, and its
// software pipeline (two accumulator sets, two A-fragment sets) is what a ONE-to-four-k-step tile needs to keep the matrix pipe
// fed.  A deep tile is 2 KST MFMAs = 320..512 cycles of matrix pipe on its own: here a wave keeps ONE accumulator set, reads
// its A fragments k-step by k-step as the MFMAs go (the compiler hoists the LDS reads as registers allow), gates the tile when
// its chain is done, and the SIMD's other wave fills the pipe meanwhile.  Budget at KST = 8, K <= 12: 64 (B) + 32 (acc) +
// ~24 (A in flight) + 36 (lists) + constants.  The candidate path -- wave-uniform resolution of a tile that passed the gate,
// per-wave LDS queue, redo list, ONE collective drain per chunk with exact fp64 evaluation (8 lanes per pair, 16 elements
// each) and the register lists' insertion network -- is knn_panel.hpp's, column side only; what the two share with the
// exhaustive kernel, the bound first of all, is written once in f16_filter.hpp.
//
// Cold start.  A block meets its references with empty lists; with no bound every pair of the first chunks would be a
// candidate (tens of thousands of exact evaluations per wave).  So every (block, reference split) first SEEDS its bounds
// from the matrix products alone: the first G = K (+ 1 with self-exclusion) groups of `tg` tiles are multiplied once with
// no gate, every lane keeps the minimum of its accumulators per group, and G group minima are G distinct rows (one may be
// the own row) -- so the K-th neighbour lies within
//      max over the groups of   ( sqrt(A_min + |x^|^2 + eps_q) + e_x + max e_y )^2 / s^2 ,
// the triangle inequality read the other way (A_min + |x^|^2 bounds |x^ - y^|^2 from above up to eps_q).  The sweep proper
// then starts from tile 0 with that bound.  Cost: the seed tiles are multiplied twice (about a quarter of a small split, 24 k
// rows of a large one).
#pragma once
#include "knn_panel.hpp"

namespace mce {

struct DeepArgs {
    const _Float16* Yh;          // packed fp16 references (f16_pack_refs_kernel, KST k-steps)
    const _Float16* Xh;          // fp16 query rows [nq_pad][16 KST]
    const double* qinfo;         // [nq_pad][2]: e_x, |x^|^2
    const double* params;        // HP_* scalars
    const double* X;             // fp64 query rows [nq, D] (exact refine)
    const double* Y;             // fp64 reference rows [nr, D]
    double* part_d;              // lists [rsplit][KCAP][nq_pad], exact squared distances
    int* part_i;
    int64_t nq, nr, nq_pad, self_offset;
    int64_t nchunk_total;        // chunks of deep_chunk_tiles(KST) tiles
    int D, ksel, self_exclude, nqblk, rsplit;
    int seed_tg;                 // tiles per seed group (0: no seed phase -- a split too small for K + 1 groups)
    int debug;                   // test hooks: 8 every candidate through the redo list
    int seed_groups = 0;         // groups of the seed phase (0: ksel + self_exclude); the SECOND pass of a search for 16 < K <= 32 neighbours
                                 // bounds the K-th distance overall, not the (K - 16)-th: K + self_exclude groups
    const double* lo_d = nullptr;   // LOWER instantiation (second pass): the first pass's lists [rsplit][KCAP][nq_pad] -- only what lies beyond a
    const int* lo_i = nullptr;      // split's 16th neighbour (lexicographically in (distance, row)) enters this pass's lists
};

__host__ __device__ constexpr int deep_chunk_tiles(int KST) { return KST == 5 ? 8 : (KST == 6 ? 8 : 6); }     // 40 / 48 / 48 KB per buffer
constexpr int kDeepQueue = 448;
__host__ __device__ constexpr size_t deep_lds_bytes(int KST)
{
    return (size_t)2 * deep_chunk_tiles(KST) * KST * 1024           // staging
           + (size_t)kHWaves * kDeepQueue * 16                        // queues: d2 (8) + packed (4) + next (4)
           + (size_t)kHWaves * kHQT * 32 * 4 + 128                     // chain heads + votes
           + (size_t)kHWaves * kHQT * 32 * 4                           // K-th bound per query as of the last drain (float, rounded up)
           + (size_t)kHWaves * deep_chunk_tiles(KST) * kHQT * 4;       // redo list
}
// (K <= 16: one pass; 17..32: two sweeps of 16-entry lists -- each split's 16 nearest, then the next K - 16 beyond them -- as the
//  exhaustive sweep does it, knn_f16.hpp LOWER)
__host__ __device__ constexpr bool deep_supported(int D, int K) { return D >= 64 && D <= 127 && K >= 1 && K <= 32; }
__host__ __device__ constexpr int deep_ksteps(int D) { return (D + 1 + 15) / 16 == 7 ? 8 : (D + 1 + 15) / 16; }     // 5, 6, 8 (seven would not tile the staging buffer)

template <int KST, int KCAP, bool LOWER = false>
__global__ __launch_bounds__(kHThreads, 2) void knn_deep_kernel(DeepArgs a)
{
    static_assert(!LOWER || KCAP == 16, "second pass: 16-entry lists");
    static_assert(kHQT == 2 && (KST == 5 || KST == 6 || KST == 8), "8 waves x 2 query tiles; 5, 6 or 8 k-steps");
    constexpr int QT = 2;
    constexpr int QPW = 64;
    constexpr int QPB = kHWaves * QPW;
    constexpr int CT = deep_chunk_tiles(KST);
    constexpr int CHUNK_BYTES = CT * KST * 1024;
    constexpr int VPT = CHUNK_BYTES / 16 / kHThreads;
    static_assert(CHUNK_BYTES % (16 * kHThreads) == 0 && CT % 2 == 0, "chunk geometry");
    constexpr int QN = kDeepQueue;

    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    char* const stage0 = lds_raw;
    double* const qd2_all = reinterpret_cast<double*>(lds_raw + 2 * CHUNK_BYTES);
    int* const qpk_all = reinterpret_cast<int*>(qd2_all + kHWaves * QN);
    int* const qnx_all = qpk_all + kHWaves * QN;
    int* const head_all = qnx_all + kHWaves * QN;
    volatile int* const wvote = head_all + kHWaves * QPW;                 // [3] drain votes (chunk index mod 3)
    float* const sthr_all = reinterpret_cast<float*>(head_all + kHWaves * QPW + 32);
    int* const redo_all = reinterpret_cast<int*>(sthr_all + kHWaves * QPW);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* const wqd = qd2_all + wave * QN;
    int* const wq = qpk_all + wave * QN;
    int* const wnx = qnx_all + wave * QN;
    int* const whead = head_all + wave * QPW;
    float* const sthr = sthr_all + wave * QPW;
    int* const wredo = redo_all + wave * (CT * QT);
    const double INF = __builtin_huge_val();

    // ---- which (query block, reference split): the split's chunks [c_lo, c_hi), balanced to within one chunk ------------
    const int qblk = (int)(blockIdx.x % (unsigned)a.nqblk);
    const int split = (int)(blockIdx.x / (unsigned)a.nqblk);
    const int64_t c_lo = a.nchunk_total * split / a.rsplit, c_hi = a.nchunk_total * (split + 1) / a.rsplit;
    const int ntot = (int)(c_hi - c_lo);
    const int64_t qwave0 = (int64_t)qblk * QPB + wave * QPW;

    whead[lane] = -1;
    if (tid < 3) wvote[tid] = 0;

    // lane l OWNS wave-local query l: its sorted top-KCAP list lives here
    double own_d[KCAP];
    int own_i[KCAP];
#pragma unroll
    for (int k = 0; k < KCAP; ++k) { own_d[k] = INF; own_i[k] = -1; }
    // second pass: the owned query's 16th neighbour of the first pass in this split (list not full: +inf, nothing is left)
    double lo_own_d = -1.0;
    int lo_own_i = -1;
    if constexpr (LOWER) {
        const int64_t o = ((int64_t)split * KCAP + (KCAP - 1)) * a.nq_pad + qwave0 + lane;
        lo_own_d = gptr(a.lo_d)[o];
        lo_own_i = gptr(a.lo_i)[o];
    }

    // ---- B fragments (fp16 query rows) + per-query gate constants -----------------------------------------------------
    v8h b[QT][KST];
    float G[QT];
    unsigned lanew[QT];
    const int k_last = a.ksel - 1;
    {
        const auto Xh = gptr(a.Xh);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int64_t q = qwave0 + qt * 32 + (lane & 31);
#pragma unroll
            for (int ks = 0; ks < KST; ++ks)
                b[qt][ks] = *(const __attribute__((address_space(1))) v8h*)(Xh + q * (int64_t)(16 * KST) + 16 * ks + 8 * (lane >> 5));
            lanew[qt] = ((unsigned)(qt * 32 + (lane & 31)) << kHRelBits) | (unsigned)(4 * (lane >> 5));
            G[qt] = -__builtin_huge_valf();
        }
    }
    // gate of query (qt, lane & 31): gq_a = e_x + max e_y (+ slack), gq_c = eps_q - |x^|^2 (-inf: padding query); see f16_filter.hpp
    double gq_a[QT], gq_c[QT], gq_xn[QT], gq_eps[QT], s2c;
    {
        const auto params = gptr(a.params);
        const auto qinfo = gptr(a.qinfo);
        const double p_scale = params[HP_SCALE], p_ey = params[HP_EY], p_ym = params[HP_YHATMAX], p_rho = params[HP_RHO];
        s2c = p_scale * p_scale;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const int64_t q = qwave0 + qt * 32 + (lane & 31);
            gq_a[qt] = 0.0;
            gq_c[qt] = -INF;
            gq_xn[qt] = 0.0;
            gq_eps[qt] = 0.0;
            if (q < a.nq) {
                const double xn = qinfo[2 * q + 1];
                const F16GateTerms t = f16_gate_terms(qinfo[2 * q], xn, p_ey, p_ym, p_rho, KST);
                gq_a[qt] = t.a;
                gq_c[qt] = t.c;
                gq_xn[qt] = xn;
                gq_eps[qt] = t.eps;
            }
        }
    }
    auto gate_of = [&](double thr, int qt) __attribute__((always_inline)) -> float { return f16_gate(thr, s2c, gq_a[qt], gq_c[qt]); };

    const int qlimit_gate = (a.debug & 8) ? -1 : QN - 64;
    int qcount = 0;
    int nredo = 0;
    double seed_thr = INF;       // the seed phase's bound on the owned query's K-th squared distance (input units)

    // ---- the drain: exact distances (phase A), list insertion (phase B), new gates -------------------------------------
    auto drain = [&]() __attribute__((always_inline)) {
        const auto X = gptr(a.X);
        const auto Y = gptr(a.Y);
        const int D = a.D;
        const int64_t nq = a.nq, nr = a.nr;
        {
            // phase A: 8 lanes share one queued pair and read the two rows in 64-byte segments (16 elements per lane: d <= 127);
            // the loads of the trip's 8 pairs are all issued before the first use
            const int sub = lane & 7;
            constexpr int EPL = 16;
            for (int b0 = 0; b0 < qcount; b0 += 8) {
                const int e = b0 + (lane >> 3);
                int ql = 0, j = 0;
                const bool valid = e < qcount;
                if (valid) {
                    const unsigned ent = (unsigned)wq[e];
                    ql = (int)(ent >> kHRelBits);
                    j = (int)(ent & ((1u << kHRelBits) - 1u));
                }
                const int64_t q = qwave0 + ql;
                const bool ok = valid && j < nr && q < nq && !(a.self_exclude && (int64_t)j == a.self_offset + q);
                const auto xp = X + (ok ? q : 0) * (int64_t)D;
                const auto yp = Y + (ok ? (int64_t)j : 0) * D;
                double xv[EPL], yv[EPL];
#pragma unroll
                for (int v = 0; v < EPL; ++v) {
                    const int iv = (sub + 8 * v < D) ? sub + 8 * v : sub;      // clamped INSIDE the row (d >= 64 > sub), masked use
                    xv[v] = xp[iv];
                    yv[v] = yp[iv];
                }
                double a0 = 0.0;
#pragma unroll
                for (int v = 0; v < EPL; ++v) {
                    const double t = (sub + 8 * v < D) ? xv[v] - yv[v] : 0.0;
                    a0 = fma(t, t, a0);
                }
                a0 += __shfl_xor(a0, 1, 64);
                a0 += __shfl_xor(a0, 2, 64);
                a0 += __shfl_xor(a0, 4, 64);
                if (sub == 0 && valid) {
                    wqd[e] = ok ? a0 : -1.0;
                    wq[e] = j;
                    // only what can still enter the query's list (K-th bound of the last drain) joins its chain
                    if (ok && !(a0 > (double)sthr[ql])) wnx[e] = atomicExch(&whead[ql], e);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // ---- phase B: every owner lane folds its chain into its register list ----------
        {
            int cur = whead[lane];
            whead[lane] = -1;
            while (__any(cur >= 0)) {
                const bool on = cur >= 0;
                const int ce = on ? cur : 0;
                double d2 = on ? wqd[ce] : INF;
                const int j = wq[ce];
                cur = on ? wnx[ce] : -1;
                if constexpr (LOWER) {      // only what lies beyond the first pass's 16th neighbour of this split
                    if (!(d2 > lo_own_d || (d2 == lo_own_d && j > lo_own_i))) d2 = INF;
                }
                list_insert<KCAP>(own_d, own_i, d2, j);
            }
        }
        qcount = 0;
        // ---- refresh the gates ----------
        double thr_own = own_d[KCAP - 1];
#pragma unroll
        for (int k = 0; k < KCAP - 1; ++k) thr_own = (k == k_last) ? own_d[k] : thr_own;
        thr_own = fmin(thr_own, seed_thr);
        sthr[lane] = __double2float_ru(thr_own);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) G[qt] = gate_of(__shfl(thr_own, qt * 32 + (lane & 31), 64), qt);
    };

    // ---- a tile with a candidate: f16_event (f16_filter.hpp), column side only ----------------------------------------------
    auto event = [&](const v16f& c, const float (&l1)[5], const int qt, const float g, const int jb0, const unsigned todo, const int qlimit) __attribute__((always_inline)) -> unsigned {
        return f16_event<false>(c, l1, lanew[qt], g, false, jb0, todo, qlimit, wq, qcount);
    };

    // ---- staging (global_load_lds DMA, linear image) + MFMA ------------------------------------------------------------
    const auto Yh_bytes = (const __attribute__((address_space(1))) char*)a.Yh;
    auto stage_async = [&](int64_t c, int buf) { f16_stage_chunk<VPT>(Yh_bytes + c * (int64_t)CHUNK_BYTES, stage0 + buf * CHUNK_BYTES, tid, wave); };
    // one 32-row tile for both query tiles (or one of them): KST MFMAs per chain; the A fragments are read as the chain goes.
    // The statement after the chain spells out the wait states before the accumulators may be read through inline asm
    // (v_min3_f32: invisible to the compiler's hazard recogniser; 11 wait states are needed after an 8-pass MFMA).
    auto tile_mfma = [&](const char* lp, v16f (&acc)[QT]) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) {
            const v8h af = *reinterpret_cast<const v8h*>(lp + ks * 1024);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                if (ks == 0) {
                    v16f z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    acc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, b[qt][0], z, 0, 0, 0);
                } else {
                    acc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, b[qt][ks], acc[qt], 0, 0, 0);
                }
            }
        }
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]));
#endif
    };

    stage_async(c_lo, 0);

    // ---- seed phase: G groups of seed_tg tiles from the start of the split, group minima only (see the header) -----------
    // (tiles [0, G * seed_tg) of the split; the chunks are staged as in the sweep proper, which then starts again at chunk 0)
    const int seed_G = a.seed_groups > 0 ? a.seed_groups : a.ksel + (a.self_exclude ? 1 : 0);
    const int seed_tiles = a.seed_tg > 0 ? seed_G * a.seed_tg : 0;
    if (seed_tiles > 0) {
        float gmax[QT] = {-__builtin_huge_valf(), -__builtin_huge_valf()};      // max over the finished groups of the lane's group minimum
        float gmin[QT] = {__builtin_huge_valf(), __builtin_huge_valf()};
        int in_group = 0;
        const int nchunks_seed = (seed_tiles + CT - 1) / CT;
        for (int k = 0; k < nchunks_seed; ++k) {
            const int buf = k & 1;
            dma_barrier();
            // (the buffer filled next is the one the sweep proper starts from when this was the last seed chunk: chunk 0 again)
            stage_async(k + 1 < nchunks_seed ? c_lo + k + 1 : c_lo, buf ^ 1);
            const char* const lbuf = stage0 + buf * CHUNK_BYTES + lane * 16;
            const int thi = seed_tiles - k * CT < CT ? seed_tiles - k * CT : CT;
            for (int t = 0; t < thi; ++t) {
                v16f acc[QT];
                tile_mfma(lbuf + (t * KST) * 1024, acc);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    float l1[5];
                    gmin[qt] = fminf(gmin[qt], f16_min16(acc[qt], l1));
                }
                if (++in_group == a.seed_tg) {
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        // the two lanes that share a query column (l, l + 32) hold the halves of its rows
                        const float m = fminf(gmin[qt], __shfl_xor(gmin[qt], 32, 64));
                        gmax[qt] = fmaxf(gmax[qt], m);
                        gmin[qt] = __builtin_huge_valf();
                    }
                    in_group = 0;
                }
            }
        }
        // bound on the K-th squared distance of the lane's gated queries, then of the query it owns
        double thr_q[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            thr_q[qt] = INF;
            if (gq_c[qt] > -INF && gmax[qt] < __builtin_huge_valf()) thr_q[qt] = f16_seed_bound((double)gmax[qt], gq_xn[qt], gq_eps[qt], gq_a[qt], s2c);
        }
        const double t_lo = __shfl(thr_q[0], lane & 31, 64), t_hi = __shfl(thr_q[1], lane & 31, 64);
        seed_thr = lane < 32 ? t_lo : t_hi;
        sthr[lane] = __double2float_ru(seed_thr);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) G[qt] = gate_of(thr_q[qt], qt);
    } else {
        sthr[lane] = __builtin_huge_valf();
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) G[qt] = gate_of(INF, qt);
    }

    // ---- the sweep: every chunk of the split -----------------------------------------------------------------------------
    for (int k = 0; k < ntot; ++k) {
        const int buf = (seed_tiles > 0 ? ((seed_tiles + CT - 1) / CT + k) : k) & 1;       // (the seed phase left chunk 0 in the buffer after its last one)
        const int64_t c = c_lo + k;
        const int vs = k % 3;
        if (qcount >= MCE_PANEL_TRIGGER && lane == 0) wvote[vs] = 1;
        dma_barrier();
        if (tid == 0) wvote[vs == 0 ? 2 : vs - 1] = 0;
        if (k + 1 < ntot) stage_async(c + 1, buf ^ 1);
        bool need_drain = __builtin_amdgcn_readfirstlane(wvote[vs]) != 0 || k + 1 == ntot;
        const char* const lbuf = stage0 + buf * CHUNK_BYTES + lane * 16;
        const int jchunk = (int)(c * (CT * 32));
        for (int t = 0; t < CT; ++t) {
            v16f acc[QT];
            tile_mfma(lbuf + (t * KST) * 1024, acc);
            float l1[QT][5], mm[QT];
            bool pq[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                mm[qt] = f16_min16(acc[qt], l1[qt]);
                pq[qt] = mm[qt] <= G[qt];
            }
            if (__any(pq[0] || pq[1])) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    if (!__any(pq[qt])) continue;
                    const unsigned rem = event(acc[qt], l1[qt], qt, G[qt], jchunk + t * 32, 0xffffu, qlimit_gate);
                    if (rem) {
                        if (lane == 0) wredo[nredo] = (int)(rem | ((unsigned)qt << 16) | ((unsigned)t << 17));
                        nredo += 1;
                    }
                }
            }
        }
        // ---- chunk end: the deferred tiles and the drain ------------------------------------------------------------
        while (need_drain || nredo > 0 || (k + 1 == ntot && qcount > 0)) {
            drain();
            need_drain = false;
            const int n = nredo;
            nredo = 0;
            for (int i = 0; i < n; ++i) {
                const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wredo[i]);
                const unsigned todo = w & 0xffffu;
                const int qt = (int)((w >> 16) & 1u), t = (int)(w >> 17);
                v16f acc[QT];
                tile_mfma(lbuf + (t * KST) * 1024, acc);
                float l1[5];
                // (wave-uniform choice of the query tile)
                unsigned rem = 0;
                if (qt == 0) {
                    const float mm = f16_min16(acc[0], l1);
                    if (__any(mm <= G[0])) rem = event(acc[0], l1, 0, G[0], jchunk + t * 32, todo, QN - 64);
                } else {
                    const float mm = f16_min16(acc[1], l1);
                    if (__any(mm <= G[1])) rem = event(acc[1], l1, 1, G[1], jchunk + t * 32, todo, QN - 64);
                }
                if (rem) {
                    if (lane == 0) wredo[nredo] = (int)(rem | ((unsigned)qt << 16) | ((unsigned)t << 17));
                    nredo += 1;
                }
            }
        }
    }

    // ---- write the lists (lane l owns wave-local query l: coalesced) -------------------------------------------------------
    {
        const int64_t q = qwave0 + lane;
        const int64_t np = a.nq_pad;
        const auto pd = gptr_w(a.part_d) + (int64_t)split * KCAP * np;
        const auto pi = gptr_w(a.part_i) + (int64_t)split * KCAP * np;
#pragma unroll
        for (int k = 0; k < KCAP; ++k) {
            pd[(int64_t)k * np + q] = own_d[k];
            pi[(int64_t)k * np + q] = own_i[k];
        }
    }
}

}  // namespace mce
