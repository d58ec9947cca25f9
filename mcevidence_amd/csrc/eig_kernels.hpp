// eig_kernels.hpp -- the batched symmetric eigen-solver of the evidence feed on the device (docs/design/device_eig.md): one
// workgroup per d x d system, parallel Jacobi in the tournament order of eig_jacobi.hpp, whose rules (schedule, rotation,
// canonical form, status) it shares with the serial driver there.  fp64 throughout, no atomics, every loop bounded by the
// sweep cap; a system's bits depend on its own matrix alone -- not on its place in the batch, nor on the batch's size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eig_jacobi.hpp"

namespace mce {

constexpr int kEigMaxDim = 127;
constexpr int kEigMaxPairs = (kEigMaxDim + 1) / 2;      // 64: one wave's lanes
constexpr int kEigMaxThreads = 1024;
constexpr int kEigNarrowDim = 64;                       // up to here: at most 256 threads, 16 rows of V per wave; beyond: 1024 threads, 8 rows
// threads per workgroup by d: a wave serves 64 pairs of one row, so small systems gain nothing from more waves but barriers
__host__ __device__ constexpr int eig_threads(int d) { return d <= 16 ? 64 : d <= 64 ? 256 : kEigMaxThreads; }
__host__ __device__ constexpr int eig_rows_per_wave(int d) { return d <= kEigNarrowDim ? 16 : 8; }      // rows of V a wave keeps in registers
static_assert(eig_threads(16) / 64 * eig_rows_per_wave(16) >= 16 && eig_threads(kEigNarrowDim) / 64 * eig_rows_per_wave(kEigNarrowDim) >= kEigNarrowDim &&
              eig_threads(kEigMaxDim) / 64 * eig_rows_per_wave(kEigMaxDim) >= kEigMaxDim, "every row of V has a wave and a register");
// LDS: the full symmetric matrix with an odd leading dimension (its rows then start in different banks) | lam[128] | sgn[128] |
// c[64] | s[64] | rank[128] | p[64] | q[64] | on[64] -- sized by d, so that small systems share a CU (d = 127: 133 384 bytes)
__host__ __device__ constexpr int eig_ld(int d) { return d | 1; }
__host__ __device__ constexpr size_t eig_lds_bytes(int d)
{
    return ((size_t)d * eig_ld(d) + 2 * (kEigMaxDim + 1) + 2 * kEigMaxPairs) * sizeof(double) + ((kEigMaxDim + 1) + 3 * kEigMaxPairs) * sizeof(int);
}

// cov [nsys][d*d] (row-major, symmetric, untouched) -> evec [nsys][d*d] (eigenvectors in the columns), scale [nsys][d] =
// 1 / sqrt(lam), lam [nsys][d] (descending), stat [nsys][mce_eig::kStatInts].
// Per step: (1) one lane per pair computes (c, s) or a skip from the matrix as it stands; (2) A <- A J, a wave per row, its
// lanes across the pairs; (3) A <- J^T A, a wave per pair, its lanes across the columns; (4) V <- V J.
// V never leaves the registers: a row of V is rotated by itself, so wave w keeps rows w, w + nw, ... for the whole solve, and
// lane k keeps, of each, the two columns of pair k -- the circle method's "top" (s + k) mod (m - 1) (lane 0: s) and "bottom"
// (s - k) mod (m - 1) (lane 0: the slot that stays, m - 1).  (4) is then a rotation inside the lane, done beside (2) with the
// same (c, s), and going from step s to s + 1 every top moves one lane down and every bottom one lane up (the last lane's bottom
// becomes its top, lane 0's top becomes lane 1's bottom): two shuffles per row, beside (3).  (The first form of this kernel kept V
// in the output buffer and paid two global round trips per step: 8.4 ms for one system at d = 127 against 7.0 ms, measured;
// a third form with 512 threads and four LDS loads in flight per lane took 12.7 ms -- docs/design/device_eig.md.)
// After whole sweeps the layout is that of step 0 again; V is then staged through A's place in LDS for the canonical form.
// A step without a rotation only shifts.
// Two instantiations, so that neither spills: <16, 256> for d <= kEigNarrowDim, <8, 1024> beyond.
template <int kEigRowsPerWave, int kThreads>
__global__ __launch_bounds__(kThreads) void eig_jacobi_kernel(const double* __restrict__ cov, int d, double* evec, double* __restrict__ scale,
                                                                   double* __restrict__ lam_out, int32_t* __restrict__ stat)
{
    extern __shared__ double eig_sh[];
    const int ld = eig_ld(d);
    double* A = eig_sh;
    double* lam = A + (size_t)d * ld;
    double* sgn = lam + (kEigMaxDim + 1);
    double* cs = sgn + (kEigMaxDim + 1);
    double* sn = cs + kEigMaxPairs;
    int* rank = reinterpret_cast<int*>(sn + kEigMaxPairs);
    int* pp = rank + (kEigMaxDim + 1);
    int* qq = pp + kEigMaxPairs;
    int* on = qq + kEigMaxPairs;

    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const size_t sys = blockIdx.x;
    const double* C = cov + sys * (size_t)d * d;
    double* V = evec + sys * (size_t)d * d;
    const int m = mce_eig::slots(d), ring = m - 1;
    double* sc = scale + sys * (size_t)d;
    double* lo = lam_out + sys * (size_t)d;
    int32_t* so = stat + sys * mce_eig::kStatInts;
    const int np = mce_eig::pairs_per_step(d), nsteps = mce_eig::steps_per_sweep(d);

    int bad = 0;
    for (int e = tid; e < d * d; e += nt) {
        const int r = e / d, c = e - r * d;
        const double x = C[e];
        A[r * ld + c] = x;
        bad |= mce_eig::is_finite(x) ? 0 : 1;
    }
    if (__syncthreads_or(bad)) {          // status 1, before the first sweep: identity, unit scales, the input's diagonal
        for (int e = tid; e < d * d; e += nt) V[e] = (e / d) == (e % d) ? 1.0 : 0.0;
        for (int i = tid; i < d; i += nt) {
            sc[i] = 1.0;
            lo[i] = A[i * ld + i];
        }
        if (tid == 0) {
            so[mce_eig::kStatCode] = mce_eig::kStatusNotFinite;
            so[mce_eig::kStatIndex] = 0;
            so[mce_eig::kStatSweeps] = 0;
            so[mce_eig::kStatRotations] = 0;
        }
        return;
    }

    // V = I in the layout of step 0: lane k holds columns k (top) and m - 1 - k (bottom; lane 0: the slot that stays)
    double vt[kEigRowsPerWave], vb[kEigRowsPerWave];
#pragma unroll
    for (int u = 0; u < kEigRowsPerWave; ++u) {
        const int r = wave + u * nw;
        vt[u] = (lane < np && r == lane) ? 1.0 : 0.0;
        vb[u] = (lane < np && r == m - 1 - lane) ? 1.0 : 0.0;          // (the padding slot's column, m - 1 = d: no row has that number)
    }
    auto shift = [&]() {          // the layout of the next step
        if (np < 2) return;
#pragma unroll
        for (int u = 0; u < kEigRowsPerWave; ++u) {
            if (wave + u * nw >= d) continue;          // (uniform over the wave)
            const double down = __shfl_down(vt[u], 1, 64);
            const double up = __shfl_up(lane == 0 ? vt[u] : vb[u], 1, 64);
            vt[u] = lane == np - 1 ? vb[u] : down;
            if (lane != 0) vb[u] = up;
        }
    };

    int sweeps = 0, rotations = 0;         // (rotations: lane k of wave 0 counts pair k's)
    while (sweeps < mce_eig::kMaxSweeps) {
        int rotated = 0;
        for (int step = 0; step < nsteps; ++step) {
            int mine = 0;
            if (tid < np) {                                                   // phase 1
                int p, q;
                mce_eig::pair_of(d, step, tid, p, q);
                double c = 1.0, s = 0.0;
                if (q < d) mine = mce_eig::rotation(A[p * ld + p], A[q * ld + q], A[p * ld + q], c, s) ? 1 : 0;
                pp[tid] = p;
                qq[tid] = q;
                cs[tid] = c;
                sn[tid] = s;
                on[tid] = mine;
                rotations += mine;
            }
            if (!__syncthreads_or(mine)) {                                    // (uniform: every thread sees the same OR)
                shift();
                continue;
            }
            rotated = 1;
            if (lane < np && on[lane]) {                                      // phase 2: columns p, q of every row; phase 4 in the registers
                const int p = pp[lane], q = qq[lane];
                const double c = cs[lane], s = sn[lane];
                for (int r = wave; r < d; r += nw) mce_eig::rotate(c, s, A[r * ld + p], A[r * ld + q]);
                const int top = lane == 0 ? step : (step + lane) % ring;
                if (top == p) {
#pragma unroll
                    for (int u = 0; u < kEigRowsPerWave; ++u) mce_eig::rotate(c, s, vt[u], vb[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < kEigRowsPerWave; ++u) mce_eig::rotate(c, s, vb[u], vt[u]);
                }
            }
            __syncthreads();
            for (int k = wave; k < np; k += nw) {                             // phase 3: rows p, q, every column
                if (!on[k]) continue;
                const int p = pp[k], q = qq[k];
                const double c = cs[k], s = sn[k];
                for (int col = lane; col < d; col += 64) mce_eig::rotate(c, s, A[p * ld + col], A[q * ld + col]);
            }
            shift();
            __syncthreads();
        }
        ++sweeps;
        if (!rotated) break;
    }

    // canonical form: the diagonal leaves A, then V takes A's place in LDS (the columns are permuted on the way out)
    __syncthreads();
    for (int i = tid; i < d; i += nt) sgn[i] = A[i * ld + i];                 // (sgn: the unsorted eigenvalues for now)
    if (tid < kEigMaxPairs) cs[tid] = (double)rotations;
    __syncthreads();
    for (int i = tid; i < d; i += nt) {
        const int r = mce_eig::rank_of(sgn, d, i);
        rank[i] = r;
        lam[r] = sgn[i];
    }
    __syncthreads();                                                          // (every diagonal entry read: V takes A's place)
    if (lane < np) {
        const int top = lane, bottom = m - 1 - lane;          // whole sweeps: the layout of step 0
#pragma unroll
        for (int u = 0; u < kEigRowsPerWave; ++u) {
            const int r = wave + u * nw;
            if (r >= d) continue;
            A[r * ld + top] = vt[u];
            if (bottom < d) A[r * ld + bottom] = vb[u];
        }
    }
    __syncthreads();
    int index = 0;
    const int code = mce_eig::status_of(lam, d, index);                       // (every thread: d <= 127 LDS reads, uniform)
    __syncthreads();
    for (int i = tid; i < d; i += nt) sgn[i] = mce_eig::sign_of(A, d, ld, i);
    __syncthreads();
    for (int e = tid; e < d * d; e += nt) {
        const int r = e / d, c = e - r * d;
        if (code == mce_eig::kStatusOk) V[(size_t)r * d + rank[c]] = sgn[c] * A[r * ld + c];
        else V[e] = r == c ? 1.0 : 0.0;
    }
    for (int i = tid; i < d; i += nt) {
        lo[i] = lam[i];
        sc[i] = code == mce_eig::kStatusOk ? 1.0 / sqrt(lam[i]) : 1.0;
    }
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < np; ++k) total += (int)cs[k];
        so[mce_eig::kStatCode] = code;
        so[mce_eig::kStatIndex] = index;
        so[mce_eig::kStatSweeps] = sweeps;
        so[mce_eig::kStatRotations] = total;
    }
}

}  // namespace mce
