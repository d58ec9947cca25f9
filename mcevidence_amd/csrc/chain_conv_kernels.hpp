// chain_conv_kernels.hpp -- the weighted per-segment moments behind converge= (mce_chain_conv_dev, capi_conv.hpp) for chains that
// are already on the device.  The rule is chain_conv.hpp's; this file arranges it into passes.  fp64 throughout, no atomics, plain
// C++ stores only, 64-bit row indices; every sum is formed in an order that the sizes of a system's own segments fix, so two runs
// give the same bits and a system's bits do not depend on its neighbours, its position or the call.  One call serves many systems:
// a segment table (rows, nrows, system, first tile) drives every launch; rows are read in place, ncols doubles apart.
//
//   conv_sum_tile_kernel     steps 1, 2: per tile of kConvTileRows = 1024 rows of a segment (counted from the segment's first row) and
//                            per column j < ndim: sum w (x_j - c_j) (c = null: sum w x_j); column ndim: sum w.  ONE kernel, launched
//                            twice: first without a centre -- it then also flags values and weights that status 3 refuses --, then
//                            with the centre the first launch gave.  (corr_mean_tile_kernel's thread layout; its body -- trunc(w),
//                            min and max -- is another sum, so the two share the layout and not the code.)
//   conv_sum_final_kernel    per (segment, column): the segment's tiles in tile order
//   conv_centre_kernel       step 1: per (system, column): c_j = the segments' sums in table order / the segments' weights
//   conv_moment_kernel       step 4, the kernel that does the work.  A workgroup owns one tile of 1024 rows and one round of up to
//                            256 blocks; a block is 4 x 4 entries (i, j) of the upper triangle.  It stages sub-tiles of
//                            kConvSubRows = 32 centred rows y = (x - c) - a_s and their weights in LDS (row-major, 4 * ceil(d / 4)
//                            doubles per row, zeros in the padding) and a thread reads per staged row 4 + 4 values -- two 32-byte
//                            runs -- for 16 FMAs acc[a][b] += (w y_i[a]) y_j[b].  With nb blocks in the round, G = 256 / nb threads
//                            share a block, thread g taking the rows g, g + G, .. of every sub-tile; their sums meet in LDS in the
//                            order g = 0, 1, ..  partial[tile][pair].
//   conv_moment_final_kernel per (segment, pair): the segment's tiles in tile order, divided by W_s -> C_s
//   conv_system_kernel       steps 3, 5, 6 and 7's normalisation: one workgroup per system, its segments in table order:
//                            Wn, delta / sigma, per_param, the status
//   (mce_eig_sym_batch_dev_f64's kernel on the Wn of all systems)
//   conv_t_kernel            step 8: one workgroup per system: v_s, then T + I
//   (the solver once more)
//   conv_result_kernel       r_minus_1 = lam[0] - 1 and the final status, packed with per_param for one copy to the host
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_conv.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kConvThreads = 256;
constexpr int kConvTileRows = 1024;
constexpr int kConvSubRows = 32;
constexpr int kConvBlock = 4;                                   // a thread's block of (i, j): 4 x 4
constexpr int kConvMaxLd = 128;                                 // doubles per staged row: 4 * ceil(127 / 4)

struct ConvSeg {
    const double* rows;      // first row of the segment
    int64_t nrows;
    int64_t tile0;           // its first tile (tiles of kConvTileRows rows, counted over the call's segments in table order)
    int32_t sys, pad;
};
struct ConvSys {
    int32_t seg0, nseg;      // its segments in the table
};

// the segment that owns tile k (tile0 ascending; a segment without rows owns none)
__device__ __forceinline__ int conv_seg_of(const ConvSeg* __restrict__ segs, int nseg, int64_t k)
{
    return mce_seg::last_at_or_below(nseg, k, [segs](int i) { return segs[i].tile0; });
}

// grid: the tiles.  Thread (rs, j): column j of the rows rs, rs + RS, .. of the tile, RS = 256 / CL row lanes, CL = the power of two
// >= ndim + 1; then the RS lanes of a column in lane order.  out[tile][ndim + 1]; bad[tile][ndim + 1] (centre == null only): a value
// of column j that is not finite; [ndim]: a weight that is negative or not finite.
__global__ __launch_bounds__(kConvThreads) void conv_sum_tile_kernel(const ConvSeg* __restrict__ segs, int nseg, int64_t ncols, int iw, int itheta, int ndim,
                                                                     int cl, const double* __restrict__ centre, double* __restrict__ out,
                                                                     int32_t* __restrict__ bad)
{
    __shared__ double s_sum[kConvThreads];
    __shared__ int s_bad[kConvThreads];
    const int tid = threadIdx.x, j = tid % cl, rs = tid / cl, nrs = kConvThreads / cl;
    const int64_t tile = blockIdx.x;
    const ConvSeg seg = segs[conv_seg_of(segs, nseg, tile)];
    const int64_t r0 = (tile - seg.tile0) * kConvTileRows;
    const int64_t r1 = r0 + kConvTileRows < seg.nrows ? r0 + kConvTileRows : seg.nrows;
    const double cj = (centre && j < ndim) ? centre[(int64_t)seg.sys * ndim + j] : 0.0;
    double sum = 0.0;
    int flag = 0;
    if (j <= ndim)
        for (int64_t r = r0 + rs; r < r1; r += nrs) {
            const double* row = seg.rows + r * ncols;
            const double w = row[iw];
            if (j < ndim) {
                const double v = row[itheta + j];
                flag |= mce_conv::conv_value_ok(v) ? 0 : 1;
                sum += w * (v - cj);
            } else {
                flag |= mce_conv::conv_weight_ok(w) ? 0 : 1;
                sum += w;
            }
        }
    s_sum[tid] = sum;
    s_bad[tid] = flag;
    __syncthreads();
    if (rs == 0 && j <= ndim) {
        for (int k = 1; k < nrs; ++k) {
            sum += s_sum[k * cl + j];
            flag |= s_bad[k * cl + j];
        }
        out[tile * (ndim + 1) + j] = sum;
        if (!centre) bad[tile * (ndim + 1) + j] = flag;
    }
}

// one thread per (segment, column <= ndim): the segment's tiles in order
__global__ __launch_bounds__(kConvThreads) void conv_sum_final_kernel(const ConvSeg* __restrict__ segs, int nseg, int ndim, const double* __restrict__ tiles,
                                                                      const int32_t* __restrict__ tbad, double* __restrict__ segsum,
                                                                      int32_t* __restrict__ segbad)
{
    const int nc = ndim + 1;
    const int64_t e = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    if (e >= (int64_t)nseg * nc) return;
    const int s = (int)(e / nc), j = (int)(e - (int64_t)s * nc);
    const ConvSeg seg = segs[s];
    const int64_t nt = (seg.nrows + kConvTileRows - 1) / kConvTileRows;
    double sum = 0.0;
    int flag = 0;
#pragma unroll 8
    for (int64_t k = 0; k < nt; ++k) {
        sum += tiles[(seg.tile0 + k) * nc + j];
        if (tbad) flag |= tbad[(seg.tile0 + k) * nc + j];
    }
    segsum[e] = sum;
    if (tbad) segbad[e] = flag;
}

// one thread per (system, column): c_j = sum_s (sum w x_j) / sum_s W_s, the segments in table order
__global__ __launch_bounds__(kConvThreads) void conv_centre_kernel(const ConvSys* __restrict__ systems, int nsys, int ndim, const double* __restrict__ seg1,
                                                                   double* __restrict__ centre)
{
    const int nc = ndim + 1;
    const int64_t e = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    if (e >= (int64_t)nsys * ndim) return;
    const int y = (int)(e / ndim), j = (int)(e - (int64_t)y * ndim);
    const ConvSys sy = systems[y];
    double sum = 0.0, W = 0.0;
    for (int s = sy.seg0; s < sy.seg0 + sy.nseg; ++s) {
        sum += seg1[(int64_t)s * nc + j];
        W += seg1[(int64_t)s * nc + ndim];
    }
    centre[e] = sum / W;
}

// grid: (tiles, rounds of 256 blocks).  partial[tile * npair + pair]
__global__ __launch_bounds__(kConvThreads) void conv_moment_kernel(const ConvSeg* __restrict__ segs, int nseg, int64_t ncols, int iw, int itheta, int ndim,
                                                                   const double* __restrict__ centre, const double* __restrict__ seg1,
                                                                   const double* __restrict__ seg2, double* __restrict__ partial)
{
    __shared__ double s_y[kConvSubRows * kConvMaxLd];          // the staged rows; afterwards the threads' sums (256 x 16 doubles: the same size)
    __shared__ double s_w[kConvSubRows];
    __shared__ double s_off[kConvMaxLd];                        // c_j + a_sj is NOT formed: s_off keeps c_j, s_a keeps a_sj
    __shared__ double s_a[kConvMaxLd];
    static_assert(kConvSubRows * kConvMaxLd == kConvThreads * kConvBlock * kConvBlock, "the sums take the staged rows' place");
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int sidx = conv_seg_of(segs, nseg, tile);
    const ConvSeg seg = segs[sidx];
    const int nbd = (ndim + kConvBlock - 1) / kConvBlock, ld = nbd * kConvBlock;
    const int nblk = nbd * (nbd + 1) / 2;
    const int blk0 = blockIdx.y * kConvThreads;
    const int nb = nblk - blk0 < kConvThreads ? nblk - blk0 : kConvThreads;      // blocks of this round
    const int G = kConvThreads / nb;                                             // threads per block
    const int b = tid % nb, g = tid / nb;
    const bool active = g < G;
    // block blk0 + b -> (bi <= bj), row-major over the upper triangle of nbd x nbd
    int bi = 0, bj = 0;
    {
        int p = blk0 + b, base = 0;
        while (base + (nbd - bi) <= p) { base += nbd - bi; ++bi; }
        bj = bi + (p - base);
    }
    const int nc = ndim + 1;
    const double Ws = seg1[(int64_t)sidx * nc + ndim];
    for (int j = tid; j < ld; j += kConvThreads) {
        s_off[j] = j < ndim ? centre[(int64_t)seg.sys * ndim + j] : 0.0;
        s_a[j] = j < ndim ? seg2[(int64_t)sidx * nc + j] / Ws : 0.0;
    }
    const int64_t r0 = (tile - seg.tile0) * kConvTileRows;
    const int64_t r1 = r0 + kConvTileRows < seg.nrows ? r0 + kConvTileRows : seg.nrows;
    double acc[kConvBlock][kConvBlock];
#pragma unroll
    for (int a = 0; a < kConvBlock; ++a)
#pragma unroll
        for (int c = 0; c < kConvBlock; ++c) acc[a][c] = 0.0;
    for (int64_t t0 = r0; t0 < r1; t0 += kConvSubRows) {
        const int rows = (int)(r1 - t0 < kConvSubRows ? r1 - t0 : kConvSubRows);
        __syncthreads();                                     // (s_off, s_a written; the previous sub-tile read)
        for (int e = tid; e < rows * ld; e += kConvThreads) {
            const int r = e / ld, j = e - r * ld;
            s_y[e] = j < ndim ? (seg.rows[(t0 + r) * ncols + itheta + j] - s_off[j]) - s_a[j] : 0.0;
        }
        if (tid < rows) s_w[tid] = seg.rows[(t0 + tid) * ncols + iw];
        __syncthreads();
        if (active)
            for (int r = g; r < rows; r += G) {
                const double w = s_w[r];
                const double* yi = s_y + r * ld + bi * kConvBlock;
                const double* yj = s_y + r * ld + bj * kConvBlock;
                double vi[kConvBlock], vj[kConvBlock];
#pragma unroll
                for (int a = 0; a < kConvBlock; ++a) { vi[a] = w * yi[a]; vj[a] = yj[a]; }
#pragma unroll
                for (int a = 0; a < kConvBlock; ++a)
#pragma unroll
                    for (int c = 0; c < kConvBlock; ++c) acc[a][c] = fma(vi[a], vj[c], acc[a][c]);
            }
    }
    __syncthreads();                                         // (the last sub-tile read: the sums take its place)
#pragma unroll
    for (int a = 0; a < kConvBlock; ++a)
#pragma unroll
        for (int c = 0; c < kConvBlock; ++c) s_y[(a * kConvBlock + c) * kConvThreads + tid] = acc[a][c];
    __syncthreads();
    if (g == 0) {
        const int npair = mce_conv::conv_npair(ndim);
#pragma unroll
        for (int a = 0; a < kConvBlock; ++a)
#pragma unroll
            for (int c = 0; c < kConvBlock; ++c) {
                const int i = bi * kConvBlock + a, j = bj * kConvBlock + c;
                if (i > j || j >= ndim) continue;
                double sum = acc[a][c];
                for (int k = 1; k < G; ++k) sum += s_y[(a * kConvBlock + c) * kConvThreads + k * nb + b];
                partial[tile * npair + mce_conv::conv_pair(ndim, i, j)] = sum;
            }
    }
}

// one thread per (segment, pair): the segment's tiles in order, divided by W_s (a segment without rows or weight: 0)
__global__ __launch_bounds__(kConvThreads) void conv_moment_final_kernel(const ConvSeg* __restrict__ segs, int nseg, int ndim, const double* __restrict__ seg1,
                                                                         const double* __restrict__ partial, double* __restrict__ Cs)
{
    const int npair = mce_conv::conv_npair(ndim);
    const int64_t e = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    if (e >= (int64_t)nseg * npair) return;
    const int s = (int)(e / npair), p = (int)(e - (int64_t)s * npair);
    const ConvSeg seg = segs[s];
    const int64_t nt = (seg.nrows + kConvTileRows - 1) / kConvTileRows;
    const double Ws = seg1[(int64_t)s * (ndim + 1) + ndim];
    double sum = 0.0;
#pragma unroll 8
    for (int64_t k = 0; k < nt; ++k) sum += partial[(seg.tile0 + k) * npair + p];
    Cs[e] = (nt > 0 && Ws > 0.0) ? sum / Ws : 0.0;
}

// one workgroup per system.  out_pp[sys][ndim], status[sys][2], used[sys]; Wn[sys][d * d]; dn[seg][d] = delta_sj / sigma_j.
// A system whose status is not 0 gets Wn = I and dn = 0, so that the solver and conv_t_kernel run through it unharmed.
__global__ __launch_bounds__(kConvThreads) void conv_system_kernel(const ConvSeg* __restrict__ segs, const ConvSys* __restrict__ systems, int ndim,
                                                                   const double* __restrict__ seg1, const int32_t* __restrict__ segbad,
                                                                   const double* __restrict__ seg2, const double* __restrict__ Cs,
                                                                   double* __restrict__ Wn, double* __restrict__ dn, double* __restrict__ out_pp,
                                                                   int32_t* __restrict__ status, int32_t* __restrict__ used)
{
    __shared__ double s_o[kConvMaxLd], s_diag[kConvMaxLd], s_sigma[kConvMaxLd];
    __shared__ int s_bad[kConvMaxLd];
    __shared__ int s_status[2], s_used, s_badw;
    const int tid = threadIdx.x, y = blockIdx.x, d = ndim, nc = ndim + 1;
    const int npair = mce_conv::conv_npair(d);
    const ConvSys sy = systems[y];
    const int s0 = sy.seg0, s1 = sy.seg0 + sy.nseg;
    if (tid == 0) {
        int M = 0, badw = 0;
        for (int s = s0; s < s1; ++s) {
            M += (segs[s].nrows > 0 && seg1[(int64_t)s * nc + d] > 0.0) ? 1 : 0;
            badw |= segbad[(int64_t)s * nc + d];
        }
        s_used = M;
        s_badw = badw;
    }
    __syncthreads();
    const int M = s_used;
    if (tid < d) {
        const int j = tid;
        double o = 0.0, Wu = 0.0, diag = 0.0;
        int flag = 0;
        for (int s = s0; s < s1; ++s) {
            flag |= segbad[(int64_t)s * nc + j];
            const double Ws = seg1[(int64_t)s * nc + d];
            if (!(segs[s].nrows > 0 && Ws > 0.0)) continue;
            o += seg2[(int64_t)s * nc + j];                    // W_s a_sj
            Wu += Ws;
            diag += Cs[(int64_t)s * npair + mce_conv::conv_pair(d, j, j)];
        }
        s_o[j] = o / Wu;
        s_diag[j] = diag / (double)M;
        s_bad[j] = flag;
    }
    __syncthreads();
    if (tid == 0) {
        int column = -1;
        s_status[0] = mce_conv::conv_status(s_badw != 0, s_bad, M, s_diag, d, &column);
        s_status[1] = column;
        status[2 * y] = s_status[0];
        status[2 * y + 1] = column;
        used[y] = M;
    }
    __syncthreads();
    const bool ok = s_status[0] == mce_conv::kConvOk;
    if (tid < d) s_sigma[tid] = ok ? sqrt(s_diag[tid]) : 1.0;
    __syncthreads();
    double* W = Wn + (int64_t)y * d * d;
    for (int p = tid; p < npair; p += kConvThreads) {
        int i = 0, base = 0;
        while (base + (d - i) <= p) { base += d - i; ++i; }
        const int j = i + (p - base);
        double v = i == j ? 1.0 : 0.0;
        if (ok && i != j) {
            double sum = 0.0;
            for (int s = s0; s < s1; ++s)
                if (segs[s].nrows > 0 && seg1[(int64_t)s * nc + d] > 0.0) sum += Cs[(int64_t)s * npair + p];
            v = (sum / (double)M) / (s_sigma[i] * s_sigma[j]);
        }
        W[i * d + j] = v;
        W[j * d + i] = v;
    }
    if (tid < d) {
        const int j = tid;
        double bjj = 0.0;
        for (int s = s0; s < s1; ++s) {
            const double Ws = seg1[(int64_t)s * nc + d];
            const bool use = ok && segs[s].nrows > 0 && Ws > 0.0;
            const double delta = use ? seg2[(int64_t)s * nc + j] / Ws - s_o[j] : 0.0;
            bjj += delta * delta;
            dn[(int64_t)s * d + j] = use ? delta / s_sigma[j] : 0.0;
        }
        out_pp[(int64_t)y * d + j] = ok ? bjj / (double)(M - 1) / s_diag[j] : NAN;
    }
}

// one workgroup per system: v[seg][e] = scale[e] sum_j evec[j][e] dn[seg][j], then T[i][j] = sum_s v_s[i] v_s[j] / (M - 1) + (i == j),
// the segments in table order (a skipped segment's dn is 0 and adds +0).  A system whose Wn is not positive definite (conv_posdef; kept in posdef[sys])
// gets T = I.  v is the call's scratch in global memory: 128 segments x 127 doubles do not fit the default LDS window.
__global__ __launch_bounds__(kConvThreads) void conv_t_kernel(const ConvSys* __restrict__ systems, int ndim, const double* __restrict__ dn,
                                                              const double* __restrict__ evec, const double* __restrict__ scale,
                                                              const double* __restrict__ lam, const int32_t* __restrict__ stat,
                                                              const int32_t* __restrict__ used, double* v, double* __restrict__ T,
                                                              int32_t* __restrict__ posdef)
{
    const int tid = threadIdx.x, y = blockIdx.x, d = ndim;
    const ConvSys sy = systems[y];
    const bool pd = mce_conv::conv_posdef(stat[y * mce_eig::kStatInts + mce_eig::kStatCode], lam[(int64_t)y * d + d - 1], d);
    const bool ok = pd && used[y] >= 2;
    if (tid == 0) posdef[y] = pd ? 1 : 0;
    const double* U = evec + (int64_t)y * d * d;
    const double* sc = scale + (int64_t)y * d;
    for (int e = tid; e < sy.nseg * d; e += kConvThreads) {
        const int s = sy.seg0 + e / d, k = e % d;
        double t = 0.0;
        for (int j = 0; j < d; ++j) t = fma(U[j * d + k], dn[(int64_t)s * d + j], t);
        v[(int64_t)s * d + k] = ok ? t * sc[k] : 0.0;
    }
    __syncthreads();                                         // (v is written and read by this workgroup alone)
    const double div = (double)(used[y] > 1 ? used[y] - 1 : 1);
    double* Ty = T + (int64_t)y * d * d;
    for (int e = tid; e < d * d; e += kConvThreads) {
        const int i = e / d, j = e - i * d;
        if (i > j) continue;
        double sum = 0.0;
        for (int s = sy.seg0; s < sy.seg0 + sy.nseg; ++s) sum = fma(v[(int64_t)s * d + i], v[(int64_t)s * d + j], sum);
        const double t = sum / div + (i == j ? 1.0 : 0.0);
        Ty[i * d + j] = t;
        Ty[j * d + i] = t;
    }
}

// res[sys * (ndim + 4) ..] = {r_minus_1, status, column, used, per_param[ndim]}: everything the host wants, in one block
__global__ __launch_bounds__(kConvThreads) void conv_result_kernel(int nsys, int ndim, const double* __restrict__ lam2, const int32_t* __restrict__ stat1,
                                                                   const int32_t* __restrict__ posdef, const int32_t* __restrict__ stat2, const int32_t* __restrict__ status,
                                                                   const int32_t* __restrict__ used, const double* __restrict__ pp,
                                                                   double* __restrict__ res)
{
    const int64_t e = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    const int nr = ndim + 4;
    if (e >= (int64_t)nsys * nr) return;
    const int y = (int)(e / nr), k = (int)(e - (int64_t)y * nr);
    int code = status[2 * y], column = status[2 * y + 1];
    if (code == mce_conv::kConvOk &&
        (!posdef[y] || stat2[y * mce_eig::kStatInts + mce_eig::kStatCode] != mce_eig::kStatusOk)) {
        code = mce_conv::kConvNotPositive;
        column = stat1[y * mce_eig::kStatInts + mce_eig::kStatIndex];
    }
    double out;
    if (k == 0) out = code == mce_conv::kConvOk ? lam2[(int64_t)y * ndim] - 1.0 : NAN;
    else if (k == 1) out = (double)code;
    else if (k == 2) out = (double)column;
    else if (k == 3) out = (double)used[y];
    else out = pp[(int64_t)y * ndim + (k - 4)];
    res[e] = out;
}

}  // namespace mce
