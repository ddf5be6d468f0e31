// mcs_kernels.hpp -- the kernels of libmcmcref_std.so behind the summary pipeline (include/mcmcref_std.h): the Blom
// table, the copy that drops the middle draw of odd chains, the series kernel (decode, chain moments, deviations) and the
// walk kernel (lag products, pooled autocovariance, Geyer's walk).  The arithmetic is mcs_core.hpp's, one text with the
// host routine.
#pragma once
#include "mcr_pipe.hpp"
#include "mcs_core.hpp"

namespace mcs {

using mcr::i64;
using mcr::u32;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kLanes;
constexpr int kLdsDraws = MCS_LDS_DRAWS;

// tab[n2], n2 < 2 S: the Blom score of rank code n2 (tab[0] is never a draw's)
__global__ __launch_bounds__(256) void k_mcs_blom(double* __restrict__ tab, i64 S)
{
    const i64 n2 = (i64)blockIdx.x * 256 + threadIdx.x;
    if (n2 >= 2 * S) return;
    tab[n2] = n2 >= 1 ? mcr::inv_cdf(blom_p(n2, S)) : 0.0;
}

// X[p][k][i], k = 2 c + h < 2 C, i < n: draw h (N - n) + i of chain c of parameter p0 + p, widened.  A grid-stride loop.
template <typename T>
__global__ __launch_bounds__(256) void k_mcs_copy_split(const T* __restrict__ src, double* __restrict__ X, i64 C, i64 N, i64 pc,
                                                        i64 sc, i64 sn, i64 sp, i64 p0)
{
    const i64 n = N / 2, S = 2 * C * n, total = pc * S;
    for (i64 at = (i64)blockIdx.x * 256 + threadIdx.x; at < total; at += (i64)gridDim.x * 256) {
        const i64 p = at / S, r = at - p * S, k = r / n, i = r - k * n;
        X[at] = (double)src[(k >> 1) * sc + ((k & 1) * (N - n) + i) * sn + (p0 + p) * sp];
    }
}

// ------------------------------------------------------------------------------------------------
// k_mcs_series: a wave owns a split chain (parameter p, chain k), four chains per workgroup.  Two passes over the chain's
// n draws, lane l taking the draws l, l + 64, ..: the sums of the series (lane_partial, then the xor tree: every lane gets
// the same bits) with their minima and maxima, then the deviations from the chain mean, which go to D, and their squares.
// Scalar loads only: nothing depends on the alignment of a row.  nser = 4, or 5 with the raw series.
// D[((p nser + s) m + k) n + i];  mom[((p nser + s) m + k) kMomRec + {mean, q, min, max}].
// ------------------------------------------------------------------------------------------------
struct SeriesIn {
    const double* X;       // [pc][S]
    const u32 *zb, *zt;    // [pc][S] rank codes of x and of |x - median|
    const double* blom;    // [2 S]
    const double* res;     // the pipeline's result table: rows R_Q0, R_Q0 + 1 are the 5 % and 95 % quantiles
    i64 m, n, pc;
    int nser;
};

__device__ __forceinline__ void series_at(const SeriesIn& a, const double* x, const u32* b, const u32* t, i64 i, u32 cmax,
                                          double q05, double q95, double (&v)[kSeries])
{
    const double xi = x[i];
    const u32 cb = b[i], ct = t[i];
    v[S_BULK] = a.blom[cb < cmax ? cb : cmax];          // (the clamp: codes of a tensor with NaN draws may be stale bytes)
    v[S_FOLD] = a.blom[ct < cmax ? ct : cmax];
    v[S_Q05] = xi <= q05 ? 1.0 : 0.0;
    v[S_Q95] = xi <= q95 ? 1.0 : 0.0;
    v[S_RAW] = xi;
}

__global__ __launch_bounds__(kThreads) void k_mcs_series(SeriesIn a, double* __restrict__ D, double* __restrict__ mom)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kLanes - 1);
    const i64 id = (i64)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (id >= a.pc * a.m) return;                          // (no workgroup barrier below: the waves are independent)
    const i64 p = id / a.m, k = id - p * a.m, n = a.n, S = a.m * n;
    const i64 row = p * S + k * n;
    const double* x = a.X + row;
    const u32 *b = a.zb + row, *t = a.zt + row;
    const u32 cmax = (u32)(2 * S - 1);
    const double q05 = a.res[(i64)mcr::R_Q0 * a.pc + p], q95 = a.res[(i64)(mcr::R_Q0 + 1) * a.pc + p];
    double s[kSeries], lo[kSeries], hi[kSeries], v[kSeries], mean[kSeries], q[kSeries];
#pragma unroll
    for (int j = 0; j < kSeries; ++j) { s[j] = 0.0; lo[j] = INFINITY; hi[j] = -INFINITY; q[j] = 0.0; }
    for (i64 i = lane; i < n; i += kLanes) {
        series_at(a, x, b, t, i, cmax, q05, q95, v);
#pragma unroll
        for (int j = 0; j < kSeries; ++j) {
            s[j] = s[j] + v[j];
            lo[j] = v[j] < lo[j] ? v[j] : lo[j];
            hi[j] = v[j] > hi[j] ? v[j] : hi[j];
        }
    }
#pragma unroll
    for (int j = 0; j < kSeries; ++j) {
        mean[j] = mcr::xor_tree_sum(s[j]) / (double)n;
        for (int o = kLanes / 2; o > 0; o >>= 1) {
            const double l2 = __shfl_xor(lo[j], o, kLanes), h2 = __shfl_xor(hi[j], o, kLanes);
            lo[j] = l2 < lo[j] ? l2 : lo[j];
            hi[j] = h2 > hi[j] ? h2 : hi[j];
        }
    }
    for (i64 i = lane; i < n; i += kLanes) {
        series_at(a, x, b, t, i, cmax, q05, q95, v);
#pragma unroll
        for (int j = 0; j < kSeries; ++j) {
            const double d = v[j] - mean[j];
            if (j < a.nser) D[((p * a.nser + j) * a.m + k) * n + i] = d;
            q[j] = q[j] + d * d;
        }
    }
#pragma unroll
    for (int j = 0; j < kSeries; ++j) {
        const double qq = mcr::xor_tree_sum(q[j]);
        if (lane == 0 && j < a.nser) {
            double* r = mom + ((p * a.nser + j) * a.m + k) * kMomRec;
            r[0] = mean[j]; r[1] = qq; r[2] = lo[j]; r[3] = hi[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_mcs_walk: one workgroup per (parameter, series).  Thread 0 pools the chain records (pool_of) and decides whether the
// series is walked at all.  Then the lags come in blocks of MCS_LAG_BLOCK = 256, thread i taking lag base + i: chain after
// chain in chain order -- its deviations staged in LDS when n <= MCS_LDS_DRAWS, else read from D -- the thread runs
// lag_product and adds the chain's gamma_k; the pooled gamma of the block goes to LDS and thread 0 walks through it pair
// by pair (Walk).  The workgroup stops after the block in which the walk ends: a converged series costs one block, a
// series that never turns negative walks to n - 5, O(n^2) products per chain.
// out[(p nser + s) kOutRec + ..]
// ------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_mcs_walk(const double* __restrict__ D, const double* __restrict__ mom, i64 m, i64 n,
                                                       int nser, double* __restrict__ out)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double stage[];
    __shared__ double gam[MCS_LAG_BLOCK];
    __shared__ int stop;
    const i64 p = blockIdx.x;
    const int s = blockIdx.y, tid = threadIdx.x;
    const double* Ds = D + (p * nser + s) * m * n;
    const double* ms = mom + (p * nser + s) * m * kMomRec;
    double* o = out + (p * nser + s) * kOutRec;
    Pool pool{};
    Walk w{};
    if (tid == 0) {
        pool = pool_of([&](i64 k, int f) { return ms[k * kMomRec + f]; }, m, n);
        stop = (n < 4 || pool.constant) ? 1 : 0;
        if (stop) out_unwalked(pool, o);
    }
    __syncthreads();
    if (stop) return;
    for (i64 base = 0; base < n; base += MCS_LAG_BLOCK) {
        const i64 t = base + tid;
        double g = 0.0;
        for (i64 k = 0; k < m; ++k) {
            const double* d = Ds + k * n;
            if (LDS) {
                __syncthreads();                           // the chain before is read to the end
                for (i64 i = tid; i < n; i += kThreads) stage[i] = d[i];
                __syncthreads();
                d = stage;
            }
            if (t < n) g = g + lag_product(d, n, t) / (double)n;
        }
        gam[tid] = g / (double)m;
        __syncthreads();
        if (tid == 0) {
            bool ok = true;
            if (base == 0) ok = w.start(gam[0], gam[1], pool.var_means, n);
            if (!ok) {
                out_unwalked(pool, o);
                o[O_RHAT] = NAN;
                stop = 1;
            } else {
                while (!w.done && w.t + 2 < base + MCS_LAG_BLOCK) w.step(gam[w.t + 2 - base], gam[w.t + 3 - base]);
                if (w.done) {
                    out_walked(pool, w, m * n, o);
                    stop = 1;
                }
            }
        }
        __syncthreads();
        if (stop) return;
    }
}

}  // namespace mcs
