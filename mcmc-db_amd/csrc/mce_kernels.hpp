// mce_kernels.hpp -- the kernels of libmcmcref_recdf.so (include/mcmcref_recdf.h holds the definition): the per-chain
// rank-ECDF counts at K points of the pooled order, the exact (value, index) minima over the pointwise table, and the
// generator of the null sample.  Everything in front of them -- the pooled ascending order, the non-finite count -- is the
// summary pipeline's, run as one chain of M draws without diagnostics: k_mce_count reads the sort stage's keys, as
// k_hdi_window does.  All outputs are integers or table entries picked by exact comparisons, so nothing here fixes an
// order of evaluation: a parameter's bits do not depend on its place in a batch, the chunking, the chain tile or the
// loads' width.  ONE text compares two candidates on the device and on the host (before / take).
#pragma once
#include <cstdint>

#include "../../include/mcmcref_recdf.h"
#include "mcr_device.hpp"

namespace mce {

using mcr::i64;
using mcr::u64;
using mcr::kWave;

constexpr int kNT = 256;                          // threads of a workgroup of either kernel
constexpr int kMaxPoints = MCE_MAX_POINTS;

// m_k, the pooled rank of point k = 1 .. K-1 (k M < 2^41).
__host__ __device__ inline i64 point_rank(i64 k, i64 M, int K) { return k * M / K; }

// Chains of one k_mce_count workgroup.  Two bounds: the LDS histogram [chains][K] of 4-byte counters stays within
// MCE_HIST_BYTES (with the 8 KB of thresholds 32 KB: five workgroups, twenty waves, per CU), and a workgroup streams about
// MCE_SLICE_DRAWS draws (128 KB) -- long chains get a workgroup each, so that a handful of parameters still fills the chip.
__host__ __device__ inline int chain_tile(i64 C, i64 n, int K)
{
    const i64 lds = MCE_HIST_BYTES / (4 * (i64)K), sl = MCE_SLICE_DRAWS / n;
    i64 t = lds < sl ? lds : sl;
    t = t < 1 ? 1 : t;
    return (int)(t < C ? t : C);
}

// A candidate of a minimum: a table entry and where it was found.  none(): behind every entry.
struct Cand {
    double w; i64 i;
    __host__ __device__ static Cand none() { return {INFINITY, (i64)0x7FFFFFFFFFFFFFFFll}; }
};
// Whether a stands before b: the smaller entry, of two equal ones the earlier index (the FIRST k, the FIRST chain).
__host__ __device__ inline bool before(const Cand& a, const Cand& b) { return a.w < b.w || (a.w == b.w && a.i < b.i); }
__host__ __device__ inline void take(Cand& best, double w, i64 i)
{
    const Cand c{w, i};
    if (before(c, best)) best = c;
}
// |a M - n R|: n M times the distance between a chain's ECDF a / n and the pooled R / M (a <= n, R <= M: below 2^62).
__host__ __device__ inline i64 ecdf_gap(i64 a, i64 R, i64 M, i64 n)
{
    const i64 d = a * M - n * R;
    return d < 0 ? -d : d;
}

// ------------------------------------------------------------------------------------------------
// k_mce_count: one workgroup per (parameter, tile of ct chains).  grid: ceil(pc / 8) * 8 * nb, nb = ceil(C / ct),
// one-dimensional (xcd_map: a parameter's workgroups on the XCD whose L2 holds the keys the sort stage has just written).
// X[pc][M]: the draws in time order, chain c of parameter p at X + p M + c n; keys[pc][M]: their ascending order.
//   1. th[j] = keys[m_{j+1} - 1], j < K-1, padded with +inf to KP - 1 entries, KP the power of two >= K (8 KB static)
//   2. every draw of the tile's chains, chain after chain: 16-byte loads (one draw peeled where the row starts 8 bytes
//      off, at most one left over), b = #{ j : th[j] < x } by a search of log2(KP) steps that reads th[pos + s - 1] <=
//      th[KP - 2], one LDS atomic on hist[chain][b].  b <= K-1 whatever the draws are (NaN compares false; the min only
//      matters for tensors the call is about to reject, whose keys need not ascend).
//   3. a prefix over b per chain -- a wave per chain, ceil(K / 64) bins per lane -- gives a[c][k] = #{ x <= t_k } =
//      sum_{b <= k-1} hist[c][b], written to counts[(p C + c)(K-1) + k-1].
// Reads X[p M + 0 .. M-1] and keys[p M + 0 .. M-2]; dynamic LDS ct K 4 bytes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void k_mce_count(const double* __restrict__ X, const double* __restrict__ keys, i64 M, i64 n,
                                                   int C, i64 pc, int K, int ct, int nb, int32_t* __restrict__ counts)
{
    __shared__ double th[kMaxPoints];
    extern __shared__ unsigned hist[];
    i64 p;
    int blk;
    if (!mcr::xcd_map(pc, nb, p, blk)) return;
    const int tid = threadIdx.x;
    const int c0 = blk * ct, rows = (c0 + ct < C ? c0 + ct : C) - c0;
    int KP = 2;
    while (KP < K) KP <<= 1;
    const double* k = keys + p * M;
    for (int j = tid; j < KP - 1; j += kNT) th[j] = j < K - 1 ? k[point_rank(j + 1, M, K) - 1] : (double)INFINITY;
    for (int j = tid; j < rows * K; j += kNT) hist[j] = 0u;
    __syncthreads();
    for (int row = 0; row < rows; ++row) {
        const double* r = X + p * M + (i64)(c0 + row) * n;
        unsigned* h = hist + row * K;
        auto bin = [&](double x) {
            int pos = 0;
            for (int s = KP >> 1; s > 0; s >>= 1) pos += th[pos + s - 1] < x ? s : 0;
            atomicAdd(&h[pos < K - 1 ? pos : K - 1], 1u);
        };
        const i64 head = (i64)(((uintptr_t)r >> 3) & 1);           // n >= 1
        if (head && tid == kNT - 1) bin(r[0]);
        const i64 np = (n - head) >> 1;
        const double2* r2 = reinterpret_cast<const double2*>(r + head);
#pragma unroll 4
        for (i64 q = tid; q < np; q += kNT) {
            const double2 v = r2[q];
            bin(v.x);
            bin(v.y);
        }
        const i64 done = head + 2 * np;
        if (done < n && tid == 0) bin(r[done]);
    }
    __syncthreads();
    const int lane = tid & (kWave - 1), per = (K + kWave - 1) / kWave;
    for (int row = tid / kWave; row < rows; row += kNT / kWave) {
        const unsigned* h = hist + row * K;
        const int j0 = lane * per, j1 = j0 + per < K ? j0 + per : K;
        unsigned own = 0u;
        for (int j = j0; j < j1; ++j) own += h[j];
        unsigned inc = own;
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += t;
        }
        unsigned run = inc - own;
        int32_t* out = counts + (p * C + c0 + row) * (i64)(K - 1);
        for (int j = j0; j < j1; ++j) {
            run += h[j];
            if (j < K - 1) out[j] = (int32_t)run;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_mce_stat: one workgroup per parameter.  R[k] = sum_c a[c][k] (a thread per k, the chains in order: coalesced over k)
// into LDS and pooled, tied = #{ R[k] != m_k }; then a wave per chain, lane l at k = l + 1, l + 65, ..: the table entry
// U[k][a] and the gap |a M - n R[k]|, the (entry, k) minimum and the largest gap across the wave by xor shuffles; the
// chains' minima meet as (u, c) candidates across the waves through LDS.  table[(K-1)(n+1)]; counts as k_mce_count left
// them (a count outside [0, n] -- stale bytes of a rejected call -- is clamped into the table).  The outputs start at the
// chunk's first parameter; a NULL one is skipped (the null sample wants g alone).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void k_mce_stat(const int32_t* __restrict__ counts, const double* __restrict__ table, i64 M, i64 n,
                                                  int C, int K, int32_t* __restrict__ pooled, int32_t* __restrict__ tied,
                                                  double* __restrict__ u, int32_t* __restrict__ kmin, int64_t* __restrict__ dev,
                                                  double* __restrict__ g, int32_t* __restrict__ chain)
{
    constexpr int NW = kNT / kWave;
    __shared__ int32_t R[kMaxPoints];
    __shared__ Cand wbest[NW];
    __shared__ int wtied[NW];
    const i64 p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int32_t* a = counts + p * C * (i64)(K - 1);
    int nt = 0;
    for (int j = tid; j < K - 1; j += kNT) {
        i64 s = 0;
        for (int c = 0; c < C; ++c) s += a[(i64)c * (K - 1) + j];
        R[j] = (int32_t)s;
        if (pooled) pooled[p * (K - 1) + j] = (int32_t)s;
        nt += s != point_rank(j + 1, M, K) ? 1 : 0;
    }
    for (int o = kWave >> 1; o > 0; o >>= 1) nt += __shfl_xor(nt, o, kWave);
    if (lane == 0) wtied[wave] = nt;
    __syncthreads();
    Cand best = Cand::none();
    for (int c = wave; c < C; c += NW) {
        const int32_t* ac = a + (i64)c * (K - 1);
        Cand cb = Cand::none();
        i64 gap = 0;
        for (int j = lane; j < K - 1; j += kWave) {
            const i64 raw = ac[j], aj = raw < 0 ? 0 : (raw > n ? n : raw);
            take(cb, table[(i64)j * (n + 1) + aj], j + 1);
            const i64 e = ecdf_gap(aj, R[j], M, n);
            gap = e > gap ? e : gap;
        }
        for (int o = kWave >> 1; o > 0; o >>= 1) {
            const Cand t{__shfl_xor(cb.w, o, kWave), (i64)__shfl_xor((long long)cb.i, o, kWave)};
            if (before(t, cb)) cb = t;
            const i64 e = (i64)__shfl_xor((long long)gap, o, kWave);
            gap = e > gap ? e : gap;
        }
        if (lane == 0) {
            if (u) u[p * C + c] = cb.w;
            if (kmin) kmin[p * C + c] = (int32_t)cb.i;
            if (dev) dev[p * C + c] = gap;
        }
        take(best, cb.w, c);
    }
    if (lane == 0) wbest[wave] = best;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int v = 0; v < NW; ++v) {
            t += wtied[v];
            if (before(wbest[v], best)) best = wbest[v];
        }
        if (tied) tied[p] = t;
        if (g) g[p] = best.w;
        if (chain) chain[p] = (int32_t)best.i;
    }
}

// ------------------------------------------------------------------------------------------------
// k_mce_null: the simulated draws of a chunk of the null sample, X[j] = (splitmix64(base + j) >> 11) 2^-53 for j < total,
// base = seed * 0x9E3779B97F4A7C15 + s0 M (wrapping): the chunk starts at simulation s0.  X is 256-byte aligned (a carved
// buffer): two draws per 16-byte store, an odd last one alone.  Grid-stride.
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline double null_draw(u64 at) { return (double)(mcr::splitmix64(at) >> 11) * 0x1.0p-53; }

__global__ __launch_bounds__(kNT) void k_mce_null(double* __restrict__ X, i64 total, u64 base)
{
    const i64 stride = (i64)gridDim.x * kNT, np = total >> 1;
    double2* X2 = reinterpret_cast<double2*>(X);
    for (i64 q = (i64)blockIdx.x * kNT + threadIdx.x; q < np; q += stride)
        X2[q] = make_double2(null_draw(base + (u64)(2 * q)), null_draw(base + (u64)(2 * q + 1)));
    if ((total & 1) && blockIdx.x == 0 && threadIdx.x == 0) X[total - 1] = null_draw(base + (u64)(total - 1));
}

}  // namespace mce
