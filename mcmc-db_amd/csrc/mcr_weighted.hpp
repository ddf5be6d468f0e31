// mcr_weighted.hpp -- importance-weighted summaries: mean, sd, the standard error of the mean and quantiles of every
// parameter under ONE weight vector shared by all of them (posterior::weight_draws + summarise_draws, loo::E_loo,
// numpy.quantile(weights=, method="inverted_cdf")).  The definition is in mcmcref_hip.h.  The pooled ascending order and
// the non-finite count are the summary pipeline's, run without diagnostics; the moments run in TIME order on the draws
// as they are (streaming, coalesced), and only the cumulative-weight search runs in the sorted order, through the gather
// w[pos[j]] of the sort stage's positions.
//
// Every sum has the ONE association of mcr_tree.hpp: balanced trees over blocks of kWgtBlock = 1024 consecutive indices,
// the blocks added in ascending order from +0.
#pragma once
#include "mcr_tree.hpp"

namespace mcr {

constexpr int kWgtMaxQ = 16;                  // MCR_WEIGHTED_MAX_Q: probabilities of a call
constexpr int kWgtNT = 256;                   // threads of k_weighted_moments and k_wq_pick
constexpr int kWgtSlice = 16;                 // blocks of a k_weighted_moments workgroup (four per wave)
constexpr int kWgtPrepNT = 1024;              // threads of the one k_weight_prepare workgroup
constexpr int kWgtTree = kWgtBlock / 4 * 2;   // doubles of k_wq_pick's tree in LDS: the nodes of levels 2 .. 10 (511)

// The call's totals, prepared once (k_weight_prepare)
enum WgtTotal { WT_BAD = 0, WT_MAX, WT_S1, WT_S2, kWgtTotals };
// A parameter's rows in the result table, behind the pipeline's; the quantiles follow
enum WgtRow { WR_MEAN = 0, WR_SD, WR_SE, WR_Q0 };

// The probabilities of a call (by value: no upload)
struct WgtArgs {
    int nq;
    double q[kWgtMaxQ];
};

// Whether v cannot be a weight: linear weights are finite and >= 0, log weights are finite or -inf.
__host__ __device__ inline bool wgt_bad(double v, int log)
{
    return log ? !(v < INFINITY) : !(v >= 0.0 && v < INFINITY);
}
// The weight of v: exp(v - vmax) of a log weight (-inf: 0), v itself otherwise.
__host__ __device__ inline double wgt_weight(double v, int log, double vmax) { return log ? exp(v - vmax) : v; }

// The terms of the sums.  Every product is rounded on its own.
__host__ __device__ inline double wgt_sq(double w)
{
#pragma clang fp contract(off)
    return w * w;
}
__host__ __device__ inline double wgt_wx(double w, double x)
{
#pragma clang fp contract(off)
    return w * x;
}
// d = x - mean, a = w d: a d (for sum w d^2) and a a (for sum w^2 d^2)
__host__ __device__ inline void wgt_dev2(double w, double x, double mean, double& t1, double& t2)
{
#pragma clang fp contract(off)
    const double d = x - mean, a = w * d;
    t1 = a * d;
    t2 = a * a;
}
// Whether a cumulative weight answers the threshold t = q * total: numpy's inverted_cdf, which never stops on a leading
// run of zero weights.
__host__ __device__ inline bool wgt_reached(double cum, double t) { return cum >= t && cum > 0.0; }

// t = q * total: one rounded product.
__host__ __device__ inline double wgt_threshold(double q, double total)
{
#pragma clang fp contract(off)
    return q * total;
}

// The first block b of nb whose prefix reaches q * total, total the prefix of all (ascending from +0); prev: the prefix in
// front of b.  -1 when none does (NaN sums).
template <class Sum>
__host__ __device__ inline i64 wgt_find_block(const Sum& sum, i64 nb, double q, double& t, double& prev)
{
#pragma clang fp contract(off)
    double total = 0.0;
    for (i64 b = 0; b < nb; ++b) total = total + sum(b);
    t = wgt_threshold(q, total);
    double acc = 0.0;
    for (i64 b = 0; b < nb; ++b) {
        const double nxt = acc + sum(b);
        if (wgt_reached(nxt, t)) { prev = acc; return b; }
        acc = nxt;
    }
    prev = acc;
    return -1;
}

// ------------------------------------------------------------------------------------------------
// k_weight_prepare: ONE workgroup of 1024 threads, once per call.  Phase 1: the count of entries that cannot be weights
// and, for log weights, the maximum (exact whatever the order).  A bad entry, or no entry above -inf, ends the kernel:
// tot = (bad, max, 0, 0), nothing else is written.  Phase 2: wave k takes the blocks k, k + 16, ...: w[m] = wgt_weight(v[m])
// and the block's sums of w and w^2 by the tree, bs[b] and bs[nb + b].  Phase 3: the waves 0 and 1 add the block sums in
// ascending order into tot[WT_S1], tot[WT_S2] (wgt_wave_serial).  v is read by 8-byte loads (a caller's device pointer:
// any alignment); reads v[0 .. M) and writes w[0 .. M), bs[0 .. 2 nb), tot[0 .. kWgtTotals) only.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWgtPrepNT) void k_weight_prepare(const double* __restrict__ v, i64 M, int log,
                                                               double* __restrict__ w, double* bs, double* __restrict__ tot)
{
    __shared__ double sh_max[kWgtPrepNT / kWave];
    __shared__ double sh_bad[kWgtPrepNT / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const i64 nb = wgt_blocks(M);
    double bad = 0.0, vmax = -INFINITY;
    for (i64 m0 = tid; m0 < M; m0 += 8 * kWgtPrepNT) {       // eight loads in flight per lane
        double x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = m0 + k * kWgtPrepNT < M ? v[m0 + k * kWgtPrepNT] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (m0 + k * kWgtPrepNT >= M) continue;
            if (wgt_bad(x[k], log)) bad += 1.0;
            else if (x[k] > vmax) vmax = x[k];
        }
    }
    for (int o = kWave >> 1; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o, kWave);
        const double y = __shfl_xor(vmax, o, kWave);
        if (y > vmax) vmax = y;
    }
    if (lane == 0) { sh_bad[wave] = bad; sh_max[wave] = vmax; }
    __syncthreads();
    bad = 0.0; vmax = -INFINITY;
    for (int k = 0; k < kWgtPrepNT / kWave; ++k) {           // (counts below 2^53: exact in any order)
        bad += sh_bad[k];
        if (sh_max[k] > vmax) vmax = sh_max[k];
    }
    if (bad > 0.0 || (log && !(vmax > -INFINITY))) {         // (uniform over the workgroup)
        if (tid == 0) { tot[WT_BAD] = bad; tot[WT_MAX] = vmax; tot[WT_S1] = 0.0; tot[WT_S2] = 0.0; }
        return;
    }
    for (i64 b = wave; b < nb; b += kWgtPrepNT / kWave) {
        double s1[kWgtRows], s2[kWgtRows];
#pragma unroll
        for (int r = 0; r < kWgtRows; ++r) {
            const i64 i = b * kWgtBlock + 2 * kWave * r + 2 * lane;
            const double a = i < M ? wgt_weight(v[i], log, vmax) : 0.0;
            const double c = i + 1 < M ? wgt_weight(v[i + 1], log, vmax) : 0.0;
            if (i < M) w[i] = a;
            if (i + 1 < M) w[i + 1] = c;
            s1[r] = wgt_add(a, c);
            s2[r] = wgt_add(wgt_sq(a), wgt_sq(c));
        }
        const double r1 = wgt_wave_root(s1), r2 = wgt_wave_root(s2);
        if (lane == 0) { bs[b] = r1; bs[nb + b] = r2; }
    }
    __threadfence_block();
    __syncthreads();
    if (wave < 2) {                                          // (one wave each: S1 and S2)
        const double S = wgt_wave_serial(bs + wave * nb, nb, lane);
        if (lane == 0) tot[wave ? WT_S2 : WT_S1] = S;
        if (tid == 0) { tot[WT_BAD] = 0.0; tot[WT_MAX] = vmax; }
    }
}

// ------------------------------------------------------------------------------------------------
// k_weighted_moments<PASS>: one workgroup per (parameter, slice of kWgtSlice blocks) in TIME order; grid: ceil(pc / 8) * 8 *
// nsl, one-dimensional (xcd_map), nsl = ceil(nb / kWgtSlice).  A wave owns a block at a time: per lane eight pairs of
// draws and eight pairs of weights, by 16-byte loads where the row X[p] is 16-byte aligned (w always is) and by 8-byte
// loads otherwise; the pair sums meet by wgt_wave_root.  No LDS, no barrier, no atomics.
// PASS 1: part[p * nb + b] = the block's sum of w x.  PASS 2: part[p * nb + b] and part[(pc + p) * nb + b] = its sums of w d^2
// and w^2 d^2, d = x - mean[p].  Reads X[p * M + 0 .. M-1] and w[0 .. M-1] only.
// ------------------------------------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(kWgtNT) void k_weighted_moments(const double* __restrict__ X, const double* __restrict__ w, i64 M,
                                                             i64 pc, const double* __restrict__ mean, double* __restrict__ part)
{
    const i64 nb = wgt_blocks(M);
    const int nsl = (int)((nb + kWgtSlice - 1) / kWgtSlice);
    i64 p;
    int s;
    if (!xcd_map(pc, nsl, p, s)) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const double* x = X + p * M;
    const bool wide_x = (reinterpret_cast<uintptr_t>(x) & 15) == 0, wide_w = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    const double m = PASS == 2 ? mean[p] : 0.0;
    const i64 b1 = ((i64)s + 1) * kWgtSlice < nb ? ((i64)s + 1) * kWgtSlice : nb;
    for (i64 b = (i64)s * kWgtSlice + wave; b < b1; b += kWgtNT / kWave) {
        double xa[kWgtRows], xb[kWgtRows], wa[kWgtRows], wb[kWgtRows];
#pragma unroll
        for (int r = 0; r < kWgtRows; ++r) {
            const i64 i = b * kWgtBlock + 2 * kWave * r + 2 * lane;
            wgt_load2(x, i, M, wide_x, xa[r], xb[r]);
            wgt_load2(w, i, M, wide_w, wa[r], wb[r]);
        }
        double s1[kWgtRows], s2[kWgtRows];
#pragma unroll
        for (int r = 0; r < kWgtRows; ++r) {
            const i64 i = b * kWgtBlock + 2 * kWave * r + 2 * lane;
            if (PASS == 1) {
                s1[r] = wgt_add(i < M ? wgt_wx(wa[r], xa[r]) : 0.0, i + 1 < M ? wgt_wx(wb[r], xb[r]) : 0.0);
            } else {
                double a1 = 0.0, a2 = 0.0, c1 = 0.0, c2 = 0.0;
                if (i < M) wgt_dev2(wa[r], xa[r], m, a1, a2);
                if (i + 1 < M) wgt_dev2(wb[r], xb[r], m, c1, c2);
                s1[r] = wgt_add(a1, c1);
                s2[r] = wgt_add(a2, c2);
            }
        }
        const double r1 = wgt_wave_root(s1);
        if (PASS == 1) {
            if (lane == 0) part[p * nb + b] = r1;
        } else {
            const double r2 = wgt_wave_root(s2);
            if (lane == 0) { part[p * nb + b] = r1; part[(pc + p) * nb + b] = r2; }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_weighted_combine<PASS>: one wave per parameter adds its block sums in ascending order (wgt_wave_serial); grid: pc.
// PASS 1: mean[p] = sum / S1.  PASS 2: mean, sd = sqrt(Q1 / S1) and mean_se = sqrt(Q2) / S1 into
// res[(field0 + WgtRow) * pc + p].
// ------------------------------------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(kWave) void k_weighted_combine(const double* __restrict__ part, i64 nb, i64 pc,
                                                            const double* __restrict__ tot, double* __restrict__ mean,
                                                            double* __restrict__ res, int field0)
{
    const i64 p = blockIdx.x;
    const int lane = threadIdx.x;
    const double S1 = tot[WT_S1];
    const double s = wgt_wave_serial(part + p * nb, nb, lane);
    if (PASS == 1) {
        if (lane == 0) mean[p] = s / S1;
    } else {
        const double q2 = wgt_wave_serial(part + (pc + p) * nb, nb, lane);
        if (lane == 0) {
            res[(i64)(field0 + WR_MEAN) * pc + p] = mean[p];
            res[(i64)(field0 + WR_SD) * pc + p] = sqrt(s / S1);
            res[(i64)(field0 + WR_SE) * pc + p] = sqrt(q2) / S1;
        }
    }
}

// The weight of sorted index j of a parameter: w at the draw's pooled position; +0 past the end (and for a position
// outside the column, which the sort never writes).
template <typename IdxT>
__device__ __forceinline__ double wgt_gather(const IdxT* __restrict__ ps, const double* __restrict__ w, i64 j, i64 M)
{
    if (j >= M) return 0.0;
    const i64 at = (i64)ps[j];
    return at < M ? w[at] : 0.0;
}

// ------------------------------------------------------------------------------------------------
// k_wq_blocks: one workgroup of ONE wave per (parameter, block of kWgtBlock sorted indices); grid: ceil(pc / 8) * 8 * nb,
// one-dimensional (xcd_map: a parameter's workgroups on the XCD whose L2 holds the positions the sort stage has just
// written; the 8 M bytes of w are shared by every parameter and stay in each L2 up to about half a million draws).
// Consecutive lanes read consecutive pairs of positions; the 16 gathers of a lane are in flight together.
// qb[p * nb + b] = the block's sum of u_j = w[pos[j]] by the tree.  IdxT: the sort's position width.
// ------------------------------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(kWave) void k_wq_blocks(const IdxT* __restrict__ pos, const double* __restrict__ w, i64 M, i64 pc,
                                                     double* __restrict__ qb)
{
    const i64 nb = wgt_blocks(M);
    i64 p;
    int b;
    if (!xcd_map(pc, (int)nb, p, b)) return;
    const int lane = threadIdx.x;
    const IdxT* ps = pos + p * M;
    double u[kWgtRows], v[kWgtRows];
#pragma unroll
    for (int r = 0; r < kWgtRows; ++r) {
        const i64 j = (i64)b * kWgtBlock + 2 * kWave * r + 2 * lane;
        u[r] = wgt_gather(ps, w, j, M);
        v[r] = wgt_gather(ps, w, j + 1, M);
    }
#pragma unroll
    for (int r = 0; r < kWgtRows; ++r) u[r] = wgt_add(u[r], v[r]);
    const double root = wgt_wave_root(u);
    if (lane == 0) qb[p * nb + b] = root;
}

// The tree of k_wq_pick's block: thread t holds the leaves 4 t .. 4 t + 3 and their nodes of levels 1 and 2; the levels
// 2 .. 10 lie in LDS, level L at wgt_level_at(L).  A thread asks only for nodes over or in front of its own leaves.
__host__ __device__ constexpr int wgt_level_at(int L) { return 2 * (kWgtBlock / 4) - (2 * kWgtBlock >> L); }
struct WgtPickNode {
    const double* tree;       // LDS
    int t;                    // the thread
    double l[4], l01, l23;
    __device__ double operator()(int L, int i) const
    {
        if (L >= 2) return tree[wgt_level_at(L) + i];
        if (L == 1) return (i & 1) ? l23 : l01;
        const int e = i - 4 * t;                               // (selects: no indexed register array)
        return e == 0 ? l[0] : e == 1 ? l[1] : e == 2 ? l[2] : l[3];
    }
};

// ------------------------------------------------------------------------------------------------
// k_wq_pick: one workgroup per parameter; grid: ceil(pc / 8) * 8 (xcd_map).  The first wave adds the parameter's block
// sums in ascending order (wgt_wave_serial), lane k < nq forms t = q_k * total and keeps the first block whose prefix
// reaches it: wgt_find_block's additions and comparisons.  Then, one probability after the other, the workgroup forms that one block's tree again -- the gathers and sums of k_wq_blocks:
// the same bits -- and every thread the in-block prefixes of its four leaves (wgt_prefix); the first index j with
// wgt_reached(prev + prefix_j, t) gives x_(j) into res[(field0 + k) * pc + p].  NaN where no block reaches t (NaN sums).
// Static LDS: 4 KB of tree nodes.  Reads keys, pos [p * M + 0 .. M-1], w[0 .. M-1], qb[p * nb + 0 .. nb-1] only.
// ------------------------------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(kWgtNT) void k_wq_pick(const double* __restrict__ keys, const IdxT* __restrict__ pos,
                                                    const double* __restrict__ w, i64 M, i64 pc, WgtArgs a,
                                                    const double* __restrict__ qb, double* __restrict__ res, int field0)
{
    __shared__ double tree[kWgtTree];
    __shared__ i64 sh_b[kWgtMaxQ];
    __shared__ double sh_t[kWgtMaxQ], sh_prev[kWgtMaxQ];
    __shared__ int sh_first;
    const i64 nb = wgt_blocks(M);
    i64 p;
    int blk;
    if (!xcd_map(pc, 1, p, blk)) return;
    const int tid = threadIdx.x;
    if (tid < kWave) {                                       // wgt_find_block's additions, by the first wave for every q at once
        const double* sums = qb + p * nb;
        double q = 0.0;
        for (int k = 0; k < a.nq; ++k) if (k == tid) q = a.q[k];        // (no indexed read of the argument)
        const double t = wgt_threshold(q, wgt_wave_serial(sums, nb, tid));
        i64 bsel = -1;
        double prev = 0.0;
        wgt_wave_serial(sums, nb, tid, [&](i64 b, double acc, double nxt) {
            if (bsel < 0 && wgt_reached(nxt, t)) { bsel = b; prev = acc; }
        });
        if (tid < a.nq) { sh_b[tid] = bsel; sh_t[tid] = t; sh_prev[tid] = prev; }
    }
    __syncthreads();
    const IdxT* ps = pos + p * M;
    for (int k = 0; k < a.nq; ++k) {
        const i64 b = sh_b[k];                                 // (uniform over the workgroup)
        double* out = res + (i64)(field0 + k) * pc + p;
        if (b < 0) { if (tid == 0) *out = NAN; continue; }
        WgtPickNode nd;
        nd.tree = tree; nd.t = tid;
#pragma unroll
        for (int e = 0; e < 4; ++e) nd.l[e] = wgt_gather(ps, w, b * kWgtBlock + 4 * tid + e, M);
        nd.l01 = wgt_add(nd.l[0], nd.l[1]);
        nd.l23 = wgt_add(nd.l[2], nd.l[3]);
        tree[tid] = wgt_add(nd.l01, nd.l23);                   // level 2
        if (tid == 0) sh_first = kWgtBlock;
        __syncthreads();
        for (int L = 3; L <= kWgtLevels; ++L) {
            const int n = kWgtBlock >> L;
            if (tid < n) {
                const double* lo = tree + wgt_level_at(L - 1) + 2 * tid;
                tree[wgt_level_at(L) + tid] = wgt_add(lo[0], lo[1]);
            }
            __syncthreads();
        }
        const double t = sh_t[k], prev = sh_prev[k];
        int first = kWgtBlock;
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            const int i = 4 * tid + e;
            if (b * kWgtBlock + i < M && wgt_reached(wgt_add(prev, wgt_prefix(nd, i + 1)), t)) first = i;
        }
        if (first < kWgtBlock) atomicMin(&sh_first, first);
        __syncthreads();
        if (tid == 0) *out = sh_first < kWgtBlock ? keys[p * M + b * kWgtBlock + sh_first] : NAN;
        __syncthreads();                                       // (the tree and sh_first are written again)
    }
}

}  // namespace mcr
