// mcr_nested.hpp -- nested R-hat (Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari, Gelman: "Nested R-hat: assessing
// the convergence of Markov chain Monte Carlo when running many short chains"; posterior::rhat_nested): the two kernels
// behind mcr_nested_rhat.  Everything in front of them -- pooled sort, tie-averaged rank codes, fold, z table -- is the
// summary pipeline's, run as ONE chain of M = C N draws, which leaves the codes zb / zt in time order.
//
//   chain       m_c = (sum_n v[c][n]) / N            q_c = sum_n (v[c][n] - m_c)^2                    k_chain_moments
//   superchain  mu_k = (sum_{c in k} m_c) / L        b_k = sum_{c in k} (m_c - mu_k)^2   w_k = sum_{c in k} q_c
//               T_k = b_k / (L - 1) + w_k / (L (N - 1))      (a term whose divisor is 0 is 0)         k_nested_combine
//   run         mu = (sum_k mu_k) / K    B = sum_k (mu_k - mu)^2 / (K - 1)    W = (sum_k T_k) / K
//               nrhat = sqrt(1 + B / W);  W == 0: 1 when B == 0, else inf;  K < 2: NaN
//
// for three kinds of value v: the draws (raw), z of the pooled ranks (bulk), z of the ranks of |x - median| (tail).
// Every variance is two-pass (mean first, then squared deviations from it).  Every sum has ONE order, a function of the
// shape (C, N, K) alone: a parameter's results do not depend on its place in the batch, on the workspace chunking or on
// the alignment of its rows.
#pragma once
#include "mcr_device.hpp"

namespace mcr {

// ------------------------------------------------------------------------------------------------
// k_chain_moments: a wave owns a chain, four chains per workgroup.  Lane l holds the draws 128 j + 2 l and 128 j + 2 l + 1
// of every block of kNestBlock = 512 draws (j < 4): with an even N and aligned rows that is one 16-byte load of x and one
// 8-byte load of each code array per lane and j, whole lines per wave; otherwise the same two elements come as two
// loads -- the assignment of draws to lanes, and so the order of every sum, is the same.  A lane adds its draws in index
// order, block after block; the 64 lane sums meet in an xor tree (32, 16, .. 1), in which every lane gets the same bits.
// All loads of a block are issued before the first use (addresses are clamped into the row, values past the end are
// masked after the load; the pairs of a short chain's block that no lane needs are skipped, wave-uniformly), then the 16
// table reads of the two code arrays.  A chain of at most 512 draws stays in registers for the second pass; a longer one is read again, block by block (the regime is many SHORT chains).
// The z table is read by element: 2 M doubles shared by all parameters of the call, served by L2 and the Infinity Cache;
// xcd_map keeps a parameter's workgroups on one XCD.  grid: ceil(pc / 8) * 8 * ceil(C / 4), one-dimensional.
// mom[((p * 3 + kind) * C + c) * 2 + {0, 1}] = m_c, q_c;  kind 0 raw, 1 bulk, 2 tail.
// ------------------------------------------------------------------------------------------------
constexpr int kNestNT = 256, kNestChains = kNestNT / kWave;
constexpr int kNestPairs = 4;                              // pairs of draws per lane and block
constexpr int kNestElems = 2 * kNestPairs;
constexpr int kNestBlock = kWave * kNestElems;             // 512 draws: the longest chain the second pass takes from registers

// The block of a chain that starts at draw `base`: v[kind][e], e = 2 j + h <-> draw base + 128 j + 2 lane + h; 0.0 past N.
template <bool VEC>
__device__ __forceinline__ void nest_load(const double* __restrict__ x, const u32* __restrict__ zb, const u32* __restrict__ zt,
                                          const double* __restrict__ ztab, i64 M, i64 N, i64 base, int lane,
                                          double (&v)[3][kNestElems])
{
    u32 cb[kNestElems], ct[kNestElems];
    const i64 left = N - base;                             // > 0; pairs of lanes 128 j .. past it are skipped (wave-uniform)
#pragma unroll
    for (int j = 0; j < kNestPairs; ++j) {
        const i64 i = base + 2 * kWave * j + 2 * lane;
        if (2 * kWave * j >= left) {
            v[0][2 * j] = v[0][2 * j + 1] = 0.0;
            cb[2 * j] = cb[2 * j + 1] = ct[2 * j] = ct[2 * j + 1] = 0u;
        } else if constexpr (VEC) {                        // N even: i < N implies i + 1 < N; a pair past the end re-reads the last one
            const i64 a = i < N ? i : N - 2;
            const double2 xx = *reinterpret_cast<const double2*>(x + a);
            const uint2 b = *reinterpret_cast<const uint2*>(zb + a);
            const uint2 t = *reinterpret_cast<const uint2*>(zt + a);
            v[0][2 * j] = xx.x; v[0][2 * j + 1] = xx.y;
            cb[2 * j] = b.x; cb[2 * j + 1] = b.y;
            ct[2 * j] = t.x; ct[2 * j + 1] = t.y;
        } else {
            const i64 a0 = i < N ? i : N - 1, a1 = i + 1 < N ? i + 1 : N - 1;
            v[0][2 * j] = x[a0]; v[0][2 * j + 1] = x[a1];
            cb[2 * j] = zb[a0]; cb[2 * j + 1] = zb[a1];
            ct[2 * j] = zt[a0]; ct[2 * j + 1] = zt[a1];
        }
    }
#pragma unroll
    for (int e = 0; e < kNestElems; ++e) {
        const bool skip = 2 * kWave * (e >> 1) >= left;
        v[1][e] = skip ? 0.0 : zdec(ztab, cb[e], M);
        v[2][e] = skip ? 0.0 : zdec(ztab, ct[e], M);
    }
#pragma unroll
    for (int e = 0; e < kNestElems; ++e) {
        const bool live = base + 2 * kWave * (e >> 1) + 2 * lane + (e & 1) < N;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k][e] = live ? v[k][e] : 0.0;
    }
}

template <bool VEC>
__device__ __forceinline__ void nest_chain(const double* __restrict__ x, const u32* __restrict__ zb, const u32* __restrict__ zt,
                                           const double* __restrict__ ztab, i64 M, i64 N, int lane, double (&m)[3], double (&q)[3])
{
    double v[3][kNestElems];
    const i64 nblk = (N + kNestBlock - 1) / kNestBlock;
    double s[3] = {0.0, 0.0, 0.0};
    for (i64 b = 0; b < nblk; ++b) {
        nest_load<VEC>(x, zb, zt, ztab, M, N, b * kNestBlock, lane, v);
#pragma unroll
        for (int e = 0; e < kNestElems; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += v[k][e];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { m[k] = xor_tree_sum(s[k]) / (double)N; q[k] = 0.0; }
    for (i64 b = 0; b < nblk; ++b) {
        if (nblk > 1) nest_load<VEC>(x, zb, zt, ztab, M, N, b * kNestBlock, lane, v);     // one block: still in registers
#pragma unroll
        for (int e = 0; e < kNestElems; ++e) {
            const bool live = b * kNestBlock + 2 * kWave * (e >> 1) + 2 * lane + (e & 1) < N;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double d = live ? v[k][e] - m[k] : 0.0;
                q[k] = fma(d, d, q[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = xor_tree_sum(q[k]);
}

__global__ __launch_bounds__(kNestNT) void k_chain_moments(const double* __restrict__ X, const u32* __restrict__ zb,
                                                           const u32* __restrict__ zt, const double* __restrict__ ztab,
                                                           i64 M, i64 C, i64 N, i64 pc, double* __restrict__ mom)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    i64 p;
    int blk;
    if (!xcd_map(pc, (int)((C + kNestChains - 1) / kNestChains), p, blk)) return;
    const i64 c = (i64)blk * kNestChains + wave;
    if (c >= C) return;                                    // (no workgroup barrier below: the waves are independent)
    const i64 row = p * M + c * N;                         // M = C N: the chains of a parameter lie back to back
    const double* x = X + row;
    const u32 *b = zb + row, *t = zt + row;
    const bool vec = (N & 1) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(t) & 7) == 0;
    double m[3], q[3];
    if (vec) nest_chain<true>(x, b, t, ztab, M, N, lane, m, q);
    else nest_chain<false>(x, b, t, ztab, M, N, lane, m, q);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            *reinterpret_cast<double2*>(mom + ((p * 3 + k) * C + c) * 2) = make_double2(m[k], q[k]);
    }
}

// ------------------------------------------------------------------------------------------------
// k_nested_combine: one workgroup per (parameter, kind).  perm lists the chains superchain after superchain (K runs of
// L chains, the host's stable order), so superchain k owns perm[k L .. k L + L).
//  1. A group of G lanes (the power of two >= min(L, 64)) owns a superchain, 64 / G superchains per wave at a time:
//     lane s of the group adds the chains s, s + G, .. in order, the group sums in an xor tree of width G.  Two passes
//     (mu_k, then b_k and w_k); sup[k] = (mu_k, T_k) goes to the workgroup's scratch in global memory.
//  2. Thread t adds the superchains t, t + 256, .. in order and the workgroup sums with block_sum (fixed shape): mu and
//     W, then B from the deviations mu_k - mu.
// res[(field0 + 3 kind + {0, 1, 2}) * pc + p] = nrhat, B, W.
// ------------------------------------------------------------------------------------------------
constexpr int kNestCombNT = 256;

__global__ __launch_bounds__(kNestCombNT) void k_nested_combine(const double* __restrict__ mom, const int* __restrict__ perm,
                                                                i64 C, i64 K, i64 L, i64 N, double* sup,
                                                                double* __restrict__ res, i64 pc, int field0)
{
    __shared__ double red[3 * kNestCombNT / kWave];
    const i64 p = blockIdx.x;
    const int kind = blockIdx.y, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const double2* mc = reinterpret_cast<const double2*>(mom) + (p * 3 + kind) * C;
    double2* sk = reinterpret_cast<double2*>(sup) + (p * 3 + kind) * K;
    int G = 1;
    while (G < kWave && G < L) G <<= 1;
    const int per = kWave / G, sub = lane & (G - 1);
    const i64 step = (i64)(kNestCombNT / kWave) * per;
    for (i64 k0 = 0; k0 < K; k0 += step) {                 // (uniform over the workgroup: every lane reaches the shuffles)
        const i64 k = k0 + (i64)wave * per + lane / G;
        const bool own = k < K;
        const int* pk = perm + k * L;
        double s = 0.0;
        if (own) for (i64 j = sub; j < L; j += G) s += mc[pk[j]].x;
        const double mu = xor_tree_sum(s, G) / (double)L;
        double b = 0.0, w = 0.0;
        if (own) for (i64 j = sub; j < L; j += G) {
            const double2 r = mc[pk[j]];
            const double d = r.x - mu;
            b = fma(d, d, b);
            w += r.y;
        }
        b = xor_tree_sum(b, G);
        w = xor_tree_sum(w, G);
        if (own && sub == 0) {
            const double tb = L > 1 ? b / (double)(L - 1) : 0.0;
            const double tw = N > 1 ? w / ((double)L * (double)(N - 1)) : 0.0;
            sk[k] = make_double2(mu, tb + tw);
        }
    }
    __threadfence_block();
    __syncthreads();
    double smu = 0.0, st = 0.0, zero = 0.0;
    for (i64 k = tid; k < K; k += kNestCombNT) { const double2 r = sk[k]; smu += r.x; st += r.y; }
    block_sum3<kNestCombNT>(smu, st, zero, red);
    const double mu = smu / (double)K, W = st / (double)K;
    double sb = 0.0;
    for (i64 k = tid; k < K; k += kNestCombNT) { const double d = sk[k].x - mu; sb = fma(d, d, sb); }
    sb = block_sum<kNestCombNT>(sb, red);
    if (tid == 0) {
        const double B = K >= 2 ? sb / (double)(K - 1) : NAN;
        double r;
        if (K < 2) r = NAN;
        else if (W == 0.0) r = (B == 0.0) ? 1.0 : INFINITY;
        else r = sqrt(1.0 + B / W);
        double* o = res + (i64)(field0 + 3 * kind) * pc + p;
        o[0] = r; o[pc] = B; o[2 * pc] = W;
    }
}

}  // namespace mcr
