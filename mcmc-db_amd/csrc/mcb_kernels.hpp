// mcb_kernels.hpp -- the kernels of libmcmcref_bm.so (gfx950, wave64): k_bm_time / k_bm_tile turn draws into batch sums
// and batch means, k_bm_mean turns the batch sums into the overall mean, k_bm_pooled makes the pooled f64 copy, and
// k_bm_finish / k_bm_pool are the element-wise steps.  include/mcmcref_bm.h states what they compute; mcb_core.hpp holds
// the arithmetic they share with the host routines.  Vector stores only, no atomics, a fixed order.
#pragma once

#include <hip/hip_runtime.h>

#include "mcb_core.hpp"

namespace mcb {

constexpr int kWave = 64;
constexpr int kThreads = 256;          // k_bm_time, k_bm_mean and the element-wise kernels: four waves
constexpr int kWaves = kThreads / kWave;
constexpr int kRows = MCB_BLOCK / (2 * kWave);   // a wave's loads per lane and block: two leaves each
constexpr int kSmall = 2 * kWave;      // a batch of up to 128 leaves is one register row of a wave
constexpr int kTile = 64;              // k_bm_tile: parameters of a wave, and leaves of one step
constexpr int kTileLevels = 6;         // log2(kTile): the level of the node a step gives
static_assert(kRows == 8, "the join of the rows is written for eight");
static_assert((1 << kTileLevels) == kTile, "a step's tree has six levels");

// Leaves i and i + 1 of the n leaves at src, +0 past the end, as one load where the address is aligned for it (16 bytes
// for f64, 8 for f32).
template <class T>
__device__ __forceinline__ void load2(const T* __restrict__ src, int64_t i, int64_t n, double pivot, double& lo, double& hi);

template <>
__device__ __forceinline__ void load2<double>(const double* __restrict__ src, int64_t i, int64_t n, double pivot, double& lo, double& hi)
{
    if (i + 1 < n && ((uintptr_t)(src + i) & 15) == 0) {
        const double2 t = *reinterpret_cast<const double2*>(src + i);
        lo = leaf(t.x, pivot);
        hi = leaf(t.y, pivot);
    } else {
        lo = i < n ? leaf(src[i], pivot) : 0.0;
        hi = i + 1 < n ? leaf(src[i + 1], pivot) : 0.0;
    }
}

template <>
__device__ __forceinline__ void load2<float>(const float* __restrict__ src, int64_t i, int64_t n, double pivot, double& lo, double& hi)
{
    if (i + 1 < n && ((uintptr_t)(src + i) & 7) == 0) {
        const float2 t = *reinterpret_cast<const float2*>(src + i);
        lo = leaf(t.x, pivot);
        hi = leaf(t.y, pivot);
    } else {
        lo = i < n ? leaf(src[i], pivot) : 0.0;
        hi = i + 1 < n ? leaf(src[i + 1], pivot) : 0.0;
    }
}

// The levels 2 .. 7 of every row at once: v[r] holds a level-1 node per lane, afterwards every lane holds the level-7
// node of each row (an IEEE sum does not depend on the order of its two operands).
__device__ __forceinline__ void wave_rows(double (&v)[kRows])
{
#pragma clang fp contract(off)
    for (int o = 1; o < kWave; o <<= 1) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) v[r] = v[r] + __shfl_xor(v[r], o, kWave);
    }
}

// The levels 8 .. 10: the root of a block from its eight level-7 nodes.
__device__ __forceinline__ double join_rows(const double (&v)[kRows])
{
#pragma clang fp contract(off)
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// The tree sum of the n values term(i) by one wave; every lane returns it.  term(i, lo, hi) gives the leaves i and i + 1.
template <class Pair>
__device__ __forceinline__ double wave_tree_sum(int64_t n, int lane, Pair&& pair)
{
    double acc = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += MCB_BLOCK) {
        double v[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            double lo, hi;
            pair(b0 + r * kSmall + 2 * lane, lo, hi);
            v[r] = add(lo, hi);
        }
        wave_rows(v);
        acc = add(acc, join_rows(v));
    }
    return acc;
}

// stride_n == 1.  A wave takes the batches [seg G, (seg + 1) G) of one (p, c).  b <= 128: eight batches at a time, one per
// row; lane r stores batch r.  Otherwise a batch at a time, a block of 1024 leaves per step.  sums [Pc][A] (the chunk's
// workspace) and bm [.][ld] may each be NULL.
template <class T>
__global__ __launch_bounds__(kThreads) void k_bm_time(const T* __restrict__ x, int64_t C, int64_t N, int64_t Pc, int64_t stride_c,
                                                      int64_t stride_p, int64_t b, int64_t a, int64_t G, int64_t segs,
                                                      double* __restrict__ sums, double* __restrict__ bm, int64_t ld)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * kWaves + wave;
    if (g >= Pc * C * segs) return;
    const int64_t row = g / segs, seg = g % segs;
    const int64_t p = row / C, c = row % C;
    const int64_t n0 = N - a * b, A = C * a;
    const int64_t k0 = seg * G, k1 = k0 + G < a ? k0 + G : a;
    const double pivot = (double)x[n0 + p * stride_p];
    const T* src = x + c * stride_c + p * stride_p + n0;
    if (b <= kSmall) {
        for (int64_t kb = k0; kb < k1; kb += kRows) {
            double v[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                double lo = 0.0, hi = 0.0;
                if (kb + r < k1) load2<T>(src + (kb + r) * b, 2 * lane, b, pivot, lo, hi);
                v[r] = add(lo, hi);
            }
            wave_rows(v);
            double mine = v[0];
#pragma unroll
            for (int r = 1; r < kRows; ++r)
                if (lane == r) mine = v[r];
            const int64_t k = kb + lane;
            if (lane < kRows && k < k1) {
                const double s = add(0.0, mine);
                if (sums) sums[p * A + c * a + k] = s;
                if (bm) bm[p * ld + c * a + k] = mean_of(pivot, s, b);
            }
        }
    } else {
        for (int64_t k = k0; k < k1; ++k) {
            const T* at = src + k * b;
            const double s = wave_tree_sum(b, lane, [&](int64_t i, double& lo, double& hi) { load2<T>(at, i, b, pivot, lo, hi); });
            if (lane == 0) {
                if (sums) sums[p * A + c * a + k] = s;
                if (bm) bm[p * ld + c * a + k] = mean_of(pivot, s, b);
            }
        }
    }
}

// Any strides.  Workgroup = one wave = (64 parameters, chain c, the batches [seg G, (seg + 1) G)); lane = parameter, so a
// step's 64 loads are 64 rows of 64 consecutive parameters -- coalesced when stride_p == 1.  A step takes the leaves 64 j ..
// 64 j + 63 of the batch (+0 past its end), sums them in the fixed tree of 64 and hands the level-6 node to a binary
// counter: st[L] holds the pending node of level 6 + L, and the sixteenth node of a block completes its root.  An
// unfinished block's pending nodes are joined from the smallest up, which is the tree with +0 in the missing leaves.
template <class T>
__global__ __launch_bounds__(kTile) void k_bm_tile(const T* __restrict__ x, int64_t C, int64_t N, int64_t Pc, int64_t stride_c,
                                                   int64_t stride_n, int64_t stride_p, int64_t b, int64_t a, int64_t G,
                                                   int64_t segs, int64_t ptiles, double* __restrict__ sums,
                                                   double* __restrict__ bm, int64_t ld)
{
    int64_t w = blockIdx.x;
    const int64_t pt = w % ptiles;
    w /= ptiles;
    const int64_t seg = w % segs, c = w / segs;
    const int lane = threadIdx.x;
    const int64_t p = pt * kTile + lane;
    const bool live = p < Pc;
    const int64_t n0 = N - a * b, A = C * a;
    const int64_t k0 = seg * G, k1 = k0 + G < a ? k0 + G : a;
    const double pivot = live ? (double)x[n0 * stride_n + p * stride_p] : 0.0;
    const int64_t steps = (b + kTile - 1) / kTile;
    constexpr int kPending = kLevels - kTileLevels;             // levels 6 .. 9
    for (int64_t k = k0; k < k1; ++k) {
        const T* at = x + c * stride_c + (n0 + k * b) * stride_n + p * stride_p;
        double st[kPending] = {0.0, 0.0, 0.0, 0.0};
        double acc = 0.0;
        for (int64_t j = 0; j < steps; ++j) {
            const int64_t left = b - j * kTile;
            double t[kTile];
#pragma unroll
            for (int r = 0; r < kTile; ++r) t[r] = (live && r < left) ? leaf(at[(j * kTile + r) * stride_n], pivot) : 0.0;
#pragma unroll
            for (int s = 1; s < kTile; s <<= 1) {
#pragma unroll
                for (int i = 0; i < kTile; i += 2 * s) t[i] = add(t[i], t[i + s]);
            }
            double carry = t[0];
            const int jb = (int)(j & ((1 << kPending) - 1));
            bool placed = false;
#pragma unroll
            for (int L = 0; L < kPending; ++L) {
                if (!placed) {
                    if (jb & (1 << L)) carry = add(st[L], carry);
                    else {
                        st[L] = carry;
                        placed = true;
                    }
                }
            }
            if (!placed) acc = add(acc, carry);                 // the sixteenth node: a block's root
        }
        const int pending = (int)(steps & ((1 << kPending) - 1));
        if (pending) {
            double root = 0.0;
            bool any = false;
#pragma unroll
            for (int L = 0; L < kPending; ++L)
                if (pending & (1 << L)) {
                    root = any ? add(st[L], root) : st[L];
                    any = true;
                }
            acc = add(acc, root);
        }
        if (live) {
            if (sums) sums[p * A + c * a + k] = acc;
            if (bm) bm[p * ld + c * a + k] = mean_of(pivot, acc, b);
        }
    }
}

// mu[p] = K_p + S / (A b), S the tree sum of the parameter's A batch sums: a wave per parameter.
template <class T>
__global__ __launch_bounds__(kThreads) void k_bm_mean(const T* __restrict__ x, int64_t N, int64_t Pc, int64_t stride_n,
                                                      int64_t stride_p, int64_t b, int64_t a, int64_t A,
                                                      const double* __restrict__ sums, double* __restrict__ mu)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * kWaves + wave;
    if (p >= Pc) return;
    const double* row = sums + p * A;
    const double S = wave_tree_sum(A, lane, [&](int64_t i, double& lo, double& hi) { load2<double>(row, i, A, 0.0, lo, hi); });
    if (lane == 0) mu[p] = mean_of((double)x[(N - a * b) * stride_n + p * stride_p], S, A * b);
}

// out[p][c N + n] = (double) x[c][n][p].
template <class T>
__global__ __launch_bounds__(kThreads) void k_bm_pooled(const T* __restrict__ x, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                                                        int64_t stride_n, int64_t stride_p, double* __restrict__ out, int64_t ld)
{
    const int64_t M = C * N, total = P * M;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const int64_t p = i / M, m = i % M;
        out[p * ld + m] = (double)x[(m / N) * stride_c + (m % N) * stride_n + p * stride_p];
    }
}

__global__ __launch_bounds__(kThreads) void k_bm_finish(const double* __restrict__ cb, const double* __restrict__ cb3, int64_t n,
                                                        double f, double f3, int r, int64_t A, double* __restrict__ sigma)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        sigma[i] = finish_entry(cb[i], r == 3 ? cb3[i] : 0.0, f, f3, r, A);
}

// idx [PL] names the live parameters, s [PL] their scales.  Thread t writes entry (t / PL, t % PL) of V; a thread t < PL
// also writes d[t] and z[t], for which it computes V_tt again.
__global__ __launch_bounds__(kThreads) void k_bm_pool(const double* __restrict__ sr, const double* __restrict__ mur, double mr,
                                                      const double* __restrict__ sa, const double* __restrict__ mua, double ma,
                                                      int64_t P, int64_t PL, const int64_t* __restrict__ idx,
                                                      const double* __restrict__ s, double jitter, double* __restrict__ v,
                                                      double* __restrict__ d, double* __restrict__ z)
{
    const bool two = sa != nullptr;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < PL * PL; t += (int64_t)gridDim.x * kThreads) {
        const int64_t i = t / PL, j = t % PL;
        const int64_t e = idx[i] * P + idx[j];
        v[t] = pool_entry(s[i], s[j], sr[e], mr, two ? sa[e] : 0.0, ma, two, i == j, jitter);
        if (t < PL) {
            const int64_t q = idx[t], ee = q * P + q;
            const double vii = pool_entry(s[t], s[t], sr[ee], mr, two ? sa[ee] : 0.0, ma, two, true, jitter);
            const double dt = pool_shift(s[t], mur[q], two ? mua[q] : 0.0, two);
            d[t] = dt;
            z[t] = pool_z(dt, vii);
        }
    }
}

}  // namespace mcb
