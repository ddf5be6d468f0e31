// mci_kernels.hpp -- the two kernels of libmcmcref_iess.so (gfx950, wave64): k_pack_time / k_pack_tile turn draws into
// bit-packed indicator chains, k_lag turns those into ESS, truncation lag and count.  include/mcmcref_iess.h states what
// they compute; mci_core.hpp holds the arithmetic they share with the host routine.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "mci_core.hpp"

namespace mci {

constexpr int kThreads = 256;          // every kernel's workgroup: four waves
constexpr int kWaves = kThreads / 64;
constexpr int kPackWords = 8;          // words (of 64 draws) a wave of k_pack_time packs: eight loads in flight per lane
constexpr int kTile = 64;              // k_pack_tile: parameters x draws of the staged tile

static_assert(MCI_LAG_BLOCK == kThreads, "one lag per thread");
static_assert(MCI_MAX_REQUESTS <= 64, "a lane per request keeps the ballot of its request");

// bits[((p K + k) C + c) Wp + w], Wp = ceil(N / 64) + 1: the last word of a chain and the bits past N are zero.
__device__ inline int64_t word_index(int64_t p, int K, int k, int64_t C, int64_t c, int64_t Wp, int64_t w)
{
    return ((p * K + k) * C + c) * Wp + w;
}

// stride_n == 1.  Workgroup = (row p, c; segment of kWaves * kPackWords words); a wave takes 64 consecutive draws per word
// and one ballot per request; lane k keeps the ballot of request k and stores it.
template <class T>
__global__ __launch_bounds__(kThreads) void k_pack_time(const T* __restrict__ x, int64_t C, int64_t N, int64_t stride_c,
                                                        int64_t stride_p, const double* __restrict__ lower,
                                                        const double* __restrict__ upper, int K, int64_t Wp,
                                                        int64_t segments, uint64_t* __restrict__ bits)
{
    const int64_t row = (int64_t)blockIdx.x / segments, seg = (int64_t)blockIdx.x % segments;
    const int64_t p = row / C, c = row % C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* src = x + c * stride_c + p * stride_p;
    const int64_t w0 = (seg * kWaves + wave) * kPackWords;
    double v[kPackWords];
    bool in[kPackWords];
#pragma unroll
    for (int i = 0; i < kPackWords; ++i) {
        const int64_t t = (w0 + i) * 64 + lane;
        in[i] = w0 + i < Wp && t < N;
        v[i] = in[i] ? (double)src[t] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kPackWords; ++i) {
        if (w0 + i >= Wp) break;                                   // (uniform over the wave)
        uint64_t mine = 0;
        for (int k = 0; k < K; ++k) {
            const double lo = lower[p * K + k], hi = upper[p * K + k];
            const uint64_t m = __ballot(in[i] && lo < v[i] && v[i] <= hi);
            if (lane == k) mine = m;
        }
        if (lane < K) bits[word_index(p, K, lane, C, c, Wp, w0 + i)] = mine;
    }
}

// Any strides.  Workgroup = (64 parameters, chain c, word w): the tile [draw][parameter] goes through LDS -- rows are
// coalesced when stride_p == 1 -- and lane = parameter builds the word of each request from its LDS column (a lane per
// 8-byte bank pair: no conflict); the waves share the requests.  A draw past N or a parameter past P reads as NaN,
// which compares false.
template <class T>
__global__ __launch_bounds__(kThreads) void k_pack_tile(const T* __restrict__ x, int64_t C, int64_t N, int64_t P,
                                                        int64_t stride_c, int64_t stride_n, int64_t stride_p,
                                                        const double* __restrict__ lower, const double* __restrict__ upper,
                                                        int K, int64_t Wp, int64_t ptiles, uint64_t* __restrict__ bits)
{
    __shared__ double tile[kTile][kTile];
    int64_t b = blockIdx.x;
    const int64_t pt = b % ptiles;
    b /= ptiles;
    const int64_t w = b % Wp, c = b / Wp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = pt * kTile + lane;
    for (int r = wave; r < kTile; r += kWaves) {
        const int64_t t = w * 64 + r;
        tile[r][lane] = (p < P && t < N) ? (double)x[c * stride_c + t * stride_n + p * stride_p] : (double)NAN;
    }
    __syncthreads();
    if (p >= P) return;
    for (int k = wave; k < K; k += kWaves) {
        const double lo = lower[p * K + k], hi = upper[p * K + k];
        uint64_t word = 0;
#pragma unroll 8
        for (int r = 0; r < kTile; ++r) {
            const double v = tile[r][lane];
            word |= (uint64_t)(lo < v && v <= hi) << r;
        }
        bits[word_index(p, K, k, C, c, Wp, w)] = word;
    }
}

// One workgroup per (parameter, request).  kLds: the C * Wp words and their running popcounts live in LDS (C * Wp <=
// MCI_LDS_WORDS), in the launch's dynamic allocation of lds_bytes(C * Wp) so that short chains leave room for several
// workgroups per CU; otherwise the words are read from `bits` and the popcounts kept in `gpre`, both global.
inline size_t lds_bytes(int64_t words) { return (size_t)words * (sizeof(uint64_t) + sizeof(uint32_t)); }

template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_lag(const uint64_t* __restrict__ bits, uint32_t* __restrict__ gpre, int64_t C,
                                                  int64_t N, int64_t Wp, double* __restrict__ ess,
                                                  int64_t* __restrict__ trunc, int64_t* __restrict__ ones)
{
    extern __shared__ uint64_t s_dyn[];
    __shared__ double s_t[MCI_LAG_BLOCK];
    __shared__ uint32_t s_scan[kThreads];
    __shared__ unsigned long long s_sum[3];
    __shared__ int s_first;

    const int tid = threadIdx.x;
    const int64_t total = C * Wp, W = Wp - 1, n = N, m = C;
    const int64_t pk = blockIdx.x;
    uint64_t* s_bits = s_dyn;
    uint32_t* s_pre = (uint32_t*)(s_dyn + total);
    const uint64_t* gB = bits + pk * total;
    const uint64_t* B = kLds ? s_bits : gB;
    uint32_t* pre = kLds ? s_pre : gpre + pk * total;
    if (kLds) {
        for (int64_t i = tid; i < total; i += kThreads) s_bits[i] = gB[i];
    }
    if (tid < 3) s_sum[tid] = 0;
    __syncthreads();

    // pre[i] = the ones of the words before i, over all chains in a row: a segment per thread, a scan of the segments
    const int64_t seg = (total + kThreads - 1) / kThreads;
    const int64_t i0 = tid * seg < total ? tid * seg : total, i1 = i0 + seg < total ? i0 + seg : total;
    uint32_t mine = 0;
    for (int64_t i = i0; i < i1; ++i) mine += (uint32_t)__builtin_popcountll(B[i]);
    s_scan[tid] = mine;
    __syncthreads();
    for (int s = 1; s < kThreads; s <<= 1) {
        const uint32_t add = tid >= s ? s_scan[tid - s] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    uint32_t run = s_scan[tid] - mine;
    for (int64_t i = i0; i < i1; ++i) {
        pre[i] = run;
        run += (uint32_t)__builtin_popcountll(B[i]);
    }
    __syncthreads();

    // the integer sums over the chains
    unsigned long long ks = 0, wn = 0, k2 = 0;
    for (int64_t c = tid; c < C; c += kThreads) {
        const unsigned long long k = pre[c * Wp + W] - pre[c * Wp];
        ks += k;
        wn += k * ((unsigned long long)n - k);
        k2 += k * k;
    }
    if (ks) atomicAdd(&s_sum[0], ks);
    if (wn) atomicAdd(&s_sum[1], wn);
    if (k2) atomicAdd(&s_sum[2], k2);
    __syncthreads();
    const int64_t ksum = (int64_t)s_sum[0], wnum = (int64_t)s_sum[1];
    const int64_t q = m * (int64_t)s_sum[2] - ksum * ksum;

    double out_ess;
    int64_t out_trunc;
    const double vh = n >= 2 ? var_hat(wnum, q, n, m) : 0.0;
    if (n < 2) {
        out_ess = (double)NAN;
        out_trunc = -1;
    } else if (vh == 0.0) {
        out_ess = (double)m * (double)n;
        out_trunc = 0;
    } else {
        double R = 0.0;
        out_trunc = n;
        for (int64_t base = 1; base <= n - 1; base += MCI_LAG_BLOCK) {
            const int64_t lag = base + tid;
            const bool live = lag <= n - 1;
            Wide A{0, 0};
            if (live) {
                const int64_t qw = lag >> 6, jh = n - lag;
                const int r = (int)(lag & 63);
                for (int64_t c = 0; c < C; ++c) {
                    const uint64_t* Bc = B + c * Wp;
                    const uint32_t* pc = pre + c * Wp;
                    int64_t S = 0;
                    uint64_t cur = Bc[qw];
                    for (int64_t w = 0; w + qw < W; ++w) {
                        const uint64_t nxt = Bc[w + qw + 1];
                        S += __builtin_popcountll(Bc[w] & funnel(cur, nxt, r));
                        cur = nxt;
                    }
                    const uint32_t p0 = pc[0];
                    const int64_t k = (int64_t)(pc[W] - p0);
                    const int64_t H = prefix_ones(pc[jh >> 6] - p0, Bc[jh >> 6], jh);
                    const int64_t T = k - prefix_ones(pc[qw] - p0, Bc[qw], lag);
                    A = wide_add(A, chain_a(n, lag, k, S, H, T));
                }
            }
            if (tid == 0) s_first = INT_MAX;
            __syncthreads();
            if (live && wide_negative(A)) atomicMin(&s_first, (int)lag);
            __syncthreads();
            const int first = s_first;
            s_t[tid] = (live && lag < first) ? rho(A, n, lag, m, vh) : 0.0;
            __syncthreads();
            R = R + block_sum(s_t, tid, kThreads, [] { __syncthreads(); });
            __syncthreads();
            if (first != INT_MAX) {
                out_trunc = first;
                break;
            }
        }
        out_ess = ess_of(n, m, R);
    }
    if (tid == 0) {
        ess[pk] = out_ess;
        trunc[pk] = out_trunc;
        ones[pk] = ksum;
    }
}

}  // namespace mci
