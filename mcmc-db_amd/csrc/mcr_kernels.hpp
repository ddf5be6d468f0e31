// mcr_kernels.hpp -- the HIP kernels of the statistics hot path (gfx950, wave64, fp64 VALU).
//
// Per model (C chains x N draws, M = C*N pooled draws per parameter, P parameters) the pipeline is
//
//   k_ingest_*      (only if the tensor is not in the Arrow layout [P][C][N])  strided -> X[P][M] f64
//   k_tile_sort     X (f64, or f32 widened on load) -> sorted 4096-draw tiles of (key f64, pooled position u16 | u32),
//                   sorted as 64-bit records (upper 52 bits + tile slot), checked, as (key, position) pairs if that fails
//                   + the tile's (count, mean, M2) + every 64th order statistic of each tile
//                   (f32 tensors: k_tile_sort32 and the RecSlots<u64> instances take the first four places of this list)
//   k_merge         only for M > 64K: pairwise merge-path passes until at most 16 sorted runs remain
//                   (k_sample_runs then takes the regular samples of those runs)
//   k_splitters     exact k-way partition by regular sampling: deterministic bucket bound
//   k_bucket_merge  per bucket: gather <= 16 sorted pieces, merge in LDS, write the pooled ascending
//                   order, and (fused) tie-averaged ranks -> rank code -> time order                 (a7)
//   (order statistics: quantiles, median, fold split point -- by the first wave of every fold workgroup;
//    a k_order_stats launch of their own for Backend.stats calls and for pooled arrays beyond 64K)      (a2/a3/a8)
//   k_fold_merge    |x - med| order by ONE merge of the two monotone halves (no second sort), fused
//                   with the rank codes of the folded values, their scatter write-combined in LDS   (a8, a7)
//   k_acov_seg / k_diag_combine(2) / k_tier3 (or k_long_list + k_dev_fill + FFT | k_acov_long + k_diag_long_scan)
//                   (mcr_diag.hpp, mcr_fft.hpp) split R-hat + ESS for bulk and folded z, lags in three tiers;
//                   combine2 also packs mean / std / rhat = pymax(bulk, tail) into the result table (k_finalize
//                   does that for calls without diagnostics)                                       (a9-a13)
//   (k_rank_z: the standalone rank kernel, used only when M > 512K and no bucket partition applies)
//
// (aN) = row of SURVEY.md section 8(a); reference file:line citations are next to each kernel.
#pragma once
#include <type_traits>
#include "mcr_pipe.hpp"      // ResField, QArgs, kMomRec
#include "mcr_sortnet.h"

namespace mcr {

// ------------------------------------------------------------------------------------------------
// z lookup table.  A draw's z depends only on its tie run [s, e) and M:
//     rank = (s + 1 + e) / 2,   z = Phi^-1((rank - 0.5) / M)          (diagnostics.py:117,130-131)
// so z is a function of the integer n2 = s + e in [1, 2M-1] alone -- the same for every parameter
// of the model.  One tiny launch evaluates it for all 2M values (same operations, hence the same
// bits as evaluating it per draw).  The rank kernels therefore scatter only the 4-byte CODE n2 of
// each draw to time order (half the bytes and half the L2 footprint of scattering z itself: the
// scattered stores are the expensive part), and the consumers (k_acov_seg,
// k_diag_combine*) turn codes into z with one read of this L2-resident table.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ztable(double* __restrict__ ztab, i64 M)
{
    const i64 n2 = (i64)blockIdx.x * 256 + threadIdx.x;
    if (n2 >= 2 * M) return;
    const double r = (double)(n2 + 1) / 2.0;
    ztab[n2] = (n2 >= 1) ? inv_cdf((r - 0.5) / (double)M) : 0.0;
}

// Codes -> z and average ranks in time order (debug outputs of mcr_diagnose_chains only).
__global__ __launch_bounds__(256) void k_decode_codes(const u32* __restrict__ code, const double* __restrict__ ztab,
                                                      i64 n, double* __restrict__ z, double* __restrict__ rank)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u32 c = code[i];
    if ((i64)c > 2 * n - 1) c = (u32)(2 * n - 1);
    if (z) z[i] = ztab[c];
    if (rank) rank[i] = (double)((i64)c + 1) / 2.0;
}

// ------------------------------------------------------------------------------------------------
// Ingest: arbitrary element strides / f32 -> X[p][c*N + t] f64.  Along z the tensors of a batch (mcr_sbc_ranks' simulations):
// tensor z starts z * ss elements into src and z * xs doubles into X; one tensor: gridDim.z = 1.
// rows variant: lanes run along t (coalesced when stride_n == 1).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ingest_rows(const T* __restrict__ src, double* __restrict__ X,
                                                     i64 C, i64 N, i64 sc, i64 sn, i64 sp, i64 p0, i64 ss, i64 xs)
{
    src += (i64)blockIdx.z * ss;
    X += (i64)blockIdx.z * xs;
    const i64 nb = (N + 255) / 256;
    const i64 c = blockIdx.x / nb, t = (blockIdx.x % nb) * 256 + threadIdx.x;
    const i64 p = blockIdx.y;
    if (t < N) X[p * (C * N) + c * N + t] = (double)src[c * sc + t * sn + (p0 + p) * sp];
}

// transpose variant: lanes run along p on the read side (coalesced when stride_p == 1, i.e. the
// [C][N][P] layout of Draws.to_numpy, src/mcmc_ref/draws.py:28-29), along t on the write side.
template <typename T>
__global__ __launch_bounds__(256) void k_ingest_transpose(const T* __restrict__ src,
                                                          double* __restrict__ X, i64 C, i64 N, i64 P,
                                                          i64 sc, i64 sn, i64 sp, i64 p0, i64 ss, i64 xs)
{
    __shared__ double tile[64][65];
    src += (i64)blockIdx.z * ss;
    X += (i64)blockIdx.z * xs;
    const i64 nb = (N + 63) / 64;
    const i64 c = blockIdx.x / nb, t0 = (blockIdx.x % nb) * 64;
    const i64 pl0 = (i64)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const i64 t = t0 + r, p = pl0 + tx;
        tile[r][tx] = (t < N && p < P) ? (double)src[c * sc + t * sn + (p0 + p) * sp] : 0.0;
    }
    __syncthreads();
    for (int q = ty; q < 64; q += 4) {
        const i64 t = t0 + tx, p = pl0 + q;
        if (t < N && p < P) X[p * (C * N) + c * N + t] = tile[tx][q];
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming moments (a2/a3/a4): one HBM pass.  Every workgroup accumulates shifted sums S1 = sum(x-K),
// S2 = sum((x-K)^2) of ITS slice around a pivot K taken from that slice (the mean of its first 64 draws, so a single
// outlying draw cannot become the pivot), converts them to the slice's (count, mean, M2 = sum (x - mean)^2), and the
// finisher merges the slices with Chan's pairwise update.  Same result as the reference's two-pass forms -- np.mean /
// np.std(ddof=0) (src/mcmc_ref/backends_numpy.py:41-42), pc.mean / pc.stddev (backends_arrow.py:38-39),
// compute_basic_stats (compare.py:58-64) -- to a few ulp even when a chain starts far from its bulk (an unconverged
// `actual` handed to compare()): the cancellation is bounded by the spread INSIDE a slice, not by |first draw - mean|.
// part[(p*S + s)*kMomRec + {0..4}] = slice pivot K, slice mean - K, slice M2 (about its mean), non-finite count, slice
// length.  The mean travels as the pair (K, mean - K): rounded to one double it would carry an error of ulp(mean) / 2,
// which Chan's update multiplies by the distance between slice means -- a relative error of eps |mean| / sigma /
// sqrt(slice) in the variance, 1e-12 for draws of spread 1e-6 around 3.
// rows variant: grid (S, P); the block streams a contiguous slice of X[p][.] with 16-byte loads.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_slice_moments(double* o, double K, double s1, double s2, double bad, double n)
{
    const double dm = (n > 0.0) ? s1 / n : 0.0;         // s1 = sum (x - K), s2 = sum (x - K)^2
    double m2 = s2 - s1 * dm;
    if (!(m2 >= 0.0) && !isnan(m2)) m2 = 0.0;          // tiny negative from rounding; NaN / +inf pass through
    o[0] = K; o[1] = dm; o[2] = m2; o[3] = bad; o[4] = n;
}

// (mean, M2, bad) of a parameter from its S slice records (fixed order): Chan et al.'s combination
//     M2 = sum_s M2_s + sum_s n_s (mean_s - mean)^2,  mean = m_0 + sum_s n_s (mean_s - m_0) / N,
// with every mean difference formed as (K_s - K_0) + (dm_s - dm_0): the pivots of slices of one parameter lie close
// together, so the first term is exact, and the second is a difference of small corrections.
__device__ __forceinline__ void merge_slice_moments(const double* __restrict__ rec, int S, double& mean, double& m2,
                                                    double& bad, double& n)
{
    const double K0 = rec[0], d0 = rec[1];
    double acc = 0.0, N = 0.0, b = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* o = rec + (i64)s * kMomRec;
        acc += o[4] * ((o[0] - K0) + (o[1] - d0)); N += o[4]; b += o[3];
    }
    const double mr = (N > 0.0) ? acc / N : NAN;        // the mean, relative to K0 + d0
    double q = 0.0;
    for (int s = 0; s < S; ++s) {
        const double* o = rec + (i64)s * kMomRec;
        const double d = ((o[0] - K0) + (o[1] - d0)) - mr;
        q += o[2]; q = fma(o[4] * d, d, q);
    }
    mean = K0 + (d0 + mr); m2 = q; bad = b; n = N;
}

template <typename T>
__global__ __launch_bounds__(256) void k_moments_rows(const T* __restrict__ X, i64 M, i64 pstride,
                                                      double* __restrict__ part, int S)
{
    __shared__ double red[12];
    const i64 p = blockIdx.y;
    const int s = blockIdx.x;
    const T* x = X + p * pstride;
    constexpr int V = 16 / sizeof(T);  // elements per 16-byte load
    i64 per = (M + S - 1) / S;
    per = (per + V - 1) / V * V;
    const i64 b = s * per, e = (b + per < M) ? b + per : M;
    // pivot: mean of the slice's first (up to) 64 draws, the same value in every lane
    double K = 0.0;
    {
        const int lane = threadIdx.x & 63;
        const i64 cnt = (e - b < 64) ? e - b : 64;
        K = (lane < cnt) ? (double)x[b + lane] : 0.0;
        K = wave_sum(K) / (double)(cnt > 0 ? cnt : 1);
        if (!isfinite(K)) K = 0.0;                      // non-finite draws: the call is rejected anyway; keep the sums defined
    }
    double s1 = 0.0, s2 = 0.0, bad = 0.0;
    auto acc1 = [&](double v) {
        const double d = v - K;
        s1 += d; s2 = fma(d, d, s2);
        bad += isfinite(v) ? 0.0 : 1.0;
    };
    i64 scalar_from = b;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && e > b) {
        const i64 nvec = (e - b) / V;  // b is a multiple of V, so x + b stays 16-byte aligned
        const float4* xv = reinterpret_cast<const float4*>(x + b);
        i64 g = threadIdx.x;
        for (; g + 3 * 256 < nvec; g += 4 * 256) {  // 4 independent 16-byte loads in flight per lane
            float4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = xv[g + u * 256];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T* v = reinterpret_cast<const T*>(&r[u]);
#pragma unroll
                for (int j = 0; j < V; ++j) acc1((double)v[j]);
            }
        }
        for (; g < nvec; g += 256) {
            const float4 r = xv[g];
            const T* v = reinterpret_cast<const T*>(&r);
#pragma unroll
            for (int j = 0; j < V; ++j) acc1((double)v[j]);
        }
        scalar_from = b + nvec * V;
    }
    for (i64 j = scalar_from + threadIdx.x; j < e; j += 256) acc1((double)x[j]);
    block_sum3<256>(s1, s2, bad, red);
    if (threadIdx.x == 0) store_slice_moments(part + (p * S + s) * kMomRec, K, s1, s2, bad, (double)(e > b ? e - b : 0));
}

// strided variant: every tensor that is not row-contiguous (stride_n != 1 or stride_c != N), whatever its stride_p
// (coalesced when stride_p == 1, the [C][N][P] layout): lanes run along p, each thread owns one parameter and walks a
// slice of the C*N rows.  grid (ceil(P/64), S), block (64, 4).
template <typename T>
__global__ __launch_bounds__(256) void k_moments_cols(const T* __restrict__ src, i64 C, i64 N, i64 P,
                                                      i64 sc, i64 sn, i64 sp, double* __restrict__ part,
                                                      int S)
{
    __shared__ double sh[3][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const i64 p = (i64)blockIdx.x * 64 + tx;
    const int s = blockIdx.y;
    const i64 M = C * N;
    const i64 per = (M + S - 1) / S, b = s * per, e = (b + per < M) ? b + per : M;
    double s1 = 0.0, s2 = 0.0, bad = 0.0, K = 0.0;
    if (p < P && b < e) {
        { const i64 c = b / N, t = b - c * N; K = (double)src[c * sc + t * sn + p * sp]; }     // pivot: first draw of the slice
        if (!isfinite(K)) K = 0.0;
        for (i64 r = b + ty; r < e; r += 4) {
            const i64 c = r / N, t = r - c * N;
            const double v = (double)src[c * sc + t * sn + p * sp], d = v - K;
            s1 += d; s2 = fma(d, d, s2);
            bad += isfinite(v) ? 0.0 : 1.0;
        }
    }
    sh[0][ty][tx] = s1; sh[1][ty][tx] = s2; sh[2][ty][tx] = bad;
    __syncthreads();
    if (ty == 0 && p < P)
        store_slice_moments(part + (p * S + s) * kMomRec, K, sh[0][0][tx] + sh[0][1][tx] + sh[0][2][tx] + sh[0][3][tx],
                            sh[1][0][tx] + sh[1][1][tx] + sh[1][2][tx] + sh[1][3][tx],
                            sh[2][0][tx] + sh[2][1][tx] + sh[2][2][tx] + sh[2][3][tx], (double)(e > b ? e - b : 0));
}

// mean/std from the S slice records of every parameter (fixed summation order).
// Writes mean[p], std[p] directly (mcr_moments_dev / mcr_basic_stats).
__global__ void k_moments_final(const double* __restrict__ part, int S, i64 P, double* __restrict__ mean,
                                double* __restrict__ stdv, double* __restrict__ bad)
{
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double mu, m2, b, n;
    merge_slice_moments(part + p * S * kMomRec, S, mu, m2, b, n);
    double var = m2 / n;
    if (isinf(m2)) var = INFINITY;          // squares overflowed: inf like np.std
    else if (!(var >= 0.0)) var = 0.0;
    mean[p] = mu;
    stdv[p] = sqrt(var);
    if (bad) bad[p] = b;
}

// ------------------------------------------------------------------------------------------------
// Tile sort: one workgroup sorts T = NT*VT pooled draws of one parameter entirely in LDS
// (thread-local odd-even network over VT registers, then log2(NT) merge-path levels), carrying the
// pooled position as a u32 payload.  Spec: the `sorted(flat, key=...)` of
// src/mcmc_ref/diagnostics.py:110 (stability is irrelevant: ties share one average rank).
// Also emits the moments (count, mean, M2) of its tile (so the draws are read from HBM once).
// Partial tiles are padded with +inf (draws are finite or the call fails with MCR_ENONFINITE).
// ------------------------------------------------------------------------------------------------
// The first two merge levels of the tile sort (16 -> 32 -> 64 sorted draws) without the LDS: bitonic merges across 2 and 4
// lanes.  Lane L of a group holds the sorted draws 16 L .. 16 L + 15 of the group's run in its registers.  To merge the
// ascending runs A and B of a group, draw e of A meets draw n-1-e of B (the partner lane is the mirror lane of the
// group, the partner register the mirror register): the A side keeps the minima, the B side the maxima, which leaves
// two bitonic sequences with every draw of the first at or below every draw of the second; half-cleaners at distance
// 16 (partner lane L ^ 1, same register; 4-lane level only) and then 8, 4, 2, 1 inside the lane sort each of them.
// The partner's registers arrive by DPP quad permutes (a VALU operand path, no LDS traffic, no waitcnt); a lane reads
// its partner's OLD registers because the wave executes the permutes of a register pair before it writes either.
// 52 VALU per draw for the two levels, no LDS, against 72 VALU + 9 LDS instructions per draw for the same two levels on
// the merge-path route.  A third level (8 lanes: row_half_mirror, then distances 32 and 16) costs the VALU of its LDS
// form and still wins for the LDS instructions and the barrier pair it saves; a fourth (16 lanes: lane ^ 4 takes two
// DPP movs per word) measured slower than its LDS form (tile sort 396 -> 408 us on 1000 parameters).  Ties keep their own side (stability is irrelevant: equal draws share one average rank).
// (The helpers themselves -- lane_pair_stage_rec, lane_bitonic_merge16_rec, lane_merge_levels_rec -- are below, once for
// every kind of register item.)
//
// b where the lane's bit of m is set, else a: one v_cndmask on a mask built on the scalar unit (the compiler's own lowering
// of a per-lane choice between two compare results goes through 0 / 1 in VGPRs: six more VALU per exchange).
__device__ __forceinline__ u32 select_by_mask(u32 a, u32 b, unsigned long long m)
{
    u32 r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
__device__ __forceinline__ double select_by_mask(double a, double b, unsigned long long m)
{
    return __hiloint2double((int)select_by_mask((u32)__double2hiint(a), (u32)__double2hiint(b), m),
                            (int)select_by_mask((u32)__double2loint(a), (u32)__double2loint(b), m));
}

// Serial merge of up to VT outputs from LDS runs A = skey[pos16(a0 + .)] (na items) and
// B = skey[pos16(b0 + .)] (nb items), starting at (ai, bi).  src[i] = LDS slot the output came from.
// Branch-free.  Which run is exhausted is decided on the POINTERS (two integer compares whose lane masks are combined
// with the key compare on the scalar unit), so the head values need no sanitising: the LDS read of the next head is
// unconditional (one slot past a run is still inside the workgroup's LDS) and whatever it returns past the end of a
// run is never selected.  Ties take from A.  ~19 VALU per output (25 with the +inf substitution this replaced).
template <int VT>
__device__ __forceinline__ void serial_merge(const double* skey, int a0, int na, int b0, int nb, int ai,
                                             int bi, int nout, double (&k)[VT], int (&src)[VT])
{
    int pa = a0 + ai, pb = b0 + bi;
    const int ea = a0 + na, eb = b0 + nb;
    double ak = skey[pos16(pa)], bk = skey[pos16(pb)];
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        if (i < nout) {
            const bool takeA = (pb >= eb) | ((pa < ea) & !(bk < ak));
            k[i] = takeA ? ak : bk;
            src[i] = takeA ? pa : pb;
            pa += takeA ? 1 : 0;
            pb += takeA ? 0 : 1;
            const int pn = takeA ? pa : pb;
            const double nv = skey[pos16(pn)];
            ak = takeA ? nv : ak;
            bk = takeA ? bk : nv;
        } else {
            src[i] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Sorting RECORDS: one 64-bit word per draw that orders by itself and carries its payload, so a compare-exchange is one
// compare + four selects (or one minimum + one maximum) instead of one compare + six selects, a lane-pair exchange moves
// two words instead of three, and nothing is gathered after a merge level.  R = u64 (f32 draws: key image << 32 |
// position, k_tile_sort32) or double (f64 draws: the draw with its low 12 mantissa bits replaced by its tile slot,
// k_tile_sort below).
// The register helpers of this section are written once, for any item R that has rec_ce, dpp_rec, select_by_mask and
// `<`: the two records, and KeyPos -- the (f64 key, position) PAIR of the pair sort, three words that order by the key.
// ------------------------------------------------------------------------------------------------
struct KeyPos { double k; u32 ix; };
__device__ __forceinline__ bool operator<(const KeyPos& a, const KeyPos& b) { return a.k < b.k; }

__device__ __forceinline__ u32 rec_key(u64 r) { return (u32)(r >> 32); }
__device__ __forceinline__ u32 rec_pos(u64 r) { return (u32)r; }
// the f64 value the statistics use
__device__ __forceinline__ double key_f64(double k) { return k; }
__device__ __forceinline__ double key_f64(u64 r) { return key_value(rec_key(r)); }

template <typename R> __device__ __forceinline__ R rec_pad();
template <> __device__ __forceinline__ u64 rec_pad<u64>() { return kRecPad; }
template <> __device__ __forceinline__ double rec_pad<double>() { return INFINITY; }

__device__ __forceinline__ void rec_ce(u64& a, u64& b)
{
    const bool sw = b < a;
    const u64 lo = sw ? b : a, hi = sw ? a : b;
    a = lo; b = hi;
}
// Double records are finite or the +inf pad, never NaN, and no two live ones are equal (they differ in the slot bits; of +0.0
// and -0.0 only slot 0 can hold one), so minimum and maximum return the two operands themselves, bit for bit (fp64
// denormals are never flushed on this target).  As instructions, not as fmin / fmax: those canonicalise operands the
// compiler cannot prove quiet -- one more instruction for every register that comes out of a DPP move.
__device__ __forceinline__ void rec_ce(double& a, double& b)
{
    double lo, hi;
    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    a = lo; b = hi;
}
__device__ __forceinline__ void rec_ce(KeyPos& a, KeyPos& b)
{
    const bool sw = b.k < a.k;
    const double lo = sw ? b.k : a.k, hi = sw ? a.k : b.k;
    const u32 ilo = sw ? b.ix : a.ix, ihi = sw ? a.ix : b.ix;
    a.k = lo; b.k = hi; a.ix = ilo; b.ix = ihi;
}

// Register sort of VT items per lane: fully static networks (60 comparators for 16 registers, mcr_sortnet.h).  Every
// index is a compile-time constant, so the items stay in VGPRs (a loop-carried index here makes hipcc emulate dynamic
// register indexing with 16-way select chains: 10x the instructions).
template <int VT, typename R>
__device__ __forceinline__ void thread_sort_rec(R (&r)[VT])
{
    static_assert(VT == 16 || VT == 8, "sorting networks exist for 16 and 8 items per lane");
#define MCR_CE(a, b) rec_ce(r[a], r[b]);
    if constexpr (VT == 16) { MCR_NET16(MCR_CE) } else { MCR_NET8(MCR_CE) }
#undef MCR_CE
}

// The first three merge levels of the tile sort (16 -> 128 items) as bitonic merges across 2, 4 and 8 lanes over DPP
// (above); an exchange is one compare per side.
template <int CTRL>
__device__ __forceinline__ u64 dpp_rec(u64 v)
{
    return ((u64)dpp_u32<CTRL>((u32)(v >> 32)) << 32) | (u64)dpp_u32<CTRL>((u32)v);
}
template <int CTRL>
__device__ __forceinline__ double dpp_rec(double v) { return dpp_f64<CTRL>(v); }
__device__ __forceinline__ u64 select_by_mask(u64 a, u64 b, unsigned long long m)
{
    return ((u64)select_by_mask((u32)(a >> 32), (u32)(b >> 32), m) << 32) | (u64)select_by_mask((u32)a, (u32)b, m);
}
template <int CTRL>
__device__ __forceinline__ KeyPos dpp_rec(const KeyPos& v) { return KeyPos{dpp_f64<CTRL>(v.k), dpp_u32<CTRL>(v.ix)}; }
__device__ __forceinline__ KeyPos select_by_mask(const KeyPos& a, const KeyPos& b, unsigned long long m)
{
    return KeyPos{select_by_mask(a.k, b.k, m), select_by_mask(a.ix, b.ix, m)};
}

template <int CTRL, bool MIRROR, unsigned long long MIN_LANES, typename R>
__device__ __forceinline__ void lane_pair_stage_rec(R (&r)[16])
{
    auto exchange = [](R& own, R o) {
        const unsigned long long lt = __builtin_amdgcn_ballot_w64(o < own), gt = __builtin_amdgcn_ballot_w64(own < o);
        own = select_by_mask(own, o, (lt & MIN_LANES) | (gt & ~MIN_LANES));
    };
#pragma unroll
    for (int i = 0; i < (MIRROR ? 8 : 16); ++i) {
        const int s = MIRROR ? 15 - i : i;
        const R o_i = dpp_rec<CTRL>(r[s]);
        if (MIRROR) {
            const R o_s = dpp_rec<CTRL>(r[i]);
            exchange(r[s], o_s);
        }
        exchange(r[i], o_i);
    }
}

template <typename R>
__device__ __forceinline__ void lane_bitonic_merge16_rec(R (&r)[16])
{
#define MCR_CE(a, b) rec_ce(r[a], r[b]);
    MCR_BITONIC16(MCR_CE)
#undef MCR_CE
}

template <typename R>
__device__ __forceinline__ void lane_merge_levels_rec(R (&r)[16])
{
    constexpr unsigned long long kEvenLanes = 0x5555555555555555ull, kLowPairs = 0x3333333333333333ull,
                                 kLowQuads = 0x0F0F0F0F0F0F0F0Full;
    lane_pair_stage_rec<0xB1, true, kEvenLanes>(r);
    lane_bitonic_merge16_rec(r);
    lane_pair_stage_rec<0x1B, true, kLowPairs>(r);
    lane_pair_stage_rec<0xB1, false, kEvenLanes>(r);
    lane_bitonic_merge16_rec(r);
    lane_pair_stage_rec<0x141, true, kLowQuads>(r);
    lane_pair_stage_rec<0x4E, false, kLowPairs>(r);
    lane_pair_stage_rec<0xB1, false, kEvenLanes>(r);
    lane_bitonic_merge16_rec(r);
}

// serial_merge on records: the record IS the payload, so there is nothing to gather afterwards.
// LIM > 0: slot indices are clamped to LIM (k_tile_sort32 declares exactly T slots so that five tiles fit a CU, and
// the unconditional read one past the last run must not leave them).
template <int VT, int LIM = 0, typename R>
__device__ __forceinline__ void serial_merge_rec(const R* srec, int a0, int na, int b0, int nb, int ai, int bi,
                                                 int nout, R (&out)[VT])
{
    int pa = a0 + ai, pb = b0 + bi;
    const int ea = a0 + na, eb = b0 + nb;
    auto slot = [](int e) { return pos16(LIM > 0 ? min(e, LIM) : e); };
    R ar = srec[slot(pa)], br = srec[slot(pb)];
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        if (i < nout) {
            const bool takeA = (pb >= eb) | ((pa < ea) & !(br < ar));
            out[i] = takeA ? ar : br;
            pa += takeA ? 1 : 0;
            pb += takeA ? 0 : 1;
            const int pn = takeA ? pa : pb;
            const R nv = srec[slot(pn)];
            ar = takeA ? nv : ar;
            br = takeA ? br : nv;
        } else {
            out[i] = rec_pad<R>();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// What a slot of the sort stage's LDS holds.  The tile sorts' shared parts and the merge pass are written once over
// one of two layouts of a workgroup's T slots:
//   PairSlots<IdxT>  an f64 key in skey[T], then its pooled position in sidx[T].  IdxT = u16 when M < 65536 (C1 and every
//                    packaged model: 10 bytes per slot, so FOUR 4096-slot workgroups are resident per CU instead of three,
//                    and 10 instead of 12 bytes per draw go to HBM and back), u32 otherwise.  Nothing else: the single read
//                    "one slot past the last run" of serial_merge lands on sidx[0] (in bounds, never selected), and the
//                    64 key slots at the top are free for scratch in every kernel that needs some (their runs are
//                    bounded by T - 64).
//   RecSlots<R>      one record in srec[T] that orders by itself and carries its position (R = u64: f32 draws; R = double:
//                    the f64 tile sort, which only stores, reads and merges them).  Two more slots than records, so that the
//                    read one past the last run stays in bounds (the tile sorts give exactly T and clamp instead: LIM).
// KeyT / PosT are the element types of the arrays in memory (a record stage has no position arrays: its position pointers are never used).
// An Item is a slot's content in registers.
// ------------------------------------------------------------------------------------------------
template <typename IdxT>
struct PairSlots {
    using KeyT = double;
    using PosT = IdxT;
    using Item = KeyPos;
    static constexpr int kTail = 0;     // slots behind the T of the workgroup
    static constexpr size_t lds_bytes(int T) { return (size_t)T * (8 + sizeof(IdxT)); }
    double* skey;
    IdxT* sidx;
    __device__ __forceinline__ PairSlots(char* smem, int T)
        : skey(reinterpret_cast<double*>(smem)), sidx(reinterpret_cast<IdxT*>(skey + T)) {}
    static __device__ __forceinline__ Item load(const double* k, const IdxT* ix, i64 g) { return Item{k[g], (u32)ix[g]}; }
    __device__ __forceinline__ void put(int e, const Item& v) const { skey[pos16(e)] = v.k; sidx[posi(e)] = (IdxT)v.ix; }
    __device__ __forceinline__ double get(int e) const { return skey[pos16(e)]; }        // what the merges order by
    // serial merge of `nout` <= VT outputs (serial_merge); the positions are gathered from the slots the keys came from
    template <int VT, int LIM = 0>
    __device__ __forceinline__ void merge(int a0, int na, int b0, int nb, int ai, int bi, int nout, Item (&out)[VT]) const
    {
        double k[VT];
        int src[VT];
        serial_merge<VT>(skey, a0, na, b0, nb, ai, bi, nout, k, src);
#pragma unroll
        for (int i = 0; i < VT; ++i) out[i] = Item{k[i], (u32)sidx[posi(src[i])]};
    }
    __device__ __forceinline__ void write(double* k, IdxT* ix, i64 g, int e) const { k[g] = skey[pos16(e)]; ix[g] = sidx[posi(e)]; }   // slot e -> element g
};

template <typename R>
struct RecSlots {
    using KeyT = R;
    using PosT = u32;
    using Item = R;
    static constexpr int kTail = 2;
    static constexpr size_t lds_bytes(int T) { return (size_t)(T + kTail) * 8; }
    R* srec;
    __device__ __forceinline__ RecSlots(char* smem, int) : srec(reinterpret_cast<R*>(smem)) {}
    static __device__ __forceinline__ R load(const R* r, const u32*, i64 g) { return r[g]; }
    __device__ __forceinline__ void put(int e, R v) const { srec[pos16(e)] = v; }
    __device__ __forceinline__ R get(int e) const { return srec[pos16(e)]; }
    // LIM > 0: see serial_merge_rec
    template <int VT, int LIM = 0>
    __device__ __forceinline__ void merge(int a0, int na, int b0, int nb, int ai, int bi, int nout, R (&out)[VT]) const
    {
        serial_merge_rec<VT, LIM>(srec, a0, na, b0, nb, ai, bi, nout, out);
    }
    __device__ __forceinline__ void write(R* r, const void*, i64 g, int e) const { r[g] = srec[pos16(e)]; }    // (no position array: a pointer nothing can be read or written through)
};

// ---- what the three tile sorts share: everything behind the lane's VT items sorted in registers ------------------
// The merge levels in the LDS behind the three register levels: the lane's items go to its slots, then every level merges
// pairs of runs by merge path and hands the lane its VT outputs in r[].  !STORE_LAST: the outputs of the last level stay in
// registers only.  LIM: see serial_merge_rec.
template <int NT, int VT, int LIM, bool STORE_LAST, class Slots>
__device__ __forceinline__ void tile_merge_levels(const Slots& s, typename Slots::Item (&r)[VT])
{
    const int tid = threadIdx.x;
    // (no barrier: this is the workgroup's first access to the LDS)
#pragma unroll
    for (int i = 0; i < VT; ++i) s.put(tid * VT + i, r[i]);
    __syncthreads();
    for (int coop = (VT == 16) ? 16 : 2; coop <= NT; coop <<= 1) {     // (16 registers per lane: lane_merge_levels_rec came first)
        const int first = tid & ~(coop - 1);
        const int run = VT * (coop >> 1);
        const int a0 = first * VT, b0 = a0 + run;
        const int diag = VT * (tid - first);
        auto A = [&](int i) { return s.get(a0 + i); };
        auto B = [&](int j) { return s.get(b0 + j); };
        const int ai = merge_path32(A, run, B, run, diag);
        s.template merge<VT, LIM>(a0, run, b0, run, ai, diag - ai, VT, r);
        __syncthreads();
        if (STORE_LAST || coop < NT) {
#pragma unroll
            for (int i = 0; i < VT; ++i) s.put(tid * VT + i, r[i]);
            __syncthreads();
        }
    }
}

// The sorted tile from the LDS to out[g0 + e], coalesced.  count == T is workgroup-uniform: a full tile (nine of C1's ten
// per parameter) takes the loop without a per-draw `e < count` test, chosen by a scalar branch -- here, in the kernels'
// loads and in tile_moments.
template <int NT, int VT, class Slots>
__device__ __forceinline__ void tile_write_out(const Slots& s, typename Slots::KeyT* __restrict__ keys,
                                               typename Slots::PosT* __restrict__ idx, i64 g0, int count)
{
    constexpr int T = NT * VT;
    const int tid = threadIdx.x;
    auto write_out = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma nounroll
        for (int e = tid; e < (FULL ? T : count); e += NT) s.write(keys + g0, idx + g0, e, e);
    };
    if (count == T) write_out(std::true_type{}); else write_out(std::false_type{});
}

// The tile sorts run on a grid (ntiles, P): this workgroup's row in the per-tile tables
__device__ __forceinline__ i64 tile_row(int ntiles) { return (i64)blockIdx.y * ntiles + (int)blockIdx.x; }

// regular samples (every 64th order statistic of the tile) for the exact bucket partition, into samp (may be null)
template <int NT, int VT, class Slots>
__device__ __forceinline__ void tile_store_samples(const Slots& s, double* __restrict__ samp, int ntiles, int count)
{
    constexpr int T = NT * VT;
    const int tid = threadIdx.x;
    if (samp != nullptr && tid < T / 64) {
        const int e = 64 * tid + 63;
        samp[tile_row(ntiles) * (T / 64) + tid] = (e < count) ? key_f64(s.get(e)) : INFINITY;
    }
}

// Moments of the tile, two-pass like the reference (mean first, then squared deviations; compare.py:62-63), from the
// lane's VT sorted draws still in registers (the draws are read from HBM exactly once): val(i) = the draw in the lane's
// sorted slot i as f64, slots at or beyond `count` hold pads.  The same values in the same slots, added in the same order,
// whichever sort put them there.  `red`: the reduction scratch, the head of the LDS once the sorted tile has left it
// (barrier before the call).  k_finalize merges the tiles' records in `part` with Chan's update.
template <int NT, int VT, class VF>
__device__ __forceinline__ void tile_moments(VF val, int count, double bad, double* red, double* __restrict__ part, int ntiles)
{
    const int tid = threadIdx.x;
    double s1 = 0.0, s2 = 0.0, e1 = 0.0, mt = 0.0;
    auto moments = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        const int nlive = count - tid * VT;         // the lane's sorted slots [0, nlive) hold draws, the others pads
#pragma unroll
        for (int i = 0; i < VT; ++i) s1 += (FULL || i < nlive) ? val(i) : 0.0;
        s1 = block_sum<NT>(s1, red);
        mt = s1 / (double)count;
        // second pass about mt; e1 = sum (x - mt) is what rounding left of the mean
#pragma unroll
        for (int i = 0; i < VT; ++i) { const double d = (FULL || i < nlive) ? val(i) - mt : 0.0; s2 = fma(d, d, s2); e1 += d; }
    };
    if (count == NT * VT) moments(std::true_type{}); else moments(std::false_type{});
    block_sum3<NT>(s2, e1, bad, red);
    if (tid == 0) store_slice_moments(part + tile_row(ntiles) * kMomRec, mt, e1, s2, bad, (double)count);
}

// The tile sort on (f64 key, position) PAIRS: the whole kernel up to round 7, and since then what a workgroup falls back to
// when its tile cannot be sorted as records (below).
// A function of its own under the record sort: inlined, the two sorts' registers exceed the 128 that four waves per SIMD
// allow, or spill on the record path.  As a call the record path has no spill; the callee's frame (104 bytes per lane, its
// callee-saved registers) is touched by falling tiles only.
template <int NT, int VT, typename IdxT, typename XT>
__device__ __noinline__ void tile_sort_pairs(const XT* __restrict__ X, i64 M,
                                             double* __restrict__ keys, IdxT* __restrict__ idx,
                                             double* __restrict__ part, int ntiles,
                                             double* __restrict__ samp)
{
    constexpr int T = NT * VT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PairSlots<IdxT> s(smem, T);

    const int tid = threadIdx.x, tile = blockIdx.x;
    const i64 p = blockIdx.y;
    const i64 base = (i64)tile * T;
    const int count = (int)((M - base < (i64)T) ? M - base : (i64)T);
    const XT* src = X + p * M + base;    // XT = float: f32 tensors in the Arrow layout are widened here, not by an ingest pass

    // Lane tid takes draws i * NT + tid straight into its sort registers (coalesced loads, no staging pass through the LDS):
    // the network and the merge levels sort whatever 16 draws a lane starts with.  Which of a tile's equal draws comes first
    // therefore differs from a blocked hand-out; nothing downstream sees it (equal draws share one average rank).
    KeyPos r[VT];
    double bad = 0.0;
    auto load = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int i = 0; i < VT; ++i) {
            const int e = i * NT + tid;
            const bool live = FULL || e < count;
            // a pad slot re-reads the tile's last draw instead of skipping the load: a load under a per-lane test waits for
            // its value inside the test, and the lane's 16 loads go out one round trip after the other
            const double v = (double)src[FULL ? e : min(e, count - 1)];
            r[i].k = live ? v : INFINITY;
            r[i].ix = live ? (u32)(base + e) : 0xFFFFFFFFu;
            bad += (live && !isfinite(v)) ? 1.0 : 0.0;
        }
    };
    if (count == T) load(std::true_type{}); else load(std::false_type{});
    thread_sort_rec<VT>(r);
    if constexpr (VT == 16) lane_merge_levels_rec(r);
    tile_merge_levels<NT, VT, 0, true>(s, r);
    tile_write_out<NT, VT>(s, keys, idx, p * M + base, count);
    tile_store_samples<NT, VT>(s, samp, ntiles, count);
    __syncthreads();                 // the reduction scratch takes the place of the keys from here on
    tile_moments<NT, VT>([&](int i) { return r[i].k; }, count, bad, s.skey, part, ntiles);
}

// ------------------------------------------------------------------------------------------------
// The tile sort proper: f64 draws as 64-bit records, with the pair sort above as the exact fallback.
// An f64 key and a 12-bit tile slot do not fit 64 bits, but they almost do: two draws of one tile that agree in their upper
// 52 bits and differ below lie within 2^-40 of each other, relatively -- rounded, tied or ordinary draws never do.  So
//   record = the draw with its low 12 mantissa bits replaced by its slot e (the 12 bits wait in slow[e], 8 KB of LDS where
//            the pair sort keeps its positions), compared as a double: the order of (upper 52 bits, then slot, up or down
//            with the sign);
//   sort     network, three DPP levels and five LDS levels on records alone (no ix[], no src[], no position traffic);
//   rebuild  key = record with slow[slot] back in its low bits (exact), position = base + slot, in registers, where the
//            lane's 16 consecutive sorted draws are -- the moments run on them as in the pair sort, bit for bit;
//   CHECK    every adjacent pair of rebuilt keys non-decreasing: 15 compares in the lane, the lane boundary over DPP, the
//            wave boundaries and the waves' flags through a few words of the dead record array.  Adjacent order is
//            sorted order.
// A workgroup whose check fails (some draws tie in the upper 52 bits and their low bits order them against their slots)
// runs tile_sort_pairs on the same 40 KB and writes the tile from there: no second launch, nothing written before the
// check.  Equal keys come out by slot instead of by hand-out; nothing downstream sees it.  Non-finite draws are counted and
// sorted as a tiny finite stand-in (the call fails with MCR_ENONFINITE anyway), pads are +inf.  f32 draws widen to
// doubles whose low 29 bits are zero: they never fall back.
// `fallbacks` (may be null) counts the tiles that fell back (mcr_tile_fallback_count).
// amdgpu_waves_per_eu(4): 40 KB of LDS put four workgroups = four waves per SIMD on a CU; told so, the compiler keeps kernel
// and callee within 128 registers (two waves per SIMD otherwise).
// ------------------------------------------------------------------------------------------------
template <int NT, int VT, typename IdxT, typename XT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_tile_sort(const XT* __restrict__ X, i64 M,
                                                  double* __restrict__ keys, IdxT* __restrict__ idx,
                                                  double* __restrict__ part, int ntiles,
                                                  double* __restrict__ samp, unsigned* __restrict__ fallbacks)
{
    constexpr int T = NT * VT;
    constexpr u32 kSlotMask = 0xFFFu;
    static_assert(T <= 4096, "a record has 12 bits for the tile slot");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const RecSlots<double> recs(smem, T);                                    // the records ...
    const PairSlots<IdxT> s(smem, T);                                        // ... then the rebuilt keys and their positions
    double* srec = recs.srec;
    unsigned short* slow = reinterpret_cast<unsigned short*>(srec + T);      // the draws' low 12 bits by slot, where the positions will be

    const int tid = threadIdx.x, tile = blockIdx.x;
    const i64 p = blockIdx.y;
    const i64 base = (i64)tile * T;
    const int count = (int)((M - base < (i64)T) ? M - base : (i64)T);
    const XT* src = X + p * M + base;
    const bool full = count == T;        // workgroup-uniform, as in the pair sort
    const int nlive = count - tid * VT;  // after the sort the lane's slots [0, nlive) hold draws, the others pads

    double r[VT];
    double bad = 0.0;
    auto load = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        XT v[VT];
#pragma unroll
        for (int i = 0; i < VT; ++i) {       // every load unconditional and in flight (a pad slot re-reads the last draw)
            const int e = i * NT + tid;
            v[i] = src[FULL ? e : min(e, count - 1)];
        }
#pragma unroll
        for (int i = 0; i < VT; ++i) {
            const int e = i * NT + tid;
            const bool live = FULL || e < count;
            const double d = (double)v[i];
            const bool fin = isfinite(d);
            bad += (live && !fin) ? 1.0 : 0.0;
            const u32 lo = (u32)__double2loint(d), hi = (u32)__double2hiint(d);
            if (live) slow[e] = (unsigned short)(lo & kSlotMask);                // lane tid, slot i * NT + tid: conflict-free
            const double rec = __hiloint2double((int)(fin ? hi : 0u), (int)((lo & ~kSlotMask) | (u32)e));
            r[i] = live ? rec : INFINITY;
        }
    };
    if (full) load(std::true_type{}); else load(std::false_type{});
    thread_sort_rec<VT>(r);
    if constexpr (VT == 16) lane_merge_levels_rec(r);
    // (the read "one slot past the last run" of serial_merge_rec lands on slow[0..3]: in bounds, never selected; the last
    //  level's records stay in registers)
    tile_merge_levels<NT, VT, 0, false>(recs, r);

    // rebuild keys and positions of the lane's 16 consecutive sorted draws; check; stage them for the coalesced write-out
    double k[VT];
    u32 slot[VT];
    bool viol = false;
    auto rebuild = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int i = 0; i < VT; ++i) {
            const u32 lo = (u32)__double2loint(r[i]);
            slot[i] = lo & kSlotMask;                     // (a pad's "slot" is 0: read, not used)
            const double key = __hiloint2double(__double2hiint(r[i]), (int)((lo & ~kSlotMask) | (u32)slow[slot[i]]));
            k[i] = (FULL || i < nlive) ? key : INFINITY;
        }
    };
    if (full) rebuild(std::true_type{}); else rebuild(std::false_type{});
#pragma unroll
    for (int i = 0; i + 1 < VT; ++i) viol |= k[i + 1] < k[i];
    // The lane boundary inside a wave over DPP (wave_shl:1 hands lane L the first key of lane L + 1); the three wave
    // boundaries and the waves' flags through 12 words at the head of the record array, which is dead since the barrier
    // behind the last level.  No __syncthreads_or: its 256 bytes of static LDS on top of the 40 960 dynamic ones would
    // leave three workgroups per CU instead of four.
    constexpr int NW = NT / kWave;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const double next_first = dpp_f64<0x130>(k[0]);
    viol |= lane + 1 < kWave && next_first < k[VT - 1];
    int* wflag = reinterpret_cast<int*>(srec + 2 * NW);
    const bool wave_viol = __builtin_amdgcn_ballot_w64(viol) != 0;
    if (lane == 0) { srec[wave] = k[0]; wflag[wave] = wave_viol ? 1 : 0; }
    if (lane == kWave - 1) srec[NW + wave] = k[VT - 1];
    __syncthreads();
    bool fall = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        fall |= wflag[w] != 0;
        if (w + 1 < NW) fall |= srec[w + 1] < srec[NW + w];
    }
    __syncthreads();                     // the scratch is read: the keys (or the pair sort) may take its place
    if (fall) {
        if (tid == 0 && fallbacks != nullptr) atomicAdd(fallbacks, 1u);
        tile_sort_pairs<NT, VT, IdxT, XT>(X, M, keys, idx, part, ntiles, samp);
        return;
    }
    // (every lane read its low bits before the first of the two barriers: the positions may take their place)
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        // (spelt out: through s.put the compiler issues the sixteen key stores in one burst behind the position stores,
        //  1.5 % of the kernel on 400 000-draw arrays)
        s.skey[pos16(tid * VT + i)] = k[i];
        s.sidx[posi(tid * VT + i)] = (IdxT)((u32)base + slot[i]);
    }
    __syncthreads();
    tile_write_out<NT, VT>(s, keys, idx, p * M + base, count);
    tile_store_samples<NT, VT>(s, samp, ntiles, count);
    __syncthreads();                 // the reduction scratch takes the place of the keys from here on
    tile_moments<NT, VT>([&](int i) { return k[i]; }, count, bad, srec, part, ntiles);
}

// ------------------------------------------------------------------------------------------------
// The tile sort of f32 draw tensors (BASELINE config 4: 4 x 100000 x 10000 f32): 4096 pooled f32 draws of one parameter
// -> sorted records, the tile's moments (two-pass on the widened values, as k_tile_sort) and every 64th order statistic.
//     record = order-preserving image of the f32 bits (f32_key) << 32 | pooled position
// instead of an f64 key plus a separate position: 8 bytes per LDS slot and per HBM element instead of 12, one integer
// compare per merge step that orders (value, position) at once, no payload gather after a merge level, and no widening
// ingest pass over the tensor (it is read from HBM exactly once, as f32).  The stages behind it (k_merge, k_bucket_merge,
// the fold) run on these records through RecSlots<u64>.  Same results as the f64 kernels bit for bit: widening f32 -> f64
// preserves order and equality, so ranks, order statistics and the widened values the moments / fold step see are
// identical.  +inf pads are kRecPad.  Reference spec of the whole stage: the `sorted(flat, key=...)` and average ranks of
// src/mcmc_ref/diagnostics.py:101-122.
// LDS: exactly T records, so that five tiles fit a CU; the merges clamp their reads to the last slot (LIM).
// ------------------------------------------------------------------------------------------------
template <int NT, int VT>
__global__ __launch_bounds__(NT) void k_tile_sort32(const float* __restrict__ X, i64 M, u64* __restrict__ recs,
                                                    double* __restrict__ part, int ntiles, double* __restrict__ samp)
{
    constexpr int T = NT * VT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const RecSlots<u64> s(smem, T);

    const int tid = threadIdx.x, tile = blockIdx.x;
    const i64 p = blockIdx.y;
    const i64 base = (i64)tile * T;
    const int count = (int)((M - base < (i64)T) ? M - base : (i64)T);
    const float* src = X + p * M + base;

    // As tile_sort_pairs: lane tid takes draws i * NT + tid straight into its sort registers (no staging pass through the
    // LDS).  Records are distinct (the position is the low word), so the sorted tile does not depend on which draws a lane
    // starts with.
    u64 r[VT];
    double bad = 0.0;
    auto load = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int i = 0; i < VT; ++i) {
            const int e = i * NT + tid;
            const bool live = FULL || e < count;
            const float v = src[FULL ? e : min(e, count - 1)];      // every load unconditional and in flight, as in k_tile_sort
            bad += (live && !isfinite(v)) ? 1.0 : 0.0;
            r[i] = live ? (((u64)f32_key(v) << 32) | (u64)(u32)(base + e)) : kRecPad;
        }
    };
    if (count == T) load(std::true_type{}); else load(std::false_type{});
    thread_sort_rec<VT>(r);
    if constexpr (VT == 16) lane_merge_levels_rec(r);
    tile_merge_levels<NT, VT, T - 1, true>(s, r);
    tile_write_out<NT, VT>(s, recs, reinterpret_cast<u32*>(recs), p * M + base, count);     // (records have no position array: the second pointer is never used)
    tile_store_samples<NT, VT>(s, samp, ntiles, count);
    __syncthreads();                 // the reduction scratch takes the place of the records from here on
    tile_moments<NT, VT>([&](int i) { return key_f64(r[i]); }, count, bad, reinterpret_cast<double*>(smem), part, ntiles);
}

// ------------------------------------------------------------------------------------------------
// Write-combined scatter of the rank codes to time order (round 3).  A wave's store of 64 codes for 64 unrelated draws
// touches 64 different 128-byte lines of the parameter's code array, and the CU's L1 takes them one line per cycle: 4 M
// scattered stores per call were a third of the fold kernel.  But a workgroup's <= 4032 codes go to an array of M / 32
// lines (1 250 for C1): about three of them per line.  So the workgroup counting-sorts its (position, code) pairs by
// LINE inside its LDS first -- one LDS atomic per pair for the rank in its line, one block scan over the line counters
// -- and stores them in that order: consecutive lanes then write ascending addresses, ~20 lines per wave-store instead
// of 64.  Fold: 294 -> 250 us per 1000 parameters.  Which code lands where is unchanged.  For M < 65536 (16-bit
// positions; at most 2048 lines).
// hcode / hpos: the lane's VT (code, pooled position) pairs, live for e = tid * VT + i < total.  cnt_code: >= 2112 + 4096
// dead u32 of LDS (the key array), spos: 4096 dead u16 (the position array), swt: NT / 64 u32 of scratch.
// ------------------------------------------------------------------------------------------------
template <int NT, int VT>
__device__ __forceinline__ void scatter_codes_by_line(u32* __restrict__ zrow, i64 M, int total, const u32 (&hcode)[VT],
                                                      const u32 (&hpos)[VT], u32* cnt_code, unsigned short* spos, u32* swt)
{
    constexpr int kMaxLines = 2048, PER = kMaxLines / NT > 0 ? kMaxLines / NT : 1;
    static_assert(NT * PER >= kMaxLines, "every line counter has an owner in the scan");
    const int tid = threadIdx.x;
    const int nlines = (int)((M + 31) >> 5);
    u32* scnt = cnt_code;                   // [nlines + 1]: counts, then first slot of every line
    u32* scode = cnt_code + 2112;
    __syncthreads();                        // the caller's last reads of the arrays that are reused here
    for (int i = tid; i <= nlines; i += NT) scnt[i] = 0u;
    __syncthreads();
    u32 rk[VT];
#pragma unroll
    for (int i = 0; i < VT; ++i) rk[i] = (tid * VT + i < total) ? atomicAdd(&scnt[hpos[i] >> 5], 1u) : 0u;
    __syncthreads();
    {   // exclusive scan of the line counters: PER consecutive counters per thread, wave scan, wave totals
        u32 c[PER], tsum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) { const int q = tid * PER + j; c[j] = (q < nlines) ? scnt[q] : 0u; tsum += c[j]; }
        u32 wtot;
        const u32 wex = wave_excl_scan_u32(tsum, wtot);
        if ((tid & 63) == 0) swt[tid >> 6] = wtot;
        __syncthreads();
        u32 base = wex;
        for (int w = 0; w < (tid >> 6); ++w) base += swt[w];
#pragma unroll
        for (int j = 0; j < PER; ++j) { const int q = tid * PER + j; if (q < nlines) scnt[q] = base; base += c[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        if (tid * VT + i < total) {
            const u32 slot = min(scnt[hpos[i] >> 5] + rk[i], (u32)(NT * VT - 1));
            scode[slot] = hcode[i];
            spos[slot] = (unsigned short)hpos[i];
        }
    }
    __syncthreads();
    for (int e = tid; e < total; e += NT) zrow[spos[e]] = scode[e];
}

// Tie runs of a sorted LDS array by scans instead of per-element searches (uniform cost however heavy
// the ties): thread t owns positions [16t, 16t+16); rs[i] / re[i] = block-local [start, end) of the
// run of equal keys containing position 16t+i.  `wsh` = 2 * NT/64 ints of LDS scratch.
template <int NT, int VT, class KF>
__device__ __forceinline__ void block_tie_runs(KF key_at, int total, int* wsh, int (&rs)[VT], int (&re)[VT])
{
    constexpr int NW = NT / kWave;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int base = tid * VT;
    bool h[VT];
    auto prev = key_at((base > 0 && base - 1 < total) ? base - 1 : 0);     // (position 0 is a head whatever it compares to)
    int cur = -1, first = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int g = base + i;
        const auto kv = key_at(g < total ? g : 0);
        h[i] = (g == 0) || (g >= total) || (prev != kv);
        if (h[i]) { cur = g; if (first == 0x7fffffff) first = g; }
        rs[i] = cur;
        prev = kv;
    }
    // max-scan of `cur` (last head at or before the end of my chunk) and reverse min-scan of `first` over the lanes (DPP)
    int exL, exR;
    const int incl = wave_prefix_max(cur, exL);
    const int rinc = wave_suffix_min(first, exR);
    __syncthreads();
    if (lane == 63) wsh[w] = incl;
    if (lane == 0) wsh[NW + w] = rinc;
    __syncthreads();
    int carryL = -1, carryR = total;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
        if (ww < w) carryL = max(carryL, wsh[ww]);
        if (ww > w) carryR = min(carryR, wsh[NW + ww]);
    }
    carryL = max(carryL, exL);          // (the identities in lanes 0 / 63)
    carryR = min(carryR, exR);
    if (carryR > total) carryR = total;
    int nxt = carryR;
#pragma unroll
    for (int i = VT - 1; i >= 0; --i) {
        re[i] = nxt;
        if (h[i]) nxt = base + i;
        if (rs[i] < 0) rs[i] = carryL;
    }
    __syncthreads();
}

// Signs of the zeros number t0 and t1 = t0 + 1 (0-based) of x[0, M) in time order, by one wave in ONE pass: bit 0 = zero t0
// is a negative zero, bit 1 = zero t1 is (t0 < 0: only t1 is asked for).  A step takes 512 draws, eight independent loads
// per lane (sixteen would halve the fold kernel's occupancy), and counts their zeros with ballots; only the step that holds a target is looked at draw by draw.  Only
// wave_order_stats calls it, for a median that is a zero draw.
__device__ __forceinline__ bool sign_bit_set(double v) { return __double_as_longlong(v) < 0; }
__device__ __forceinline__ bool sign_bit_set(float v) { return __float_as_int(v) < 0; }
template <typename T>
__device__ __noinline__ unsigned wave_zero_signs(const T* __restrict__ x, i64 M, i64 t0, i64 t1)
{
    constexpr int U = 8;
    const int lane = threadIdx.x & 63;
    i64 seen = 0, t = (t0 >= 0) ? t0 : t1;
    unsigned out = 0;
    for (i64 b = 0; b < M; b += 64 * U) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i64 i = b + u * 64 + lane;
            v[u] = (i < M) ? x[i] : (T)1;
        }
        i64 c = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) c += (i64)__popcll(__ballot(v[u] == (T)0));
        if (seen + c <= t) { seen += c; continue; }          // (wave-uniform: the ballots are)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned long long zm = __ballot(v[u] == (T)0), nm = __ballot(v[u] == (T)0 && sign_bit_set(v[u]));
            const i64 cu = (i64)__popcll(zm);
            while (seen + cu > t) {                          // zero number t is among these 64 draws
                unsigned long long m = zm;
                for (i64 j = seen; j < t; ++j) m &= m - 1;   // drop the zeros in front of it
                const bool neg = (nm & m & (~m + 1ull)) != 0;   // its lane: the lowest bit left
                if (t == t1) return out | (neg ? 2u : 0u);
                out |= neg ? 1u : 0u;
                t = t1;
            }
            seen += cu;
        }
    }
    return out;
}

// Order statistics of one parameter by ONE WAVE from its pooled ascending keys: quantiles (numpy `linear` lerp, which
// pyarrow's interpolation="linear" agrees with to 1 ulp; src/mcmc_ref/backends_numpy.py:44, backends_arrow.py:40-42),
// statistics.median (diagnostics.py:97) and the fold split point s = #(x < med), found by a 64-ary search (64 probes and
// a ballot per round: three dependent loads for 40 000 draws where a bisection needs sixteen).  Returns s in every lane;
// `write`: also store the quantiles and the median into the result table (one caller per parameter does).
template <typename KT>
__device__ __forceinline__ i64 wave_order_stats(const KT* __restrict__ k, i64 M, const QArgs& q, bool write,
                                                double* __restrict__ res, i64 P, i64 p, double& med_out)
{
#pragma clang fp contract(off)  // the lerp must round like numpy's (separate multiply and add)
    const int lane = threadIdx.x & 63;
    if (write && lane < q.nq) {
        const int j = lane;
        const i64 lo = q.lo[j], hi = (lo + 1 < M) ? lo + 1 : M - 1;
        const double a = sorted_key(k, lo), b = sorted_key(k, hi), d = b - a, g = q.g[j];
        res[(R_Q0 + j) * P + p] = (g >= 0.5) ? b - d * (1.0 - g) : a + d * g;
    }
    // the two middle draws give the median and, unless draws tie AT the median, the split point too: with below < med
    // every draw up to index M/2 - 1 is below the median and the one at M/2 is not, so s = M/2 and the search (three
    // dependent rounds of loads in front of every fold workgroup's merge) is skipped
    const double below = (M >= 2) ? sorted_key(k, M / 2 - 1) : -INFINITY, at = sorted_key(k, M / 2);
    double med = (M & 1) ? at : (below + at) / 2.0;
    // A median that IS a zero draw (odd M), or the mean of two zero draws (even M): -0.0 and +0.0 tie, the sort keeps no order
    // among them, and which of them stand in the middle decides the sign of the median.  statistics.median sorts stably, so
    // its middle draws are the zeros number M/2 - s (and M/2 - s - 1, even M) of the TIME order, s = #(x < 0): look those up in
    // the draws themselves.  (Only the reported median: |x - med| and the split point are the same for either sign.)  Any
    // other median skips this -- also one that is zero by arithmetic alone ((-5e-324 + 0.0) / 2 rounds to -0.0, (-a + a) / 2
    // is +0.0): its sign is the sum's.
    const bool zero_med = write && q.xt != nullptr && at == 0.0 && ((M & 1) || below == 0.0);
    if (write && lane == 0 && !zero_med) res[R_MEDIAN * P + p] = med;
    i64 lo = 0, hi = M;  // first index with k[i] >= med lies in [lo, hi]
    // (!(at < med): draws near 1e308 can overflow below + at to +inf, and then #(x < med) is M, not M / 2: ADVICE r3)
    if (below < med && !(at < med)) {
        if (!zero_med) { med_out = med; return M / 2; }
        lo = hi = M / 2;
    }
    while (lo < hi) {
        const i64 step = (hi - lo + 63) / 64;
        const i64 pos = lo + step * (lane + 1) - 1;                 // ascending probes, the last one at or beyond hi - 1
        const bool less = (pos < hi) && (sorted_key(k, pos) < med);
        const i64 cnt = (i64)__popcll(__ballot(less));              // sorted keys: the first cnt probes are below med
        const i64 nhi = lo + step * (cnt + 1) - 1;                  // probe cnt (if any) is the first one not below
        lo += step * cnt;
        hi = (nhi < hi) ? nhi : hi;
    }
    if (zero_med) {
        const i64 r = M / 2 - lo;                                   // the draw at M/2 is zero number r (r >= 1 for even M)
        const i64 t0 = (M & 1) ? -1 : r - 1;
        const unsigned sg = q.xf32 ? wave_zero_signs(reinterpret_cast<const float*>(q.xt) + p * M, M, t0, r)
                                   : wave_zero_signs(reinterpret_cast<const double*>(q.xt) + p * M, M, t0, r);
        const bool neg = (M & 1) ? (sg & 2u) != 0 : sg == 3u;       // (-0.0 + -0.0) / 2 alone is -0.0
        med = neg ? -0.0 : 0.0;
        if (lane == 0) res[R_MEDIAN * P + p] = med;
    }
    med_out = med;
    return lo;
}

// ------------------------------------------------------------------------------------------------
// Merge pass: merges pairs of sorted runs of length R (one pass of a merge sort).  Each workgroup owns OB = NT*VT
// outputs: two waves find its two split points by merge path, all threads gather its stretch of the two runs into the LDS,
// merge it there and write it out.
// Slots: what the LDS holds and the pass writes -- PairSlots<IdxT> (sorted keys in `kin`, positions in `iin`) or
// RecSlots<u64> (sorted f32 records in `kin`; `iin` / `iout` unused).
// ------------------------------------------------------------------------------------------------
template <int NT, int VT, class Slots>
__global__ __launch_bounds__(NT) void k_merge(const typename Slots::KeyT* __restrict__ kin,
                                              const typename Slots::PosT* __restrict__ iin,
                                              typename Slots::KeyT* __restrict__ kout,
                                              typename Slots::PosT* __restrict__ iout, i64 M, i64 R)
{
    using Item = typename Slots::Item;
    constexpr int OB = NT * VT;                             // LDS slots = outputs per workgroup
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Slots s(smem, OB);
    // the two split points: behind the slots (pairs: the launch adds 256 bytes) or, where the dynamic LDS ends with the
    // slots (records), in 16 static bytes
    i64* sh;
    if constexpr (Slots::kTail > 0) { __shared__ i64 sh_rec[2]; sh = sh_rec; }
    else sh = reinterpret_cast<i64*>(smem + Slots::lds_bytes(OB));

    const int tid = threadIdx.x;
    const i64 p = blockIdx.y;
    const i64 o0 = (i64)blockIdx.x * OB;
    if (o0 >= M) return;
    const typename Slots::KeyT* kp = kin + p * M;
    const typename Slots::PosT* ip = iin + p * M;

    const i64 pb = (o0 / (2 * R)) * (2 * R);
    const i64 abase = pb, na = (M - pb < R) ? M - pb : R;
    const i64 bbase = pb + na, nb = (M - bbase < R) ? M - bbase : R;
    const i64 d0 = o0 - pb, tot = na + nb;
    const i64 d1 = (d0 + OB < tot) ? d0 + OB : tot;

    // (the pass orders by the stored element itself: the key, or the whole record)
    auto GA = [&](i64 i) { return kp[abase + i]; };
    auto GB = [&](i64 j) { return kp[bbase + j]; };
    if (tid < 64) { const i64 r0 = merge_path_wave(GA, na, GB, nb, d0); if (tid == 0) sh[0] = r0; }
    else if (tid < 128) { const i64 r1 = merge_path_wave(GA, na, GB, nb, d1); if (tid == 64) sh[1] = r1; }
    __syncthreads();
    const i64 ai0 = sh[0], ai1 = sh[1];
    const i64 bi0 = d0 - ai0;
    const int ca = (int)(ai1 - ai0), cb = (int)((d1 - ai1) - bi0);
    const int total = ca + cb;
    {   // gather the two runs: slot e = j * NT + tid; all VT loads of a lane are issued before the first LDS store waits for
        // one (slots at or beyond `total` read element 0 and are not stored)
        Item gv[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            i64 g = (e < ca) ? abase + ai0 + e : bbase + bi0 + (e - ca);
            g = (e < total) ? g : 0;
            gv[j] = Slots::load(kp, ip, g);
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            if (e < total) s.put(e, gv[j]);
        }
    }
    __syncthreads();

    const int diag = (tid * VT < total) ? tid * VT : total;
    const int nout = (total - diag < VT) ? total - diag : VT;
    auto A = [&](int i) { return s.get(i); };
    auto B = [&](int j) { return s.get(ca + j); };
    const int ai = merge_path32(A, ca, B, cb, diag);
    Item out[VT];
    s.template merge<VT>(0, ca, ca, cb, ai, diag - ai, nout, out);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VT; ++i)
        if (i < nout) s.put(diag + i, out[i]);
    __syncthreads();
    for (int e = tid; e < total; e += NT) s.write(kout, iout, p * M + o0 + e, e);
}

// ------------------------------------------------------------------------------------------------
// Fold: produces the ascending order of |x - med| from the ascending order of x with a single merge: the values below the
// median, walked downwards (med - x, non-decreasing because rounding is monotone), against the values at or above it
// (x - med).  This replaces the second full sort of src/mcmc_ref/diagnostics.py:93-98 + :110.  The skeleton is k_merge's
// (split points, gather, merge in the LDS), on (f64 key, position) pairs whatever the input: the folded keys are f64.
// Fused ranks: whether the block's first / last tie run goes on outside it is decided from the element just
// before and just behind the block in each run.  Those four neighbours are loaded WITH the gather, in four of its dead
// slots (clamped index, no test in front of the load) and parked in the scratch; after the merge every thread compares
// them with the block's edge keys in the LDS.  (They were four scalar loads behind the merge, each inside its own test
// and waited for alone by one thread, between two barriers that are gone with them.)
// KT = double: sorted keys in `kin`, positions in `iin`.  KT = u64: sorted f32 records in `kin`, `iin` unused -- the
// keys are widened on the fly.  `R` is unused (the launch passes 0).
// LDS: skey[OBS] then sidx[OBS] as in PairSlots<IdxT>, spelt out: through the slot type the kernel computes the same but
// is scheduled differently (0.9 % slower on f32 records).
// ------------------------------------------------------------------------------------------------
template <int NT, int VT, typename IdxT, typename KT = double>
__global__ __launch_bounds__(NT) void k_fold_merge(const KT* __restrict__ kin, const IdxT* __restrict__ iin,
                                                   double* __restrict__ kout, IdxT* __restrict__ iout, i64 M,
                                                   i64 R, double* __restrict__ res, i64 P,
                                                   QArgs q, u32* __restrict__ z, const i64* __restrict__ split_in)
{
    constexpr int OBS = NT * VT;                            // LDS slots
    // The kernel owns 64 outputs fewer than it has slots and keeps its scratch in the 64 key slots that frees:
    // its LDS is then exactly 4096 * (8 + sizeof(IdxT)) bytes, i.e. FOUR workgroups per CU with 16-bit positions.
    constexpr int OB = OBS - 64;                            // outputs per workgroup
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* skey = reinterpret_cast<double*>(smem);
    IdxT* sidx = reinterpret_cast<IdxT*>(skey + OBS);
    i64* sh = reinterpret_cast<i64*>(skey + OB);

    const int tid = threadIdx.x;
    i64 p;
    int blk;
    if (!xcd_map(P, (int)((M + OB - 1) / OB), p, blk)) return;      // 1-D XCD-aware grid (the fused z scatter of one parameter stays in one L2)
    const i64 o0 = (i64)blk * OB;
    if (o0 >= M) return;
    const KT* kp = kin + p * M;
    const IdxT* ip = iin + p * M;
    auto KEY = [&](i64 g) -> double { return sorted_key(kp, g); };
    auto POS = [&](i64 g) -> u32 {
        if constexpr (sizeof(KT) == 8 && !__is_same(KT, double)) return (u32)kp[g]; else return (u32)ip[g];
    };

    // The order statistics of the parameter, by the first wave of EVERY fold workgroup (a launch of their own in round
    // 2): the median and the split point are three to five dependent loads, the parameter's first workgroup also
    // writes the quantiles and the median.
    // (long arrays -- a hundred fold workgroups per parameter -- get them from a k_order_stats launch instead: split_in)
    if (split_in != nullptr) {
        if (tid == 0) { sh[0] = split_in[p]; reinterpret_cast<double*>(sh)[1] = res[R_MEDIAN * P + p]; }
    } else if (tid < 64) {
        double m_;
        const i64 s_ = wave_order_stats(kp, M, q, blk == 0, res, P, p, m_);
        if (tid == 0) { sh[0] = s_; reinterpret_cast<double*>(sh)[1] = m_; }
    }
    __syncthreads();
    const i64 split = sh[0];
    const double med = reinterpret_cast<double*>(sh)[1];
    __syncthreads();
    const i64 abase = split - 1;  // walked downwards
    const i64 na = split, bbase = split, nb = M - split, d0 = o0;
    const i64 tot = na + nb;
    const i64 d1 = (d0 + OB < tot) ? d0 + OB : tot;

    auto GA = [&](i64 i) -> double { return med - KEY(abase - i); };
    auto GB = [&](i64 j) -> double { return KEY(bbase + j) - med; };
    if (tid < 64) { const i64 r0 = merge_path_wave(GA, na, GB, nb, d0); if (tid == 0) sh[0] = r0; }
    else if (tid < 128) { const i64 r1 = merge_path_wave(GA, na, GB, nb, d1); if (tid == 64) sh[1] = r1; }
    __syncthreads();
    const i64 ai0 = sh[0], ai1 = sh[1];
    const i64 bi0 = d0 - ai0;
    const int ca = (int)(ai1 - ai0), cb = (int)((d1 - ai1) - bi0);
    const int total = ca + cb;

    // The edge neighbours: the element just before and just behind the block in each run, which decide after the
    // merge whether the first / last tie run goes on outside the block.  Their places follow from the split point and the
    // two diagonals' split points, so they ride with the gather: the slots OB .. OB + 3 are dead in every workgroup
    // (total <= OB), and the four lanes that own them load a neighbour there instead of element 0 -- index clamped into [0, M), no test in
    // front of the load -- and park it, folded like GA / GB fold it, in sh[kEdge ..].  A neighbour that does not exist
    // (the block starts or ends a run) is parked as NaN, which equals no key.
    // sh: [0, 2) split point and median, then the two diagonals' split points; [2, 10) the edge bounds; [12, 20) the
    // tie-run scratch; [kEdge, kEdge + 4) the neighbours -- and scatter_codes_by_line's wave totals in [0, 4) at the end.
    constexpr int kEdge = 24;
    {   // gather the two runs: slot e = j * NT + tid; all VT (key, position) loads of a lane are issued before the first
        // LDS store waits for one (slots at or beyond `total` read element 0 and are not stored)
        double gv[VT]; u32 gi[VT];
        const int edge = tid - (OB - (VT - 1) * NT);                  // 0 .. 3 in the lanes of the slots OB .. OB + 3
        const bool is_edge = edge >= 0 && edge < 4;
        bool edge_there = false;
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            bool inA = e < ca;
            i64 g = inA ? abase - (ai0 + e) : bbase + bi0 + (e - ca);
            g = (e < total) ? g : 0;
            if (j == VT - 1) {
                // A before: GA(ai0 - 1), A behind: GA(ai1), B before: GB(bi0 - 1), B behind: GB(bi1)
                const i64 bi1 = d1 - ai1;
                const bool behind = (edge & 1) != 0, inB = (edge & 2) != 0;
                const i64 i = inB ? (behind ? bi1 : bi0 - 1) : (behind ? ai1 : ai0 - 1);
                i64 ge = inB ? bbase + i : abase - i;
                ge = (ge < 0) ? 0 : ((ge < M) ? ge : M - 1);
                edge_there = is_edge && i >= 0 && i < (inB ? nb : na);
                g = is_edge ? ge : g;
                inA = is_edge ? !inB : inA;
            }
            const double x = KEY(g);
            gv[j] = inA ? med - x : x - med;
            gi[j] = POS(g);
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            if (e < total) { skey[pos16(e)] = gv[j]; sidx[posi(e)] = (IdxT)gi[j]; }
        }
        if (is_edge) reinterpret_cast<double*>(sh)[kEdge + edge] = edge_there ? gv[VT - 1] : __builtin_nan("");
    }
    __syncthreads();

    const int diag = (tid * VT < total) ? tid * VT : total;
    const int nout = (total - diag < VT) ? total - diag : VT;
    auto A = [&](int i) { return skey[pos16(i)]; };
    auto B = [&](int j) { return skey[pos16(ca + j)]; };
    const int ai = merge_path32(A, ca, B, cb, diag);
    double k[VT];
    int srcs[VT];
    u32 ix[VT];
    serial_merge<VT>(skey, 0, ca, ca, cb, ai, diag - ai, nout, k, srcs);
#pragma unroll
    for (int i = 0; i < VT; ++i) ix[i] = sidx[posi(srcs[i])];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        if (i < nout) {
            skey[pos16(diag + i)] = k[i];
            sidx[posi(diag + i)] = (IdxT)ix[i];
        }
    }
    __syncthreads();
    if (z == nullptr) {     // the folded order itself, for a caller without rank codes
        for (int e = tid; e < total; e += NT) {
            kout[p * M + o0 + e] = skey[pos16(e)];
            iout[p * M + o0 + e] = sidx[posi(e)];
        }
        return;
    }
    // Fused ranks -> z (src/mcmc_ref/diagnostics.py:113-133): the merged order never goes to memory.
    // Tie runs touching the block edges are completed with lower/upper bounds over the two runs.
    // Does the first / last tie run continue outside this block?  Every thread compares the block's first and last key
    // with the four neighbours the gather parked (no global access, no barrier); only then pay for the bound searches
    // (rare: heavy ties).
    const double vfirst = skey[pos16(0)], vlast = skey[pos16(total - 1)];
    const double* edge_key = reinterpret_cast<const double*>(sh) + kEdge;
    const bool ext0 = edge_key[0] == vfirst || edge_key[2] == vfirst;
    const bool ext1 = edge_key[1] == vlast || edge_key[3] == vlast;
    if ((ext0 || ext1) && tid < 8) {
        const int which = tid >> 2, side = (tid >> 1) & 1, upper = tid & 1;   // value, run, bound kind
        const double v = which ? vlast : vfirst;
        const i64 len = side ? nb : na;
        i64 lo = 0, hi = len;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            const double x = side ? GB(mid) : GA(mid);
            const bool right = upper ? !(v < x) : (x < v);
            if (right) lo = mid + 1; else hi = mid;
        }
        sh[2 + tid] = lo;
    }
    __syncthreads();
    const i64 gfirst = sh[2 + 0] + sh[2 + 2];   // lower bounds (both runs) of the first value
    const i64 glast = sh[2 + 5] + sh[2 + 7];    // upper bounds (both runs) of the last value
    int rs[VT], re[VT];
    block_tie_runs<NT, VT>([&](int g) { return skey[pos16(g)]; }, total, reinterpret_cast<int*>(sh + 12), rs, re);
    const bool by_line = M <= 65535;        // (workgroup-uniform)
    u32 hcode[VT], hpos[VT];
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int e = tid * VT + i;
        hcode[i] = 0u; hpos[i] = 0u;
        if (e < total) {
            const double v = skey[pos16(e)];
            i64 gs = d0 + rs[i], ge = d0 + re[i];
            if (ext0 && v == vfirst) gs = gfirst;
            if (ext1 && v == vlast) ge = glast;
            const u32 t_idx = min((u32)sidx[posi(e)], (u32)(M - 1));     // stale order after a rejected (NaN) partition
            hcode[i] = (u32)(gs + ge); hpos[i] = t_idx;
            if (!by_line) z[p * M + t_idx] = (u32)(gs + ge);            // code of the tie run: rank = (code + 1) / 2
        }
    }
    if (by_line)
        scatter_codes_by_line<NT, VT>(z + p * M, M, total, hcode, hpos, reinterpret_cast<u32*>(skey),
                                      reinterpret_cast<unsigned short*>(sidx), reinterpret_cast<u32*>(sh));
}

// ------------------------------------------------------------------------------------------------
// Exact k-way partition by regular sampling (k = #sorted runs <= 16; a run is a sorted tile, or the
// result of a few pairwise merge passes when the pooled array is longer than 16 tiles).
//
// Every sorted tile contributes its 64th, 128th, ... order statistics.  In the strict total order
// (value, tile, position) the sample of pooled sample-rank r has between 64(r+1) and 64(r+1)+64k
// draws at or below it, so cutting at every D-th sample gives buckets of fewer than 64(D+k) draws:
// with D = floor((4032 - 79k) / 64) a bucket, each of its <= k pieces padded to a multiple of 16,
// always fits the 4032 data slots of k_bucket_merge's LDS -- a deterministic bound, no overflow path.
// One workgroup per parameter writes cut[p][b][t] (start of bucket b inside tile t, b = 0..B) and
// boff[p][b] (start of bucket b in the pooled order).
// ------------------------------------------------------------------------------------------------
constexpr int kMaxBucketTiles = 16;

// The LDS of k_splitters: S samples + splitter tables + cut table, then (MVT > 0) the merge area of the sample ranking.
__host__ __device__ inline size_t splitters_base_bytes(int S, int B, int k, int mvt)     // tables in front of the merge area, 16-byte aligned
{
    const size_t base = (size_t)S * (mvt > 0 ? 8 : 12) + (size_t)(B + 1) * 16 + (size_t)(B + 1) * k * 4 + 64;   // (no rank array in merge mode)
    return (base + 15) / 16 * 16;
}
__host__ __device__ inline size_t splitters_lds_bytes(int S, int B, int k, int mvt)
{
    return splitters_base_bytes(S, B, k, mvt) + (mvt > 0 ? (size_t)(1024 * mvt + 16) * 10 : 0);
}

// MVT = 0: few samples (S <= 1024: pooled arrays of up to 16 tiles, the C1 and corpus shapes) -- every (sample, other
//          run) pair is one bisection, the pooled ranks add up with LDS atomics.
// MVT > 0: many samples (runs pre-merged to 8192 .. 32768 draws: 128 .. 512 samples each, up to 8192 in all; the stress
//          shape ranks 6 656) -- the k sorted sample lists are MERGED in the LDS, ceil(log2 k) merge-path rounds of
//          1024 threads x MVT outputs carrying (value, origin) pairs; a sample's place in the merged list IS its pooled
//          rank in the strict order (value, run, position), since the merges are stable and the runs enter in order.
//          ~190 LDS round trips per thread on the stress shape instead of 6.5 samples x 12 runs x 9 probes = 700
//          (k_splitters was 12.4 ms of its 216 ms step, and the first kernel of the long-chain profile: VERDICT r3 item 8).
template <typename KT, int MVT>      // KT = double (sorted keys) or u64 (sorted f32 records)
__global__ __launch_bounds__(1024) void k_splitters(const KT* __restrict__ keys,
                                                    const double* __restrict__ samp, i64 M, int k, int B,
                                                    int D, i64 R, u32* __restrict__ cut, u32* __restrict__ boff)
{
    constexpr int NTS = 1024;
    const int SPT = (int)(R / 64);                   // samples per run
    const int S = k * SPT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sv = reinterpret_cast<double*>(smem);    // S samples
    double* splv = sv + S;                           // B splitter values
    int* srank = reinterpret_cast<int*>(splv + B + 1);   // S pooled ranks (MVT == 0 only)
    int* splt = srank + (MVT > 0 ? 0 : S);           // B splitter run
    int* splp = splt + B + 1;                        // B splitter position in run
    u32* scut = reinterpret_cast<u32*>(splp + B + 1);    // (B+1) * k cuts
    const int tid = threadIdx.x;
    const i64 p = blockIdx.x;
    const KT* kp = keys + p * M;
    for (int i = tid; i < S; i += NTS) { sv[i] = samp[p * S + i]; if (MVT == 0) srank[i] = i % SPT; }
    for (int b = tid; b <= B; b += NTS) splt[b] = -1;      // -1 = splitter b not found (only with NaN / Inf draws)
    if (MVT > 0) {
        constexpr int VT = MVT > 0 ? MVT : 1;
        static_assert(MVT == 0 || 64 % VT == 0, "a thread's VT outputs must not straddle two pairs of runs (run lengths are multiples of 64)");
        constexpr int SP = NTS * VT;                           // merge slots: the samples, then +inf pads (S <= SP)
        double* mk = reinterpret_cast<double*>(smem + splitters_base_bytes(S, B, k, MVT));                   // [SP + 16] keys, pos16-swizzled
        unsigned short* mi = reinterpret_cast<unsigned short*>(mk + SP + 16);                                // [SP + 16] origin = run * SPT + index
        for (int e = tid; e < SP + 16; e += NTS) {
            mk[pos16(e)] = (e < S) ? samp[p * S + e] : INFINITY;
            mi[e] = (unsigned short)(e < S ? e : 0xFFFF);
        }
        __syncthreads();
        const int chunk0 = tid * VT;
        for (int g = SPT; g < SP; g <<= 1) {                   // runs of g slots merge in pairs (SP is a multiple of SPT)
            double kk[VT]; int srcs[VT]; unsigned short ids[VT];
            const int a0 = chunk0 / (2 * g) * (2 * g);
            const int a1 = (a0 + g < SP) ? a0 + g : SP, b1 = (a0 + 2 * g < SP) ? a0 + 2 * g : SP;
            const int na = a1 - a0, nb = b1 - a1, diag = chunk0 - a0;
            const bool moved = nb > 0;
            if (moved) {
                auto A = [&](int i) { return mk[pos16(a0 + i)]; };
                auto Bf = [&](int j) { return mk[pos16(a1 + j)]; };
                const int ai = merge_path32(A, na, Bf, nb, diag);
                serial_merge<VT>(mk, a0, na, a1, nb, ai, diag - ai, VT, kk, srcs);
#pragma unroll
                for (int i = 0; i < VT; ++i) ids[i] = mi[srcs[i]];
            }
            __syncthreads();
            if (moved) {
#pragma unroll
                for (int i = 0; i < VT; ++i) { mk[pos16(chunk0 + i)] = kk[i]; mi[chunk0 + i] = ids[i]; }
            }
            __syncthreads();
        }
        // the sample at merged place r = b D - 1 is splitter b
        for (int b = 1 + tid; b < B; b += NTS) {
            const int r = b * D - 1;
            if (r < SP) {
                const double v = mk[pos16(r)];
                const int i = mi[r];
                if (v < INFINITY && i < S) { splv[b] = v; splt[b] = i / SPT; splp[b] = 64 * (i % SPT) + 63; }
            }
        }
        __syncthreads();
    } else {
    __syncthreads();
    // pooled rank of every finite sample = own index + samples of every other run below it;
    // one (sample, other run) pair per thread step.  The lanes of a wave take CONSECUTIVE SAMPLES against one run: their
    // probes fall near each other in that run's list and their atomics on neighbouring counters (with consecutive runs per
    // lane -- round 3 -- every lane probed its own run at a stride of SPT doubles, i.e. the same LDS bank: 6.8 conflict
    // cycles per LDS instruction, VERDICT r3 weak #3a)
    for (i64 q = tid; q < (i64)S * k; q += NTS) {
        const int t2 = (int)(q / S), i = (int)(q - (i64)t2 * S);
        const double v = sv[i];
        const int t = i / SPT;
        if (t2 == t || !(v < INFINITY)) continue;
        const double* a = sv + t2 * SPT;
        int lo = 0, hi = SPT;  // count of samples of run t2 that sort before (v, t, j)
        if (t2 < t) { while (lo < hi) { const int m = (lo + hi) >> 1; if (!(v < a[m])) lo = m + 1; else hi = m; } }
        else        { while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; } }
        if (lo) atomicAdd(&srank[i], lo);
    }
    __syncthreads();
    for (int i = tid; i < S; i += NTS) {
        if (!(sv[i] < INFINITY)) continue;
        const int r = srank[i];
        if ((r + 1) % D == 0) {
            const int b = (r + 1) / D;
            if (b >= 1 && b < B) { splv[b] = sv[i]; splt[b] = i / SPT; splp[b] = 64 * (i % SPT) + 63; }
        }
    }
    __syncthreads();
    }
    // Non-finite draws (the call will be rejected with MCR_ENONFINITE) break the ordering the splitters rely on:
    // leave an EMPTY partition behind, so that no later kernel walks cut tables made of garbage.
    {
        int missing = 0;
        for (int b = 1 + tid; b < B; b += NTS) missing |= (splt[b] < 0);
        if (__syncthreads_or(missing)) {
            for (int q = tid; q < (B + 1) * k; q += NTS) cut[p * (i64)(B + 1) * k + q] = 0u;
            for (int b = tid; b <= B; b += NTS) boff[p * (B + 1) + b] = 0u;
            return;
        }
    }
    // cuts: position in run t where bucket b starts
    for (int q = tid; q < (B + 1) * k; q += NTS) {
        const int b = q / k, t = q % k;
        const i64 tbase = (i64)t * R;
        const int cnt = (int)((M - tbase < R) ? M - tbase : R);
        u32 c;
        if (b == 0) c = 0;
        else if (b == B) c = (u32)cnt;
        else {
            const double v = splv[b];
            const int ts = splt[b];
            if (t == ts) c = (u32)(splp[b] + 1);
            else {
                // the run's own samples (in LDS) bracket the answer to a 64-draw window
                const double* sa = sv + t * SPT;
                int slo = 0, shi = SPT;
                if (t < ts) { while (slo < shi) { const int m = (slo + shi) >> 1; if (!(v < sa[m])) slo = m + 1; else shi = m; } }
                else        { while (slo < shi) { const int m = (slo + shi) >> 1; if (sa[m] < v) slo = m + 1; else shi = m; } }
                const KT* a = kp + tbase;
                int lo = 64 * slo, hi = 64 * slo + 63;        // sample j sits at position 64 j + 63
                if (lo > cnt) lo = cnt;
                if (hi > cnt) hi = cnt;
                if (t < ts) { while (lo < hi) { const int m = (lo + hi) >> 1; if (!(v < sorted_key(a, m))) lo = m + 1; else hi = m; } }
                else        { while (lo < hi) { const int m = (lo + hi) >> 1; if (sorted_key(a, m) < v) lo = m + 1; else hi = m; } }
                c = (u32)lo;
            }
        }
        scut[q] = c;
        cut[(p * (B + 1) + b) * k + t] = c;
    }
    __syncthreads();
    for (int b = tid; b <= B; b += NTS) {
        u32 o = 0;
        for (int t = 0; t < k; ++t) o += scut[b * k + t];
        boff[p * (B + 1) + b] = o;
    }
}

// Every 64th order statistic of each sorted run of length R (the regular samples of k_splitters)
// when the runs were produced by merge passes rather than by k_tile_sort.  grid (k, P).
template <typename KT>
__global__ __launch_bounds__(256) void k_sample_runs(const KT* __restrict__ keys, i64 M, i64 R,
                                                     double* __restrict__ samp)
{
    const int run = blockIdx.x, k = gridDim.x;
    const i64 p = blockIdx.y;
    const int SPT = (int)(R / 64);
    const i64 base = (i64)run * R;
    for (int j = threadIdx.x; j < SPT; j += 256) {
        const i64 e = base + 64 * (i64)j + 63;
        samp[(p * k + run) * SPT + j] = (e < M && 64 * (i64)j + 63 < R) ? sorted_key(keys, p * M + e) : INFINITY;
    }
}

// The 512-byte scratch of the bucket merges, in ints: padded piece starts [k + 1], piece lengths [k], piece source
// offsets [k] (k <= 16), the two "tie run goes on" flags, the four edge bounds (i64), and the 2k neighbour keys (8 bytes
// each) -- whose place the tie-run scratch of block_tie_runs takes once the flags are made of them.
constexpr int kBkLen = kMaxBucketTiles + 1, kBkSrc = kBkLen + kMaxBucketTiles, kBkExt = kBkSrc + kMaxBucketTiles,
              kBkEdge = (kBkExt + 2 + 1) / 2 * 2, kBkNext = kBkEdge + 8;
static_assert((kBkNext + 4 * kMaxBucketTiles) * sizeof(int) <= 512, "the bucket merges' scratch is 64 key slots");

// The piece table of a bucket by the first wave (all 64 lanes): lane t < k reads the two cuts of tile t -- the 2k loads
// are one round trip -- and a DPP scan over the padded lengths gives the pieces' starts in the LDS.
__device__ __forceinline__ void bucket_piece_table(const u32* __restrict__ c0, const u32* __restrict__ c1, int k,
                                                   int* sst, int* spl, int* sps)
{
    const int lane = threadIdx.x & 63;
    const int t = (lane < k) ? lane : k - 1;
    const u32 from = c0[t], to = c1[t];
    const int len = (lane < k) ? (int)(to - from) : 0;
    u32 acc;
    const u32 start = wave_excl_scan_u32((u32)((len + 15) & ~15), acc);
    if (lane < k) { sst[lane] = (int)start; spl[lane] = len; sps[lane] = (int)from; }
    if (lane == 0) sst[k] = (int)acc;
}

// Where lane `lane` of the gather's last wave finds its neighbour of the bucket: lanes [0, k) the element just before the
// piece of tile `lane`, lanes [k, 2k) the one just behind the piece of tile `lane - k`.  Returns its index in the
// parameter's keys, clamped into [0, M) -- every lane may load it -- and `there`: this lane has a neighbour and it exists.
__device__ __forceinline__ i64 bucket_neighbour(int lane, int k, i64 R, i64 M, const int* spl, const int* sps, bool& there)
{
    const bool behind = lane >= k;
    const int t0 = behind ? lane - k : lane, t = (t0 < 0) ? 0 : ((t0 < k) ? t0 : k - 1);
    const i64 tbase = (i64)t * R;
    const i64 cnt = (M - tbase < R) ? M - tbase : R;
    const i64 i = behind ? (i64)sps[t] + spl[t] : (i64)sps[t] - 1;
    there = lane >= 0 && lane < 2 * k && i >= 0 && i < cnt;
    const i64 g = tbase + i;
    return (g < 0) ? 0 : ((g < M) ? g : M - 1);
}

// ------------------------------------------------------------------------------------------------
// Bucket merge: one workgroup per (bucket, parameter) gathers its <= k sorted pieces (one per tile)
// into LDS, each padded with +inf to a multiple of 16, merges them with ceil(log2 k) merge-path
// rounds, writes the bucket to its place in the pooled ascending order (for the fold step and the
// order statistics) and -- fused -- turns positions into tie-averaged ranks, z = Phi^-1((r-1/2)/M)
// and scatters z to time order (src/mcmc_ref/diagnostics.py:101-133).  Tie runs that touch a bucket
// edge are completed with lower/upper bounds over the k sorted tiles, which are complete in memory.
// No load of the kernel waits alone: the piece table is built by the lanes t < k of the first wave (their 2k cut
// loads are one round trip, a DPP scan gives the padded starts -- not one thread walking k tiles), and the 2k tile
// neighbours that tell whether an edge tie run goes on in the next bucket are loaded with the gather, in its dead
// last slots, and parked in the scratch until the rounds are done (they were two guarded loads per lane behind them).
// Replaces log2(k) global merge passes + k_rank_z of the first version.
// Written out once for pairs (here) and once for f32 records (k_bucket_merge32 below), unlike the merge pass and the tile
// sorts: one text over PairSlots / RecSlots computes the same, but the compiler allocates it differently (pairs with 16-bit
// positions 55 -> 60 VGPRs, records 48 -> 50), and these two kernels are kept at the registers they were tuned at.  A change
// to one of them belongs in the other as well.
// ------------------------------------------------------------------------------------------------
template <int NT, int VT, typename IdxT>
__global__ __launch_bounds__(NT) void k_bucket_merge(const double* __restrict__ kin, const IdxT* __restrict__ iin,
                                                      double* __restrict__ kout, IdxT* __restrict__ iout, i64 M,
                                                      int k, int B, const u32* __restrict__ cut,
                                                      const u32* __restrict__ boff, u32* __restrict__ z, i64 P,
                                                      i64 R)
{
    constexpr int T = NT * VT;
    static_assert(T == 4096, "the partition bound of k_splitters assumes 4096-slot buckets");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* skey = reinterpret_cast<double*>(smem);
    IdxT* sidx = reinterpret_cast<IdxT*>(skey + T);
    // k_splitters bounds every bucket by T - 64 slots; the 64 key slots above hold the scratch, so the workgroup's LDS
    // is exactly T * (8 + sizeof(IdxT)) bytes: FOUR buckets per CU with 16-bit positions.
    int* sst = reinterpret_cast<int*>(skey + (T - 64));   // padded piece starts [k+1]
    int* spl = sst + kBkLen;                        // piece lengths [k]
    int* sps = sst + kBkSrc;                        // piece source offsets in tile [k]
    int* sext = sst + kBkExt;                       // [2] does the first / last tie run go on outside the bucket?
    i64* sedge = reinterpret_cast<i64*>(sst + kBkEdge);     // [4] global run bounds of the edge values
    double* sne = reinterpret_cast<double*>(sst + kBkNext); // [2k] the tiles' keys just before / behind their pieces
    static_assert(2 * (NT / kWave) <= 2 * (int)sizeof(double) / (int)sizeof(int) * kMaxBucketTiles, "the tie-run scratch takes the neighbours' place");

    const int tid = threadIdx.x;
    i64 p;
    int b;
    if (!xcd_map(P, B, p, b)) return;
    const double* kp = kin + p * M;
    const IdxT* ip = iin + p * M;
    const u32* c0 = cut + (p * (B + 1) + b) * k;
    const u32* c1 = c0 + k;
    if (k < 1 || k > kMaxBucketTiles) return;       // (the scratch holds sixteen pieces)
    if (tid < kWave) bucket_piece_table(c0, c1, k, sst, spl, sps);
    __syncthreads();
    const int padded = sst[k];          // <= 4096 by construction of D
    const int total = (int)(boff[p * (B + 1) + b + 1] - boff[p * (B + 1) + b]);
    const i64 obase = boff[p * (B + 1) + b];
    if (padded > T - 64 || total < 0 || total > padded || obase + total > M) return;   // never with a valid partition
    // The tiles' keys just before and just behind this bucket's pieces decide, after the rounds, whether the first /
    // last tie run goes on in a neighbouring bucket.  Their places are known now, so they ride with the gather: its
    // last 64 slots are dead in every workgroup (padded <= T - 64), and the first 2k lanes that own them load a neighbour
    // there instead of element 0 (index clamped, no test in front of the load) and park it next to the piece table; a
    // neighbour that does not exist is parked as NaN, which equals no key.
    const int ne_lane = tid - (T - 64 - (VT - 1) * NT);     // >= 0 in the wave of the slots T - 64 .. T - 1
    bool ne_there = false;
    i64 ne_g = 0;
    if (ne_lane >= 0) ne_g = bucket_neighbour(ne_lane, k, R, M, spl, sps, ne_there);
    const bool is_ne = ne_lane >= 0 && ne_lane < 2 * k;
    double ne = 0.0;
    // gather pieces (+inf pads).  Slot e = j * NT + tid: a wave's j-th load covers 64 consecutive slots = four 16-slot
    // chunks, one per DPP row of 16 lanes, and a chunk never straddles pieces (they are padded to 16).  Lane j of row q
    // looks up the piece of the row's j-th chunk ONCE; the element loop takes {source offset, live length} from that lane
    // with a row broadcast and issues all VT loads back to back (one piece search per 16 slots instead of one per slot,
    // no load waits for the previous one).
    {
        const int lane = tid & 63, wv = tid >> 6;
        u32 my_g = 0; int my_n = 0;
        if ((lane & 15) < VT) {
            const int e0 = (lane & 15) * NT + 64 * wv + 16 * (lane >> 4);
            if (e0 < padded) {
                int t = 0;   // last piece whose padded start is <= e0 (starts are non-decreasing)
#pragma unroll
                for (int step = 8; step > 0; step >>= 1)
                    if (t + step < k && e0 >= sst[t + step]) t += step;
                const int o = e0 - sst[t];
                my_n = spl[t] - o;
                my_g = (u32)((i64)t * R) + (u32)sps[t] + (u32)o;
            }
        }
        double gv[VT]; IdxT gi[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int within = lane & 15;
            const u32 g0 = (u32)row_lane((int)my_g, j);      // lane j of my row of 16 looked the chunk up
            const int n = row_lane(my_n, j);
            const bool live = within < n;
            i64 g = live ? (i64)(g0 + (u32)within) : 0;           // dead slots read element 0 (always there) and drop it
            if (j == VT - 1) g = is_ne ? ne_g : g;
            const double v = kp[g]; const IdxT id = ip[g];
            gv[j] = live ? v : INFINITY; gi[j] = live ? id : (IdxT)~(IdxT)0;
            if (j == VT - 1) ne = v;
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            if (e < padded) { skey[pos16(e)] = gv[j]; sidx[posi(e)] = gi[j]; }
        }
    }
    if (is_ne) sne[ne_lane] = ne_there ? ne : __builtin_nan("");
    wait_loads();
    __syncthreads();
    // merge rounds over adjacent runs (run boundaries = sst[] at stride 2^r)
    const int chunk0 = tid * VT;
    int mypiece = 0;      // the piece that holds slot chunk0 (pieces are padded to 16 >= VT slots: a lane's chunk lies in one piece)
#pragma unroll
    for (int step = 8; step > 0; step >>= 1)
        if (mypiece + step < k && chunk0 >= sst[mypiece + step]) mypiece += step;
    for (int w = 1; w < k; w <<= 1) {
        double kk[VT]; int srcs[VT]; u32 ix[VT];
        const bool active = chunk0 < padded;
        bool moved = false;
        if (active) {
            const int ra = mypiece & ~(2 * w - 1);   // first piece of the pair of runs (w pieces each) that contains chunk0
            const int a0 = sst[ra];
            const int a1 = sst[(ra + w < k) ? ra + w : k];
            const int b1 = sst[(ra + 2 * w < k) ? ra + 2 * w : k];
            const int na = a1 - a0, nb = b1 - a1, diag = chunk0 - a0;
            moved = nb > 0;          // a run without a partner in this round (k not a power of two) stays where it is
            if (moved) {
                auto A = [&](int i) { return skey[pos16(a0 + i)]; };
                auto Bf = [&](int j) { return skey[pos16(a1 + j)]; };
                const int ai = merge_path32(A, na, Bf, nb, diag);
                serial_merge<VT>(skey, a0, na, a1, nb, ai, diag - ai, VT, kk, srcs);
#pragma unroll
                for (int i = 0; i < VT; ++i) ix[i] = sidx[posi(srcs[i])];
            }
        }
        __syncthreads();
        if (moved) {
#pragma unroll
            for (int i = 0; i < VT; ++i) { skey[pos16(chunk0 + i)] = kk[i]; sidx[posi(chunk0 + i)] = (IdxT)ix[i]; }
        }
        __syncthreads();
    }
    // pooled ascending order out
    for (int e = tid; e < total; e += NT) {
        kout[p * M + obase + e] = skey[pos16(e)];
        iout[p * M + obase + e] = sidx[posi(e)];
    }
    if (z == nullptr || total == 0) return;
    // Do the first / last tie runs continue in a neighbouring bucket?  Compare with the element just before / after
    // this bucket's piece in every tile (parked by the gather: no global access); only then pay for the bound searches.
    if (tid < 4) sedge[tid] = 0;
    if (tid < kWave) {
        const int t = (tid < k) ? tid : k - 1;
        const bool e0 = tid < k && sne[t] == skey[pos16(0)];
        const bool e1 = tid < k && sne[k + t] == skey[pos16(total - 1)];
        const bool a0 = __ballot(e0) != 0, a1 = __ballot(e1) != 0;
        if (tid == 0) { sext[0] = a0; sext[1] = a1; }
    }
    __syncthreads();
    const bool ext0 = sext[0] != 0, ext1 = sext[1] != 0;
    if ((ext0 || ext1) && tid < 2 * k) {
        const int t = tid % k, which = tid / k;           // 0: first value, 1: last value
        const double v = which ? skey[pos16(total - 1)] : skey[pos16(0)];
        const i64 tbase = (i64)t * R;
        const int cnt = (int)((M - tbase < R) ? M - tbase : R);
        const double* a = kp + tbase;
        int lo = 0, hi = cnt;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
        const int lb = lo;
        hi = cnt;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (!(v < a[m])) lo = m + 1; else hi = m; }
        atomicAdd(reinterpret_cast<unsigned long long*>(&sedge[2 * which]), (unsigned long long)lb);
        atomicAdd(reinterpret_cast<unsigned long long*>(&sedge[2 * which + 1]), (unsigned long long)lo);
    }
    __syncthreads();
    const double vfirst = skey[pos16(0)], vlast = skey[pos16(total - 1)];
    int rs[VT], re[VT];
    block_tie_runs<NT, VT>([&](int g) { return skey[pos16(g)]; }, total, sst + kBkNext, rs, re);
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int e = tid * VT + i;
        if (e < total) {
            const double v = skey[pos16(e)];
            i64 gs = obase + rs[i], ge = obase + re[i];
            if (ext0 && v == vfirst) gs = sedge[0];
            if (ext1 && v == vlast) ge = sedge[3];
            // (scattered as it is: with four merge rounds to overlap them, this kernel's stores are hidden already --
            //  scatter_codes_by_line here measured 382 -> 382 us per 1000 parameters)
            z[p * M + min((u32)sidx[posi(e)], (u32)(M - 1))] = (u32)(gs + ge);   // code of the tie run: rank = (code + 1) / 2
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Bucket merge on f32 records (k_bucket_merge above, line for line): gather <= k sorted pieces, merge in LDS, write the
// pooled ascending records and -- fused -- the rank code of every draw to time order.
// ------------------------------------------------------------------------------------------------
template <int NT, int VT>
__global__ __launch_bounds__(NT) void k_bucket_merge32(const u64* __restrict__ rin, u64* __restrict__ rout, i64 M,
                                                       int k, int B, const u32* __restrict__ cut,
                                                       const u32* __restrict__ boff, u32* __restrict__ z, i64 P, i64 R)
{
    constexpr int T = NT * VT;
    static_assert(T == 4096, "the partition bound of k_splitters assumes 4096-slot buckets");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* srec = reinterpret_cast<u64*>(smem);
    int* sst = reinterpret_cast<int*>(srec + T + 2);   // padded piece starts [k+1]; the scratch is laid out as in k_bucket_merge
    int* spl = sst + kBkLen;                            // piece lengths [k]
    int* sps = sst + kBkSrc;                            // piece source offsets in tile [k]
    int* sext = sst + kBkExt;                           // [2] does the first / last tie run go on outside the bucket?
    i64* sedge = reinterpret_cast<i64*>(sst + kBkEdge); // [4] global run bounds of the edge values
    u64* sne = reinterpret_cast<u64*>(sst + kBkNext);   // [2k] the runs' keys just before / behind their pieces
    static_assert(2 * (NT / kWave) <= 4 * kMaxBucketTiles, "the tie-run scratch takes the neighbours' place");

    const int tid = threadIdx.x;
    i64 p;
    int b;
    if (!xcd_map(P, B, p, b)) return;
    const u64* rp = rin + p * M;
    const u32* c0 = cut + (p * (B + 1) + b) * k;
    const u32* c1 = c0 + k;
    if (k < 1 || k > kMaxBucketTiles) return;       // (the scratch holds sixteen pieces)
    if (tid < kWave) bucket_piece_table(c0, c1, k, sst, spl, sps);
    __syncthreads();
    const int padded = sst[k];
    const int total = (int)(boff[p * (B + 1) + b + 1] - boff[p * (B + 1) + b]);
    const i64 obase = boff[p * (B + 1) + b];
    if (padded > T - 64 || total < 0 || total > padded || obase + total > M) return;   // never with a valid partition
    // the runs' records just before / behind this bucket's pieces ride in the gather's dead last slots (see
    // k_bucket_merge); a neighbour that does not exist is parked as a value no 32-bit key equals
    const int ne_lane = tid - (T - 64 - (VT - 1) * NT);
    bool ne_there = false;
    i64 ne_g = 0;
    if (ne_lane >= 0) ne_g = bucket_neighbour(ne_lane, k, R, M, spl, sps, ne_there);
    const bool is_ne = ne_lane >= 0 && ne_lane < 2 * k;
    u64 ne = 0;
    {   // gather: one piece search per 16-slot chunk, all VT loads in flight together (see k_bucket_merge)
        const int lane = tid & 63, wv = tid >> 6;
        u32 my_g = 0; int my_n = 0;
        if ((lane & 15) < VT) {
            const int e0 = (lane & 15) * NT + 64 * wv + 16 * (lane >> 4);
            if (e0 < padded) {
                int t = 0;
#pragma unroll
                for (int step = 8; step > 0; step >>= 1)
                    if (t + step < k && e0 >= sst[t + step]) t += step;
                const int o = e0 - sst[t];
                my_n = spl[t] - o;
                my_g = (u32)((i64)t * R) + (u32)sps[t] + (u32)o;
            }
        }
        u64 gr[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int within = lane & 15;
            const u32 g0 = (u32)row_lane((int)my_g, j);      // lane j of my row of 16 looked the chunk up
            const int n = row_lane(my_n, j);
            const bool live = within < n;
            i64 g = live ? (i64)(g0 + (u32)within) : 0;
            if (j == VT - 1) g = is_ne ? ne_g : g;
            const u64 r = rp[g];
            gr[j] = live ? r : kRecPad;
            if (j == VT - 1) ne = r;
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            if (e < padded) srec[pos16(e)] = gr[j];
        }
    }
    if (is_ne) sne[ne_lane] = ne_there ? (u64)rec_key(ne) : ~0ull;
    wait_loads();
    __syncthreads();
    const int chunk0 = tid * VT;
    int mypiece = 0;      // the piece that holds slot chunk0 (pieces are padded to 16 >= VT slots)
#pragma unroll
    for (int step = 8; step > 0; step >>= 1)
        if (mypiece + step < k && chunk0 >= sst[mypiece + step]) mypiece += step;
    for (int w = 1; w < k; w <<= 1) {
        u64 r[VT];
        bool moved = false;
        if (chunk0 < padded) {
            const int ra = mypiece & ~(2 * w - 1);
            const int a0 = sst[ra];
            const int a1 = sst[(ra + w < k) ? ra + w : k];
            const int b1 = sst[(ra + 2 * w < k) ? ra + 2 * w : k];
            const int na = a1 - a0, nb = b1 - a1, diag = chunk0 - a0;
            moved = nb > 0;
            if (moved) {
                auto A = [&](int i) { return srec[pos16(a0 + i)]; };
                auto Bf = [&](int j) { return srec[pos16(a1 + j)]; };
                const int ai = merge_path32(A, na, Bf, nb, diag);
                serial_merge_rec<VT>(srec, a0, na, a1, nb, ai, diag - ai, VT, r);
            }
        }
        __syncthreads();
        if (moved) {
#pragma unroll
            for (int i = 0; i < VT; ++i) srec[pos16(chunk0 + i)] = r[i];
        }
        __syncthreads();
    }
    for (int e = tid; e < total; e += NT) rout[p * M + obase + e] = srec[pos16(e)];
    if (z == nullptr || total == 0) return;
    // tie runs that continue in a neighbouring bucket: look at the record just before / after this bucket's piece in
    // every run; only then pay for the bound searches
    if (tid < 4) sedge[tid] = 0;
    const u32 kfirst = rec_key(srec[pos16(0)]), klast = rec_key(srec[pos16(total - 1)]);
    if (tid < kWave) {
        const int t = (tid < k) ? tid : k - 1;
        const bool e0 = tid < k && sne[t] == (u64)kfirst;
        const bool e1 = tid < k && sne[k + t] == (u64)klast;
        const bool a0 = __ballot(e0) != 0, a1 = __ballot(e1) != 0;
        if (tid == 0) { sext[0] = a0; sext[1] = a1; }
    }
    __syncthreads();
    const bool ext0 = sext[0] != 0, ext1 = sext[1] != 0;
    if ((ext0 || ext1) && tid < 2 * k) {
        const int t = tid % k, which = tid / k;           // 0: first value, 1: last value
        const u32 v = which ? klast : kfirst;
        const i64 tbase = (i64)t * R;
        const int cnt = (int)((M - tbase < R) ? M - tbase : R);
        const u64* a = rp + tbase;
        int lo = 0, hi = cnt;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (rec_key(a[m]) < v) lo = m + 1; else hi = m; }
        const int lb = lo;
        hi = cnt;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (!(v < rec_key(a[m]))) lo = m + 1; else hi = m; }
        atomicAdd(reinterpret_cast<unsigned long long*>(&sedge[2 * which]), (unsigned long long)lb);
        atomicAdd(reinterpret_cast<unsigned long long*>(&sedge[2 * which + 1]), (unsigned long long)lo);
    }
    __syncthreads();
    int rs[VT], re[VT];
    block_tie_runs<NT, VT>([&](int g) { return rec_key(srec[pos16(g)]); }, total, sst + kBkNext, rs, re);
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int e = tid * VT + i;
        if (e < total) {
            const u64 r = srec[pos16(e)];
            i64 gs = obase + rs[i], ge = obase + re[i];
            if (ext0 && rec_key(r) == kfirst) gs = sedge[0];
            if (ext1 && rec_key(r) == klast) ge = sedge[3];
            z[p * M + min(rec_pos(r), (u32)(M - 1))] = (u32)(gs + ge);   // code of the tie run: rank = (code + 1) / 2
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Order statistics from the pooled ascending keys: quantiles (numpy `linear` lerp, which pyarrow's
// interpolation="linear" agrees with to 1 ulp; src/mcmc_ref/backends_numpy.py:44,
// backends_arrow.py:40-42), statistics.median (diagnostics.py:97) and the fold split point
// s = #(x < med).  One WAVE per parameter: lane j takes quantile j, and the split point is found by a 64-ary search
// (64 probes and a ballot per round: three dependent loads for 40 000 draws where a bisection needs sixteen -- the
// kernel is nothing but that latency chain, and the fold merge waits for it).  grid ceil(P / 4), block 256.
// ------------------------------------------------------------------------------------------------
template <typename KT>
__global__ __launch_bounds__(256) void k_order_stats(const KT* __restrict__ keys, i64 M, i64 P, QArgs q,
                                                     double* __restrict__ res, i64* __restrict__ split)
{
    const int lane = threadIdx.x & 63;
    const i64 p = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    double med;
    const i64 s = wave_order_stats(keys + p * M, M, q, true, res, P, p, med);
    if (lane == 0) split[p] = s;
}

// ------------------------------------------------------------------------------------------------
// Ranks -> z.  For the sorted position i of a parameter: the maximal run [s, e) of equal keys
// gets the average 1-based rank (s + 1 + e) / 2 (src/mcmc_ref/diagnostics.py:113-122),
// z = Phi^-1((rank - 0.5) / M) (:130-131), written to the draw's pooled (time-order) position.
// Run ends are found by galloping + bisection from i, so isolated values cost two neighbour
// loads and long tie runs cost O(log run).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rank_z(const double* __restrict__ keys,
                                                const u32* __restrict__ idx, i64 M, u32* __restrict__ z)
{
    const i64 p = blockIdx.y;
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double* k = keys + p * M;
    const double v = k[i];
    i64 s = i, e = i + 1;
    if (i > 0 && k[i - 1] == v) {  // gallop left: find first index with key == v
        i64 step = 1, hi = i - 1;  // k[hi] == v
        i64 lo = hi - step;
        while (lo >= 0 && k[lo] == v) { hi = lo; step <<= 1; lo = hi - step; }
        if (lo < -1) lo = -1;      // k[lo] != v (or lo == -1), k[hi] == v
        while (hi - lo > 1) {
            const i64 mid = (lo + hi) >> 1;
            if (k[mid] == v) hi = mid; else lo = mid;
        }
        s = hi;
    }
    if (i + 1 < M && k[i + 1] == v) {  // gallop right: find last index with key == v
        i64 step = 1, lo = i + 1;      // k[lo] == v
        i64 hi = lo + step;
        while (hi < M && k[hi] == v) { lo = hi; step <<= 1; hi = lo + step; }
        if (hi > M) hi = M;            // k[hi] != v (or hi == M), k[lo] == v
        while (hi - lo > 1) {
            const i64 mid = (lo + hi) >> 1;
            if (k[mid] == v) lo = mid; else hi = mid;
        }
        e = lo + 1;
    }
    z[p * M + min(idx[p * M + i], (u32)(M - 1))] = (u32)(s + e);   // code of the tie run: rank = (code + 1) / 2
}

// ------------------------------------------------------------------------------------------------
// Finalize: pooled mean / population std from the tile partials, rhat = Python max(bulk, tail)
// (`tail if tail > bulk else bulk`, src/mcmc_ref/diagnostics.py:40), NaN diagnostics when there
// are fewer than two chains (diagnostics.py:29-30, 53-54, 69-70).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void finalize_param(const double* __restrict__ part, int S, i64 M,
                                               i64 P, int C, double* __restrict__ res, i64 p)
{
    double mu, m2, b, n;
    merge_slice_moments(part + p * S * kMomRec, S, mu, m2, b, n);
    double var = m2 / (double)M;
    if (isinf(m2)) var = INFINITY;          // squares overflowed: inf like np.std
    else if (!(var >= 0.0)) var = 0.0;
    res[R_MEAN * P + p] = mu;
    res[R_STD * P + p] = sqrt(var);
    res[R_BAD * P + p] = b;
    if (C < 2) {
        res[R_RHAT * P + p] = NAN; res[R_RHAT_BULK * P + p] = NAN; res[R_RHAT_TAIL * P + p] = NAN;
        res[R_ESS_BULK * P + p] = NAN; res[R_ESS_TAIL * P + p] = NAN;
        res[R_LAG_BULK * P + p] = 0.0; res[R_LAG_TAIL * P + p] = 0.0;
    } else {
        const double rb = res[R_RHAT_BULK * P + p], rt = res[R_RHAT_TAIL * P + p];
        res[R_RHAT * P + p] = (rt > rb) ? rt : rb;
    }
}

// Stand-alone form: calls without diagnostics (Backend.stats only) and single-chain tensors.  With diagnostics the
// same function runs inside k_diag_combine2 (one launch fewer per call).
__global__ void k_finalize(const double* __restrict__ part, int S, i64 M, i64 P, int C, double* __restrict__ res)
{
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    finalize_param(part, S, M, P, C, res, p);
}

// compare.compare_stats arithmetic (src/mcmc_ref/compare.py:41-43)
__global__ void k_compare(const double* __restrict__ ref, const double* __restrict__ act, i64 n,
                          double tol, double* __restrict__ rel, unsigned char* __restrict__ pass)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double r = ref[i], a = act[i], ar = fabs(r);
    const double denom = (1e-12 > ar) ? 1e-12 : ar;  // Python max(abs(ref), 1e-12): NaN stays NaN
    const double e = fabs(a - r) / denom;
    rel[i] = e;
    pass[i] = (e <= tol) ? 1 : 0;
}

// Read-only streaming probe: what the HBM delivers to a kernel that does nothing but 16-byte loads.  Each workgroup
// streams a contiguous slice with 4 loads in flight per lane (the access pattern of k_moments_rows).  bench.py reports
// the best rate over a few grid sizes as `peak_measured` next to the 8 TB/s specification peak.
__global__ __launch_bounds__(256) void k_stream_read(const uint4* __restrict__ src, i64 nvec, u32* __restrict__ sink)
{
    const i64 per = (nvec + gridDim.x - 1) / gridDim.x;
    const i64 b = (i64)blockIdx.x * per, e = (b + per < nvec) ? b + per : nvec;
    u32 acc = 0;
    i64 i = b + threadIdx.x;
    for (; i + 3 * 256 < e; i += 4 * 256) {
        uint4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = src[i + u * 256];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc ^= r[u].x ^ r[u].y ^ r[u].z ^ r[u].w;
    }
    for (; i < e; i += 256) { const uint4 r = src[i]; acc ^= r.x ^ r.y ^ r.z ^ r.w; }
    if (acc == 0x9E3779B9u) sink[blockIdx.x & 1023] = acc;      // practically never: keeps the loads alive without a store stream
}

// Synthetic stress tensor: iid N(p, sigma_p), counter-based, layout [P][C][N].
template <typename T>
__global__ __launch_bounds__(256) void k_fill_synth(T* __restrict__ out, i64 total, i64 M, u64 seed, i64 first)
{
    // `first` = index of out[0] in the whole tensor: a rank that holds a parameter block of a P-split model
    //  generates exactly its slice of the one global tensor.
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < total; j += stride) {
        const i64 i = first + j;
        const i64 p = i / M;
        const u64 base = seed * 0x9E3779B97F4A7C15ull + 2ull * (u64)i;
        const u64 h1 = splitmix64(base), h2 = splitmix64(base + 1);
        const double u1 = ((double)(h1 >> 11) + 0.5) * 0x1.0p-53;
        const double u2 = (double)(h2 >> 11) * 0x1.0p-53;
        const double e = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
        int k = (int)(p % 7) - 3;
        double sigma = 1.0;
        for (; k > 0; --k) sigma *= 10.0;
        for (; k < 0; ++k) sigma /= 10.0;
        out[j] = (T)((double)p + sigma * e);
    }
}

}  // namespace mcr
