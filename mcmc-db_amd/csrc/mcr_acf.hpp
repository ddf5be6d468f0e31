// mcr_acf.hpp -- per-chain autocorrelation functions of the RAW draws up to a maximum lag, the within-chain pooled ACF per
// parameter, and the integrated autocorrelation time with Sokal's automatic window (posterior::autocorrelation, ArviZ's
// autocorr, emcee's integrated_time).  The definition is in mcmcref_hip.h.  Nothing here is shared with the ESS kernels
// (k_acov_seg / k_tier3 / the FFT tier): those work on rank-normalised z, sum over chains and stop at the truncation lag.
//
//   m = (sum_i x_i) / N     d_i = x_i - m     S_l = sum_{i < N-l} d_i d_{i+l}     gamma_l = S_l / N  (unbiased: / (N - l))
//   rho_l = gamma_l / gamma_0     tau_W = 2 (rho_0 + .. + rho_W) - 1     window = the first W with W >= window_c tau_W
//
// ONE order of summation, a function of (N, l) and C alone:
//   m      lane j of 64 adds x_j, x_{j+64}, .. in index order; the 64 sums meet in an xor tree (32, 16, .. 1), that is
//          v_j += v_{j+o} for j < o, o = 32, 16, .. 1; m = v_0 / N.
//   S_l    the draws are cut into blocks of kAcfBlock consecutive i.  Block b, lag l: acc = +0, then
//          acc = fma(d_i, d_{i+l}, acc) for i = b B .. min(b B + B, N - l) - 1 in ascending order (an explicit fma: the
//          compiler's contraction choices play no part).  S_l = ((0 + acc_0) + acc_1) + .. in block order, over all
//          ceil(N / B) blocks (one without a product of the lag adds +0).
//   pooled gamma-bar_l = ((0 + gamma_{l,0}) + gamma_{l,1} + ..) / C in chain order.
//   tau    the running sum left to right from +0.
// The device pads a chain with d = 0 past its end and lets every thread of k_acf_products run whole steps of 4 draws:
// fma(d, 0, acc) leaves the bits of acc (acc is never -0: it starts at +0), so the padding is not part of the order.
// acf_gamma, acf_rho, acf_tau_scan and acf_lane_sum are the text of both sides; mcr_autocorr_host runs them with the
// block loop above and uses only +, -, x, / and fma: it equals the device in bits.
#pragma once
#include <cmath>
#include "mcr_device.hpp"

namespace mcr {

constexpr i64 kAcfMaxLag = 4096;              // MCR_ACF_MAX_LAG
constexpr int kAcfBlock = 512;                // MCR_ACF_BLOCK: consecutive draws of one fma chain
constexpr int kAcfNT = 256;                   // threads of a k_acf_products workgroup (fewer for a chain of one block and few lags)
constexpr int kAcfLags = 4;                   // consecutive lags of a thread
constexpr int kAcfDraws = 4;                  // draws of a step: 16 fma for 4 broadcast and 4 strided doubles read from LDS
constexpr int kAcfMaxSpan = 8;                // draw blocks of a workgroup at most (32 KB of deviations)
constexpr int kAcfSlack = 4;                  // doubles behind a staged stream that the last step's prefetch may touch
constexpr int kAcfFinNT = 256;                // threads of k_acf_finish / k_acf_pool

// ---- the text of both sides -----------------------------------------------------------------------
// Lane `lane` of 64: its draws in index order.  *bad counts the non-finite ones.
__host__ __device__ inline double acf_lane_sum(const double* __restrict__ x, i64 N, int lane, i64* bad)
{
    double s = 0.0;
    i64 nb = 0;
#pragma unroll 4
    for (i64 i = lane; i < N; i += kWave) {
        const double v = x[i];
        s += v;
        nb += v - v == 0.0 ? 0 : 1;                                 // (NaN and +-Inf: v - v is NaN)
    }
    *bad += nb;
    return s;
}
__host__ __device__ inline double acf_gamma(double S, i64 N, i64 l, bool unbiased)
{
    return S / (double)(unbiased ? N - l : N);
}
__host__ __device__ inline double acf_rho(double g, double g0) { return g0 == 0.0 ? NAN : g / g0; }
// Sokal's window on rho[0 .. L]: the first W with W >= wc * tau_W; none: window = -1 and tau = tau_L.  Eight values are
// read ahead of the serial sum (the reads do not wait for one another).
__host__ __device__ inline void acf_tau_scan(const double* rho, i64 L, double wc, double& tau, i64& window)
{
    double s = 0.0, t = NAN;
    window = -1;
    for (i64 w0 = 0; w0 <= L; w0 += 8) {
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = w0 + k <= L ? rho[w0 + k] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (w0 + k > L) break;
            s += r[k];
            t = 2.0 * s - 1.0;                                     // (2 s is exact: a contraction changes nothing)
            if ((double)(w0 + k) >= wc * t) { tau = t; window = w0 + k; return; }
        }
    }
    tau = t;
}

// The shape of a k_acf_products launch for chains of N draws and lags 0 .. L: a workgroup takes `span` consecutive draw
// blocks x `qw` consecutive lag quads (span * qw = 256, qw >= 32: the 16 lanes the LDS serves together share a block and
// read one broadcast address); nlb such lag groups cover the nq quads, nbg block groups the nblk blocks.
struct AcfGeom { int span, qw, nq, nlb, lp; i64 nblk, nbg; };
__host__ __device__ inline AcfGeom acf_geom(i64 N, i64 L)
{
    AcfGeom g;
    g.nq = (int)((L + kAcfLags) / kAcfLags);
    g.lp = g.nq * kAcfLags;                                          // lags of a row of part / gam (padded to whole quads)
    g.nblk = (N + kAcfBlock - 1) / kAcfBlock;
    g.span = 1;
    while (g.span < kAcfMaxSpan && g.span < g.nblk && kAcfNT / (2 * g.span) >= g.nq) g.span *= 2;
    g.qw = kAcfNT / g.span;
    g.nlb = (g.nq + g.qw - 1) / g.qw;
    g.nbg = (g.nblk + g.span - 1) / g.span;
    return g;
}
// Doubles of LDS of such a workgroup: the lag stream (span blocks + the lags), and in front of it the draw stream when the
// lag group does not start at lag 0 (then the two do not overlap).
__host__ __device__ inline size_t acf_lds_doubles(const AcfGeom& g)
{
    const size_t nA = (size_t)g.span * kAcfBlock;
    return (g.nlb > 1 ? nA + kAcfSlack : 0) + nA + (size_t)kAcfLags * g.qw + kAcfSlack;
}
__host__ __device__ inline int acf_threads(const AcfGeom& g)
{
    const int need = g.span > 1 ? kAcfNT : (g.nq + kWave - 1) / kWave * kWave;
    return need < kAcfNT ? need : kAcfNT;
}

// The chain of a workgroup whose grid spreads the chains (or groups of them) over y and z.
__device__ __forceinline__ i64 acf_grid_chain() { return (i64)blockIdx.z * gridDim.y + blockIdx.y; }

// ------------------------------------------------------------------------------------------------
// k_acf_mean: a wave owns a chain, four chains per workgroup.  grid: x = ceil(pc / 8) * 8 (xcd_map), y * z >= ceil(C / 4).
// mean[p * C + c] = m, bad[p * C + c] = the chain's non-finite draws.  8-byte loads by element: the alignment of a row
// plays no part.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_acf_mean(const double* __restrict__ X, i64 C, i64 N, i64 pc, double* __restrict__ mean,
                                                  double* __restrict__ bad)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    i64 p;
    int blk;
    if (!xcd_map(pc, 1, p, blk)) return;
    const i64 c = acf_grid_chain() * 4 + wave;
    if (c >= C) return;                                              // (no workgroup barrier below)
    i64 nb = 0;
    const double s = xor_tree_sum(acf_lane_sum(X + (p * C + c) * N, N, lane, &nb));
    const double b = xor_tree_sum((double)nb);
    if (lane == 0) { mean[p * C + c] = s / (double)N; bad[p * C + c] = b; }
}

// ------------------------------------------------------------------------------------------------
// k_acf_products: one workgroup per (parameter, chain, group of g.span draw blocks, group of g.qw lag quads).  grid: x =
// ceil(pc / 8) * 8 * g.nbg * g.nlb (xcd_map), y * z >= C.  It stages the deviations of its draws and of the lag window
// behind them in LDS once (8-byte loads by element, 0 past the row's end: nothing is read past N - 1).  Thread (sb, q)
// owns block b0 + sb and the lags 4 qg .. 4 qg + 3 and walks the block in steps of 4 draws: the 4 draws are one 32-byte
// broadcast read, the lag window slides by one 32-byte read per lane (consecutive lanes, consecutive quads: no bank
// conflict), the reads of the next step are issued before the 16 fma of this one.  A step reads 8 doubles per 16 fma.
// part[((p * C + c) * nblk + b) * lp + l] = the block's fma chain of lag l.  No atomics.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAcfNT) void k_acf_products(const double* __restrict__ X, const double* __restrict__ mean, i64 C,
                                                         i64 N, i64 pc, AcfGeom g, double* __restrict__ part)
{
    extern __shared__ __align__(16) double acf_sh[];
    i64 p;
    int blk;
    if (!xcd_map(pc, (int)(g.nbg * g.nlb), p, blk)) return;
    const i64 c = acf_grid_chain();
    if (c >= C) return;                                              // (uniform over the workgroup)
    const i64 bg = blk / g.nlb;
    const int lb = blk % g.nlb;
    const i64 b0 = bg * g.span, base = b0 * kAcfBlock;               // the first block and draw of the workgroup
    const int lag0 = lb * g.qw * kAcfLags;                           // its first lag
    const int nA = g.span * kAcfBlock;
    const int nW = nA + kAcfLags * g.qw;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double* x = X + (p * C + c) * N;
    const double m = mean[p * C + c];
    // A stream of `count` deviations (a multiple of 4) lies in LDS as two arrays of 16-byte pairs: the pairs (4k, 4k + 1)
    // in dst[0 .. count / 2), the pairs (4k + 2, 4k + 3) behind them.  A lane reads its quad k as one pair from each: lanes
    // with consecutive k then read consecutive 16 bytes, which the LDS serves without a bank conflict (32 bytes apart in
    // one array they would collide two by two).
    const int cA = nA + kAcfSlack, cW = nW + kAcfSlack;
    double* A = acf_sh;                                              // d[base + k]
    double* W = acf_sh + (lag0 ? cA : 0);                            // d[base + lag0 + k]
    // no thread uses a deviation at or past N + 12 (its steps end within 3 of its last product, the window is 7 wide)
    auto stage = [&](double* dst, i64 first, int count) {
        const i64 lim = N + 12 - first;
        const int n = lim < count ? (lim < 0 ? 0 : (int)lim) : count;
        for (int k = tid; k < n; k += nt) {
            const i64 i = first + k;
            dst[((k >> 1) & 1) * (count >> 1) + ((k >> 2) << 1) + (k & 1)] = i < N ? x[i] - m : 0.0;
        }
    };
    if (lag0) stage(A, base, cA);
    stage(W, base + lag0, cW);
    __syncthreads();
    const int sb = tid / g.qw, q = tid % g.qw;
    const i64 b = b0 + sb;
    const int qg = lb * g.qw + q;
    if (b >= g.nblk || qg >= g.nq) return;
    const i64 l0 = (i64)kAcfLags * qg;
    const i64 rem = N - l0 - b * kAcfBlock;                          // products of the thread's first lag in this block
    const int iend = rem > kAcfBlock ? kAcfBlock : (rem < 0 ? 0 : (int)rem);
    const int steps = (iend + kAcfDraws - 1) / kAcfDraws;
    const int qa = sb * (kAcfBlock / 4), qw = qa + q;                // the thread's first quad in either stream
    const double2* Ae = reinterpret_cast<const double2*>(A) + qa;
    const double2* Ao = reinterpret_cast<const double2*>(A + ((lag0 ? cA : cW) >> 1)) + qa;
    const double2* We = reinterpret_cast<const double2*>(W) + qw;
    const double2* Wo = reinterpret_cast<const double2*>(W + (cW >> 1)) + qw;
    double acc[kAcfLags] = {0.0, 0.0, 0.0, 0.0};
    double2 a01 = Ae[0], a23 = Ao[0], w01 = We[0], w23 = Wo[0], w45 = We[1], w67 = Wo[1];
    for (int s = 0; s < steps; ++s) {
        const double2 na01 = Ae[s + 1], na23 = Ao[s + 1], nw45 = We[s + 2], nw67 = Wo[s + 2];
        const double a[kAcfDraws] = {a01.x, a01.y, a23.x, a23.y};
        const double w[kAcfDraws + kAcfLags - 1] = {w01.x, w01.y, w23.x, w23.y, w45.x, w45.y, w67.x};
#pragma unroll
        for (int d = 0; d < kAcfDraws; ++d)                          // draw after draw: every lag's chain in ascending i
#pragma unroll
            for (int k = 0; k < kAcfLags; ++k) acc[k] = fma(a[d], w[d + k], acc[k]);
        a01 = na01; a23 = na23; w01 = w45; w23 = w67; w45 = nw45; w67 = nw67;
    }
    double2* o = reinterpret_cast<double2*>(part + ((p * C + c) * g.nblk + b) * g.lp + l0);
    o[0] = make_double2(acc[0], acc[1]);
    o[1] = make_double2(acc[2], acc[3]);
}

// rho[0 .. L] in LDS holds gamma; normalises it in place, writes it to acf (NULL: skipped) and lets thread 0 run the scan.
__device__ __forceinline__ void acf_normalise_scan(double* rho, i64 L, double wc, double* __restrict__ acf, double& g0,
                                                   double& tau, i64& window)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    g0 = rho[0];
    __syncthreads();
    for (i64 l = tid; l <= L; l += nt) {
        const double r = acf_rho(rho[l], g0);
        rho[l] = r;
        if (acf) acf[l] = r;
    }
    __syncthreads();
    if (tid == 0) acf_tau_scan(rho, L, wc, tau, window);
}

// ------------------------------------------------------------------------------------------------
// k_acf_finish: one workgroup per (parameter, chain); L + 1 doubles of LDS.  Thread t joins the blocks of the lags t, t +
// 256, .. in block order, divides, keeps gamma for k_acf_pool (gam[(p * C + c) * lp + l]), normalises; thread 0 runs the
// tau scan.  acf / var / tau / window point at the chunk's first parameter.  grid as k_acf_products with one block each.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAcfFinNT) void k_acf_finish(const double* __restrict__ part, i64 C, i64 N, i64 pc, i64 L, AcfGeom g,
                                                          int unbiased, double wc, double* __restrict__ gam,
                                                          double* __restrict__ acf, double* __restrict__ var,
                                                          double* __restrict__ tau, i64* __restrict__ window)
{
    extern __shared__ __align__(16) double acf_sh[];
    i64 p;
    int blk;
    if (!xcd_map(pc, 1, p, blk)) return;
    const i64 c = acf_grid_chain();
    if (c >= C) return;
    const i64 pcn = p * C + c;
    const double* pr = part + pcn * g.nblk * g.lp;
    for (i64 l = threadIdx.x; l <= L; l += kAcfFinNT) {
        double S = 0.0;
#pragma unroll 4
        for (i64 b = 0; b < g.nblk; ++b) S += pr[b * g.lp + l];
        const double gl = acf_gamma(S, N, l, unbiased != 0);
        gam[pcn * g.lp + l] = gl;
        acf_sh[l] = gl;
    }
    double g0, t;
    i64 w;
    acf_normalise_scan(acf_sh, L, wc, acf ? acf + pcn * (L + 1) : nullptr, g0, t, w);
    if (threadIdx.x == 0) { var[pcn] = g0; tau[pcn] = t; window[pcn] = w; }
}

// ------------------------------------------------------------------------------------------------
// k_acf_pool: one workgroup per parameter; the chains' gamma_l are added in chain order, divided by C, normalised,
// scanned.  grid: ceil(pc / 8) * 8 (xcd_map).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAcfFinNT) void k_acf_pool(const double* __restrict__ gam, i64 C, i64 pc, i64 L, int lp, double wc,
                                                        double* __restrict__ acf_pooled, double* __restrict__ tau_pooled,
                                                        i64* __restrict__ window_pooled)
{
    extern __shared__ __align__(16) double acf_sh[];
    i64 p;
    int blk;
    if (!xcd_map(pc, 1, p, blk)) return;
    const double* gp = gam + p * C * lp;
    for (i64 l = threadIdx.x; l <= L; l += kAcfFinNT) {
        double s = 0.0;
#pragma unroll 4
        for (i64 c = 0; c < C; ++c) s += gp[c * lp + l];
        acf_sh[l] = s / (double)C;
    }
    double g0, t;
    i64 w;
    acf_normalise_scan(acf_sh, L, wc, acf_pooled + p * (L + 1), g0, t, w);
    if (threadIdx.x == 0) { tau_pooled[p] = t; window_pooled[p] = w; }
}

}  // namespace mcr
