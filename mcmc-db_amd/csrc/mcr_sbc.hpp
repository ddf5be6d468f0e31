// mcr_sbc.hpp -- simulation-based calibration (Talts et al. 2018; the SBC R package): for S simulations x P parameters at
// once, where the true value stands among the L pooled posterior draws of its fit -- n_less, n_equal -- and the draws' mean
// and population sd (for the z score and the posterior contraction).  The definition is in mcmcref_hip.h.  Also the host
// side of the method, which needs no device: the chi-square survival function, the rank histogram's uniformity statistics.
//
// A row is one (simulation, parameter): L consecutive fp64 draws, row = s * P + p.  Rows are short (L is 100 .. 4000) and
// there are many (S P is 1e4 .. 1e6), so a WAVE owns a row and a workgroup of four waves four consecutive rows: no LDS, no
// barrier, no atomics.  The two sums of a row -- sum x, then sum (x - mean)^2 -- use the one association of
// mcr_tree.hpp: the balanced tree over the 1024 adjacent indices of a block (+0 past the end), blocks added in
// ascending order from +0.  It is defined on the indices of the row, so a row's bits depend neither on where the row
// lies (16-byte loads when its first draw is 16-byte aligned, 8-byte loads otherwise: wgt_load2) nor on the rows around it.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "mcr_tree.hpp"

namespace mcr {

constexpr int kSbcNT = 256;                   // threads of k_sbc_ranks: a wave per row
constexpr int kSbcRows = kSbcNT / kWave;      // rows of a workgroup
constexpr int kSbcRegBlocks = 4;              // rows of up to this many blocks (4096 draws) are read once and kept in registers
// A row's entries in the result table: res[field * rows + row]
enum SbcField { SB_LESS = 0, SB_EQUAL, SB_MEAN, SB_SD, SB_BAD, kSbcFields };

// (x - mean)^2: the difference and the product are rounded one after the other.
__host__ __device__ inline double sbc_dev2(double x, double mean)
{
#pragma clang fp contract(off)
    const double d = x - mean;
    return d * d;
}
__host__ __device__ inline bool sbc_nonfinite(double x) { return !(fabs(x) < INFINITY); }

// The lane's 16 draws of block b of the row x[0 .. L): the pairs 1024 b + 128 r + 2 lane (+0 past the end).
__device__ __forceinline__ void sbc_load(const double* __restrict__ x, i64 b, i64 L, bool wide, int lane, double (&xa)[kWgtRows],
                                         double (&xb)[kWgtRows])
{
#pragma unroll
    for (int r = 0; r < kWgtRows; ++r) wgt_load2(x, b * kWgtBlock + 2 * kWave * r + 2 * lane, L, wide, xa[r], xb[r]);
}

// The lane's draws of block b below t, equal to t, and not finite (IEEE comparisons: -0.0 == +0.0, NaN is neither).
__device__ __forceinline__ void sbc_count(const double (&xa)[kWgtRows], const double (&xb)[kWgtRows], i64 b, i64 L, int lane, double t,
                                          int& less, int& equal, int& bad)
{
#pragma unroll
    for (int r = 0; r < kWgtRows; ++r) {
        const i64 i = b * kWgtBlock + 2 * kWave * r + 2 * lane;
        if (i < L) { less += xa[r] < t; equal += xa[r] == t; bad += sbc_nonfinite(xa[r]); }
        if (i + 1 < L) { less += xb[r] < t; equal += xb[r] == t; bad += sbc_nonfinite(xb[r]); }
    }
}

// The block's tree of x (the +0 past the end is what was loaded) ...
__device__ __forceinline__ double sbc_root_x(const double (&xa)[kWgtRows], const double (&xb)[kWgtRows], int lane)
{
    double v[kWgtRows];
#pragma unroll
    for (int r = 0; r < kWgtRows; ++r) v[r] = wgt_add(xa[r], xb[r]);
    return sbc_wave_root(v, lane);
}
// ... and of (x - mean)^2
__device__ __forceinline__ double sbc_root_d(const double (&xa)[kWgtRows], const double (&xb)[kWgtRows], i64 b, i64 L, int lane, double mean)
{
    double v[kWgtRows];
#pragma unroll
    for (int r = 0; r < kWgtRows; ++r) {
        const i64 i = b * kWgtBlock + 2 * kWave * r + 2 * lane;
        v[r] = wgt_add(i < L ? sbc_dev2(xa[r], mean) : 0.0, i + 1 < L ? sbc_dev2(xb[r], mean) : 0.0);
    }
    return sbc_wave_root(v, lane);
}

__device__ __forceinline__ int sbc_wave_sum(int v)
{
    for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// ------------------------------------------------------------------------------------------------
// k_sbc_ranks<RB>: a wave per row, kSbcRows rows per workgroup; grid: ceil(rows / kSbcRows), one-dimensional.  A row of at
// most RB blocks is loaded once -- every load of the lane in flight together -- and both passes run on the registers; a
// longer row is streamed block by block, twice: the second pass finds it in cache (32 KB per 4096 draws).  Both forms add
// the same roots in the same order.  Counts are per-lane integers (L < 2^31 - 1) joined by a wave reduction.
// res[f * stride + row], f of SbcField: n_less, n_equal, mean = sum / L, sd = sqrt(sum (x - mean)^2 / L), non-finite count.
// Reads X[row * L + 0 .. L-1] and truth[row], row < rows, only; L >= 1.
// ------------------------------------------------------------------------------------------------
template <int RB>
__global__ __launch_bounds__(kSbcNT) void k_sbc_ranks(const double* __restrict__ X, i64 L, i64 rows, const double* __restrict__ truth,
                                                      double* __restrict__ res, i64 stride)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const i64 row = (i64)blockIdx.x * kSbcRows + wave;
    if (row >= rows) return;                                  // (the whole wave)
    const double* x = X + row * L;
    const bool wide = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const double t = truth[row];
    const i64 nb = wgt_blocks(L);
    int less = 0, equal = 0, bad = 0;
    double s = 0.0, q = 0.0, mean;
    if (nb <= RB) {
        double xa[RB][kWgtRows], xb[RB][kWgtRows];
#pragma unroll
        for (int b = 0; b < RB; ++b)
            if (b < nb) sbc_load(x, b, L, wide, lane, xa[b], xb[b]);
#pragma unroll
        for (int b = 0; b < RB; ++b)
            if (b < nb) {
                sbc_count(xa[b], xb[b], b, L, lane, t, less, equal, bad);
                s = wgt_add(s, sbc_root_x(xa[b], xb[b], lane));
            }
        mean = s / (double)L;
#pragma unroll
        for (int b = 0; b < RB; ++b)
            if (b < nb) q = wgt_add(q, sbc_root_d(xa[b], xb[b], b, L, lane, mean));
    } else {
        double xa[kWgtRows], xb[kWgtRows];
        for (i64 b = 0; b < nb; ++b) {
            sbc_load(x, b, L, wide, lane, xa, xb);
            sbc_count(xa, xb, b, L, lane, t, less, equal, bad);
            s = wgt_add(s, sbc_root_x(xa, xb, lane));
        }
        mean = s / (double)L;
        for (i64 b = 0; b < nb; ++b) {
            sbc_load(x, b, L, wide, lane, xa, xb);
            q = wgt_add(q, sbc_root_d(xa, xb, b, L, lane, mean));
        }
    }
    less = sbc_wave_sum(less); equal = sbc_wave_sum(equal); bad = sbc_wave_sum(bad);
    if (lane == 0) {
        res[(i64)SB_LESS * stride + row] = (double)less;
        res[(i64)SB_EQUAL * stride + row] = (double)equal;
        res[(i64)SB_MEAN * stride + row] = mean;
        res[(i64)SB_SD * stride + row] = sqrt(q / (double)L);
        res[(i64)SB_BAD * stride + row] = (double)bad;
    }
}

// The same row on the host: the counts and the two sums in the one association (wgt_host_sum).  L >= 1.
inline void sbc_row_host(WgtHostTree& tr, const double* x, i64 L, double t, i64& less, i64& equal, i64& bad, double& mean, double& sd)
{
    less = equal = bad = 0;
    for (i64 i = 0; i < L; ++i) { less += x[i] < t; equal += x[i] == t; bad += sbc_nonfinite(x[i]); }
    mean = wgt_host_sum(tr, L, [&](i64 i) { return x[i]; }) / (double)L;
    const double m = mean;
    sd = sqrt(wgt_host_sum(tr, L, [&](i64 i) { return sbc_dev2(x[i], m); }) / (double)L);
}

// ---- the chi-square survival function ------------------------------------------------------------------------------------
// Q(a, x), the regularised upper incomplete gamma function, a > 0: below a + 1 one minus the series of P(a, x), above it
// the continued fraction of Q by the modified Lentz recurrence.  Both carry the factor exp(-x + a log x - lgamma(a)).
inline double sbc_gamma_q(double a, double x)
{
    if (!(x > 0.0)) return x == 0.0 ? 1.0 : NAN;
    if (x == INFINITY) return 0.0;
    const double front = exp(-x + a * log(x) - lgamma(a));
    if (x < a + 1.0) {
        double ap = a, term = 1.0 / a, sum = term;
        for (int n = 0; n < 100000; ++n) {
            ap += 1.0;
            term *= x / ap;
            sum += term;
            if (fabs(term) < fabs(sum) * 1e-17) break;
        }
        return 1.0 - sum * front;
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int n = 1; n < 100000; ++n) {
        const double an = -(double)n * ((double)n - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return front * h;
}

// ---- the rank histogram's uniformity -------------------------------------------------------------------------------------
// The first rank of bin b of B over the ranks 0 .. L: a rank r lies in bin floor(r B / (L + 1)).
inline i64 sbc_bin_start(i64 b, i64 B, i64 L) { return (b * (L + 1) + B - 1) / B; }

// One parameter's column of S ranks (stride P): the bins' counts, chi2 against expected[], and the largest distance of the
// ranks' ECDF from the uniform one, |#{ranks <= r} (L + 1) - (r + 1) S| maximised as an integer over r and divided once.
// sorted: scratch of S entries.  false: a rank outside 0 .. L.
inline bool sbc_uniform_column(const i64* ranks, i64 S, i64 P, i64 L, i64 B, const double* expected, std::vector<i64>& sorted, i64* counts,
                               double& chi2, double& ecdf)
{
    std::vector<i64> cnt((size_t)B, 0);
    for (i64 s = 0; s < S; ++s) {
        const i64 r = ranks[s * P];
        if (r < 0 || r > L) return false;
        sorted[(size_t)s] = r;
        cnt[(size_t)(r * B / (L + 1))] += 1;
    }
    chi2 = 0.0;
    for (i64 b = 0; b < B; ++b) {
        const double d = (double)cnt[(size_t)b] - expected[b];
        chi2 += d * d / expected[b];
        if (counts) counts[b] = cnt[(size_t)b];
    }
    std::sort(sorted.begin(), sorted.end());
    // the ECDF is flat between two ranks that occur and the uniform one rises: the distance peaks at a rank that occurs (all
    // of its ties counted) or at the rank in front of one (none of them counted)
    i64 best = 0;
    auto see = [&](i64 cum, i64 r) { const i64 d = cum * (L + 1) - (r + 1) * S; if ((d < 0 ? -d : d) > best) best = d < 0 ? -d : d; };
    for (i64 k = 0; k < S;) {
        i64 e = k;
        while (e < S && sorted[(size_t)e] == sorted[(size_t)k]) ++e;
        if (sorted[(size_t)k] > 0) see(k, sorted[(size_t)k] - 1);
        see(e, sorted[(size_t)k]);
        k = e;
    }
    ecdf = (double)best / ((double)S * (double)(L + 1));
    return true;
}
}  // namespace mcr
