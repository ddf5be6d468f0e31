// mcr_pareto.hpp -- Pareto k-hat of the draws' tails (Vehtari, Simpson, Gelman, Yao, Gabry: "Pareto smoothed importance
// sampling"; pareto_khat(tail = "both") of the R package posterior, with Zhang and Stephens' (2009) profile fit): the
// shape k of a generalised Pareto distribution fitted to the t largest and the t smallest draws of a parameter.  The
// definition is in mcmcref_hip.h.  Everything in front of the kernel -- the pooled ascending order, the non-finite
// count -- is the summary pipeline's, run without diagnostics: the kernel reads the sort stage's keys.
//
//   exceedances   right  e_i = x_(M-t+i) - x_(M-t-1)      left  e_i = x_(t) - x_(t-1-i)       i = 0 .. t-1, ascending
//                 (then scaled by the power of two that brings e_(n-1) into [1, 2): exact)
//   grid          theta_j = 1 / e_(n-1) + (1 - sqrt(G / (j - 0.5))) / 3 / xstar               j = 1 .. G = 30 + isqrt(n)
//   profile       k_j = (sum_i log1p(-theta_j e_i)) / n     l_j = n (log(-theta_j / k_j) - k_j - 1)
//   posterior     theta = sum_j theta_j exp(l_j - L),  L = log sum_j exp(l_j)
//   shape         k = (sum_i log1p(-theta e_i)) / n,  khat = (k n + 5) / (n + 10)
//
// ONE text computes a tail on the device and on the host (pareto_fit): it is written over a "wave" W that says who
// takes which grid point and how 64 partial sums meet.  Every sum over i is 64 partial sums (partial l adds the terms
// l, l + 64, .. in index order) joined by the xor tree 32, 16, .. 1; every sum and the maximum over j likewise.  The order
// is a function of n alone, so a parameter's bits do not depend on its place in a batch, the chunking or the entry.
// Host and device differ only in their libm (log1p, log, exp).
#pragma once
#include "mcr_device.hpp"

namespace mcr {

constexpr int kParetoNT = 1024;               // threads of a k_pareto_fit workgroup: 16 waves share the grid points
constexpr int kParetoLdsTail = 8192;          // the longest tail staged in LDS (64 KB of exceedances)
constexpr int kParetoMinTail = 5;

// floor(sqrt(n)) in integers: the double root is only a first guess.
__host__ __device__ inline i64 pareto_isqrt(i64 n)
{
    if (n <= 0) return 0;
    i64 r = (i64)sqrt((double)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}
__host__ __device__ inline int pareto_grid(i64 n) { return 30 + (int)pareto_isqrt(n); }

// The effective tail length of M draws for a requested one (>= 1): min(max(t_req, 5), floor(M / 2)).
__host__ __device__ inline i64 pareto_tail_eff(i64 M, i64 t_req)
{
    const i64 t = t_req > kParetoMinTail ? t_req : kParetoMinTail;
    return t < M / 2 ? t : M / 2;
}

// max that hands a NaN on (numpy's), whichever side it stands on
__host__ __device__ inline double pareto_max(double a, double b) { return (b > a || b != b) ? b : a; }

// The wave of the host entry: one thread plays the 64 partial sums in turn and takes every grid point.
struct ParetoHostWave {
    template <class F> __host__ __device__ double sum(F&& f) const
    {
        double v[kWave];
        for (int l = 0; l < kWave; ++l) v[l] = f(l);
        for (int o = kWave >> 1; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) v[l] += v[l + o];
        return v[0];
    }
    template <class F> __host__ __device__ double max(F&& f) const
    {
        double v[kWave];
        for (int l = 0; l < kWave; ++l) v[l] = f(l);
        for (int o = kWave >> 1; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) v[l] = pareto_max(v[l], v[l + o]);
        return v[0];
    }
    __host__ __device__ int first() const { return 0; }
    __host__ __device__ int step() const { return 1; }
    __host__ __device__ bool writer() const { return true; }
    __host__ __device__ bool finisher() const { return true; }
    __host__ __device__ void barrier() const {}
};

// One tail of n >= 5 ascending exceedances e.  lg: G doubles of scratch for the profile values l_j, shared by the waves
// of W.  Returns khat in every thread for which W::finisher() holds (and in every thread when it returns before the
// grid: a constant tail, xstar == 0).  raw (optional; mcr_psis.hpp): where the grid was run, the finisher's unregularised
// k, theta and the power-of-two scale into raw[0 .. 2]; untouched by the early returns.
template <class W>
__host__ __device__ inline double pareto_fit(const W& w, const double* e, int n, double* lg, double* raw = nullptr)
{
#pragma clang fp contract(off)  // the host and the device round every product and sum alike
    if (e[n - 1] == e[0]) return NAN;                      // a constant tail
    const int G = pareto_grid(n);
    if (e[(n + 2) / 4 - 1] == 0.0) return INFINITY;        // xstar == 0: the tail's first quarter ties with the cutoff
    // The fit is scale-free in exact arithmetic but log(-theta_j / k_j) is not in floating point: the exceedances are read
    // through the power of two that brings e_(n-1) into [1, 2), so that khat(x) and khat(2^m x) have the same bits.
    int ex;
    frexp(e[n - 1], &ex);
    const double sc = ldexp(1.0, 1 - (ex < -1000 ? -1000 : ex > 1000 ? 1000 : ex));
    const double emax = e[n - 1] * sc, xstar = e[(n + 2) / 4 - 1] * sc;   // xstar = e_(floor(n / 4 + 0.5) - 1)
    const double dn = (double)n, dG = (double)G;
    auto theta_j = [&](int j) { return 1.0 / emax + (1.0 - sqrt(dG / ((double)j - 0.5))) / 3.0 / xstar; };
    auto profile = [&](double th) {
        return w.sum([&](int l) { double s = 0.0; for (int i = l; i < n; i += kWave) s += log1p(-th * (e[i] * sc)); return s; }) / dn;
    };
    for (int j = 1 + w.first(); j <= G; j += w.step()) {   // no barrier per grid point: a wave owns its points
        const double th = theta_j(j);
        const double k = profile(th);
        if (w.writer()) lg[j - 1] = dn * (log(-th / k) - k - 1.0);
    }
    w.barrier();
    if (!w.finisher()) return NAN;
    const double m = w.max([&](int l) { double v = -INFINITY; for (int j = l; j < G; j += kWave) v = pareto_max(v, lg[j]); return v; });
    const double se = w.sum([&](int l) { double s = 0.0; for (int j = l; j < G; j += kWave) s += exp(lg[j] - m); return s; });
    const double L = m + log(se);
    const double th = w.sum([&](int l) { double s = 0.0; for (int j = l; j < G; j += kWave) s += theta_j(j + 1) * exp(lg[j] - L); return s; });
    const double k = profile(th);
    if (raw) { raw[0] = k; raw[1] = th; raw[2] = sc; }
    const double khat = (k * dn + 5.0) / (dn + 10.0);      // the weakly informative prior: mean 0.5, weight 10
    return khat != khat ? INFINITY : khat;
}

// The wave of the kernel: lane l holds partial sum l, the waves of the workgroup take the grid points round robin,
// wave 0 finishes.  Every lane ends a sum with the same bits (the xor tree adds the same pairs in every lane).
struct ParetoDevWave {
    int lane, wave, nwaves;
    template <class F> __device__ double sum(F&& f) const { return xor_tree_sum(f(lane)); }
    template <class F> __device__ double max(F&& f) const
    {
        double v = f(lane);
        for (int o = kWave >> 1; o > 0; o >>= 1) v = pareto_max(v, __shfl_xor(v, o, kWave));
        return v;
    }
    __device__ int first() const { return wave; }
    __device__ int step() const { return nwaves; }
    __device__ bool writer() const { return lane == 0; }
    __device__ bool finisher() const { return wave == 0; }
    __device__ void barrier() const { __threadfence_block(); __syncthreads(); }
};

// ------------------------------------------------------------------------------------------------
// k_pareto_fit: one workgroup per (parameter, tail); tail 0 left, 1 right.  grid: ceil(pc / 8) * 8 * 2, one-dimensional
// (xcd_map: both tails of a parameter on the XCD whose L2 holds its keys).  The workgroup forms its t exceedances from
// the ascending keys -- into dynamic LDS while t <= kParetoLdsTail (consecutive lanes read consecutive doubles: no bank
// conflict), else into the sort stage's free key buffer, which the t <= M / 2 entries of the two tails never share and
// L2 serves -- then runs pareto_fit: the G x t log1p evaluations are the work, G / 16 grid points per wave.
// tail[p] is the effective t of parameter p (the host's pareto_tail_eff; clamped here once more, t < 5: NaN).
// lgrid[(p * 2 + tail) * gmax ..] are the tail's l_j.   res[(field0 + tail) * pc + p] = khat.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kParetoNT) void k_pareto_fit(const double* __restrict__ keys, i64 M, i64 pc,
                                                          const i64* __restrict__ tail, double* ex, double* lgrid,
                                                          i64 gmax, double* __restrict__ res, int field0)
{
    extern __shared__ __align__(16) double sh_e[];
    i64 p;
    int side;
    if (!xcd_map(pc, 2, p, side)) return;
    const int tid = threadIdx.x;
    i64 t64 = tail[p];
    if (t64 > M / 2) t64 = M / 2;
    double* out = res + (i64)(field0 + side) * pc + p;
    if (t64 < kParetoMinTail || pareto_grid(t64) > gmax) {     // (uniform over the workgroup)
        if (tid == 0) *out = NAN;
        return;
    }
    const int t = (int)t64;
    const double* k = keys + p * M;
    const bool lds = t <= kParetoLdsTail;
    double* e = lds ? sh_e : ex + p * M + (side ? M - t : 0);
    const double cut = side ? k[M - t - 1] : k[t];
    for (int i = tid; i < t; i += kParetoNT) e[i] = side ? k[M - t + i] - cut : cut - k[t - 1 - i];
    __threadfence_block();
    __syncthreads();
    const ParetoDevWave w{tid & (kWave - 1), tid >> 6, kParetoNT / kWave};
    double* lg = lgrid + (p * 2 + side) * gmax;
    const double khat = lds ? pareto_fit(w, (const double*)sh_e, t, lg) : pareto_fit(w, (const double*)e, t, lg);
    if (tid == 0) *out = khat;
}
}  // namespace mcr
