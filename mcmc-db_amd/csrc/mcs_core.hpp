// mcs_core.hpp -- the arithmetic of include/mcmcref_std.h that the host routine and the kernels share as ONE text: the
// lane-strided sum, the lag product, the pooled moments of a series (R-hat, the variance of the chain means, the pooled
// sd) and Geyer's walk.  Compiled without fused multiply-add on both sides (the pragmas below and -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>

#include "mcmcref_std.h"

#if defined(__HIPCC__)
#define MCS_HD __host__ __device__ inline
#else
#define MCS_HD inline
#endif

namespace mcs {

enum Series { S_BULK = 0, S_FOLD, S_Q05, S_Q95, S_RAW, kSeries };
constexpr int kMomRec = 4;                 // a chain's record: mean, sum of squared deviations, min, max
constexpr int kOutRec = 6;                 // a series' results: ess, lag, rhat, margin, sd, tau
enum OutField { O_ESS = 0, O_LAG, O_RHAT, O_MARGIN, O_SD, O_TAU };
constexpr int kLanes = 64;

// Lane `lane` of the lane-strided sum of v(0) .. v(n - 1): the terms lane, lane + 64, .. in ascending order.
template <class F>
MCS_HD double lane_partial(F&& v, int64_t n, int lane)
{
#pragma clang fp contract(off)
    double a = 0.0;
    for (int64_t i = lane; i < n; i += kLanes) a = a + v(i);
    return a;
}

// The 64 lane sums meet in the xor tree (32, 16, .. 1); a[l] + a[l ^ o] is computed once per pair (addition commutes).
inline double tree64(double* a)
{
    for (int o = kLanes / 2; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) a[l] = a[l] + a[l + o];
    return a[0];
}

// sum_{i < n - t} d[i] d[i + t]: one accumulator, ascending i, the product rounded before the addition.
template <class T>
MCS_HD double lag_product(const T* d, int64_t n, int64_t t)
{
#pragma clang fp contract(off)
    double a = 0.0;
    for (int64_t i = 0; i + t < n; ++i) a = a + d[i] * d[i + t];
    return a;
}

// What a series' chain records give: mom(k, f) is field f of split chain k.
struct Pool {
    double var_means, rhat, sd;
    bool constant;
};

template <class Mom>
MCS_HD Pool pool_of(Mom&& mom, int64_t m, int64_t n)
{
#pragma clang fp contract(off)
    double lo = mom(0, 2), hi = mom(0, 3), sm = 0.0, sq = 0.0;
    for (int64_t k = 0; k < m; ++k) {
        sm = sm + mom(k, 0);
        sq = sq + mom(k, 1) / (double)(n - 1);
        lo = mom(k, 2) < lo ? mom(k, 2) : lo;
        hi = mom(k, 3) > hi ? mom(k, 3) : hi;
    }
    const double mean = sm / (double)m, W = sq / (double)m;
    double b = 0.0, ss = 0.0;
    for (int64_t k = 0; k < m; ++k) {
        const double d = mom(k, 0) - mean;
        b = b + d * d;
        ss = ss + (mom(k, 1) + (double)n * (d * d));
    }
    Pool p;
    p.var_means = m > 1 ? b / (double)(m - 1) : 0.0;
    p.rhat = std::sqrt(((double)n * p.var_means / W + (double)(n - 1)) / (double)n);
    p.sd = std::sqrt(ss / (double)(m * n - 1));
    p.constant = !(lo < hi);
    if (p.constant) p.rhat = NAN;
    return p;
}

// Geyer's initial positive and monotone sequence, as a stream of pairs: the monotone pass looks one pair back only, so
// the pair at lag t is settled -- adjusted and added to the sum -- the moment the walk moves on to t + 2.
struct Walk {
    double mean_var, var_plus, re, ro, pe, po, sum, margin;
    int64_t t, n;
    bool done;

    MCS_HD double rho(double g) const
    {
#pragma clang fp contract(off)
        return 1.0 - (mean_var - g) / var_plus;
    }
    MCS_HD bool goes_on() const { return t < n - 5 && re + ro > 0.0; }

    // gamma(0), gamma(1) and the variance of the chain means; false: var_plus is not positive (the ESS is NaN)
    MCS_HD bool start(double g0, double g1, double var_means, int64_t n_)
    {
#pragma clang fp contract(off)
        n = n_;
        mean_var = g0 * (double)n / (double)(n - 1);
        var_plus = g0 + var_means;
        t = 0;
        re = 1.0;
        ro = rho(g1);
        pe = po = sum = 0.0;
        margin = std::fabs(re + ro);
        done = !goes_on();
        return var_plus > 0.0;
    }
    // gamma(t + 2), gamma(t + 3): only while !done
    MCS_HD void step(double ge, double go)
    {
#pragma clang fp contract(off)
        if (t >= 2 && re + ro > pe + po) {
            re = (pe + po) / 2.0;
            ro = re;
        }
        sum = sum + re;
        sum = sum + ro;
        pe = re;
        po = ro;
        t += 2;
        re = rho(ge);
        ro = rho(go);
        const double a = std::fabs(re + ro);
        margin = a < margin ? a : margin;
        done = !goes_on();
    }
    // after the last step: max_t = t
    MCS_HD double tau() const
    {
#pragma clang fp contract(off)
        const double last = (re > 0.0 || re + ro >= 0.0) ? re : 0.0;
        return -1.0 + 2.0 * sum + last;
    }
};

// out[kOutRec] of a series that is not walked: n < 4, a constant series, var_plus not positive.
MCS_HD void out_unwalked(const Pool& p, double* out)
{
    out[O_ESS] = NAN;
    out[O_LAG] = -1.0;
    out[O_RHAT] = p.rhat;
    out[O_MARGIN] = NAN;
    out[O_SD] = p.sd;
    out[O_TAU] = NAN;
}

MCS_HD void out_walked(const Pool& p, const Walk& w, int64_t S, double* out)
{
#pragma clang fp contract(off)
    const double floor_tau = 1.0 / std::log10((double)S);
    double tau = w.tau();
    tau = tau > floor_tau ? tau : floor_tau;
    out[O_ESS] = (double)S / tau;
    out[O_LAG] = (double)w.t;
    out[O_RHAT] = p.rhat;
    out[O_MARGIN] = w.margin;
    out[O_SD] = p.sd;
    out[O_TAU] = tau;
}

// The Blom score of rank code n2 (average rank (n2 + 1) / 2) among S draws is inv((r - 3/8) / (S + 1/4)).
MCS_HD double blom_p(int64_t n2, int64_t S)
{
#pragma clang fp contract(off)
    const double r = (double)(n2 + 1) * 0.5;
    return (r - 0.375) / ((double)S + 0.25);
}

// numpy's "linear" quantile from the two neighbouring order statistics a <= b and the fraction g (wave_order_stats).
MCS_HD double lerp7(double a, double b, double g)
{
#pragma clang fp contract(off)
    const double d = b - a;
    return (g >= 0.5) ? b - d * (1.0 - g) : a + d * g;
}

}  // namespace mcs
