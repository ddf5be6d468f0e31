// mcr_psis.hpp -- Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry; psislw of ArviZ, psis of the
// R package loo) and PSIS-LOO: the second half of what mcr_pareto.hpp starts.  The largest importance ratios of a column
// are replaced with the expected order statistics of the generalised Pareto distribution fitted to them, the weights
// are normalised, and from a column of pointwise log-likelihoods (negate) come lppd, elpd_loo and p_loo.  The definition
// is in mcmcref_hip.h.  Everything in front of the kernels -- the pooled ascending order with every draw's position, the
// non-finite count -- is the summary pipeline's, run without diagnostics, as for k_pareto_fit.
//
//   x_(i)         the column ascending: keys[i], or with negate -keys[M-1-i]           y_(i) = x_(i) - x_(M-1)
//   tail          cut = max(y_(M-t-1), log DBL_MIN);  the n <= t values y > cut;  e_j = exp(y_(M-n+j)) - exp(cut)
//   fit           pareto_fit(e): khat, and sigma = -k / theta / scale from the unregularised k
//   smoothing     [s, e) the run of equal e_j around j,  p = (s + e) / (2 n)
//                 lw = min(log(sigma expm1(-khat log1p(-p)) / khat + exp(cut)), 0)
//   weights       log_norm = logsumexp_i lw_(i);  a draw's log weight is lw - log_norm
//   LOO           lppd = logsumexp_i(-x_(i)) - log M,  elpd = logsumexp_i(lw_(i) - x_(i)) - log_norm,  p_loo = lppd - elpd
//
// ONE text computes a column on the device and on the host (psis_column, over a "group" G that says who takes which
// index and how partial results meet).  Every sum and every maximum over the M sorted values is kPsisNT = 256 partial
// results (partial s takes the terms s, s + 256, .. in index order); each 64 consecutive partials are joined by the xor
// tree 32, 16, .. 1, and the four results r_0 .. r_3 as (r_0 + r_2) + (r_1 + r_3).  The order is a function of M alone, and
// it runs over the SORTED values, so it needs no positions and does not depend on the order the sort left among ties.
#pragma once
#include <cfloat>
#include "mcr_pareto.hpp"

namespace mcr {

constexpr int kPsisNT = 256;                  // threads of a k_psis_column workgroup = partial results of every sum
constexpr int kPsisWaves = kPsisNT / kWave;
constexpr int kPsisScratch = 16;              // doubles of LDS in front of the staged tail: the waves' partial results
constexpr int kPsisBlock = 1024;              // sorted indices of a k_psis_weights workgroup
constexpr double kPsisLogMin = -0x1.6232bdd7abcd2p+9;     // the double nearest log(DBL_MIN) = -708.3964185322641
static_assert(kPsisWaves == 4, "the join of the waves' results is written for four");

// The per-column scalars k_psis_column leaves for k_psis_weights
enum PsisCol { PS_FIRST = 0, PS_N, PS_KHAT, PS_SIGMA, PS_ECUT, PS_XMAX, PS_LOGNORM, PS_SMOOTH, kPsisCols };
// Its rows in the result table, behind the pipeline's
enum PsisRow { PR_KHAT = 0, PR_NTAIL, PR_LPPD, PR_ELPD, PR_PLOO, kPsisRows };

// The column in ascending order of x: the sort stage's ascending keys, read backwards and negated for log-likelihoods.
struct PsisKeys {
    const double* k; i64 M; int negate;
    __host__ __device__ double x(i64 i) const { return negate ? -k[M - 1 - i] : k[i]; }
};

// The tail's exceedances: staged (LDS, the free key buffer, a host array) or formed again from the keys.
struct PsisTailStaged {
    const double* e;
    __host__ __device__ double operator()(i64 j) const { return e[j]; }
};
struct PsisTailKeys {
    PsisKeys s; i64 first; double xmax, ecut;
    __host__ __device__ double operator()(i64 j) const
    {
#pragma clang fp contract(off)
        return exp(s.x(first + j) - xmax) - ecut;
    }
};

// The smoothed log ratio of tail index j of n: the expected order statistic of the fitted distribution at the middle of
// j's run of equal exceedances (a draw's weight is a function of its value alone: the sorts keep no order among ties).
template <class E>
__host__ __device__ inline double psis_smoothed(const E& e, i64 n, i64 j, double khat, double sigma, double ecut)
{
#pragma clang fp contract(off)
    const double v = e(j);
    i64 lo = -1, hi = j;                                   // e(lo) < v <= e(hi): the run's first
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if (e(mid) < v) lo = mid; else hi = mid;
    }
    const i64 s = hi;
    lo = j; hi = n;                                        // e(lo) <= v < e(hi): behind the run's last
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if (e(mid) > v) hi = mid; else lo = mid;
    }
    const double p = (double)(s + hi) / (2.0 * (double)n);
    const double l1 = log1p(-p);
    const double q = fabs(khat) < DBL_EPSILON ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
    const double lw = log(q + ecut);
    return lw < 0.0 ? lw : 0.0;
}

// The group of the host routine: one thread plays the 256 partial results in turn.
struct PsisHostGroup {
    template <int K, bool MAX, class F> __host__ __device__ void reduce(i64 n, F&& f, double (&out)[K]) const
    {
#pragma clang fp contract(off)
        double a[K][kPsisNT];
        for (int s = 0; s < kPsisNT; ++s) {
            double acc[K];
            for (int k = 0; k < K; ++k) acc[k] = MAX ? -INFINITY : 0.0;
            for (i64 i = s; i < n; i += kPsisNT) {
                double t[K];
                f(i, t);
                for (int k = 0; k < K; ++k) acc[k] = MAX ? pareto_max(acc[k], t[k]) : acc[k] + t[k];
            }
            for (int k = 0; k < K; ++k) a[k][s] = acc[k];
        }
        for (int k = 0; k < K; ++k) {
            double r[kPsisWaves];
            for (int w = 0; w < kPsisWaves; ++w) {
                double* v = a[k] + w * kWave;
                for (int o = kWave >> 1; o > 0; o >>= 1)
                    for (int l = 0; l < o; ++l) v[l] = MAX ? pareto_max(v[l], v[l + o]) : v[l] + v[l + o];
                r[w] = v[0];
            }
            out[k] = MAX ? pareto_max(pareto_max(r[0], r[2]), pareto_max(r[1], r[3])) : (r[0] + r[2]) + (r[1] + r[3]);
        }
    }
    template <class F> __host__ __device__ void for_each(i64 n, F&& f) const { for (i64 i = 0; i < n; ++i) f(i); }
    __host__ __device__ void barrier() const {}
    __host__ __device__ void share(double (&)[4]) const {}             // the finisher's values to every thread
    __host__ __device__ ParetoHostWave wave() const { return ParetoHostWave{}; }
};

// The group of the kernel: thread s holds partial result s; the waves meet through the LDS scratch sh.
struct PsisDevGroup {
    int tid; double* sh;
    template <int K, bool MAX, class F> __device__ void reduce(i64 n, F&& f, double (&out)[K]) const
    {
#pragma clang fp contract(off)
        static_assert(K * kPsisWaves <= kPsisScratch, "the scratch holds every wave's results");
        double acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = MAX ? -INFINITY : 0.0;
        for (i64 i = tid; i < n; i += kPsisNT) {
            double t[K];
            f(i, t);
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = MAX ? pareto_max(acc[k], t[k]) : acc[k] + t[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            for (int o = kWave >> 1; o > 0; o >>= 1) {
                const double u = __shfl_xor(acc[k], o, kWave);
                acc[k] = MAX ? pareto_max(acc[k], u) : acc[k] + u;
            }
        __syncthreads();                                   // (the scratch's last readers are through)
        if ((tid & (kWave - 1)) == 0)
            for (int k = 0; k < K; ++k) sh[(tid >> 6) * K + k] = acc[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double r0 = sh[k], r1 = sh[K + k], r2 = sh[2 * K + k], r3 = sh[3 * K + k];
            out[k] = MAX ? pareto_max(pareto_max(r0, r2), pareto_max(r1, r3)) : (r0 + r2) + (r1 + r3);
        }
    }
    template <class F> __device__ void for_each(i64 n, F&& f) const { for (i64 i = tid; i < n; i += kPsisNT) f(i); }
    __device__ void barrier() const { __threadfence_block(); __syncthreads(); }
    __device__ void share(double (&v)[4]) const
    {
        __syncthreads();
        if (tid == 0) for (int k = 0; k < 4; ++k) sh[k] = v[k];
        __syncthreads();
        for (int k = 0; k < 4; ++k) v[k] = sh[k];
    }
    __device__ ParetoDevWave wave() const { return ParetoDevWave{tid & (kWave - 1), tid >> 6, kPsisWaves}; }
};

// What a column comes to.
struct PsisResult {
    double khat, lppd, elpd, ploo;
    double sigma, ecut, xmax, log_norm;
    i64 first, n;                                          // the tail: x_(first) .. x_(M-1), n = M - first of them
    int smooth;
};

// The maxima and the sums of a column's K log-sum-exps, in the one order: term k of index i is t[k] of terms(i, t).
template <int K, class G, class T>
__host__ __device__ inline void psis_lse(const G& g, i64 M, T&& terms, double (&lse)[K])
{
#pragma clang fp contract(off)
    double m[K], s[K];
    g.template reduce<K, true>(M, terms, m);
    g.template reduce<K, false>(M, [&](i64 i, double (&t)[K]) {
        terms(i, t);
        for (int k = 0; k < K; ++k) t[k] = exp(t[k] - m[k]);
    }, s);
    for (int k = 0; k < K; ++k) lse[k] = m[k] + log(s[k]);
}

// One column of M >= 1 values with effective tail length t (clamped to M - 1 here once more).  e: room for t doubles,
// lg: for pareto_grid(t) doubles, both shared by the group's threads.  Every thread returns the same result.
template <class G>
__host__ __device__ inline PsisResult psis_column(const G& g, const PsisKeys& s, i64 t, double* e, double* lg)
{
#pragma clang fp contract(off)
    const i64 M = s.M;
    PsisResult c;
    c.xmax = s.x(M - 1);
    c.first = M; c.n = 0; c.khat = INFINITY; c.sigma = NAN; c.ecut = 0.0; c.smooth = 0;
    c.lppd = c.elpd = c.ploo = NAN;
    if (t > M - 1) t = M - 1;
    if (t >= 1) {
        double cut = s.x(M - t - 1) - c.xmax;
        if (!(cut > kPsisLogMin)) cut = kPsisLogMin;
        i64 lo = M - t - 1, hi = M;                        // y(lo) <= cut < y(hi): no more than t values lie above the cutoff
        while (hi - lo > 1) {
            const i64 mid = lo + (hi - lo) / 2;
            if (s.x(mid) - c.xmax > cut) hi = mid; else lo = mid;
        }
        c.first = hi;
        c.n = M - hi;
        c.ecut = exp(cut);
        if (c.n > 4) {
            const double xmax = c.xmax, ecut = c.ecut;
            const i64 first = c.first;
            g.for_each(c.n, [&](i64 j) { e[j] = exp(s.x(first + j) - xmax) - ecut; });
            g.barrier();
            double v[4] = {NAN, NAN, NAN, NAN};            // khat, then the fit's k, theta and scale
            v[0] = pareto_fit(g.wave(), (const double*)e, (int)c.n, lg, v + 1);
            g.share(v);
            c.khat = v[0] != v[0] ? INFINITY : v[0];       // (a constant tail)
            c.sigma = -v[1] / v[2] / v[3];
            c.smooth = c.khat < INFINITY && c.khat > -INFINITY && c.sigma > 0.0;
        }
    }
    const PsisTailStaged tail{e};
    auto lw = [&](i64 i) {
        return c.smooth && i >= c.first ? psis_smoothed(tail, c.n, i - c.first, c.khat, c.sigma, c.ecut) : s.x(i) - c.xmax;
    };
    if (s.negate) {
        double lse[3];
        psis_lse<3>(g, M, [&](i64 i, double (&t3)[3]) {
            const double l = lw(i), x = s.x(i);
            t3[0] = l; t3[1] = l - x; t3[2] = -x;
        }, lse);
        c.log_norm = lse[0];
        c.lppd = lse[2] - log((double)M);
        c.elpd = lse[1] - lse[0];
        c.ploo = c.lppd - c.elpd;
    } else {
        double lse[1];
        psis_lse<1>(g, M, [&](i64 i, double (&t1)[1]) { t1[0] = lw(i); }, lse);
        c.log_norm = lse[0];
    }
    return c;
}

// The log weight of sorted index i of a finished column, from the keys alone (k_psis_weights, the host routine).
__host__ __device__ inline double psis_log_weight(const PsisKeys& s, const PsisResult& c, i64 i)
{
#pragma clang fp contract(off)
    const double lw = c.smooth && i >= c.first
                          ? psis_smoothed(PsisTailKeys{s, c.first, c.xmax, c.ecut}, c.n, i - c.first, c.khat, c.sigma, c.ecut)
                          : s.x(i) - c.xmax;
    return lw - c.log_norm;
}

// ------------------------------------------------------------------------------------------------
// k_psis_column: one workgroup of 256 threads per column.  grid: ceil(pc / 8) * 8, one-dimensional (xcd_map: on the XCD
// whose L2 holds the column's keys).  The workgroup finds the tail by a search in the ascending keys, stages the n <= t
// exceedances -- behind the scratch in dynamic LDS while t <= kParetoLdsTail, else in the sort stage's free key buffer,
// where column p owns ex[p * M ..] -- runs pareto_fit over its four waves, and forms the log-sum-exps: M exp per sum and
// for every tail index two searches in the staged tail, an expm1, a log1p and a log, twice (the maxima, the sums).
// tail[p]: the effective t of column p (the host's min(t_req, M - 1)).  lgrid[p * gmax ..]: the fit's l_j, gmax >=
// pareto_grid(M - 1).  res[(field0 + PsisRow) * pc + p], cols[p * kPsisCols + PsisCol].
// Reads keys[p * M + 0 .. M-1] only: every search stays inside [M - t - 1, M], every tail index inside [0, n), n <= t.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPsisNT) void k_psis_column(const double* __restrict__ keys, i64 M, i64 pc, int negate,
                                                         const i64* __restrict__ tail, double* ex, double* lgrid, i64 gmax,
                                                         double* __restrict__ res, int field0, double* __restrict__ cols)
{
    extern __shared__ __align__(16) double sh_psis[];
    i64 p;
    int blk;
    if (!xcd_map(pc, 1, p, blk)) return;
    const int tid = threadIdx.x;
    i64 t = tail[p];
    if (t > M - 1) t = M - 1;
    if (t < 0 || pareto_grid(t) > gmax) t = 0;             // (never: the host sizes the grid scratch for M - 1)
    const bool lds = t <= kParetoLdsTail;
    double* e = lds ? sh_psis + kPsisScratch : ex + p * M;
    const PsisDevGroup g{tid, sh_psis};
    const PsisKeys s{keys + p * M, M, negate};
    const PsisResult c = psis_column(g, s, t, e, lgrid + p * gmax);
    if (tid == 0) {
        double* r = res + (i64)field0 * pc + p;
        r[PR_KHAT * pc] = c.khat; r[PR_NTAIL * pc] = (double)c.n;
        r[PR_LPPD * pc] = c.lppd; r[PR_ELPD * pc] = c.elpd; r[PR_PLOO * pc] = c.ploo;
        double* q = cols + p * kPsisCols;
        q[PS_FIRST] = (double)c.first; q[PS_N] = (double)c.n; q[PS_KHAT] = c.khat; q[PS_SIGMA] = c.sigma;
        q[PS_ECUT] = c.ecut; q[PS_XMAX] = c.xmax; q[PS_LOGNORM] = c.log_norm; q[PS_SMOOTH] = (double)c.smooth;
    }
}

// ------------------------------------------------------------------------------------------------
// k_psis_weights: the log weights in time order, launched only when they are asked for.  One workgroup per (column, block
// of kPsisBlock sorted indices); grid: ceil(pc / 8) * 8 * ceil(M / kPsisBlock), one-dimensional (xcd_map: the 8 M bytes a
// column scatters meet in one L2).  Consecutive lanes read consecutive keys and positions; a tail index forms its smoothed
// value again from the keys (the column kernel's operations on the column kernel's scalars: the same bits); one 8-byte
// store per draw to out[p * M + position].  IdxT: the sort's position width.  first and n are clamped to the column, so
// that no index leaves [0, M) whatever the scalars hold.
// ------------------------------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(256) void k_psis_weights(const double* __restrict__ keys, const IdxT* __restrict__ pos, i64 M,
                                                      i64 pc, int negate, const double* __restrict__ cols,
                                                      double* __restrict__ out)
{
    const int nb = (int)((M + kPsisBlock - 1) / kPsisBlock);
    i64 p;
    int blk;
    if (!xcd_map(pc, nb, p, blk)) return;
    const double* q = cols + p * kPsisCols;
    PsisResult c;
    c.n = (i64)q[PS_N];
    if (!(c.n >= 0 && c.n <= M)) c.n = 0;
    c.first = M - c.n;
    c.khat = q[PS_KHAT]; c.sigma = q[PS_SIGMA]; c.ecut = q[PS_ECUT]; c.xmax = q[PS_XMAX]; c.log_norm = q[PS_LOGNORM];
    c.smooth = q[PS_SMOOTH] != 0.0 && c.n > 0;
    const PsisKeys s{keys + p * M, M, negate};
    const IdxT* ps = pos + p * M;
    double* o = out + p * M;
#pragma unroll
    for (int r = 0; r < kPsisBlock / 256; ++r) {
        const i64 j = (i64)blk * kPsisBlock + r * 256 + threadIdx.x;      // the keys' order: coalesced
        if (j < M) {
            const i64 at = (i64)ps[j];
            if (at < M) o[at] = psis_log_weight(s, c, negate ? M - 1 - j : j);
        }
    }
}
}  // namespace mcr
