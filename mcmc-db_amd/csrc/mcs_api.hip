// mcs_api.hip -- the entries of include/mcmcref_std.h.  The library holds the objects of libmcmcref_hip.so's units beside
// this one (a version script keeps every name but mcs_* local): a handle owns an mcr_ctx of its own, and a call runs the
// summary pipeline of mcr_api.hip on the kept draws as ONE chain -- sort, quantiles, rank codes of x and |x - median| in
// time order -- through mcr_pipe.hpp, as mcr_stats.hip does, then the kernels of mcs_kernels.hpp.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "mcc_handle.hpp"
#include "mcs_kernels.hpp"

using namespace mcr;
using namespace mcr::host;

namespace mcs {

// limit (the context's default at first), the phase timer and the error text are the companions' common part; mcc::fail
// writes that text (a bare fail is the context's here).
struct Handle : mcc::Common<MCS_KERNELS> {
    mcr_ctx* ctx = nullptr;
    mcr::host::DevBuf blom;             // the Blom table of blom_S kept draws
    i64 blom_S = -1;
};

using mcc::g_err;

// A failure of the context's: its message becomes the handle's.
static int from_ctx(Handle* h, int rc)
{
    if (rc) std::snprintf(h->err, sizeof h->err, "%s", h->ctx->err);
    return rc;
}

// The [1] or [P] outputs of a call, in the order of the header; NULL: skipped.
struct Outs {
    double *rhat, *rhat_bulk, *rhat_tail, *ess_bulk, *ess_tail, *ess_q05, *ess_q95, *margin, *rhat_basic, *ess_mean, *mcse_mean;
    int64_t *lag_bulk, *lag_q05, *lag_q95, *lag_mean;
};

static void put(double* dst, i64 p, double v) { if (dst) dst[p] = v; }
static void put(int64_t* dst, i64 p, double v) { if (dst) dst[p] = (int64_t)v; }

// Parameter p's outputs from its series records r[nser][kOutRec].
static void scatter(const Outs& o, i64 p, const double* r, int nser)
{
    const double *bulk = r + S_BULK * kOutRec, *fold = r + S_FOLD * kOutRec, *lo = r + S_Q05 * kOutRec, *hi = r + S_Q95 * kOutRec;
    const double rb = bulk[O_RHAT], rt = fold[O_RHAT];
    put(o.rhat, p, rt > rb ? rt : rb);                      // Python's max(bulk, tail)
    put(o.rhat_bulk, p, rb);
    put(o.rhat_tail, p, rt);
    put(o.ess_bulk, p, bulk[O_ESS]);
    put(o.lag_bulk, p, bulk[O_LAG]);
    put(o.margin, p, bulk[O_MARGIN]);
    put(o.ess_q05, p, lo[O_ESS]);
    put(o.lag_q05, p, lo[O_LAG]);
    put(o.ess_q95, p, hi[O_ESS]);
    put(o.lag_q95, p, hi[O_LAG]);
    const double a = lo[O_ESS], b = hi[O_ESS];
    put(o.ess_tail, p, (std::isnan(a) || std::isnan(b)) ? (double)NAN : (b < a ? b : a));
    const double* raw = nser > S_RAW ? r + S_RAW * kOutRec : nullptr;
    put(o.rhat_basic, p, raw ? raw[O_RHAT] : (double)NAN);
    put(o.ess_mean, p, raw ? raw[O_ESS] : (double)NAN);
    put(o.lag_mean, p, raw ? raw[O_LAG] : -1.0);
    put(o.mcse_mean, p, raw ? raw[O_SD] / std::sqrt(raw[O_ESS]) : (double)NAN);
}

// What every entry refuses, in one place; `err` receives the cause.
static int check_call(char* err, const void* draws, int dtype, i64 C, i64 N, i64 P, i64 sc, i64 sn, i64 sp, int flags)
{
    if (!draws) return mcc::fail(err, MCR_EINVAL, "a NULL tensor pointer");
    if (dtype != MCR_F64 && dtype != MCR_F32) return mcc::fail(err, MCR_EINVAL, "dtype %d is neither MCR_F64 nor MCR_F32", dtype);
    if (C < 1 || P < 1 || N < 2) return mcc::fail(err, MCR_EINVAL, "C and P must be >= 1 and N >= 2 (a split chain has N / 2 draws)");
    if (N > MCS_MAX_DRAWS) return mcc::fail(err, MCR_EINVAL, "N = %lld exceeds MCS_MAX_DRAWS = %d draws per chain", (long long)N, MCS_MAX_DRAWS);
    if (C >= INT32_MAX || C * N >= (i64)INT32_MAX) return mcc::fail(err, MCR_EINVAL, "C * N must be below 2^31 - 1");
    if (sc < 0 || sn < 0 || sp < 0) return mcc::fail(err, MCR_EINVAL, "negative strides are not supported");
    if (flags & ~MCS_WANT_BASIC) return mcc::fail(err, MCR_EINVAL, "flags = %d: only MCS_WANT_BASIC is defined", flags);
    return MCR_OK;
}

// ---- the device call --------------------------------------------------------------------------------------------------

struct Call {
    const void* draws; int dtype; i64 C, N, P, sc, sn, sp; int nser;
    i64 n() const { return N / 2; }
    i64 m() const { return 2 * C; }
    i64 S() const { return m() * n(); }
    // contiguous f64 [P][C][N] with an even N is [P][2 C][n] as it lies
    bool in_place() const { return dtype == MCR_F64 && (N & 1) == 0 && !needs_ingest(C, N, P, sc, sn, sp); }
};

constexpr int kPipeFields = R_Q0 + 2;                       // the pipeline's rows with the two quantiles

// The workspace of a chunk of pc parameters: the summary pipeline's layout for one chain of S draws, then the chain
// records and the deviations.  Returns the copy of the kept draws (NULL in place).
struct Chunk {
    const Call& c;
    PipeIn a{}; double *mom = nullptr, *D = nullptr;
    double* operator()(Carve& cv, i64 pc)
    {
        const i64 S = c.S();
        a = PipeIn{};
        a.M = S; a.pc = pc; a.C = 1; a.n = 1; a.nh = 0; a.nstage = 1; a.do_diag = true;
        a.q.nq = 2;
        const double probs[2] = {0.05, 0.95};
        for (int j = 0; j < 2; ++j) {                       // numpy's virtual index (S - 1) q, as the summary's quantiles
            const double hq = (double)(S - 1) * probs[j], fl = std::floor(hq);
            a.q.lo[j] = (i64)fl;
            a.q.g[j] = hq - fl;
        }
        double* X = carve_pipe(cv, a, true, FftPlan{}, !c.in_place());
        mom = cv.take<double>((size_t)pc * c.nser * (size_t)c.m() * kMomRec);
        D = cv.take<double>((size_t)pc * c.nser * (size_t)S);
        return X;
    }
};

static int plan(Handle* h, Chunk& ch, i64& pcmax)
{
    const i64 grid_cap = ((i64)INT32_MAX / ch.c.m()) * kWaves;         // k_mcs_series: ceil(pc m / 4) workgroups
    const i64 cap = std::min<i64>(grid_cap, kMaxGridY / 2);
    auto measure = [&](i64 pc) { Carve mcv{nullptr}; ch(mcv, pc); return mcv.off; };
    pcmax = most_that_fit(std::min(ch.c.P, cap), [&](i64 pc) { return measure(pc) <= h->limit; });
    if (!pcmax) return mcc::fail(h->err, MCR_ENOMEM, "one parameter needs %zu bytes of workspace; the limit is %zu", measure(1), h->limit);
    return MCR_OK;
}

static int get_blom(Handle* h, i64 S, double** out)
{
    mcr_ctx* ctx = h->ctx;
    if (h->blom_S != S) {
        h->blom_S = -1;
        if (const int rc = h->blom.reserve(ctx, sizeof(double) * (size_t)(2 * S))) return rc;
        hipLaunchKernelGGL(k_mcs_blom, dim3((unsigned)((2 * S + 255) / 256)), dim3(256), 0, ctx->stream, h->blom.as<double>(), S);
        HIP_TRY(ctx, hipGetLastError());
        h->blom_S = S;
    }
    *out = h->blom.as<double>();
    return MCR_OK;
}

#define MCS_LAUNCHED(ctx, what)                                                                             \
    do {                                                                                                    \
        const hipError_t le_ = hipGetLastError();                                                           \
        if (le_ != hipSuccess) return fail(ctx, MCR_EHIP, "launch %s failed: %s", what, hipGetErrorString(le_)); \
    } while (0)

// The call on the context; a failure leaves its message in ctx->err.
static int run_ctx(Handle* h, const Call& c, const Outs& o)
{
    mcr_ctx* ctx = h->ctx;
    const i64 n = c.n(), m = c.m(), S = c.S(), P = c.P;
    Chunk ch{c};
    i64 pcmax = 0;
    if (plan(h, ch, pcmax)) { std::snprintf(ctx->err, sizeof ctx->err, "%s", h->err); return MCR_ENOMEM; }
    double *ztab = nullptr, *blom = nullptr, *d_res = nullptr, *d_out = nullptr;
    int rc = get_ztab(ctx, S, &ztab);
    if (!rc) rc = get_blom(h, S, &blom);
    const size_t res_n = (size_t)kPipeFields * (size_t)P, out_n = (size_t)P * c.nser * kOutRec;
    if (!rc) rc = carve(ctx, ctx->call_dev, [&](Carve& cv) { d_res = cv.take<double>(res_n); d_out = cv.take<double>(out_n); });
    if (rc) return rc;
    const bool lds = n <= kLdsDraws;
    for (i64 p0 = 0; p0 < P; p0 += pcmax) {
        const i64 pc = std::min(P - p0, pcmax);
        double* copy = nullptr;
        rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { copy = ch(cv, pc); });
        if (rc) return rc;
        HIP_TRY(ctx, h->timer.begin(ctx->stream));
        const double* X = copy;
        if (c.in_place()) X = reinterpret_cast<const double*>(c.draws) + p0 * S;
        else if ((c.N & 1) == 0) rc = launch_ingest(ctx, c.draws, c.dtype, copy, c.C, c.N, pc, c.sc, c.sn, c.sp, p0);
        else {
            const i64 blocks = (pc * S + 255) / 256;
            const dim3 grid((unsigned)std::min<i64>(blocks, (i64)1 << 20));
            if (c.dtype == MCR_F64)
                hipLaunchKernelGGL(k_mcs_copy_split<double>, grid, dim3(256), 0, ctx->stream, (const double*)c.draws, copy, c.C, c.N, pc, c.sc, c.sn, c.sp, p0);
            else
                hipLaunchKernelGGL(k_mcs_copy_split<float>, grid, dim3(256), 0, ctx->stream, (const float*)c.draws, copy, c.C, c.N, pc, c.sc, c.sn, c.sp, p0);
            MCS_LAUNCHED(ctx, "k_mcs_copy_split");
        }
        if (rc) return rc;
        PipeIn& a = ch.a;
        a.ztab = ztab;
        a.X = X;
        a.d_res = d_res + (size_t)kPipeFields * (size_t)p0;
        rc = run_pipeline(ctx, a);                          // one chain: sort, quantiles, bulk codes, fold, finalize (the bad count)
        if (rc) return rc;
        HIP_TRY(ctx, h->timer.mark(ctx->stream, MCS_KERNEL_PIPE));
        const SeriesIn si{X, a.zb, a.zt, blom, a.d_res, m, n, pc, c.nser};
        hipLaunchKernelGGL(k_mcs_series, dim3((unsigned)((pc * m + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, si, ch.D, ch.mom);
        MCS_LAUNCHED(ctx, "k_mcs_series");
        HIP_TRY(ctx, h->timer.mark(ctx->stream, MCS_KERNEL_SERIES));
        double* out_at = d_out + (size_t)p0 * c.nser * kOutRec;
        const dim3 wgrid((unsigned)pc, (unsigned)c.nser);
        if (lds) hipLaunchKernelGGL(k_mcs_walk<true>, wgrid, dim3(kThreads), (size_t)n * 8, ctx->stream, (const double*)ch.D, (const double*)ch.mom, m, n, c.nser, out_at);
        else hipLaunchKernelGGL(k_mcs_walk<false>, wgrid, dim3(kThreads), 0, ctx->stream, (const double*)ch.D, (const double*)ch.mom, m, n, c.nser, out_at);
        MCS_LAUNCHED(ctx, "k_mcs_walk");
        HIP_TRY(ctx, h->timer.mark(ctx->stream, MCS_KERNEL_WALK));
        if (h->timer.on) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, h->timer.collect());
        }
    }
    const size_t bytes = sizeof(double) * (res_n + out_n);
    rc = ctx->call_host.reserve(ctx, bytes);
    if (rc) return rc;
    double* hres = ctx->call_host.as<double>();
    double* hout = hres + res_n;
    HIP_TRY(ctx, hipMemcpyAsync(hres, d_res, sizeof(double) * res_n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hout, d_out, sizeof(double) * out_n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (i64 at = 0; at < P; ++at) {
        const i64 p = at % pcmax, p0 = at - p, pc = std::min(P - p0, pcmax);
        nbad += hres[(size_t)kPipeFields * (size_t)p0 + (size_t)R_BAD * pc + p];
        scatter(o, at, hout + (size_t)at * c.nser * kOutRec, c.nser);
    }
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

static int run_dev(Handle* h, Call c, const Outs& o, bool host)
{
    mcr_ctx* ctx = h->ctx;
    h->timer.clear();
    if (hipSetDevice(ctx->device) != hipSuccess) return mcc::fail(h->err, MCR_EHIP, "hipSetDevice(%d) failed", ctx->device);
    int rc = MCR_OK;
    if (host) {                                             // the span the strides reach, into the context's staging buffer
        const size_t bytes = (size_t)tensor_extent(c.C, c.N, c.P, c.sc, c.sn, c.sp) * (c.dtype == MCR_F64 ? 8 : 4);
        void* X = nullptr;
        rc = stage_buffers(ctx, {bytes}, &X);
        if (!rc && hipMemcpyAsync(X, c.draws, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            rc = fail(ctx, MCR_EHIP, "the upload of the tensor failed");
        c.draws = X;
    }
    if (!rc) rc = run_ctx(h, c, o);
    if (rc && rc != MCR_ENONFINITE) rc = drain(ctx, rc, true);
    return from_ctx(h, rc);
}

// ---- the definition on the host ------------------------------------------------------------------------------------------

// AS241 (Wichura 1988) PPND16 with libm's log and sqrt: the evaluation order of the device's inv_cdf (mcr_device.hpp).
static double host_inv_cdf(double p)
{
#pragma clang fp contract(off)
    double q = p - 0.5, r, num, den, x;
    if (std::fabs(q) <= 0.425) {
        r = 0.180625 - q * q;
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                   4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                   2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    r = (q <= 0.0) ? p : 1.0 - p;
    r = std::sqrt(-std::log(r));
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                5.99832206555887937690e-1) * r + 1.0);
    }
    x = num / den;
    return (q < 0.0) ? -x : x;
}

// The ascending order of v (ties in any order) and the Blom scores of its tie-averaged ranks.
static void host_scores(const std::vector<double>& v, std::vector<double>& sorted, std::vector<double>& score)
{
    const i64 S = (i64)v.size();
    std::vector<i64> idx((size_t)S);
    std::iota(idx.begin(), idx.end(), (i64)0);
    std::sort(idx.begin(), idx.end(), [&](i64 a, i64 b) { return v[(size_t)a] < v[(size_t)b]; });
    sorted.resize((size_t)S);
    score.resize((size_t)S);
    for (i64 i = 0; i < S;) {
        i64 j = i + 1;
        while (j < S && v[(size_t)idx[(size_t)j]] == v[(size_t)idx[(size_t)i]]) ++j;
        const double z = host_inv_cdf(blom_p(i + j, S));    // the run's average rank (i + 1 + j) / 2 has code i + j
        for (i64 r = i; r < j; ++r) { sorted[(size_t)r] = v[(size_t)idx[(size_t)r]]; score[(size_t)idx[(size_t)r]] = z; }
        i = j;
    }
}

// One series v[m][n] by the definition, into out[kOutRec].
static void host_series(const double* v, i64 m, i64 n, double* out)
{
#pragma clang fp contract(off)
    std::vector<double> mom((size_t)(m * kMomRec)), d((size_t)(m * n));
    for (i64 k = 0; k < m; ++k) {
        const double* vk = v + k * n;
        double part[kLanes], lo = vk[0], hi = vk[0];
        for (int l = 0; l < kLanes; ++l) part[l] = lane_partial([&](i64 i) { return vk[i]; }, n, l);
        const double mean = tree64(part) / (double)n;
        for (i64 i = 0; i < n; ++i) {
            d[(size_t)(k * n + i)] = vk[i] - mean;
            lo = vk[i] < lo ? vk[i] : lo;
            hi = vk[i] > hi ? vk[i] : hi;
        }
        const double* dk = d.data() + k * n;
        for (int l = 0; l < kLanes; ++l) part[l] = lane_partial([&](i64 i) { return dk[i] * dk[i]; }, n, l);
        double* r = mom.data() + k * kMomRec;
        r[0] = mean; r[1] = tree64(part); r[2] = lo; r[3] = hi;
    }
    const Pool pool = pool_of([&](i64 k, int f) { return mom[(size_t)(k * kMomRec + f)]; }, m, n);
    if (n < 4 || pool.constant) { out_unwalked(pool, out); return; }
    auto gamma = [&](i64 t) {
        double g = 0.0;
        for (i64 k = 0; k < m; ++k) g = g + lag_product(d.data() + k * n, n, t) / (double)n;
        return g / (double)m;
    };
    Walk w;
    if (!w.start(gamma(0), gamma(1), pool.var_means, n)) {
        out_unwalked(pool, out);
        out[O_RHAT] = NAN;
        return;
    }
    while (!w.done) {
        const double ge = gamma(w.t + 2), go = gamma(w.t + 3);
        w.step(ge, go);
    }
    out_walked(pool, w, m * n, out);
}

static int host_param(const double* chains, i64 C, i64 N, int flags, const Outs& o)
{
    const i64 n = N / 2, m = 2 * C, S = m * n;
    const int nser = (flags & MCS_WANT_BASIC) ? kSeries : kSeries - 1;
    std::vector<double> x((size_t)S);
    for (i64 k = 0; k < m; ++k)
        for (i64 i = 0; i < n; ++i) x[(size_t)(k * n + i)] = chains[(k >> 1) * N + (k & 1) * (N - n) + i];
    for (double v : x)
        if (!std::isfinite(v)) return mcc::fail(g_err, MCR_ENONFINITE, "draws contain non-finite value(s)");
    std::vector<double> sorted, series((size_t)S), unused, fold((size_t)S);
    std::vector<double> out((size_t)(nser * kOutRec));
    host_scores(x, sorted, series);
    host_series(series.data(), m, n, out.data() + S_BULK * kOutRec);
    const double med = (sorted[(size_t)(S / 2 - 1)] + sorted[(size_t)(S / 2)]) / 2.0;      // S is even
    for (i64 i = 0; i < S; ++i) fold[(size_t)i] = std::fabs(x[(size_t)i] - med);
    host_scores(fold, unused, series);
    host_series(series.data(), m, n, out.data() + S_FOLD * kOutRec);
    const double probs[2] = {0.05, 0.95};
    for (int j = 0; j < 2; ++j) {
        const double hq = (double)(S - 1) * probs[j], fl = std::floor(hq);
        const i64 lo = (i64)fl, hi = lo + 1 < S ? lo + 1 : S - 1;
        const double q = lerp7(sorted[(size_t)lo], sorted[(size_t)hi], hq - fl);
        for (i64 i = 0; i < S; ++i) series[(size_t)i] = x[(size_t)i] <= q ? 1.0 : 0.0;
        host_series(series.data(), m, n, out.data() + (S_Q05 + j) * kOutRec);
    }
    if (nser > S_RAW) host_series(x.data(), m, n, out.data() + S_RAW * kOutRec);
    scatter(o, 0, out.data(), nser);
    return MCR_OK;
}

}  // namespace mcs

using namespace mcs;

extern "C" {

#define MCS_EXPORT __attribute__((visibility("default")))
#define MCS_OUTS_PARAMS                                                                                                      \
    double *rhat, double *rhat_bulk, double *rhat_tail, double *ess_bulk, double *ess_tail, double *ess_q05, double *ess_q95, \
        double *margin, double *rhat_basic, double *ess_mean, double *mcse_mean, int64_t *lag_bulk, int64_t *lag_q05,        \
        int64_t *lag_q95, int64_t *lag_mean
#define MCS_OUTS                                                                                                             \
    Outs { rhat, rhat_bulk, rhat_tail, ess_bulk, ess_tail, ess_q05, ess_q95, margin, rhat_basic, ess_mean, mcse_mean, lag_bulk, \
           lag_q05, lag_q95, lag_mean }

MCS_EXPORT int mcs_version(void) { return MCS_VERSION; }

MCS_EXPORT void mcs_free(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)sync_all(h->ctx);
    }
    h->blom.release();
    h->timer.destroy();
    if (h->ctx) mcr_free(h->ctx);
    delete h;
}

MCS_EXPORT int mcs_init(int device, void** handle)
{
    if (!handle) return mcc::fail(g_err, MCR_EINVAL, "mcs_init: NULL handle pointer");
    *handle = nullptr;
    Handle* h = new Handle;
    const int rc = mcr_init(device, &h->ctx);
    if (rc) {
        std::snprintf(g_err, sizeof g_err, "%s", mcr_last_error(nullptr));
        h->ctx = nullptr;
        delete h;
        return rc;
    }
    const hipError_t e = h->timer.create();
    if (e != hipSuccess) {
        mcc::fail(g_err, MCR_EHIP, "mcs_init: %s", hipGetErrorString(e));
        mcs_free(h);
        return MCR_EHIP;
    }
    h->limit = h->ctx->ws_limit;
    *handle = h;
    return MCR_OK;
}

MCS_EXPORT const char* mcs_last_error(void* handle) { return mcc::last_error((Handle*)handle); }

MCS_EXPORT int mcs_set_workspace_limit(void* handle, size_t bytes) { return mcc::set_workspace_limit((Handle*)handle, bytes); }

MCS_EXPORT int mcs_plan(void* handle, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                        int64_t stride_p, int flags, int64_t* params_per_chunk)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (!params_per_chunk) return mcc::fail(h->err, MCR_EINVAL, "a NULL result pointer");
    if (const int rc = check_call(h->err, h, dtype, C, N, P, stride_c, stride_n, stride_p, flags)) return rc;
    const Call c{nullptr, dtype, C, N, P, stride_c, stride_n, stride_p, (flags & MCS_WANT_BASIC) ? kSeries : kSeries - 1};
    Chunk ch{c};
    i64 pcmax = 0;
    if (const int rc = plan(h, ch, pcmax)) return rc;
    *params_per_chunk = pcmax;
    return MCR_OK;
}

MCS_EXPORT int mcs_diagnostics_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                                   int64_t stride_n, int64_t stride_p, int flags, MCS_OUTS_PARAMS)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_call(h->err, draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p, flags)) return rc;
    const Call c{draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p, (flags & MCS_WANT_BASIC) ? kSeries : kSeries - 1};
    return run_dev(h, c, MCS_OUTS, false);
}

MCS_EXPORT int mcs_diagnostics(void* handle, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                               int64_t stride_n, int64_t stride_p, int flags, MCS_OUTS_PARAMS)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_call(h->err, draws, dtype, C, N, P, stride_c, stride_n, stride_p, flags)) return rc;
    const Call c{draws, dtype, C, N, P, stride_c, stride_n, stride_p, (flags & MCS_WANT_BASIC) ? kSeries : kSeries - 1};
    return run_dev(h, c, MCS_OUTS, true);
}

MCS_EXPORT int mcs_diagnostics_host(const double* chains, int64_t C, int64_t N, int flags, MCS_OUTS_PARAMS)
{
    if (const int rc = check_call(g_err, chains, MCR_F64, C, N, 1, N, 1, 0, flags)) return rc;
    return host_param(chains, C, N, flags, MCS_OUTS);
}

MCS_EXPORT int mcs_profile_enable(void* handle, int on) { return mcc::profile_enable((Handle*)handle, on); }

MCS_EXPORT int mcs_kernel_ms(void* handle, double* ms, int cap) { return mcc::kernel_ms((Handle*)handle, "mcs", "MCS", ms, cap); }

}  // extern "C"
