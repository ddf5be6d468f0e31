// mce_api.hip -- the entries of include/mcmcref_recdf.h.  As libmcmcref_std.so the library holds the objects of
// libmcmcref_hip.so's units beside this one (a version script keeps every name but mce_* local): a handle owns an mcr_ctx
// of its own, and a call runs the summary pipeline of mcr_api.hip on the kept draws as ONE chain without diagnostics --
// the sort and the non-finite count -- through mcr_pipe.hpp, then the kernels of mce_kernels.hpp on the sorted keys.  The
// null sample is the same path on draws a kernel writes, a chunk of simulations at a time.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mcc_handle.hpp"
#include "mce_kernels.hpp"
#include "mcr_pipe.hpp"

using namespace mcr;
using namespace mcr::host;

namespace mce {

// limit (the context's default at first), the kernel timer and the error text are the companions' common part.
struct Handle : mcc::Common<MCE_KERNELS> {
    mcr_ctx* ctx = nullptr;
    mcr::host::DevBuf table;            // the pointwise table of (tab_M, tab_n, tab_K)
    i64 tab_M = -1, tab_n = -1;
    int tab_K = -1;
};

using mcc::g_err;

static int from_ctx(Handle* h, int rc)
{
    if (rc) std::snprintf(h->err, sizeof h->err, "%s", h->ctx->err);
    return rc;
}

// The outputs of a call, in the order of the header; NULL: skipped.
struct Outs {
    int32_t *counts, *pooled, *tied; double* u; int32_t* kmin; int64_t* dev; double* g; int32_t* chain;
};

// What every entry refuses of a shape, in one place; `err` receives the cause.
static int check_shape(char* err, i64 C, i64 n, int K)
{
    if (C < 1 || n < 1) return mcc::fail(err, MCR_EINVAL, "C and n must be >= 1");
    if (C >= INT32_MAX || n >= INT32_MAX || C * n >= (i64)INT32_MAX) return mcc::fail(err, MCR_EINVAL, "C * n must be below 2^31 - 1");
    if (K < 2 || K > MCE_MAX_POINTS || K > C * n)
        return mcc::fail(err, MCR_EINVAL, "K = %d: the points must be in [2, min(C * n, MCE_MAX_POINTS = %d)]", K, MCE_MAX_POINTS);
    if ((i64)(K - 1) * (n + 1) > (i64)MCE_MAX_TABLE)
        return mcc::fail(err, MCR_EINVAL, "(K - 1)(n + 1) = %lld exceeds MCE_MAX_TABLE = %d table entries", (long long)((i64)(K - 1) * (n + 1)), MCE_MAX_TABLE);
    return MCR_OK;
}

static int check_call(char* err, const void* draws, int dtype, i64 C, i64 n, i64 P, i64 sc, i64 sn, i64 sp, int K)
{
    if (!draws) return mcc::fail(err, MCR_EINVAL, "a NULL tensor pointer");
    if (dtype != MCR_F64 && dtype != MCR_F32) return mcc::fail(err, MCR_EINVAL, "dtype %d is neither MCR_F64 nor MCR_F32", dtype);
    if (P < 1) return mcc::fail(err, MCR_EINVAL, "P must be >= 1");
    if (sc < 0 || sn < 0 || sp < 0) return mcc::fail(err, MCR_EINVAL, "negative strides are not supported");
    return check_shape(err, C, n, K);
}

// ---- the pointwise table (the header: "Pointwise table") ----------------------------------------------------------------

// Row k of the table: U[j], j = 0 .. n, for X ~ Hypergeometric(M, m marked, n drawn).  w: n + 1 doubles of scratch.
static void table_row(i64 M, i64 m, i64 n, double* U, double* w)
{
#pragma clang fp contract(off)
    const i64 lo = n - (M - m) > 0 ? n - (M - m) : 0, hi = n < m ? n : m;
    i64 mode = (n + 1) * (m + 1) / (M + 2);
    mode = mode < lo ? lo : (mode > hi ? hi : mode);
    // w_{j+1} / w_j = (m - j)(n - j) / ((j + 1)(M - m - n + j + 1))
    auto up = [&](i64 j) { return ((double)(m - j) * (double)(n - j)) / ((double)(j + 1) * (double)(M - m - n + j + 1)); };
    auto down = [&](i64 j) { return ((double)j * (double)(M - m - n + j)) / ((double)(m - j + 1) * (double)(n - j + 1)); };   // w_{j-1} / w_j
    w[mode] = 1.0;
    for (i64 j = mode; j < hi; ++j) w[j + 1] = w[j] * up(j);
    for (i64 j = mode; j > lo; --j) w[j - 1] = w[j] * down(j);
    double total = 0.0;                                     // small to large on either side of the mode
    {
        double below = 0.0, above = 0.0;
        for (i64 j = lo; j < mode; ++j) below = below + w[j];
        for (i64 j = hi; j > mode; --j) above = above + w[j];
        total = (below + above) + w[mode];
    }
    for (i64 j = 0; j <= n; ++j) U[j] = 0.0;
    double acc = 0.0;
    for (i64 j = lo; j <= hi; ++j) { acc = acc + w[j]; U[j] = acc; }          // P(X <= j) total, from the low end inward
    acc = 0.0;
    for (i64 j = hi; j >= lo; --j) {                        // P(X >= j) total, from the high end inward
        acc = acc + w[j];
        U[j] = (acc < U[j] ? acc : U[j]) / total;
    }
}

static void table_host(i64 M, i64 n, int K, double* table)
{
    std::vector<double> w((size_t)(n + 1));
    for (int k = 1; k < K; ++k) table_row(M, point_rank(k, M, K), n, table + (size_t)(k - 1) * (size_t)(n + 1), w.data());
}

// ---- the definition on the host ---------------------------------------------------------------------------------------

// One parameter x[C][n] (finite) by the definition; scratch vectors are the caller's, for the null sample's loop.
struct HostWork { std::vector<double> sorted, chain; std::vector<int32_t> a, R; };

static void host_param(const double* x, i64 C, i64 n, int K, const double* table, const Outs& o, HostWork& hw)
{
    const i64 M = C * n;
    const size_t K1 = (size_t)(K - 1);
    hw.sorted.assign(x, x + M);
    std::sort(hw.sorted.begin(), hw.sorted.end());
    hw.a.assign((size_t)C * K1, 0);
    hw.R.assign(K1, 0);
    hw.chain.resize((size_t)n);
    for (i64 c = 0; c < C; ++c) {
        std::copy(x + c * n, x + (c + 1) * n, hw.chain.begin());
        std::sort(hw.chain.begin(), hw.chain.end());
        for (int k = 1; k < K; ++k) {
            const double t = hw.sorted[(size_t)(point_rank(k, M, K) - 1)];
            const int32_t a = (int32_t)(std::upper_bound(hw.chain.begin(), hw.chain.end(), t) - hw.chain.begin());       // #{ x <= t }
            hw.a[(size_t)c * K1 + (size_t)(k - 1)] = a;
            hw.R[(size_t)(k - 1)] += a;
        }
    }
    int32_t tied = 0;
    for (int k = 1; k < K; ++k) tied += hw.R[(size_t)(k - 1)] != point_rank(k, M, K) ? 1 : 0;
    Cand best = Cand::none();
    for (i64 c = 0; c < C; ++c) {
        Cand cb = Cand::none();
        i64 gap = 0;
        for (int k = 1; k < K; ++k) {
            const i64 a = hw.a[(size_t)c * K1 + (size_t)(k - 1)];
            take(cb, table[(size_t)(k - 1) * (size_t)(n + 1) + (size_t)a], k);
            const i64 e = ecdf_gap(a, hw.R[(size_t)(k - 1)], M, n);
            gap = e > gap ? e : gap;
        }
        if (o.u) o.u[c] = cb.w;
        if (o.kmin) o.kmin[c] = (int32_t)cb.i;
        if (o.dev) o.dev[c] = gap;
        take(best, cb.w, c);
    }
    if (o.counts) std::copy(hw.a.begin(), hw.a.end(), o.counts);
    if (o.pooled) std::copy(hw.R.begin(), hw.R.end(), o.pooled);
    if (o.tied) *o.tied = tied;
    if (o.g) *o.g = best.w;
    if (o.chain) *o.chain = (int32_t)best.i;
}

// ---- the device call --------------------------------------------------------------------------------------------------

// A tensor call (draws != NULL) or a null sample (P simulations from `seed`).
struct Call {
    const void* draws; int dtype; i64 C, n, P, sc, sn, sp; int K; u64 seed;
    i64 M() const { return C * n; }
    bool null() const { return draws == nullptr; }
    // contiguous f64 [P][C][n] is read as it lies
    bool in_place() const { return !null() && dtype == MCR_F64 && !needs_ingest(C, n, P, sc, sn, sp); }
    int tile() const { return chain_tile(C, n, K); }
    i64 nb() const { return (C + tile() - 1) / tile(); }
};

constexpr int kPipeFields = R_Q0;                           // the pipeline runs without quantiles: its rows end here

// The workspace of a chunk of pc parameters: the summary pipeline's layout for one chain of M draws, sort only, with the
// split points k_order_stats writes; the null sample's counts, which nobody reads back, behind it.  Returns the f64 copy
// of the draws (NULL in place).
struct Chunk {
    const Call& c;
    PipeIn a{}; int32_t* counts = nullptr;
    double* operator()(Carve& cv, i64 pc)
    {
        a = PipeIn{};
        a.M = c.M(); a.pc = pc; a.C = 1; a.n = 1; a.nh = 0; a.nstage = 1; a.q.nq = 0; a.do_diag = false;
        double* X = carve_pipe(cv, a, false, FftPlan{}, !c.in_place());
        a.split = cv.take<i64>((size_t)pc);
        counts = c.null() ? cv.take<int32_t>((size_t)pc * (size_t)c.C * (size_t)(c.K - 1)) : nullptr;
        return X;
    }
};

static int plan(Handle* h, Chunk& ch, i64& pcmax)
{
    const i64 grid_cap = ((i64)INT32_MAX / ch.c.nb()) / 8 * 8 - 8;      // k_mce_count: ceil(pc / 8) * 8 * nb workgroups
    if (grid_cap < 1) return mcc::fail(h->err, MCR_EINVAL, "%lld tiles of chains per parameter exceed a launch", (long long)ch.c.nb());
    const i64 cap = std::min<i64>(grid_cap, kMaxGridY / 2);
    auto measure = [&](i64 pc) { Carve mcv{nullptr}; ch(mcv, pc); return mcv.off; };
    pcmax = most_that_fit(std::min(ch.c.P, cap), [&](i64 pc) { return measure(pc) <= h->limit; });
    if (!pcmax) return mcc::fail(h->err, MCR_ENOMEM, "one parameter needs %zu bytes of workspace; the limit is %zu", measure(1), h->limit);
    return MCR_OK;
}

// The table of (M, n, K) on the device: computed on the host and uploaded when the handle holds another.
static int get_table(Handle* h, i64 M, i64 n, int K, const double** out)
{
    mcr_ctx* ctx = h->ctx;
    if (h->tab_M != M || h->tab_n != n || h->tab_K != K) {
        h->tab_M = -1;
        const size_t entries = (size_t)(K - 1) * (size_t)(n + 1);
        std::vector<double> tab(entries);
        table_host(M, n, K, tab.data());
        if (const int rc = h->table.reserve(ctx, sizeof(double) * entries)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(h->table.as<double>(), tab.data(), sizeof(double) * entries, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));    // (tab leaves scope)
        h->tab_M = M; h->tab_n = n; h->tab_K = K;
    }
    *out = h->table.as<double>();
    return MCR_OK;
}

#define MCE_LAUNCHED(ctx, what)                                                                             \
    do {                                                                                                    \
        const hipError_t le_ = hipGetLastError();                                                           \
        if (le_ != hipSuccess) return fail(ctx, MCR_EHIP, "launch %s failed: %s", what, hipGetErrorString(le_)); \
    } while (0)

// The whole call's outputs on the device and on the host: one buffer each, the arrays in the order of Outs.
struct Results {
    double* res = nullptr; int32_t *counts = nullptr, *pooled = nullptr, *tied = nullptr; double* u = nullptr; int32_t* kmin = nullptr;
    int64_t* dev = nullptr; double* g = nullptr; int32_t* chain = nullptr;
    void operator()(Carve& cv, const Call& c)
    {
        const size_t P = (size_t)c.P, C = (size_t)c.C, K1 = (size_t)(c.K - 1);
        res = cv.take<double>((size_t)kPipeFields * P);
        g = cv.take<double>(P);
        if (c.null()) return;
        counts = cv.take<int32_t>(P * C * K1);
        pooled = cv.take<int32_t>(P * K1);
        tied = cv.take<int32_t>(P);
        u = cv.take<double>(P * C);
        kmin = cv.take<int32_t>(P * C);
        dev = cv.take<int64_t>(P * C);
        chain = cv.take<int32_t>(P);
    }
};

template <typename T> static void give(T* dst, const T* src, size_t count)
{
    if (dst) std::memcpy(dst, src, sizeof(T) * count);
}

// The call on the context; a failure leaves its message in ctx->err.
static int run_ctx(Handle* h, const Call& c, const Outs& o)
{
    mcr_ctx* ctx = h->ctx;
    const i64 n = c.n, M = c.M(), P = c.P;
    const int K = c.K, ct = c.tile(), nb = (int)c.nb();
    Chunk ch{c};
    i64 pcmax = 0;
    if (plan(h, ch, pcmax)) { std::snprintf(ctx->err, sizeof ctx->err, "%s", h->err); return MCR_ENOMEM; }
    const double* table = nullptr;
    int rc = get_table(h, M, n, K, &table);
    Results d;
    size_t bytes = 0;
    if (!rc) rc = carve(ctx, ctx->call_dev, [&](Carve& cv) { d(cv, c); bytes = cv.off; });
    if (rc) return rc;
    for (i64 p0 = 0; p0 < P; p0 += pcmax) {
        const i64 pc = std::min(P - p0, pcmax);
        double* copy = nullptr;
        rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { copy = ch(cv, pc); });
        if (rc) return rc;
        HIP_TRY(ctx, h->timer.begin(ctx->stream));
        const double* X = copy;
        if (c.null()) {
            const i64 total = pc * M, blocks = ((total >> 1) + kNT - 1) / kNT;
            const u64 base = c.seed * 0x9E3779B97F4A7C15ull + (u64)p0 * (u64)M;
            hipLaunchKernelGGL(k_mce_null, dim3((unsigned)std::min<i64>(std::max<i64>(blocks, 1), 4096)), dim3(kNT), 0, ctx->stream, copy, total, base);
            MCE_LAUNCHED(ctx, "k_mce_null");
            HIP_TRY(ctx, h->timer.mark(ctx->stream, MCE_KERNEL_FILL));
        } else if (c.in_place()) X = reinterpret_cast<const double*>(c.draws) + p0 * M;
        else rc = launch_ingest(ctx, c.draws, c.dtype, copy, c.C, c.n, pc, c.sc, c.sn, c.sp, p0);
        if (rc) return rc;
        PipeIn& a = ch.a;
        a.X = X;
        a.d_res = d.res + (size_t)kPipeFields * (size_t)p0;
        Sorted so;
        rc = run_pipeline(ctx, a, &so);                     // one chain: sort, order statistics, finalize (the bad count)
        if (rc) return rc;
        HIP_TRY(ctx, h->timer.mark(ctx->stream, MCE_KERNEL_PIPE));
        int32_t* counts = c.null() ? ch.counts : d.counts + (size_t)p0 * (size_t)c.C * (size_t)(K - 1);
        hipLaunchKernelGGL(k_mce_count, dim3((unsigned)((pc + 7) / 8 * 8 * nb)), dim3(kNT), (size_t)ct * K * sizeof(unsigned), ctx->stream, X,
                           (const double*)so.keys, M, n, (int)c.C, pc, K, ct, nb, counts);
        MCE_LAUNCHED(ctx, "k_mce_count");
        HIP_TRY(ctx, h->timer.mark(ctx->stream, MCE_KERNEL_COUNT));
        auto at = [&](auto* base, size_t per) { return base ? base + (size_t)p0 * per : base; };
        hipLaunchKernelGGL(k_mce_stat, dim3((unsigned)pc), dim3(kNT), 0, ctx->stream, (const int32_t*)counts, table, M, n, (int)c.C, K,
                           at(d.pooled, (size_t)(K - 1)), at(d.tied, 1), at(d.u, (size_t)c.C), at(d.kmin, (size_t)c.C), at(d.dev, (size_t)c.C),
                           at(d.g, 1), at(d.chain, 1));
        MCE_LAUNCHED(ctx, "k_mce_stat");
        HIP_TRY(ctx, h->timer.mark(ctx->stream, MCE_KERNEL_STAT));
        if (h->timer.on) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, h->timer.collect());
        }
    }
    rc = ctx->call_host.reserve(ctx, bytes);
    if (rc) return rc;
    char* hb = ctx->call_host.as<char>();
    HIP_TRY(ctx, hipMemcpyAsync(hb, ctx->call_dev.as<char>(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    Results r;
    Carve hcv{hb, bytes};
    r(hcv, c);
    if (!c.null()) {
        double nbad = 0.0;
        for (i64 at = 0; at < P; ++at) {
            const i64 p = at % pcmax, p0 = at - p, pc = std::min(P - p0, pcmax);
            nbad += r.res[(size_t)kPipeFields * (size_t)p0 + (size_t)R_BAD * pc + p];
        }
        if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    }
    const size_t Ps = (size_t)P, Cs = (size_t)c.C, K1 = (size_t)(K - 1);
    give(o.g, r.g, Ps);
    if (c.null()) return MCR_OK;
    give(o.counts, r.counts, Ps * Cs * K1);
    give(o.pooled, r.pooled, Ps * K1);
    give(o.tied, r.tied, Ps);
    give(o.u, r.u, Ps * Cs);
    give(o.kmin, r.kmin, Ps * Cs);
    give(o.dev, r.dev, Ps * Cs);
    give(o.chain, r.chain, Ps);
    return MCR_OK;
}

static int run_dev(Handle* h, Call c, const Outs& o, bool host)
{
    mcr_ctx* ctx = h->ctx;
    h->timer.clear();
    if (hipSetDevice(ctx->device) != hipSuccess) return mcc::fail(h->err, MCR_EHIP, "hipSetDevice(%d) failed", ctx->device);
    int rc = MCR_OK;
    if (host) {                                             // the span the strides reach, into the context's staging buffer
        const size_t bytes = (size_t)tensor_extent(c.C, c.n, c.P, c.sc, c.sn, c.sp) * (c.dtype == MCR_F64 ? 8 : 4);
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

}  // namespace mce

using namespace mce;

extern "C" {

#define MCE_EXPORT __attribute__((visibility("default")))
#define MCE_OUTS_PARAMS int32_t *counts, int32_t *pooled, int32_t *tied, double *u, int32_t *kmin, int64_t *dev, double *g, int32_t *chain
#define MCE_OUTS Outs { counts, pooled, tied, u, kmin, dev, g, chain }

MCE_EXPORT int mce_version(void) { return MCE_VERSION; }

MCE_EXPORT void mce_free(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)sync_all(h->ctx);
    }
    h->table.release();
    h->timer.destroy();
    if (h->ctx) mcr_free(h->ctx);
    delete h;
}

MCE_EXPORT int mce_init(int device, void** handle)
{
    if (!handle) return mcc::fail(g_err, MCR_EINVAL, "mce_init: NULL handle pointer");
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
        mcc::fail(g_err, MCR_EHIP, "mce_init: %s", hipGetErrorString(e));
        mce_free(h);
        return MCR_EHIP;
    }
    h->limit = h->ctx->ws_limit;
    *handle = h;
    return MCR_OK;
}

MCE_EXPORT const char* mce_last_error(void* handle) { return mcc::last_error((Handle*)handle); }

MCE_EXPORT int mce_set_workspace_limit(void* handle, size_t bytes) { return mcc::set_workspace_limit((Handle*)handle, bytes); }

MCE_EXPORT int mce_plan(void* handle, int dtype, int64_t C, int64_t n, int64_t P, int64_t stride_c, int64_t stride_n, int64_t stride_p,
                        int K, int64_t* params_per_chunk)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (!params_per_chunk) return mcc::fail(h->err, MCR_EINVAL, "a NULL result pointer");
    if (const int rc = check_call(h->err, h, dtype, C, n, P, stride_c, stride_n, stride_p, K)) return rc;
    const Call c{h, dtype, C, n, P, stride_c, stride_n, stride_p, K, 0};
    Chunk ch{c};
    i64 pcmax = 0;
    if (const int rc = plan(h, ch, pcmax)) return rc;
    *params_per_chunk = pcmax;
    return MCR_OK;
}

MCE_EXPORT int mce_null_plan(void* handle, int64_t C, int64_t n, int K, int64_t S, int64_t* sims_per_chunk)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (!sims_per_chunk) return mcc::fail(h->err, MCR_EINVAL, "a NULL result pointer");
    if (S < 1) return mcc::fail(h->err, MCR_EINVAL, "S must be >= 1");
    if (const int rc = check_shape(h->err, C, n, K)) return rc;
    const Call c{nullptr, MCR_F64, C, n, S, n, 1, C * n, K, 0};
    Chunk ch{c};
    i64 pcmax = 0;
    if (const int rc = plan(h, ch, pcmax)) return rc;
    *sims_per_chunk = pcmax;
    return MCR_OK;
}

MCE_EXPORT int mce_rank_ecdf_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t n, int64_t P, int64_t stride_c,
                                 int64_t stride_n, int64_t stride_p, int K, MCE_OUTS_PARAMS)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_call(h->err, draws_dev, dtype, C, n, P, stride_c, stride_n, stride_p, K)) return rc;
    return run_dev(h, Call{draws_dev, dtype, C, n, P, stride_c, stride_n, stride_p, K, 0}, MCE_OUTS, false);
}

MCE_EXPORT int mce_rank_ecdf(void* handle, const void* draws, int dtype, int64_t C, int64_t n, int64_t P, int64_t stride_c,
                             int64_t stride_n, int64_t stride_p, int K, MCE_OUTS_PARAMS)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_call(h->err, draws, dtype, C, n, P, stride_c, stride_n, stride_p, K)) return rc;
    return run_dev(h, Call{draws, dtype, C, n, P, stride_c, stride_n, stride_p, K, 0}, MCE_OUTS, true);
}

MCE_EXPORT int mce_null_sample(void* handle, int64_t C, int64_t n, int K, int64_t S, uint64_t seed, double* g0)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (!g0) return mcc::fail(h->err, MCR_EINVAL, "a NULL result pointer");
    if (S < 1) return mcc::fail(h->err, MCR_EINVAL, "S must be >= 1");
    if (const int rc = check_shape(h->err, C, n, K)) return rc;
    Outs o{};
    o.g = g0;
    return run_dev(h, Call{nullptr, MCR_F64, C, n, S, n, 1, C * n, K, (u64)seed}, o, false);
}

MCE_EXPORT int mce_table_host(int64_t M, int64_t n, int K, double* table)
{
    if (!table) return mcc::fail(g_err, MCR_EINVAL, "a NULL result pointer");
    if (n < 1 || n > M || M >= (i64)INT32_MAX) return mcc::fail(g_err, MCR_EINVAL, "the table needs 1 <= n <= M < 2^31 - 1");
    if (K < 2 || K > MCE_MAX_POINTS || K > M)
        return mcc::fail(g_err, MCR_EINVAL, "K = %d: the points must be in [2, min(M, MCE_MAX_POINTS = %d)]", K, MCE_MAX_POINTS);
    table_host(M, n, K, table);
    return MCR_OK;
}

MCE_EXPORT int mce_rank_ecdf_host(const double* chains, int64_t C, int64_t n, int K, const double* table, MCE_OUTS_PARAMS)
{
    if (const int rc = check_call(g_err, chains, MCR_F64, C, n, 1, n, 1, 0, K)) return rc;
    for (i64 i = 0; i < C * n; ++i)
        if (!std::isfinite(chains[i])) return mcc::fail(g_err, MCR_ENONFINITE, "draws contain non-finite value(s)");
    std::vector<double> own;
    if (!table) {
        own.resize((size_t)(K - 1) * (size_t)(n + 1));
        table_host(C * n, n, K, own.data());
        table = own.data();
    }
    HostWork hw;
    host_param(chains, C, n, K, table, MCE_OUTS, hw);
    return MCR_OK;
}

MCE_EXPORT int mce_null_sample_host(int64_t C, int64_t n, int K, int64_t S, uint64_t seed, double* g0)
{
    if (!g0) return mcc::fail(g_err, MCR_EINVAL, "a NULL result pointer");
    if (S < 1) return mcc::fail(g_err, MCR_EINVAL, "S must be >= 1");
    if (const int rc = check_shape(g_err, C, n, K)) return rc;
    const i64 M = C * n;
    std::vector<double> table((size_t)(K - 1) * (size_t)(n + 1)), y((size_t)M);
    table_host(M, n, K, table.data());
    HostWork hw;
    Outs o{};
    for (i64 s = 0; s < S; ++s) {
        const u64 base = (u64)seed * 0x9E3779B97F4A7C15ull + (u64)s * (u64)M;
        for (i64 j = 0; j < M; ++j) y[(size_t)j] = null_draw(base + (u64)j);
        o.g = g0 + s;
        host_param(y.data(), C, n, K, table.data(), o, hw);
    }
    return MCR_OK;
}

MCE_EXPORT int mce_profile_enable(void* handle, int on) { return mcc::profile_enable((Handle*)handle, on); }

MCE_EXPORT int mce_kernel_ms(void* handle, double* ms, int cap) { return mcc::kernel_ms((Handle*)handle, "mce", "MCE", ms, cap); }

}  // extern "C"
