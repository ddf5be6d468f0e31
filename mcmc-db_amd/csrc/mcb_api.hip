// mcb_api.hip -- the entries of include/mcmcref_bm.h: the handle (that of mcc_handle.hpp: a stream, two cached device
// allocations that only grow), the chunked batch-means call, the element-wise steps and the definitions on the host.  The
// library stands alone: nothing of libmcmcref_hip.so's or libmcmcref_iess.so's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mcb_kernels.hpp"
#include "mcc_handle.hpp"

namespace mcb {

using Handle = mcc::Handle<MCB_KERNELS>;     // ws: one chunk's batch sums; the pool's live indices and scales.  up: the
                                             // host entry's copy of the tensor, and its outputs
using mcc::align_up;
using mcc::fail;
using mcc::g_err;

// What every entry that takes a tensor refuses, in one place; `err` receives the cause.
static int check_tensor(char* err, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp)
{
    if (!draws) return fail(err, MCR_EINVAL, "a NULL tensor pointer");
    if (dtype != MCR_F64 && dtype != MCR_F32) return fail(err, MCR_EINVAL, "dtype %d is neither MCR_F64 nor MCR_F32", dtype);
    if (C < 1 || N < 1 || P < 1) return fail(err, MCR_EINVAL, "C, N and P must be >= 1");
    if (sc < 0 || sn < 0 || sp < 0) return fail(err, MCR_EINVAL, "negative strides are not supported");
    int64_t cn = 0, cnp = 0;
    if (__builtin_mul_overflow(C, N, &cn) || __builtin_mul_overflow(cn, P, &cnp) || cnp > ((int64_t)1 << 56))
        return fail(err, MCR_EINVAL, "C * N * P must not exceed 2^56");
    return MCR_OK;
}

static int check_means(char* err, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                       int64_t b, const double* bm, int64_t ld, const double* mu)
{
    if (const int rc = check_tensor(err, draws, dtype, C, N, P, sc, sn, sp)) return rc;
    if (!bm && !mu) return fail(err, MCR_EINVAL, "both output pointers are NULL");
    if (b < 1 || b > N) return fail(err, MCR_EINVAL, "batch size b = %lld is outside [1, N = %lld]", (long long)b, (long long)N);
    const int64_t A = C * (N / b);
    if (bm && ld < A) return fail(err, MCR_EINVAL, "ld = %lld is smaller than A = %lld batch means", (long long)ld, (long long)A);
    return MCR_OK;
}

static int check_finish(char* err, const double* cb, const double* cb3, int64_t P, int64_t b, int64_t A, int64_t A3, int r,
                        const double* sigma)
{
    if (r != 1 && r != 3) return fail(err, MCR_EINVAL, "r = %d is neither 1 nor 3", r);
    if (!cb || !sigma || (r == 3 && !cb3)) return fail(err, MCR_EINVAL, "a NULL matrix pointer");
    if (P < 1) return fail(err, MCR_EINVAL, "P must be >= 1");
    if (b < 1 || A < 1) return fail(err, MCR_EINVAL, "b and A must be >= 1");
    if (r == 3 && b % 3 != 0) return fail(err, MCR_EINVAL, "r = 3 needs a batch size divisible by 3; b = %lld", (long long)b);
    if (r == 3 && A3 < 1) return fail(err, MCR_EINVAL, "A3 must be >= 1");
    return MCR_OK;
}

// The pool's refusals; fills idx and s with the live parameters and their scales.
static int check_pool(char* err, const double* sr, const double* mur, int64_t Mr, const double* sa, const double* mua, int64_t Ma,
                      int64_t P, const double* scale, double jitter, const double* v, const double* d, const double* z,
                      const int64_t* p_live, std::vector<int64_t>* idx, std::vector<double>* s)
{
    if (!sr || !mur || !v || !d || !z || !p_live) return fail(err, MCR_EINVAL, "a NULL pointer");
    if ((sa == nullptr) != (mua == nullptr)) return fail(err, MCR_EINVAL, "a NULL pointer: one of the actual sample's pair");
    if (P < 1) return fail(err, MCR_EINVAL, "P must be >= 1");
    if (Mr < 1 || (sa && Ma < 1)) return fail(err, MCR_EINVAL, "M_ref and M_act must be >= 1");
    if (!(std::isfinite(jitter) && jitter >= 0.0)) return fail(err, MCR_EINVAL, "jitter must be finite and >= 0");
    for (int64_t p = 0; p < P; ++p) {
        const double sp = scale ? scale[p] : 1.0;
        if (!(std::isfinite(sp) && sp >= 0.0)) return fail(err, MCR_EINVAL, "scale %lld must be finite and >= 0", (long long)p);
        if (sp > 0.0) {
            idx->push_back(p);
            s->push_back(sp);
        }
    }
    return MCR_OK;
}

struct Plan {
    int64_t a = 0, A = 0;
    bool time = false;
    int64_t G = 0, segs = 0;            // batches of one wave, waves per (parameter, chain)
    int64_t chunk = 0;
};

static int make_plan(Handle* h, int64_t C, int64_t N, int64_t P, int64_t sn, int64_t b, bool sums, Plan* pl)
{
    pl->a = N / b;
    pl->A = C * pl->a;
    pl->time = sn == 1;
    if (pl->time) {
        const int64_t g = 2 * MCB_BLOCK / b > 1 ? 2 * MCB_BLOCK / b : 1;
        pl->G = b <= kSmall ? (g + kRows - 1) / kRows * kRows : g;
    } else {
        pl->G = 2 * kTile / b > 1 ? 2 * kTile / b : 1;
    }
    pl->segs = (pl->a + pl->G - 1) / pl->G;
    const size_t per = sums ? (size_t)pl->A * 8 : 0;
    const int64_t lo = mcc::most_that_fit(P, [&](int64_t pc) { return align_up((size_t)pc * per, 256) <= h->limit; });
    if (!lo) return fail(h->err, MCR_ENOMEM, "one parameter needs %zu bytes of workspace, the limit is %zu", align_up(per, 256), h->limit);
    const int64_t waves = C * pl->segs;                        // per parameter: no grid of a chunk reaches 2^31
    const int64_t grid_cap = ((int64_t)INT32_MAX - kTile) / waves;
    if (grid_cap < 1) return fail(h->err, MCR_EINVAL, "%lld batches are too many for one launch", (long long)pl->A);
    pl->chunk = lo < grid_cap ? lo : grid_cap;
    return MCR_OK;
}

template <class T>
static void launch_route(Handle* h, const Plan& pl, const T* x, int64_t C, int64_t N, int64_t Pc, int64_t sc, int64_t sn, int64_t sp,
                         int64_t b, double* sums, double* bm, int64_t ld)
{
    if (pl.time) {
        const int64_t wgs = (Pc * C * pl.segs + kWaves - 1) / kWaves;
        hipLaunchKernelGGL(k_bm_time<T>, dim3((unsigned)wgs), dim3(kThreads), 0, h->stream, x, C, N, Pc, sc, sp, b, pl.a, pl.G, pl.segs,
                           sums, bm, ld);
    } else {
        const int64_t ptiles = (Pc + kTile - 1) / kTile;
        hipLaunchKernelGGL(k_bm_tile<T>, dim3((unsigned)(ptiles * pl.segs * C)), dim3(kTile), 0, h->stream, x, C, N, Pc, sc, sn, sp, b,
                           pl.a, pl.G, pl.segs, ptiles, sums, bm, ld);
    }
}

template <class T>
static void launch_mean(Handle* h, const Plan& pl, const T* x, int64_t N, int64_t Pc, int64_t sn, int64_t sp, int64_t b,
                        const double* sums, double* mu)
{
    hipLaunchKernelGGL(k_bm_mean<T>, dim3((unsigned)((Pc + kWaves - 1) / kWaves)), dim3(kThreads), 0, h->stream, x, N, Pc, sn, sp, b,
                       pl.a, pl.A, sums, mu);
}

static int run_means(Handle* h, const void* x_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                     int64_t b, double* bm_dev, int64_t ld, double* mu_dev)
{
    Plan pl;
    if (const int rc = make_plan(h, C, N, P, sn, b, mu_dev != nullptr, &pl)) return rc;
    MCC_HIP(h, hipSetDevice(h->device));
    if (mu_dev)
        if (const int rc = mcc::ensure(h, &h->ws, &h->ws_bytes, align_up((size_t)pl.chunk * (size_t)pl.A * 8, 256), "for the batch sums")) return rc;
    h->timer.clear();
    const size_t es = dtype == MCR_F64 ? 8 : 4;
    const int route = pl.time ? MCB_KERNEL_TIME : MCB_KERNEL_TILE;
    for (int64_t p0 = 0; p0 < P; p0 += pl.chunk) {
        const int64_t Pc = P - p0 < pl.chunk ? P - p0 : pl.chunk;
        const char* x = (const char*)x_dev + (size_t)p0 * (size_t)sp * es;
        double* sums = mu_dev ? (double*)h->ws : nullptr;
        double* bm = bm_dev ? bm_dev + p0 * ld : nullptr;
        MCC_HIP(h, h->timer.begin(h->stream));
        if (dtype == MCR_F64) launch_route(h, pl, (const double*)x, C, N, Pc, sc, sn, sp, b, sums, bm, ld);
        else launch_route(h, pl, (const float*)x, C, N, Pc, sc, sn, sp, b, sums, bm, ld);
        MCC_HIP(h, hipGetLastError());
        MCC_HIP(h, h->timer.mark(h->stream, route));
        if (mu_dev) {
            if (dtype == MCR_F64) launch_mean(h, pl, (const double*)x, N, Pc, sn, sp, b, sums, mu_dev + p0);
            else launch_mean(h, pl, (const float*)x, N, Pc, sn, sp, b, sums, mu_dev + p0);
            MCC_HIP(h, hipGetLastError());
            MCC_HIP(h, h->timer.mark(h->stream, MCB_KERNEL_MEAN));
        }
        MCC_HIP(h, hipStreamSynchronize(h->stream));             // the next chunk writes the same workspace
        MCC_HIP(h, h->timer.collect());
    }
    return MCR_OK;
}

// One kernel on the handle's stream, timed when profiling is on; synchronous.
template <class Launch>
static int run_one(Handle* h, int kernel, Launch&& launch)
{
    h->timer.clear();
    MCC_HIP(h, h->timer.begin(h->stream));
    launch();
    MCC_HIP(h, hipGetLastError());
    MCC_HIP(h, h->timer.mark(h->stream, kernel));
    MCC_HIP(h, hipStreamSynchronize(h->stream));
    MCC_HIP(h, h->timer.collect());
    return MCR_OK;
}

static unsigned flat_grid(int64_t n)
{
    const int64_t g = (n + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}

template <class T>
static void host_means(const T* x, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp, int64_t b, double* bm,
                       int64_t ld, double* mu)
{
    const int64_t a = N / b, A = C * a, n0 = N - a * b;
    std::vector<double> sums((size_t)A);
    for (int64_t p = 0; p < P; ++p) {
        const double pivot = (double)x[n0 * sn + p * sp];
        for (int64_t c = 0; c < C; ++c)
            for (int64_t k = 0; k < a; ++k) {
                const T* at = x + c * sc + (n0 + k * b) * sn + p * sp;
                const double s = tree_sum(b, [&](int64_t i) { return leaf(at[i * sn], pivot); });
                sums[(size_t)(c * a + k)] = s;
                if (bm) bm[p * ld + c * a + k] = mean_of(pivot, s, b);
            }
        if (mu) mu[p] = mean_of(pivot, tree_sum(A, [&](int64_t i) { return sums[(size_t)i]; }), A * b);
    }
}

}  // namespace mcb

using namespace mcb;

extern "C" {

int mcb_version(void) { return MCB_VERSION; }

int mcb_init(int device, void** handle)
{
    return mcc::open<Handle>(device, handle, "mcb_init", [] { return hipSuccess; });
}

void mcb_free(void* handle) { mcc::close((Handle*)handle); }

const char* mcb_last_error(void* handle) { return mcc::last_error((Handle*)handle); }

int mcb_set_workspace_limit(void* handle, size_t bytes) { return mcc::set_workspace_limit((Handle*)handle, bytes); }

int mcb_batch_size(int64_t N, int r, int64_t* b, int64_t* a)
{
    if (!b || !a) return fail(g_err, MCR_EINVAL, "a NULL result pointer");
    if (N < 1) return fail(g_err, MCR_EINVAL, "N must be >= 1");
    if (r != 1 && r != 3) return fail(g_err, MCR_EINVAL, "r = %d is neither 1 nor 3", r);
    if (r == 3 && N < 3) return fail(g_err, MCR_EINVAL, "r = 3 needs N >= 3 draws per chain; N = %lld", (long long)N);
    int64_t root = (int64_t)std::sqrt((double)N);                // floor(sqrt(N)), exactly
    while (root * root > N) --root;
    while ((root + 1) * (root + 1) <= N) ++root;
    *b = r == 1 ? root : 3 * (root / 3 > 1 ? root / 3 : 1);
    *a = N / *b;
    return MCR_OK;
}

int mcb_batch_means_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                        int64_t stride_n, int64_t stride_p, int64_t b, double* bm_dev, int64_t ld, double* mu_dev)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_means(h->err, draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p, b, bm_dev, ld, mu_dev)) return rc;
    return run_means(h, draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p, b, bm_dev, ld, mu_dev);
}

int mcb_batch_means(void* handle, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                    int64_t stride_n, int64_t stride_p, int64_t b, double* bm, int64_t ld, double* mu)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_means(h->err, draws, dtype, C, N, P, stride_c, stride_n, stride_p, b, bm, ld, mu)) return rc;
    const size_t bm_bytes = bm ? (size_t)P * (size_t)ld * 8 : 0, mu_bytes = mu ? (size_t)P * 8 : 0;
    char* at = nullptr;                                                     // the outputs, behind the tensor
    if (const int rc = mcc::upload_span(h, draws, dtype, C, N, P, stride_c, stride_n, stride_p, align_up(bm_bytes, 256) + mu_bytes, &at))
        return rc;
    double* d_bm = bm ? (double*)at : nullptr;
    double* d_mu = mu ? (double*)(at + align_up(bm_bytes, 256)) : nullptr;
    if (bm && ld > C * (N / b)) MCC_HIP(h, hipMemcpy(d_bm, bm, bm_bytes, hipMemcpyHostToDevice));   // the padding comes back as it was
    if (const int rc = run_means(h, h->up, dtype, C, N, P, stride_c, stride_n, stride_p, b, d_bm, ld, d_mu)) return rc;
    if (bm) MCC_HIP(h, hipMemcpy(bm, d_bm, bm_bytes, hipMemcpyDeviceToHost));
    if (mu) MCC_HIP(h, hipMemcpy(mu, d_mu, mu_bytes, hipMemcpyDeviceToHost));
    return MCR_OK;
}

int mcb_batch_means_host(const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c, int64_t stride_n,
                         int64_t stride_p, int64_t b, double* bm, int64_t ld, double* mu)
{
    if (const int rc = check_means(g_err, draws, dtype, C, N, P, stride_c, stride_n, stride_p, b, bm, ld, mu)) return rc;
    if (dtype == MCR_F64) host_means((const double*)draws, C, N, P, stride_c, stride_n, stride_p, b, bm, ld, mu);
    else host_means((const float*)draws, C, N, P, stride_c, stride_n, stride_p, b, bm, ld, mu);
    return MCR_OK;
}

int mcb_pooled_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                   int64_t stride_n, int64_t stride_p, double* pooled_dev, int64_t ld)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_tensor(h->err, draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p)) return rc;
    if (!pooled_dev) return fail(h->err, MCR_EINVAL, "a NULL output pointer");
    if (ld < C * N) return fail(h->err, MCR_EINVAL, "ld = %lld is smaller than C * N = %lld draws", (long long)ld, (long long)(C * N));
    MCC_HIP(h, hipSetDevice(h->device));
    return run_one(h, MCB_KERNEL_POOLED, [&] {
        if (dtype == MCR_F64)
            hipLaunchKernelGGL(k_bm_pooled<double>, dim3(flat_grid(C * N * P)), dim3(kThreads), 0, h->stream, (const double*)draws_dev, C,
                               N, P, stride_c, stride_n, stride_p, pooled_dev, ld);
        else
            hipLaunchKernelGGL(k_bm_pooled<float>, dim3(flat_grid(C * N * P)), dim3(kThreads), 0, h->stream, (const float*)draws_dev, C, N,
                               P, stride_c, stride_n, stride_p, pooled_dev, ld);
    });
}

int mcb_lrv_finish_dev(void* handle, const double* cb_dev, const double* cb3_dev, int64_t P, int64_t b, int64_t A, int64_t A3,
                       int r, double* sigma_dev)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_finish(h->err, cb_dev, cb3_dev, P, b, A, A3, r, sigma_dev)) return rc;
    const double f = lrv_factor(b, A), f3 = r == 3 ? lrv_factor(b / 3, A3) : 0.0;
    MCC_HIP(h, hipSetDevice(h->device));
    return run_one(h, MCB_KERNEL_FINISH, [&] {
        hipLaunchKernelGGL(k_bm_finish, dim3(flat_grid(P * P)), dim3(kThreads), 0, h->stream, cb_dev, cb3_dev, P * P, f, f3, r, A,
                           sigma_dev);
    });
}

int mcb_lrv_finish_host(const double* cb, const double* cb3, int64_t P, int64_t b, int64_t A, int64_t A3, int r, double* sigma)
{
    if (const int rc = check_finish(g_err, cb, cb3, P, b, A, A3, r, sigma)) return rc;
    const double f = lrv_factor(b, A), f3 = r == 3 ? lrv_factor(b / 3, A3) : 0.0;
    for (int64_t i = 0; i < P * P; ++i) sigma[i] = finish_entry(cb[i], r == 3 ? cb3[i] : 0.0, f, f3, r, A);
    return MCR_OK;
}

int mcb_pool_dev(void* handle, const double* sig_ref_dev, const double* mu_ref_dev, int64_t M_ref, const double* sig_act_dev,
                 const double* mu_act_dev, int64_t M_act, int64_t P, const double* scale, double jitter, double* v_dev,
                 double* d_dev, double* z_dev, int64_t* p_live)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    std::vector<int64_t> idx;
    std::vector<double> s;
    if (const int rc = check_pool(h->err, sig_ref_dev, mu_ref_dev, M_ref, sig_act_dev, mu_act_dev, M_act, P, scale, jitter, v_dev, d_dev,
                                  z_dev, p_live, &idx, &s))
        return rc;
    const int64_t PL = (int64_t)idx.size();
    *p_live = PL;
    h->timer.clear();
    if (PL == 0) return MCR_OK;
    MCC_HIP(h, hipSetDevice(h->device));
    const size_t half = align_up((size_t)PL * 8, 256);
    if (const int rc = mcc::ensure(h, &h->ws, &h->ws_bytes, 2 * half, "for the live parameters")) return rc;
    int64_t* d_idx = (int64_t*)h->ws;
    double* d_s = (double*)((char*)h->ws + half);
    MCC_HIP(h, hipMemcpyAsync(d_idx, idx.data(), (size_t)PL * 8, hipMemcpyHostToDevice, h->stream));
    MCC_HIP(h, hipMemcpyAsync(d_s, s.data(), (size_t)PL * 8, hipMemcpyHostToDevice, h->stream));
    return run_one(h, MCB_KERNEL_POOL, [&] {
        hipLaunchKernelGGL(k_bm_pool, dim3(flat_grid(PL * PL)), dim3(kThreads), 0, h->stream, sig_ref_dev, mu_ref_dev, (double)M_ref,
                           sig_act_dev, mu_act_dev, (double)M_act, P, PL, d_idx, d_s, jitter, v_dev, d_dev, z_dev);
    });
}

int mcb_pool_host(const double* sig_ref, const double* mu_ref, int64_t M_ref, const double* sig_act, const double* mu_act,
                  int64_t M_act, int64_t P, const double* scale, double jitter, double* v, double* d, double* z, int64_t* p_live)
{
    std::vector<int64_t> idx;
    std::vector<double> s;
    if (const int rc = check_pool(g_err, sig_ref, mu_ref, M_ref, sig_act, mu_act, M_act, P, scale, jitter, v, d, z, p_live, &idx, &s))
        return rc;
    const int64_t PL = (int64_t)idx.size();
    *p_live = PL;
    const bool two = sig_act != nullptr;
    const double mr = (double)M_ref, ma = (double)M_act;
    for (int64_t i = 0; i < PL; ++i) {
        for (int64_t j = 0; j < PL; ++j) {
            const int64_t e = idx[(size_t)i] * P + idx[(size_t)j];
            v[i * PL + j] = pool_entry(s[(size_t)i], s[(size_t)j], sig_ref[e], mr, two ? sig_act[e] : 0.0, ma, two, i == j, jitter);
        }
        const int64_t q = idx[(size_t)i];
        d[i] = pool_shift(s[(size_t)i], mu_ref[q], two ? mu_act[q] : 0.0, two);
        z[i] = pool_z(d[i], v[i * PL + i]);
    }
    return MCR_OK;
}

int mcb_tree_sum_host(const double* y, int64_t n, int squares, double* sum)
{
    if (!sum || (!y && n > 0)) return fail(g_err, MCR_EINVAL, "a NULL pointer");
    if (n < 0) return fail(g_err, MCR_EINVAL, "n must be >= 0");
    *sum = tree_sum(n, [&](int64_t i) {
#pragma clang fp contract(off)
        const double sq = y[i] * y[i];
        return squares ? sq : y[i];
    });
    return MCR_OK;
}

int mcb_profile_enable(void* handle, int on) { return mcc::profile_enable((Handle*)handle, on); }

int mcb_kernel_ms(void* handle, double* ms, int cap) { return mcc::kernel_ms((Handle*)handle, "mcb", "MCB", ms, cap); }

}  // extern "C"
