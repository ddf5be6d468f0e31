// mci_api.hip -- the entries of include/mcmcref_iess.h: the handle (a stream, two cached device allocations that only
// grow), the chunked call, and the definition on the host.  The library stands alone: nothing of libmcmcref_hip.so's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mci_kernels.hpp"

namespace mci {

struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    void* ws = nullptr;                 // one chunk's thresholds, outputs, words and popcounts
    size_t ws_bytes = 0;
    void* up = nullptr;                 // the host entry's copy of the tensor
    size_t up_bytes = 0;
    size_t limit = (size_t)1 << 30;
    bool profile = false;
    double ms[MCI_KERNELS] = {0.0, 0.0};
    char err[256] = "";
};

static thread_local char g_init_err[256] = "";

static int fail(char* err, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(err, 256, fmt, ap);
    va_end(ap);
    return code;
}

#define MCI_HIP(h, call)                                                                                       \
    do {                                                                                                       \
        const hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return fail((h)->err, MCR_EHIP, "%s: %s", #call, hipGetErrorString(e_));         \
    } while (0)

static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// What every entry refuses, in one place; `err` receives the cause.
static int check_dims(char* err, int dtype, int64_t C, int64_t N, int64_t P, int K)
{
    if (dtype != MCR_F64 && dtype != MCR_F32) return fail(err, MCR_EINVAL, "dtype %d is neither MCR_F64 nor MCR_F32", dtype);
    if (C < 1 || N < 1 || P < 1) return fail(err, MCR_EINVAL, "C, N and P must be >= 1");
    if (N > MCI_MAX_DRAWS) return fail(err, MCR_EINVAL, "N = %lld exceeds MCI_MAX_DRAWS = %d draws per chain", (long long)N, MCI_MAX_DRAWS);
    if (C >= INT32_MAX || C * N >= (int64_t)INT32_MAX) return fail(err, MCR_EINVAL, "C * N must be below 2^31 - 1");
    if (K < 1 || K > MCI_MAX_REQUESTS) return fail(err, MCR_EINVAL, "K = %d requests: 1 <= K <= MCI_MAX_REQUESTS = %d", K, MCI_MAX_REQUESTS);
    return MCR_OK;
}

static int check_call(char* err, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                      int64_t sp, const double* lower, const double* upper, int K)
{
    if (!draws || !lower || !upper) return fail(err, MCR_EINVAL, "a NULL tensor or threshold pointer");
    if (const int rc = check_dims(err, dtype, C, N, P, K)) return rc;
    if (sc < 0 || sn < 0 || sp < 0) return fail(err, MCR_EINVAL, "negative strides are not supported");
    for (int64_t i = 0; i < P * K; ++i)
        if (std::isnan(lower[i]) || std::isnan(upper[i]))
            return fail(err, MCR_EINVAL, "threshold %lld of parameter %lld is NaN", (long long)(i % K), (long long)(i / K));
    return MCR_OK;
}

struct Plan {
    int64_t Wp = 0, words = 0;          // words of one chain (with the zero word), of one (parameter, request)
    bool lds = false;
    int64_t chunk = 0;
};

static size_t chunk_bytes(const Plan& pl, int64_t Pc, int K)
{
    const size_t pk = (size_t)Pc * (size_t)K;
    return 2 * align_up(pk * 8) + 3 * align_up(pk * 8) + align_up(pk * (size_t)pl.words * 8) +
           (pl.lds ? 0 : align_up(pk * (size_t)pl.words * 4));
}

static int make_plan(Handle* h, int64_t C, int64_t N, int64_t P, int K, Plan* pl)
{
    pl->Wp = (N + 63) / 64 + 1;
    pl->words = C * pl->Wp;
    pl->lds = pl->words <= MCI_LDS_WORDS;
    if (chunk_bytes(*pl, 1, K) > h->limit)
        return fail(h->err, MCR_ENOMEM, "one parameter needs %zu bytes of workspace, the limit is %zu", chunk_bytes(*pl, 1, K), h->limit);
    int64_t lo = 1, hi = P;                                   // the most parameters under the limit
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (chunk_bytes(*pl, mid, K) <= h->limit) lo = mid;
        else hi = mid - 1;
    }
    // no grid of a chunk reaches 2^31: k_pack_* launch at most `words` workgroups per parameter, k_lag K
    const int64_t grid_cap = ((int64_t)INT32_MAX - 1) / (pl->words > K ? pl->words : K);
    if (grid_cap < 1) return fail(h->err, MCR_EINVAL, "%lld chains are too many for one launch", (long long)C);
    pl->chunk = lo < grid_cap ? lo : grid_cap;
    return MCR_OK;
}

template <class T>
static void launch_pack(Handle* h, const Plan& pl, const T* x, int64_t C, int64_t N, int64_t Pc, int64_t sc, int64_t sn, int64_t sp,
                        const double* lo, const double* hi, int K, uint64_t* bits)
{
    if (sn == 1) {
        const int64_t segments = (pl.Wp + kWaves * kPackWords - 1) / (kWaves * kPackWords);
        hipLaunchKernelGGL(k_pack_time<T>, dim3((unsigned)(Pc * C * segments)), dim3(kThreads), 0, h->stream, x, C, N, sc, sp, lo, hi,
                           K, pl.Wp, segments, bits);
    } else {
        const int64_t ptiles = (Pc + kTile - 1) / kTile;
        hipLaunchKernelGGL(k_pack_tile<T>, dim3((unsigned)(ptiles * pl.Wp * C)), dim3(kThreads), 0, h->stream, x, C, N, Pc, sc, sn,
                           sp, lo, hi, K, pl.Wp, ptiles, bits);
    }
}

static int run_dev(Handle* h, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                   const double* lower, const double* upper, int K, double* ess, int64_t* trunc, int64_t* ones)
{
    Plan pl;
    if (const int rc = make_plan(h, C, N, P, K, &pl)) return rc;
    MCI_HIP(h, hipSetDevice(h->device));
    const size_t need = chunk_bytes(pl, pl.chunk, K);
    if (need > h->ws_bytes) {
        if (h->ws) MCI_HIP(h, hipFree(h->ws));
        h->ws = nullptr;
        h->ws_bytes = 0;
        if (hipMalloc(&h->ws, need) != hipSuccess) {
            h->ws = nullptr;
            (void)hipGetLastError();
            return fail(h->err, MCR_ENOMEM, "cannot allocate %zu bytes of device workspace", need);
        }
        h->ws_bytes = need;
    }
    h->ms[0] = h->ms[1] = 0.0;
    const size_t es = dtype == MCR_F64 ? 8 : 4;
    for (int64_t p0 = 0; p0 < P; p0 += pl.chunk) {
        const int64_t Pc = P - p0 < pl.chunk ? P - p0 : pl.chunk;
        const size_t pk = (size_t)Pc * (size_t)K;
        char* at = (char*)h->ws;
        double* d_lo = (double*)at;       at += align_up(pk * 8);
        double* d_hi = (double*)at;       at += align_up(pk * 8);
        double* d_ess = (double*)at;      at += align_up(pk * 8);
        int64_t* d_trunc = (int64_t*)at;  at += align_up(pk * 8);
        int64_t* d_ones = (int64_t*)at;   at += align_up(pk * 8);
        uint64_t* d_bits = (uint64_t*)at; at += align_up(pk * (size_t)pl.words * 8);
        uint32_t* d_pre = pl.lds ? nullptr : (uint32_t*)at;
        MCI_HIP(h, hipMemcpyAsync(d_lo, lower + p0 * K, pk * 8, hipMemcpyHostToDevice, h->stream));
        MCI_HIP(h, hipMemcpyAsync(d_hi, upper + p0 * K, pk * 8, hipMemcpyHostToDevice, h->stream));
        const char* x = (const char*)draws_dev + (size_t)p0 * (size_t)sp * es;
        if (h->profile) MCI_HIP(h, hipEventRecord(h->ev[0], h->stream));
        if (dtype == MCR_F64) launch_pack(h, pl, (const double*)x, C, N, Pc, sc, sn, sp, d_lo, d_hi, K, d_bits);
        else launch_pack(h, pl, (const float*)x, C, N, Pc, sc, sn, sp, d_lo, d_hi, K, d_bits);
        MCI_HIP(h, hipGetLastError());
        if (h->profile) MCI_HIP(h, hipEventRecord(h->ev[1], h->stream));
        if (pl.lds) hipLaunchKernelGGL(k_lag<true>, dim3((unsigned)pk), dim3(kThreads), lds_bytes(pl.words), h->stream, d_bits, d_pre, C, N, pl.Wp, d_ess, d_trunc, d_ones);
        else hipLaunchKernelGGL(k_lag<false>, dim3((unsigned)pk), dim3(kThreads), 0, h->stream, d_bits, d_pre, C, N, pl.Wp, d_ess, d_trunc, d_ones);
        MCI_HIP(h, hipGetLastError());
        if (h->profile) MCI_HIP(h, hipEventRecord(h->ev[2], h->stream));
        if (ess) MCI_HIP(h, hipMemcpyAsync(ess + p0 * K, d_ess, pk * 8, hipMemcpyDeviceToHost, h->stream));
        if (trunc) MCI_HIP(h, hipMemcpyAsync(trunc + p0 * K, d_trunc, pk * 8, hipMemcpyDeviceToHost, h->stream));
        if (ones) MCI_HIP(h, hipMemcpyAsync(ones + p0 * K, d_ones, pk * 8, hipMemcpyDeviceToHost, h->stream));
        MCI_HIP(h, hipStreamSynchronize(h->stream));
        if (h->profile) {
            float a = 0.f, b = 0.f;
            MCI_HIP(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
            MCI_HIP(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
            h->ms[MCI_KERNEL_PACK] += a;
            h->ms[MCI_KERNEL_LAG] += b;
        }
    }
    return MCR_OK;
}

// The definition, for one request on the packed words of C chains (Wp words each, as the pack kernels write them).
static void host_request(const uint64_t* B, int64_t C, int64_t N, int64_t Wp, double* ess, int64_t* trunc, int64_t* ones)
{
    const int64_t W = Wp - 1, n = N, m = C;
    std::vector<uint32_t> pre((size_t)(C * Wp));
    uint32_t run = 0;
    for (int64_t i = 0; i < C * Wp; ++i) {
        pre[(size_t)i] = run;
        run += (uint32_t)__builtin_popcountll(B[i]);
    }
    int64_t ksum = 0, wnum = 0, k2 = 0;
    for (int64_t c = 0; c < C; ++c) {
        const int64_t k = (int64_t)(pre[(size_t)(c * Wp + W)] - pre[(size_t)(c * Wp)]);
        ksum += k;
        wnum += k * (n - k);
        k2 += k * k;
    }
    if (ones) *ones = ksum;
    double out_ess;
    int64_t out_trunc;
    const double vh = n >= 2 ? var_hat(wnum, m * k2 - ksum * ksum, n, m) : 0.0;
    if (n < 2) {
        out_ess = (double)NAN;
        out_trunc = -1;
    } else if (vh == 0.0) {
        out_ess = (double)m * (double)n;
        out_trunc = 0;
    } else {
        double R = 0.0, t[MCI_LAG_BLOCK];
        out_trunc = n;
        for (int64_t base = 1; base <= n - 1 && out_trunc == n; base += MCI_LAG_BLOCK) {
            for (int i = 0; i < MCI_LAG_BLOCK; ++i) t[i] = 0.0;
            for (int i = 0; i < MCI_LAG_BLOCK && base + i <= n - 1; ++i) {
                const int64_t lag = base + i, qw = lag >> 6, jh = n - lag;
                const int r = (int)(lag & 63);
                Wide A{0, 0};
                for (int64_t c = 0; c < C; ++c) {
                    const uint64_t* Bc = B + c * Wp;
                    const uint32_t* pc = pre.data() + c * Wp;
                    int64_t S = 0;
                    for (int64_t w = 0; w + qw < W; ++w) S += __builtin_popcountll(Bc[w] & funnel(Bc[w + qw], Bc[w + qw + 1], r));
                    const uint32_t p0 = pc[0];
                    const int64_t k = (int64_t)(pc[W] - p0);
                    const int64_t H = prefix_ones(pc[jh >> 6] - p0, Bc[jh >> 6], jh);
                    const int64_t T = k - prefix_ones(pc[qw] - p0, Bc[qw], lag);
                    A = wide_add(A, chain_a(n, lag, k, S, H, T));
                }
                if (wide_negative(A)) {
                    out_trunc = lag;
                    break;
                }
                t[i] = rho(A, n, lag, m, vh);
            }
            R = R + block_sum(t, 0, 1, [] {});
        }
        out_ess = ess_of(n, m, R);
    }
    if (ess) *ess = out_ess;
    if (trunc) *trunc = out_trunc;
}

}  // namespace mci

using namespace mci;

extern "C" {

int mci_version(void) { return MCI_VERSION; }

int mci_init(int device, void** handle)
{
    if (!handle) return fail(g_init_err, MCR_EINVAL, "mci_init: NULL handle pointer");
    *handle = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(g_init_err, MCR_ENODEVICE, "no HIP device is usable");
    }
    if (device < 0 || device >= count) return fail(g_init_err, MCR_ENODEVICE, "device %d: %d device(s) are visible", device, count);
    Handle* h = new Handle;
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev[i]);
    if (e == hipSuccess)                                        // beyond the 64 KiB a launch may ask for by default
        e = hipFuncSetAttribute((const void*)k_lag<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(MCI_LDS_WORDS));
    if (e != hipSuccess) {
        fail(g_init_err, MCR_EHIP, "mci_init: %s", hipGetErrorString(e));
        mci_free(h);
        return MCR_EHIP;
    }
    *handle = h;
    return MCR_OK;
}

void mci_free(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ws) (void)hipFree(h->ws);
    if (h->up) (void)hipFree(h->up);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* mci_last_error(void* handle) { return handle ? ((Handle*)handle)->err : g_init_err; }

int mci_set_workspace_limit(void* handle, size_t bytes)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (bytes == 0) return fail(h->err, MCR_EINVAL, "a workspace limit of 0 bytes");
    h->limit = bytes;
    return MCR_OK;
}

int mci_indicator_plan(void* handle, int dtype, int64_t C, int64_t N, int64_t P, int K, int64_t* params_per_chunk)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (!params_per_chunk) return fail(h->err, MCR_EINVAL, "a NULL result pointer");
    if (const int rc = check_dims(h->err, dtype, C, N, P, K)) return rc;
    Plan pl;
    if (const int rc = make_plan(h, C, N, P, K, &pl)) return rc;
    *params_per_chunk = pl.chunk;
    return MCR_OK;
}

int mci_indicator_ess_dev(void* handle, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                          int64_t stride_n, int64_t stride_p, const double* lower, const double* upper, int K, double* ess,
                          int64_t* trunc, int64_t* ones)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_call(h->err, draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p, lower, upper, K)) return rc;
    return run_dev(h, draws_dev, dtype, C, N, P, stride_c, stride_n, stride_p, lower, upper, K, ess, trunc, ones);
}

int mci_indicator_ess(void* handle, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t stride_c,
                      int64_t stride_n, int64_t stride_p, const double* lower, const double* upper, int K, double* ess,
                      int64_t* trunc, int64_t* ones)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (const int rc = check_call(h->err, draws, dtype, C, N, P, stride_c, stride_n, stride_p, lower, upper, K)) return rc;
    const size_t es = dtype == MCR_F64 ? 8 : 4;
    const size_t span = ((size_t)(C - 1) * (size_t)stride_c + (size_t)(N - 1) * (size_t)stride_n + (size_t)(P - 1) * (size_t)stride_p + 1) * es;
    MCI_HIP(h, hipSetDevice(h->device));
    if (span > h->up_bytes) {
        if (h->up) MCI_HIP(h, hipFree(h->up));
        h->up = nullptr;
        h->up_bytes = 0;
        if (hipMalloc(&h->up, span) != hipSuccess) {
            h->up = nullptr;
            (void)hipGetLastError();
            return fail(h->err, MCR_ENOMEM, "cannot allocate %zu bytes for the tensor", span);
        }
        h->up_bytes = span;
    }
    MCI_HIP(h, hipMemcpy(h->up, draws, span, hipMemcpyHostToDevice));      // (complete on return: the kernels may start)
    return run_dev(h, h->up, dtype, C, N, P, stride_c, stride_n, stride_p, lower, upper, K, ess, trunc, ones);
}

int mci_indicator_ess_host(const double* chains, int64_t C, int64_t N, const double* lower, const double* upper, int K,
                           double* ess, int64_t* trunc, int64_t* ones)
{
    if (const int rc = check_call(g_init_err, chains, MCR_F64, C, N, 1, N, 1, 0, lower, upper, K)) return rc;
    const int64_t Wp = (N + 63) / 64 + 1;
    std::vector<uint64_t> B((size_t)(C * Wp));
    for (int k = 0; k < K; ++k) {
        std::fill(B.begin(), B.end(), 0ull);
        for (int64_t c = 0; c < C; ++c)
            for (int64_t t = 0; t < N; ++t) {
                const double v = chains[c * N + t];
                if (lower[k] < v && v <= upper[k]) B[(size_t)(c * Wp + (t >> 6))] |= 1ull << (t & 63);
            }
        host_request(B.data(), C, N, Wp, ess ? ess + k : nullptr, trunc ? trunc + k : nullptr, ones ? ones + k : nullptr);
    }
    return MCR_OK;
}

int mci_profile_enable(void* handle, int on)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    h->profile = on != 0;
    h->ms[0] = h->ms[1] = 0.0;
    return MCR_OK;
}

int mci_kernel_ms(void* handle, double* ms, int cap)
{
    Handle* h = (Handle*)handle;
    if (!h) return MCR_EINVAL;
    if (!ms || cap < MCI_KERNELS) return fail(h->err, MCR_EINVAL, "mci_kernel_ms needs room for MCI_KERNELS = %d times", MCI_KERNELS);
    for (int i = 0; i < MCI_KERNELS; ++i) ms[i] = h->ms[i];
    return MCR_OK;
}

}  // extern "C"
