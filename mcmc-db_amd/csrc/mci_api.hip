// mci_api.hip -- the entries of include/mcmcref_iess.h: the handle (that of mcc_handle.hpp: a stream, two cached device
// allocations that only grow), the chunked call, and the definition on the host.  The library stands alone: nothing of
// libmcmcref_hip.so's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mcc_handle.hpp"
#include "mci_kernels.hpp"

namespace mci {

using Handle = mcc::Handle<MCI_KERNELS>;     // ws: one chunk's thresholds, outputs, words and popcounts
using mcc::Carve;
using mcc::fail;
using mcc::g_err;

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

// The buffers of a chunk of Pc parameters, as they lie in the workspace.
struct Chunk {
    double *lo, *hi, *ess; int64_t *trunc, *ones; uint64_t* bits; uint32_t* pre;
    Chunk(Carve& cv, const Plan& pl, int64_t Pc, int K)
    {
        const size_t pk = (size_t)Pc * (size_t)K;
        lo = cv.take<double>(pk);
        hi = cv.take<double>(pk);
        ess = cv.take<double>(pk);
        trunc = cv.take<int64_t>(pk);
        ones = cv.take<int64_t>(pk);
        bits = cv.take<uint64_t>(pk * (size_t)pl.words);
        pre = pl.lds ? nullptr : cv.take<uint32_t>(pk * (size_t)pl.words);
    }
};

static size_t chunk_bytes(const Plan& pl, int64_t Pc, int K)
{
    Carve m{nullptr};
    Chunk(m, pl, Pc, K);
    return mcc::align_up(m.off, 256);                         // what the limit is held against: the last buffer rounded too
}

static int make_plan(Handle* h, int64_t C, int64_t N, int64_t P, int K, Plan* pl)
{
    pl->Wp = (N + 63) / 64 + 1;
    pl->words = C * pl->Wp;
    pl->lds = pl->words <= MCI_LDS_WORDS;
    const int64_t lo = mcc::most_that_fit(P, [&](int64_t pc) { return chunk_bytes(*pl, pc, K) <= h->limit; });
    if (!lo) return fail(h->err, MCR_ENOMEM, "one parameter needs %zu bytes of workspace, the limit is %zu", chunk_bytes(*pl, 1, K), h->limit);
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
    MCC_HIP(h, hipSetDevice(h->device));
    if (const int rc = mcc::ensure(h, &h->ws, &h->ws_bytes, chunk_bytes(pl, pl.chunk, K), "of device workspace")) return rc;
    h->timer.clear();
    const size_t es = dtype == MCR_F64 ? 8 : 4;
    for (int64_t p0 = 0; p0 < P; p0 += pl.chunk) {
        const int64_t Pc = P - p0 < pl.chunk ? P - p0 : pl.chunk;
        const size_t pk = (size_t)Pc * (size_t)K;
        Carve cv{(char*)h->ws, h->ws_bytes};
        const Chunk d(cv, pl, Pc, K);
        MCC_HIP(h, hipMemcpyAsync(d.lo, lower + p0 * K, pk * 8, hipMemcpyHostToDevice, h->stream));
        MCC_HIP(h, hipMemcpyAsync(d.hi, upper + p0 * K, pk * 8, hipMemcpyHostToDevice, h->stream));
        const char* x = (const char*)draws_dev + (size_t)p0 * (size_t)sp * es;
        MCC_HIP(h, h->timer.begin(h->stream));
        if (dtype == MCR_F64) launch_pack(h, pl, (const double*)x, C, N, Pc, sc, sn, sp, d.lo, d.hi, K, d.bits);
        else launch_pack(h, pl, (const float*)x, C, N, Pc, sc, sn, sp, d.lo, d.hi, K, d.bits);
        MCC_HIP(h, hipGetLastError());
        MCC_HIP(h, h->timer.mark(h->stream, MCI_KERNEL_PACK));
        if (pl.lds) hipLaunchKernelGGL(k_lag<true>, dim3((unsigned)pk), dim3(kThreads), lds_bytes(pl.words), h->stream, d.bits, d.pre, C, N, pl.Wp, d.ess, d.trunc, d.ones);
        else hipLaunchKernelGGL(k_lag<false>, dim3((unsigned)pk), dim3(kThreads), 0, h->stream, d.bits, d.pre, C, N, pl.Wp, d.ess, d.trunc, d.ones);
        MCC_HIP(h, hipGetLastError());
        MCC_HIP(h, h->timer.mark(h->stream, MCI_KERNEL_LAG));
        if (ess) MCC_HIP(h, hipMemcpyAsync(ess + p0 * K, d.ess, pk * 8, hipMemcpyDeviceToHost, h->stream));
        if (trunc) MCC_HIP(h, hipMemcpyAsync(trunc + p0 * K, d.trunc, pk * 8, hipMemcpyDeviceToHost, h->stream));
        if (ones) MCC_HIP(h, hipMemcpyAsync(ones + p0 * K, d.ones, pk * 8, hipMemcpyDeviceToHost, h->stream));
        MCC_HIP(h, hipStreamSynchronize(h->stream));
        MCC_HIP(h, h->timer.collect());
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
    return mcc::open<Handle>(device, handle, "mci_init", [] {      // beyond the 64 KiB a launch may ask for by default
        return hipFuncSetAttribute((const void*)k_lag<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(MCI_LDS_WORDS));
    });
}

void mci_free(void* handle) { mcc::close((Handle*)handle); }

const char* mci_last_error(void* handle) { return mcc::last_error((Handle*)handle); }

int mci_set_workspace_limit(void* handle, size_t bytes) { return mcc::set_workspace_limit((Handle*)handle, bytes); }

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
    if (const int rc = mcc::upload_span(h, draws, dtype, C, N, P, stride_c, stride_n, stride_p)) return rc;
    return run_dev(h, h->up, dtype, C, N, P, stride_c, stride_n, stride_p, lower, upper, K, ess, trunc, ones);
}

int mci_indicator_ess_host(const double* chains, int64_t C, int64_t N, const double* lower, const double* upper, int K,
                           double* ess, int64_t* trunc, int64_t* ones)
{
    if (const int rc = check_call(g_err, chains, MCR_F64, C, N, 1, N, 1, 0, lower, upper, K)) return rc;
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

int mci_profile_enable(void* handle, int on) { return mcc::profile_enable((Handle*)handle, on); }

int mci_kernel_ms(void* handle, double* ms, int cap) { return mcc::kernel_ms((Handle*)handle, "mci", "MCI", ms, cap); }

}  // extern "C"
