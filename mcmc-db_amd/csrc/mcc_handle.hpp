// mcc_handle.hpp -- what the companion libraries (libmcmcref_iess.so, libmcmcref_bm.so, libmcmcref_std.so, libmcmcref_recdf.so) share around
// their kernels: the error text, the HIP-call macro, the kernel timer, the limit / profile / kernel_ms entries, and for the
// libraries that stand alone (mci_api.hip, mcb_api.hip) the handle with its stream and two grow-only device allocations.
// Header-only, and nothing of libmcmcref_hip.so's but the return codes and the context-free mcr_carve.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/mcmcref_hip.h"
#include "mcr_carve.hpp"

namespace mcc {

using mcr::host::Carve;
using mcr::host::align_up;
using mcr::host::most_that_fit;

constexpr size_t kErr = 512;
inline thread_local char g_err[kErr] = "";                   // the error of an entry that takes no handle, init among them

inline int fail(char* err, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(err, kErr, fmt, ap);
    va_end(ap);
    return code;
}

#define MCC_HIP(h, call)                                                                                            \
    do {                                                                                                            \
        const hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) return mcc::fail((h)->err, MCR_EHIP, "%s: %s", #call, hipGetErrorString(e_));         \
    } while (0)

// The kernels of one call between events on its stream: begin, a mark behind each kernel (or phase), and after the
// stream was synchronised collect adds every interval to its kernel's time.  Off (the default): nothing is recorded.
template <int kKernels> struct Timer {
    static constexpr int kMarks = kKernels > 3 ? kKernels : 3;
    bool on = false;
    hipEvent_t ev[kMarks + 1] = {};
    int kernel[kMarks] = {}, n = 0;
    double ms[kKernels] = {};

    hipError_t create()
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i <= kMarks && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
        return e;
    }
    void destroy()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void clear()
    {
        for (double& v : ms) v = 0.0;
    }
    hipError_t begin(hipStream_t s)
    {
        n = 0;
        return on ? hipEventRecord(ev[0], s) : hipSuccess;
    }
    hipError_t mark(hipStream_t s, int k)
    {
        if (!on) return hipSuccess;
        kernel[n] = k;
        return hipEventRecord(ev[++n], s);
    }
    hipError_t collect()
    {
        for (int i = 0; i < n; ++i) {
            float t = 0.f;
            if (const hipError_t e = hipEventElapsedTime(&t, ev[i], ev[i + 1])) return e;
            ms[kernel[i]] += t;
        }
        n = 0;
        return hipSuccess;
    }
};

// What every companion handle has, one that runs on an mcr_ctx too.
template <int kKernels> struct Common {
    size_t limit = (size_t)1 << 30;     // workspace of one chunk of parameters
    Timer<kKernels> timer;
    char err[kErr] = "";
};

// The handle of a library that stands alone.
template <int kKernels> struct Handle : Common<kKernels> {
    int device = 0;
    hipStream_t stream = nullptr;
    void* ws = nullptr;                 // one chunk's workspace
    size_t ws_bytes = 0;
    void* up = nullptr;                 // the host entry's copy of the tensor (and what the library puts behind it)
    size_t up_bytes = 0;
};

template <class H> void close(H* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ws) (void)hipFree(h->ws);
    if (h->up) (void)hipFree(h->up);
    h->timer.destroy();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// <entry> is the library's init, for its messages; post() is what only that library sets up, after the device is current.
template <class H, class Post> int open(int device, void** handle, const char* entry, Post&& post)
{
    if (!handle) return fail(g_err, MCR_EINVAL, "%s: NULL handle pointer", entry);
    *handle = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(g_err, MCR_ENODEVICE, "no HIP device is usable");
    }
    if (device < 0 || device >= count) return fail(g_err, MCR_ENODEVICE, "device %d: %d device(s) are visible", device, count);
    H* h = new H;
    h->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = h->timer.create();
    if (e == hipSuccess) e = post();
    if (e != hipSuccess) {
        fail(g_err, MCR_EHIP, "%s: %s", entry, hipGetErrorString(e));
        close(h);
        return MCR_EHIP;
    }
    *handle = h;
    return MCR_OK;
}

// The one growth rule of ws and up: large enough, or freed and allocated anew.  `what` ends the message.
template <class H> int ensure(H* h, void** ptr, size_t* have, size_t need, const char* what)
{
    if (need <= *have) return MCR_OK;
    if (*ptr) MCC_HIP(h, hipFree(*ptr));
    *ptr = nullptr;
    *have = 0;
    if (hipMalloc(ptr, need) != hipSuccess) {
        *ptr = nullptr;
        (void)hipGetLastError();
        return fail(h->err, MCR_ENOMEM, "cannot allocate %zu bytes %s", need, what);
    }
    *have = need;
    return MCR_OK;
}

// A host tensor's span -- the bytes its strides reach -- into h->up, with `behind` more bytes after it (256-aligned, at
// *tail).  Complete on return: the kernels may start.
template <class H> int upload_span(H* h, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                                   int64_t sp, size_t behind = 0, char** tail = nullptr)
{
    const size_t span = ((size_t)(C - 1) * (size_t)sc + (size_t)(N - 1) * (size_t)sn + (size_t)(P - 1) * (size_t)sp + 1) *
                        (dtype == MCR_F64 ? 8 : 4);
    MCC_HIP(h, hipSetDevice(h->device));
    if (const int rc = ensure(h, &h->up, &h->up_bytes, align_up(span, 256) + behind, "for the tensor")) return rc;
    if (tail) *tail = (char*)h->up + align_up(span, 256);
    MCC_HIP(h, hipMemcpy(h->up, draws, span, hipMemcpyHostToDevice));
    return MCR_OK;
}

// ---- the bodies of <prefix>_last_error, _set_workspace_limit, _profile_enable and _kernel_ms -------------------------------

template <class H> const char* last_error(H* h) { return h ? h->err : g_err; }

template <class H> int set_workspace_limit(H* h, size_t bytes)
{
    if (!h) return MCR_EINVAL;
    if (bytes == 0) return fail(h->err, MCR_EINVAL, "a workspace limit of 0 bytes");
    h->limit = bytes;
    return MCR_OK;
}

template <class H> int profile_enable(H* h, int on)
{
    if (!h) return MCR_EINVAL;
    h->timer.on = on != 0;
    h->timer.clear();
    return MCR_OK;
}

// lib / LIB: the library's prefix in both cases, as its entry and its constant are spelt.
template <class H> int kernel_ms(H* h, const char* lib, const char* LIB, double* ms, int cap)
{
    if (!h) return MCR_EINVAL;
    constexpr int kKernels = (int)(sizeof h->timer.ms / sizeof(double));
    if (!ms || cap < kKernels) return fail(h->err, MCR_EINVAL, "%s_kernel_ms needs room for %s_KERNELS = %d times", lib, LIB, kKernels);
    for (int i = 0; i < kKernels; ++i) ms[i] = h->timer.ms[i];
    return MCR_OK;
}

}  // namespace mcc
