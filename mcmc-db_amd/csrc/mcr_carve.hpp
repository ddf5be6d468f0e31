// mcr_carve.hpp -- cutting a workspace into buffers and fitting a chunk under a limit.  Knows nothing of the context:
// mcr_host.hpp includes it for the units of libmcmcref_hip.so, mcc_handle.hpp for the companion libraries that stand alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mcr {

using i64 = long long;                                       // (as mcr_device.hpp)

namespace host {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Cuts a workspace into 256-byte aligned buffers.  A Carve with a null base only measures: off ends as the byte count.
// Over a real workspace of `end` bytes a take past the end hands out nullptr, and the caller fails on over().
struct Carve {
    char* base; size_t end = SIZE_MAX; size_t off = 0;
    template <typename T> T* take(size_t n)
    {
        off = align_up(off, 256);
        T* p = base && off + n * sizeof(T) <= end ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
    bool over() const { return off > end; }
};

// The chunk size of a call under the workspace limit: the largest k in [1, hi] that fits, 0 when not even 1 does.  fits
// is monotone (k fits: so does every smaller count) and is asked about hi first -- a call that fits whole costs one
// measurement.
template <class Fits> i64 most_that_fit(i64 hi, Fits&& fits)
{
    if (hi < 1) return 0;
    if (fits(hi)) return hi;
    if (!fits(1)) return 0;
    i64 lo = 1;                                              // lo fits, hi does not
    while (hi - lo > 1) { const i64 mid = lo + (hi - lo) / 2; if (fits(mid)) lo = mid; else hi = mid; }
    return lo;
}

}  // namespace host
}  // namespace mcr
