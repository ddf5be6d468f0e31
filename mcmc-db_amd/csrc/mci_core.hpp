// mci_core.hpp -- the arithmetic of include/mcmcref_iess.h that the host routine and the lag kernel share as ONE text:
// the hi/lo pair of A(lag), its conversion to double, var_hat, rho, the funnel of two words, the count of a bit prefix
// and the halving tree of a block of terms.  Compiled without fused multiply-add on both sides (the pragma below and
// -ffp-contract=off), so the two agree in bits.
#pragma once

#include <cstdint>

#include "mcmcref_iess.h"

#if defined(__HIPCC__)
#define MCI_HD __host__ __device__ inline
#else
#define MCI_HD inline
#endif

namespace mci {

// A(lag): a 128-bit two's complement integer as a pair.
struct Wide {
    int64_t hi;
    uint64_t lo;
};

MCI_HD Wide wide_add(Wide a, int64_t v)
{
    const uint64_t lo = a.lo + (uint64_t)v;
    const int64_t carry = lo < a.lo ? 1 : 0;
    return Wide{a.hi + (v < 0 ? -1 : 0) + carry, lo};
}

MCI_HD bool wide_negative(Wide a) { return a.hi < 0; }

MCI_HD double wide_to_double(Wide a)
{
#pragma clang fp contract(off)
    const bool neg = a.hi < 0;
    uint64_t hi = (uint64_t)a.hi, lo = a.lo;
    if (neg) {                                     // the magnitude: ~a + 1
        lo = ~lo + 1u;
        hi = ~hi + (lo == 0 ? 1u : 0u);
    }
    const double mag = (double)hi * 18446744073709551616.0 + (double)lo;
    return neg ? -mag : mag;
}

// b_i b_{i+lag} for the 64 draws of word w, given the words that hold draws 64 (w + q) ... : lag = 64 q + r.
MCI_HD uint64_t funnel(uint64_t a, uint64_t b, int r) { return r == 0 ? a : (a >> r) | (b << (64 - r)); }

// ones among the first j bits of a chain: pre = the ones of its words before word j / 64, word = that word.
MCI_HD int64_t prefix_ones(uint32_t pre, uint64_t word, int64_t j)
{
    const int r = (int)(j & 63);
    return (int64_t)pre + (r ? (int64_t)__builtin_popcountll(word & ((1ull << r) - 1ull)) : 0);
}

// A_c(lag) from the integer counts.
MCI_HD int64_t chain_a(int64_t n, int64_t lag, int64_t k, int64_t S, int64_t H, int64_t T)
{
    return n * n * S - n * k * (H + T) + (n - lag) * k * k;
}

MCI_HD double var_hat(int64_t wnum, int64_t q, int64_t n, int64_t m)
{
#pragma clang fp contract(off)
    const double dn = (double)n, dm = (double)m;
    const double W = (double)wnum / (dn * (double)(n - 1)) / dm;
    const double B = m > 1 ? (double)q / (dm * dn * (double)(m - 1)) : 0.0;
    const double a = ((double)(n - 1) / dn) * W;
    const double b = B / dn;
    return a + b;
}

MCI_HD double rho(Wide A, int64_t n, int64_t lag, int64_t m, double vh)
{
#pragma clang fp contract(off)
    const double dn = (double)n;
    const double den = dn * dn * (double)(n - lag);
    const double scale = (double)m * vh;
    return wide_to_double(A) / den / scale;
}

MCI_HD double ess_of(int64_t n, int64_t m, double R)
{
#pragma clang fp contract(off)
    const double twice = 2.0 * R;
    return ((double)m * (double)n) / (1.0 + twice);
}

// The halving tree over the MCI_LAG_BLOCK terms of a block: the host walks it alone (first = 0, step = 1, a barrier that
// does nothing), a workgroup with first = its thread, step = its size and __syncthreads.
template <class Barrier>
MCI_HD double block_sum(double* t, int first, int step, Barrier barrier)
{
    for (int s = MCI_LAG_BLOCK / 2; s >= 1; s >>= 1) {
        for (int i = first; i < s; i += step) t[i] = t[i] + t[i + s];
        barrier();
    }
    return t[0];
}

}  // namespace mci
