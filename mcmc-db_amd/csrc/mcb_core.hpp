// mcb_core.hpp -- the arithmetic of include/mcmcref_bm.h that the host routines and the kernels share as ONE text: the
// leaf, the batch mean, the finish and the pool, and the host's statement of the summation tree.  Compiled without fused
// multiply-add on both sides (the pragmas below and -ffp-contract=off), so the two agree in bits.  The tree is the
// project's one association (csrc/mcr_tree.hpp), restated here because this library includes nothing of the main one.
#pragma once

#include <cmath>
#include <cstdint>

#include "mcmcref_bm.h"

#if defined(__HIPCC__)
#define MCB_HD __host__ __device__ inline
#else
#define MCB_HD inline
#endif

namespace mcb {

constexpr int kLevels = 10;                    // log2(MCB_BLOCK)
static_assert((1 << kLevels) == MCB_BLOCK, "the tree of a block has ten levels");

// A node of the tree: one rounded sum.
MCB_HD double add(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

// t_i = x_i - K_p, rounded once; an f32 draw is widened exactly first.
template <class T>
MCB_HD double leaf(T x, double pivot)
{
#pragma clang fp contract(off)
    return (double)x - pivot;
}

// K_p + s / count: a batch mean from its sum (count = b) and the overall mean from the sum of the sums (count = A b).
MCB_HD double mean_of(double pivot, double s, int64_t count)
{
#pragma clang fp contract(off)
    const double q = s / (double)count;
    return pivot + q;
}

// f = b A / (A - 1), the operations left to right.
MCB_HD double lrv_factor(int64_t b, int64_t A)
{
#pragma clang fp contract(off)
    const double ba = (double)b * (double)A;
    return ba / (double)(A - 1);
}

// One entry of Sigma: cb f for r = 1, 2 (cb f) - cb3 f3 for r = 3; NaN for A < 2.
MCB_HD double finish_entry(double cb, double cb3, double f, double f3, int r, int64_t A)
{
#pragma clang fp contract(off)
    if (A < 2) return (double)NAN;
    const double sb = cb * f;
    if (r == 1) return sb;
    const double s3 = cb3 * f3;
    const double twice = 2.0 * sb;
    return twice - s3;
}

// One entry of V; sa is not read when one matrix is pooled alone (two == false).
MCB_HD double pool_entry(double si, double sj, double sr, double mr, double sa, double ma, bool two, bool diag, double jitter)
{
#pragma clang fp contract(off)
    const double ss = si * sj;
    double t = sr / mr;
    if (two) {
        const double u = sa / ma;
        t = t + u;
    }
    const double v = ss * t;
    return diag ? v + jitter : v;
}

MCB_HD double pool_shift(double s, double mu_ref, double mu_act, bool two)
{
#pragma clang fp contract(off)
    const double diff = two ? mu_act - mu_ref : mu_ref;
    return s * diff;
}

MCB_HD double pool_z(double d, double vii)
{
#pragma clang fp contract(off)
    return d / sqrt(vii);
}

// The host's tree: the sum of term(0) ... term(n - 1) in blocks of MCB_BLOCK, every level written out.  A short last block
// is built over the smallest power of two that holds it: the levels above only add +0, which changes nothing but the sign
// of a zero root, and the sum with the accumulator settles that.
template <class Term>
inline double tree_sum(int64_t n, Term&& term)
{
    double lev[MCB_BLOCK];
    double acc = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += MCB_BLOCK) {
        int width = 1;
        while (width < MCB_BLOCK && b0 + width < n) width *= 2;
        for (int i = 0; i < width; ++i) lev[i] = b0 + i < n ? term(b0 + i) : 0.0;
        for (int w = width / 2; w >= 1; w >>= 1)
            for (int i = 0; i < w; ++i) lev[i] = add(lev[2 * i], lev[2 * i + 1]);
        acc = add(acc, lev[0]);
    }
    return acc;
}

}  // namespace mcb
