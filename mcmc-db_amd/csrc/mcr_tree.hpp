// mcr_tree.hpp -- the fixed-association sum of the importance-weighted summaries (mcr_weighted.hpp) and of simulation-based
// calibration (mcr_sbc.hpp), on the device and on the host.
//
// ONE association for every sum.  The indices of a sum are cut into blocks of kWgtBlock = 1024 consecutive ones; a
// block's terms are the leaves of the balanced binary tree over adjacent indices (leaf i of the block is index
// 1024 b + i, +0 past the end):
//     node(0, i) = leaf i          node(L, i) = node(L-1, 2 i) + node(L-1, 2 i + 1)          block sum = node(10, 0)
// and the blocks are added in ascending order from +0.  The in-block prefix of c = j + 1 leaves is the root of the SAME
// tree with the leaves from c on replaced by +0 (wgt_prefix): for c = 1024 it is the root, so a block's sum IS its last
// in-block prefix; it never falls as c grows, and zero weights leave it where it is, so that "the first j whose
// cumulative weight reaches t" is one index whichever way it is searched.  Products are rounded before they are added
// (fp contract off).
#pragma once
#include <vector>
#include "mcr_device.hpp"

namespace mcr {

constexpr int kWgtBlock = 1024;               // MCR_WEIGHTED_BLOCK: consecutive indices of one tree
constexpr int kWgtLevels = 10;                // log2(kWgtBlock)
constexpr int kWgtRows = kWgtBlock / (2 * kWave);   // a wave's 16-byte loads per lane and block
static_assert(kWgtRows == 8 && (1 << kWgtLevels) == kWgtBlock, "the wave's join of its rows is written for eight");

__host__ __device__ inline i64 wgt_blocks(i64 M) { return (M + kWgtBlock - 1) / kWgtBlock; }

// A node of the tree: one rounded sum.
__host__ __device__ inline double wgt_add(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}

// The in-block prefix of the first c leaves, c in [1, kWgtBlock]: the root of the tree whose leaves from c on are +0.
// A sum with +0 is its other operand, so what is left are the aligned nodes named by the binary digits of c, added from
// the smallest to the largest.  node(L, i) is the tree's node i of level L.  Every sum is monotone in its operands: the
// prefix never falls from c to c + 1, and it stays where the weights are zero.
template <class Node>
__host__ __device__ inline double wgt_prefix(const Node& node, int c)
{
    double acc = 0.0;
    bool any = false;
    for (int L = 0; L <= kWgtLevels; ++L)
        if (c & (1 << L)) {
            const double n = node(L, (c >> L) - 1);
            acc = any ? wgt_add(n, acc) : n;
            any = true;
        }
    return acc;
}

// The root of a block's tree from one wave: v[r] = leaf(128 r + 2 lane) + leaf(128 r + 2 lane + 1), level 1.  The xor
// steps 1 .. 32 are the levels 2 .. 7 (an IEEE sum does not depend on the order of its two operands), the join of the eight
// rows the levels 8 .. 10.  Every lane returns the root.
__device__ __forceinline__ double wgt_wave_root(double (&v)[kWgtRows])
{
#pragma clang fp contract(off)
    for (int o = 1; o < kWave; o <<= 1) {
#pragma unroll
        for (int r = 0; r < kWgtRows; ++r) v[r] = v[r] + __shfl_xor(v[r], o, kWave);
    }
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// sums[0] + sums[1] + ... + sums[n - 1] in ascending order from +0 by one wave: 64 consecutive sums per coalesced load,
// then the additions one after the other on every lane (a broadcast per term, no dependent load in the chain).  Every
// lane returns the sum.  hit(b, acc, next) sees every step: the prefix in front of b and the one that includes it.
template <class Hit>
__device__ __forceinline__ double wgt_wave_serial(const double* sums, i64 n, int lane, Hit&& hit)
{
    double acc = 0.0;
    for (i64 b0 = 0; b0 < n; b0 += kWave) {
        const double v = b0 + lane < n ? sums[b0 + lane] : 0.0;
        const int m = n - b0 < kWave ? (int)(n - b0) : kWave;
#pragma unroll
        for (int l = 0; l < kWave; ++l) {                    // (unrolled: the lane is a constant, the broadcasts run ahead)
            if (l < m) {
                const double nxt = wgt_add(acc, __shfl(v, l, kWave));
                hit(b0 + l, acc, nxt);
                acc = nxt;
            }
        }
    }
    return acc;
}
__device__ __forceinline__ double wgt_wave_serial(const double* sums, i64 n, int lane)
{
    return wgt_wave_serial(sums, n, lane, [](i64, double, double) {});
}

// Elements i and i + 1 of a[0 .. M), +0 past the end.  wide: a + i is 16-byte aligned (i is even: the alignment of a).
__device__ __forceinline__ void wgt_load2(const double* __restrict__ a, i64 i, i64 M, bool wide, double& lo, double& hi)
{
    if (wide && i + 1 < M) {
        const double2 t = *reinterpret_cast<const double2*>(a + i);
        lo = t.x; hi = t.y;
    } else {
        lo = i < M ? a[i] : 0.0;
        hi = i + 1 < M ? a[i + 1] : 0.0;
    }
}

// wgt_wave_root's sums -- the same operands at every node, so the same bits -- with 10 cross-lane exchanges of a double
// instead of 48.  The eight rows each need the xor tree over the 64 lanes; at the steps 1, 2 and 4 a lane keeps the half of
// its values its lane bit names and sends the other half to the partner, who keeps those: both add own + partner's, which
// is what v + shfl_xor(v) adds (an IEEE sum does not depend on the order of its operands).  From step 8 on one value is
// left per lane, row 4 b0 + 2 b1 + b2 of the lane's low bits b0 b1 b2; the rows' totals are then read from the lanes
// 0, 4, 2, 6, 1, 5, 3, 7 and joined as levels 8 .. 10.  Every lane returns the root.
__device__ __forceinline__ double sbc_wave_root(const double (&v)[kWgtRows], int lane)
{
#pragma clang fp contract(off)
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
    double a[4], c[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = (b0 ? v[j + 4] : v[j]) + __shfl_xor(b0 ? v[j] : v[j + 4], 1, kWave);
#pragma unroll
    for (int j = 0; j < 2; ++j) c[j] = (b1 ? a[j + 2] : a[j]) + __shfl_xor(b1 ? a[j] : a[j + 2], 2, kWave);
    double d = (b2 ? c[1] : c[0]) + __shfl_xor(b2 ? c[0] : c[1], 4, kWave);
    for (int o = 8; o < kWave; o <<= 1) d = d + __shfl_xor(d, o, kWave);
    const double t0 = __shfl(d, 0, kWave), t1 = __shfl(d, 4, kWave), t2 = __shfl(d, 2, kWave), t3 = __shfl(d, 6, kWave);
    const double t4 = __shfl(d, 1, kWave), t5 = __shfl(d, 5, kWave), t6 = __shfl(d, 3, kWave), t7 = __shfl(d, 7, kWave);
    return ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7));
}

// The host routine's tree of one block: every level, level L at lev[L].
struct WgtHostTree {
    std::vector<double> lev[kWgtLevels + 1];
    WgtHostTree() { for (int L = 0; L <= kWgtLevels; ++L) lev[L].resize((size_t)(kWgtBlock >> L)); }
    // leaf(i): term i of the block, +0 past the end of the sum
    template <class Leaf> double build(Leaf&& leaf)
    {
        for (int i = 0; i < kWgtBlock; ++i) lev[0][(size_t)i] = leaf(i);
        for (int L = 1; L <= kWgtLevels; ++L)
            for (int i = 0; i < (kWgtBlock >> L); ++i) lev[L][(size_t)i] = wgt_add(lev[L - 1][(size_t)(2 * i)], lev[L - 1][(size_t)(2 * i + 1)]);
        return lev[kWgtLevels][0];
    }
    double operator()(int L, int i) const { return lev[L][(size_t)i]; }
};

// A sum of M terms in the one association: the blocks' roots, added in ascending order from +0.  roots: kept where given.
template <class Term> inline double wgt_host_sum(WgtHostTree& tr, i64 M, Term&& term, std::vector<double>* roots = nullptr)
{
    double acc = 0.0;
    for (i64 b = 0; b < wgt_blocks(M); ++b) {
        const double r = tr.build([&](int i) { const i64 m = b * kWgtBlock + i; return m < M ? term(m) : 0.0; });
        if (roots) roots->push_back(r);
        acc = wgt_add(acc, r);
    }
    return acc;
}

}  // namespace mcr
