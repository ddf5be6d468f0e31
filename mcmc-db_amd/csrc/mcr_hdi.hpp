// mcr_hdi.hpp -- highest-density intervals: the shortest interval that holds a given share of a parameter's pooled draws
// (ArviZ's unimodal hdi: numpy.argmin(s[inc:] - s[:M - inc]) on the sorted draws s).  The definition is in mcmcref_hip.h.
// Everything in front of the kernels -- the pooled ascending order, the non-finite count -- is the summary pipeline's,
// run without diagnostics: the kernels read the sort stage's keys, as k_pareto_fit does.
//
//   inc = floor(prob * M)  (the host's, one rounded product)      W = M - inc windows
//   w_i = x_(i + inc) - x_(i),  i = 0 .. W-1                      i* = the first i with the least w_i
//   lo = x_(i*),  hi = x_(i* + inc),  index = i*
//
// The least (width, index) in lexicographic order is the same however the windows are grouped, so nothing here fixes an
// order of evaluation: a parameter's bits do not depend on its place in a batch, the chunking, the slice length or the
// loads' width.  ONE text compares two candidates on the device and on the host (hdi_before).
#pragma once
#include "mcr_device.hpp"

namespace mcr {

constexpr int kHdiNT = 256;                   // threads of a k_hdi_window workgroup
constexpr i64 kHdiSlice = 16384;              // windows of a workgroup (MCR_HDI_SLICE): 64 per lane, 256 KB of keys
constexpr int kHdiMaxProbs = 16;              // probabilities of a call (MCR_HDI_MAX_PROBS)

// A candidate: a window's width and its first draw.  none(): behind every window, +inf wide ones included.
struct HdiCand {
    double w; i64 i;
    __host__ __device__ static HdiCand none() { return {INFINITY, (i64)0x7FFFFFFFFFFFFFFFll}; }
};
// Whether a stands before b: the narrower one, of two equally wide ones the earlier (numpy.argmin's first minimum).  A
// NaN width (non-finite draws: the call fails with MCR_ENONFINITE anyway) stands before nothing.
__host__ __device__ inline bool hdi_before(const HdiCand& a, const HdiCand& b)
{
    return a.w < b.w || (a.w == b.w && a.i < b.i);
}
__host__ __device__ inline void hdi_take(HdiCand& best, double w, i64 i)
{
    const HdiCand c{w, i};
    if (hdi_before(c, best)) best = c;
}

// The probabilities of a call as window offsets (by value: no upload)
struct HdiArgs {
    int nprob;
    i64 inc[kHdiMaxProbs];
};

__host__ __device__ inline i64 hdi_slices(i64 W) { return W < 1 ? 0 : (W + kHdiSlice - 1) / kHdiSlice; }

// ------------------------------------------------------------------------------------------------
// k_hdi_window: one workgroup per (parameter, probability, slice of kHdiSlice windows).  grid: ceil(pc / 8) * 8 * nprob *
// nsl, one-dimensional (xcd_map: a parameter's workgroups on the XCD whose L2 holds the keys the sort stage has just
// written); nsl = hdi_slices(M), the most any probability needs -- a workgroup whose slice lies behind its probability's
// W windows returns at once.  Lane l takes windows l, l + 256, .. of the slice (consecutive lanes, consecutive doubles in
// both streams k[i] and k[i + inc]); where both streams are 16-byte aligned at once -- inc even, after at most one
// peeled window -- a lane takes two windows per pair of 16-byte loads.  The (width, index) minimum stays in registers,
// meets across the wave by xor shuffles and across the four waves through LDS.
// part[((p * nprob + j) * nsl + s)] = the slice's candidate.  Reads keys[p * M + 0 .. M-1] only: i + inc <= W-1 + inc = M-1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHdiNT) void k_hdi_window(const double* __restrict__ keys, i64 M, i64 pc, HdiArgs a, int nsl,
                                                       HdiCand* __restrict__ part)
{
    __shared__ HdiCand sh[kHdiNT / kWave];
    i64 p;
    int blk;
    if (!xcd_map(pc, a.nprob * nsl, p, blk)) return;
    const int j = blk / nsl, s = blk % nsl;
    const i64 inc = a.inc[j], W = M - inc;
    const i64 i0 = (i64)s * kHdiSlice;
    if (i0 >= W) return;                                           // (uniform over the workgroup)
    const i64 i1 = i0 + kHdiSlice < W ? i0 + kHdiSlice : W;
    const int tid = threadIdx.x;
    const double* k = keys + p * M;
    HdiCand best = HdiCand::none();
    i64 done = i0;                                                 // windows [i0, done) are taken by the wide loop
    if ((inc & 1) == 0 && i1 - i0 >= 4) {
        const i64 ia = i0 + (i64)(((uintptr_t)(k + i0) >> 3) & 1); // the first window whose k[i] is 16-byte aligned
        const i64 np = (i1 - ia) >> 1;                             // pairs of windows from there
        if (ia > i0 && tid == kHdiNT - 1) hdi_take(best, k[i0 + inc] - k[i0], i0);
        const double2* lo2 = reinterpret_cast<const double2*>(k + ia);
        const double2* hi2 = reinterpret_cast<const double2*>(k + ia + inc);
#pragma unroll 4
        for (i64 q = tid; q < np; q += kHdiNT) {
            const double2 l = lo2[q], h = hi2[q];
            hdi_take(best, h.x - l.x, ia + 2 * q);
            hdi_take(best, h.y - l.y, ia + 2 * q + 1);
        }
        done = ia + 2 * np;                                        // at most one window is left
    }
#pragma unroll 4
    for (i64 i = done + tid; i < i1; i += kHdiNT) hdi_take(best, k[i + inc] - k[i], i);
    for (int o = kWave >> 1; o > 0; o >>= 1) {
        const HdiCand c{__shfl_xor(best.w, o, kWave), (i64)__shfl_xor((long long)best.i, o, kWave)};
        if (hdi_before(c, best)) best = c;
    }
    if ((tid & (kWave - 1)) == 0) sh[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < kHdiNT / kWave; ++v)
            if (hdi_before(sh[v], best)) best = sh[v];
        part[(p * a.nprob + j) * nsl + s] = best;
    }
}

// ------------------------------------------------------------------------------------------------
// k_hdi_pick: one thread per (parameter, probability) takes the least of the pair's slice candidates, in slice order, and
// writes lo, hi and the index (a double: exact below 2^53) into the result table behind the pipeline's rows:
// res[(field0 + 3 j + {0, 1, 2}) * pc + p].  W < 1 (the product rounded up to M): NaN, NaN, -1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hdi_pick(const double* __restrict__ keys, i64 M, i64 pc, HdiArgs a, int nsl,
                                                 const HdiCand* __restrict__ part, double* __restrict__ res, int field0)
{
    const i64 t = (i64)blockIdx.x * 64 + threadIdx.x;
    if (t >= pc * a.nprob) return;
    const i64 p = t / a.nprob;
    const int j = (int)(t % a.nprob);
    const i64 inc = a.inc[j];
    const int ns = (int)hdi_slices(M - inc);
    HdiCand best = HdiCand::none();
    for (int s = 0; s < ns; ++s) {
        const HdiCand c = part[(p * a.nprob + j) * nsl + s];
        if (hdi_before(c, best)) best = c;
    }
    const bool ok = best.i >= 0 && best.i < M - inc;              // (no window, or only NaN widths: nothing to index)
    double* r = res + (i64)(field0 + 3 * j) * pc + p;
    r[0] = ok ? keys[p * M + best.i] : NAN;
    r[pc] = ok ? keys[p * M + best.i + inc] : NAN;
    r[2 * pc] = ok ? (double)best.i : -1.0;
}
}  // namespace mcr
