// mcr_layout.hpp -- the row order of a long draws table, on the device.
//
// Reference: `_chains_from_table` (src/mcmc_ref/convert.py:150-161) groups the rows by chain id and sorts every group
// by draw index with Python's stable sort, then walks the chain ids in ascending order: the order of the values is
// np.lexsort((draw, chain)) -- chain ascending, draw ascending within a chain, rows with equal (chain, draw) in file
// order.  Here that order is a stable LSD radix sort of one packed key per row:
//     key = (chain - cmin) << bits(dmax - dmin) | (draw - dmin)          (differences taken as unsigned 64-bit)
// so a table with few chains and some thousand draws has two significant key bytes and takes two 8-bit passes.
// The rows of most tables are in that order already: k_layout_scan makes pq::k_chain_layout's test row by row, in
// parallel, together with the min / max reduction the key needs, and an ordered table is never sorted.  A pass
// is three launches: k_layout_hist (digit histogram of every workgroup's span of kLayoutSpan rows), k_layout_offsets
// (exclusive scan over (digit, workgroup)), k_layout_scatter (a workgroup walks its span in rounds of 256 rows; a
// row's place among the rows of its digit is the count of earlier rows of the round with that digit -- wave ballots
// and the waves' counts in the LDS -- behind the rounds before it, so rows of equal digit keep their input order).
// Keys are u64, row numbers u32 (M < 2^31).  Plain HIP C++, vector stores only.
#pragma once
#include "mcr_device.hpp"
#include "mcr_parquet.hpp"

namespace mcr {
namespace layout {

constexpr int kLayoutNT = 256;
constexpr int kLayoutRounds = 8;
constexpr int kLayoutSpan = kLayoutNT * kLayoutRounds;       // rows per workgroup of a histogram / scatter launch
constexpr int kScanGrid = 64;                                // workgroups (partial records) per table of k_layout_scan

// One table's id columns in device memory (the descriptor pq::k_chain_layout takes: mcr_parquet.hpp).
using Table = pq::FileIds;

// The layout test of pq::k_chain_layout (rows already in (chain ascending, draw ascending) order?) taken row-parallel,
// and the extremes of both columns, for the tables of a call at once: grid (kScanGrid, tables).
// part[(t kScanGrid + g) 5 .. + 5) = (min chain, max chain, min draw, max draw, 1 if a row sorts before the row in
// front of it) over the rows workgroup g of table t strides through (a table without rows: zeros).
__global__ __launch_bounds__(kLayoutNT) void k_layout_scan(const Table* __restrict__ tables, i64* __restrict__ part)
{
    __shared__ i64 red[5][kLayoutNT];
    const Table f = tables[blockIdx.y];
    const i64 M = f.M;
    const int tid = threadIdx.x;
    i64 c0 = 0, c1 = 0, d0 = 0, d1 = 0, bad = 0;
    if (M > 0) { c0 = c1 = f.chain[0]; d0 = d1 = f.draw[0]; }
    for (i64 r = (i64)blockIdx.x * kLayoutNT + tid; r < M; r += (i64)gridDim.x * kLayoutNT) {
        const i64 c = f.chain[r], d = f.draw[r];
        c0 = c < c0 ? c : c0; c1 = c > c1 ? c : c1;
        d0 = d < d0 ? d : d0; d1 = d > d1 ? d : d1;
        if (r > 0) {
            const i64 cp = f.chain[r - 1], dp = f.draw[r - 1];
            if (c < cp || (c == cp && d < dp)) bad = 1;
        }
    }
    red[0][tid] = c0; red[1][tid] = c1; red[2][tid] = d0; red[3][tid] = d1; red[4][tid] = bad;
    __syncthreads();
    for (int s = kLayoutNT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = red[0][tid + s] < red[0][tid] ? red[0][tid + s] : red[0][tid];
            red[1][tid] = red[1][tid + s] > red[1][tid] ? red[1][tid + s] : red[1][tid];
            red[2][tid] = red[2][tid + s] < red[2][tid] ? red[2][tid + s] : red[2][tid];
            red[3][tid] = red[3][tid + s] > red[3][tid] ? red[3][tid + s] : red[3][tid];
            red[4][tid] |= red[4][tid + s];
        }
        __syncthreads();
    }
    if (tid < 5) part[((i64)blockIdx.y * gridDim.x + blockIdx.x) * 5 + tid] = red[tid][0];
}

// res[t stride .. + 4) = the four extremes over table t's G partial records, res[t stride + 4] = 1 if its rows are in
// order.  grid (tables), block 64 (one thread per field).
__global__ void k_layout_scan_final(const i64* __restrict__ part, int G, i64* __restrict__ res, i64 stride)
{
    const int f = threadIdx.x;
    if (f >= 5) return;
    const i64* p = part + (i64)blockIdx.x * G * 5;
    i64 v = p[f];
    for (int g = 1; g < G; ++g) {
        const i64 x = p[5 * (i64)g + f];
        v = f == 4 ? (v | x) : ((f & 1) ? (x > v ? x : v) : (x < v ? x : v));
    }
    res[(i64)blockIdx.x * stride + f] = f == 4 ? (v ? 0 : 1) : v;
}

// key[r] = (chain[r] - cmin) << dbits | (draw[r] - dmin), idx[r] = r.
__global__ __launch_bounds__(kLayoutNT) void k_layout_keys(const i64* __restrict__ chain, const i64* __restrict__ draw,
                                                           i64 M, i64 cmin, i64 dmin, int dbits, u64* __restrict__ key,
                                                           u32* __restrict__ idx)
{
    const i64 r = (i64)blockIdx.x * kLayoutNT + threadIdx.x;
    if (r >= M) return;
    const u64 c = (u64)chain[r] - (u64)cmin, d = (u64)draw[r] - (u64)dmin;
    key[r] = (dbits < 64 ? c << dbits : (u64)0) | d;
    idx[r] = (u32)r;
}

// hist[digit * G + g] = rows of workgroup g's span whose key byte `shift / 8` is digit.  grid G.
__global__ __launch_bounds__(kLayoutNT) void k_layout_hist(const u64* __restrict__ key, i64 M, int shift, int G,
                                                           u32* __restrict__ hist)
{
    __shared__ u32 h[256];
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const i64 r0 = (i64)blockIdx.x * kLayoutSpan;
    for (int k = 0; k < kLayoutRounds; ++k) {
        const i64 r = r0 + k * kLayoutNT + tid;
        if (r < M) atomicAdd(&h[(u32)(key[r] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(i64)tid * G + blockIdx.x] = h[tid];
}

// Exclusive scan of hist[0 .. n) in place (n = 256 G; digit-major, so the result is every (digit, workgroup)'s first
// output row).  grid 1, block 1024.
__global__ __launch_bounds__(1024) void k_layout_offsets(u32* __restrict__ hist, i64 n)
{
    __shared__ u32 wtot[16];
    __shared__ u32 s_base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_base = 0u;
    __syncthreads();
    for (i64 k0 = 0; k0 < n; k0 += 1024) {
        const i64 k = k0 + tid;
        const u32 v = k < n ? hist[k] : 0u;
        u32 incl = v;                                        // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const u32 t = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        u32 before = s_base, total = 0u;
        for (int ww = 0; ww < 16; ++ww) { const u32 t = wtot[ww]; if (ww < w) before += t; total += t; }
        if (k < n) hist[k] = before + incl - v;
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
}

// Moves workgroup g's span to its places of this pass; offs as k_layout_offsets left it.  grid G.
__global__ __launch_bounds__(kLayoutNT) void k_layout_scatter(const u64* __restrict__ key, const u32* __restrict__ idx,
                                                              i64 M, int shift, int G, const u32* __restrict__ offs,
                                                              u64* __restrict__ key_out, u32* __restrict__ idx_out)
{
    constexpr int NW = kLayoutNT / kWave;
    __shared__ u32 base[256];
    __shared__ u32 wcnt[NW][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    base[tid] = offs[(i64)tid * G + blockIdx.x];
    for (int ww = 0; ww < NW; ++ww) wcnt[ww][tid] = 0u;
    __syncthreads();
    const i64 r0 = (i64)blockIdx.x * kLayoutSpan;
    for (int k = 0; k < kLayoutRounds; ++k) {
        const i64 r = r0 + k * kLayoutNT + tid;
        const bool live = r < M;
        const u64 kv = live ? key[r] : (u64)0;
        const u32 iv = live ? idx[r] : 0u;
        const u32 d = (u32)(kv >> shift) & 255u;
        // lanes of this wave that hold a live row of the same digit
        unsigned long long same = __ballot(live);
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? bal : ~bal;
        }
        const u32 below = (u32)__popcll(same & ((1ull << lane) - 1ull));
        if (live && below == 0u) wcnt[w][d] = (u32)__popcll(same);     // the first lane of every digit group writes its size
        __syncthreads();
        if (live) {
            u32 pos = base[d] + below;
            for (int ww = 0; ww < w; ++ww) pos += wcnt[ww][d];
            if (pos < (u32)M) { key_out[pos] = kv; idx_out[pos] = iv; }  // (always true for a consistent histogram)
        }
        __syncthreads();
        {
            u32 t = 0u;
            for (int ww = 0; ww < NW; ++ww) { t += wcnt[ww][tid]; wcnt[ww][tid] = 0u; }
            base[tid] += t;
        }
        __syncthreads();
    }
}

// order[k] = idx[k] as the i64 the gather takes.
__global__ __launch_bounds__(kLayoutNT) void k_layout_order(const u32* __restrict__ idx, i64 M, i64* __restrict__ order)
{
    const i64 k = (i64)blockIdx.x * kLayoutNT + threadIdx.x;
    if (k < M) order[k] = (i64)idx[k];
}

// The distinct chain ids of a table's rows taken in the order idx (nullptr: file order), ascending, and the first
// position of each: out = res + t stride; out[0] = count, out[1 + j] = id, out[1 + cap + j] = first row, j < min(count,
// cap).  One workgroup per table walks its rows.  grid (tables), block 1024; idx belongs to table 0 of a one-table call.
__global__ __launch_bounds__(1024) void k_layout_bounds(const Table* __restrict__ tables, const u32* __restrict__ idx,
                                                        int cap, i64* __restrict__ res, i64 stride)
{
    __shared__ u32 wtot[16];
    __shared__ u32 s_base;
    const Table f = tables[blockIdx.x];
    const i64 M = f.M;
    const i64* __restrict__ chain = f.chain;
    i64* out = res + (i64)blockIdx.x * stride;
    i64* ids = out + 1;
    i64* starts = out + 1 + cap;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_base = 0u;
    __syncthreads();
    for (i64 k0 = 0; k0 < M; k0 += 1024) {
        const i64 k = k0 + tid;
        i64 c = 0;
        bool bound = false;
        if (k < M) {
            c = chain[idx ? (i64)idx[k] : k];
            bound = k == 0 || chain[idx ? (i64)idx[k - 1] : k - 1] != c;
        }
        const unsigned long long bal = __ballot(bound);
        if (lane == 0) wtot[w] = (u32)__popcll(bal);
        __syncthreads();
        u32 before = s_base, total = 0u;
        for (int ww = 0; ww < 16; ++ww) { const u32 t = wtot[ww]; if (ww < w) before += t; total += t; }
        const u32 j = before + (u32)__popcll(bal & ((1ull << lane) - 1ull));
        if (bound && j < (u32)cap) { ids[j] = c; starts[j] = k; }
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    if (tid == 0) out[0] = (i64)s_base;
}

// dst[p][k] = src[p][order[k]] with the order in device memory; an entry outside [0, M) is not read and raises err[0].
__global__ __launch_bounds__(256) void k_gather_rows_order(const double* __restrict__ src, const i64* __restrict__ order,
                                                           i64 M, double* __restrict__ dst, int* __restrict__ err)
{
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 p = blockIdx.y;
    if (k >= M) return;
    const i64 o = order[k];
    if (o < 0 || o >= M) { if (p == 0) atomicOr(err, 1); return; }
    dst[p * M + k] = src[p * M + o];
}

}  // namespace layout
}  // namespace mcr
