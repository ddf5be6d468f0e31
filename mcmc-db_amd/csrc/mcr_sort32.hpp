// mcr_sort32.hpp -- the sort stage for f32 draw tensors (BASELINE config 4: 4 x 100000 x 10000 f32).
//
// Same algorithm as the f64 kernels of mcr_kernels.hpp (tile sort -> pairwise passes -> exact bucket partition ->
// in-LDS bucket merge fused with tie-averaged ranks), same results bit for bit (widening f32 -> f64 preserves order
// and equality, so ranks, order statistics and the widened values the moments / fold step see are identical), but the
// unit that moves is ONE 64-bit record per draw
//     record = order-preserving image of the f32 bits (f32_key) << 32 | pooled position
// instead of an f64 key plus a separate position: 8 bytes per LDS slot and per HBM element instead of 12, one integer
// compare per merge step that orders (value, position) at once, no payload gather after a merge level, and no widening
// ingest pass over the tensor.  +inf pads are kRecPad.  Reference spec of the whole stage: the `sorted(flat, key=...)`
// and average ranks of src/mcmc_ref/diagnostics.py:101-122.
#pragma once
#include "mcr_kernels.hpp"

namespace mcr {

__device__ __forceinline__ u32 rec_key(u64 r) { return (u32)(r >> 32); }
__device__ __forceinline__ u32 rec_pos(u64 r) { return (u32)r; }

// (thread_sort_rec, lane_merge_levels_rec and serial_merge_rec -- the register sort, the three DPP merge levels and the
// serial LDS merge on records -- live in mcr_kernels.hpp: the f64 tile sort runs on records as well.)

// One more slot than records: the unconditional read "one past the last run" of serial_merge_rec stays in bounds.
constexpr size_t rec_lds_bytes(int T) { return (size_t)(T + 2) * 8; }

// ------------------------------------------------------------------------------------------------
// Tile sort: 4096 pooled f32 draws of one parameter -> sorted records, the tile's moments (two-pass on the widened
// values, as k_tile_sort) and every 64th order statistic.  The tensor is read from HBM exactly once, as f32.
// ------------------------------------------------------------------------------------------------
template <int NT, int VT>
__global__ __launch_bounds__(NT) void k_tile_sort32(const float* __restrict__ X, i64 M, u64* __restrict__ recs,
                                                    double* __restrict__ part, int ntiles, double* __restrict__ samp)
{
    constexpr int T = NT * VT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* srec = reinterpret_cast<u64*>(smem);
    double* red = reinterpret_cast<double*>(smem);      // only after the sorted tile has left LDS

    const int tid = threadIdx.x, tile = blockIdx.x;
    const i64 p = blockIdx.y;
    const i64 base = (i64)tile * T;
    const int count = (int)((M - base < (i64)T) ? M - base : (i64)T);
    const float* src = X + p * M + base;

    // As k_tile_sort: lane tid takes draws i * NT + tid straight into its sort registers (no staging pass through the LDS),
    // and a full tile (count == T, workgroup-uniform) runs without the per-draw `e < count` tests.  Records are distinct
    // (the position is the low word), so the sorted tile does not depend on which draws a lane starts with.
    const bool full = count == T;
    u64 r[VT];
    double bad = 0.0;
    auto load = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int i = 0; i < VT; ++i) {
            const int e = i * NT + tid;
            const bool live = FULL || e < count;
            const float v = src[FULL ? e : min(e, count - 1)];      // every load unconditional and in flight, as in k_tile_sort
            bad += (live && !isfinite(v)) ? 1.0 : 0.0;
            r[i] = live ? (((u64)f32_key(v) << 32) | (u64)(u32)(base + e)) : kRecPad;
        }
    };
    if (full) load(std::true_type{}); else load(std::false_type{});
    thread_sort_rec<VT>(r);
    constexpr bool kLaneLevels = MCR_TILE_DPP_LEVELS >= 3 && VT == 16;
    if constexpr (kLaneLevels) lane_merge_levels_rec(r);
    // (no barrier: this is the workgroup's first access to the LDS)
#pragma unroll
    for (int i = 0; i < VT; ++i) srec[pos16(tid * VT + i)] = r[i];
    __syncthreads();

    for (int coop = kLaneLevels ? 16 : 2; coop <= NT; coop <<= 1) {
        const int first = tid & ~(coop - 1);
        const int run = VT * (coop >> 1);
        const int a0 = first * VT, b0 = a0 + run;
        const int diag = VT * (tid - first);
        auto A = [&](int i) { return srec[pos16(a0 + i)]; };
        auto B = [&](int j) { return srec[pos16(b0 + j)]; };
        const int ai = merge_path32(A, run, B, run, diag);
        serial_merge_rec<VT, T - 1>(srec, a0, run, b0, run, ai, diag - ai, VT, r);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VT; ++i) srec[pos16(tid * VT + i)] = r[i];
        __syncthreads();
    }
    auto write_out = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
#pragma nounroll
        for (int e = tid; e < (FULL ? T : count); e += NT) recs[p * M + base + e] = srec[pos16(e)];
    };
    if (full) write_out(std::true_type{}); else write_out(std::false_type{});
    if (samp != nullptr && tid < T / 64) {
        const int e = 64 * tid + 63;
        samp[(p * ntiles + tile) * (T / 64) + tid] = (e < count) ? key_value(rec_key(srec[pos16(e)])) : INFINITY;
    }
    __syncthreads();                 // `red` aliases srec from here on
    double s1 = 0.0, s2 = 0.0, e1 = 0.0, mt = 0.0;
    auto moments = [&](auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        const int nlive = count - tid * VT;         // the lane's sorted slots [0, nlive) hold draws, the others pads
#pragma unroll
        for (int i = 0; i < VT; ++i) s1 += (FULL || i < nlive) ? key_value(rec_key(r[i])) : 0.0;
        s1 = block_sum<NT>(s1, red);
        mt = s1 / (double)count;
#pragma unroll
        for (int i = 0; i < VT; ++i) { const double d = (FULL || i < nlive) ? key_value(rec_key(r[i])) - mt : 0.0; s2 = fma(d, d, s2); e1 += d; }
    };
    if (full) moments(std::true_type{}); else moments(std::false_type{});
    block_sum3<NT>(s2, e1, bad, red);
    if (tid == 0) store_slice_moments(part + (p * ntiles + tile) * kMomRec, mt, e1, s2, bad, (double)count);
}

// ------------------------------------------------------------------------------------------------
// One pairwise merge-path pass over sorted runs of R records (pooled arrays longer than 16 tiles).
// ------------------------------------------------------------------------------------------------
template <int NT, int VT>
__global__ __launch_bounds__(NT) void k_merge32(const u64* __restrict__ rin, u64* __restrict__ rout, i64 M, i64 R)
{
    constexpr int OB = NT * VT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* srec = reinterpret_cast<u64*>(smem);
    __shared__ i64 sh[2];
    const int tid = threadIdx.x;
    const i64 p = blockIdx.y;
    const i64 o0 = (i64)blockIdx.x * OB;
    if (o0 >= M) return;
    const u64* rp = rin + p * M;
    const i64 pb = (o0 / (2 * R)) * (2 * R);
    const i64 abase = pb, na = (M - pb < R) ? M - pb : R;
    const i64 bbase = pb + na, nb = (M - bbase < R) ? M - bbase : R;
    const i64 d0 = o0 - pb, tot = na + nb;
    const i64 d1 = (d0 + OB < tot) ? d0 + OB : tot;
    auto GA = [&](i64 i) { return rp[abase + i]; };
    auto GB = [&](i64 j) { return rp[bbase + j]; };
    if (tid < 64) { const i64 r0 = merge_path_wave(GA, na, GB, nb, d0); if (tid == 0) sh[0] = r0; }
    else if (tid < 128) { const i64 r1 = merge_path_wave(GA, na, GB, nb, d1); if (tid == 64) sh[1] = r1; }
    __syncthreads();
    const i64 ai0 = sh[0], ai1 = sh[1], bi0 = d0 - ai0;
    const int ca = (int)(ai1 - ai0), cb = (int)((d1 - ai1) - bi0);
    const int total = ca + cb;
    {   // all VT loads of a lane in flight before the first LDS store (slots beyond `total` read record 0, not stored)
        u64 gr[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            const i64 g = (e < ca) ? abase + ai0 + e : bbase + bi0 + (e - ca);
            gr[j] = rp[(e < total) ? g : 0];
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            if (e < total) srec[pos16(e)] = gr[j];
        }
    }
    __syncthreads();
    const int diag = (tid * VT < total) ? tid * VT : total;
    const int nout = (total - diag < VT) ? total - diag : VT;
    auto A = [&](int i) { return srec[pos16(i)]; };
    auto B = [&](int j) { return srec[pos16(ca + j)]; };
    const int ai = merge_path32(A, ca, B, cb, diag);
    u64 r[VT];
    serial_merge_rec<VT>(srec, 0, ca, ca, cb, ai, diag - ai, nout, r);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VT; ++i)
        if (i < nout) srec[pos16(diag + i)] = r[i];
    __syncthreads();
    for (int e = tid; e < total; e += NT) rout[p * M + o0 + e] = srec[pos16(e)];
}

// ------------------------------------------------------------------------------------------------
// Bucket merge on records (k_bucket_merge of mcr_kernels.hpp): gather <= k sorted pieces, merge in LDS, write the
// pooled ascending records and -- fused -- the rank code of every draw to time order.
// ------------------------------------------------------------------------------------------------
template <int NT, int VT>
__global__ __launch_bounds__(NT) void k_bucket_merge32(const u64* __restrict__ rin, u64* __restrict__ rout, i64 M,
                                                       int k, int B, const u32* __restrict__ cut,
                                                       const u32* __restrict__ boff, u32* __restrict__ z, i64 P, i64 R)
{
    constexpr int T = NT * VT;
    static_assert(T == 4096, "the partition bound of k_splitters assumes 4096-slot buckets");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* srec = reinterpret_cast<u64*>(smem);
    int* sst = reinterpret_cast<int*>(srec + T + 2);   // padded piece starts [k+1]; the scratch is laid out as in k_bucket_merge
    int* spl = sst + kBkLen;                            // piece lengths [k]
    int* sps = sst + kBkSrc;                            // piece source offsets in tile [k]
    int* sext = sst + kBkExt;                           // [2] does the first / last tie run go on outside the bucket?
    i64* sedge = reinterpret_cast<i64*>(sst + kBkEdge); // [4] global run bounds of the edge values
    u64* sne = reinterpret_cast<u64*>(sst + kBkNext);   // [2k] the runs' keys just before / behind their pieces
    static_assert(2 * (NT / kWave) <= 4 * kMaxBucketTiles, "the tie-run scratch takes the neighbours' place");

    const int tid = threadIdx.x;
    i64 p;
    int b;
    if (!xcd_map(P, B, p, b)) return;
    const u64* rp = rin + p * M;
    const u32* c0 = cut + (p * (B + 1) + b) * k;
    const u32* c1 = c0 + k;
    if (k < 1 || k > kMaxBucketTiles) return;       // (the scratch holds sixteen pieces)
    if (tid < kWave) bucket_piece_table(c0, c1, k, sst, spl, sps);
    __syncthreads();
    const int padded = sst[k];
    const int total = (int)(boff[p * (B + 1) + b + 1] - boff[p * (B + 1) + b]);
    const i64 obase = boff[p * (B + 1) + b];
    if (padded > T - 64 || total < 0 || total > padded || obase + total > M) return;   // never with a valid partition
    // the runs' records just before / behind this bucket's pieces ride in the gather's dead last slots (see
    // k_bucket_merge); a neighbour that does not exist is parked as a value no 32-bit key equals
    const int ne_lane = tid - (T - 64 - (VT - 1) * NT);
    bool ne_there = false;
    i64 ne_g = 0;
    if (ne_lane >= 0) ne_g = bucket_neighbour(ne_lane, k, R, M, spl, sps, ne_there);
    const bool is_ne = ne_lane >= 0 && ne_lane < 2 * k;
    u64 ne = 0;
    {   // gather: one piece search per 16-slot chunk, all VT loads in flight together (see k_bucket_merge)
        const int lane = tid & 63, wv = tid >> 6;
        u32 my_g = 0; int my_n = 0;
        if ((lane & 15) < VT) {
            const int e0 = (lane & 15) * NT + 64 * wv + 16 * (lane >> 4);
            if (e0 < padded) {
                int t = 0;
#pragma unroll
                for (int step = 8; step > 0; step >>= 1)
                    if (t + step < k && e0 >= sst[t + step]) t += step;
                const int o = e0 - sst[t];
                my_n = spl[t] - o;
                my_g = (u32)((i64)t * R) + (u32)sps[t] + (u32)o;
            }
        }
        u64 gr[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int within = lane & 15;
            const u32 g0 = (u32)row_lane((int)my_g, j);      // lane j of my row of 16 looked the chunk up
            const int n = row_lane(my_n, j);
            const bool live = within < n;
            i64 g = live ? (i64)(g0 + (u32)within) : 0;
            if (j == VT - 1) g = is_ne ? ne_g : g;
            const u64 r = rp[g];
            gr[j] = live ? r : kRecPad;
            if (j == VT - 1) ne = r;
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
            const int e = j * NT + tid;
            if (e < padded) srec[pos16(e)] = gr[j];
        }
    }
    if (is_ne) sne[ne_lane] = ne_there ? (u64)rec_key(ne) : ~0ull;
    wait_loads();
    __syncthreads();
    const int chunk0 = tid * VT;
    int mypiece = 0;      // the piece that holds slot chunk0 (pieces are padded to 16 >= VT slots)
#pragma unroll
    for (int step = 8; step > 0; step >>= 1)
        if (mypiece + step < k && chunk0 >= sst[mypiece + step]) mypiece += step;
    for (int w = 1; w < k; w <<= 1) {
        u64 r[VT];
        bool moved = false;
        if (chunk0 < padded) {
            const int ra = mypiece & ~(2 * w - 1);
            const int a0 = sst[ra];
            const int a1 = sst[(ra + w < k) ? ra + w : k];
            const int b1 = sst[(ra + 2 * w < k) ? ra + 2 * w : k];
            const int na = a1 - a0, nb = b1 - a1, diag = chunk0 - a0;
            moved = nb > 0;
            if (moved) {
                auto A = [&](int i) { return srec[pos16(a0 + i)]; };
                auto Bf = [&](int j) { return srec[pos16(a1 + j)]; };
                const int ai = merge_path32(A, na, Bf, nb, diag);
                serial_merge_rec<VT>(srec, a0, na, a1, nb, ai, diag - ai, VT, r);
            }
        }
        __syncthreads();
        if (moved) {
#pragma unroll
            for (int i = 0; i < VT; ++i) srec[pos16(chunk0 + i)] = r[i];
        }
        __syncthreads();
    }
    for (int e = tid; e < total; e += NT) rout[p * M + obase + e] = srec[pos16(e)];
    if (z == nullptr || total == 0) return;
    // tie runs that continue in a neighbouring bucket: look at the record just before / after this bucket's piece in
    // every run; only then pay for the bound searches
    if (tid < 4) sedge[tid] = 0;
    const u32 kfirst = rec_key(srec[pos16(0)]), klast = rec_key(srec[pos16(total - 1)]);
    if (tid < kWave) {
        const int t = (tid < k) ? tid : k - 1;
        const bool e0 = tid < k && sne[t] == (u64)kfirst;
        const bool e1 = tid < k && sne[k + t] == (u64)klast;
        const bool a0 = __ballot(e0) != 0, a1 = __ballot(e1) != 0;
        if (tid == 0) { sext[0] = a0; sext[1] = a1; }
    }
    __syncthreads();
    const bool ext0 = sext[0] != 0, ext1 = sext[1] != 0;
    if ((ext0 || ext1) && tid < 2 * k) {
        const int t = tid % k, which = tid / k;           // 0: first value, 1: last value
        const u32 v = which ? klast : kfirst;
        const i64 tbase = (i64)t * R;
        const int cnt = (int)((M - tbase < R) ? M - tbase : R);
        const u64* a = rp + tbase;
        int lo = 0, hi = cnt;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (rec_key(a[m]) < v) lo = m + 1; else hi = m; }
        const int lb = lo;
        hi = cnt;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (!(v < rec_key(a[m]))) lo = m + 1; else hi = m; }
        atomicAdd(reinterpret_cast<unsigned long long*>(&sedge[2 * which]), (unsigned long long)lb);
        atomicAdd(reinterpret_cast<unsigned long long*>(&sedge[2 * which + 1]), (unsigned long long)lo);
    }
    __syncthreads();
    int rs[VT], re[VT];
    block_tie_runs<NT, VT>([&](int g) { return rec_key(srec[pos16(g)]); }, total, sst + kBkNext, rs, re);
#pragma unroll
    for (int i = 0; i < VT; ++i) {
        const int e = tid * VT + i;
        if (e < total) {
            const u64 r = srec[pos16(e)];
            i64 gs = obase + rs[i], ge = obase + re[i];
            if (ext0 && rec_key(r) == kfirst) gs = sedge[0];
            if (ext1 && rec_key(r) == klast) ge = sedge[3];
            z[p * M + min(rec_pos(r), (u32)(M - 1))] = (u32)(gs + ge);   // code of the tie run: rank = (code + 1) / 2
        }
    }
}

}  // namespace mcr
