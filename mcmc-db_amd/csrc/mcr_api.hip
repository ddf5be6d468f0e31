// mcr_api.hip -- the summary unit of libmcmcref_hip.so's C ABI (see include/mcmcref_hip.h): the context's life, the
// summary pipeline and its entries, the moments, compare, profile, probe and synthetic-fill entries, with their host-side
// launch logic: workspace carving, parameter chunking, async result slots, HIP-event profiling.  The other statistics are
// mcr_stats.hip -- they run the pipeline through mcr_pipe.hpp -- the file and text entries mcr_files.hip, the communicator
// mcr_comm.hip; mcr_host.hpp is what the four share.  Plain HIP runtime only: no torch, no hipify, no compatibility layers.
#include "mcr_pipe.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <new>

#include "mcr_kernels.hpp"
#include "mcr_diag.hpp"
#include "mcr_fft.hpp"

using namespace mcr;
using namespace mcr::host;

namespace {

// Threads x draws per lane of the tile sort and of the merge kernels (passes, bucket merge, fold): the fastest measured
// (DESIGN.md section 4): 16 draws per lane give the tile sort its register merge levels, more waves hide the merges' LDS.
constexpr int kTileNT = 256, kTileVT = 16;
constexpr int kMergeNT = 512, kMergeVT = 8;
static_assert(kTileNT * kTileVT == kTile && kMergeNT * kMergeVT == kTile, "sort geometry");
constexpr i64 kIdx16Max = 65535;      // pooled arrays up to this length carry 16-bit positions through the sort
constexpr int kMaxChains = 256;
constexpr int kT3Workgroups = 256;    // workgroups of a k_tier3 launch (they share the (listed pair, lag group) items)

char g_init_err[512] = "";

}  // namespace

// What mcr_host.hpp declares for every unit and this one defines (get_ztab: mcr_pipe.hpp).
namespace mcr {
namespace host {

const char* const kKernelNames[K_COUNT] = {MCR_KERNELS(MCR_KERNEL_NAME)};

int fail(mcr_ctx* ctx, int code, const char* fmt, ...)
{
    char* dst = ctx ? ctx->err : g_init_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

// Stream must be idle (synchronised) when this is called.
void prof_resolve(mcr_ctx* ctx)
{
    for (EvPair& pr : ctx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.a, pr.b) == hipSuccess) {
            ctx->k_ms[pr.kid] += ms;
            ctx->k_launches[pr.kid] += 1;
        }
        ctx->free_ev.push_back(pr.a);
        ctx->free_ev.push_back(pr.b);
    }
    ctx->pending.clear();
}

// Every stream of the context idle (ctx->stream is always one of them); the first failure.
hipError_t sync_all(mcr_ctx* ctx)
{
    hipError_t first = hipSuccess;
    auto sync = [&](hipStream_t s) { const hipError_t e = s ? hipStreamSynchronize(s) : hipSuccess; if (first == hipSuccess) first = e; };
    for (const mcr_ctx::Lane& l : ctx->lanes) { sync(l.aux); sync(l.stream); }    // (aux is joined into the lane's stream in normal operation)
    sync(ctx->copy_stream);
    return first;
}

// Room in ctx->stage, the device copy of a host entry's arrays, for one buffer per byte count: ptr[i] is the i-th,
// 256-byte aligned like everything carved.
int stage_buffers(mcr_ctx* ctx, std::initializer_list<size_t> bytes, void** ptr)
{
    return carve(ctx, ctx->stage, [&](Carve& cv) { void** p = ptr; for (size_t b : bytes) *p++ = cv.take<char>(b); });
}

// Device z table of pooled length M (2M doubles), from the context's cache; filled on first use.
constexpr size_t kMaxZTabs = 24;
int get_ztab(mcr_ctx* ctx, i64 M, double** out)
{
    for (size_t k = 0; k < ctx->ztabs.size(); ++k)
        if (ctx->ztabs[k].M == M) {
            std::rotate(ctx->ztabs.begin(), ctx->ztabs.begin() + (long)k, ctx->ztabs.begin() + (long)k + 1);
            *out = ctx->ztabs[0].tab.as<double>();
            return MCR_OK;
        }
    if (ctx->ztabs.size() >= kMaxZTabs) {           // the evicted table may still be read by a call in flight
        sync_all(ctx);
        ctx->ztabs.pop_back();
    }
    mcr_ctx::ZTab z{M, DevBuf()};
    const int rc = z.tab.reserve(ctx, sizeof(double) * (size_t)(2 * M > 2 ? 2 * M : 2));
    if (rc) return rc;
    *out = z.tab.as<double>();
    hipLaunchKernelGGL(k_ztable, dim3((unsigned)((2 * M + 255) / 256)), dim3(256), 0, ctx->stream, *out, M);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // other lanes will read it: complete before anyone can
    if (e != hipSuccess) return fail(ctx, MCR_EHIP, "k_ztable failed: %s", hipGetErrorString(e));
    ctx->ztabs.insert(ctx->ztabs.begin(), std::move(z));
    return MCR_OK;
}

}  // namespace host
}  // namespace mcr

namespace {

// Twiddle table of a sub-transform length (at most 11 distinct lengths exist), from the context's cache.
int get_twiddles(mcr_ctx* ctx, int L, double2** out)
{
    for (const mcr_ctx::Twiddle& t : ctx->twiddles)
        if (t.L == L) { *out = t.tab.as<double2>(); return MCR_OK; }
    mcr_ctx::Twiddle t{L, DevBuf()};
    const int rc = t.tab.reserve(ctx, sizeof(double2) * (size_t)(L / 2 > 1 ? L / 2 : 1));
    if (rc) return rc;
    *out = t.tab.as<double2>();
    hipLaunchKernelGGL(fft::k_fft_twiddles, dim3((unsigned)((L / 2 + 255) / 256)), dim3(256), 0, ctx->stream, *out, L);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, MCR_EHIP, "k_fft_twiddles failed: %s", hipGetErrorString(e));
    ctx->twiddles.push_back(std::move(t));
    return MCR_OK;
}

// FFT tier of the ESS lags: chains of more than kFftMinN draws (and at most 2^21, so that N = 2^ceil(log2 2n) splits
// into two sub-transforms of at most 2048).  slots = listed pairs served per call (the rest take the direct rounds).
constexpr i64 kFftMinN = 16384;
constexpr int kFftChainBatch = 4;
FftPlan plan_fft(i64 n, int C, bool enabled)
{
    FftPlan f;
    if (!enabled || n <= kFftMinN || C < 2) return f;
    int lg = 1;
    while (((i64)1 << lg) < 2 * n) ++lg;
    if (lg > 22) return f;
    f.on = true; f.logN = lg; f.log1 = lg / 2; f.log2 = lg - f.log1;
    const i64 N = (i64)1 << lg;
    i64 slots = ((i64)1 << 23) / N;
    f.slots = (int)(slots < 2 ? 2 : (slots > 32 ? 32 : slots));
    f.cb = (C + 1) / 2 < kFftChainBatch ? (C + 1) / 2 : kFftChainBatch;     // transforms per batch: two chains share one
    return f;
}

int ensure_slot(mcr_ctx* ctx, Slot& s, size_t res_doubles, size_t off_entries)
{
    const size_t res = res_doubles * sizeof(double), off = off_entries * sizeof(i64);
    if (off > s.d_off.cap) s.off_C = s.off_N = -1;       // a new offset table holds no resident offsets
    int rc = s.d_res.reserve(ctx, res);
    if (!rc) rc = s.h_res.reserve(ctx, res);
    if (!rc) rc = s.d_off.reserve(ctx, off);
    return rc ? rc : s.h_off.reserve(ctx, off);
}

// Tiling of the sort of M pooled draws
struct WsPlan {
    i64 ntiles;
    // bucket path: the pooled array is cut into bk_k <= 16 sorted runs of length bk_R (a tile, or tiles
    // pre-merged by a few pairwise passes); #buckets, samples per bucket
    int bk_B = 0, bk_D = 0, bk_k = 0;
    i64 bk_R = 0;
};

WsPlan plan_ws(i64 M)
{
    WsPlan w;
    w.ntiles = (M + kTile - 1) / kTile;
    {
        i64 R = kTile;
        while ((M + R - 1) / R > kMaxBucketTiles) R *= 2;
        const i64 k = (M + R - 1) / R;
        if (k * (R / 64) <= 8192) {                           // the samples of one parameter must fit LDS
            const i64 last = M - (k - 1) * R;
            const i64 sf = (k - 1) * (R / 64) + last / 64;    // finite regular samples
            w.bk_R = R; w.bk_k = (int)k;
            w.bk_D = (int)((4096 - 64 - 79 * k) / 64);        // 64*D + 64*k + 15*k <= 4032: the top 64 slots are the kernel's scratch
            w.bk_B = (int)((sf + w.bk_D - 1) / w.bk_D);
            if (w.bk_B < 1) w.bk_B = 1;
        }
    }
    return w;
}

// The FFT tier's buffers: shared by all parameters of a call.
void carve_fft(Carve& cv, PipeIn& a, const FftPlan& fp)
{
    a.fft = fp;
    if (!fp.on) return;
    const size_t Nf = (size_t)1 << fp.logN;
    a.fft_A = cv.take<double2>((size_t)fp.slots * fp.cb * Nf);
    a.fft_S = cv.take<double>((size_t)fp.slots * Nf);
    a.fft_B = cv.take<double2>((size_t)fp.slots * Nf);
}

}  // namespace

// The pipeline as mcr_pipe.hpp declares it for mcr_stats.hip: this block and the next two of the namespace.
namespace mcr {
namespace host {

// The one layout of the pipeline's workspace: the buffers of a.pc parameters of a.M draws in a.C chains (the shortest
// a.n draws long, the segment grid over a.nstage).  Every entry point carves with it, and measures with it (null base)
// how much workspace it needs.  records = false: the sort alone, without rank codes and diagnostics records.  ingest:
// an f64 copy X[pc][M] of the draws at the end, returned.
double* carve_pipe(Carve& cv, PipeIn& a, bool records, const FftPlan& fp, bool ingest)
{
    const WsPlan wp = plan_ws(a.M);
    const size_t pc = (size_t)a.pc, M = (size_t)a.M;
    a.ntiles = wp.ntiles;
    a.idx16 = a.M <= kIdx16Max;
    a.bk_B = wp.bk_B; a.bk_D = wp.bk_D; a.bk_k = wp.bk_k; a.bk_R = wp.bk_R;
    a.kA = cv.take<double>(pc * M); a.kB = cv.take<double>(pc * M);
    a.iA = cv.take<u32>(pc * M);    a.iB = cv.take<u32>(pc * M);
    if (records) { a.zb = cv.take<u32>(pc * M); a.zt = cv.take<u32>(pc * M); }
    a.part = cv.take<double>(pc * wp.ntiles * kMomRec);
    if (records) {
        const size_t cc = (size_t)(a.C > 0 ? a.C : 1), ns = (size_t)((a.nstage + kSeg - 1) / kSeg + 1);
        a.split = cv.take<i64>(pc);
        a.rec = cv.take<double>(pc * 2 * cc * ns * kSegRec);
        a.rec2 = cv.take<double>(pc * 2 * cc * ns * 64 * kMoreBlocks);
        a.chstate = cv.take<double>(pc * 2 * cc * kChState);
        a.more = cv.take<unsigned>(pc * 2);
        a.state = cv.take<double>(pc * 2 * kPairState);
        a.acov = cv.take<double>(pc * 2 * (size_t)(a.n > 0 ? a.n : 1));
        a.long_count = cv.take<unsigned>(1);
        a.long_list = cv.take<unsigned>(pc * 2);
        a.t3c = cv.take<unsigned>(pc * 2 * (kT3Stages + 1));
    }
    a.samp = cv.take<double>(pc * (wp.ntiles + 16) * 64);
    a.cut = cv.take<u32>(pc * (wp.bk_B + 1) * (size_t)(wp.bk_k + 1));
    a.boff = cv.take<u32>(pc * (wp.bk_B + 1));
    carve_fft(cv, a, fp);
    return ingest ? cv.take<double>(pc * M) : nullptr;
}

}  // namespace host
}  // namespace mcr

namespace {

// One k_acov_seg pass of NT threads over SEG-draw segments: tier 1 (FIRST, every pair, lags 0..63, into a.rec) or tier 2
// (the pairs a.more flags, lags 64..255, into a.rec2).
template <int NT, int SEG, bool FIRST>
int launch_acov_seg(mcr_ctx* ctx, const PipeIn& a, int nseg, int kind_sel)
{
    const unsigned pk = (unsigned)((kind_sel < 0 ? 2 : 1) * a.pc);
    LAUNCH(ctx, FIRST ? K_ACOV_SEG : K_ACOV_MORE, (k_acov_seg<NT, SEG, FIRST>), dim3((unsigned)nseg, (unsigned)a.C, pk),
           dim3(NT), 0, (const u32*)a.zb, (const u32*)a.zt, (const double*)a.ztab, a.M, a.d_off, a.C, a.n, a.nh, nseg,
           FIRST ? (const unsigned*)nullptr : (const unsigned*)a.more, FIRST ? a.rec : a.rec2, kind_sel);
    return MCR_OK;
}

// Tiers 1 and 2 of one kind (0 bulk, 1 folded) or of both (kind_sel < 0): segment products, combine, the flagged pairs'
// lags 64..255 -- everything of the diagnostics that does not need the other kind.  On ctx->stream.
int launch_diag_front(mcr_ctx* ctx, const PipeIn& a, int kind_sel)
{
    // short chains (<= 1024 draws, e.g. the packaged corpus): half-size segments on 128-thread
    // workgroups, so twice as many of the latency-bound workgroups are resident per CU
    const bool small = a.nstage <= 1024;
    const int seg = small ? 1024 : kSeg;
    const int nseg = (int)((a.nstage + seg - 1) / seg);
    const unsigned ky = kind_sel < 0 ? 2u : 1u;
    int rc = small ? launch_acov_seg<128, 1024, true>(ctx, a, nseg, kind_sel) : launch_acov_seg<256, kSeg, true>(ctx, a, nseg, kind_sel);
    if (rc) return rc;
    LAUNCH(ctx, K_DIAG, k_diag_combine, dim3((unsigned)a.pc, ky), dim3(64u * (unsigned)(a.C < kCombineWaves ? a.C : kCombineWaves)), (size_t)6 * a.C * 8, (const u32*)a.zb,
           (const u32*)a.zt, (const double*)a.ztab, a.M, a.d_off, a.C, a.n, a.nh, nseg, (const double*)a.rec, a.d_res, a.pc, a.more, a.state, a.chstate,
           a.long_count, a.t3c,
           ctx->rho_band, ctx->guard_count.as<unsigned>(), kind_sel);
    // tier 2 for pairs whose first negative rho lies beyond lag 63 (others exit at once)
    return small ? launch_acov_seg<128, 1024, false>(ctx, a, nseg, kind_sel) : launch_acov_seg<256, kSeg, false>(ctx, a, nseg, kind_sel);
}

// Split R-hat + ESS (mcr_diag.hpp): the joint part -- tier 2's combine (+ finalize), tier 3.
int launch_diag(mcr_ctx* ctx, const PipeIn& a)
{
    const bool small = a.nstage <= 1024;
    const int seg = small ? 1024 : kSeg;
    const int nseg = (int)((a.nstage + seg - 1) / seg);
    const bool fused_tier3 = !a.fft.on && a.n <= 16384 && 2 * a.pc <= kTier3MaxPairs;     // k_tier3: one launch for the whole tier
    LAUNCH(ctx, K_DIAG2, k_diag_combine2, dim3((unsigned)a.pc, 2), dim3(1024), (size_t)2 * a.C * 8, (const u32*)a.zb,
           (const u32*)a.zt, (const double*)a.ztab, a.M, a.d_off, a.C,
           a.n, nseg, (const double*)a.rec2, (const unsigned*)a.more, a.state,
           a.chstate, a.d_res, a.pc, a.kA, a.kB,   // kA / kB: the sort's key buffers, free by now
           (const double*)a.part, (int)a.ntiles, fused_tier3 ? 0 : 1, ctx->rho_band, ctx->guard_count.as<unsigned>());
    if (a.n <= kLag2) return MCR_OK;       // chains short enough to be decided by lag 255 never reach tier 3
    if (fused_tier3) {
        // the common case in ONE launch: list, products of the lags [256, n) stage by stage, scans (k_tier3); a fixed number
        // of workgroups (kT3Workgroups) shares the (listed pair, lag group) items
        const i64 groups = (a.n - kLag2 + kLongGroup - 1) / kLongGroup;
        const i64 most = 2 * a.pc * groups;                                  // work items if every pair were listed
        const unsigned wgs = (unsigned)(most < (i64)kT3Workgroups ? most : (i64)kT3Workgroups);
        LAUNCH(ctx, K_ACOV_LONG, k_tier3, dim3(wgs), dim3(256), 0, (const double*)a.kA, (const double*)a.kB, a.M, a.d_off,
               a.C, a.n, (const unsigned*)a.more, a.state, a.acov, a.d_res, a.pc, ctx->rho_band, ctx->guard_count.as<unsigned>(), a.t3c,
               (const u32*)a.zb, (const u32*)a.zt, (const double*)a.ztab, a.chstate);
        return MCR_OK;
    }
    LAUNCH(ctx, K_DIAG2, k_long_list, dim3(1), dim3(1024), 0, (const unsigned*)a.more, (const double*)a.state, a.pc,
           a.long_count, a.long_list);
    {
        const unsigned slots = (unsigned)((2 * a.pc < 64) ? 2 * a.pc : 64);
        LAUNCH(ctx, K_DIAG2, k_dev_fill, dim3((unsigned)((a.M + 4095) / 4096), slots), dim3(256), 0, (const u32*)a.zb, (const u32*)a.zt,
               (const double*)a.ztab, a.M, a.d_off, a.C, a.n, (const double*)a.chstate, (const unsigned*)a.long_count,
               (const unsigned*)a.long_list, a.kA, a.kB);
    }
    // tier 3 for the pairs still undecided at lag 256.
    //  * chains of more than 16 384 draws: ALL lags of the first fft.slots listed pairs by FFT (mcr_fft.hpp);
    //  * everything else (and list entries beyond those slots): direct products over the whole chip, in rounds
    //    [256, 16384) -- one round, i.e. two near-empty launches, for chains up to 16 384 draws -- then growing 4x.
    unsigned slot_from = 0;
    if (a.fft.on) {
        const fft::Plan pl{a.fft.log1, a.fft.log2};
        const int N1 = 1 << pl.log1, N2 = 1 << pl.log2, cols = fft::kColElems >> pl.log1;
        const unsigned F = (unsigned)a.fft.slots;
        const size_t lds_cols = (size_t)fft::kColElems * 16, lds_rows = (size_t)N2 * 16;
        for (int c0 = 0; c0 < a.C; c0 += 2 * a.fft.cb) {          // a batch = fft.cb transforms = 2 fft.cb chains (two per transform)
            const int left = (a.C - c0 + 1) / 2;
            const int nb = (left < a.fft.cb) ? left : a.fft.cb;
            LAUNCH(ctx, K_FFT, (fft::k_fft_cols<256>), dim3((unsigned)(N2 / cols), (unsigned)nb, F), dim3(256), lds_cols,
                   (const double*)a.kA, (const double*)a.kB, a.M, a.d_off, c0, a.C, a.n, pl, (const double2*)a.tw1,
                   (const unsigned*)a.long_count, (const unsigned*)a.long_list, (const double*)a.state, a.fft_A, a.fft.cb);
            LAUNCH(ctx, K_FFT, (fft::k_fft_rows_power<256>), dim3((unsigned)N1, F), dim3(256), lds_rows, (const double2*)a.fft_A, pl,
                   (const double2*)a.tw2, (const unsigned*)a.long_count, (const unsigned*)a.long_list, (const double*)a.state,
                   a.fft_S, a.fft.cb, nb, c0 == 0 ? 1 : 0);
        }
        LAUNCH(ctx, K_FFT, (fft::k_fft_rows_spec<256>), dim3((unsigned)N1, F), dim3(256), lds_rows, (const double*)a.fft_S, pl,
               (const double2*)a.tw2, (const unsigned*)a.long_count, (const unsigned*)a.long_list, (const double*)a.state, a.fft_B);
        LAUNCH(ctx, K_FFT, (fft::k_fft_cols_out<256>), dim3((unsigned)(N2 / cols), F), dim3(256), lds_cols, (const double2*)a.fft_B, pl,
               (const double2*)a.tw1, a.n, (const unsigned*)a.long_count, (const unsigned*)a.long_list, (const double*)a.state,
               a.acov);
        slot_from = F;
    }
    const unsigned scan_slots = (unsigned)((2 * a.pc < 16) ? 2 * a.pc : 16);      // one light workgroup per listed pair at a time
    for (i64 L0 = kLag2; L0 < a.n;) {
        const i64 L1 = (L0 < 16384) ? 16384 : L0 * 4;
        const i64 lend = (L1 < a.n) ? L1 : a.n;
        const unsigned groups = (unsigned)((lend - L0 + kLongGroup - 1) / kLongGroup);
        unsigned slots = 256u / (groups ? groups : 1u);                             // ~256 workgroups when the round has few lag groups
        slots = slots < (unsigned)kLongSlots ? (unsigned)kLongSlots : (slots > 64u ? 64u : slots);
        if ((i64)slots > 2 * a.pc) slots = (unsigned)(2 * a.pc);
        LAUNCH(ctx, K_ACOV_LONG, (k_acov_long<256>), dim3(groups, slots), dim3(256), 0, (const double*)a.kA, (const double*)a.kB,
               a.M, a.d_off, a.C, a.n, L0, L1, (const unsigned*)a.long_count, (const unsigned*)a.long_list,
               (const double*)a.state, a.acov, slot_from);
        LAUNCH(ctx, K_DIAG_LONG, k_diag_long_scan, dim3(scan_slots), dim3(256), 0, a.C, a.n, L0, L1, (const unsigned*)a.long_count,
               (const unsigned*)a.long_list, a.state, a.acov, a.d_res, a.pc, (const u32*)a.zb, (const u32*)a.zt,
               (const double*)a.ztab, a.chstate, a.M, a.d_off, ctx->rho_band, ctx->guard_count.as<unsigned>());
        L0 = L1;
    }
    return MCR_OK;
}

// k_splitters for the runs in `keys`: few samples (S <= 1024) are ranked pair by pair, more by merging the runs' sample
// lists in the LDS (MVT outputs per thread and round: the smallest of 2, 4, 8 that holds S samples in 1024 MVT slots).
template <typename KT, int MVT>
int launch_splitters_v(mcr_ctx* ctx, const PipeIn& a, const KT* keys)
{
    const int S = a.bk_k * (int)(a.bk_R / 64);
    const size_t lds_spl = splitters_lds_bytes(S, a.bk_B, a.bk_k, MVT);
    if (lds_spl > 160 * 1024) return fail(ctx, MCR_ENOMEM, "k_splitters needs %zu bytes of LDS", lds_spl);
    if (lds_spl > 60 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_splitters<KT, MVT>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_spl));
    LAUNCH(ctx, K_SPLITTERS, (k_splitters<KT, MVT>), dim3((unsigned)a.pc), dim3(1024), lds_spl, keys, (const double*)a.samp,
           a.M, a.bk_k, a.bk_B, a.bk_D, a.bk_R, a.cut, a.boff);
    return MCR_OK;
}
template <typename KT>
int launch_splitters(mcr_ctx* ctx, const PipeIn& a, const KT* keys)
{
    const int S = a.bk_k * (int)(a.bk_R / 64);
    if (S <= 1024 || ctx->splitters_pairwise) return launch_splitters_v<KT, 0>(ctx, a, keys);
    if (S <= 2048) return launch_splitters_v<KT, 2>(ctx, a, keys);
    if (S <= 4096) return launch_splitters_v<KT, 4>(ctx, a, keys);
    return launch_splitters_v<KT, 8>(ctx, a, keys);       // (MVT must divide the runs' 64 j samples: a thread's outputs never straddle two pairs of runs)
}

// The tile sort of the stage: k_tile_sort for pairs (f64 draws, or f32 widened on load), k_tile_sort32 for f32 records.
template <class Slots>
int launch_tile_sort(mcr_ctx* ctx, const PipeIn& a, typename Slots::KeyT* keys, typename Slots::PosT* pos, double* samp)
{
    const dim3 grid((unsigned)a.ntiles, (unsigned)a.pc);
    if constexpr (std::is_same<Slots, RecSlots<u64>>::value) {
        LAUNCH(ctx, K_TILE_SORT, (k_tile_sort32<kTileNT, kTileVT>), grid, dim3(kTileNT), (size_t)kTile * 8,
               (const float*)a.X, a.M, keys, a.part, (int)a.ntiles, samp);
    } else if (a.x_f32) {
        LAUNCH(ctx, K_TILE_SORT, (k_tile_sort<kTileNT, kTileVT, typename Slots::PosT, float>), grid, dim3(kTileNT),
               Slots::lds_bytes(kTile), (const float*)a.X, a.M, keys, pos, a.part, (int)a.ntiles, samp,
               ctx->guard_count.as<unsigned>() + 1);
    } else {
        LAUNCH(ctx, K_TILE_SORT, (k_tile_sort<kTileNT, kTileVT, typename Slots::PosT, double>), grid, dim3(kTileNT),
               Slots::lds_bytes(kTile), (const double*)a.X, a.M, keys, pos, a.part, (int)a.ntiles, samp,
               ctx->guard_count.as<unsigned>() + 1);
    }
    return MCR_OK;
}

// Tile sort + (bucket partition | merge passes), on (f64 key, position) pairs in the key and position buffers, or -- f32
// tensors in the Arrow layout on the bucket path -- on packed records: those live in the f64 key buffers kA / kB (8 bytes
// per draw), and the position buffers travel along unused.
template <class Slots>
int sort_stage_t(mcr_ctx* ctx, PipeIn& a, Sorted& out)
{
    using KeyT = typename Slots::KeyT;
    using PosT = typename Slots::PosT;
    const i64 M = a.M, pc = a.pc;
    const unsigned py = (unsigned)pc;
    constexpr bool kRec = Slots::kTail > 0;
    constexpr size_t lds = Slots::lds_bytes(kTile);
    // (the z lookup table of this M comes from the context's cache: get_ztab)
    KeyT *kin = reinterpret_cast<KeyT*>(a.kA), *kout = reinterpret_cast<KeyT*>(a.kB);
    PosT *iin = (PosT*)a.iA, *iout = (PosT*)a.iB;
    // 1. tile sort (+ moment partials, + regular samples when a tile is already a run)
    const bool bucket = a.bk_B > 0;
    {
        const int rc = launch_tile_sort<Slots>(ctx, a, kin, iin, (bucket && a.bk_R == kTile) ? a.samp : (double*)nullptr);
        if (rc) return rc;
    }
    const unsigned nblk = (unsigned)((M + kTile - 1) / kTile);
    // 2. pairwise merge-path passes: up to the run length of the bucket partition, or all the way
    //    (two split points per workgroup: behind the pairs' slots, in static LDS next to the records')
    const i64 Rstop = bucket ? a.bk_R : M;
    for (i64 R = kTile; R < Rstop; R *= 2) {
        LAUNCH(ctx, K_MERGE, (k_merge<kMergeNT, kMergeVT, Slots>), dim3(nblk, py), dim3(kMergeNT), lds + (kRec ? 0 : 256),
               (const KeyT*)kin, (const PosT*)iin, kout, iout, M, R);
        std::swap(kin, kout);
        std::swap(iin, iout);
    }
    if (bucket) {
        // 3. exact k-way partition + in-LDS bucket merge, fused with ranks -> z
        if (a.bk_R != kTile)
            LAUNCH(ctx, K_SPLITTERS, k_sample_runs<KeyT>, dim3((unsigned)a.bk_k, py), dim3(256), 0, (const KeyT*)kin, M,
                   a.bk_R, a.samp);
        {
            const int rc = launch_splitters<KeyT>(ctx, a, (const KeyT*)kin);
            if (rc) return rc;
        }
        const unsigned pgrp = (unsigned)((pc + 7) / 8 * 8);   // XCD-aware 1-D grid (xcd_map)
        // (two kernels, see k_bucket_merge; the scratch: in the pairs' top 64 key slots, 512 bytes behind the records)
        u32* const zb = a.do_diag ? a.zb : (u32*)nullptr;
        if constexpr (kRec) {
            LAUNCH(ctx, K_BUCKET_MERGE, (k_bucket_merge32<kMergeNT, kMergeVT>), dim3(pgrp * (unsigned)a.bk_B), dim3(kMergeNT),
                   lds + 512, (const u64*)kin, kout, M, a.bk_k, a.bk_B, (const u32*)a.cut, (const u32*)a.boff, zb, pc, a.bk_R);
        } else {
            LAUNCH(ctx, K_BUCKET_MERGE, (k_bucket_merge<kMergeNT, kMergeVT, PosT>), dim3(pgrp * (unsigned)a.bk_B), dim3(kMergeNT),
                   lds, (const double*)kin, (const PosT*)iin, kout, iout, M, a.bk_k, a.bk_B, (const u32*)a.cut,
                   (const u32*)a.boff, zb, pc, a.bk_R);
        }
        std::swap(kin, kout);
        std::swap(iin, iout);
    }
    out = Sorted{reinterpret_cast<double*>(kin), iin, reinterpret_cast<double*>(kout), iout, bucket};
    return MCR_OK;
}

// Order statistics by the fold kernel's own workgroups (a launch less) while a parameter has few of them; a pooled
// array beyond 16-bit positions has a hundred fold workgroups per parameter, and one k_order_stats launch serves them.
inline bool order_stats_in_fold(const PipeIn& a) { return a.do_diag && a.idx16; }

// Fold: one merge of the two monotone halves around the median, fused with ranks -> z (and the order statistics).
// The records fold takes the LDS of the position width all the same.
template <typename IdxT>
int launch_fold(mcr_ctx* ctx, const PipeIn& a, const Sorted& s)
{
    const unsigned fgrid = (unsigned)((a.pc + 7) / 8 * 8) * (unsigned)((a.M + (kTile - 64) - 1) / (kTile - 64));   // 4032 outputs per fold workgroup
    const i64* split = order_stats_in_fold(a) ? (const i64*)nullptr : (const i64*)a.split;
    if (a.records) {
        LAUNCH(ctx, K_FOLD_MERGE, (k_fold_merge<kMergeNT, kMergeVT, IdxT, u64>), dim3(fgrid), dim3(kMergeNT),
               PairSlots<IdxT>::lds_bytes(kTile), (const u64*)s.keys, (const IdxT*)s.pos, (double*)nullptr, (IdxT*)nullptr, a.M,      // (positions unused: not null, the kernel offsets the pointer)
               (i64)0, a.d_res, a.pc, a.q, a.zt, split);
    } else {
        LAUNCH(ctx, K_FOLD_MERGE, (k_fold_merge<kMergeNT, kMergeVT, IdxT>), dim3(fgrid), dim3(kMergeNT),
               PairSlots<IdxT>::lds_bytes(kTile), (const double*)s.keys, (const IdxT*)s.pos, s.keys_free, (IdxT*)s.pos_free, a.M,
               (i64)0, a.d_res, a.pc, a.q, a.zt, split);
    }
    return MCR_OK;
}

// nt tensors in one launch (along z, at most kMaxGridY): tensor z starts z * ss elements into src, its copy z * xs into X.
// The summary and the tensor calls ingest ONE tensor per chunk (nt = 1, ss = xs = 0: the launch they always made); only
// mcr_sbc_ranks passes a batch, its chunk's simulations.
template <typename T>
int launch_ingest_as(mcr_ctx* ctx, const void* src, double* X, i64 C, i64 N, i64 pc, i64 sc, i64 sn, i64 sp, i64 p0, i64 nt, i64 ss, i64 xs)
{
    if (sp == 1 && sn != 1 && pc > 1) {
        const i64 nb = (N + 63) / 64;
        LAUNCH(ctx, K_INGEST, (k_ingest_transpose<T>), dim3((unsigned)(nb * C), (unsigned)((pc + 63) / 64), (unsigned)nt),
               dim3(256), 0, (const T*)src, X, C, N, pc, sc, sn, sp, p0, ss, xs);
    } else {
        const i64 nb = (N + 255) / 256;
        LAUNCH(ctx, K_INGEST, (k_ingest_rows<T>), dim3((unsigned)(nb * C), (unsigned)pc, (unsigned)nt), dim3(256), 0,
               (const T*)src, X, C, N, sc, sn, sp, p0, ss, xs);
    }
    return MCR_OK;
}

}  // namespace

// (mcr_pipe.hpp)
namespace mcr {
namespace host {

int sort_stage(mcr_ctx* ctx, PipeIn& a, Sorted& out)
{
    if (a.records) return sort_stage_t<RecSlots<u64>>(ctx, a, out);
    return a.idx16 ? sort_stage_t<PairSlots<unsigned short>>(ctx, a, out) : sort_stage_t<PairSlots<u32>>(ctx, a, out);
}

// The whole per-chunk pipeline on ctx->stream.  M >= 1, pc >= 1.  sorted_out (optional): what the sort stage left.
int run_pipeline(mcr_ctx* ctx, PipeIn& a, Sorted* sorted_out)
{
    const i64 M = a.M, pc = a.pc;
    const unsigned py = (unsigned)pc;
    a.q.xt = a.X; a.q.xf32 = a.x_f32 ? 1 : 0;      // the time order, for the sign of a median made of zero draws
    Sorted so;
    {
        const int rc = sort_stage(ctx, a, so);
        if (rc) return rc;
    }
    if (sorted_out) *sorted_out = so;
    // 3. order statistics: with diagnostics, by the fold kernel itself; a launch of their own for Backend.stats calls
    if (!order_stats_in_fold(a)) {
        if (a.records) {
            LAUNCH(ctx, K_ORDER_STATS, k_order_stats<u64>, dim3((unsigned)((pc + 3) / 4)), dim3(256), 0,
                   (const u64*)so.keys, M, pc, a.q, a.d_res, a.split);
        } else {
            LAUNCH(ctx, K_ORDER_STATS, k_order_stats<double>, dim3((unsigned)((pc + 3) / 4)), dim3(256), 0,
                   (const double*)so.keys, M, pc, a.q, a.d_res, a.split);
        }
    }
    if (a.do_diag) {
        // 4. bulk ranks -> z (already done by k_bucket_merge on the bucket path)
        if (!so.ranked)
            LAUNCH(ctx, K_RANK_Z, k_rank_z, dim3((unsigned)((M + 255) / 256), py), dim3(256), 0,
                   (const double*)so.keys, (const u32*)so.pos, M, a.zb);       // no bucket path only beyond 512 K draws: u32 positions
        // A LONE call (nothing else in flight on the context: what reference.compare makes) forks here: the bulk half of
        // tiers 1 and 2 needs only the bulk rank codes, which exist now, so it runs on the lane's second stream UNDER the fold
        // kernel, and the two halves join in front of combine2 -- ~35 us off the critical path of a 0.3 ms call.  A pipelined
        // caller keeps the single stream: its lanes are full anyway, and three more launches per call would only cost.
        const mcr_ctx::Lane& ln = ctx->lanes[ctx->lane];
        const bool fork = a.fork && a.C >= 2 && ln.aux != nullptr;
        hipStream_t main_stream = ctx->stream;
        if (fork) {
            HIP_TRY(ctx, hipEventRecord(ln.fork, main_stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ln.aux, ln.fork, 0));
            ctx->stream = ln.aux;
            const int rc = launch_diag_front(ctx, a, 0);
            ctx->stream = main_stream;
            if (rc) return rc;
            HIP_TRY(ctx, hipEventRecord(ln.join, ln.aux));
        }
        // 5+6. fold: one merge of the two monotone halves around the median, fused with ranks -> z
        {
            const int rc = a.idx16 ? launch_fold<unsigned short>(ctx, a, so) : launch_fold<u32>(ctx, a, so);
            if (rc) return rc;
        }
        // 7. R-hat + ESS (+ the finalize step, inside k_diag_combine2)
        if (a.C >= 2) {
            const int rc = launch_diag_front(ctx, a, fork ? 1 : -1);
            if (rc) return rc;
            if (fork) HIP_TRY(ctx, hipStreamWaitEvent(main_stream, ln.join, 0));
            return launch_diag(ctx, a);
        }
    }
    // 8. finalize (calls without diagnostics, single chains)
    LAUNCH(ctx, K_FINALIZE, k_finalize, dim3((unsigned)((pc + 63) / 64)), dim3(64), 0, (const double*)a.part,
           (int)a.ntiles, M, pc, (a.do_diag ? a.C : 0), a.d_res);
    return MCR_OK;
}

int launch_ingest(mcr_ctx* ctx, const void* src, int dtype, double* X, i64 C, i64 N, i64 pc, i64 sc, i64 sn, i64 sp, i64 p0, i64 nt,
                  i64 ss, i64 xs)
{
    return dtype == MCR_F64 ? launch_ingest_as<double>(ctx, src, X, C, N, pc, sc, sn, sp, p0, nt, ss, xs)
                            : launch_ingest_as<float>(ctx, src, X, C, N, pc, sc, sn, sp, p0, nt, ss, xs);
}

}  // namespace host
}  // namespace mcr

namespace {

int prep_quantiles(mcr_ctx* ctx, const double* qs, int nq, i64 M, QArgs& q, i64* qlo_out)
{
    if (nq < 0 || nq > MCR_MAX_QUANTILES) return fail(ctx, MCR_EINVAL, "n_q must be in [0, %d]; got %d", MCR_MAX_QUANTILES, nq);
    if (nq > 0 && !qs) return fail(ctx, MCR_EINVAL, "quantiles is NULL");
    q.nq = nq;
    for (int k = 0; k < nq; ++k) {
        if (!(qs[k] >= 0.0 && qs[k] <= 1.0)) return fail(ctx, MCR_EINVAL, "Quantiles must be in the range [0, 1]");
        const double h = (double)(M - 1) * qs[k];   // numpy: virtual index (n-1)*q ; arrow: same
        const double fl = std::floor(h);
        i64 lo = (i64)fl;
        if (lo < 0) lo = 0;
        if (M > 0 && lo > M - 1) lo = M - 1;
        q.lo[k] = lo;
        q.g[k] = h - fl;
        qlo_out[k] = lo;
    }
    return MCR_OK;
}

constexpr int res_fields(int nq) { return R_Q0 + nq; }

void fill_nan(const mcr_summary& o, i64 P, int nq)
{
    double* arrs[] = {o.mean, o.std, o.median, o.rhat, o.rhat_bulk, o.rhat_tail, o.ess_bulk, o.ess_tail};
    for (double* a : arrs)
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o.q) for (i64 i = 0; i < P * nq; ++i) o.q[i] = NAN;
    if (o.lag_bulk) for (i64 p = 0; p < P; ++p) o.lag_bulk[p] = 0;
    if (o.lag_tail) for (i64 p = 0; p < P; ++p) o.lag_tail[p] = 0;
}

// Copies slot results (already on the host) into the caller's arrays.  Returns MCR_ENONFINITE
// if any parameter saw NaN/Inf draws.
int unpack_slot(mcr_ctx* ctx, Slot& s)
{
    const mcr_summary& o = s.out;
    if (o.q_lo) for (int k = 0; k < s.nq; ++k) o.q_lo[k] = s.qlo[k];
    if (s.trivial_nan) { fill_nan(o, s.P, s.nq); return MCR_OK; }
    double nbad = 0.0;
    for (i64 p0 = 0; p0 < s.P; p0 += s.pcmax) {
        const i64 pc = s.P - p0 < s.pcmax ? s.P - p0 : s.pcmax;
        const double* r = s.h_res.as<double>() + (size_t)res_fields(s.nq) * (size_t)p0;
        auto cp = [&](double* dst, int field) {
            if (dst) memcpy(dst + p0, r + (size_t)field * pc, sizeof(double) * (size_t)pc);
        };
        cp(o.mean, R_MEAN); cp(o.std, R_STD); cp(o.median, R_MEDIAN); cp(o.rhat, R_RHAT);
        cp(o.rhat_bulk, R_RHAT_BULK); cp(o.rhat_tail, R_RHAT_TAIL); cp(o.ess_bulk, R_ESS_BULK);
        cp(o.ess_tail, R_ESS_TAIL);
        for (i64 p = 0; p < pc; ++p) {
            if (o.lag_bulk) o.lag_bulk[p0 + p] = (int64_t)r[(size_t)R_LAG_BULK * pc + p];
            if (o.lag_tail) o.lag_tail[p0 + p] = (int64_t)r[(size_t)R_LAG_TAIL * pc + p];
            nbad += r[(size_t)R_BAD * pc + p];
            if (o.q) for (int k = 0; k < s.nq; ++k) o.q[(p0 + p) * s.nq + k] = r[(size_t)(R_Q0 + k) * pc + p];
        }
    }
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

int check_common(mcr_ctx* ctx, const void* draws, int dtype, i64 C, i64 N, i64 P, int min_chains,
                 const mcr_summary* out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!out) return fail(ctx, MCR_EINVAL, "out is NULL");
    if (dtype != MCR_F64 && dtype != MCR_F32) return fail(ctx, MCR_EINVAL, "unsupported dtype %d", dtype);
    if (C < 0 || N < 0 || P < 0) return fail(ctx, MCR_EINVAL, "negative dimension (C=%lld N=%lld P=%lld)", C, N, P);
    if (min_chains < 1) return fail(ctx, MCR_EMINCHAINS_ARG, "min_chains must be >= 1; got %d", min_chains);
    if (C < min_chains)
        return fail(ctx, MCR_EMINCHAINS, "diagnostics require at least %d chains; got %lld chain(s)", min_chains, C);
    if (C > kMaxChains) return fail(ctx, MCR_EINVAL, "at most %d chains are supported; got %lld", kMaxChains, C);
    if (C * N >= (i64)0x7FFFFFFFll) return fail(ctx, MCR_EINVAL, "C*N must be < 2^31");   // 2M-1 rank codes in u32
    if (!draws && C * N * P > 0) return fail(ctx, MCR_EINVAL, "draws is NULL");
    return MCR_OK;
}

// How a call of this shape is cut into workspace chunks of parameters (a pure function of the shape, the workspace limit
// and MCR_FFT): shared by run_summary and mcr_plan_chunks.
struct ChunkPlan { bool ingest = false; FftPlan fp{}; i64 pcmax = 0; size_t bytes = 0; };

// The chain structure of a call as the kernels see it next to the offset table: C chains, M pooled draws, n = the
// shortest chain (what _ess walks, src/mcmc_ref/diagnostics.py:154-169), nh = the smallest half len / 2 over the chains
// of at least two draws (_split_chains, diagnostics.py:76-85; a chain of one draw contributes no halves), nstage = the
// longest chain prefix k_acov_seg reads (n, or second half start + nh).  Rectangular tensors are the case off[c] = c N.
struct ChainShape { i64 C = 0, M = 0, n = 0, nh = 0, nstage = 1; };
ChainShape shape_regular(i64 C, i64 N)
{
    ChainShape h;
    h.C = C; h.M = C * N; h.n = N; h.nh = (N >= 2) ? N / 2 : 0; h.nstage = N > 0 ? N : 1;
    return h;
}
ChainShape shape_offsets(const i64* off, i64 C)
{
    ChainShape h;
    h.C = C; h.M = C > 0 ? off[C] : 0;
    bool have_h = false;
    for (i64 c = 0; c < C; ++c) {
        const i64 len = off[c + 1] - off[c];
        if (c == 0 || len < h.n) h.n = len;
        if (len >= 2) { if (!have_h || len / 2 < h.nh) h.nh = len / 2; have_h = true; }
    }
    h.nstage = h.n > 0 ? h.n : 1;
    for (i64 c = 0; c < C; ++c) {
        const i64 len = off[c + 1] - off[c];
        if (len >= 2 && len / 2 + h.nh > h.nstage) h.nstage = len / 2 + h.nh;
    }
    return h;
}

// fft_slot_cap > 0: the FFT tier gets at most that many slots (a caller that knows how few pairs it can list).
int plan_chunks(mcr_ctx* ctx, const ChainShape& h, i64 P, bool ingest, bool do_diag, ChunkPlan& cp, int fft_slot_cap = 0)
{
    const i64 M = h.M, C = h.C;
    cp.ingest = ingest;
    cp.fp = plan_fft(h.n, (int)C, do_diag && ctx->fft_on);
    if (fft_slot_cap > 0 && cp.fp.slots > fft_slot_cap) cp.fp.slots = fft_slot_cap;
    auto fft_bytes = [&]() {
        PipeIn a{};
        Carve m{nullptr};
        carve_fft(m, a, cp.fp);
        return m.off;
    };
    auto measure = [&](i64 pc) {
        PipeIn a{};
        a.M = M; a.pc = pc; a.C = (int)C; a.n = h.n; a.nstage = h.nstage;
        Carve m{nullptr};
        carve_pipe(m, a, true, cp.fp, cp.ingest);
        return m.off;
    };
    // the FFT tier is an accelerator, not a requirement: under a tight workspace limit it gets fewer slots, or none
    // (the direct rounds then serve every listed pair), but at least a third of the limit stays with the parameters
    while (cp.fp.on && fft_bytes() > ctx->ws_limit / 3) {
        if (cp.fp.slots <= 1) { cp.fp = FftPlan{}; break; }
        cp.fp.slots /= 2;
    }
    // the most parameters whose layout fits the limit; k_acov_seg uses grid.z = 2 * pc
    cp.pcmax = most_that_fit(P < kMaxGridY / 2 ? P : kMaxGridY / 2, [&](i64 pc) { return measure(pc) <= ctx->ws_limit; });
    if (!cp.pcmax)
        return fail(ctx, MCR_ENOMEM, "one parameter needs %zu bytes of workspace (%zu of them for the FFT tier); limit is %zu",
                    measure(1), fft_bytes(), ctx->ws_limit);
    cp.bytes = measure(cp.pcmax);
    return MCR_OK;
}

// The call-wide tables of a pipeline, from the context's caches: the FFT tier's twiddles (fp.on), the z table (ztab).
int get_tables(mcr_ctx* ctx, PipeIn& a, const FftPlan& fp, bool ztab)
{
    int rc = fp.on ? get_twiddles(ctx, 1 << fp.log1, &a.tw1) : MCR_OK;
    if (!rc && fp.on) rc = get_twiddles(ctx, 1 << fp.log2, &a.tw2);
    return (!rc && ztab) ? get_ztab(ctx, a.M, &a.ztab) : rc;
}

// Acceptance of a chain offset table of C + 1 entries: it is there, starts at 0, never decreases, and the pooled length
// fits the rank codes (2M - 1 of them in u32).
int check_chain_table(mcr_ctx* ctx, const i64* chain_off, i64 C)
{
    if (C <= 0) return MCR_OK;
    if (!chain_off) return fail(ctx, MCR_EINVAL, "chain_off is NULL");
    if (chain_off[0] != 0) return fail(ctx, MCR_EINVAL, "chain_off[0] must be 0");
    for (i64 c = 0; c < C; ++c)
        if (chain_off[c + 1] < chain_off[c]) return fail(ctx, MCR_EINVAL, "chain_off must be non-decreasing");
    if (chain_off[C] >= (i64)0x7FFFFFFFll) return fail(ctx, MCR_EINVAL, "pooled length out of range");
    return MCR_OK;
}

// Acceptance of a ragged call: the codes mcr_diagnose_chains answers with.
int check_chains(mcr_ctx* ctx, const void* draws, const i64* chain_off, i64 C, i64 P, i64 sp, int min_chains,
                 const mcr_summary* out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!out) return fail(ctx, MCR_EINVAL, "out is NULL");
    if (C < 0 || P < 0) return fail(ctx, MCR_EINVAL, "negative dimension (C=%lld P=%lld)", (long long)C, (long long)P);
    if (min_chains < 1) return fail(ctx, MCR_EMINCHAINS_ARG, "min_chains must be >= 1; got %d", min_chains);
    if (C < min_chains)
        return fail(ctx, MCR_EMINCHAINS, "diagnostics require at least %d chains; got %lld chain(s)", min_chains, (long long)C);
    if (C > kMaxChains) return fail(ctx, MCR_EINVAL, "at most %d chains are supported; got %lld", kMaxChains, (long long)C);
    const int rc = check_chain_table(ctx, chain_off, C);
    if (rc) return rc;
    const i64 M = C > 0 ? chain_off[C] : 0;
    if (P > 1 && M > 0 && sp < M) return fail(ctx, MCR_EINVAL, "stride_p must be at least the pooled length");
    if (!draws && M * P > 0) return fail(ctx, MCR_EINVAL, "draws is NULL");
    return MCR_OK;
}

// An accepted call (the context's device is current): shape, quantiles, slot and lane, the chunk plan, the offset table,
// the chunks, the result copy, and the slot goes in flight.
int run_summary(mcr_ctx* ctx, const SummaryCall& c)
{
    const i64 C = c.C, N = c.N, P = c.P;
    const bool ragged = c.ragged;
    const ChainShape h = ragged ? shape_offsets(c.chain_off, C) : shape_regular(C, N);
    const i64 M = h.M;
    int si = c.slot;
    for (int k = 0; si < 0 && k < MCR_MAX_INFLIGHT; ++k) {
        const int f = (ctx->next_slot + k) % MCR_MAX_INFLIGHT;
        if (std::find(ctx->order.begin(), ctx->order.end(), f) == ctx->order.end()) si = f;
    }
    QArgs q;
    int rc = prep_quantiles(ctx, c.quantiles, c.nq, M, q, ctx->slots[si].qlo);
    if (rc) return rc;
    if (c.slot < 0) use_lane(ctx, si % ctx->n_lanes);
    Slot& s = ctx->slots[si];           // the call this slot serves
    s.out = *c.out; s.P = P; s.nq = c.nq; s.trivial_nan = (M == 0 || P == 0); s.pcmax = P;
    if (!s.trivial_nan) {
        const mcr_summary* out = c.out;
        const bool do_diag = c.always_diag || out->rhat || out->rhat_bulk || out->rhat_tail || out->ess_bulk ||
                             out->ess_tail || out->lag_bulk || out->lag_tail;
        // the ingest pass sees a ragged parameter as one row of M draws
        const i64 iC = ragged ? 1 : C, iN = ragged ? M : N, isc = ragged ? M : c.sc, isn = ragged ? 1 : c.sn;
        ChunkPlan cp;
        rc = plan_chunks(ctx, h, P, needs_ingest(iC, iN, P, isc, isn, c.sp), do_diag, cp, c.fft_slot_cap);
        if (rc) return rc;
        const i64 pcmax = s.pcmax = cp.pcmax;
        rc = lane_ws(ctx).reserve(ctx, cp.bytes);
        if (rc) return rc;
        const int R = res_fields(c.nq);
        rc = ensure_slot(ctx, s, (size_t)R * (size_t)P, (size_t)C + 1);
        if (rc) return rc;
        const bool off_resident = !ragged && s.off_C == C && s.off_N == N;
        if (ragged) {
            memcpy(s.h_off.p, c.chain_off, sizeof(i64) * (size_t)(C + 1));
            s.off_C = s.off_N = -1;
        } else if (!off_resident) {
            for (i64 k = 0; k <= C; ++k) s.h_off.as<i64>()[k] = k * N;
        }
        PipeIn call{};                  // the fields every chunk shares
        call.M = M; call.C = (int)C; call.d_off = s.d_off.as<i64>(); call.n = h.n; call.nh = h.nh; call.q = q;
        call.nstage = h.nstage; call.do_diag = do_diag;
        rc = get_tables(ctx, call, cp.fp, do_diag);
        if (rc) return rc;
        if (!off_resident)
            HIP_TRY(ctx, hipMemcpyAsync(s.d_off.p, s.h_off.p, sizeof(i64) * (size_t)(C + 1), hipMemcpyHostToDevice, ctx->stream));
        for (i64 p0 = 0; p0 < P; p0 += pcmax) {
            const i64 pc = (P - p0 < pcmax) ? P - p0 : pcmax;
            Carve cv{lane_ws(ctx).as<char>(), lane_ws(ctx).cap};
            PipeIn a = call;
            a.pc = pc;
            double* X = carve_pipe(cv, a, true, cp.fp, cp.ingest);
            if (cv.over()) return fail(ctx, MCR_ENOMEM, "workspace layout needs %zu bytes; the workspace has %zu", cv.off, cv.end);
            // (the per-kernel event pairs of the profiling mode keep the single stream)
            a.fork = c.may_fork && ctx->fork_lone && ctx->order.empty() && !ctx->prof && P <= pcmax &&
                     (double)M * (double)pc >= 2e6 && (double)M * (double)pc <= 8e6;    // kernels long enough to be worth
                                               // three more launches and two event waits (measured: C1 4 M param-draws 306 -> 288 us,
                                               // 10 x 1000 x 45 149 -> 166, 4 x 1000 x 10 124 -> 133), short enough not to fill the chip
            if (cp.ingest) {
                rc = launch_ingest(ctx, c.draws_dev, c.dtype, X, iC, iN, pc, isc, isn, c.sp, p0);      // (one tensor: z = 1)
                if (rc) return rc;
                a.X = X;
            } else {
                a.x_f32 = c.dtype == MCR_F32;
                a.records = a.x_f32 && a.bk_B > 0 && ctx->f32_records;
                a.X = a.x_f32 ? (const void*)(reinterpret_cast<const float*>(c.draws_dev) + p0 * M)
                              : (const void*)(reinterpret_cast<const double*>(c.draws_dev) + p0 * M);
            }
            a.d_res = s.d_res.as<double>() + (size_t)R * (size_t)p0;
            rc = run_pipeline(ctx, a);
            if (rc) return rc;
            if (c.last) *c.last = a;
        }
        HIP_TRY(ctx, hipMemcpyAsync(s.h_res.p, s.d_res.p, sizeof(double) * (size_t)R * (size_t)P, hipMemcpyDeviceToHost,
                                    ctx->stream));
    }
    if (!s.trivial_nan && !ragged) { s.off_C = C; s.off_N = N; }
    // the slot's completion event behind the call's work on its lane: the slot is in flight
    if (!s.done) HIP_TRY(ctx, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(s.done, ctx->stream));
    ctx->order.push_back(si);
    if (c.slot < 0) ctx->next_slot = (si + 1) % MCR_MAX_INFLIGHT;
    return MCR_OK;
}

// Waits for a slot's completion event.  The host polls the event for a while before it blocks in the runtime: a blocking
// wait is woken through an interrupt and the scheduler, which costs a lone synchronous call (what reference.compare makes,
// src/mcmc_ref/reference.py:107-122) some 20 - 40 us on top of its 0.3 ms; a pipelined caller seldom waits at all.
int wait_event(mcr_ctx* ctx, hipEvent_t ev)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return MCR_OK;
        if (q != hipErrorNotReady) return fail(ctx, MCR_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        if ((spin & 63) == 63 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2e-3) break;
    }
    HIP_TRY(ctx, hipEventSynchronize(ev));
    return MCR_OK;
}

int wait_impl(mcr_ctx* ctx)
{
    // every slot in flight records its event behind its last copy on its lane: waiting for the events (polled, see
    // wait_event) leaves every lane idle; the stream synchronisations below then return at once
    for (int si : ctx->order) { const int rc = wait_event(ctx, ctx->slots[si].done); if (rc) return rc; }
    for (const mcr_ctx::Lane& l : ctx->lanes) if (l.stream) HIP_TRY(ctx, hipStreamSynchronize(l.stream));
    use_lane(ctx, 0);
    prof_resolve(ctx);
    int rc = MCR_OK;
    for (int si : ctx->order) { const int r = unpack_slot(ctx, ctx->slots[si]); if (r && !rc) rc = r; }
    ctx->order.clear();
    return rc;
}

// Drops any enqueued-but-unwaited work after an error so the ctx stays usable.
void abort_inflight(mcr_ctx* ctx)
{
    sync_all(ctx);
    use_lane(ctx, 0);
    prof_resolve(ctx);
    ctx->order.clear();
}

}  // namespace

// The summary path as mcr_host.hpp declares it (mcr_summarize_files of mcr_files.hip enqueues on it).
namespace mcr {
namespace host {

// A summary call on a free slot and the next lane: acceptance, then the shared path.
int enqueue_impl(mcr_ctx* ctx, const SummaryCall& c)
{
    const int rc = c.ragged ? check_chains(ctx, c.draws_dev, c.chain_off, c.C, c.P, c.sp, c.min_chains, c.out)
                            : check_common(ctx, c.draws_dev, c.dtype, c.C, c.N, c.P, c.min_chains, c.out);
    if (rc) return rc;
    if (ctx->order.size() >= MCR_MAX_INFLIGHT) return fail(ctx, MCR_EINVAL, "more than %d summaries in flight", MCR_MAX_INFLIGHT);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return run_summary(ctx, c);
}

// Waits for the OLDEST outstanding enqueue only and delivers its results; the others keep running.
int wait_one_impl(mcr_ctx* ctx)
{
    if (ctx->order.empty()) return MCR_OK;
    Slot& s = ctx->slots[ctx->order.front()];
    { const int rc = wait_event(ctx, s.done); if (rc) return rc; }
    const int rc = unpack_slot(ctx, s);
    ctx->order.erase(ctx->order.begin());
    return rc;
}

// Ends a call that enqueued summaries: delivers everything in flight (or, abort, drops it) and returns the first error,
// rc with its message before the outcome of the wait.
int drain(mcr_ctx* ctx, int rc, bool abort)
{
    char keep[sizeof ctx->err];
    memcpy(keep, ctx->err, sizeof keep);
    const int rw = abort ? (abort_inflight(ctx), MCR_OK) : wait_impl(ctx);
    if (rc) memcpy(ctx->err, keep, sizeof keep);
    return rc ? rc : rw;
}

// The results of parameter p0 on: every array of o shifted by p0 parameters (q by p0 * nq quantiles).
mcr_summary summary_at(mcr_summary r, i64 p0, int nq)
{
    for (double** a : {&r.mean, &r.std, &r.median, &r.rhat, &r.rhat_bulk, &r.rhat_tail, &r.ess_bulk, &r.ess_tail})
        if (*a) *a += p0;
    for (int64_t** a : {&r.lag_bulk, &r.lag_tail})
        if (*a) *a += p0;
    if (r.q) r.q += p0 * nq;
    return r;
}

}  // namespace host
}  // namespace mcr

namespace {

template <typename T>
int moments_impl(mcr_ctx* ctx, const T* src, i64 C, i64 N, i64 P, i64 sc, i64 sn, i64 sp, double* d_mean,
                 double* d_std, double* part, int S, bool rows)
{
    const i64 M = C * N;
    if (rows) {
        LAUNCH(ctx, K_MOMENTS, (k_moments_rows<T>), dim3((unsigned)S, (unsigned)P), dim3(256), 0, src, M, sp, part, S);
    } else {
        LAUNCH(ctx, K_MOMENTS, (k_moments_cols<T>), dim3((unsigned)((P + 63) / 64), (unsigned)S), dim3(256), 0, src,
               C, N, P, sc, sn, sp, part, S);
    }
    LAUNCH(ctx, K_MOMENTS_FINAL, k_moments_final, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
           (const double*)part, S, P, d_mean, d_std, (double*)nullptr);
    return MCR_OK;
}

}  // namespace

// (mcr_pipe.hpp)
namespace mcr {
namespace host {

// k_moments_rows and the finisher on f64 rows X[P][M] (mcr_covariance's means): the moments kernels stay in this unit.
int moments_rows(mcr_ctx* ctx, const double* src, i64 M, i64 P, double* d_mean, double* d_std, double* part, int S)
{
    return moments_impl<double>(ctx, src, 1, M, P, M, 1, M, d_mean, d_std, part, S, true);
}

// The host entries of the two-sample calls: ref [P][Mr] and act [P][Ma] uploaded side by side into ctx->stage.
int stage_two_samples(mcr_ctx* ctx, const double* ref, i64 Mr, const double* act, i64 Ma, i64 P, const double** ref_dev,
                      const double** act_dev)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t br = sizeof(double) * (size_t)P * Mr, ba = sizeof(double) * (size_t)P * Ma;
    void* X[2];
    const int rc = stage_buffers(ctx, {br, ba}, X);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(X[0], ref, br, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(X[1], act, ba, hipMemcpyHostToDevice, ctx->stream));
    *ref_dev = (const double*)X[0];
    *act_dev = (const double*)X[1];
    return MCR_OK;
}

}  // namespace host
}  // namespace mcr

// =================================================================================================
extern "C" {

int mcr_version(void) { return MCR_VERSION; }

int mcr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* mcr_last_error(const mcr_ctx* ctx) { return ctx ? ctx->err : g_init_err; }

int mcr_init(int device, mcr_ctx** out)
{
    if (!out) return fail(nullptr, MCR_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, MCR_ENODEVICE, "no HIP device available (%s); libmcmcref_hip has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= n) return fail(nullptr, MCR_ENODEVICE, "device %d out of range [0, %d)", device, n);
    mcr_ctx* ctx = new (std::nothrow) mcr_ctx();
    if (!ctx) return fail(nullptr, MCR_ENOMEM, "out of host memory");
    ctx->device = device;
    ctx->rho_band = kRhoBand;
    ctx->energy_launch_work = MCR_ENERGY_LAUNCH_WORK;
    if (const char* env = getenv("MCR_LANES")) {
        const int v = atoi(env);
        ctx->n_lanes = v < 1 ? 1 : (v > MCR_MAX_INFLIGHT ? MCR_MAX_INFLIGHT : v);
    }
    if (const char* env = getenv("MCR_IO_PIECE_KB")) {
        const long v = atol(env);
        ctx->io_piece = (size_t)(v < 64 ? 64 : (v > (1 << 20) ? (1 << 20) : v)) << 10;
    }
    if (const char* env = getenv("MCR_IO_THREADS")) {
        const int v = atoi(env);
        ctx->io_threads = v < 1 ? 1 : (v > 64 ? 64 : v);
    }
    e = hipSetDevice(device);
    for (int l = 0; l < ctx->n_lanes && e == hipSuccess; ++l)
        e = hipStreamCreateWithFlags(&ctx->lanes[l].stream, hipStreamNonBlocking);
    for (int l = 0; l < ctx->n_lanes && e == hipSuccess; ++l) {
        e = hipStreamCreateWithFlags(&ctx->lanes[l].aux, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->lanes[l].fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->lanes[l].join, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        mcr_free(ctx);
        return fail(nullptr, MCR_EHIP, "device %d init failed: %s", device, hipGetErrorString(e));
    }
    use_lane(ctx, 0);
    size_t mb = 8192;
    if (const char* env = getenv("MCR_WORKSPACE_MB")) { const long v = atol(env); if (v > 0) mb = (size_t)v; }
    ctx->ws_limit = mb << 20;
    if (const char* env = getenv("MCR_F32_RECORDS")) ctx->f32_records = atoi(env) != 0;
    if (const char* env = getenv("MCR_FFT")) ctx->fft_on = atoi(env) != 0;
    if (const char* env = getenv("MCR_SPLITTERS_PAIRWISE")) ctx->splitters_pairwise = atoi(env) != 0;
    if (const char* env = getenv("MCR_FORK")) ctx->fork_lone = atoi(env) != 0;
    if (const char* env = getenv("MCR_ENERGY_LAUNCH_WORK")) { const long long v = atoll(env); if (v > 0 && v <= MCR_ENERGY_LAUNCH_WORK) ctx->energy_launch_work = v; }
    if (const char* env = getenv("MCR_RHO_BAND")) { const double v = atof(env); if (v >= 0.0 && v < 1.0) ctx->rho_band = v; }
    if (ctx->guard_count.reserve(ctx, 2 * sizeof(unsigned)) != MCR_OK ||
        hipMemsetAsync(ctx->guard_count.p, 0, 2 * sizeof(unsigned), ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        mcr_free(ctx);
        return fail(nullptr, MCR_ENOMEM, "device %d: cannot allocate the guard counter", device);
    }
    *out = ctx;
    return MCR_OK;
}

void mcr_free(mcr_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    sync_all(ctx);
    prof_resolve(ctx);
    // what no member owns: the event pool, the slots' completion events, the copy stream; the rest goes with the members
    for (hipEvent_t e : ctx->free_ev) hipEventDestroy(e);
    for (Slot& s : ctx->slots) if (s.done) hipEventDestroy(s.done);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    delete ctx;
}

int mcr_rho_guard_count(mcr_ctx* ctx, int64_t* rederived)
{
    if (!ctx || !rederived) return fail(ctx, MCR_EINVAL, "NULL argument");
    hipSetDevice(ctx->device);
    sync_all(ctx);
    unsigned v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, ctx->guard_count.p, sizeof(unsigned), hipMemcpyDeviceToHost));
    *rederived = (int64_t)v;
    return MCR_OK;
}

int mcr_tile_fallback_count(mcr_ctx* ctx, int64_t* tiles)
{
    if (!ctx || !tiles) return fail(ctx, MCR_EINVAL, "NULL argument");
    hipSetDevice(ctx->device);
    sync_all(ctx);
    unsigned v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, ctx->guard_count.as<unsigned>() + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
    *tiles = (int64_t)v;
    return MCR_OK;
}

int mcr_set_workspace_limit(mcr_ctx* ctx, size_t bytes)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (bytes < (1u << 20)) return fail(ctx, MCR_EINVAL, "workspace limit must be at least 1 MiB");
    ctx->ws_limit = bytes;
    return MCR_OK;
}

int mcr_plan_chunks(mcr_ctx* ctx, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp, int diagnostics,
                    int64_t* params_per_chunk)
{
    if (!ctx || !params_per_chunk) return fail(ctx, MCR_EINVAL, "mcr_plan_chunks: NULL argument");
    if (C <= 0 || N <= 0 || P <= 0) { *params_per_chunk = 0; return MCR_OK; }
    ChunkPlan cp;
    const int rc = plan_chunks(ctx, shape_regular(C, N), P, needs_ingest(C, N, P, sc, sn, sp), diagnostics != 0, cp);
    if (rc) return rc;
    *params_per_chunk = cp.pcmax;
    return MCR_OK;
}

int mcr_dev_alloc(mcr_ctx* ctx, size_t bytes, void** dptr)
{
    if (!ctx || !dptr) return fail(ctx, MCR_EINVAL, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : 1));
    return MCR_OK;
}
int mcr_dev_free(mcr_ctx* ctx, void* dptr)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (dptr) HIP_TRY(ctx, hipFree(dptr));
    return MCR_OK;
}
int mcr_memcpy_h2d(mcr_ctx* ctx, void* dptr, const void* hptr, size_t bytes)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCR_OK;
}
int mcr_memcpy_d2h(mcr_ctx* ctx, void* hptr, const void* dptr, size_t bytes)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCR_OK;
}
int mcr_sync(mcr_ctx* ctx)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    for (const mcr_ctx::Lane& l : ctx->lanes) if (l.stream) HIP_TRY(ctx, hipStreamSynchronize(l.stream));
    return MCR_OK;
}

int mcr_summarize_enqueue(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P,
                          int64_t sc, int64_t sn, int64_t sp, int min_chains, const double* quantiles, int n_q,
                          mcr_summary* out)
{
    const int rc = enqueue_impl(ctx, SummaryCall{draws_dev, dtype, C, N, P, sc, sn, sp, nullptr, false, min_chains, quantiles, n_q, out});
    if (rc && ctx && rc != MCR_EMINCHAINS && rc != MCR_EMINCHAINS_ARG && rc != MCR_EINVAL) return drain(ctx, rc, true);
    return rc;
}

int mcr_summarize_chains_enqueue(mcr_ctx* ctx, const double* draws_dev, int64_t stride_p, const int64_t* chain_off, int C,
                                 int64_t P, int min_chains, const double* quantiles, int n_q, mcr_summary* out)
{
    const int rc = enqueue_impl(ctx, SummaryCall{draws_dev, MCR_F64, C, 0, P, 0, 1, stride_p, reinterpret_cast<const i64*>(chain_off),
                                                 true, min_chains, quantiles, n_q, out});
    if (rc && ctx && rc != MCR_EMINCHAINS && rc != MCR_EMINCHAINS_ARG && rc != MCR_EINVAL) return drain(ctx, rc, true);
    return rc;
}

int mcr_summarize_chains_dev(mcr_ctx* ctx, const double* draws_dev, int64_t stride_p, const int64_t* chain_off, int C,
                             int64_t P, int min_chains, const double* quantiles, int n_q, mcr_summary* out)
{
    const int rc = mcr_summarize_chains_enqueue(ctx, draws_dev, stride_p, chain_off, C, P, min_chains, quantiles, n_q, out);
    if (rc) return rc;
    return wait_impl(ctx);
}

int mcr_plan_chunks_chains(mcr_ctx* ctx, const int64_t* chain_off, int C, int64_t P, int diagnostics,
                           int64_t* params_per_chunk)
{
    if (!ctx || !params_per_chunk) return fail(ctx, MCR_EINVAL, "mcr_plan_chunks_chains: NULL argument");
    if (C < 0 || C > kMaxChains) return fail(ctx, MCR_EINVAL, "mcr_plan_chunks_chains: bad chain count %d", C);
    const i64* off = reinterpret_cast<const i64*>(chain_off);
    int rc = check_chain_table(ctx, off, C);
    if (rc) return rc;
    if (C == 0 || P <= 0 || off[C] == 0) { *params_per_chunk = 0; return MCR_OK; }
    ChunkPlan cp;
    rc = plan_chunks(ctx, shape_offsets(off, C), P, false, diagnostics != 0, cp);
    if (rc) return rc;
    *params_per_chunk = cp.pcmax;
    return MCR_OK;
}

int mcr_summarize_wait(mcr_ctx* ctx)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    return wait_impl(ctx);
}

int mcr_summarize_wait_one(mcr_ctx* ctx)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    return wait_one_impl(ctx);
}

int mcr_summarize_models(mcr_ctx* ctx, const mcr_model_desc* models, int n_models, const double* quantiles,
                         int n_q, mcr_summary* outs)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (n_models < 0 || (n_models > 0 && (!models || !outs))) return fail(ctx, MCR_EINVAL, "bad argument");
    int rc = MCR_OK;
    for (int i = 0; i < n_models && !rc; ++i) {
        if (ctx->order.size() >= MCR_MAX_INFLIGHT) rc = wait_one_impl(ctx);
        if (rc) break;
        const mcr_model_desc& m = models[i];
        rc = mcr_summarize_enqueue(ctx, m.draws_dev, m.dtype, m.C, m.N, m.P, m.stride_c, m.stride_n, m.stride_p,
                                   m.min_chains, quantiles, n_q, &outs[i]);
    }
    return drain(ctx, rc);                  // deliver everything that was enqueued
}

int mcr_summarize_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                      int64_t sn, int64_t sp, int min_chains, const double* quantiles, int n_q, mcr_summary* out)
{
    int rc = mcr_summarize_enqueue(ctx, draws_dev, dtype, C, N, P, sc, sn, sp, min_chains, quantiles, n_q, out);
    if (rc) return rc;
    return wait_impl(ctx);
}

int mcr_summarize(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                  int64_t sn, int64_t sp, int min_chains, const double* quantiles, int n_q, mcr_summary* out)
{
    int rc = check_common(ctx, draws, dtype, C, N, P, min_chains, out);
    if (rc) return rc;
    const i64 ext = tensor_extent(C, N, P, sc, sn, sp);
    if (ext < 0) return fail(ctx, MCR_EINVAL, "negative strides are not supported");
    const size_t es = dtype == MCR_F64 ? 8 : 4;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* X = ctx->stage.p;
    if (ext > 0) {
        rc = stage_buffers(ctx, {(size_t)ext * es}, &X);
        if (rc) return rc;
    }
    // Parameter-major tensors (the Arrow column layout) of some size go up in a few pieces: while piece k + 1
    // crosses PCIe on the copy stream, the kernels of piece k already run on a lane (pageable host memory makes
    // the copy itself synchronous for the host, which has nothing better to do).
    const i64 per_param = tensor_extent(C, N, 1, sc, sn, 0);
    const bool separable = P >= 2 && C * N > 0 && sp >= per_param && ctx->order.empty() && ctx->n_lanes > 1;
    if (separable && (size_t)ext * es >= ((size_t)8 << 20)) {
        int pieces = ctx->n_lanes < 4 ? ctx->n_lanes : 4;
        if ((i64)pieces > P) pieces = (int)P;
        for (int k = 0; k < pieces && !rc; ++k) {
            const i64 p0 = P * k / pieces, p1 = P * (k + 1) / pieces, pc = p1 - p0;
            const size_t b0 = (size_t)p0 * (size_t)sp * es;
            const size_t bytes = (size_t)tensor_extent(C, N, pc, sc, sn, sp) * es;
            hipError_t e = hipMemcpyAsync((char*)X + b0, (const char*)draws + b0, bytes, hipMemcpyHostToDevice, ctx->copy_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_stream);
            if (e != hipSuccess) { rc = fail(ctx, MCR_EHIP, "upload failed: %s", hipGetErrorString(e)); break; }
            mcr_summary o = summary_at(*out, p0, n_q > 0 ? n_q : 0);
            rc = mcr_summarize_enqueue(ctx, (char*)X + b0, dtype, C, N, pc, sc, sn, sp, min_chains, quantiles, n_q, &o);
        }
        return drain(ctx, rc);
    }
    if (ext > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(X, draws, (size_t)ext * es, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the pipeline may run on the other lane
    }
    return mcr_summarize_dev(ctx, X, dtype, C, N, P, sc, sn, sp, min_chains, quantiles, n_q, out);
}

int mcr_diagnose_chains(mcr_ctx* ctx, const double* pooled, const int64_t* chain_off, int C, int min_chains,
                        mcr_summary* out, double* z_bulk, double* z_tail, double* rank_bulk, double* rank_tail)
{
    const i64* off = reinterpret_cast<const i64*>(chain_off);
    int rc = check_chains(ctx, pooled, off, C, 1, 0, min_chains, out);
    if (rc) return rc;
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_diagnose_chains with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const i64 M = C > 0 ? off[C] : 0;
    const size_t row = sizeof(double) * (size_t)M;
    double* const dst[4] = {z_bulk, z_tail, rank_bulk, rank_tail};
    const bool want_dbg = M > 0 && (z_bulk || z_tail || rank_bulk || rank_tail);
    void* d[5] = {};                    // the draws; z_bulk, z_tail, rank_bulk, rank_tail (decoded codes)
    if (M > 0) {
        rc = want_dbg ? stage_buffers(ctx, {row, row, row, row, row}, d) : stage_buffers(ctx, {row}, d);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d[0], pooled, row, hipMemcpyHostToDevice, ctx->stream));
    }
    // one parameter of the ragged path, consumed where it lies: slot 0 on the current lane, diagnostics whatever `out`
    // holds, and two (parameter, kind) pairs at most for the FFT tier
    PipeIn a{};
    SummaryCall c{d[0], MCR_F64, C, 0, 1, 0, 1, M, off, true, min_chains, nullptr, 0, out};
    c.slot = 0; c.always_diag = true; c.may_fork = false; c.fft_slot_cap = 2; c.last = &a;
    rc = run_summary(ctx, c);
    if (!rc && want_dbg) {
        auto decode = [&]() {
            const unsigned nb = (unsigned)((M + 255) / 256);
            auto dev = [&](int i) { return dst[i] ? (double*)d[1 + i] : (double*)nullptr; };
            hipLaunchKernelGGL(k_decode_codes, dim3(nb), dim3(256), 0, ctx->stream, (const u32*)a.zb, (const double*)a.ztab, M, dev(0), dev(2));
            hipLaunchKernelGGL(k_decode_codes, dim3(nb), dim3(256), 0, ctx->stream, (const u32*)a.zt, (const double*)a.ztab, M, dev(1), dev(3));
            HIP_TRY(ctx, hipGetLastError());
            for (int i = 0; i < 4; ++i)
                if (dst[i]) HIP_TRY(ctx, hipMemcpyAsync(dst[i], d[1 + i], row, hipMemcpyDeviceToHost, ctx->stream));
            return (int)MCR_OK;
        };
        rc = decode();
    }
    return drain(ctx, rc, rc != MCR_OK);
}

int mcr_moments_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                    int64_t sn, int64_t sp, double* mean, double* std)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (dtype != MCR_F64 && dtype != MCR_F32) return fail(ctx, MCR_EINVAL, "unsupported dtype %d", dtype);
    if (C < 0 || N < 0 || P < 0 || !mean || !std) return fail(ctx, MCR_EINVAL, "bad argument");
    const i64 M = C * N;
    if (P == 0) return MCR_OK;
    if (M == 0) { for (i64 p = 0; p < P; ++p) mean[p] = std[p] = NAN; return MCR_OK; }
    if (!draws_dev) return fail(ctx, MCR_EINVAL, "draws is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool rows = (N <= 1 || sn == 1) && (C <= 1 || sc == N);
    if (rows && P > kMaxGridY) return fail(ctx, MCR_EINVAL, "P > %d not supported by mcr_moments_dev rows path", kMaxGridY);
    int S;
    if (rows) {
        const i64 vec = dtype == MCR_F64 ? 2 : 4;
        i64 smax = (M + 256 * vec * 4 - 1) / (256 * vec * 4);   // >= one unrolled sweep per block
        i64 want = (4096 + P - 1) / P;
        S = (int)(want < smax ? want : smax);
        if (S < 1) S = 1;
    } else {
        i64 want = (2048 + (P + 63) / 64 - 1) / ((P + 63) / 64);
        i64 smax = (M + 63) / 64;
        S = (int)(want < smax ? want : smax);
        if (S < 1) S = 1;
        if (S > kMaxGridY) S = kMaxGridY;
    }
    double *part, *d_mean, *d_std;
    int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) {
        part = cv.take<double>((size_t)P * S * kMomRec);
        d_mean = cv.take<double>((size_t)P);
        d_std = cv.take<double>((size_t)P);
    });
    if (rc) return rc;
    rc = dtype == MCR_F64 ? moments_impl<double>(ctx, (const double*)draws_dev, C, N, P, sc, sn, sp, d_mean, d_std, part, S, rows)
                          : moments_impl<float>(ctx, (const float*)draws_dev, C, N, P, sc, sn, sp, d_mean, d_std, part, S, rows);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(mean, d_mean, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(std, d_std, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcr_basic_stats(mcr_ctx* ctx, const void* values, int dtype, int64_t n, double* mean, double* std)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!mean || !std || n < 0) return fail(ctx, MCR_EINVAL, "bad argument");
    if (dtype != MCR_F64 && dtype != MCR_F32) return fail(ctx, MCR_EINVAL, "unsupported dtype %d", dtype);
    if (n == 0) { *mean = NAN; *std = NAN; return MCR_OK; }   /* compare.py:60-61 */
    if (!values) return fail(ctx, MCR_EINVAL, "values is NULL");
    const size_t es = dtype == MCR_F64 ? 8 : 4;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* X = nullptr;
    const int rc = stage_buffers(ctx, {(size_t)n * es}, &X);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(X, values, (size_t)n * es, hipMemcpyHostToDevice, ctx->stream));
    return mcr_moments_dev(ctx, X, dtype, 1, n, 1, n, 1, n, mean, std);
}

int mcr_compare(mcr_ctx* ctx, const double* ref, const double* actual, int64_t n, double tol, double* rel_error,
                uint8_t* passed)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (n < 0 || (n > 0 && (!ref || !actual || !rel_error || !passed))) return fail(ctx, MCR_EINVAL, "bad argument");
    if (n == 0) return MCR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *d_ref, *d_act, *d_rel;
    unsigned char* d_ok;
    const int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) {
        d_ref = cv.take<double>((size_t)n);
        d_act = cv.take<double>((size_t)n);
        d_rel = cv.take<double>((size_t)n);
        d_ok = cv.take<unsigned char>((size_t)n);
    });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_ref, ref, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_act, actual, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, K_COMPARE, k_compare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const double*)d_ref,
           (const double*)d_act, (i64)n, tol, d_rel, d_ok);
    HIP_TRY(ctx, hipMemcpyAsync(rel_error, d_rel, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(passed, d_ok, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcr_profile_enable(mcr_ctx* ctx, int on)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    ctx->prof = on != 0;
    return MCR_OK;
}
int mcr_profile_reset(mcr_ctx* ctx)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    for (int k = 0; k < K_COUNT; ++k) { ctx->k_launches[k] = 0; ctx->k_ms[k] = 0.0; }
    return MCR_OK;
}
int mcr_profile_get(mcr_ctx* ctx, mcr_kernel_time* out, int max, int* n)
{
    if (!ctx || !n) return fail(ctx, MCR_EINVAL, "NULL argument");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    int cnt = 0;
    for (int k = 0; k < K_COUNT; ++k) {
        if (!ctx->k_launches[k]) continue;
        if (out && cnt < max) {
            memset(&out[cnt], 0, sizeof(mcr_kernel_time));
            strncpy(out[cnt].name, kKernelNames[k], sizeof(out[cnt].name) - 1);
            out[cnt].launches = ctx->k_launches[k];
            out[cnt].total_ms = ctx->k_ms[k];
        }
        ++cnt;
    }
    *n = cnt;
    return MCR_OK;
}

int mcr_hbm_probe(mcr_ctx* ctx, size_t bytes, int iters, double* read_gbps, double* copy_gbps)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (bytes < ((size_t)1 << 20) || iters < 1 || (!read_gbps && !copy_gbps)) return fail(ctx, MCR_EINVAL, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bytes &= ~(size_t)4095;
    DevBuf src, dst;
    int rc = src.reserve(ctx, bytes);
    if (!rc) rc = dst.reserve(ctx, copy_gbps ? bytes : 4096 * 4);
    if (rc) return rc;
    void *const a = src.p, *const b = dst.p;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipStream_t st = ctx->stream;
    auto best_of = [&](auto&& launch) -> double {
        float best = 1e30f;
        launch();                                                  // warm-up (page faults, clocks)
        for (int k = 0; k < iters; ++k) {
            hipEventRecord(e0, st); launch(); hipEventRecord(e1, st);
            hipEventSynchronize(e1);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.f && ms < best) best = ms;
        }
        return (double)best;
    };
    if (hipMemsetAsync(a, 0x5A, bytes, st) != hipSuccess) rc = fail(ctx, MCR_EHIP, "memset failed");
    if (!rc && read_gbps) {
        const i64 nvec = (i64)(bytes / 16);
        double ms = 1e30;
        for (unsigned grid : {2048u, 4096u, 8192u, 16384u, 32768u}) {
            const double t = best_of([&] { hipLaunchKernelGGL(k_stream_read, dim3(grid), dim3(256), 0, st, (const uint4*)a, nvec, (u32*)b); });
            if (t < ms) ms = t;
        }
        *read_gbps = (double)bytes / (ms * 1e-3) / 1e9;
    }
    if (!rc && copy_gbps) {
        const double ms = best_of([&] { hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, st); });
        *copy_gbps = 2.0 * (double)bytes / (ms * 1e-3) / 1e9;     // bytes read + bytes written
    }
    hipStreamSynchronize(st);
    if (hipGetLastError() != hipSuccess && !rc) rc = fail(ctx, MCR_EHIP, "probe launch failed");
    hipEventDestroy(e0); hipEventDestroy(e1);
    return rc;
}

int mcr_fill_synthetic_at(mcr_ctx* ctx, void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t p0, uint64_t seed)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (dtype != MCR_F64 && dtype != MCR_F32) return fail(ctx, MCR_EINVAL, "unsupported dtype %d", dtype);
    if (C < 0 || N < 0 || P < 0 || p0 < 0) return fail(ctx, MCR_EINVAL, "negative dimension");
    const i64 total = C * N * P;
    if (total <= 0) return MCR_OK;
    if (!draws_dev) return fail(ctx, MCR_EINVAL, "draws is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    i64 blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    const i64 first = p0 * C * N;       // element index of the block's first draw in the whole tensor
    if (dtype == MCR_F64) {
        LAUNCH(ctx, K_FILL, (k_fill_synth<double>), dim3((unsigned)blocks), dim3(256), 0, (double*)draws_dev, total,
               (i64)(C * N), (u64)seed, first);
    } else {
        LAUNCH(ctx, K_FILL, (k_fill_synth<float>), dim3((unsigned)blocks), dim3(256), 0, (float*)draws_dev, total,
               (i64)(C * N), (u64)seed, first);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcr_fill_synthetic(mcr_ctx* ctx, void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, uint64_t seed)
{
    return mcr_fill_synthetic_at(ctx, draws_dev, dtype, C, N, P, 0, seed);
}

}  // extern "C"
