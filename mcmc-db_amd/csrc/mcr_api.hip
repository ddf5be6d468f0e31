// mcr_api.hip -- the statistics unit of libmcmcref_hip.so's C ABI (see include/mcmcref_hip.h): the context's life, the
// summary pipeline and every statistics entry, with their host-side launch logic: workspace carving, parameter chunking,
// async result slots, HIP-event profiling.  The file and text entries are mcr_files.hip, the communicator mcr_comm.hip;
// mcr_host.hpp is what the three share.  Plain HIP runtime only: no torch, no hipify, no compatibility layers.
#include "mcr_host.hpp"

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
#include "mcr_ext.hpp"
#include "mcr_energy.hpp"
#include "mcr_nested.hpp"
#include "mcr_acf.hpp"
#include "mcr_pareto.hpp"
#include "mcr_psis.hpp"
#include "mcr_hdi.hpp"
#include "mcr_weighted.hpp"
#include "mcr_sbc.hpp"

using namespace mcr;
using namespace mcr::host;

namespace {

constexpr int kTile = 4096;          // pooled draws per sorted tile / bucket capacity
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

// What mcr_host.hpp declares for every unit and this one defines.
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

}  // namespace host
}  // namespace mcr

namespace {

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
struct FftPlan { bool on = false; int logN = 0, log1 = 0, log2 = 0, slots = 0, cb = 0; };
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

}  // namespace

// (mcr_host.hpp names the type, for SummaryCall::last)
struct mcr::host::PipeIn {
    const void* X;       // [pc][M] contiguous: f64 (user tensor or ingest buffer) or, x_f32, the user's f32 tensor itself
    bool x_f32 = false;
    // f32 tensors take the packed records (k_tile_sort32, RecSlots<u64>) whenever the bucket partition applies (pooled arrays up to
    // 512 K draws) and MCR_F32_RECORDS is not 0; otherwise the tile sort widens the f32 draws and the f64 kernels run
    bool records = false;
    bool idx16 = false;  // M <= kIdx16Max: 16-bit positions through the sort (else 32-bit)
    i64 M, pc;
    int C;
    const i64* d_off;
    i64 n, nh;
    QArgs q;
    double* d_res;       // chunk's result table, stride pc
    // carved buffers
    double *kA, *kB, *part;
    u32 *zb, *zt;        // rank codes n2 of every draw in time order (z = ztab[n2], rank = (n2 + 1) / 2)
    void *iA, *iB;       // pooled-position payload of the sort: u16 when idx16, else u32
    i64* split;
    double* rec;         // [pc][2][C][nseg][kSegRec] first-pass segment records
    unsigned* more;      // [pc][2] continuation flags
    double* state;       // [pc][2][4] rho scan state
    double* chstate;     // [pc][2][C][kChState]
    double* rec2;        // [pc][2][C][nseg][64*kMoreBlocks] lag products of tier 2 (lags 64..255)
    double* acov;        // [pc][2][n] deviation products of tier 3 (lags >= 256), listed pairs only
    unsigned* long_count; // [1] number of pairs in the tier-3 list of this call
    unsigned* long_list;  // [2 pc]
    unsigned* t3c;        // [kT3Stages + 1][2 pc] k_tier3: per pair and stage the finished lag groups (+ kT3Prev), then "decided"
    FftPlan fft;          // FFT tier for long chains (mcr_fft.hpp): buffers shared by the chunks of a call
    double2 *fft_A = nullptr, *fft_B = nullptr; double* fft_S = nullptr;
    double2 *tw1 = nullptr, *tw2 = nullptr;
    i64 nstage;          // longest chain prefix the segment grid has to cover
    double* ztab;        // [2M] z of every possible tie run (shared by all parameters of the call)
    double* samp;        // [pc][ntiles][64] regular samples of the sorted tiles
    u32* cut;            // [pc][B+1][ntiles]
    u32* boff;           // [pc][B+1]
    int bk_B = 0, bk_D = 0, bk_k = 0;
    i64 bk_R = 0;
    i64 ntiles;
    bool do_diag = true;  // false: Backend.stats only (sort + order statistics + moments)
    bool fork = false;    // lone call: the bulk half of the diagnostics on the lane's second stream (run_pipeline)
};

namespace {

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

// What the sort stage leaves: the ascending (key, position) order of every parameter in one of the two ping-pong buffer
// pairs, the other pair free, and whether the bulk rank codes z_bulk are written already (bucket path with do_diag).
// On the f32 records path the keys are packed (key, position) records and the positions are unused: pos / pos_free are then
// the two position buffers in no particular order (which is which depends on the number of merge passes), nothing may read them.
struct Sorted {
    double* keys; void* pos;
    double* keys_free; void* pos_free;
    bool ranked;
};

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

int sort_stage(mcr_ctx* ctx, PipeIn& a, Sorted& out)
{
    if (a.records) return sort_stage_t<RecSlots<u64>>(ctx, a, out);
    return a.idx16 ? sort_stage_t<PairSlots<unsigned short>>(ctx, a, out) : sort_stage_t<PairSlots<u32>>(ctx, a, out);
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

// The whole per-chunk pipeline on ctx->stream.  M >= 1, pc >= 1.  sorted_out (optional): what the sort stage left.
int run_pipeline(mcr_ctx* ctx, PipeIn& a, Sorted* sorted_out = nullptr)
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
int launch_ingest(mcr_ctx* ctx, const void* src, int dtype, double* X, i64 C, i64 N, i64 pc, i64 sc, i64 sn, i64 sp, i64 p0, i64 nt = 1,
                  i64 ss = 0, i64 xs = 0)
{
    return dtype == MCR_F64 ? launch_ingest_as<double>(ctx, src, X, C, N, pc, sc, sn, sp, p0, nt, ss, xs)
                            : launch_ingest_as<float>(ctx, src, X, C, N, pc, sc, sn, sp, p0, nt, ss, xs);
}

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

// Tensors in the Arrow column layout [P][C][N] are consumed in place, f64 and f32 alike (the tile sort widens f32 as it
// loads); anything else goes through one ingest pass into X[P][M] f64.
inline bool needs_ingest(i64 C, i64 N, i64 P, i64 sc, i64 sn, i64 sp)
{
    return !((N <= 1 || sn == 1) && (C <= 1 || sc == N) && (P <= 1 || sp == C * N));
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

// Extent (in elements) touched by a strided tensor, or -1 if strides are negative.
i64 tensor_extent(i64 C, i64 N, i64 P, i64 sc, i64 sn, i64 sp)
{
    if (C == 0 || N == 0 || P == 0) return 0;
    if (sc < 0 || sn < 0 || sp < 0) return -1;
    return (C - 1) * sc + (N - 1) * sn + (P - 1) * sp + 1;
}

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

}  // namespace

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
    ctx->energy_launch_work = kEnLaunchWork;
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
    if (const char* env = getenv("MCR_ENERGY_LAUNCH_WORK")) { const long long v = atoll(env); if (v > 0 && v <= kEnLaunchWork) ctx->energy_launch_work = v; }
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

// The workspace of a two-sample pass over P rows: the two samples, the parked sorted reference, the merge partials, the
// results, the non-finite counts, then the two sorts one after the other in the same space.
struct TwoSampleWs {
    double *Xr, *Xa, *Sr, *part, *d_ks, *d_w, *bad;
    PipeIn ar{}, aa{};
    int nblk;
};

static void carve_two_sample(Carve& cv, TwoSampleWs& t, i64 P, i64 Mr, i64 Ma)
{
    t.nblk = (int)((Mr + Ma + kTile - 1) / kTile);
    t.ar.M = Mr; t.aa.M = Ma;
    t.ar.pc = t.aa.pc = P; t.ar.C = t.aa.C = 1; t.ar.do_diag = t.aa.do_diag = false;
    t.Xr = cv.take<double>((size_t)P * Mr);
    t.Xa = cv.take<double>((size_t)P * Ma);
    t.Sr = cv.take<double>((size_t)P * Mr);
    t.part = cv.take<double>((size_t)P * t.nblk * 2);
    t.d_ks = cv.take<double>((size_t)P);
    t.d_w = cv.take<double>((size_t)P);
    t.bad = cv.take<double>((size_t)P * 2);
    const size_t base = cv.off;
    carve_pipe(cv, t.ar, false, FftPlan{}, false);
    const size_t end_r = cv.off;
    cv.off = base;
    carve_pipe(cv, t.aa, false, FftPlan{}, false);
    if (end_r > cv.off) cv.off = end_r;
}

// From the rows t.Xr [P][Mr], t.Xa [P][Ma] on the device to ks[P], w1[P] on the host: the two sorts, the non-finite
// counts, one merge-path pass, the finisher and the non-finite check (`what` names the rows in its message).  Synchronous.
static int two_sample_tail(mcr_ctx* ctx, TwoSampleWs& t, i64 P, double* ks, double* w1, const char* what)
{
    const i64 Mr = t.ar.M, Ma = t.aa.M;
    const int nblk = t.nblk;
    Sorted so;
    t.ar.X = t.Xr;                // ascending order of the reference sample, parked in Sr
    int rc = sort_stage(ctx, t.ar, so);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(t.Sr, so.keys, sizeof(double) * (size_t)P * Mr, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_bad_count, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.ar.part,
                       (int)t.ar.ntiles, (i64)P, t.bad);
    t.aa.X = t.Xa;                // ascending order of the actual sample, then one merge-path pass over both
    rc = sort_stage(ctx, t.aa, so);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bad_count, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (const double*)t.aa.part,
                       (int)t.aa.ntiles, (i64)P, t.bad + P);
    LAUNCH(ctx, K_TWO_SAMPLE, (k_two_sample<256, 16>), dim3((unsigned)nblk, (unsigned)P), dim3(256), 0,
           (const double*)t.Sr, (i64)Mr, (const double*)so.keys, (i64)Ma, t.part, nblk);
    LAUNCH(ctx, K_TWO_SAMPLE, k_two_sample_final, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
           (const double*)t.part, nblk, (i64)P, (double)Mr * (double)Ma, t.d_ks, t.d_w);
    HIP_TRY(ctx, hipMemcpyAsync(ks, t.d_ks, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w1, t.d_w, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> h_bad((size_t)2 * (size_t)P);
    HIP_TRY(ctx, hipMemcpyAsync(h_bad.data(), t.bad, sizeof(double) * h_bad.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    for (i64 p = 0; p < P; ++p)
        if (h_bad[(size_t)p] != 0.0 || h_bad[(size_t)(P + p)] != 0.0 || !(ks[p] == ks[p]) || !(w1[p] == w1[p]) || std::isinf(w1[p]))
            return fail(ctx, MCR_ENONFINITE, "%s contain non-finite values", what);
    return MCR_OK;
}

// The length limits of a two-sample pass (positions are 32-bit; the KS numerator must stay exact in f64).
static bool two_sample_too_long(i64 Mr, i64 Ma)
{
    return Mr >= (i64)0xFFFFFFFFll || Ma >= (i64)0xFFFFFFFFll || (double)Mr * (double)Ma >= 9007199254740992.0;
}

int mcr_two_sample(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                   double* ks, double* w1)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || Mr < 1 || Ma < 1 || (P > 0 && (!ref || !act || !ks || !w1)))
        return fail(ctx, MCR_EINVAL, "bad argument (both samples need at least one draw)");
    if (P == 0) return MCR_OK;
    if (P > kMaxGridY) return fail(ctx, MCR_EINVAL, "P > %d", kMaxGridY);
    if (two_sample_too_long(Mr, Ma)) return fail(ctx, MCR_EINVAL, "samples too long (Mr * Ma must stay below 2^53)");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_two_sample with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TwoSampleWs t;
    const int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_two_sample(cv, t, P, Mr, Ma); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(t.Xr, ref, sizeof(double) * (size_t)P * Mr, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(t.Xa, act, sizeof(double) * (size_t)P * Ma, hipMemcpyHostToDevice, ctx->stream));
    return two_sample_tail(ctx, t, P, ks, w1, "draws");
}

// One k_project launch: Z[K][M] = W[K][P] (X[P][M] - c[P]).  The 16-byte instance when every row of X and Z starts
// 16-byte aligned; both instances give the same bits.
static int launch_project(mcr_ctx* ctx, const double* X, const double* W, const double* c, i64 M, i64 P, i64 K, double* Z)
{
    const i64 mtiles = ((M + kProjTileM - 1) / kProjTileM + 7) / 8 * 8, ktiles = (K + kProjTileK - 1) / kProjTileK;
    if (mtiles * ktiles > 0x7FFFFFFFll) return fail(ctx, MCR_EINVAL, "too many draws x directions for one projection launch");
    const dim3 grid((unsigned)(mtiles * ktiles));
    if ((M & 1) == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Z)) & 15) == 0)
        LAUNCH(ctx, K_PROJECT, (k_project<true>), grid, dim3(kProjNT), 0, X, W, c, M, P, K, Z);
    else
        LAUNCH(ctx, K_PROJECT, (k_project<false>), grid, dim3(kProjNT), 0, X, W, c, M, P, K, Z);
    return MCR_OK;
}

// The workspace of kc directions of a sliced call: the two-sample workspace over kc rows (its Xr / Xa are the
// projections), the chunk's directions and the center.
struct SlicedWs { TwoSampleWs t; double *W, *c; };

static void carve_sliced(Carve& cv, SlicedWs& s, i64 kc, i64 Mr, i64 Ma, i64 P)
{
    carve_two_sample(cv, s.t, kc, Mr, Ma);
    s.W = cv.take<double>((size_t)kc * P);
    s.c = cv.take<double>((size_t)P);
}

// Directions per workspace chunk: the most whose workspace fits the limit (all K when they fit at once).
static int plan_sliced(mcr_ctx* ctx, i64 Mr, i64 Ma, i64 P, i64 K, i64& kc)
{
    auto measure = [&](i64 k) { Carve m{nullptr}; SlicedWs s; carve_sliced(m, s, k, Mr, Ma, P); return m.off; };
    const i64 Mmax = Mr > Ma ? Mr : Ma;                // k_project's one-dimensional grid: draw tiles x direction tiles < 2^31
    const i64 grid_cap = 0x7FFFFFFFll / (((Mmax + kProjTileM - 1) / kProjTileM + 7) / 8 * 8) * kProjTileK;
    if (K > grid_cap) K = grid_cap;
    kc = most_that_fit(K, [&](i64 k) { return measure(k) <= ctx->ws_limit; });
    if (!kc)
        return fail(ctx, MCR_ENOMEM, "workspace limit too small: one direction needs %zu bytes, the limit is %zu", measure(1),
                    ctx->ws_limit);
    return MCR_OK;
}

static int sliced_check(mcr_ctx* ctx, const void* ref, i64 Mr, const void* act, i64 Ma, i64 P, const double* dirs,
                 const double* center, i64 K, const double* ks, const double* w1)
{
    if (K < 0 || Mr < 1 || Ma < 1 || (K > 0 && (P < 1 || !ref || !act || !dirs || !ks || !w1)))
        return fail(ctx, MCR_EINVAL, "bad argument (both samples need at least one draw and one parameter)");
    if (K == 0) return MCR_OK;
    if (K > kMaxGridY) return fail(ctx, MCR_EINVAL, "K > %d", kMaxGridY);
    if (two_sample_too_long(Mr, Ma)) return fail(ctx, MCR_EINVAL, "samples too long (Mr * Ma must stay below 2^53)");
    for (i64 i = 0; i < K * P; ++i)
        if (!std::isfinite(dirs[i])) return fail(ctx, MCR_EINVAL, "direction %lld has a non-finite weight", (long long)(i / P));
    for (i64 p = 0; center && p < P; ++p)
        if (!std::isfinite(center[p])) return fail(ctx, MCR_EINVAL, "center[%lld] is not finite", (long long)p);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_sliced_two_sample with summaries in flight");
    return MCR_OK;
}

static_assert(kProjTileM == MCR_PROJ_TILE_M && kProjTileK == MCR_PROJ_TILE_K && kProjChunkP == MCR_PROJ_CHUNK_P,
              "mcmcref_hip.h states k_project's geometry");

int mcr_sliced_plan(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, int64_t K, int64_t* dirs_per_chunk)
{
    if (!ctx || !dirs_per_chunk) return fail(ctx, MCR_EINVAL, "mcr_sliced_plan: NULL argument");
    if (Mr < 1 || Ma < 1 || P < 1 || K < 1 || K > kMaxGridY) { *dirs_per_chunk = 0; return MCR_OK; }
    i64 kc = 0;
    const int rc = plan_sliced(ctx, Mr, Ma, P, K, kc);
    if (rc) return rc;
    *dirs_per_chunk = kc;
    return MCR_OK;
}

int mcr_sliced_two_sample_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                              const double* dirs, const double* center, int64_t K, double* ks, double* w1,
                              double* proj_ref, double* proj_act)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = sliced_check(ctx, ref_dev, Mr, act_dev, Ma, P, dirs, center, K, ks, w1);
    if (rc || K == 0) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    i64 kcmax = 0;
    rc = plan_sliced(ctx, Mr, Ma, P, K, kcmax);
    if (rc) return rc;
    const std::vector<double> zeros(center ? 0 : (size_t)P, 0.0);
    for (i64 k0 = 0; k0 < K; k0 += kcmax) {            // the directions are independent: chunking changes no bit
        const i64 kc = K - k0 < kcmax ? K - k0 : kcmax;
        SlicedWs s;
        rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_sliced(cv, s, kc, Mr, Ma, P); });
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(s.W, dirs + k0 * P, sizeof(double) * (size_t)kc * P, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(s.c, center ? center : zeros.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice,
                                    ctx->stream));
        rc = launch_project(ctx, ref_dev, s.W, s.c, Mr, P, kc, s.t.Xr);
        if (!rc) rc = launch_project(ctx, act_dev, s.W, s.c, Ma, P, kc, s.t.Xa);
        if (rc) return rc;
        if (proj_ref)
            HIP_TRY(ctx, hipMemcpyAsync(proj_ref + k0 * Mr, s.t.Xr, sizeof(double) * (size_t)kc * Mr, hipMemcpyDeviceToHost, ctx->stream));
        if (proj_act)
            HIP_TRY(ctx, hipMemcpyAsync(proj_act + k0 * Ma, s.t.Xa, sizeof(double) * (size_t)kc * Ma, hipMemcpyDeviceToHost, ctx->stream));
        rc = two_sample_tail(ctx, s.t, kc, ks + k0, w1 + k0, "draws or their projections");
        if (rc) return rc;
    }
    return MCR_OK;
}

int mcr_sliced_two_sample(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                          const double* dirs, const double* center, int64_t K, double* ks, double* w1,
                          double* proj_ref, double* proj_act)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = sliced_check(ctx, ref, Mr, act, Ma, P, dirs, center, K, ks, w1);
    if (rc || K == 0) return rc;
    const double *Xr, *Xa;
    rc = stage_two_samples(ctx, ref, Mr, act, Ma, P, &Xr, &Xa);
    if (rc) return rc;
    return mcr_sliced_two_sample_dev(ctx, Xr, Mr, Xa, Ma, P, dirs, center, K, ks, w1, proj_ref, proj_act);
}

// ---- energy distance (mcr_energy.hpp) ---------------------------------------------------------------------------------
static_assert(kEnTI == MCR_ENERGY_TILE_I && kEnTJ == MCR_ENERGY_TILE_J && kEnPC == MCR_ENERGY_CHUNK_P &&
              kEnMaxWork == MCR_ENERGY_MAX_WORK && kEnLaunchWork == MCR_ENERGY_LAUNCH_WORK,
              "mcmcref_hip.h states k_energy_pairs' geometry and the work limits");

// The workspace of a call: one partial per tile job, the scales, the results (six outputs + the three sums).
struct EnergyWs { double *part, *scale, *res; };

static void carve_energy(Carve& cv, EnergyWs& w, const EnergyJobs& jb, i64 P)
{
    w.part = cv.take<double>((size_t)jb.total());
    w.scale = cv.take<double>((size_t)P);
    w.res = cv.take<double>(9);
}

// The shape of a call: MCR_EINVAL with the cause, else MCR_OK.
static int energy_shape_check(mcr_ctx* ctx, i64 Mr, i64 Ma, i64 P)
{
    if (Mr < 1 || Ma < 1) return fail(ctx, MCR_EINVAL, "mcr_energy_distance: both samples need at least one draw (Mr = %lld, Ma = %lld)", Mr, Ma);
    if (P < 1) return fail(ctx, MCR_EINVAL, "mcr_energy_distance: P = %lld, at least one parameter is needed", P);
    if (!energy_work_ok(Mr, Ma, P))
        return fail(ctx, MCR_EINVAL, "mcr_energy_distance: (Mr Ma + Mr (Mr + 1) / 2 + Ma (Ma + 1) / 2) P is over the work limit "
                    "MCR_ENERGY_MAX_WORK = %lld pair-parameters (Mr = %lld, Ma = %lld, P = %lld): thin the samples", kEnMaxWork, Mr, Ma, P);
    return MCR_OK;
}

static int energy_check(mcr_ctx* ctx, const void* ref, i64 Mr, const void* act, i64 Ma, i64 P, const double* scale, const double* out)
{
    if (!ref || !act || !out) return fail(ctx, MCR_EINVAL, "mcr_energy_distance: NULL argument (%s)", !ref ? "ref" : !act ? "act" : "out");
    const int rc = energy_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    for (i64 p = 0; scale && p < P; ++p)
        if (!(scale[p] >= 0.0) || std::isinf(scale[p]))
            return fail(ctx, MCR_EINVAL, "mcr_energy_distance: scale[%lld] is negative or not finite", (long long)p);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_energy_distance with summaries in flight");
    return MCR_OK;
}

int mcr_energy_workspace(mcr_ctx* ctx, int64_t Mr, int64_t Ma, int64_t P, size_t* bytes)
{
    if (!ctx || !bytes) return fail(ctx, MCR_EINVAL, "mcr_energy_workspace: NULL argument");
    const int rc = energy_shape_check(ctx, Mr, Ma, P);
    if (rc) return rc;
    Carve m{nullptr};
    EnergyWs w;
    carve_energy(m, w, energy_jobs(Mr, Ma), P);
    *bytes = m.off;
    return MCR_OK;
}

int mcr_energy_distance_dev(mcr_ctx* ctx, const double* ref_dev, int64_t Mr, const double* act_dev, int64_t Ma, int64_t P,
                            const double* scale, double* out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = energy_check(ctx, ref_dev, Mr, act_dev, Ma, P, scale, out);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const EnergyJobs jb = energy_jobs(Mr, Ma);
    EnergyWs w;
    { Carve m{nullptr}; carve_energy(m, w, jb, P);
      if (m.off > ctx->ws_limit)
          return fail(ctx, MCR_ENOMEM, "workspace limit too small: the energy distance of this shape needs %zu bytes, the limit is %zu",
                      m.off, ctx->ws_limit); }
    rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_energy(cv, w, jb, P); });
    if (rc) return rc;
    const std::vector<double> ones(scale ? 0 : (size_t)P, 1.0);            // x * 1.0 is x: one kernel text for both
    HIP_TRY(ctx, hipMemcpyAsync(w.scale, scale ? scale : ones.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    const bool aligned = ((Mr | Ma) & 1) == 0 &&
                         ((reinterpret_cast<uintptr_t>(ref_dev) | reinterpret_cast<uintptr_t>(act_dev)) & 15) == 0;
    i64 launches = 0, per = 0;
    energy_launches(jb, P, ctx->energy_launch_work, launches, per);
    for (i64 l = 0; l < launches; ++l) {                 // a partial per job: how the jobs are cut into launches changes no bit
        const i64 job0 = l * per, n = jb.total() - job0 < per ? jb.total() - job0 : per;
        const dim3 grid((unsigned)((n + 7) / 8 * 8));
        if (aligned)
            LAUNCH(ctx, K_ENERGY_PAIRS, (k_energy_pairs<true>), grid, dim3(kEnNT), 0, ref_dev, (i64)Mr, act_dev, (i64)Ma, (i64)P,
                   (const double*)w.scale, job0, n, w.part);
        else
            LAUNCH(ctx, K_ENERGY_PAIRS, (k_energy_pairs<false>), grid, dim3(kEnNT), 0, ref_dev, (i64)Mr, act_dev, (i64)Ma, (i64)P,
                   (const double*)w.scale, job0, n, w.part);
    }
    LAUNCH(ctx, K_ENERGY_REDUCE, k_energy_reduce, dim3(1), dim3(kEnNT), 0, (const double*)w.part, (i64)Mr, (i64)Ma, w.res);
    double res[9];
    HIP_TRY(ctx, hipMemcpyAsync(res, w.res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    if (!std::isfinite(res[6]) || !std::isfinite(res[7]) || !std::isfinite(res[8]))
        return fail(ctx, MCR_ENONFINITE, "draws contain non-finite values, or a squared distance overflows");
    memcpy(out, res, 6 * sizeof(double));
    return MCR_OK;
}

int mcr_energy_distance(mcr_ctx* ctx, const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P,
                        const double* scale, double* out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = energy_check(ctx, ref, Mr, act, Ma, P, scale, out);
    if (rc) return rc;
    const double *Xr, *Xa;
    rc = stage_two_samples(ctx, ref, Mr, act, Ma, P, &Xr, &Xa);
    if (rc) return rc;
    return mcr_energy_distance_dev(ctx, Xr, Mr, Xa, Ma, P, scale, out);
}

int mcr_energy_distance_host(const double* ref, int64_t Mr, const double* act, int64_t Ma, int64_t P, const double* scale,
                             double* out)
{
    try {
        const int rc = energy_host(ref, Mr, act, Ma, P, scale, out);
        return rc == 0 ? MCR_OK : rc == 1 ? MCR_EINVAL : MCR_ENONFINITE;
    } catch (const std::exception&) {
        return MCR_ENOMEM;
    }
}

}  // extern "C"

// ---- Calls on the pooled ascending order, and the other calls on one draw tensor ------------------------------------------
// Nested R-hat, Pareto k-hat, PSIS, HDI and autocorrelation each take one (C, N, P) tensor, run synchronously and cut its
// parameters into chunks under the workspace limit.  What that takes is here, once: the tensor and its acceptance
// (Tensor, pooled_check), the entry and the plan entry (tensor_entry, plan_entry), the chunk size and the chunk loop
// (plan_params, tensor_chunks) and the context's two call buffers (call_table, pooled_results).  Pareto k-hat, PSIS and HDI
// run the summary pipeline without diagnostics and quantiles -- tile sort, merges / bucket partition, k_order_stats,
// k_finalize for the non-finite count -- and then their own kernels on the keys the sort stage left (pooled_chunks); the
// two with tails share tail_check and tail_lds.  A family below supplies its own arguments' check, its chunk's layout,
// its launches and the scatter of its results, and nothing else.  Simulation-based calibration takes S such tensors (the
// Tensor's fourth axis) through the same entry and cuts its SIMULATIONS into chunks, where it needs the ingest copy at all.
namespace {

struct Tensor {
    const void* draws; int dtype; i64 C, N, P, sc, sn, sp;
    i64 S = 1, ss = 0;   // the fourth axis (mcr_sbc_ranks): S such tensors, each ss elements behind the one before
    i64 M() const { return C * N; }
    i64 extent() const
    {
        const i64 e = tensor_extent(C, N, P, sc, sn, sp);
        if (S < 1 || e <= 0) return S < 1 ? 0 : e;
        return ss < 0 ? -1 : (S - 1) * ss + e;
    }
    // f32 draws are widened by the ingest pass: the answer is the f64 call's on the widened tensor
    bool ingest() const { return dtype == MCR_F32 || needs_ingest(C, N, P, sc, sn, sp) || (S > 1 && ss != P * M()); }
};

// Acceptance of the tensor of such a call (`what` names the entry in the message).
int pooled_check(mcr_ctx* ctx, const char* what, const Tensor& t, const void* out)
{
    if (!out) return fail(ctx, MCR_EINVAL, "out is NULL");
    if (t.dtype != MCR_F64 && t.dtype != MCR_F32) return fail(ctx, MCR_EINVAL, "unsupported dtype %d", t.dtype);
    if (t.C < 0 || t.N < 0 || t.P < 0) return fail(ctx, MCR_EINVAL, "negative dimension (C=%lld N=%lld P=%lld)", (long long)t.C, (long long)t.N, (long long)t.P);
    if (t.N > 0 && (t.C > (i64)0x7FFFFFFFll / t.N || t.M() >= (i64)0x7FFFFFFFll)) return fail(ctx, MCR_EINVAL, "C*N must be < 2^31 - 1");
    if (!t.draws && t.S != 0 && t.M() * t.P > 0) return fail(ctx, MCR_EINVAL, "draws is NULL");   // (S == 0: nothing to read)
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "%s with summaries in flight", what);
    return MCR_OK;
}

// A host entry's upload: the tensor's extent (> 0) into ctx->stage; t.draws becomes the device copy.
int pooled_upload(mcr_ctx* ctx, Tensor& t)
{
    const size_t bytes = (size_t)t.extent() * (t.dtype == MCR_F64 ? 8 : 4);
    void* X = nullptr;
    const int rc = stage_buffers(ctx, {bytes}, &X);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(X, t.draws, bytes, hipMemcpyHostToDevice, ctx->stream));
    t.draws = X;
    return MCR_OK;
}

// An entry of such a call, the host's (the draws are uploaded) or the device's.  check(): the call's own arguments,
// once, behind the tensor's acceptance: every refusal comes before anything is uploaded or written.  empty(): the
// results of a tensor without draws (it has no extent: nothing is uploaded, and its strides are not looked at).
// run(t): the call on the tensor in device memory.
template <class Check, class Empty, class Run>
int tensor_entry(mcr_ctx* ctx, const char* what, Tensor t, const void* out, bool host, Check&& check, Empty&& empty, Run&& run)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    int rc = pooled_check(ctx, what, t, out);
    if (!rc) rc = check();
    if (rc || t.P == 0 || t.S == 0) return rc;
    if (t.M() == 0) { empty(); return MCR_OK; }
    if (t.extent() < 0) return fail(ctx, MCR_EINVAL, "negative strides are not supported");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (host && (rc = pooled_upload(ctx, t))) return rc;
    rc = run(t);
    return rc ? drain(ctx, rc, true) : rc;
}

// Parameters per workspace chunk: the most, up to P and to cap (what the launches' grids hold), whose layout fits the
// workspace limit.  layout(cv, pc) carves a chunk of pc parameters.
template <class Layout>
int plan_params(mcr_ctx* ctx, i64 P, i64 cap, Layout&& layout, i64& pcmax)
{
    auto measure = [&](i64 pc) { Carve m{nullptr}; layout(m, pc); return m.off; };
    pcmax = most_that_fit(P < cap ? P : cap, [&](i64 pc) { return measure(pc) <= ctx->ws_limit; });
    if (!pcmax) return fail(ctx, MCR_ENOMEM, "one parameter needs %zu bytes of workspace; limit is %zu", measure(1), ctx->ws_limit);
    return MCR_OK;
}

// An mcr_*_plan entry: 0 for a shape no call runs on (empty, or one pooled_check refuses), else what plan(pcmax) --
// the call's own argument check where it has one, then its plan_params -- answers (0 when it leaves pcmax alone).
template <class Plan>
int plan_entry(mcr_ctx* ctx, const char* what, const Tensor& t, int64_t* params_per_chunk, Plan&& plan)
{
    if (!ctx || !params_per_chunk) return fail(ctx, MCR_EINVAL, "%s: NULL argument", what);
    i64 pcmax = 0;
    if (t.C >= 1 && t.N >= 1 && t.P >= 1 && t.C <= (i64)0x7FFFFFFFll / t.N && t.M() < (i64)0x7FFFFFFFll) {
        const int rc = plan(pcmax);
        if (rc) return rc;
    }
    *params_per_chunk = pcmax;
    return MCR_OK;
}

// The chunks of a call: per chunk of at most pcmax parameters its workspace -- layout(cv, pc), as in plan_params,
// returns the chunk's ingest copy -- the ingest pass where the tensor needs one, then body(pc, p0, X): the call's launches
// on the chunk's f64 draws X[pc][M], the copy or the user's tensor at parameter p0.
template <class Layout, class Body>
int tensor_chunks(mcr_ctx* ctx, const Tensor& t, i64 pcmax, Layout&& layout, Body&& body)
{
    const bool ingest = t.ingest();
    for (i64 p0 = 0; p0 < t.P; p0 += pcmax) {
        const i64 pc = (t.P - p0 < pcmax) ? t.P - p0 : pcmax;
        double* copy = nullptr;
        int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { copy = layout(cv, pc); });
        if (!rc && ingest) rc = launch_ingest(ctx, t.draws, t.dtype, copy, t.C, t.N, pc, t.sc, t.sn, t.sp, p0);   // (one tensor: z = 1)
        if (!rc) rc = body(pc, p0, ingest ? copy : reinterpret_cast<const double*>(t.draws) + p0 * t.M());
        if (rc) return rc;
    }
    return MCR_OK;
}

// The call-level device table (the context's, shared by these calls): `head` -- a call's tail lengths, its chain
// permutation -- uploaded, and behind it the result rows.
template <typename T>
int call_table(mcr_ctx* ctx, const std::vector<T>& head, size_t res_doubles, T*& d_head, double*& d_res)
{
    const int rc = carve(ctx, ctx->call_dev, [&](Carve& cv) { d_head = cv.take<T>(head.size()); d_res = cv.take<double>(res_doubles); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_head, head.data(), sizeof(T) * head.size(), hipMemcpyHostToDevice, ctx->stream));
    return MCR_OK;
}

// The one D2H of the result table at the end of a call whose chunks ran the pipeline; each(r, pc, p0, p): the rows r of
// the chunk at p0, parameter p of its pc.  MCR_ENONFINITE when the pipeline counted a NaN or Inf draw (the outputs are
// written all the same).
template <class Each>
int pooled_results(mcr_ctx* ctx, const double* d_res, int fields, i64 P, i64 pcmax, Each&& each)
{
    const size_t bytes = sizeof(double) * (size_t)fields * (size_t)P;
    const int rc = ctx->call_host.reserve(ctx, bytes);
    if (rc) return rc;
    const double* h = ctx->call_host.as<double>();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->call_host.p, d_res, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (i64 at = 0; at < P; ++at) {
        const i64 p = at % pcmax, p0 = at - p, pc = (P - p0 < pcmax) ? P - p0 : pcmax;
        const double* r = h + (size_t)fields * (size_t)p0;
        nbad += r[(size_t)R_BAD * pc + p];
        each(r, pc, p0, p);
    }
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

constexpr int kPoolField0 = R_Q0;                          // the pipeline runs without quantiles: its rows end here

// The pipeline on pc parameters of one chain of M pooled draws, without quantiles; do_diag: with the rank codes.
PipeIn one_chain_pipe(i64 M, i64 pc, bool do_diag)
{
    PipeIn a{};
    a.M = M; a.pc = pc; a.C = 1; a.n = 1; a.nh = 0; a.nstage = 1; a.q.nq = 0; a.do_diag = do_diag;
    return a;
}

// The layout of a stats-only chunk, into a: the sort alone and the split points k_order_stats writes, then extra(cv, a):
// what the caller needs behind the pipeline's buffers.
template <class Extra>
auto pooled_layout(const Tensor& t, PipeIn& a, Extra& extra)
{
    return [&](Carve& cv, i64 pc) {
        a = one_chain_pipe(t.M(), pc, false);
        double* X = carve_pipe(cv, a, false, FftPlan{}, t.ingest());
        a.split = cv.take<i64>((size_t)pc);
        extra(cv, a);
        return X;
    };
}

// Parameters per workspace chunk of a call on the pooled order; grid_hi: what its own kernels' grids hold.
template <class Extra>
int plan_pooled(mcr_ctx* ctx, const Tensor& t, Extra&& extra, i64& pcmax, i64 grid_hi = kMaxGridY / 2)
{
    PipeIn a{};
    return plan_params(ctx, t.P, grid_hi < kMaxGridY / 2 ? grid_hi : kMaxGridY / 2, pooled_layout(t, a, extra), pcmax);
}

// The chunks of such a call: the stats-only pipeline into the chunk's rows d_res + fields * p0, then after(a, so, p0):
// the caller's kernels on the chunk's keys.
template <class Extra, class After>
int pooled_chunks(mcr_ctx* ctx, const Tensor& t, i64 pcmax, int fields, double* d_res, Extra&& extra, After&& after)
{
    PipeIn a{};
    return tensor_chunks(ctx, t, pcmax, pooled_layout(t, a, extra), [&](i64, i64 p0, const double* X) {
        a.X = X;
        a.d_res = d_res + (size_t)fields * (size_t)p0;
        Sorted so;
        const int rc = run_pipeline(ctx, a, &so);          // sort, order statistics, finalize (the bad count)
        return rc ? rc : after(a, so, p0);
    });
}

// A caller's tail length of parameter p, where it gives any.
int tail_check(mcr_ctx* ctx, const int64_t* ndraws_tail, i64 p)
{
    if (ndraws_tail && ndraws_tail[p] < 1)
        return fail(ctx, MCR_EINVAL, "ndraws_tail[%lld] = %lld: a tail length must be >= 1", (long long)p, (long long)ndraws_tail[p]);
    return MCR_OK;
}

// The dynamic LDS of a tail kernel on the chunk [p0, p0 + pc): `base` doubles and the chunk's longest tail that is staged
// there.  Above 60 KB the kernel is told.
int tail_lds(mcr_ctx* ctx, const std::vector<i64>& teff, i64 p0, i64 pc, size_t base, const void* kernel, size_t& lds)
{
    i64 tmax = 0;
    for (i64 p = p0; p < p0 + pc; ++p)
        if (teff[(size_t)p] <= kParetoLdsTail && teff[(size_t)p] > tmax) tmax = teff[(size_t)p];
    lds = sizeof(double) * (base + (size_t)tmax);
    if (lds > 60 * 1024) HIP_TRY(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MCR_OK;
}

}  // namespace

extern "C" {

// ---- nested R-hat (mcr_nested.hpp) ------------------------------------------------------------------------------------
constexpr i64 kMaxNestedChains = (i64)1 << 20;
constexpr int kNestKinds = 3;                              // raw, bulk, tail
constexpr int kNestField0 = kPoolField0;
constexpr int kNestFields = kNestField0 + 3 * kNestKinds;  // + (nrhat, B, W) per kind

static_assert(kMaxNestedChains == MCR_NESTED_MAX_CHAINS && kNestBlock == MCR_NESTED_BLOCK, "mcmcref_hip.h states the nested limits");

// The workspace of a chunk of pc parameters: the summary pipeline's layout for ONE chain of M draws (no buffer grows
// with chains x segments), then the chain moments and the superchain records.  Returns the ingest copy.
struct NestedChunk {
    const Tensor& t; i64 K;
    PipeIn a{}; double *mom = nullptr, *sup = nullptr;
    double* operator()(Carve& cv, i64 pc)
    {
        a = one_chain_pipe(t.M(), pc, true);
        double* X = carve_pipe(cv, a, true, FftPlan{}, t.ingest());
        mom = cv.take<double>((size_t)pc * kNestKinds * (size_t)t.C * 2);
        sup = cv.take<double>((size_t)pc * kNestKinds * (size_t)(K > 0 ? K : 1) * 2);
        return X;
    }
};

// Parameters per workspace chunk of a nested call (the most whose layout fits the limit and whose grids fit a launch).
static int plan_nested(mcr_ctx* ctx, NestedChunk& ch, i64& pcmax)
{
    const i64 nb = (ch.t.C + kNestChains - 1) / kNestChains;
    const i64 grid_cap = ((i64)0x7FFFFFFF / nb) / 8 * 8;   // k_chain_moments: ceil(pc / 8) * 8 * nb workgroups
    return plan_params(ctx, ch.t.P, grid_cap < kMaxGridY / 2 ? grid_cap : kMaxGridY / 2, ch, pcmax);
}

// What a nested call asks beyond pooled_check, and the chains ordered by superchain (stable): K runs of L chains in perm.
static int nested_check(mcr_ctx* ctx, i64 C, const int32_t* superchain, std::vector<int32_t>& perm, i64& K, i64& L)
{
    if (C > kMaxNestedChains)
        return fail(ctx, MCR_EINVAL, "nested R-hat supports at most %lld chains; got %lld", (long long)kMaxNestedChains, (long long)C);
    if (C > 0 && !superchain) return fail(ctx, MCR_EINVAL, "superchain is NULL");
    // superchains in the order of their first chain, chains in index order inside: the labels are names only
    std::unordered_map<int32_t, int32_t> dense;
    std::vector<int32_t> sid((size_t)C), count, first_label;
    for (i64 c = 0; c < C; ++c) {
        const auto it = dense.emplace(superchain[c], (int32_t)count.size());
        if (it.second) { count.push_back(0); first_label.push_back(superchain[c]); }
        sid[(size_t)c] = it.first->second;
        ++count[(size_t)it.first->second];
    }
    K = (i64)count.size();
    L = K > 0 ? count[0] : 0;
    for (i64 k = 1; k < K; ++k)
        if (count[(size_t)k] != L)
            return fail(ctx, MCR_EINVAL, "superchains must have the same number of chains: superchain %d has %lld, superchain %d has %lld",
                        (int)first_label[0], (long long)L, (int)first_label[(size_t)k], (long long)count[(size_t)k]);
    perm.resize((size_t)C);
    std::vector<i64> fill((size_t)K, 0);
    for (i64 c = 0; c < C; ++c) { const i64 k = sid[(size_t)c]; perm[(size_t)(k * L + fill[(size_t)k]++)] = (int32_t)c; }
    return MCR_OK;
}

static int nested_run(mcr_ctx* ctx, const Tensor& t, const std::vector<int32_t>& perm, i64 K, i64 L, const mcr_nested* out)
{
    const i64 M = t.M(), C = t.C, N = t.N, P = t.P;        // (the raw kind reads f64 rows: those of the ingest copy for f32 draws)
    NestedChunk ch{t, K};
    i64 pcmax = 0;
    int rc = plan_nested(ctx, ch, pcmax);
    if (rc) return rc;
    int32_t* d_perm = nullptr;
    double *d_res = nullptr, *ztab = nullptr;
    rc = get_ztab(ctx, M, &ztab);
    if (!rc) rc = call_table(ctx, perm, (size_t)kNestFields * (size_t)P, d_perm, d_res);
    if (rc) return rc;
    rc = tensor_chunks(ctx, t, pcmax, ch, [&](i64 pc, i64 p0, const double* X) -> int {
        PipeIn& a = ch.a;
        a.ztab = ztab;
        a.X = X;
        a.d_res = d_res + (size_t)kNestFields * (size_t)p0;
        const int rc = run_pipeline(ctx, a);   // one chain: sort, order statistics, bulk codes, fold, finalize (the bad count)
        if (rc) return rc;
        const i64 nb = (C + kNestChains - 1) / kNestChains;
        LAUNCH(ctx, K_CHAIN_MOMENTS, k_chain_moments, dim3((unsigned)((pc + 7) / 8 * 8 * nb)), dim3(kNestNT), 0,
               X, (const u32*)a.zb, (const u32*)a.zt, (const double*)ztab, M, C, N, pc, ch.mom);
        LAUNCH(ctx, K_NESTED_COMBINE, k_nested_combine, dim3((unsigned)pc, kNestKinds), dim3(kNestCombNT), 0,
               (const double*)ch.mom, (const int*)d_perm, C, K, L, N, ch.sup, a.d_res, pc, kNestField0);
        return MCR_OK;
    });
    if (rc) return rc;
    double* const dst[kNestKinds][3] = {{out->nrhat_raw, out->between_raw, out->within_raw},
                                        {out->nrhat_bulk, out->between_bulk, out->within_bulk},
                                        {out->nrhat_tail, out->between_tail, out->within_tail}};
    return pooled_results(ctx, d_res, kNestFields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        for (int k = 0; k < kNestKinds; ++k)
            for (int f = 0; f < 3; ++f)
                if (dst[k][f]) dst[k][f][p0 + p] = r[(size_t)(kNestField0 + 3 * k + f) * pc + p];
        if (out->nrhat) {                      // Python's max(bulk, tail)
            const double rb = r[(size_t)(kNestField0 + 3) * pc + p], rt = r[(size_t)(kNestField0 + 6) * pc + p];
            out->nrhat[p0 + p] = (rt > rb) ? rt : rb;
        }
    });
}

static void nested_fill_nan(const mcr_nested* o, i64 P)
{
    double* arrs[] = {o->nrhat, o->nrhat_bulk, o->nrhat_tail, o->nrhat_raw, o->between_bulk, o->within_bulk,
                      o->between_tail, o->within_tail, o->between_raw, o->within_raw};
    for (double* a : arrs)
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
}

int mcr_nested_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                    int64_t K, int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_nested_plan", t, params_per_chunk, [&](i64& pcmax) -> int {
        if (K < 1 || C > kMaxNestedChains) return MCR_OK;
        NestedChunk ch{t, K};
        return plan_nested(ctx, ch, pcmax);
    });
}

static int nested_entry(mcr_ctx* ctx, const Tensor& t, const int32_t* superchain, mcr_nested* out, bool host)
{
    std::vector<int32_t> perm;
    i64 K = 0, L = 0;
    return tensor_entry(ctx, "mcr_nested_rhat", t, out, host, [&] { return nested_check(ctx, t.C, superchain, perm, K, L); },
                        [&] { nested_fill_nan(out, t.P); },
                        [&](const Tensor& dev) { return nested_run(ctx, dev, perm, K, L, out); });
}

int mcr_nested_rhat_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                        int64_t sn, int64_t sp, const int32_t* superchain, mcr_nested* out)
{
    return nested_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, superchain, out, false);
}

int mcr_nested_rhat(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                    int64_t sp, const int32_t* superchain, mcr_nested* out)
{
    return nested_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, superchain, out, true);
}

// ---- Pareto k-hat (mcr_pareto.hpp) --------------------------------------------------------------------------------------
constexpr int kParField0 = kPoolField0;
constexpr int kParFields = kParField0 + 2;                 // + khat_left, khat_right

static_assert(kParetoLdsTail == MCR_PARETO_LDS_TAIL, "mcmcref_hip.h states the LDS tail");

// Behind the pipeline's buffers: the grid values l_j of every tail.
static double* carve_pareto(Carve& cv, const PipeIn& a)
{
    return cv.take<double>((size_t)a.pc * 2 * (size_t)pareto_grid(a.M / 2));
}

// Parameters per workspace chunk of a Pareto call.
static int plan_pareto(mcr_ctx* ctx, const Tensor& t, i64& pcmax)
{
    return plan_pooled(ctx, t, [](Carve& cv, PipeIn& a) { carve_pareto(cv, a); }, pcmax);
}

// The default tail length: the smallest t with t^2 r_eff >= 9 M (that is ceil(3 sqrt(M / r_eff))) for M > 225, else
// floor(M / 5).  A bisection over integers: t^2 is exact, its product with r_eff rounds once and is monotone in t, no
// sqrt takes part.  Capped at 2^31, beyond the floor(M / 2) of any call.  (pareto_tail_bisect: the bisection alone, for
// every M -- mcr_psis takes its minimum with ceil(M / 5).)
static i64 pareto_tail_bisect(i64 M, double r_eff)
{
    const double need = 9.0 * (double)M;
    i64 lo = 0, hi = (i64)1 << 31;                         // lo fails, hi holds (or is the cap)
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if ((double)(mid * mid) * r_eff >= need) hi = mid; else lo = mid;
    }
    return hi;
}
static i64 pareto_default_tail(i64 M, double r_eff) { return M <= 225 ? M / 5 : pareto_tail_bisect(M, r_eff); }

// The tail lengths a Pareto call is given, and the effective tail length of every parameter.
static int pareto_check(mcr_ctx* ctx, i64 M, i64 P, const int64_t* ndraws_tail, std::vector<i64>& teff)
{
    teff.resize((size_t)P);
    for (i64 p = 0; p < P; ++p) {
        const int rc = tail_check(ctx, ndraws_tail, p);
        if (rc) return rc;
        teff[(size_t)p] = pareto_tail_eff(M, ndraws_tail ? ndraws_tail[p] : pareto_default_tail(M, 1.0));
    }
    return MCR_OK;
}

static int pareto_run(mcr_ctx* ctx, const Tensor& t, const std::vector<i64>& teff, const mcr_pareto* out)
{
    const i64 M = t.M(), P = t.P;
    i64 pcmax = 0;
    int rc = plan_pareto(ctx, t, pcmax);
    i64* d_tail = nullptr;
    double* d_res = nullptr;
    if (!rc) rc = call_table(ctx, teff, (size_t)kParFields * (size_t)P, d_tail, d_res);
    if (rc) return rc;
    const i64 gmax = pareto_grid(M / 2);
    double* lg = nullptr;
    rc = pooled_chunks(ctx, t, pcmax, kParFields, d_res, [&](Carve& cv, PipeIn& a) { lg = carve_pareto(cv, a); },
                       [&](const PipeIn& a, const Sorted& so, i64 p0) -> int {
        size_t lds = 0;
        const int rc = tail_lds(ctx, teff, p0, a.pc, 0, reinterpret_cast<const void*>(&k_pareto_fit), lds);
        if (rc) return rc;
        LAUNCH(ctx, K_PARETO_FIT, k_pareto_fit, dim3((unsigned)((a.pc + 7) / 8 * 8 * 2)), dim3(kParetoNT), lds,
               (const double*)so.keys, M, a.pc, (const i64*)(d_tail + p0), so.keys_free, lg, gmax, a.d_res, kParField0);
        return MCR_OK;
    });
    if (rc) return rc;
    return pooled_results(ctx, d_res, kParFields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        const double kl = r[(size_t)kParField0 * pc + p], kr = r[(size_t)(kParField0 + 1) * pc + p];
        if (out->khat_left) out->khat_left[p0 + p] = kl;
        if (out->khat_right) out->khat_right[p0 + p] = kr;
        if (out->khat) out->khat[p0 + p] = (kr > kl) ? kr : kl;     // Python's max(left, right)
        if (out->ndraws_tail) out->ndraws_tail[p0 + p] = teff[(size_t)(p0 + p)];
    });
}

static void pareto_fill_nan(const mcr_pareto* o, i64 P)
{
    for (double* a : {o->khat, o->khat_left, o->khat_right})
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o->ndraws_tail) for (i64 p = 0; p < P; ++p) o->ndraws_tail[p] = 0;
}

int mcr_pareto_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                    int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_pareto_plan", t, params_per_chunk, [&](i64& pcmax) { return plan_pareto(ctx, t, pcmax); });
}

static int pareto_entry(mcr_ctx* ctx, const Tensor& t, const int64_t* ndraws_tail, mcr_pareto* out, bool host)
{
    std::vector<i64> teff;
    return tensor_entry(ctx, "mcr_pareto_khat", t, out, host, [&] { return pareto_check(ctx, t.M(), t.P, ndraws_tail, teff); },
                        [&] { pareto_fill_nan(out, t.P); }, [&](const Tensor& dev) { return pareto_run(ctx, dev, teff, out); });
}

int mcr_pareto_khat_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                        int64_t sn, int64_t sp, const int64_t* ndraws_tail, mcr_pareto* out)
{
    return pareto_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, ndraws_tail, out, false);
}

int mcr_pareto_khat(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                    int64_t sp, const int64_t* ndraws_tail, mcr_pareto* out)
{
    return pareto_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, ndraws_tail, out, true);
}

int64_t mcr_pareto_tail_length(int64_t M, double r_eff)
{
    if (!(r_eff > 0.0) || std::isinf(r_eff)) return MCR_EINVAL;
    return M < 1 ? 0 : pareto_default_tail(M, r_eff);
}

int mcr_pareto_fit_host(const double* sorted, int64_t M, int64_t ndraws_tail, double* khat_left, double* khat_right,
                        int64_t* t_eff)
{
    if (M < 0 || ndraws_tail < 0 || (M > 0 && !sorted)) return MCR_EINVAL;
    const i64 t = pareto_tail_eff(M, ndraws_tail > 0 ? ndraws_tail : pareto_default_tail(M, 1.0));
    if (t_eff) *t_eff = t;
    double kl = NAN, kr = NAN;
    if (t >= kParetoMinTail && t < (i64)0x7FFFFFFFll) {
        std::vector<double> e((size_t)t), lg((size_t)pareto_grid(t));
        const ParetoHostWave w;
        for (i64 i = 0; i < t; ++i) e[(size_t)i] = sorted[t] - sorted[t - 1 - i];
        kl = pareto_fit(w, e.data(), (int)t, lg.data());
        for (i64 i = 0; i < t; ++i) e[(size_t)i] = sorted[M - t + i] - sorted[M - t - 1];
        kr = pareto_fit(w, e.data(), (int)t, lg.data());
    }
    if (khat_left) *khat_left = kl;
    if (khat_right) *khat_right = kr;
    return MCR_OK;
}

// ---- Pareto-smoothed importance sampling and PSIS-LOO (mcr_psis.hpp) ------------------------------------------------------
constexpr int kPsisField0 = kPoolField0;
constexpr int kPsisFields = kPsisField0 + kPsisRows;       // + khat, ndraws_tail, lppd, elpd, p_loo

struct PsisWs { double *lg, *cols, *w; };

// The fit's grid values of a column: carve_pareto's scratch as it is, 2 pareto_grid(M / 2) >= pareto_grid(M - 1) doubles.
static i64 psis_gmax(i64 M) { return 2 * (i64)pareto_grid(M / 2); }

// Behind the pipeline's buffers: that scratch, the columns' scalars for k_psis_weights and, for the host entry's weights,
// the chunk's [pc][M] log weights.
static void carve_psis(Carve& cv, const PipeIn& a, bool host_weights, PsisWs& w)
{
    w.lg = carve_pareto(cv, a);
    w.cols = cv.take<double>((size_t)a.pc * kPsisCols);
    w.w = host_weights ? cv.take<double>((size_t)a.pc * (size_t)a.M) : nullptr;
}

// Columns per workspace chunk of a PSIS call: what fits, and no more than k_psis_weights' one-dimensional grid holds.
static int plan_psis(mcr_ctx* ctx, const Tensor& t, bool host_weights, i64& pcmax)
{
    const i64 grid_hi = ((i64)0x7FFFFFFFll / ((t.M() + kPsisBlock - 1) / kPsisBlock)) / 8 * 8;     // >= 1016: M < 2^31
    return plan_pooled(ctx, t, [&](Carve& cv, PipeIn& a) { PsisWs w; carve_psis(cv, a, host_weights, w); }, pcmax, grid_hi);
}

static bool psis_r_eff_ok(double r) { return r > 0.0 && !std::isinf(r); }

// The default tail length of M >= 1 values: min(ceil(M / 5), the smallest t with t^2 r_eff >= 9 M).
static i64 psis_default_tail(i64 M, double r_eff)
{
    const i64 fifth = (M + 4) / 5, root = pareto_tail_bisect(M, r_eff);
    return fifth < root ? fifth : root;
}

// The effective tail length: min(t_req, M - 1), t_req the caller's (>= 1) or the default.
static i64 psis_tail_eff(i64 M, i64 t_req, double r_eff)
{
    if (t_req < 1) t_req = psis_default_tail(M, r_eff);
    return t_req < M - 1 ? t_req : M - 1;
}

// The arguments of a PSIS call, and the effective tail length of every column.
static int psis_check(mcr_ctx* ctx, i64 M, i64 P, int negate, const double* r_eff, const int64_t* ndraws_tail, std::vector<i64>& teff)
{
    if (negate != 0 && negate != 1) return fail(ctx, MCR_EINVAL, "negate must be 0 or 1; got %d", negate);
    teff.resize((size_t)P);
    for (i64 p = 0; p < P; ++p) {
        const int rc = tail_check(ctx, ndraws_tail, p);
        if (rc) return rc;
        if (r_eff && !psis_r_eff_ok(r_eff[p]))
            return fail(ctx, MCR_EINVAL, "r_eff[%lld] = %g: a relative efficiency must be finite and > 0", (long long)p, r_eff[p]);
        teff[(size_t)p] = M < 1 ? 0 : psis_tail_eff(M, ndraws_tail ? ndraws_tail[p] : 0, r_eff ? r_eff[p] : 1.0);
    }
    return MCR_OK;
}

static int psis_run(mcr_ctx* ctx, const Tensor& t, int negate, const std::vector<i64>& teff, const mcr_psis_out* out, bool host_weights)
{
    const i64 M = t.M(), P = t.P;
    const bool hw = host_weights && out->log_weights;
    i64 pcmax = 0;
    int rc = plan_psis(ctx, t, hw, pcmax);
    i64* d_tail = nullptr;
    double* d_res = nullptr;
    if (!rc) rc = call_table(ctx, teff, (size_t)kPsisFields * (size_t)P, d_tail, d_res);
    if (rc) return rc;
    const i64 gmax = psis_gmax(M);
    const unsigned nb = (unsigned)((M + kPsisBlock - 1) / kPsisBlock);
    PsisWs w{};
    rc = pooled_chunks(ctx, t, pcmax, kPsisFields, d_res, [&](Carve& cv, PipeIn& a) { carve_psis(cv, a, hw, w); },
                       [&](const PipeIn& a, const Sorted& so, i64 p0) -> int {
        size_t lds = 0;
        const int rc = tail_lds(ctx, teff, p0, a.pc, kPsisScratch, reinterpret_cast<const void*>(&k_psis_column), lds);
        if (rc) return rc;
        const unsigned pgrp = (unsigned)((a.pc + 7) / 8 * 8);
        LAUNCH(ctx, K_PSIS_COLUMN, k_psis_column, dim3(pgrp), dim3(kPsisNT), lds, (const double*)so.keys, M, a.pc, negate,
               (const i64*)(d_tail + p0), so.keys_free, w.lg, gmax, a.d_res, kPsisField0, w.cols);
        if (!out->log_weights) return MCR_OK;
        double* dst = hw ? w.w : out->log_weights + p0 * M;
        if (a.idx16)
            LAUNCH(ctx, K_PSIS_WEIGHTS, k_psis_weights<unsigned short>, dim3(pgrp * nb), dim3(256), 0, (const double*)so.keys,
                   (const unsigned short*)so.pos, M, a.pc, negate, (const double*)w.cols, dst);
        else
            LAUNCH(ctx, K_PSIS_WEIGHTS, k_psis_weights<u32>, dim3(pgrp * nb), dim3(256), 0, (const double*)so.keys,
                   (const u32*)so.pos, M, a.pc, negate, (const double*)w.cols, dst);
        if (hw)
            HIP_TRY(ctx, hipMemcpyAsync(out->log_weights + p0 * M, w.w, sizeof(double) * (size_t)a.pc * (size_t)M,
                                        hipMemcpyDeviceToHost, ctx->stream));
        return MCR_OK;
    });
    if (rc) return rc;
    return pooled_results(ctx, d_res, kPsisFields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        const double* f = r + (size_t)kPsisField0 * pc + p;
        if (out->khat) out->khat[p0 + p] = f[PR_KHAT * pc];
        if (out->ndraws_tail) out->ndraws_tail[p0 + p] = (i64)f[PR_NTAIL * pc];
        if (out->lppd) out->lppd[p0 + p] = f[PR_LPPD * pc];
        if (out->elpd) out->elpd[p0 + p] = f[PR_ELPD * pc];
        if (out->p_loo) out->p_loo[p0 + p] = f[PR_PLOO * pc];
    });
}

static void psis_fill_nan(const mcr_psis_out* o, i64 P)
{
    for (double* a : {o->khat, o->lppd, o->elpd, o->p_loo})
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o->ndraws_tail) for (i64 p = 0; p < P; ++p) o->ndraws_tail[p] = 0;
}

// host: the host entry, whose log weights (like its draws) are the caller's host memory.
static int psis_entry(mcr_ctx* ctx, const Tensor& t, int negate, const double* r_eff, const int64_t* ndraws_tail, mcr_psis_out* out,
                      bool host)
{
    std::vector<i64> teff;
    return tensor_entry(ctx, "mcr_psis", t, out, host, [&] { return psis_check(ctx, t.M(), t.P, negate, r_eff, ndraws_tail, teff); },
                        [&] { psis_fill_nan(out, t.P); },
                        [&](const Tensor& dev) { return psis_run(ctx, dev, negate, teff, out, host); });
}

int mcr_psis_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                  int host_weights, int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_psis_plan", t, params_per_chunk, [&](i64& pcmax) { return plan_psis(ctx, t, host_weights != 0, pcmax); });
}

int mcr_psis_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                 int64_t sp, int negate, const double* r_eff, const int64_t* ndraws_tail, mcr_psis_out* out)
{
    return psis_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, negate, r_eff, ndraws_tail, out, false);
}

int mcr_psis(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
             int negate, const double* r_eff, const int64_t* ndraws_tail, mcr_psis_out* out)
{
    return psis_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, negate, r_eff, ndraws_tail, out, true);
}

int64_t mcr_psis_tail_length(int64_t M, double r_eff)
{
    if (!psis_r_eff_ok(r_eff)) return MCR_EINVAL;
    return M < 1 ? 0 : psis_default_tail(M, r_eff);
}

int mcr_psis_host(const double* values, int64_t M, int negate, double r_eff, int64_t ndraws_tail, double* khat,
                  int64_t* n_tail, double* lppd, double* elpd, double* p_loo, double* log_weights)
{
    if (M < 0 || M >= (i64)0x7FFFFFFFll || (M > 0 && !values) || (negate != 0 && negate != 1) || ndraws_tail < 0 ||
        !psis_r_eff_ok(r_eff))
        return MCR_EINVAL;
    PsisResult c{};
    c.khat = c.lppd = c.elpd = c.ploo = NAN;
    if (M > 0) {
        for (i64 i = 0; i < M; ++i)
            if (!std::isfinite(values[i])) return MCR_ENONFINITE;
        std::vector<i64> at((size_t)M);
        for (i64 i = 0; i < M; ++i) at[(size_t)i] = i;
        std::sort(at.begin(), at.end(), [&](i64 a, i64 b) { return values[a] < values[b]; });
        std::vector<double> keys((size_t)M);
        for (i64 j = 0; j < M; ++j) keys[(size_t)j] = values[at[(size_t)j]];
        const i64 t = psis_tail_eff(M, ndraws_tail, r_eff);
        std::vector<double> e((size_t)(t > 0 ? t : 1)), lg((size_t)pareto_grid(t));
        const PsisKeys s{keys.data(), M, negate};
        c = psis_column(PsisHostGroup{}, s, t, e.data(), lg.data());
        if (log_weights)
            for (i64 j = 0; j < M; ++j) log_weights[at[(size_t)j]] = psis_log_weight(s, c, negate ? M - 1 - j : j);
    }
    if (khat) *khat = c.khat;
    if (n_tail) *n_tail = c.n;
    if (lppd) *lppd = c.lppd;
    if (elpd) *elpd = c.elpd;
    if (p_loo) *p_loo = c.ploo;
    return MCR_OK;
}

// ---- Highest-density intervals (mcr_hdi.hpp) ----------------------------------------------------------------------------
constexpr int kHdiField0 = kPoolField0;
constexpr int hdi_fields(int nprob) { return kHdiField0 + 3 * nprob; }     // + lo, hi, index of every probability

static_assert(kHdiSlice == MCR_HDI_SLICE && kHdiMaxProbs == MCR_HDI_MAX_PROBS, "mcmcref_hip.h states the slice and the cap");
static_assert((kHdiSlice & (kHdiSlice - 1)) == 0, "a slice is a power of two");

// Behind the pipeline's buffers: one candidate per (parameter, probability, slice), for the most slices a probability can
// need (inc = 0: W = M) -- the plan knows the number of probabilities, not their values.
static HdiCand* carve_hdi(Carve& cv, const PipeIn& a, int nprob)
{
    return cv.take<HdiCand>((size_t)a.pc * (size_t)nprob * (size_t)hdi_slices(a.M));
}

// Parameters per workspace chunk of an HDI call: what fits, and no more than k_hdi_window's one-dimensional grid holds.
static int plan_hdi(mcr_ctx* ctx, const Tensor& t, int nprob, i64& pcmax)
{
    const i64 grid_hi = ((i64)0x7FFFFFFFll / ((i64)nprob * hdi_slices(t.M()))) / 8 * 8;  // >= 4096: M < 2^31, nprob <= 16
    return plan_pooled(ctx, t, [&](Carve& cv, PipeIn& a) { carve_hdi(cv, a, nprob); }, pcmax, grid_hi);
}

// The probabilities of a call, and inc = floor(prob * M) of every one: one rounded product.
static int hdi_check(mcr_ctx* ctx, const double* probs, int nprob, i64 M, HdiArgs& h)
{
    if (nprob < 1 || nprob > kHdiMaxProbs) return fail(ctx, MCR_EINVAL, "nprob must be in [1, %d]; got %d", kHdiMaxProbs, nprob);
    if (!probs) return fail(ctx, MCR_EINVAL, "probs is NULL");
    h.nprob = nprob;
    for (int j = 0; j < nprob; ++j) {
        if (!(probs[j] > 0.0 && probs[j] < 1.0)) return fail(ctx, MCR_EINVAL, "probs[%d] = %g: a probability must lie in (0, 1)", j, probs[j]);
        h.inc[j] = (i64)std::floor(probs[j] * (double)M);
    }
    return MCR_OK;
}

static void hdi_store(const mcr_hdi_out* o, i64 at, double lo, double hi, i64 index)
{
    if (o->lo) o->lo[at] = lo;
    if (o->hi) o->hi[at] = hi;
    if (o->index) o->index[at] = index;
}

static int hdi_run(mcr_ctx* ctx, const Tensor& t, const HdiArgs& h, const mcr_hdi_out* out)
{
    const i64 M = t.M(), P = t.P;
    const int nprob = h.nprob, fields = hdi_fields(nprob), nsl = (int)hdi_slices(M);
    i64 pcmax = 0;
    int rc = plan_hdi(ctx, t, nprob, pcmax);
    double* d_res = nullptr;
    if (!rc) rc = carve(ctx, ctx->call_dev, [&](Carve& cv) { d_res = cv.take<double>((size_t)fields * (size_t)P); });
    if (rc) return rc;
    HdiCand* part = nullptr;
    rc = pooled_chunks(ctx, t, pcmax, fields, d_res, [&](Carve& cv, PipeIn& a) { part = carve_hdi(cv, a, nprob); },
                       [&](const PipeIn& a, const Sorted& so, i64) -> int {
        LAUNCH(ctx, K_HDI_WINDOW, k_hdi_window, dim3((unsigned)((a.pc + 7) / 8 * 8 * nprob * nsl)), dim3(kHdiNT), 0,
               (const double*)so.keys, M, a.pc, h, nsl, part);
        LAUNCH(ctx, K_HDI_PICK, k_hdi_pick, dim3((unsigned)((a.pc * nprob + 63) / 64)), dim3(64), 0,
               (const double*)so.keys, M, a.pc, h, nsl, (const HdiCand*)part, a.d_res, kHdiField0);
        return MCR_OK;
    });
    if (rc) return rc;
    return pooled_results(ctx, d_res, fields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        for (int j = 0; j < nprob; ++j) {
            const double* f = r + (size_t)(kHdiField0 + 3 * j) * pc + p;
            hdi_store(out, (p0 + p) * nprob + j, f[0], f[pc], (i64)f[2 * pc]);
        }
    });
}

int mcr_hdi_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp, int nprob,
                 int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_hdi_plan", t, params_per_chunk, [&](i64& pcmax) {
        if (nprob < 1 || nprob > kHdiMaxProbs) return fail(ctx, MCR_EINVAL, "nprob must be in [1, %d]; got %d", kHdiMaxProbs, nprob);
        return plan_hdi(ctx, t, nprob, pcmax);
    });
}

static int hdi_entry(mcr_ctx* ctx, const Tensor& t, const double* probs, int nprob, mcr_hdi_out* out, bool host)
{
    HdiArgs h{};
    return tensor_entry(ctx, "mcr_hdi", t, out, host, [&] { return hdi_check(ctx, probs, nprob, t.M(), h); },
                        [&] { for (i64 at = 0; at < t.P * nprob; ++at) hdi_store(out, at, NAN, NAN, -1); },
                        [&](const Tensor& dev) { return hdi_run(ctx, dev, h, out); });
}

int mcr_hdi_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                int64_t sp, const double* probs, int nprob, mcr_hdi_out* out)
{
    return hdi_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, probs, nprob, out, false);
}

int mcr_hdi(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
            const double* probs, int nprob, mcr_hdi_out* out)
{
    return hdi_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, probs, nprob, out, true);
}

int mcr_hdi_sorted_host(const double* sorted, int64_t M, const double* probs, int nprob, double* lo, double* hi, int64_t* index)
{
    if (M < 0 || (M > 0 && !sorted) || !probs || nprob < 1 || nprob > kHdiMaxProbs) return MCR_EINVAL;
    for (int j = 0; j < nprob; ++j)
        if (!(probs[j] > 0.0 && probs[j] < 1.0)) return MCR_EINVAL;
    for (int j = 0; j < nprob; ++j) {
        const i64 inc = (i64)std::floor(probs[j] * (double)M), W = M - inc;
        HdiCand best = HdiCand::none();
        for (i64 i = 0; i < W; ++i) hdi_take(best, sorted[i + inc] - sorted[i], i);
        const bool ok = best.i >= 0 && best.i < W;
        if (lo) lo[j] = ok ? sorted[best.i] : NAN;
        if (hi) hi[j] = ok ? sorted[best.i + inc] : NAN;
        if (index) index[j] = ok ? best.i : -1;
    }
    return MCR_OK;
}

// ---- Importance-weighted summaries (mcr_weighted.hpp) -------------------------------------------------------------------
constexpr int kWgtField0 = kPoolField0;
constexpr int wgt_fields(int nq) { return kWgtField0 + WR_Q0 + nq; }       // + mean, sd, mean_se and every quantile

static_assert(kWgtBlock == MCR_WEIGHTED_BLOCK && kWgtMaxQ == MCR_WEIGHTED_MAX_Q, "mcmcref_hip.h states the block and the cap");

struct WgtWs { double *part, *mean, *qb; };

// Behind the pipeline's buffers: the moment passes' block sums (two per block in the second pass), the means between the
// passes and, with quantiles, the sorted order's block sums.
static void carve_weighted(Carve& cv, const PipeIn& a, int nq, WgtWs& w)
{
    const size_t nb = (size_t)wgt_blocks(a.M);
    w.part = cv.take<double>((size_t)a.pc * nb * 2);
    w.mean = cv.take<double>((size_t)a.pc);
    w.qb = nq > 0 ? cv.take<double>((size_t)a.pc * nb) : nullptr;
}

// Parameters per workspace chunk of a weighted call: what fits, and no more than the one-dimensional grids hold.
static int plan_weighted(mcr_ctx* ctx, const Tensor& t, int nq, i64& pcmax)
{
    const i64 grid_hi = ((i64)0x7FFFFFFFll / wgt_blocks(t.M())) / 8 * 8;          // >= 1016: M < 2^31
    return plan_pooled(ctx, t, [&](Carve& cv, PipeIn& a) { WgtWs w; carve_weighted(cv, a, nq, w); }, pcmax, grid_hi);
}

// The call's own arguments: the flags, the weight vector's presence, the probabilities.
static int weighted_check(mcr_ctx* ctx, const double* v, i64 M, int flags, const double* probs, int nq, WgtArgs& g)
{
    if (flags & ~MCR_W_LOG) return fail(ctx, MCR_EINVAL, "unknown flag bits 0x%x", flags & ~MCR_W_LOG);
    if (nq < 0 || nq > kWgtMaxQ) return fail(ctx, MCR_EINVAL, "nq must be in [0, %d]; got %d", kWgtMaxQ, nq);
    if (nq > 0 && !probs) return fail(ctx, MCR_EINVAL, "probs is NULL");
    if (M > 0 && !v) return fail(ctx, MCR_EINVAL, "weights is NULL");
    g.nq = nq;
    for (int j = 0; j < nq; ++j) {
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return fail(ctx, MCR_EINVAL, "probs[%d] = %g: a probability must lie in [0, 1]", j, probs[j]);
        g.q[j] = probs[j];
    }
    return MCR_OK;
}

// What the prepared totals say about the weight vector, in one text for the device and the host routine.
static const char* weighted_refusal(const double* tot, char* text, size_t len)
{
    if (tot[WT_BAD] > 0.0) snprintf(text, len, "weights: %.0f entries are not weights (linear: finite and >= 0; log: finite or -inf)", tot[WT_BAD]);
    else if (!(tot[WT_S1] > 0.0)) snprintf(text, len, "weights: no entry is positive");
    else if (std::isinf(tot[WT_S1]) || std::isinf(tot[WT_S2])) snprintf(text, len, "weights: their sum or sum of squares overflows");
    else return nullptr;
    return text;
}

static void weighted_fill_nan(const mcr_weighted_out* o, i64 P, int nq)
{
    for (double* a : {o->mean, o->sd, o->mean_se})
        if (a) for (i64 p = 0; p < P; ++p) a[p] = NAN;
    if (o->quantiles) for (i64 at = 0; at < P * nq; ++at) o->quantiles[at] = NAN;
    if (o->ess) *o->ess = NAN;
    if (o->weight_sum) *o->weight_sum = NAN;
}

// host: the host entry, whose weight vector and weights output (like its draws) are the caller's host memory.
static int weighted_run(mcr_ctx* ctx, const Tensor& t, const double* v, int flags, const WgtArgs& g, const mcr_weighted_out* out, bool host)
{
    const i64 M = t.M(), P = t.P, nb = wgt_blocks(M);
    const int nq = g.nq, fields = wgt_fields(nq), log = (flags & MCR_W_LOG) ? 1 : 0;
    i64 pcmax = 0;
    int rc = plan_weighted(ctx, t, nq, pcmax);
    double *d_v = nullptr, *d_w = nullptr, *d_bs = nullptr, *d_tot = nullptr, *d_res = nullptr;
    if (!rc) rc = carve(ctx, ctx->call_dev, [&](Carve& cv) {
        d_v = host ? cv.take<double>((size_t)M) : nullptr;
        d_w = cv.take<double>((size_t)M);
        d_bs = cv.take<double>((size_t)nb * 2);
        d_tot = cv.take<double>(kWgtTotals);
        d_res = cv.take<double>((size_t)fields * (size_t)P);
    });
    if (rc) return rc;
    if (host) HIP_TRY(ctx, hipMemcpyAsync(d_v, v, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, K_WEIGHT_PREPARE, k_weight_prepare, dim3(1), dim3(kWgtPrepNT), 0, host ? (const double*)d_v : v, M, log, d_w, d_bs, d_tot);
    double tot[kWgtTotals];
    HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    char text[160];
    if (weighted_refusal(tot, text, sizeof text)) return fail(ctx, MCR_EINVAL, "%s", text);
    WgtWs w{};
    const unsigned nsl = (unsigned)((nb + kWgtSlice - 1) / kWgtSlice);
    rc = pooled_chunks(ctx, t, pcmax, fields, d_res, [&](Carve& cv, PipeIn& a) { carve_weighted(cv, a, nq, w); },
                       [&](const PipeIn& a, const Sorted& so, i64) -> int {
        const unsigned pgrp = (unsigned)((a.pc + 7) / 8 * 8);
        LAUNCH(ctx, K_WEIGHTED_MOMENTS, k_weighted_moments<1>, dim3(pgrp * nsl), dim3(kWgtNT), 0, (const double*)a.X, (const double*)d_w, M, a.pc,
               (const double*)w.mean, w.part);
        LAUNCH(ctx, K_WEIGHTED_COMBINE, k_weighted_combine<1>, dim3((unsigned)a.pc), dim3(kWave), 0, (const double*)w.part, nb, a.pc,
               (const double*)d_tot, w.mean, a.d_res, kWgtField0);
        LAUNCH(ctx, K_WEIGHTED_MOMENTS, k_weighted_moments<2>, dim3(pgrp * nsl), dim3(kWgtNT), 0, (const double*)a.X, (const double*)d_w, M, a.pc,
               (const double*)w.mean, w.part);
        LAUNCH(ctx, K_WEIGHTED_COMBINE, k_weighted_combine<2>, dim3((unsigned)a.pc), dim3(kWave), 0, (const double*)w.part, nb, a.pc,
               (const double*)d_tot, w.mean, a.d_res, kWgtField0);
        if (!nq) return MCR_OK;
        if (a.idx16) {
            LAUNCH(ctx, K_WQ_BLOCKS, k_wq_blocks<unsigned short>, dim3(pgrp * (unsigned)nb), dim3(kWave), 0,
                   (const unsigned short*)so.pos, (const double*)d_w, M, a.pc, w.qb);
            LAUNCH(ctx, K_WQ_PICK, k_wq_pick<unsigned short>, dim3(pgrp), dim3(kWgtNT), 0, (const double*)so.keys,
                   (const unsigned short*)so.pos, (const double*)d_w, M, a.pc, g, (const double*)w.qb, a.d_res, kWgtField0 + WR_Q0);
        } else {
            LAUNCH(ctx, K_WQ_BLOCKS, k_wq_blocks<u32>, dim3(pgrp * (unsigned)nb), dim3(kWave), 0, (const u32*)so.pos,
                   (const double*)d_w, M, a.pc, w.qb);
            LAUNCH(ctx, K_WQ_PICK, k_wq_pick<u32>, dim3(pgrp), dim3(kWgtNT), 0, (const double*)so.keys, (const u32*)so.pos,
                   (const double*)d_w, M, a.pc, g, (const double*)w.qb, a.d_res, kWgtField0 + WR_Q0);
        }
        return MCR_OK;
    });
    if (rc) return rc;
    if (out->weights)
        HIP_TRY(ctx, hipMemcpyAsync(out->weights, d_w, sizeof(double) * (size_t)M, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                    ctx->stream));
    if (out->ess) *out->ess = wgt_sq(tot[WT_S1]) / tot[WT_S2];
    if (out->weight_sum) *out->weight_sum = tot[WT_S1];
    return pooled_results(ctx, d_res, fields, P, pcmax, [&](const double* r, i64 pc, i64 p0, i64 p) {
        const double* f = r + (size_t)kWgtField0 * pc + p;
        if (out->mean) out->mean[p0 + p] = f[WR_MEAN * pc];
        if (out->sd) out->sd[p0 + p] = f[WR_SD * pc];
        if (out->mean_se) out->mean_se[p0 + p] = f[WR_SE * pc];
        if (out->quantiles) for (int j = 0; j < nq; ++j) out->quantiles[(p0 + p) * nq + j] = f[(WR_Q0 + j) * pc];
    });
}

int mcr_weighted_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp, int nq,
                      int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_weighted_plan", t, params_per_chunk, [&](i64& pcmax) {
        if (nq < 0 || nq > kWgtMaxQ) return fail(ctx, MCR_EINVAL, "nq must be in [0, %d]; got %d", kWgtMaxQ, nq);
        return plan_weighted(ctx, t, nq, pcmax);
    });
}

static int weighted_entry(mcr_ctx* ctx, const Tensor& t, const double* v, int flags, const double* probs, int nq,
                          mcr_weighted_out* out, bool host)
{
    WgtArgs g{};
    return tensor_entry(ctx, "mcr_weighted_summary", t, out, host, [&] { return weighted_check(ctx, v, t.M(), flags, probs, nq, g); },
                        [&] { weighted_fill_nan(out, t.P, nq); },
                        [&](const Tensor& dev) { return weighted_run(ctx, dev, v, flags, g, out, host); });
}

int mcr_weighted_summary_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc,
                             int64_t sn, int64_t sp, const double* weights_dev, int flags, const double* probs, int nq,
                             mcr_weighted_out* out)
{
    return weighted_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, weights_dev, flags, probs, nq, out, false);
}

int mcr_weighted_summary(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                         int64_t sp, const double* weights, int flags, const double* probs, int nq, mcr_weighted_out* out)
{
    return weighted_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, weights, flags, probs, nq, out, true);
}

int mcr_weighted_host(const double* x, const double* v, int64_t M, int flags, const double* probs, int nq, double* mean,
                      double* sd, double* mean_se, double* quantiles, double* ess, double* weight_sum, double* weights)
{
    if (M < 0 || M >= (i64)0x7FFFFFFFll || (M > 0 && (!x || !v)) || (flags & ~MCR_W_LOG) || nq < 0 || nq > kWgtMaxQ || (nq > 0 && !probs))
        return MCR_EINVAL;
    for (int j = 0; j < nq; ++j)
        if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return MCR_EINVAL;
    double r_mean = NAN, r_sd = NAN, r_se = NAN, r_ess = NAN, r_s1 = NAN;
    std::vector<double> q((size_t)nq, NAN);
    if (M > 0) {
        const int log = (flags & MCR_W_LOG) ? 1 : 0;
        double tot[kWgtTotals] = {0.0, -INFINITY, 0.0, 0.0};
        for (i64 m = 0; m < M; ++m) {
            if (wgt_bad(v[m], log)) tot[WT_BAD] += 1.0;
            else if (v[m] > tot[WT_MAX]) tot[WT_MAX] = v[m];
        }
        std::vector<double> w((size_t)M, 0.0);
        WgtHostTree tr;
        if (!(tot[WT_BAD] > 0.0) && !(log && !(tot[WT_MAX] > -INFINITY))) {
            for (i64 m = 0; m < M; ++m) w[(size_t)m] = wgt_weight(v[m], log, tot[WT_MAX]);
            tot[WT_S1] = wgt_host_sum(tr, M, [&](i64 m) { return w[(size_t)m]; });
            tot[WT_S2] = wgt_host_sum(tr, M, [&](i64 m) { return wgt_sq(w[(size_t)m]); });
        }
        char text[160];
        if (weighted_refusal(tot, text, sizeof text)) return MCR_EINVAL;
        for (i64 m = 0; m < M; ++m)
            if (!std::isfinite(x[m])) return MCR_ENONFINITE;
        const double S1 = tot[WT_S1];
        r_s1 = S1;
        r_ess = wgt_sq(S1) / tot[WT_S2];
        r_mean = wgt_host_sum(tr, M, [&](i64 m) { return wgt_wx(w[(size_t)m], x[m]); }) / S1;
        double t1, t2;
        const double q1 = wgt_host_sum(tr, M, [&](i64 m) { wgt_dev2(w[(size_t)m], x[m], r_mean, t1, t2); return t1; });
        const double q2 = wgt_host_sum(tr, M, [&](i64 m) { wgt_dev2(w[(size_t)m], x[m], r_mean, t1, t2); return t2; });
        r_sd = std::sqrt(q1 / S1);
        r_se = std::sqrt(q2) / S1;
        if (nq > 0) {
            std::vector<i64> at((size_t)M);
            for (i64 i = 0; i < M; ++i) at[(size_t)i] = i;
            std::sort(at.begin(), at.end(), [&](i64 a, i64 b) { return x[a] < x[b] || (x[a] == x[b] && a < b); });
            const auto u = [&](i64 j) { return w[(size_t)at[(size_t)j]]; };
            std::vector<double> roots;
            wgt_host_sum(tr, M, u, &roots);
            for (int j = 0; j < nq; ++j) {
                double t = 0.0, prev = 0.0;
                const i64 b = wgt_find_block([&](i64 k) { return roots[(size_t)k]; }, (i64)roots.size(), probs[j], t, prev);
                if (b < 0) continue;
                tr.build([&](int i) { const i64 k = b * kWgtBlock + i; return k < M ? u(k) : 0.0; });
                for (int i = 0; i < kWgtBlock && b * kWgtBlock + i < M; ++i)
                    if (wgt_reached(wgt_add(prev, wgt_prefix(tr, i + 1)), t)) { q[(size_t)j] = x[at[(size_t)(b * kWgtBlock + i)]]; break; }
            }
        }
        if (weights) for (i64 m = 0; m < M; ++m) weights[m] = w[(size_t)m];
    }
    if (mean) *mean = r_mean;
    if (sd) *sd = r_sd;
    if (mean_se) *mean_se = r_se;
    if (ess) *ess = r_ess;
    if (weight_sum) *weight_sum = r_s1;
    if (quantiles) for (int j = 0; j < nq; ++j) quantiles[j] = q[(size_t)j];
    return MCR_OK;
}

// ---- Simulation-based calibration (mcr_sbc.hpp) ------------------------------------------------------------------------------
// The tensor's fourth axis: the call is cut into chunks of SIMULATIONS, not of parameters, and only where it needs the
// ingest copy; the result table [kSbcFields][S P] lies behind the uploaded truth in the call's device table.

// What a call asks of its shape beyond pooled_check (`ctx` NULL: the host routine's, no message kept): the plan entry's too.
static int sbc_shape_check(mcr_ctx* ctx, i64 S, i64 P)
{
    if (S < 0) return fail(ctx, MCR_EINVAL, "negative dimension (S=%lld)", (long long)S);
    if (P > 0 && S > (i64)0x7FFFFFFFll / P) return fail(ctx, MCR_EINVAL, "S*P must be < 2^31");
    return MCR_OK;
}

// ... and of its true values.
static int sbc_check(mcr_ctx* ctx, i64 S, i64 P, const double* truth)
{
    const int rc = sbc_shape_check(ctx, S, P);
    if (rc) return rc;
    if (!truth && S * P > 0) return fail(ctx, MCR_EINVAL, "truth is NULL");
    for (i64 k = 0; k < S * P; ++k)
        if (!std::isfinite(truth[k]))
            return fail(ctx, MCR_EINVAL, "truth[%lld][%lld] = %g: the true values must be finite", (long long)(k / P), (long long)(k % P), truth[k]);
    return MCR_OK;
}

// Simulations without draws: the counts 0, NaN mean and sd.
static void sbc_fill_empty(const mcr_sbc_out* o, i64 rows)
{
    for (int64_t* a : {o->n_less, o->n_equal})
        if (a) for (i64 k = 0; k < rows; ++k) a[k] = 0;
    for (double* a : {o->mean, o->sd})
        if (a) for (i64 k = 0; k < rows; ++k) a[k] = NAN;
}

// Simulations per workspace chunk: all of them where the kernel reads the caller's rows, else as many ingest copies as fit.
static int plan_sbc(mcr_ctx* ctx, const Tensor& t, i64& scmax)
{
    scmax = t.S;
    if (!t.ingest()) return MCR_OK;
    // k P < 2^31 rows (sbc_shape_check) of M < 2^31 - 1 draws: the count of doubles stays below 2^62; its bytes may not fit
    auto measure = [&](i64 k) {
        const size_t n = (size_t)k * (size_t)t.P * (size_t)t.M();
        if (n > SIZE_MAX / (2 * sizeof(double))) return (size_t)SIZE_MAX;
        Carve m{nullptr};
        m.take<double>(n);
        return m.off;
    };
    scmax = most_that_fit(t.S, [&](i64 k) { return measure(k) <= ctx->ws_limit; });
    if (!scmax) return fail(ctx, MCR_ENOMEM, "one simulation needs %zu bytes of workspace; limit is %zu", measure(1), ctx->ws_limit);
    return MCR_OK;
}

// Rows of up to kSbcRegBlocks blocks stay in registers between the passes; one block needs a quarter of them.
static int launch_sbc(mcr_ctx* ctx, const double* X, i64 L, i64 rows, const double* d_truth, double* d_res, i64 stride)
{
    const dim3 grid((unsigned)((rows + kSbcRows - 1) / kSbcRows));
    if (L > kWgtBlock && L <= (i64)kSbcRegBlocks * kWgtBlock)
        LAUNCH(ctx, K_SBC_RANKS, (k_sbc_ranks<kSbcRegBlocks>), grid, dim3(kSbcNT), 0, X, L, rows, d_truth, d_res, stride);
    else
        LAUNCH(ctx, K_SBC_RANKS, (k_sbc_ranks<1>), grid, dim3(kSbcNT), 0, X, L, rows, d_truth, d_res, stride);
    return MCR_OK;
}

static int sbc_run(mcr_ctx* ctx, const Tensor& t, const double* truth, const mcr_sbc_out* out)
{
    const i64 L = t.M(), P = t.P, rows = t.S * P;
    i64 scmax = 0;
    int rc = plan_sbc(ctx, t, scmax);
    if (rc) return rc;
    const std::vector<double> head(truth, truth + rows);
    double *d_truth = nullptr, *d_res = nullptr;
    rc = call_table(ctx, head, (size_t)kSbcFields * (size_t)rows, d_truth, d_res);
    if (!rc) rc = ctx->call_host.reserve(ctx, sizeof(double) * (size_t)kSbcFields * (size_t)rows);
    if (rc) return rc;
    const bool ingest = t.ingest();
    const size_t es = t.dtype == MCR_F64 ? 8 : 4;
    for (i64 s0 = 0; s0 < t.S; s0 += scmax) {
        const i64 sc = t.S - s0 < scmax ? t.S - s0 : scmax, r0 = s0 * P;
        const double* X = reinterpret_cast<const double*>(t.draws) + r0 * L;
        if (ingest) {
            double* copy = nullptr;
            rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { copy = cv.take<double>((size_t)sc * (size_t)P * (size_t)L); });
            for (i64 s = 0; s < sc && !rc; s += kMaxGridY)                         // (k_ingest's simulations lie along z,
                for (i64 p0 = 0; p0 < P && !rc; p0 += kMaxGridY / 2) {             //  its parameters along y)
                    const i64 ns = sc - s < kMaxGridY ? sc - s : kMaxGridY, pc = P - p0 < kMaxGridY / 2 ? P - p0 : kMaxGridY / 2;
                    rc = launch_ingest(ctx, static_cast<const char*>(t.draws) + (size_t)(s0 + s) * (size_t)t.ss * es, t.dtype,
                                       copy + (s * P + p0) * L, t.C, t.N, pc, t.sc, t.sn, t.sp, p0, ns, t.ss, P * L);
                }
            if (rc) return rc;
            X = copy;
        }
        rc = launch_sbc(ctx, X, L, sc * P, d_truth + r0, d_res + r0, rows);
        if (rc) return rc;
    }
    const double* h = ctx->call_host.as<double>();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->call_host.p, d_res, sizeof(double) * (size_t)kSbcFields * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (i64 k = 0; k < rows; ++k) {
        if (out->n_less) out->n_less[k] = (int64_t)h[(size_t)SB_LESS * (size_t)rows + (size_t)k];
        if (out->n_equal) out->n_equal[k] = (int64_t)h[(size_t)SB_EQUAL * (size_t)rows + (size_t)k];
        nbad += h[(size_t)SB_BAD * (size_t)rows + (size_t)k];
    }
    if (out->mean) memcpy(out->mean, h + (size_t)SB_MEAN * (size_t)rows, sizeof(double) * (size_t)rows);
    if (out->sd) memcpy(out->sd, h + (size_t)SB_SD * (size_t)rows, sizeof(double) * (size_t)rows);
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

static Tensor sbc_tensor(const void* draws, int dtype, i64 S, i64 C, i64 N, i64 P, i64 ss, i64 sc, i64 sn, i64 sp)
{
    Tensor t{draws, dtype, C, N, P, sc, sn, sp};
    t.S = S; t.ss = ss;
    return t;
}

static int sbc_entry(mcr_ctx* ctx, const Tensor& t, const double* truth, mcr_sbc_out* out, bool host)
{
    return tensor_entry(ctx, "mcr_sbc_ranks", t, out, host, [&] { return sbc_check(ctx, t.S, t.P, truth); },
                        [&] { sbc_fill_empty(out, t.S * t.P); }, [&](const Tensor& dev) { return sbc_run(ctx, dev, truth, out); });
}

int mcr_sbc_ranks_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t ss,
                      int64_t sc, int64_t sn, int64_t sp, const double* truth, mcr_sbc_out* out)
{
    return sbc_entry(ctx, sbc_tensor(draws_dev, dtype, S, C, N, P, ss, sc, sn, sp), truth, out, false);
}

int mcr_sbc_ranks(mcr_ctx* ctx, const void* draws, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t ss, int64_t sc,
                  int64_t sn, int64_t sp, const double* truth, mcr_sbc_out* out)
{
    return sbc_entry(ctx, sbc_tensor(draws, dtype, S, C, N, P, ss, sc, sn, sp), truth, out, true);
}

int mcr_sbc_plan(mcr_ctx* ctx, int dtype, int64_t S, int64_t C, int64_t N, int64_t P, int64_t ss, int64_t sc, int64_t sn,
                 int64_t sp, int64_t* sims_per_chunk)
{
    const Tensor t = sbc_tensor(nullptr, dtype, S, C, N, P, ss, sc, sn, sp);
    return plan_entry(ctx, "mcr_sbc_plan", t, sims_per_chunk, [&](i64& scmax) {
        const int rc = sbc_shape_check(ctx, S, P);                         // (what the call would refuse, the plan refuses)
        return rc || S < 1 ? rc : plan_sbc(ctx, t, scmax);
    });
}

int mcr_sbc_ranks_host(const double* x, int64_t S, int64_t P, int64_t L, const double* truth, mcr_sbc_out* out)
{
    if (!out || P < 0 || L < 0 || L >= (i64)0x7FFFFFFFll) return MCR_EINVAL;
    const int rc = sbc_check(nullptr, S, P, truth);
    if (rc) return rc;
    const i64 rows = S * P;
    if (rows == 0) return MCR_OK;
    if (L == 0) { sbc_fill_empty(out, rows); return MCR_OK; }
    if (!x) return MCR_EINVAL;
    WgtHostTree tr;
    i64 nbad = 0;
    for (i64 k = 0; k < rows; ++k) {
        i64 less, equal, bad;
        double mean, sd;
        sbc_row_host(tr, x + k * L, L, truth[k], less, equal, bad, mean, sd);
        if (out->n_less) out->n_less[k] = less;
        if (out->n_equal) out->n_equal[k] = equal;
        if (out->mean) out->mean[k] = mean;
        if (out->sd) out->sd[k] = sd;
        nbad += bad;
    }
    return nbad > 0 ? MCR_ENONFINITE : MCR_OK;
}

double mcr_chi2_sf(double x, double dof)
{
    if (!(dof > 0.0) || !(x >= 0.0)) return NAN;
    return sbc_gamma_q(0.5 * dof, 0.5 * x);
}

int mcr_sbc_uniformity(const int64_t* ranks, int64_t S, int64_t P, int64_t L, int64_t B, int64_t* counts, double* expected,
                       double* chi2, double* pvalue, double* ecdf_dev)
{
    if (!ranks || S < 1 || P < 0 || L < 0 || L >= (i64)0x7FFFFFFFll || B < 2 || B > L + 1) return MCR_EINVAL;
    std::vector<double> ex((size_t)B);
    for (i64 b = 0; b < B; ++b)
        ex[(size_t)b] = (double)S * (double)(sbc_bin_start(b + 1, B, L) - sbc_bin_start(b, B, L)) / (double)(L + 1);
    if (expected) memcpy(expected, ex.data(), sizeof(double) * (size_t)B);
    std::vector<i64> sorted((size_t)S);
    for (i64 p = 0; p < P; ++p) {
        double c2, ec;
        if (!sbc_uniform_column(reinterpret_cast<const i64*>(ranks) + p, S, P, L, B, ex.data(), sorted, counts ? reinterpret_cast<i64*>(counts) + p * B : nullptr, c2, ec))
            return MCR_EINVAL;
        if (chi2) chi2[p] = c2;
        if (pvalue) pvalue[p] = mcr_chi2_sf(c2, (double)(B - 1));
        if (ecdf_dev) ecdf_dev[p] = ec;
    }
    return MCR_OK;
}

// ---- Autocorrelation functions and times (mcr_acf.hpp) ---------------------------------------------------------------------
static_assert(kAcfMaxLag == MCR_ACF_MAX_LAG && kAcfBlock == MCR_ACF_BLOCK, "mcmcref_hip.h states the lag limit and the block");

// The workspace of a chunk of pc parameters: the ingest copy (returned), the chains' means, the blocks' lag products, the
// chains' gamma.
struct AcfChunk {
    const Tensor& t; AcfGeom g;
    double *mean = nullptr, *part = nullptr, *gam = nullptr;
    double* operator()(Carve& cv, i64 pc)
    {
        const size_t chains = (size_t)pc * (size_t)t.C;
        double* X = t.ingest() ? cv.take<double>(chains * (size_t)t.N) : nullptr;
        mean = cv.take<double>(chains);
        part = cv.take<double>(chains * (size_t)g.nblk * (size_t)g.lp);
        gam = cv.take<double>(chains * (size_t)g.lp);
        return X;
    }
};

// Parameters per workspace chunk of an autocorrelation call: what fits, and no more than k_acf_products' grid holds.
static int plan_acf(mcr_ctx* ctx, AcfChunk& ch, i64& pcmax)
{
    return plan_params(ctx, ch.t.P, ((i64)0x7FFFFFFFll / (ch.g.nbg * ch.g.nlb)) / 8 * 8, ch, pcmax);
}

// The lag, flag and window arguments of a call on chains of N draws (`ctx` NULL: the host routine's, no message kept).
static int acf_check_args(mcr_ctx* ctx, i64 N, i64 L, int flags, double wc)
{
    if (L < 0) return fail(ctx, MCR_EINVAL, "max_lag = %lld: a maximum lag must be >= 0", (long long)L);
    if (L > kAcfMaxLag) return fail(ctx, MCR_EINVAL, "max_lag = %lld exceeds MCR_ACF_MAX_LAG = %lld", (long long)L, (long long)kAcfMaxLag);
    if (N >= 1 && L > N - 1) return fail(ctx, MCR_EINVAL, "max_lag = %lld exceeds N - 1 = %lld", (long long)L, (long long)(N - 1));
    if (flags & ~MCR_ACF_UNBIASED) return fail(ctx, MCR_EINVAL, "unknown flag bits 0x%x", (unsigned)(flags & ~MCR_ACF_UNBIASED));
    if (!std::isfinite(wc) || !(wc > 0.0)) return fail(ctx, MCR_EINVAL, "window_c = %g: the window constant must be finite and > 0", wc);
    return MCR_OK;
}

// An empty chain (or none): NaN and -1 everywhere.
static void acf_fill_nan(const mcr_acf_out* o, i64 C, i64 P, i64 L)
{
    const i64 pcn = P * C;
    if (o->acf) for (i64 k = 0; k < pcn * (L + 1); ++k) o->acf[k] = NAN;
    for (double* a : {o->var, o->tau})
        if (a) for (i64 k = 0; k < pcn; ++k) a[k] = NAN;
    if (o->window) for (i64 k = 0; k < pcn; ++k) o->window[k] = -1;
    if (o->acf_pooled) for (i64 k = 0; k < P * (L + 1); ++k) o->acf_pooled[k] = NAN;
    if (o->tau_pooled) for (i64 p = 0; p < P; ++p) o->tau_pooled[p] = NAN;
    if (o->window_pooled) for (i64 p = 0; p < P; ++p) o->window_pooled[p] = -1;
}

static int acf_run(mcr_ctx* ctx, const Tensor& t, i64 L, int flags, double wc, const mcr_acf_out* out)
{
    const i64 C = t.C, N = t.N, P = t.P;
    AcfChunk ch{t, acf_geom(N, L)};
    const AcfGeom& g = ch.g;
    i64 pcmax = 0;
    int rc = plan_acf(ctx, ch, pcmax);
    if (rc) return rc;
    const size_t pcn = (size_t)P * (size_t)C, nl = (size_t)(L + 1);
    double *d_acf = nullptr, *d_var, *d_tau, *d_bad, *d_acfp, *d_taup;
    i64 *d_win, *d_winp;
    rc = carve(ctx, ctx->call_dev, [&](Carve& cv) {
        d_acf = out->acf ? cv.take<double>(pcn * nl) : nullptr;
        d_var = cv.take<double>(pcn); d_tau = cv.take<double>(pcn); d_win = cv.take<i64>(pcn); d_bad = cv.take<double>(pcn);
        d_acfp = cv.take<double>((size_t)P * nl); d_taup = cv.take<double>((size_t)P); d_winp = cv.take<i64>((size_t)P);
    });
    if (!rc) rc = ctx->call_host.reserve(ctx, sizeof(double) * pcn);
    if (rc) return rc;
    // the chains of a launch lie along y and z (any C), four per workgroup in k_acf_mean
    auto chain_grid = [](i64 n, unsigned gx) { const i64 gy = n < kMaxGridY ? n : kMaxGridY; return dim3(gx, (unsigned)gy, (unsigned)((n + gy - 1) / gy)); };
    const size_t lds = sizeof(double) * acf_lds_doubles(g), lds_fin = sizeof(double) * nl;
    rc = tensor_chunks(ctx, t, pcmax, ch, [&](i64 pc, i64 p0, const double* X) -> int {
        const unsigned gx = (unsigned)((pc + 7) / 8 * 8);
        const size_t at = (size_t)p0 * (size_t)C;
        LAUNCH(ctx, K_ACF_MEAN, k_acf_mean, chain_grid((C + 3) / 4, gx), dim3(256), 0, X, C, N, pc, ch.mean, d_bad + at);
        LAUNCH(ctx, K_ACF_PRODUCTS, k_acf_products, chain_grid(C, (unsigned)(gx * g.nbg * g.nlb)), dim3((unsigned)acf_threads(g)), lds,
               X, (const double*)ch.mean, C, N, pc, g, ch.part);
        LAUNCH(ctx, K_ACF_FINISH, k_acf_finish, chain_grid(C, gx), dim3(kAcfFinNT), lds_fin, (const double*)ch.part, C, N, pc, L, g,
               flags & MCR_ACF_UNBIASED, wc, ch.gam, d_acf ? d_acf + at * nl : nullptr, d_var + at, d_tau + at, d_win + at);
        LAUNCH(ctx, K_ACF_POOL, k_acf_pool, dim3(gx), dim3(kAcfFinNT), lds_fin, (const double*)ch.gam, C, pc, L, g.lp, wc,
               d_acfp + (size_t)p0 * nl, d_taup + p0, d_winp + p0);
        return MCR_OK;
    });
    if (rc) return rc;
    double* h_bad = ctx->call_host.as<double>();
    auto fetch = [&](void* dst, const void* src, size_t bytes) {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    };
    HIP_TRY(ctx, fetch(h_bad, d_bad, sizeof(double) * pcn));
    HIP_TRY(ctx, fetch(out->acf, d_acf, sizeof(double) * pcn * nl));
    HIP_TRY(ctx, fetch(out->var, d_var, sizeof(double) * pcn));
    HIP_TRY(ctx, fetch(out->tau, d_tau, sizeof(double) * pcn));
    HIP_TRY(ctx, fetch(out->window, d_win, sizeof(i64) * pcn));
    HIP_TRY(ctx, fetch(out->acf_pooled, d_acfp, sizeof(double) * (size_t)P * nl));
    HIP_TRY(ctx, fetch(out->tau_pooled, d_taup, sizeof(double) * (size_t)P));
    HIP_TRY(ctx, fetch(out->window_pooled, d_winp, sizeof(i64) * (size_t)P));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    double nbad = 0.0;
    for (size_t k = 0; k < pcn; ++k) nbad += h_bad[k];
    if (nbad > 0.0) return fail(ctx, MCR_ENONFINITE, "draws contain %.0f non-finite value(s)", nbad);
    return MCR_OK;
}

int mcr_autocorr_plan(mcr_ctx* ctx, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                      int64_t max_lag, int64_t* params_per_chunk)
{
    const Tensor t{nullptr, dtype, C, N, P, sc, sn, sp};
    return plan_entry(ctx, "mcr_autocorr_plan", t, params_per_chunk, [&](i64& pcmax) {
        const int rc = acf_check_args(ctx, N, max_lag, 0, 1.0);
        if (rc) return rc;
        AcfChunk ch{t, acf_geom(N, max_lag)};
        return plan_acf(ctx, ch, pcmax);
    });
}

static int acf_entry(mcr_ctx* ctx, const Tensor& t, i64 L, int flags, double wc, mcr_acf_out* out, bool host)
{
    return tensor_entry(ctx, "mcr_autocorr", t, out, host, [&] { return acf_check_args(ctx, t.N, L, flags, wc); },
                        [&] { acf_fill_nan(out, t.C, t.P, L); }, [&](const Tensor& dev) { return acf_run(ctx, dev, L, flags, wc, out); });
}

int mcr_autocorr_dev(mcr_ctx* ctx, const void* draws_dev, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn,
                     int64_t sp, int64_t max_lag, int flags, double window_c, mcr_acf_out* out)
{
    return acf_entry(ctx, {draws_dev, dtype, C, N, P, sc, sn, sp}, max_lag, flags, window_c, out, false);
}

int mcr_autocorr(mcr_ctx* ctx, const void* draws, int dtype, int64_t C, int64_t N, int64_t P, int64_t sc, int64_t sn, int64_t sp,
                 int64_t max_lag, int flags, double window_c, mcr_acf_out* out)
{
    return acf_entry(ctx, {draws, dtype, C, N, P, sc, sn, sp}, max_lag, flags, window_c, out, true);
}

int mcr_autocorr_host(const double* chains, int64_t C, int64_t N, int64_t max_lag, int flags, double window_c, mcr_acf_out* out)
{
    if (!out || C < 0 || N < 0 || (N > 0 && (C > (i64)0x7FFFFFFFll / N || C * N >= (i64)0x7FFFFFFFll)) || (C * N > 0 && !chains)) return MCR_EINVAL;
    const i64 L = max_lag;
    const int rc = acf_check_args(nullptr, N, L, flags, window_c);
    if (rc) return rc;
    if (C * N == 0) { acf_fill_nan(out, C, 1, L); return MCR_OK; }
    const bool unbiased = (flags & MCR_ACF_UNBIASED) != 0;
    const i64 nblk = (N + kAcfBlock - 1) / kAcfBlock;
    std::vector<double> d((size_t)N), gam((size_t)(L + 1)), rho((size_t)(L + 1)), pool((size_t)(L + 1), 0.0);
    i64 nbad = 0;
    for (i64 c = 0; c < C; ++c) {
        const double* x = chains + c * N;
        double v[kWave];
        for (int j = 0; j < kWave; ++j) v[j] = acf_lane_sum(x, N, j, &nbad);
        for (int o = kWave >> 1; o > 0; o >>= 1)                       // the xor tree, as lane 0 sees it
            for (int j = 0; j < o; ++j) v[j] = v[j] + v[j + o];
        const double m = v[0] / (double)N;
        for (i64 i = 0; i < N; ++i) d[(size_t)i] = x[i] - m;
        for (i64 l = 0; l <= L; ++l) {
            double S = 0.0;
            for (i64 b = 0; b < nblk; ++b) {
                const i64 i0 = b * kAcfBlock, i1 = i0 + kAcfBlock < N - l ? i0 + kAcfBlock : N - l;
                double acc = 0.0;
                for (i64 i = i0; i < i1; ++i) acc = fma(d[(size_t)i], d[(size_t)(i + l)], acc);
                S += acc;
            }
            gam[(size_t)l] = acf_gamma(S, N, l, unbiased);
            pool[(size_t)l] += gam[(size_t)l];
        }
        for (i64 l = 0; l <= L; ++l) rho[(size_t)l] = acf_rho(gam[(size_t)l], gam[0]);
        double t;
        i64 w;
        acf_tau_scan(rho.data(), L, window_c, t, w);
        if (out->acf) memcpy(out->acf + c * (L + 1), rho.data(), sizeof(double) * (size_t)(L + 1));
        if (out->var) out->var[c] = gam[0];
        if (out->tau) out->tau[c] = t;
        if (out->window) out->window[c] = w;
    }
    for (i64 l = 0; l <= L; ++l) pool[(size_t)l] = pool[(size_t)l] / (double)C;
    for (i64 l = 0; l <= L; ++l) rho[(size_t)l] = acf_rho(pool[(size_t)l], pool[0]);
    double t;
    i64 w;
    acf_tau_scan(rho.data(), L, window_c, t, w);
    if (out->acf_pooled) memcpy(out->acf_pooled, rho.data(), sizeof(double) * (size_t)(L + 1));
    if (out->tau_pooled) *out->tau_pooled = t;
    if (out->window_pooled) *out->window_pooled = w;
    return nbad > 0 ? MCR_ENONFINITE : MCR_OK;
}

// Device-resident form (draws_dev [P][M] f64, cov_dev [P][P] f64, both in this context's device memory): what
// tools/cov_bench.py times.  Synchronous.
int mcr_covariance_dev(mcr_ctx* ctx, const double* draws_dev, int64_t M, int64_t P, double* cov_dev)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || M < 1 || (P > 0 && (!draws_dev || !cov_dev))) return fail(ctx, MCR_EINVAL, "bad argument");
    if (P == 0) return MCR_OK;
    if (P > 8192) return fail(ctx, MCR_EINVAL, "P > 8192 not supported by mcr_covariance");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_covariance with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int nb = (int)((P + kCovBM - 1) / kCovBM);
    const i64 P64 = (i64)nb * kCovBM;
    const i64 tiles = (i64)nb * (nb + 1) / 2;                        // workgroups per draw slice (none below the diagonal)
    int ksplit = (int)((512 + tiles - 1) / tiles);                   // >= ~512 workgroups: two per CU
    const i64 maxsplit = (M + 16 * kCovBK - 1) / (16 * kCovBK);      // a slice is at least 16 panels long
    if (ksplit > maxsplit) ksplit = (int)maxsplit;
    {   // the slices' partial tiles are summed by k_cov_final: at most 128 MB of them
        const i64 cap = ((i64)128 << 20) / (P64 * P64 * 8);
        if (ksplit > cap) ksplit = (int)(cap < 1 ? 1 : cap);
    }
    if (ksplit < 1) ksplit = 1;
    i64 kchunk = (M + ksplit - 1) / ksplit;
    kchunk = (kchunk + kCovBK - 1) / kCovBK * kCovBK;
    ksplit = (int)((M + kchunk - 1) / kchunk);
    const int S = 8;
    double *partial, *mpart, *d_mean, *d_std;
    int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) {
        partial = cv.take<double>((size_t)ksplit * P64 * P64);
        mpart = cv.take<double>((size_t)P * S * kMomRec);
        d_mean = cv.take<double>((size_t)P);
        d_std = cv.take<double>((size_t)P);
    });
    if (rc) return rc;
    rc = moments_impl<double>(ctx, draws_dev, 1, M, P, M, 1, M, d_mean, d_std, mpart, (M >= 8 * 2048) ? S : 1, true);
    if (rc) return rc;
    if ((M & 1) == 0 && (reinterpret_cast<uintptr_t>(draws_dev) & 15) == 0) {
        LAUNCH(ctx, K_COV, (k_cov_mfma<true>), dim3((unsigned)tiles, (unsigned)ksplit), dim3(256), 0, draws_dev,
               (const double*)d_mean, (i64)M, (i64)P, nb, kchunk, partial);
    } else {
        LAUNCH(ctx, K_COV, (k_cov_mfma<false>), dim3((unsigned)tiles, (unsigned)ksplit), dim3(256), 0, draws_dev,
               (const double*)d_mean, (i64)M, (i64)P, nb, kchunk, partial);
    }
    LAUNCH(ctx, K_COV_FINAL, k_cov_final, dim3((unsigned)((P * P + 255) / 256)), dim3(256), 0, (const double*)partial,
           ksplit, nb, (i64)M, (i64)P, cov_dev);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

int mcr_covariance(mcr_ctx* ctx, const double* draws, int64_t M, int64_t P, double* cov)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || M < 1 || (P > 0 && (!draws || !cov))) return fail(ctx, MCR_EINVAL, "bad argument");
    if (P == 0) return MCR_OK;
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_covariance with summaries in flight");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* buf[2];
    int rc = stage_buffers(ctx, {sizeof(double) * (size_t)P * M, sizeof(double) * (size_t)P * P}, buf);
    if (rc) return rc;
    double *X = (double*)buf[0], *d_cov = (double*)buf[1];
    HIP_TRY(ctx, hipMemcpyAsync(X, draws, sizeof(double) * (size_t)P * M, hipMemcpyHostToDevice, ctx->stream));
    rc = mcr_covariance_dev(ctx, X, M, P, d_cov);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(cov, d_cov, sizeof(double) * (size_t)P * P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
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
