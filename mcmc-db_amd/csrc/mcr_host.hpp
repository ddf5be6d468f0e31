// mcr_host.hpp -- what the translation units of libmcmcref_hip.so share: the context, its buffers and the tools of a call
// (fail, HIP_TRY, LAUNCH, the profiling events, the workspace carving: Carve, align_up and most_that_fit of mcr_carve.hpp).  With mcr_pipe.hpp -- how mcr_stats.hip runs the
// pipeline of mcr_api.hip -- this is the complete list of what mcr_api.hip (context, summary pipeline), mcr_stats.hip (the
// other statistics), mcr_files.hip (file and text ingest, writers) and mcr_comm.hip (RCCL) may use of each other; everything
// else lives in its unit's anonymous namespace.  Internal: not installed, and it includes no kernel header.
#pragma once
#include "../../include/mcmcref_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "mcr_carve.hpp"
#include "mcr_device.hpp"

namespace mcr {
namespace host {

constexpr int kMaxGridY = 65535;

// The kernels the profiling mode accounts for (mcr_profile_get): id and name, in the order of the ids.
#define MCR_KERNELS(X)                                   \
    X(K_INGEST, "k_ingest")                              \
    X(K_MOMENTS, "k_moments")                            \
    X(K_MOMENTS_FINAL, "k_moments_final")                \
    X(K_TILE_SORT, "k_tile_sort")                        \
    X(K_MERGE, "k_merge")                                \
    X(K_ORDER_STATS, "k_order_stats")                    \
    X(K_RANK_Z, "k_rank_z")                              \
    X(K_FOLD_MERGE, "k_fold_merge")                      \
    X(K_DIAG, "k_diag")                                  \
    X(K_FINALIZE, "k_finalize")                          \
    X(K_COMPARE, "k_compare")                            \
    X(K_FILL, "k_fill_synth")                            \
    X(K_SPLITTERS, "k_splitters")                        \
    X(K_BUCKET_MERGE, "k_bucket_merge")                  \
    X(K_ACOV_MORE, "k_acov_more")                        \
    X(K_DIAG2, "k_diag_combine2")                        \
    X(K_ACOV_SEG, "k_acov_seg")                          \
    X(K_TWO_SAMPLE, "k_two_sample")                      \
    X(K_COV, "k_cov_mfma")                               \
    X(K_ZTABLE, "k_ztable")                              \
    X(K_PQ_SNAPPY, "k_pq_snappy")                        \
    X(K_PQ_DECODE, "k_pq_decode")                        \
    X(K_GATHER, "k_gather_rows")                         \
    X(K_ACOV_LONG, "k_acov_long")                        \
    X(K_DIAG_LONG, "k_diag_long_scan")                   \
    X(K_COV_FINAL, "k_cov_final")                        \
    X(K_FFT, "k_fft")                                    \
    X(K_CSV_LINES, "k_csv_lines")                        \
    X(K_CSV_SCAN, "k_csv_scan")                          \
    X(K_CSV_PARSE, "k_csv_parse")                        \
    X(K_CSV_PATCH, "k_csv_patch")                        \
    X(K_CSV_TABLE_PARSE, "k_csv_table_parse")            \
    X(K_CSV_UNSIGN_ZERO, "k_csv_unsign_zero")            \
    X(K_JSON_INDEX, "k_json_index")                      \
    X(K_JSON_SCAN, "k_json_scan")                        \
    X(K_JSON_PARSE, "k_json_parse")                      \
    X(K_LAYOUT_SCAN, "k_layout_scan")                    \
    X(K_LAYOUT_KEYS, "k_layout_keys")                    \
    X(K_LAYOUT_HIST, "k_layout_hist")                    \
    X(K_LAYOUT_OFFSETS, "k_layout_offsets")              \
    X(K_LAYOUT_SCATTER, "k_layout_scatter")              \
    X(K_LAYOUT_BOUNDS, "k_layout_bounds")                \
    X(K_PQW_ENCODE, "k_pqw_encode")                      \
    X(K_PQW_COMPACT, "k_pqw_compact")                    \
    X(K_CSVW_FORMAT, "k_csvw_format")                    \
    X(K_CSVW_SCAN, "k_csvw_scan")                        \
    X(K_CSVW_COMPACT, "k_csvw_compact")                  \
    X(K_SELECT_ROWS, "k_select_rows")                    \
    X(K_PROJECT, "k_project")                            \
    X(K_CHAIN_MOMENTS, "k_chain_moments")                \
    X(K_NESTED_COMBINE, "k_nested_combine")              \
    X(K_PARETO_FIT, "k_pareto_fit")                      \
    X(K_PSIS_COLUMN, "k_psis_column")                    \
    X(K_PSIS_WEIGHTS, "k_psis_weights")                  \
    X(K_HDI_WINDOW, "k_hdi_window")                      \
    X(K_HDI_PICK, "k_hdi_pick")                          \
    X(K_WEIGHT_PREPARE, "k_weight_prepare")              \
    X(K_WEIGHTED_MOMENTS, "k_weighted_moments")          \
    X(K_WEIGHTED_COMBINE, "k_weighted_combine")          \
    X(K_WQ_BLOCKS, "k_wq_blocks")                        \
    X(K_WQ_PICK, "k_wq_pick")                            \
    X(K_SBC_RANKS, "k_sbc_ranks")                        \
    X(K_ACF_MEAN, "k_acf_mean")                          \
    X(K_ACF_PRODUCTS, "k_acf_products")                  \
    X(K_ACF_FINISH, "k_acf_finish")                      \
    X(K_ACF_POOL, "k_acf_pool")                          \
    X(K_ENERGY_PAIRS, "k_energy_pairs")                  \
    X(K_ENERGY_REDUCE, "k_energy_reduce")                \
    X(K_CHOL_PANEL, "k_chol_panel")                      \
    X(K_CHOL_BELOW, "k_chol_below")                      \
    X(K_CHOL_UPDATE, "k_chol_update")                    \
    X(K_CHOL_FINISH, "k_chol_finish")                    \
    X(K_SOLVE_LOWER, "k_solve_lower")                    \
    X(K_SYM_SCALE, "k_sym_scale")                        \
    X(K_ROW_SUMSQ, "k_row_sumsq")                        \
    X(K_GAUSS_SUMS, "k_gauss_sums")                      \
    X(K_ROW_MEAN, "k_row_mean")
#define MCR_KERNEL_ID(id, name) id,
#define MCR_KERNEL_NAME(id, name) name,
enum KernelId { MCR_KERNELS(MCR_KERNEL_ID) K_COUNT };       // K_INGEST = 0
extern const char* const kKernelNames[K_COUNT];            // (mcr_api.hip)

struct EvPair { hipEvent_t a, b; int kid; };

// The owners of the library's memory: DevBuf (hipMalloc) and PinBuf (pinned host memory, hipHostMalloc).  Move-only; the
// destructor frees.  reserve is the one growth rule (defined behind the context, whose streams it waits for).
template <bool kPinned> struct Buf {
    void* p = nullptr; size_t cap = 0;       // bytes
    size_t slack_div = 0;                    // reserve allocates bytes + bytes / slack_div, so that near-equal sizes do not
                                             // reallocate (0: the exact size)
    explicit Buf(size_t slack = 0) : slack_div(slack) {}
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap), slack_div(o.slack_div) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(slack_div, o.slack_div); return *this; }
    ~Buf() { release(); }
    void release() { if (p) { kPinned ? hipHostFree(p) : hipFree(p); } p = nullptr; cap = 0; }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    int reserve(mcr_ctx* ctx, size_t bytes);
};
using DevBuf = Buf<false>;
using PinBuf = Buf<true>;

struct Slot {
    DevBuf d_res, d_off; PinBuf h_res, h_off;   // result table (doubles) and chain offsets (i64): device, pinned host
    i64 off_C = -1, off_N = -1;     // regular chain offsets c * N already resident in d_off (no upload per call)
    mcr_summary out{};
    i64 P = 0; int nq = 0;
    bool trivial_nan = false;  // M == 0: no kernels ran
    hipEvent_t done = nullptr;  // recorded on the slot's lane after its last copy (mcr_summarize_wait_one)
    i64 qlo[MCR_MAX_QUANTILES];
    i64 pcmax = 0;             // parameters per workspace chunk: chunk k has the results of [k pcmax, (k + 1) pcmax)
};

}  // namespace host
}  // namespace mcr

struct mcr_ctx {
    using i64 = mcr::i64; using DevBuf = mcr::host::DevBuf; using PinBuf = mcr::host::PinBuf;
    int device = 0;
    hipStream_t stream = nullptr;
    char err[512] = "";
    size_t ws_limit = 0;
    // Lanes = streams with a workspace each (MCR_LANES, default 4): consecutive enqueues rotate lanes, so the
    // tail of one call's kernels (partial last waves of workgroups) overlaps the next call's head.
    struct Lane {
        hipStream_t stream = nullptr;
        hipStream_t aux = nullptr;                     // second stream + its fork / join events (lone calls: run_pipeline)
        hipEvent_t fork = nullptr, join = nullptr;
        DevBuf ws{8};
        Lane() = default;
        Lane(const Lane&) = delete;
        ~Lane()
        {
            for (hipStream_t s : {stream, aux}) if (s) hipStreamDestroy(s);
            for (hipEvent_t e : {fork, join}) if (e) hipEventDestroy(e);
        }
    };
    Lane lanes[MCR_MAX_INFLIGHT];
    int lane = 0, n_lanes = 4;                        // the current lane: `stream` is its stream, or for a forked half its aux
    bool fork_lone = true;                            // MCR_FORK=0: never fork
    DevBuf stage;                                     // device copy of host tensors (mcr_summarize)
    hipStream_t copy_stream = nullptr;                // uploads of mcr_summarize, overlapped with the lanes' kernels
    // Parquet ingest (mcr_parquet_decode): decompression scratch, page table + page lists + error word
    DevBuf pq_scratch{4}, pq_tab{4};
    DevBuf fs_arena{4};                               // mcr_summarize_files: decoded draws + chain / draw ids
    // The file bytes of an ingest call -- the column chunks or whole images of draws files, the text of CSV files -- and what
    // mcr_csv_stage derives from the text.  gen counts the times any of it was handed out for writing (rewrite, the only way
    // to write it from outside mcr_csv_stage): the handles of mcr_csv_open_paths and the staged tables hold the value they saw.
    struct FileImage {
        PinBuf pin{4};                                // the bytes in pinned host memory (mcr_summarize_files, mcr_csv_*)
        DevBuf dev{4};                                // their device copy
        DevBuf tab{4};                                // staged: FileDesc, chunk -> file, chunk counts / first rows, file_row0
        DevBuf rows{4};                               // staged: start offset of every data row
        uint64_t gen = 0;
        struct File { size_t img, len, body; int ncols; std::string path; };
        std::vector<File> files; std::vector<uint32_t> row0;             // staged files, first data row of each (+ total)
        uint64_t staged_gen = 0; bool staged = false;
        bool table = false;                           // the staged files are table CSVs (mcr_csv_open_table*)
        size_t row0_off = 0;                          // file_row0 within tab
        bool is_staged() const { return staged && staged_gen == gen; }
        // Room for a call's bytes on the device, in pinned memory, and for row starts: whatever was opened or staged is gone.
        int rewrite(mcr_ctx* ctx, size_t dev_bytes, size_t pin_bytes, size_t rows_bytes)
        {
            ++gen;
            int rc = dev.reserve(ctx, dev_bytes);
            if (!rc) rc = pin.reserve(ctx, pin_bytes);
            return rc ? rc : rows.reserve(ctx, rows_bytes);
        }
    } img;
    DevBuf parse_scratch{4};   // a text decoder's call: slot tables, hard list, counters, patch list; mcr_json_open: chunk counts
    DevBuf pow5;               // device copy of csv::kPow5
    DevBuf pow10;              // device copy of csvw::kPow10
    uint32_t csv_hard_cap = 4096;
    int io_threads = 8;                                    // MCR_IO_THREADS: host threads that read the file images and parse their footers
    size_t io_piece = (size_t)2 << 20;                     // MCR_IO_PIECE_KB: the finished prefix is uploaded in pieces of at least this size
    // z tables (k_ztable): a function of M alone, so they are computed once per pooled length and kept for the life of
    // the context instead of being relaunched by every call (most recently used first; a handful of shapes is typical)
    struct ZTab { i64 M; DevBuf tab; };
    std::vector<ZTab> ztabs;
    struct Twiddle { int L; DevBuf tab; };          // exp(-2 pi i t / L), t < L / 2, per sub-transform length (mcr_fft.hpp)
    std::vector<Twiddle> twiddles;
    mcr::host::Slot slots[MCR_MAX_INFLIGHT];
    int next_slot = 0;
    std::vector<int> order;  // busy slots in enqueue order (the summaries in flight)
    bool prof = false;
    std::vector<mcr::host::EvPair> pending;
    std::vector<hipEvent_t> free_ev;
    int64_t k_launches[mcr::host::K_COUNT] = {0};
    double k_ms[mcr::host::K_COUNT] = {0};
    bool fft_on = true;      // MCR_FFT=0: long chains take the direct tier-3 rounds only (A/B measurements, parity tests)
    bool f32_records = true; // MCR_F32_RECORDS=0: f32 tensors take the f64 kernels (widened by the tile sort) instead of the packed records (k_tile_sort32, RecSlots)
    bool splitters_pairwise = false;   // MCR_SPLITTERS_PAIRWISE=1: rank the regular samples pair by pair whatever their number (A/B, parity tests)
    double rho_band = 0;          // MCR_RHO_BAND (mcr_init: kRhoBand): half-width of the guard band of the tier-3 scan (0 = decide on the raw values)
    DevBuf call_dev{4};                // the tensor calls (nested R-hat ... autocorrelation, one at a time): the call's result
                                       // table behind its tail lengths or chain permutation
    PinBuf call_host{4};               // its results (mcr_autocorr: the chains' non-finite counts) on the host
    i64 energy_launch_work = 0;   // MCR_ENERGY_LAUNCH_WORK (mcr_init): pair-parameters of one k_energy_pairs launch (tests lower it)
    DevBuf guard_count;                // device counters (2 unsigned): band lags re-derived the reference's way (mcr_rho_guard_count),
                                       // tiles the tile sort sorted as pairs after all (mcr_tile_fallback_count)
};

namespace mcr {
namespace host {

// Defined once, in mcr_api.hip, where their comments are.
int fail(mcr_ctx* ctx, int code, const char* fmt, ...);
void prof_resolve(mcr_ctx* ctx);
hipError_t sync_all(mcr_ctx* ctx);
int stage_buffers(mcr_ctx* ctx, std::initializer_list<size_t> bytes, void** ptr);

#define HIP_TRY(ctx, call)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(ctx, e_ == hipErrorOutOfMemory ? MCR_ENOMEM : MCR_EHIP, "%s failed: %s", \
                        #call, hipGetErrorString(e_));                                            \
    } while (0)

inline void prof_begin(mcr_ctx* ctx, int kid)
{
    if (!ctx->prof) return;
    EvPair pr{nullptr, nullptr, kid};
    for (hipEvent_t* e : {&pr.a, &pr.b}) {
        if (!ctx->free_ev.empty()) { *e = ctx->free_ev.back(); ctx->free_ev.pop_back(); }
        else if (hipEventCreate(e) != hipSuccess) *e = nullptr;
    }
    if (pr.a && pr.b) { hipEventRecord(pr.a, ctx->stream); ctx->pending.push_back(pr); }
}
inline void prof_end(mcr_ctx* ctx)
{
    if (!ctx->prof || ctx->pending.empty()) return;
    hipEventRecord(ctx->pending.back().b, ctx->stream);
}

#define LAUNCH(ctx, kid, kern, grid, block, smem, ...)                                         \
    do {                                                                                       \
        prof_begin(ctx, kid);                                                                  \
        hipLaunchKernelGGL(kern, grid, block, smem, (ctx)->stream, __VA_ARGS__);               \
        prof_end(ctx);                                                                         \
        hipError_t le_ = hipGetLastError();                                                    \
        if (le_ != hipSuccess)                                                                 \
            return fail(ctx, MCR_EHIP, "launch %s failed: %s", kKernelNames[kid],             \
                        hipGetErrorString(le_));                                               \
    } while (0)

inline void use_lane(mcr_ctx* ctx, int lane)
{
    ctx->lane = lane;
    ctx->stream = ctx->lanes[lane].stream;
}
inline DevBuf& lane_ws(mcr_ctx* ctx) { return ctx->lanes[ctx->lane].ws; }

// The one growth rule.  Large enough: nothing happens.  Otherwise everything that can touch the old allocation finishes
// first (growth is amortised, and hipFree synchronises the device anyway), then the buffer is replaced by one of the new
// size plus its slack, or of the exact size when that is out of memory.  The contents are not kept.
template <bool kPinned> int Buf<kPinned>::reserve(mcr_ctx* ctx, size_t bytes)
{
    if (bytes <= cap) return MCR_OK;
    if (p) HIP_TRY(ctx, sync_all(ctx));
    release();
    auto alloc = [&](size_t n) { return kPinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n); };
    size_t want = bytes + (slack_div ? bytes / slack_div : 0);
    hipError_t e = alloc(want);
    if (e != hipSuccess && want > bytes) { (void)hipGetLastError(); e = alloc(want = bytes); }     // (the launches check the last error)
    if (e != hipSuccess) {
        p = nullptr;
        return fail(ctx, e == hipErrorOutOfMemory ? MCR_ENOMEM : MCR_EHIP, "%s(%zu) failed: %s", kPinned ? "hipHostMalloc" : "hipMalloc",
                    bytes, hipGetErrorString(e));
    }
    cap = want;
    return MCR_OK;
}

// Measures a layout (a callable on a Carve&), makes the buffer that large, then carves it.
template <class Layout> int carve(mcr_ctx* ctx, DevBuf& buf, Layout&& layout)
{
    Carve m{nullptr};
    layout(m);
    const int rc = buf.reserve(ctx, m.off);
    if (rc) return rc;
    Carve cv{buf.as<char>(), buf.cap};
    layout(cv);
    if (cv.over()) return fail(ctx, MCR_ENOMEM, "buffer layout needs %zu bytes; the buffer has %zu", cv.off, cv.end);
    return MCR_OK;
}

// ---- the summary path, as far as mcr_summarize_files enqueues on it (defined in mcr_api.hip, with the comments) ----

struct PipeIn;      // a pipeline's arguments and carved buffers (mcr_pipe.hpp): mcr_api.hip and mcr_stats.hip look inside

// One summary call.  !ragged: a rectangular tensor (C, N, strides), chain c at c * N -- the offset table stays resident
// in the slot between calls of one shape.  ragged: f64 draws with the chains back to back as chain_off says (host, C + 1
// entries), parameter p at draws_dev + p * sp; N, sc and sn are unused and the table goes up with the call.  The members
// with a default are what mcr_diagnose_chains asks for.
struct SummaryCall {
    const void* draws_dev; int dtype; i64 C, N, P, sc, sn, sp;
    const i64* chain_off; bool ragged;
    int min_chains; const double* quantiles; int nq; const mcr_summary* out;
    int slot = -1;              // >= 0: that slot on the current lane, next_slot stays (else: a free slot and the next lane)
    bool always_diag = false;   // the rank and diagnostics kernels whatever `out` asks for
    bool may_fork = true;       // a lone call may put its bulk half on the lane's second stream (ctx->fork_lone)
    int fft_slot_cap = 0;       // > 0: at most so many FFT slots (plan_chunks)
    PipeIn* last = nullptr;     // receives the last chunk's pipeline: its rank codes and the z table
};

int enqueue_impl(mcr_ctx* ctx, const SummaryCall& c);
int wait_one_impl(mcr_ctx* ctx);
int drain(mcr_ctx* ctx, int rc, bool abort = false);
mcr_summary summary_at(mcr_summary r, i64 p0, int nq);

}  // namespace host
}  // namespace mcr
