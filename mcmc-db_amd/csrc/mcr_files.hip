// mcr_files.hip -- the file unit of libmcmcref_hip.so's C ABI (see include/mcmcref_hip.h): Parquet decode and write, CSV
// write, row layout and gather, mcr_summarize_files, and the CSV and JSON text ingest, with their host-side launch logic.
// Of the statistics unit (mcr_api.hip) it uses what mcr_host.hpp declares: the tools of a call and, for
// mcr_summarize_files, the summary path's enqueue and drain.
#include "mcr_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <exception>
#include <memory>
#include <thread>
#include <unordered_map>
#include <functional>
#include <new>

#include "mcr_parquet.hpp"
#include "mcr_pqwrite.hpp"
#include "mcr_csvwrite.hpp"
#include "mcr_layout.hpp"
#include "mcr_csv.hpp"
#include "mcr_json.hpp"

using namespace mcr;
using namespace mcr::host;

extern "C" {

// ---- Parquet ingest (replaces pq.read_table at store.py:79-95 / convert.py:61-65) -----------

struct mcr_parquet { mcr::pq::File f; };
// A chain CSV's header.  owner / gen / img: the image is this context's img.pin + img and already uploaded (mcr_csv_open_paths).
// table / tflags / twhere: a table CSV (mcr_csv_open_table*), its MCR_CSV_T_* header flags and the first one's byte offset.
struct mcr_csv { mcr::csv::Image im; mcr_ctx* owner = nullptr; uint64_t gen = 0; size_t img = 0; bool table = false; int tflags = 0; size_t twhere = 0; };

int mcr_parquet_open(mcr_ctx* ctx, const void* bytes, size_t len, mcr_parquet** out)
{
    if (!bytes || !out) return fail(ctx, MCR_EINVAL, "NULL argument");     // ctx may be NULL: parsing needs no device
    mcr_parquet* f = new (std::nothrow) mcr_parquet();
    if (!f) return fail(ctx, MCR_ENOMEM, "out of host memory");
    bool ok = false;
    try { ok = mcr::pq::open(f->f, bytes, len); }
    catch (const std::exception& e) { f->f.error = std::string("host allocation failed: ") + e.what(); }
    if (!ok) {
        const int rc = fail(ctx, MCR_EINVAL, "parquet: %s", f->f.error.c_str());
        delete f;
        return rc;
    }
    *out = f;
    return MCR_OK;
}

void mcr_parquet_close(mcr_parquet* f) { delete f; }
int64_t mcr_parquet_num_rows(const mcr_parquet* f) { return f ? f->f.num_rows : -1; }
int mcr_parquet_num_columns(const mcr_parquet* f) { return f ? (int)f->f.cols.size() : -1; }
const char* mcr_parquet_column_name(const mcr_parquet* f, int col)
{
    return (f && col >= 0 && col < (int)f->f.cols.size()) ? f->f.cols[col].name.c_str() : nullptr;
}
int mcr_parquet_column_type(const mcr_parquet* f, int col)
{
    return (f && col >= 0 && col < (int)f->f.cols.size()) ? f->f.cols[col].type : -1;
}

int mcr_parquet_num_pages(const mcr_parquet* f) { return f ? (int)f->f.pages.size() : -1; }
int mcr_parquet_page_info(const mcr_parquet* f, int page, int64_t* info)
{
    if (!f || !info || page < 0 || page >= (int)f->f.pages.size()) return MCR_EINVAL;
    const mcr::pq::Page& p = f->f.pages[page];
    info[0] = p.col; info[1] = p.kind; info[2] = p.encoding; info[3] = p.codec; info[4] = (int64_t)p.payload_off;
    info[5] = p.comp_size; info[6] = p.uncomp_size; info[7] = p.num_values; info[8] = (int64_t)p.row_off; info[9] = p.dict;
    return MCR_OK;
}

namespace {
// A batched decode in three steps: pq_plan (host only: byte spans to stage, page table), pq_buffers (device buffers +
// table uploads), pq_launch (the two kernels).  The caller makes room for the file bytes first (FileImage::rewrite) and
// stages the spans at img.dev + span.stage_off before the launch: mcr_parquet_decode copies them from the caller's file image (pageable memory),
// mcr_summarize_files reads them into pinned memory on host threads and uploads behind them.
struct PqSpan { const mcr::pq::File* f; u64 start, end; size_t stage_off; };
struct PqPlan {
    std::vector<PqSpan> merged;
    size_t stage_total = 0, scratch_total = 0;
    std::vector<mcr::pq::PageDev> tab;
    std::vector<int> l_snappy, l_decode;
    mcr::pq::PageDev* d_tab = nullptr; int* d_ls = nullptr; int* d_ld = nullptr; int* d_err = nullptr;
};

// whole_files: (file, offset of its whole image in the staging buffer) sorted by file pointer, and the total staged
// bytes -- the caller stages whole file images instead of the packed column chunks (mcr_summarize_files, which wants
// nearly every byte of every file anyway and starts uploading before the footers are parsed).
using FileBase = std::pair<const mcr::pq::File*, size_t>;
int pq_plan(mcr_ctx* ctx, const mcr_parquet_request* reqs, int n_reqs, PqPlan& P,
            const std::vector<FileBase>* whole_files = nullptr, size_t whole_total = 0)
{
    namespace pq = mcr::pq;
    std::vector<PqSpan> spans;
    std::vector<pq::PageDev>& tab = P.tab;
    // 1. byte spans to upload: the column chunks of the requested columns, merged when (nearly) adjacent
    for (int r = 0; r < n_reqs; ++r) {
        const mcr_parquet_request& q = reqs[r];
        if (!q.file) return fail(ctx, MCR_EINVAL, "request %d: file is NULL", r);
        const pq::File& f = q.file->f;
        if (q.column < 0 || q.column >= (int)f.cols.size()) return fail(ctx, MCR_EINVAL, "request %d: column %d out of range", r, q.column);
        const pq::Column& col = f.cols[q.column];
        if (col.type != pq::T_INT32 && col.type != pq::T_INT64 && col.type != pq::T_FLOAT && col.type != pq::T_DOUBLE)
            return fail(ctx, MCR_EINVAL, "parquet: column '%s' has physical type %d; only INT32, INT64, FLOAT and DOUBLE columns are decoded", col.name.c_str(), col.type);
        if (q.out_kind != MCR_PQ_F64 && q.out_kind != MCR_PQ_I64) return fail(ctx, MCR_EINVAL, "request %d: bad out_kind %d", r, q.out_kind);
        if (q.out_kind == MCR_PQ_I64 && col.type != pq::T_INT32 && col.type != pq::T_INT64)
            return fail(ctx, MCR_EINVAL, "parquet: column '%s' is not an integer column", col.name.c_str());
        if (f.num_rows > 0 && !q.out_dev) return fail(ctx, MCR_EINVAL, "request %d: out_dev is NULL", r);
        for (const pq::Chunk& ch : f.chunks)
            if (ch.col == q.column && ch.end > ch.start) spans.push_back(PqSpan{&f, ch.start, ch.end, 0});
    }
    std::sort(spans.begin(), spans.end(), [](const PqSpan& a, const PqSpan& b) {
        return a.f != b.f ? std::less<const pq::File*>()(a.f, b.f) : a.start < b.start; });
    std::vector<PqSpan>& merged = P.merged;
    for (const PqSpan& s : spans) {
        if (!merged.empty() && merged.back().f == s.f && s.start <= merged.back().end + 4096) {
            if (s.end > merged.back().end) merged.back().end = s.end;
        } else merged.push_back(s);
    }
    size_t stage_total = 0;
    if (whole_files) {
        for (PqSpan& s : merged) {
            auto it = std::lower_bound(whole_files->begin(), whole_files->end(), s.f, [](const FileBase& a, const mcr::pq::File* key) {
                return std::less<const mcr::pq::File*>()(a.first, key); });
            if (it == whole_files->end() || it->first != s.f) return fail(ctx, MCR_EINVAL, "parquet: request on a file that is not staged");
            s.stage_off = it->second + (size_t)s.start;
        }
        stage_total = whole_total;
    } else {
        for (PqSpan& s : merged) { s.stage_off = align_up(stage_total, 256); stage_total = s.stage_off + (size_t)(s.end - s.start); }
    }
    P.stage_total = stage_total;
    // staged position of the file bytes [off, off + n): the WHOLE payload must lie inside one uploaded span
    // (spans are sorted by (file, start): binary search for the file's first span, then a short walk)
    auto stage_of = [&](const pq::File* f, u64 off, u64 n) -> size_t {
        auto it = std::lower_bound(merged.begin(), merged.end(), f, [](const PqSpan& s, const pq::File* key) {
            return std::less<const pq::File*>()(s.f, key); });
        for (; it != merged.end() && it->f == f; ++it)
            if (off >= it->start && off + n <= it->end) return it->stage_off + (size_t)(off - it->start);
        return (size_t)-1;
    };
    // 2. page table
    size_t scratch_total = 0;
    for (int r = 0; r < n_reqs; ++r) {
        const mcr_parquet_request& q = reqs[r];
        const pq::File& f = q.file->f;
        const pq::Column& col = f.cols[q.column];
        const u32 es = (col.type == pq::T_INT64 || col.type == pq::T_DOUBLE) ? 8 : 4;
        for (const pq::Chunk& ch : f.chunks) {
            if (ch.col != q.column) continue;
            int dict_idx = -1;
            for (int k = 0; k < ch.n_pages; ++k) {
                const pq::Page& pg = f.pages[(size_t)ch.first_page + k];
                if (pg.codec != pq::CODEC_NONE && pg.codec != pq::CODEC_SNAPPY)
                    return fail(ctx, MCR_EINVAL, "parquet: column '%s' uses compression codec %d; only UNCOMPRESSED and SNAPPY are decoded", col.name.c_str(), pg.codec);
                pq::PageDev d; memset(&d, 0, sizeof(d));
                const bool v2 = pg.kind == pq::PAGE_DATA_V2;
                const u32 lvl = v2 ? pg.rep_bytes + pg.def_bytes : 0;
                const bool comp = pg.codec == pq::CODEC_SNAPPY && (!v2 || pg.v2_compressed);
                if (pg.uncomp_size < lvl) return fail(ctx, MCR_EINVAL, "parquet: v2 page smaller than its levels");
                d.src_off = stage_of(&f, pg.payload_off, pg.comp_size);
                if (pg.comp_size > 0 && d.src_off == (u64)(size_t)-1) return fail(ctx, MCR_EINVAL, "parquet: page outside its column chunk");
                d.comp_size = pg.comp_size - lvl; d.uncomp_size = pg.uncomp_size - lvl;
                d.num_values = pg.num_values; d.lvl_bytes = lvl; d.def_bytes = v2 ? pg.def_bytes : 0;
                d.kind = (unsigned char)pg.kind; d.compressed = comp ? 1 : 0; d.phys_type = (unsigned char)col.type;
                d.max_def = (unsigned char)((v2 && pg.def_bytes == 0) ? 0 : col.max_def);   // v2 without level bytes: all defined
                d.out_kind = (unsigned char)q.out_kind;
                d.dict_page = -1;
                if (v2 && pg.rep_bytes) return fail(ctx, MCR_EINVAL, "parquet: repetition levels in a flat column");
                if (!comp && d.comp_size != d.uncomp_size) return fail(ctx, MCR_EINVAL, "parquet: uncompressed page with differing sizes");
                if (comp) { d.dst_off = align_up(scratch_total, 16); scratch_total = (size_t)d.dst_off + d.uncomp_size + 16; }
                if (pg.kind == pq::PAGE_DICT) {
                    if (pg.encoding != pq::ENC_PLAIN && pg.encoding != pq::ENC_PLAIN_DICT)
                        return fail(ctx, MCR_EINVAL, "parquet: dictionary page encoding %d is not supported", pg.encoding);
                    if ((u64)pg.num_values * es > d.uncomp_size) return fail(ctx, MCR_EINVAL, "parquet: dictionary page shorter than its entries");
                    d.encoding = pq::ENC_PLAIN;
                    dict_idx = (int)tab.size();
                } else {
                    if (pg.encoding == pq::ENC_PLAIN) d.encoding = pq::ENC_PLAIN;
                    else if (pg.encoding == pq::ENC_RLE_DICT || pg.encoding == pq::ENC_PLAIN_DICT) {
                        if (pg.dict < 0 || dict_idx < 0) return fail(ctx, MCR_EINVAL, "parquet: dictionary-encoded page without a dictionary page");
                        d.encoding = pq::ENC_RLE_DICT; d.dict_page = dict_idx; d.dict_count = pg.dict_count;
                    } else
                        return fail(ctx, MCR_EINVAL, "parquet: column '%s' uses value encoding %d; only PLAIN and RLE_DICTIONARY are decoded", col.name.c_str(), pg.encoding);
                    d.out = q.out_dev; d.out_off = pg.row_off;
                    P.l_decode.push_back((int)tab.size());
                }
                if (comp) P.l_snappy.push_back((int)tab.size());
                tab.push_back(d);
            }
        }
    }
    P.scratch_total = scratch_total;
    return MCR_OK;
}

// 3. device buffers + the page table and the two page lists, on ctx->stream.  The staged bytes' buffer is the caller's to
//    size (pq_stage_bytes: it may be uploading into it already), never reallocated here.
inline size_t pq_stage_bytes(size_t staged) { return staged + mcr::pq::kInWin + 256; }    // the kernels' read window behind the end
int pq_buffers(mcr_ctx* ctx, PqPlan& P)
{
    namespace pq = mcr::pq;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->img.dev.cap < pq_stage_bytes(P.stage_total))
        return fail(ctx, MCR_EINVAL, "parquet: the plan stages %zu bytes; the caller made room for %zu", pq_stage_bytes(P.stage_total), ctx->img.dev.cap);
    int rc = ctx->pq_scratch.reserve(ctx, P.scratch_total + 256);
    if (rc) return rc;
    const size_t tab_bytes = align_up(P.tab.size() * sizeof(pq::PageDev), 256);
    const size_t ls_bytes = align_up(P.l_snappy.size() * 4 + 4, 256), ld_bytes = align_up(P.l_decode.size() * 4 + 4, 256);
    rc = ctx->pq_tab.reserve(ctx, tab_bytes + ls_bytes + ld_bytes + 256);
    if (rc) return rc;
    char* tb = ctx->pq_tab.as<char>();
    P.d_tab = (pq::PageDev*)tb;
    P.d_ls = (int*)(tb + tab_bytes); P.d_ld = (int*)(tb + tab_bytes + ls_bytes);
    P.d_err = (int*)(tb + tab_bytes + ls_bytes + ld_bytes);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(ctx->img.dev.as<char>() + P.stage_total, 0, pq::kInWin + 256, st));
    if (!P.tab.empty()) HIP_TRY(ctx, hipMemcpyAsync(P.d_tab, P.tab.data(), P.tab.size() * sizeof(pq::PageDev), hipMemcpyHostToDevice, st));
    if (!P.l_snappy.empty()) HIP_TRY(ctx, hipMemcpyAsync(P.d_ls, P.l_snappy.data(), P.l_snappy.size() * 4, hipMemcpyHostToDevice, st));
    if (!P.l_decode.empty()) HIP_TRY(ctx, hipMemcpyAsync(P.d_ld, P.l_decode.data(), P.l_decode.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(P.d_err, 0, 8, st));
    return MCR_OK;
}

int pq_launch(mcr_ctx* ctx, const PqPlan& P)
{
    namespace pq = mcr::pq;
    if (!P.l_snappy.empty())
        LAUNCH(ctx, K_PQ_SNAPPY, pq::k_pq_snappy, dim3((unsigned)P.l_snappy.size()), dim3(64), 0, ctx->img.dev.as<const unsigned char>(),
               ctx->pq_scratch.as<unsigned char>(), (const pq::PageDev*)P.d_tab, (const int*)P.d_ls, P.d_err);
    if (!P.l_decode.empty())
        LAUNCH(ctx, K_PQ_DECODE, pq::k_pq_decode, dim3((unsigned)P.l_decode.size()), dim3(256), 0, ctx->img.dev.as<const unsigned char>(),
               ctx->pq_scratch.as<const unsigned char>(), (const pq::PageDev*)P.d_tab, (const int*)P.d_ld, P.d_err);
    return MCR_OK;
}

int pq_error(mcr_ctx* ctx, const int* h_err)
{
    if (!h_err[0]) return MCR_OK;
    static const char* const what[] = {"", "corrupt Snappy stream", "null values are not supported", "corrupt definition levels",
                                       "corrupt RLE / bit-packed runs", "dictionary index out of range", "page shorter than its values"};
    const int c = h_err[0];
    return fail(ctx, MCR_EINVAL, "parquet: %s (page %d of the request)", (c > 0 && c < 7) ? what[c] : "decode error", h_err[1]);
}
}  // namespace

int mcr_parquet_decode(mcr_ctx* ctx, const mcr_parquet_request* reqs, int n_reqs)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (n_reqs < 0 || (n_reqs > 0 && !reqs)) return fail(ctx, MCR_EINVAL, "bad request list");
    if (n_reqs == 0) return MCR_OK;
    try {
        PqPlan P;
        int rc = pq_plan(ctx, reqs, n_reqs, P);
        if (rc) return rc;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        rc = ctx->img.rewrite(ctx, pq_stage_bytes(P.stage_total), 0, 0);
        if (!rc) rc = pq_buffers(ctx, P);
        if (rc) return rc;
        hipStream_t st = ctx->stream;
        for (const PqSpan& s : P.merged)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->img.dev.as<char>() + s.stage_off, s.f->bytes + s.start, (size_t)(s.end - s.start), hipMemcpyHostToDevice, st));
        rc = pq_launch(ctx, P);
        if (rc) return rc;
        int h_err[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(h_err, P.d_err, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        prof_resolve(ctx);
        rc = pq_error(ctx, h_err);
        if (rc) return rc;
    } catch (const std::exception& e) {
        return fail(ctx, MCR_ENOMEM, "parquet: host allocation failed: %s", e.what());
    }
    return MCR_OK;
}

int mcr_gather_rows_dev(mcr_ctx* ctx, const double* src_dev, int64_t P, int64_t M, const int64_t* order, double* dst_dev)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || M < 0 || P > kMaxGridY) return fail(ctx, MCR_EINVAL, "bad shape");
    if (P == 0 || M == 0) return MCR_OK;
    if (!src_dev || !dst_dev || !order) return fail(ctx, MCR_EINVAL, "NULL argument");
    if (src_dev == dst_dev) return fail(ctx, MCR_EINVAL, "gather cannot run in place");
    for (i64 k = 0; k < M; ++k) if (order[k] < 0 || order[k] >= M) return fail(ctx, MCR_EINVAL, "order[%lld] out of range", (long long)k);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    i64* d_order = nullptr;
    const int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { d_order = cv.take<i64>((size_t)M); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_order, order, (size_t)M * 8, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, K_GATHER, mcr::pq::k_gather_rows, dim3((unsigned)((M + 255) / 256), (unsigned)P), dim3(256), 0, src_dev,
           (const i64*)d_order, (i64)M, dst_dev);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

// ---- Parquet writing (mcr_pqwrite.hpp; replaces pq.write_table at convert.py:64) --------------------------------

struct mcr_pq_image { unsigned char* data = nullptr; size_t size = 0; int pages = 0; bool pinned = false; };

namespace {
namespace pqw = mcr::pqw;
static_assert(pqw::kPageRows == MCR_PQW_PAGE_ROWS && pqw::kRowGroupRows == MCR_PQW_ROW_GROUP_ROWS, "the header states the page geometry");
static_assert(pqw::SRC_F64 == MCR_PQW_F64 && pqw::SRC_I64 == MCR_PQW_I64 && pqw::SRC_SEQ == MCR_PQW_SEQ, "source kinds");

struct PqwJob {
    std::vector<pqw::ColSpec> specs; std::vector<pqw::ColDev> cols; std::vector<pqw::PagePlan> pages;
    std::vector<u64> slot_off; size_t slots_total = 0;
};

int pqw_args(mcr_ctx* ctx, const char* who, const mcr_pq_column* cols, int n_cols, int64_t rows, int64_t row_group_rows,
             mcr_pq_image** out, PqwJob& J)
{
    namespace pq = mcr::pq;
    if (!cols || !out || n_cols < 1) return fail(ctx, MCR_EINVAL, "%s: NULL argument or no columns", who);
    if (rows <= 0 || rows >= (int64_t)1 << 31) return fail(ctx, MCR_EINVAL, "%s: row count %lld out of range (1 .. 2^31 - 1)", who, (long long)rows);
    if (row_group_rows < 0) return fail(ctx, MCR_EINVAL, "%s: negative row_group_rows", who);
    std::vector<int> types;
    for (int c = 0; c < n_cols; ++c) {
        const mcr_pq_column& q = cols[c];
        if (!q.name || !*q.name) return fail(ctx, MCR_EINVAL, "%s: column %d has an empty name", who, c);
        for (int b = 0; b < c; ++b)
            if (strcmp(cols[b].name, q.name) == 0) return fail(ctx, MCR_EINVAL, "%s: duplicate column name '%s'", who, q.name);
        if (q.type != MCR_PQ_INT32 && q.type != MCR_PQ_INT64 && q.type != MCR_PQ_DOUBLE)
            return fail(ctx, MCR_EINVAL, "%s: column '%s' has type %d; only INT32, INT64 and DOUBLE are written", who, q.name, q.type);
        if (q.src_kind == MCR_PQW_F64 || q.src_kind == MCR_PQW_I64) {
            if (!q.src_dev || q.stride < 1) return fail(ctx, MCR_EINVAL, "%s: column '%s' needs a source and a stride >= 1", who, q.name);
        } else if (q.src_kind == MCR_PQW_SEQ) {
            if (q.seq_div < 1 || q.seq_mod < 1) return fail(ctx, MCR_EINVAL, "%s: column '%s' needs seq_div >= 1 and seq_mod >= 1", who, q.name);
        } else return fail(ctx, MCR_EINVAL, "%s: column '%s' has source kind %d", who, q.name, q.src_kind);
        if (q.src_kind != MCR_PQW_F64 && q.type == MCR_PQ_DOUBLE)
            return fail(ctx, MCR_EINVAL, "%s: column '%s': an integer source is written as INT32 or INT64", who, q.name);
        J.specs.push_back(pqw::ColSpec{q.name, q.type});
        J.cols.push_back(pqw::ColDev{q.src_dev, (i64)q.stride, (i64)q.seq_div, (i64)q.seq_mod, q.src_kind, q.type});
        types.push_back(q.type);
    }
    pqw::plan_pages(n_cols, types.data(), (i64)rows, row_group_rows ? (i64)row_group_rows : pqw::kRowGroupRows, J.pages);
    if (J.pages.size() > (size_t)0x3FFFFFFF) return fail(ctx, MCR_EINVAL, "%s: too many pages", who);
    for (const pqw::PagePlan& p : J.pages) { J.slot_off.push_back(J.slots_total); J.slots_total += pqw::slot_bytes(p.uncomp); }
    return MCR_OK;
}

int pqw_bad_value(mcr_ctx* ctx, const char* who, const PqwJob& J, int col, long long row)
{
    const int t = J.specs[col].type;
    return fail(ctx, MCR_EINVAL, "%s: column '%s', row %lld: the value is not an integer or is outside the range of %s", who,
                J.specs[col].name.c_str(), row, t == MCR_PQ_INT32 ? "INT32" : "INT64");
}
}  // namespace

int mcr_parquet_write_dev(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, int64_t row_group_rows,
                          mcr_pq_image** out)
{
    static const char* who = "mcr_parquet_write_dev";
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "%s with summaries in flight", who);
    mcr_pq_image* img = nullptr;
    try {
        PqwJob J;
        int rc = pqw_args(ctx, who, cols, n_cols, rows, row_group_rows, out, J);
        if (rc) return rc;
        *out = nullptr;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t np = J.pages.size(), bound = pqw::image_bound(J.specs, J.pages), blob_cap = bound - J.slots_total;
        pqw::ColDev* d_cols; pqw::PageW* d_pages; pqw::PageRec* d_recs; unsigned long long* d_err; pqw::Seg* d_segs;
        unsigned char *d_slots, *d_blob, *d_image;
        rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) {
            d_cols = cv.take<pqw::ColDev>((size_t)n_cols); d_pages = cv.take<pqw::PageW>(np); d_recs = cv.take<pqw::PageRec>(np);
            d_err = cv.take<unsigned long long>((size_t)n_cols); d_segs = cv.take<pqw::Seg>(2 * np + 2);
            d_slots = cv.take<unsigned char>(J.slots_total); d_blob = cv.take<unsigned char>(blob_cap);
            d_image = cv.take<unsigned char>(bound);
        });
        if (rc) return rc;
        std::vector<pqw::PageW> h_pages(np);
        for (size_t k = 0; k < np; ++k) h_pages[k] = pqw::PageW{J.pages[k].col, J.pages[k].nrows, J.pages[k].row0, J.slot_off[k]};
        std::vector<pqw::PageRec> recs(np);
        std::vector<unsigned long long> h_err((size_t)n_cols);
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemcpyAsync(d_cols, J.cols.data(), sizeof(pqw::ColDev) * (size_t)n_cols, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_pages, h_pages.data(), sizeof(pqw::PageW) * np, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(d_err, 0xFF, 8 * (size_t)n_cols, st));
        LAUNCH(ctx, K_PQW_ENCODE, pqw::k_pqw_encode, dim3((unsigned)np), dim3(pqw::kNT), 0, (const pqw::ColDev*)d_cols,
               (const pqw::PageW*)d_pages, d_slots, d_recs, d_err);
        HIP_TRY(ctx, hipMemcpyAsync(recs.data(), d_recs, sizeof(pqw::PageRec) * np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(h_err.data(), d_err, 8 * (size_t)n_cols, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int c = 0; c < n_cols; ++c)
            if (h_err[c] != ~0ull) { prof_resolve(ctx); return pqw_bad_value(ctx, who, J, c, (long long)h_err[c]); }
        pqw::Layout L;
        pqw::build_layout(J.specs, J.pages, recs, J.slot_off, (i64)rows, MCR_VERSION, L);
        if (L.blob.size() > blob_cap || L.image_bytes > bound || L.segs.size() > 2 * np + 2) {
            prof_resolve(ctx);
            return fail(ctx, MCR_ENOMEM, "%s: the file image (%zu bytes) exceeds its bound (%zu)", who, L.image_bytes, bound);
        }
        for (size_t k = 0; k < np; ++k)
            if (recs[k].comp_size > pqw::slot_bytes(J.pages[k].uncomp)) return prof_resolve(ctx), fail(ctx, MCR_EHIP, "%s: page %zu overran its slot", who, k);
        img = new mcr_pq_image();
        img->size = L.image_bytes; img->pages = (int)np; img->pinned = true;
        {
            const hipError_t e = hipHostMalloc((void**)&img->data, L.image_bytes, hipHostMallocDefault);
            if (e != hipSuccess) { delete img; return fail(ctx, MCR_ENOMEM, "hipHostMalloc(%zu) failed: %s", L.image_bytes, hipGetErrorString(e)); }
        }
        auto drop = [&](int code) { hipHostFree(img->data); delete img; return code; };
        hipError_t e = hipMemcpyAsync(d_blob, L.blob.data(), L.blob.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_segs, L.segs.data(), sizeof(pqw::Seg) * L.segs.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return drop(fail(ctx, MCR_EHIP, "%s: upload failed: %s", who, hipGetErrorString(e)));
        prof_begin(ctx, K_PQW_COMPACT);
        hipLaunchKernelGGL(pqw::k_pqw_compact, dim3((unsigned)L.segs.size()), dim3(256), 0, st, (const pqw::Seg*)d_segs,
                           (const unsigned char*)d_slots, (const unsigned char*)d_blob, d_image);
        prof_end(ctx);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(img->data, d_image, L.image_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        prof_resolve(ctx);
        if (e != hipSuccess) return drop(fail(ctx, MCR_EHIP, "%s: compaction failed: %s", who, hipGetErrorString(e)));
        *out = img;
    } catch (const std::exception& ex) {
        return fail(ctx, MCR_ENOMEM, "%s: host allocation failed: %s", who, ex.what());
    }
    return MCR_OK;
}

int mcr_parquet_write_host(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, int64_t row_group_rows,
                           mcr_pq_image** out)
{
    static const char* who = "mcr_parquet_write_host";
    try {
        PqwJob J;
        int rc = pqw_args(ctx, who, cols, n_cols, rows, row_group_rows, out, J);
        if (rc) return rc;
        *out = nullptr;
        const size_t np = J.pages.size();
        std::vector<unsigned char> payload;
        std::vector<pqw::PageRec> recs(np);
        std::vector<u64> at(np);
        long long bad_row = -1; int bad_col = -1;
        for (size_t k = 0; k < np; ++k) {
            const pqw::PagePlan& p = J.pages[k];
            at[k] = payload.size();
            const i64 bad = pqw::encode_page_host(J.cols[p.col], pqw::PageW{p.col, p.nrows, p.row0, 0}, payload, recs[k]);
            if (bad >= 0 && (bad_col < 0 || p.col < bad_col || (p.col == bad_col && bad < bad_row))) { bad_col = p.col; bad_row = bad; }
            if (bad >= 0) recs[k].comp_size = 0;
        }
        if (bad_col >= 0) return pqw_bad_value(ctx, who, J, bad_col, bad_row);
        pqw::Layout L;
        pqw::build_layout(J.specs, J.pages, recs, at, (i64)rows, MCR_VERSION, L);
        mcr_pq_image* img = new mcr_pq_image();
        img->data = (unsigned char*)malloc(L.image_bytes);
        if (!img->data) { delete img; return fail(ctx, MCR_ENOMEM, "%s: out of host memory", who); }
        img->size = L.image_bytes; img->pages = (int)np;
        for (const pqw::Seg& sg : L.segs)
            memcpy(img->data + sg.dst_off, (sg.from_blob ? L.blob.data() : payload.data()) + sg.src_off, sg.len);
        *out = img;
    } catch (const std::exception& ex) {
        return fail(ctx, MCR_ENOMEM, "%s: host allocation failed: %s", who, ex.what());
    }
    return MCR_OK;
}

const void* mcr_pq_image_data(const mcr_pq_image* im) { return im ? im->data : nullptr; }
size_t mcr_pq_image_size(const mcr_pq_image* im) { return im ? im->size : 0; }
int mcr_pq_image_pages(const mcr_pq_image* im) { return im ? im->pages : -1; }
void mcr_pq_image_free(mcr_pq_image* im)
{
    if (!im) return;
    if (im->pinned) hipHostFree(im->data); else free(im->data);
    delete im;
}

// ---- CSV writing (mcr_csvwrite.hpp; replaces pacsv.write_csv of the reference's draws command, cli.py:100-127) ------

struct mcr_text_image { PinBuf pin; std::vector<unsigned char> host; size_t size = 0; bool pinned = false; };

namespace {
namespace csvw = mcr::csvw;
static_assert(csvw::kTileFields == MCR_CSVW_TILE_FIELDS && csvw::kFieldMax == MCR_CSVW_FIELD_MAX && csvw::kSelectNT == MCR_SELECT_BLOCK_ROWS,
              "the header states the tile geometry");
static_assert(csvw::HEADER_QUOTED == MCR_CSVW_HEADER_QUOTED && csvw::HEADER_PLAIN == MCR_CSVW_HEADER_PLAIN && csvw::HEADER_NONE == MCR_CSVW_HEADER_NONE,
              "header modes");

struct CsvwJob {
    std::vector<std::string> names; std::vector<pqw::ColDev> cols; std::vector<unsigned char> header;
    csvw::Tiling tiling; i64 count = 0;       // rows to write
};

int csvw_args(mcr_ctx* ctx, const char* who, const mcr_pq_column* cols, int n_cols, int64_t rows, const int64_t* index, int64_t n_index,
              int header, mcr_text_image** out, CsvwJob& J)
{
    namespace pq = mcr::pq;
    if (!cols || !out) return fail(ctx, MCR_EINVAL, "%s: NULL argument", who);
    if (n_cols < 1) return fail(ctx, MCR_EINVAL, "%s: n_cols = %d; at least one column is needed", who, n_cols);
    if (rows < 0 || rows >= (int64_t)1 << 31) return fail(ctx, MCR_EINVAL, "%s: row count %lld out of range (0 .. 2^31 - 1)", who, (long long)rows);
    if (index && (n_index < 0 || n_index >= (int64_t)1 << 31))
        return fail(ctx, MCR_EINVAL, "%s: row list length %lld out of range (0 .. 2^31 - 1)", who, (long long)n_index);
    if (header != MCR_CSVW_HEADER_QUOTED && header != MCR_CSVW_HEADER_PLAIN && header != MCR_CSVW_HEADER_NONE)
        return fail(ctx, MCR_EINVAL, "%s: header mode %d", who, header);
    for (int c = 0; c < n_cols; ++c) {
        const mcr_pq_column& q = cols[c];
        if (!q.name) return fail(ctx, MCR_EINVAL, "%s: column %d has no name", who, c);
        if (header == MCR_CSVW_HEADER_PLAIN && strpbrk(q.name, "\",\r\n"))
            return fail(ctx, MCR_EINVAL, "%s: column '%s' cannot be written in a plain header (quote, comma or line end in the name)", who, q.name);
        if (q.type != MCR_PQ_INT32 && q.type != MCR_PQ_INT64 && q.type != MCR_PQ_DOUBLE)
            return fail(ctx, MCR_EINVAL, "%s: column '%s' has type %d; only INT32, INT64 and DOUBLE are written", who, q.name, q.type);
        if (q.src_kind == MCR_PQW_F64 || q.src_kind == MCR_PQW_I64) {
            if (q.stride < 1) return fail(ctx, MCR_EINVAL, "%s: column '%s' has stride %lld; a stride >= 1 is needed", who, q.name, (long long)q.stride);
            if (!q.src_dev && rows > 0) return fail(ctx, MCR_EINVAL, "%s: column '%s' has no source", who, q.name);
        } else if (q.src_kind == MCR_PQW_SEQ) {
            if (q.seq_div < 1 || q.seq_mod < 1) return fail(ctx, MCR_EINVAL, "%s: column '%s' needs seq_div >= 1 and seq_mod >= 1", who, q.name);
        } else return fail(ctx, MCR_EINVAL, "%s: column '%s' has source kind %d", who, q.name, q.src_kind);
        if (q.src_kind != MCR_PQW_F64 && q.type == MCR_PQ_DOUBLE)
            return fail(ctx, MCR_EINVAL, "%s: column '%s': an integer source is written as INT32 or INT64", who, q.name);
        J.names.push_back(q.name);
        J.cols.push_back(pqw::ColDev{q.src_dev, (i64)q.stride, (i64)q.seq_div, (i64)q.seq_mod, q.src_kind,
                                     q.type == MCR_PQ_DOUBLE ? pq::T_DOUBLE : pq::T_INT64});
    }
    J.tiling = csvw::make_tiling(n_cols);
    J.count = index ? (i64)n_index : (i64)rows;
    csvw::put_header(J.names, header, J.header);
    return MCR_OK;
}

// err as k_csvw_format leaves it
int csvw_bad(mcr_ctx* ctx, const char* who, const CsvwJob& J, const unsigned long long* err, i64 rows)
{
    if (err[0] != ~0ull)
        return fail(ctx, MCR_EINVAL, "%s: entry %llu of the row list is outside the source's rows (0 .. %lld)", who, err[0], (long long)rows - 1);
    const unsigned long long nc = (unsigned long long)J.cols.size();
    return fail(ctx, MCR_EINVAL, "%s: column '%s', row %llu of the output: the value is not an integer", who, J.names[err[1] % nc].c_str(), err[1] / nc);
}

int ensure_pow10(mcr_ctx* ctx)
{
    if (ctx->pow10.p) return MCR_OK;
    const int rc = ctx->pow10.reserve(ctx, sizeof(csvw::kPow10));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->pow10.p, csvw::kPow10, sizeof(csvw::kPow10), hipMemcpyHostToDevice));
    return MCR_OK;
}

struct CsvwBufs { pqw::ColDev* cols; unsigned long long* err; u32* sizes; u64* offs; unsigned char *slots, *image; };
constexpr i64 kCsvwMaxTiles = (i64)1 << 30;       // of one launch

// The one layout of a row range's workspace: nr rows of the job.
void carve_csvw(Carve& cv, const CsvwJob& J, i64 nr, CsvwBufs& b)
{
    const size_t nt = (size_t)csvw::tile_count(J.tiling, nr);
    b.cols = cv.take<pqw::ColDev>(J.cols.size()); b.err = cv.take<unsigned long long>(2);
    b.sizes = cv.take<u32>(nt); b.offs = cv.take<u64>(nt + 1);
    b.slots = cv.take<unsigned char>(nt * csvw::slot_bytes(J.tiling));
    b.image = cv.take<unsigned char>((size_t)nr * J.cols.size() * csvw::kFieldMax);
}
}  // namespace

int mcr_csv_write_dev(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, const int64_t* index_dev, int64_t n_index,
                      int header, mcr_text_image** out)
{
    static const char* who = "mcr_csv_write_dev";
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "%s with summaries in flight", who);
    try {
        CsvwJob J;
        int rc = csvw_args(ctx, who, cols, n_cols, rows, index_dev, n_index, header, out, J);
        if (rc) return rc;
        *out = nullptr;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        rc = ensure_pow10(ctx);
        if (rc) return rc;
        std::unique_ptr<mcr_text_image> img(new mcr_text_image());
        img->pinned = true;
        const size_t hdr = J.header.size();
        const i64 count = J.count;
        auto measure = [&](i64 nr) { Carve m{nullptr}; CsvwBufs b; carve_csvw(m, J, nr, b); return m.off; };
        // rows per range: all of them, or the most whole tiles whose layout fits the workspace limit
        const i64 step = J.tiling.R;
        i64 per = count;
        if (count > 0) {
            auto fits = [&](i64 k) { const i64 nr = std::min(count, k * step); return measure(nr) <= ctx->ws_limit && csvw::tile_count(J.tiling, nr) <= kCsvwMaxTiles; };
            const i64 k = most_that_fit((count + step - 1) / step, fits);
            if (!k) return fail(ctx, MCR_ENOMEM, "%s: %lld row(s) of %d columns need %zu bytes of workspace; limit is %zu", who, (long long)step,
                                n_cols, measure(std::min(count, step)), ctx->ws_limit);
            per = std::min(count, k * step);
        }
        size_t used = 0;
        // room for `need` bytes of the image (or `hint`, when that is more), the first `used` kept
        auto ensure = [&](size_t need, size_t hint) {
            if (need <= img->pin.cap) return (int)MCR_OK;
            PinBuf grown;
            const int rc2 = grown.reserve(ctx, std::max(need, hint));
            if (rc2) return rc2;
            if (used) memcpy(grown.p, img->pin.p, used);
            img->pin = std::move(grown);
            return (int)MCR_OK;
        };
        auto with_header = [&](size_t body, size_t hint) {
            if (used || hdr + body == 0) return ensure(used + body, hint);
            const int rc2 = ensure(hdr + body, hint);
            if (rc2) return rc2;
            memcpy(img->pin.p, J.header.data(), hdr);
            used = hdr;
            return (int)MCR_OK;
        };
        hipStream_t st = ctx->stream;
        for (i64 r0 = 0; r0 < count; r0 += per) {
            const i64 nr = std::min(per, count - r0);
            const i64 nt = csvw::tile_count(J.tiling, nr);
            CsvwBufs b;
            rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_csvw(cv, J, nr, b); });
            if (rc) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(b.cols, J.cols.data(), sizeof(pqw::ColDev) * J.cols.size(), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(b.err, 0xFF, 16, st));
            const csvw::FormatArgs fa{b.cols, J.tiling, r0, nr, (const i64*)index_dev, (i64)rows, ctx->pow10.as<const uint64_t>(), b.slots, b.sizes, b.err};
            LAUNCH(ctx, K_CSVW_FORMAT, csvw::k_csvw_format, dim3((unsigned)nt), dim3(csvw::kNT), 0, fa);
            LAUNCH(ctx, K_CSVW_SCAN, csvw::k_csvw_scan, dim3(1), dim3(256), 0, (const u32*)b.sizes, nt, b.offs);
            unsigned long long h_err[2]; u64 total = 0;
            HIP_TRY(ctx, hipMemcpyAsync(h_err, b.err, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(&total, b.offs + nt, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (h_err[0] != ~0ull || h_err[1] != ~0ull) { prof_resolve(ctx); return csvw_bad(ctx, who, J, h_err, (i64)rows); }
            if (total > (u64)nr * J.cols.size() * csvw::kFieldMax) { prof_resolve(ctx); return fail(ctx, MCR_EHIP, "%s: the text overran its bound", who); }
            // a later range of several: room for the rest at this range's bytes per row, and a twentieth more
            const size_t hint = r0 + nr < count ? hdr + (size_t)((double)(used + total) / (double)(r0 + nr) * 1.05 * (double)count) : 0;
            rc = with_header((size_t)total, hint);
            if (rc) { prof_resolve(ctx); return rc; }
            LAUNCH(ctx, K_CSVW_COMPACT, csvw::k_csvw_compact, dim3((unsigned)nt), dim3(256), 0, (const unsigned char*)b.slots, csvw::slot_bytes(J.tiling),
                   (const u32*)b.sizes, (const u64*)b.offs, b.image);
            HIP_TRY(ctx, hipMemcpyAsync(img->pin.as<unsigned char>() + used, b.image, (size_t)total, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            prof_resolve(ctx);
            used += (size_t)total;
        }
        if (!used) { rc = with_header(0, 0); if (rc) return rc; }
        img->size = used;
        *out = img.release();
    } catch (const std::exception& ex) {
        return fail(ctx, MCR_ENOMEM, "%s: host allocation failed: %s", who, ex.what());
    }
    return MCR_OK;
}

int mcr_csv_write_host(mcr_ctx* ctx, const mcr_pq_column* cols, int n_cols, int64_t rows, const int64_t* index, int64_t n_index, int header,
                       mcr_text_image** out)
{
    static const char* who = "mcr_csv_write_host";
    try {
        CsvwJob J;
        const int rc = csvw_args(ctx, who, cols, n_cols, rows, index, n_index, header, out, J);
        if (rc) return rc;
        *out = nullptr;
        std::unique_ptr<mcr_text_image> img(new mcr_text_image());
        img->host = std::move(J.header);
        unsigned long long err[2] = {~0ull, ~0ull};
        csvw::format_host(J.cols.data(), J.tiling, J.count, (const i64*)index, (i64)rows, img->host, err);
        if (err[0] != ~0ull || err[1] != ~0ull) return csvw_bad(ctx, who, J, err, (i64)rows);
        img->size = img->host.size();
        *out = img.release();
    } catch (const std::exception& ex) {
        return fail(ctx, MCR_ENOMEM, "%s: host allocation failed: %s", who, ex.what());
    }
    return MCR_OK;
}

const void* mcr_text_image_data(const mcr_text_image* im) { return !im ? nullptr : im->pinned ? im->pin.p : (const void*)im->host.data(); }
size_t mcr_text_image_size(const mcr_text_image* im) { return im ? im->size : 0; }
void mcr_text_image_free(mcr_text_image* im) { delete im; }

int mcr_format_double(double v, char* out26, int* len)
{
    if (!out26 || !len) return MCR_EINVAL;
    u64 bits;
    memcpy(&bits, &v, 8);
    const csvw::Dec d = csvw::dec_double(bits, csvw::kPow10);
    csvw::dec_put(d, (unsigned char*)out26);
    *len = (int)csvw::dec_len(d);
    return MCR_OK;
}

int mcr_select_rows_dev(mcr_ctx* ctx, const int64_t* chain_dev, int64_t M, const int64_t* chains, int n_chains, int64_t* rows_dev,
                        int64_t* n_selected)
{
    static const char* who = "mcr_select_rows_dev";
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!n_selected || n_chains < 0 || (n_chains > 0 && !chains)) return fail(ctx, MCR_EINVAL, "%s: NULL argument or a negative list length", who);
    if (M < 0 || M >= (int64_t)1 << 31) return fail(ctx, MCR_EINVAL, "%s: row count %lld out of range (0 .. 2^31 - 1)", who, (long long)M);
    *n_selected = 0;
    if (M == 0 || n_chains == 0) return MCR_OK;
    if (!chain_dev || !rows_dev) return fail(ctx, MCR_EINVAL, "%s: NULL argument", who);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "%s with summaries in flight", who);
    try {
        std::vector<i64> list(chains, chains + n_chains);
        std::sort(list.begin(), list.end());
        list.erase(std::unique(list.begin(), list.end()), list.end());
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const i64 nb = (M + csvw::kSelectNT - 1) / csvw::kSelectNT;
        i64* d_list; u32* d_counts; u64* d_offs;
        const int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) {
            d_list = cv.take<i64>(list.size()); d_counts = cv.take<u32>((size_t)nb); d_offs = cv.take<u64>((size_t)nb + 1);
        });
        if (rc) return rc;
        hipStream_t st = ctx->stream;
        HIP_TRY(ctx, hipMemcpyAsync(d_list, list.data(), 8 * list.size(), hipMemcpyHostToDevice, st));
        LAUNCH(ctx, K_SELECT_ROWS, csvw::k_select_rows<false>, dim3((unsigned)nb), dim3(csvw::kSelectNT), 0, (const i64*)chain_dev, (i64)M,
               (const i64*)d_list, (int)list.size(), d_counts, (const u64*)d_offs, (i64*)rows_dev);
        LAUNCH(ctx, K_CSVW_SCAN, csvw::k_csvw_scan, dim3(1), dim3(256), 0, (const u32*)d_counts, nb, d_offs);
        LAUNCH(ctx, K_SELECT_ROWS, csvw::k_select_rows<true>, dim3((unsigned)nb), dim3(csvw::kSelectNT), 0, (const i64*)chain_dev, (i64)M,
               (const i64*)d_list, (int)list.size(), d_counts, (const u64*)d_offs, (i64*)rows_dev);
        u64 total = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&total, d_offs + nb, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        prof_resolve(ctx);
        *n_selected = (int64_t)total;
    } catch (const std::exception& ex) {
        return fail(ctx, MCR_ENOMEM, "%s: host allocation failed: %s", who, ex.what());
    }
    return MCR_OK;
}

// ---- device row order (mcr_layout.hpp) -------------------------------------------------------------------------

namespace {
namespace lay = mcr::layout;
static_assert(lay::kLayoutSpan == MCR_LAYOUT_SPAN, "the header states the sort span");

// The one layout of the row-order workspace: per table the block the host reads (res, `stride` words each: the four
// extremes, the in-order word, then the distinct chains' count, ids and first rows), the table descriptors and the scan's
// partial records, then -- the sort of one table of M rows -- the ping-pong key / row-number buffers and the (digit,
// workgroup) histogram.
struct LayoutBufs {
    i64 *res, *part; lay::Table* tab;
    u64 *kA, *kB; u32 *iA, *iB, *hist;
};
constexpr int kLayoutRes = 8;         // words of a table's res in front of its bounds
inline size_t layout_stride(int cap) { return (size_t)kLayoutRes + 1 + 2 * (size_t)cap; }
void carve_layout(Carve& cv, LayoutBufs& b, int n, int cap, i64 sort_M)
{
    b.res = cv.take<i64>((size_t)n * layout_stride(cap));
    b.tab = cv.take<lay::Table>((size_t)n);
    b.part = cv.take<i64>((size_t)n * 5 * (size_t)lay::kScanGrid);
    if (sort_M <= 0) return;
    const size_t m = (size_t)sort_M, G = (size_t)((sort_M + lay::kLayoutSpan - 1) / lay::kLayoutSpan);
    b.kA = cv.take<u64>(m); b.kB = cv.take<u64>(m);
    b.iA = cv.take<u32>(m); b.iB = cv.take<u32>(m);
    b.hist = cv.take<u32>(256 * G);
}
inline int bit_length(u64 v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// Step 1 for n tables in one round trip: already in (chain, draw) order?  + the extremes of both columns, + the chains of
// every table as it stands (all an ordered table needs: most are).  h receives the n result blocks.
int layout_scan(mcr_ctx* ctx, const lay::Table* tables, int n, int cap, LayoutBufs& b, std::vector<i64>& h)
{
    int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_layout(cv, b, n, cap, 0); });
    if (rc) return rc;
    try { h.resize((size_t)n * layout_stride(cap)); } catch (const std::exception&) { return fail(ctx, MCR_ENOMEM, "host allocation failed"); }
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(b.tab, tables, sizeof(lay::Table) * (size_t)n, hipMemcpyHostToDevice, st));
    LAUNCH(ctx, K_LAYOUT_SCAN, lay::k_layout_scan, dim3((unsigned)lay::kScanGrid, (unsigned)n), dim3(lay::kLayoutNT), 0,
           (const lay::Table*)b.tab, b.part);
    LAUNCH(ctx, K_LAYOUT_SCAN, lay::k_layout_scan_final, dim3((unsigned)n), dim3(64), 0, (const i64*)b.part, lay::kScanGrid,
           b.res, (i64)layout_stride(cap));
    LAUNCH(ctx, K_LAYOUT_BOUNDS, lay::k_layout_bounds, dim3((unsigned)n), dim3(1024), 0, (const lay::Table*)b.tab,
           (const u32*)nullptr, cap, b.res + kLayoutRes, (i64)layout_stride(cap));
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), b.res, sizeof(i64) * h.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));      // (the pageable copies above are done with `tables` and `h` by now)
    return MCR_OK;
}

// ids / counts of one table from its result block; false when it has more than cap distinct chains.
bool layout_chains(const i64* blk, int cap, i64 M, int64_t* ids, int64_t* counts, int* n_chains)
{
    const i64* hb = blk + kLayoutRes;
    *n_chains = (int)(hb[0] < 0x7FFFFFFF ? hb[0] : 0x7FFFFFFF);
    if (hb[0] > cap) return false;
    const int n = (int)hb[0];
    for (int j = 0; j < n; ++j) {
        ids[j] = hb[1 + j];
        counts[j] = (j + 1 < n ? hb[1 + cap + j + 1] : M) - hb[1 + cap + j];
    }
    return true;
}

int layout_args(mcr_ctx* ctx, int cap, const int64_t* chain_ids, const int64_t* counts, const int* n_chains, const int* in_order)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!n_chains || !in_order || cap < 0 || (cap > 0 && (!chain_ids || !counts)))
        return fail(ctx, MCR_EINVAL, "chain layout: NULL argument");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "chain layout with summaries in flight");
    return MCR_OK;
}

}  // namespace

int mcr_chain_layout_dev(mcr_ctx* ctx, const int64_t* chain_dev, const int64_t* draw_dev, int64_t M, int64_t* order_dev,
                         int64_t* chain_ids, int64_t* counts, int cap, int* n_chains, int* in_order)
{
    int rc = layout_args(ctx, cap, chain_ids, counts, n_chains, in_order);
    if (rc) return rc;
    if (M < 0 || M >= (i64)0x7FFFFFFFll) return fail(ctx, MCR_EINVAL, "mcr_chain_layout_dev: row count out of range");
    *n_chains = 0; *in_order = 1;
    if (M == 0) return MCR_OK;
    if (!chain_dev || !draw_dev) return fail(ctx, MCR_EINVAL, "mcr_chain_layout_dev: NULL id column");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const lay::Table tab{reinterpret_cast<const i64*>(chain_dev), reinterpret_cast<const i64*>(draw_dev), (i64)M};
    LayoutBufs b{};
    std::vector<i64> h;
    rc = layout_scan(ctx, &tab, 1, cap, b, h);
    if (rc) return rc;
    const bool ordered = h[4] != 0;
    if (!ordered) {
        if (!order_dev) return fail(ctx, MCR_EINVAL, "mcr_chain_layout_dev: order_dev is NULL");
        hipStream_t st = ctx->stream;
        const i64 cmin = h[0], dmin = h[2];
        const int cbits = bit_length((u64)h[1] - (u64)cmin), dbits = bit_length((u64)h[3] - (u64)dmin);
        if (cbits + dbits > 64) {
            prof_resolve(ctx);
            return fail(ctx, MCR_EFALLBACK, "chain ids span %d bits and draw indices %d: no 64-bit row key", cbits, dbits);
        }
        // 2. keys + a stable 8-bit pass per significant key byte
        rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { carve_layout(cv, b, 1, cap, M); });
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(b.tab, &tab, sizeof tab, hipMemcpyHostToDevice, st));      // (the workspace may have moved)
        const unsigned nb = (unsigned)((M + lay::kLayoutNT - 1) / lay::kLayoutNT);
        const int G = (int)((M + lay::kLayoutSpan - 1) / lay::kLayoutSpan);
        LAUNCH(ctx, K_LAYOUT_KEYS, lay::k_layout_keys, dim3(nb), dim3(lay::kLayoutNT), 0, tab.chain, tab.draw, (i64)M, cmin, dmin,
               dbits, b.kA, b.iA);
        u64 *kin = b.kA, *kout = b.kB;
        u32 *iin = b.iA, *iout = b.iB;
        const int passes = (cbits + dbits + 7) / 8;
        for (int ps = 0; ps < passes; ++ps) {
            LAUNCH(ctx, K_LAYOUT_HIST, lay::k_layout_hist, dim3((unsigned)G), dim3(lay::kLayoutNT), 0, (const u64*)kin, (i64)M,
                   8 * ps, G, b.hist);
            LAUNCH(ctx, K_LAYOUT_OFFSETS, lay::k_layout_offsets, dim3(1), dim3(1024), 0, b.hist, (i64)256 * G);
            LAUNCH(ctx, K_LAYOUT_SCATTER, lay::k_layout_scatter, dim3((unsigned)G), dim3(lay::kLayoutNT), 0, (const u64*)kin,
                   (const u32*)iin, (i64)M, 8 * ps, G, (const u32*)b.hist, kout, iout);
            std::swap(kin, kout);
            std::swap(iin, iout);
        }
        LAUNCH(ctx, K_LAYOUT_KEYS, lay::k_layout_order, dim3(nb), dim3(lay::kLayoutNT), 0, (const u32*)iin, (i64)M,
               reinterpret_cast<i64*>(order_dev));
        // 3. the chains again, over the sorted rows
        LAUNCH(ctx, K_LAYOUT_BOUNDS, lay::k_layout_bounds, dim3(1), dim3(1024), 0, (const lay::Table*)b.tab, (const u32*)iin, cap,
               b.res + kLayoutRes, (i64)layout_stride(cap));
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), b.res, sizeof(i64) * h.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    prof_resolve(ctx);
    *in_order = ordered ? 1 : 0;
    if (!layout_chains(h.data(), cap, M, chain_ids, counts, n_chains))
        return fail(ctx, MCR_EINVAL, "%d distinct chain ids; the caller has room for %d", *n_chains, cap);
    return MCR_OK;
}

int mcr_chain_layout_many_dev(mcr_ctx* ctx, const mcr_id_columns* tables, int n_tables, int64_t* chain_ids, int64_t* counts,
                              int cap, int* n_chains, int* in_order)
{
    int rc = layout_args(ctx, cap, chain_ids, counts, n_chains, in_order);
    if (rc) return rc;
    if (n_tables < 0 || n_tables > kMaxGridY || (n_tables > 0 && !tables)) return fail(ctx, MCR_EINVAL, "mcr_chain_layout_many_dev: bad table list");
    if (n_tables == 0) return MCR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<lay::Table> tabs;
    std::vector<i64> h;
    try { tabs.resize((size_t)n_tables); } catch (const std::exception&) { return fail(ctx, MCR_ENOMEM, "host allocation failed"); }
    for (int t = 0; t < n_tables; ++t) {
        const mcr_id_columns& c = tables[t];
        if (c.rows < 0 || c.rows >= (i64)0x7FFFFFFFll) return fail(ctx, MCR_EINVAL, "mcr_chain_layout_many_dev: row count out of range");
        if (c.rows > 0 && (!c.chain_dev || !c.draw_dev)) return fail(ctx, MCR_EINVAL, "mcr_chain_layout_many_dev: NULL id column");
        tabs[(size_t)t] = lay::Table{reinterpret_cast<const i64*>(c.chain_dev), reinterpret_cast<const i64*>(c.draw_dev), (i64)c.rows};
    }
    LayoutBufs b{};
    rc = layout_scan(ctx, tabs.data(), n_tables, cap, b, h);
    if (rc) return rc;
    prof_resolve(ctx);
    for (int t = 0; t < n_tables; ++t) {
        const i64* blk = h.data() + (size_t)t * layout_stride(cap);
        in_order[t] = blk[4] != 0 ? 1 : 0;
        layout_chains(blk, cap, tabs[(size_t)t].M, chain_ids + (size_t)t * cap, counts + (size_t)t * cap, &n_chains[t]);
    }
    return MCR_OK;
}

int mcr_gather_rows_order_dev(mcr_ctx* ctx, const double* src_dev, int64_t P, int64_t M, const int64_t* order_dev,
                              double* dst_dev)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (P < 0 || M < 0 || P > kMaxGridY) return fail(ctx, MCR_EINVAL, "bad shape");
    if (P == 0 || M == 0) return MCR_OK;
    if (!src_dev || !dst_dev || !order_dev) return fail(ctx, MCR_EINVAL, "NULL argument");
    if (src_dev == dst_dev) return fail(ctx, MCR_EINVAL, "gather cannot run in place");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int* d_err = nullptr;
    const int rc = carve(ctx, lane_ws(ctx), [&](Carve& cv) { d_err = cv.take<int>(1); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
    LAUNCH(ctx, K_GATHER, lay::k_gather_rows_order, dim3((unsigned)((M + 255) / 256), (unsigned)P), dim3(256), 0, src_dev,
           (const i64*)order_dev, (i64)M, dst_dev, d_err);
    int h_err = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    if (h_err) return fail(ctx, MCR_EINVAL, "order has an entry outside [0, %lld)", (long long)M);
    return MCR_OK;
}


// ---- many files in one call -------------------------------------------------------------------------------

struct mcr_fileset {
    double phase_ms[MCR_FS_PHASES] = {0};
    int n_q = 0, n_jobs = 0;
    struct Entry {
        std::vector<std::string> names;
        i64 C = 0, N = 0;
        std::vector<double> f[MCR_FS_FIELDS];   // MCR_FS_* fields
    };
    std::vector<Entry> files;
};

namespace {
namespace pq = mcr::pq;

struct BatchFile {    // a file of mcr_summarize_files: descriptor, image, parsed metadata, column roles, place in the arena
    int fd = -1; size_t len = 0, img = 0; mcr_parquet* pq = nullptr;   // img: offset of the image in img.pin and img.dev
    mcr_csv* csv = nullptr;                                            // FileBatch::csv: the parsed header instead of pq
    int rc = MCR_OK; std::string err;                                  // set by its reader
    std::vector<int> cols; int chain = -1, draw = -1;
    i64 M = 0, C = 0, N = 0; size_t off = 0, ioff = 0;                 // draws at arena + off, ids at arena + ids_base + ioff
    BatchFile() = default; BatchFile(const BatchFile&) = delete;
    ~BatchFile() { if (pq) mcr_parquet_close(pq); if (csv) mcr_csv_close(csv); if (fd >= 0) close(fd); }
};

// What the stages of mcr_summarize_files hand on.  It holds the host ends of their copies, so that these outlive any copy
// still queued when a stage returns early.
struct FileBatch {
    const char* const* paths;
    bool csv = false;                                                // CmdStan chain CSVs (mcr_csv_open_paths), else draws files
    bool table = false;                                              // csv: table CSVs (mcr_csv_open_table_paths)
    std::vector<BatchFile> f;
    size_t img_total = 0, ids_base = 0, lay_base = 0, lay_out = 0;   // arena: draws, ids, FileIds, chain layouts
    char* arena = nullptr;
    std::vector<mcr_parquet_request> reqs; PqPlan pp;
    std::vector<pq::FileIds> fids; std::vector<i64> lay; int h_err[2] = {0, 0};   // lay: k_chain_layout, 4 per file
    FileBatch(const char* const* p, int n) : paths(p), f((size_t)n) {}
};

// 1. Opens and sizes the files, lays their images out back to back and makes the device and pinned staging that large.
int fs_open(mcr_ctx* ctx, FileBatch& B)
{
    for (size_t i = 0; i < B.f.size(); ++i) {
        BatchFile& m = B.f[i];
        m.fd = open(B.paths[i], O_RDONLY);
        struct stat st;
        if (m.fd < 0 || fstat(m.fd, &st) != 0) return fail(ctx, MCR_EINVAL, "cannot open %s", B.paths[i]);
        m.len = (size_t)st.st_size;
        if (m.len == 0 && !B.csv) return fail(ctx, MCR_EINVAL, "parquet: %s is empty", B.paths[i]);
        m.img = B.img_total;
        B.img_total = align_up(m.img + m.len, 256);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ctx->img.rewrite(ctx, pq_stage_bytes(B.img_total), B.img_total, 0);
}

// The readers of fs_read: however the stage ends, the pool stops handing out files and joins every thread it started.
struct ReaderPool {
    int n; std::atomic<int> next{0}; std::vector<std::thread> th;
    ~ReaderPool() { next.store(n); for (std::thread& t : th) t.join(); }
};

// 2. The images go WHOLE into one pinned host buffer (nearly every byte of a draws file is a column chunk this call decodes):
//    MCR_IO_THREADS host threads pread() them -- the page cache's copy lands in memory the DMA engine reads directly; no
//    mapping is set up or torn down (57 munmaps cost 2 ms of TLB shoot-downs in a process with this many threads), no page
//    faults, no pageable staging inside the runtime -- and parse each footer and its page headers from that image, while
//    THIS thread, the only one making HIP calls, uploads the finished prefix behind them in pieces of >= 2 MB.
int fs_read(mcr_ctx* ctx, FileBatch& B)
{
    const int n = (int)B.f.size();
    if (n == 0) return MCR_OK;
    char* pin = ctx->img.pin.as<char>();
    std::vector<std::atomic<int>> done((size_t)n);       // (value-initialised: 0)
    hipError_t he = hipSuccess;
    {
        ReaderPool pool{n};
        auto reader = [&]() {
            for (int i; (i = pool.next.fetch_add(1)) < n;) {
                BatchFile& m = B.f[(size_t)i];
                auto bad = [&](int code, const std::string& msg) { m.rc = code; m.err = msg; };
                try {
                    size_t got = 0;
                    for (ssize_t r; got < m.len && (r = pread(m.fd, pin + m.img + got, m.len - got, (off_t)got)) > 0;) got += (size_t)r;
                    if (got < m.len) bad(MCR_EINVAL, std::string("short read of ") + B.paths[i]);
                    else if (B.csv) {
                        m.csv = new mcr_csv();
                        if (B.table) { m.csv->table = true; m.csv->tflags = csv::open_table_image(m.csv->im, pin + m.img, m.len, &m.csv->twhere); }
                        else csv::open_image(m.csv->im, pin + m.img, m.len);
                        m.csv->im.path = B.paths[i];
                    } else {
                        m.pq = new mcr_parquet();
                        if (!pq::open(m.pq->f, pin + m.img, m.len)) bad(MCR_EINVAL, std::string(B.paths[i]) + ": parquet: " + m.pq->f.error);
                    }
                } catch (const std::exception& e) { bad(MCR_ENOMEM, std::string("host allocation failed: ") + e.what()); }
                done[(size_t)i].store(1, std::memory_order_release);
            }
        };
        try { while ((int)pool.th.size() < std::min(ctx->io_threads, n)) pool.th.emplace_back(reader); }
        catch (const std::exception&) {}    // std::system_error under a thread limit: the readers started share the files
        if (pool.th.empty()) reader();      // none: this thread reads them
        int sent = 0;                                        // files [0, sent) are uploaded
        for (int i = 0; i < n; ++i) {
            while (done[(size_t)i].load(std::memory_order_acquire) == 0) std::this_thread::yield();
            const size_t from = B.f[(size_t)sent].img, upto = align_up(B.f[(size_t)i].img + B.f[(size_t)i].len, 256);
            if (he == hipSuccess && (upto - from >= ctx->io_piece || i + 1 == n)) {
                if (upto > from) he = hipMemcpyAsync(ctx->img.dev.as<char>() + from, pin + from, upto - from, hipMemcpyHostToDevice, ctx->stream);
                sent = i + 1;
            }
        }
    }
    for (const BatchFile& m : B.f)
        if (m.rc) return fail(ctx, m.rc, "%s", m.err.c_str());
    if (he != hipSuccess) return fail(ctx, MCR_EHIP, "hipMemcpyAsync of the file images failed: %s", hipGetErrorString(he));
    return MCR_OK;
}

// 3. Column roles, the arena ([P][M] draws per file, packed, then the chain / draw ids), the decode requests and the page
//    table.  Arena order = path order: on the packaged corpus (statistics phase 1.18 - 1.20 ms, five tensors as the files
//    come, before k_tier3's short-chain slots) files of one shape side by side measured 1.42 - 1.48 ms, tensors capped at
//    160 / 100 / 60 / 30 parameters 1.29 / 1.33 / 1.40 / 1.90 ms, every tensor forked over two streams 1.31 - 1.34 ms.
int fs_layout(mcr_ctx* ctx, FileBatch& B)
{
    size_t arena = 0, ids = 0;
    for (size_t i = 0; i < B.f.size(); ++i) {
        BatchFile& m = B.f[i];
        const pq::File& f = m.pq->f;
        for (int c = 0; c < (int)f.cols.size(); ++c) {
            const int ty = f.cols[(size_t)c].type;
            const bool numeric = ty == pq::T_INT32 || ty == pq::T_INT64 || ty == pq::T_FLOAT || ty == pq::T_DOUBLE;
            if (f.cols[(size_t)c].name == "chain") m.chain = c;
            else if (f.cols[(size_t)c].name == "draw") m.draw = c;
            else if (numeric) m.cols.push_back(c);
        }
        if (m.chain < 0 || m.draw < 0) return fail(ctx, MCR_EINVAL, "%s: no chain / draw columns", B.paths[i]);
        m.M = f.num_rows;
        m.ioff = ids; ids += (size_t)2 * (size_t)m.M * 8;
        m.off = arena; arena += m.cols.size() * (size_t)m.M * 8;
    }
    const size_t n = B.f.size();
    B.ids_base = align_up(arena, 256);
    B.lay_base = align_up(B.ids_base + ids, 256), B.lay_out = align_up(B.lay_base + n * sizeof(pq::FileIds), 256);
    const int rc = ctx->fs_arena.reserve(ctx, B.lay_out + n * 32 + 256);
    if (rc) return rc;
    char* base = B.arena = ctx->fs_arena.as<char>();
    std::vector<FileBase> bases;
    for (const BatchFile& m : B.f) {
        for (size_t j = 0; j < m.cols.size(); ++j)
            B.reqs.push_back(mcr_parquet_request{m.pq, m.cols[j], MCR_PQ_F64, base + m.off + j * (size_t)m.M * 8});
        B.reqs.push_back(mcr_parquet_request{m.pq, m.chain, MCR_PQ_I64, base + B.ids_base + m.ioff});
        B.reqs.push_back(mcr_parquet_request{m.pq, m.draw, MCR_PQ_I64, base + B.ids_base + m.ioff + (size_t)m.M * 8});
        bases.emplace_back(&m.pq->f, m.img);
    }
    if (B.reqs.empty()) return MCR_OK;
    std::sort(bases.begin(), bases.end(), [](const FileBase& a, const FileBase& b) { return std::less<const pq::File*>()(a.first, b.first); });
    const int rp = pq_plan(ctx, B.reqs.data(), (int)B.reqs.size(), B.pp, &bases, B.img_total);
    return rp ? rp : pq_buffers(ctx, B.pp);   // (the images are uploading into img.dev, which fs_open sized for this plan)
}

// 4. Decode kernels + the chain / draw bookkeeping on the device (k_chain_layout: 32 bytes per file come back instead of the
//    id columns), then the layout checks (convert._chains_from_table): rows must already be in (chain, draw) order.
int fs_decode(mcr_ctx* ctx, FileBatch& B, int min_chains, int diagnostics)
{
    const size_t n = B.f.size();
    B.lay.assign(n * 4, 0);
    if (!B.reqs.empty()) {
        int rc = pq_launch(ctx, B.pp);
        if (rc) return rc;
        for (const BatchFile& m : B.f) {
            const i64* id = (const i64*)(B.arena + B.ids_base + m.ioff);
            B.fids.push_back(pq::FileIds{id, id + m.M, m.M});
        }
        char* fids = B.arena + B.lay_base;
        i64* lay = (i64*)(B.arena + B.lay_out);
        HIP_TRY(ctx, hipMemcpyAsync(fids, B.fids.data(), n * sizeof(pq::FileIds), hipMemcpyHostToDevice, ctx->stream));
        LAUNCH(ctx, K_GATHER, pq::k_chain_layout, dim3((unsigned)n), dim3(256), 0, (const pq::FileIds*)fids, lay);
        HIP_TRY(ctx, hipMemcpyAsync(B.lay.data(), lay, n * 32, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(B.h_err, B.pp.d_err, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        prof_resolve(ctx);
        rc = pq_error(ctx, B.h_err);
        if (rc) return rc;
    }
    for (size_t i = 0; i < n; ++i) {
        BatchFile& m = B.f[i];
        const i64* L = B.lay.data() + i * 4;
        if (m.M > 0 && !L[3]) return fail(ctx, MCR_ELAYOUT, "%s: rows are not in (chain, draw) order", B.paths[i]);
        const bool equal = m.M == 0 || L[2] != 0;
        m.C = m.M > 0 ? L[0] : 0;
        m.N = m.M > 0 ? L[1] : 0;
        if (diagnostics && !m.cols.empty()) {
            if (m.C < min_chains) return fail(ctx, MCR_EMINCHAINS, "%s: R-hat diagnostics require at least %d chains; got %lld chain(s)", B.paths[i], min_chains, (long long)m.C);
            if (!equal) return fail(ctx, MCR_ELAYOUT, "%s: chains of unequal length", B.paths[i]);
        }
        if (!diagnostics && !m.cols.empty() && m.M == 0) return fail(ctx, MCR_EINVAL, "%s: cannot compute stats of empty columns", B.paths[i]);
    }
    return MCR_OK;
}

// One statistics call: the files [first, first + count), parameters [p0, p0 + P) of the batch in path order.
struct Job { int first, count; i64 C, N, P, p0; };

// Every job's results, parameters in path order, until fs_scatter hands them to the files.
struct Staged { std::vector<double> f[MCR_FS_FIELDS]; std::vector<int64_t> lag[2], qlo; };

// 5. The result set (NaN until filled), the jobs (runs of neighbouring files of one shape are one tensor), enqueue, drain.
int fs_stats(mcr_ctx* ctx, const FileBatch& B, mcr_fileset& fs, Staged& S, int min_chains, const double* quantiles, int n_q,
             int diagnostics)
{
    std::vector<Job> jobs;
    fs.files.resize(B.f.size());
    i64 p0 = 0;
    for (int i = 0; i < (int)B.f.size(); ++i) {
        const BatchFile& m = B.f[(size_t)i];
        const i64 P = (i64)m.cols.size(), Cj = diagnostics ? m.C : 1, Nj = diagnostics ? m.N : m.M;
        mcr_fileset::Entry& e = fs.files[(size_t)i];
        for (int c : m.cols) e.names.push_back(m.pq->f.cols[(size_t)c].name);
        e.C = m.C; e.N = m.N;
        for (int k = 0; k < MCR_FS_FIELDS; ++k) e.f[k].assign((size_t)P * (k == MCR_FS_Q ? (size_t)fs.n_q : 1), NAN);
        if (P == 0) continue;
        Job* j = jobs.empty() ? nullptr : &jobs.back();      // (the arena holds the files' draws back to back in path order)
        if (j && j->first + j->count == i && j->C == Cj && j->N == Nj) { ++j->count; j->P += P; }
        else jobs.push_back(Job{i, 1, Cj, Nj, P, p0});
        p0 += P;
    }
    fs.n_jobs = (int)jobs.size();
    const size_t P = (size_t)p0;
    for (int k = 0; k < MCR_FS_FIELDS; ++k) S.f[k].assign(P * (k == MCR_FS_Q ? (size_t)n_q : 1), NAN);
    S.lag[0].assign(P, 0); S.lag[1].assign(P, 0); S.qlo.assign((size_t)(n_q > 0 ? n_q : 1), 0);
    mcr_summary all{};
    all.mean = S.f[MCR_FS_MEAN].data(); all.std = S.f[MCR_FS_STD].data();
    all.q = n_q > 0 ? S.f[MCR_FS_Q].data() : nullptr; all.median = S.f[MCR_FS_MEDIAN].data();
    all.q_lo = S.qlo.data();
    if (diagnostics) {
        all.rhat = S.f[MCR_FS_RHAT].data(); all.ess_bulk = S.f[MCR_FS_ESS_BULK].data(); all.ess_tail = S.f[MCR_FS_ESS_TAIL].data();
        all.rhat_bulk = S.f[MCR_FS_RHAT_BULK].data(); all.rhat_tail = S.f[MCR_FS_RHAT_TAIL].data();
        all.lag_bulk = S.lag[0].data(); all.lag_tail = S.lag[1].data();
    }
    int rc = MCR_OK;
    for (size_t k = 0; k < jobs.size() && !rc; ++k) {
        const Job& j = jobs[k];
        mcr_summary o = summary_at(all, j.p0, n_q);
        if (ctx->order.size() >= MCR_MAX_INFLIGHT) rc = wait_one_impl(ctx);
        if (!rc)
            rc = enqueue_impl(ctx, SummaryCall{B.arena + B.f[(size_t)j.first].off, MCR_F64, j.C, j.N, j.P, j.N, 1, j.C * j.N, nullptr, false,
                                               diagnostics ? min_chains : 1, quantiles, n_q, &o});
    }
    return drain(ctx, rc);
}

// 6. The staged results into the set, file by file.
void fs_scatter(Staged& S, int diagnostics, mcr_fileset& fs)
{
    for (size_t p = 0; diagnostics && p < S.lag[0].size(); ++p) {
        S.f[MCR_FS_LAG_BULK][p] = (double)S.lag[0][p];
        S.f[MCR_FS_LAG_TAIL][p] = (double)S.lag[1][p];
    }
    size_t p0 = 0;
    for (mcr_fileset::Entry& e : fs.files) {
        const size_t P = e.names.size();
        for (int k = 0; k < MCR_FS_FIELDS; ++k) {
            const size_t w = k == MCR_FS_Q ? (size_t)fs.n_q : 1;
            if (w) memcpy(e.f[k].data(), S.f[k].data() + p0 * w, P * w * sizeof(double));
        }
        p0 += P;
    }
}

struct StreamSync { hipStream_t st; ~StreamSync() { if (st) hipStreamSynchronize(st); } };   // unless released (st = nullptr)
}  // namespace

int mcr_summarize_files(mcr_ctx* ctx, const char* const* paths, int n_paths, int min_chains, const double* quantiles,
                        int n_q, int diagnostics, mcr_fileset** out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!out || n_paths < 0 || (n_paths > 0 && !paths)) return fail(ctx, MCR_EINVAL, "bad argument");
    if (min_chains < 1) return fail(ctx, MCR_EMINCHAINS_ARG, "min_chains must be >= 1; got %d", min_chains);
    if (n_q < 0 || n_q > MCR_MAX_QUANTILES || (n_q > 0 && !quantiles)) return fail(ctx, MCR_EINVAL, "bad quantile list");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_summarize_files with summaries in flight");
    try {
        std::unique_ptr<mcr_fileset> fs(new mcr_fileset());
        fs->n_q = n_q;
        using clk = std::chrono::steady_clock;
        const clk::time_point t_start = clk::now();
        clk::time_point t_prev = t_start;
        auto lap = [&](int k) { const clk::time_point now = clk::now(); fs->phase_ms[k] += std::chrono::duration<double, std::milli>(now - t_prev).count(); t_prev = now; };
        FileBatch B(paths, n_paths);
        int rc = fs_open(ctx, B);
        if (rc) return rc;
        lap(MCR_FS_PH_OPEN);
        StreamSync uploads{ctx->stream};   // they read img.pin, which the next call's readers write: a return waits for them
        rc = fs_read(ctx, B);
        if (!rc) { lap(MCR_FS_PH_READ); rc = fs_layout(ctx, B); }
        if (!rc) { lap(MCR_FS_PH_PLAN); rc = fs_decode(ctx, B, min_chains, diagnostics); }
        if (rc) return rc;
        uploads.st = nullptr;                                 // fs_decode waited for the stream
        lap(MCR_FS_PH_DECODE);
        Staged S;
        rc = fs_stats(ctx, B, *fs, S, min_chains, quantiles, n_q, diagnostics);
        if (rc) return rc;
        lap(MCR_FS_PH_STATS);
        fs_scatter(S, diagnostics, *fs);
        lap(MCR_FS_PH_COLLECT);
        B.f.clear();                                          // close, free the parsed metadata
        lap(MCR_FS_PH_CLOSE);
        fs->phase_ms[MCR_FS_PH_TOTAL] = std::chrono::duration<double, std::milli>(clk::now() - t_start).count();
        *out = fs.release();
        return MCR_OK;
    } catch (const std::exception& e) {
        return fail(ctx, MCR_ENOMEM, "mcr_summarize_files: host allocation failed: %s", e.what());
    }
}

int mcr_fileset_size(const mcr_fileset* fs) { return fs ? (int)fs->files.size() : -1; }
static const mcr_fileset::Entry* fs_entry(const mcr_fileset* fs, int file)
{
    return (fs && file >= 0 && file < (int)fs->files.size()) ? &fs->files[(size_t)file] : nullptr;
}
int64_t mcr_fileset_params(const mcr_fileset* fs, int file) { const auto* e = fs_entry(fs, file); return e ? (int64_t)e->names.size() : -1; }
int64_t mcr_fileset_chains(const mcr_fileset* fs, int file) { const auto* e = fs_entry(fs, file); return e ? e->C : -1; }
int64_t mcr_fileset_draws(const mcr_fileset* fs, int file) { const auto* e = fs_entry(fs, file); return e ? e->N : -1; }
const char* mcr_fileset_param_name(const mcr_fileset* fs, int file, int64_t param)
{
    const auto* e = fs_entry(fs, file);
    return (e && param >= 0 && param < (int64_t)e->names.size()) ? e->names[(size_t)param].c_str() : nullptr;
}
const double* mcr_fileset_field(const mcr_fileset* fs, int file, int field)
{
    const auto* e = fs_entry(fs, file);
    return (e && field >= 0 && field < MCR_FS_FIELDS) ? e->f[field].data() : nullptr;
}
int64_t mcr_fileset_export(const mcr_fileset* fs, double* rows, int64_t cap_rows)
{
    if (!fs) return -1;
    static const int order[10] = {MCR_FS_MEAN, MCR_FS_STD, MCR_FS_MEDIAN, MCR_FS_RHAT, MCR_FS_ESS_BULK, MCR_FS_ESS_TAIL,
                                  MCR_FS_RHAT_BULK, MCR_FS_RHAT_TAIL, MCR_FS_LAG_BULK, MCR_FS_LAG_TAIL};
    const size_t w = 10 + (size_t)fs->n_q;
    int64_t row = 0;
    for (const mcr_fileset::Entry& e : fs->files)
        for (size_t p = 0; p < e.names.size(); ++p, ++row) {
            if (!rows || row >= cap_rows) continue;
            double* r = rows + (size_t)row * w;
            for (int k = 0; k < 10; ++k) r[k] = e.f[order[k]][p];
            for (int q = 0; q < fs->n_q; ++q) r[10 + q] = e.f[MCR_FS_Q][p * (size_t)fs->n_q + (size_t)q];
        }
    return row;
}

int64_t mcr_fileset_names(const mcr_fileset* fs, char* buf, int64_t cap)
{
    if (!fs) return -1;
    int64_t need = 0;
    for (const mcr_fileset::Entry& e : fs->files)
        for (const std::string& n : e.names) {
            const int64_t len = (int64_t)n.size() + 1;
            if (buf && need + len <= cap) memcpy(buf + need, n.c_str(), (size_t)len);
            need += len;
        }
    return need;
}

int mcr_fileset_jobs(const mcr_fileset* fs) { return fs ? fs->n_jobs : -1; }
int mcr_fileset_phases(const mcr_fileset* fs, double* ms, int cap)
{
    if (!fs || !ms || cap < 0) return -1;
    const int n = cap < MCR_FS_PHASES ? cap : MCR_FS_PHASES;
    for (int k = 0; k < n; ++k) ms[k] = fs->phase_ms[k];
    return MCR_FS_PHASES;
}
void mcr_fileset_free(mcr_fileset* fs) { delete fs; }

// ---- CmdStan CSV ingest (replaces parse_cmdstan_csv, src/mcmc_ref/cmdstan_generate.py:13-29) --------

int mcr_csv_open(mcr_ctx* ctx, const void* bytes, size_t len, mcr_csv** out)
{
    if ((!bytes && len) || !out) return fail(ctx, MCR_EINVAL, "NULL argument");     // ctx may be NULL: host only
    try {
        std::unique_ptr<mcr_csv> f(new mcr_csv());
        csv::open_image(f->im, (const char*)bytes, len);
        *out = f.release();
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "csv: host allocation failed: %s", e.what()); }
    return MCR_OK;
}
void mcr_csv_close(mcr_csv* f) { delete f; }
int mcr_csv_num_columns(const mcr_csv* f) { return f ? (int)f->im.names.size() : -1; }
const char* mcr_csv_column_name(const mcr_csv* f, int col)
{
    return (f && col >= 0 && col < (int)f->im.names.size()) ? f->im.names[(size_t)col].c_str() : nullptr;
}
int64_t mcr_csv_body_offset(const mcr_csv* f) { return f ? (int64_t)f->im.body : -1; }

int mcr_parse_double(const char* text, size_t len, double* out)
{
    if ((!text && len) || !out) return MCR_EINVAL;
    uint64_t bits = 0;
    if (csv::parse_field(text, len, csv::kPow5, &bits) == 0) { memcpy(out, &bits, 8); return 0; }
    return csv::finish_field(text, len, out) ? 1 : MCR_EINVAL;
}

}  // extern "C"

namespace {
constexpr size_t kCsvTextMax = ((size_t)1 << 32) - ((size_t)1 << 20);   // offsets are 32-bit

std::string csv_file_name(const mcr_ctx* ctx, size_t f)
{
    const std::string& p = ctx->img.files[f].path;
    return p.empty() ? "file " + std::to_string(f) : p;
}

// ---- what the text decoders share (mcr_csv_decode, mcr_csv_decode_table, mcr_json_decode) ---------------------------

int ensure_pow5(mcr_ctx* ctx)
{
    if (ctx->pow5.p) return MCR_OK;
    const int rc = ctx->pow5.reserve(ctx, sizeof(csv::kPow5));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pow5.p, csv::kPow5, sizeof(csv::kPow5), hipMemcpyHostToDevice, ctx->stream));
    return MCR_OK;
}

// One parse with a hard list of Rec (csv::HardField, json::HardToken) in parse_scratch, and once more with a list that fits
// when the first overflows.  layout(cv) takes the decoder's own tables in front of the list (it runs twice per pass,
// measuring and carving, so it only takes); fill() enqueues their uploads and initial values; launch(hard, cap, count,
// err) enqueues the kernel and the read-back of the decoder's flags.  Hands back the list and the error key (~0: none).
template <class Rec, class Layout, class Fill, class Launch>
int hard_pass(mcr_ctx* ctx, std::vector<Rec>& list, unsigned long long* err, Layout&& layout, Fill&& fill, Launch&& launch)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ensure_pow5(ctx);
    for (int pass = 0; pass < 2 && !rc; ++pass) {
        const uint32_t cap = ctx->csv_hard_cap;
        Rec* d_hard = nullptr;
        unsigned long long* d_ctr = nullptr;                  // [0] the error key, smallest wins; [1] the hard count
        rc = carve(ctx, ctx->parse_scratch, [&](Carve& cv) {
            layout(cv);
            d_hard = cv.take<Rec>(cap);
            d_ctr = cv.take<unsigned long long>(2);
        });
        if (!rc) rc = fill();
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0xFF, 8, st));
        HIP_TRY(ctx, hipMemsetAsync(d_ctr + 1, 0, 8, st));
        rc = launch(d_hard, cap, (uint32_t*)(d_ctr + 1), d_ctr);
        if (rc) return rc;
        uint32_t count = 0;
        HIP_TRY(ctx, hipMemcpyAsync(err, d_ctr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&count, d_ctr + 1, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (count <= cap) {
            list.resize(count);
            if (count) HIP_TRY(ctx, hipMemcpy(list.data(), d_hard, (size_t)count * sizeof(Rec), hipMemcpyDeviceToHost));
            break;
        }
        ctx->csv_hard_cap = count + (count >> 3);
    }
    prof_resolve(ctx);
    return rc;
}

// out_dev[idx[i]] = val[i]: the values the host finished, in one upload and one scatter.
int patch_values(mcr_ctx* ctx, double* out_dev, const std::vector<long long>& idx, const std::vector<double>& val)
{
    const size_t n = idx.size();
    if (!n) return MCR_OK;
    long long* d_idx = nullptr;
    double* d_val = nullptr;
    const int rc = carve(ctx, ctx->parse_scratch, [&](Carve& cv) { d_idx = cv.take<long long>(n); d_val = cv.take<double>(n); });
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, idx.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_val, val.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, K_CSV_PATCH, csv::k_csv_patch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, out_dev, (const long long*)d_idx,
           (const double*)d_val, (uint32_t)n);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    prof_resolve(ctx);
    return MCR_OK;
}

// Column c of file f, whose nc slot table entries start at slots[s0], goes to `slot`.
int claim_slot(mcr_ctx* ctx, std::vector<int>& slots, size_t s0, int nc, size_t f, int c, int slot)
{
    if (c < 0 || c >= nc) return fail(ctx, MCR_EINVAL, "csv: %s has no column %d", csv_file_name(ctx, f).c_str(), c);
    if (slots[s0 + (size_t)c] != -1) return fail(ctx, MCR_EINVAL, "csv: column %d of %s is requested twice", c, csv_file_name(ctx, f).c_str());
    slots[s0 + (size_t)c] = slot;
    return MCR_OK;
}
}  // namespace

extern "C" {

namespace {
int csv_open_paths(mcr_ctx* ctx, const char* const* paths, int n_paths, mcr_csv** out, bool table)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!out || n_paths < 0 || (n_paths > 0 && !paths)) return fail(ctx, MCR_EINVAL, "bad argument");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_csv_open_paths with summaries in flight");
    try {
        FileBatch B(paths, n_paths);
        B.csv = true;
        B.table = table;
        ctx->img.staged = false;
        int rc = fs_open(ctx, B);
        if (rc) return rc;
        if (B.img_total > kCsvTextMax) return fail(ctx, MCR_EINVAL, "csv: the files of one call hold %zu bytes; the limit is 4 GiB", B.img_total);
        StreamSync uploads{ctx->stream};                      // the handles promise that the text is on the device
        rc = fs_read(ctx, B);
        if (rc) return rc;
        for (int i = 0; i < n_paths; ++i) {
            BatchFile& m = B.f[(size_t)i];
            m.csv->im.bytes = ctx->img.pin.as<const char>() + m.img;
            m.csv->owner = ctx; m.csv->gen = ctx->img.gen; m.csv->img = m.img;
            out[i] = m.csv;
            m.csv = nullptr;
        }
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "csv: host allocation failed: %s", e.what()); }
    return MCR_OK;
}

// "<file>: <what> (byte <offset within the file>)": the message of a table that goes back to the host reader.
int table_fallback(mcr_ctx* ctx, const std::string& file, const char* what, size_t byte)
{
    return fail(ctx, MCR_EFALLBACK, "csv table: %s: %s (byte %zu)", file.c_str(), what, byte);
}

const char* table_flag_text(int flags)
{
    if (flags & csv::kTabBom) return "a byte-order mark";
    if (flags & csv::kTabNoHeader) return "no header line";
    if (flags & csv::kTabHdrQuote) return "a '\"' in the header";
    if (flags & csv::kTabHdrCr) return "a carriage return without a line feed in the header";
    if (flags & csv::kTabEmptyName) return "an empty header name";
    return "a duplicated header name";
}
}  // namespace

int mcr_csv_open_paths(mcr_ctx* ctx, const char* const* paths, int n_paths, mcr_csv** out)
{
    return csv_open_paths(ctx, paths, n_paths, out, false);
}
int mcr_csv_open_table_paths(mcr_ctx* ctx, const char* const* paths, int n_paths, mcr_csv** out)
{
    return csv_open_paths(ctx, paths, n_paths, out, true);
}

int mcr_csv_open_table(mcr_ctx* ctx, const void* bytes, size_t len, mcr_csv** out)
{
    if ((!bytes && len) || !out) return fail(ctx, MCR_EINVAL, "NULL argument");     // ctx may be NULL: host only
    try {
        std::unique_ptr<mcr_csv> f(new mcr_csv());
        f->table = true;
        f->tflags = csv::open_table_image(f->im, (const char*)bytes, len, &f->twhere);
        *out = f.release();
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "csv: host allocation failed: %s", e.what()); }
    return MCR_OK;
}
int mcr_csv_table_flags(const mcr_csv* f) { return (f && f->table) ? f->tflags : -1; }

int mcr_parse_csv_number(const char* text, size_t len, double* value, int* is_int)
{
    if ((!text && len) || !value || !is_int) return MCR_EINVAL;
    uint64_t bits = 0;
    bool integer = false;
    const int rc = csv::strict_number(text, len, csv::kPow5, &bits, &integer);
    *is_int = integer;
    if (rc == csv::kNumDecided) { memcpy(value, &bits, 8); return 0; }
    if (rc != csv::kNumHard) return MCR_EFALLBACK;
    return csv::finish_field(text, len, value) ? 1 : MCR_EFALLBACK;
}

int mcr_csv_stage(mcr_ctx* ctx, const mcr_csv* const* files, int n_files, int64_t* rows)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (n_files < 0 || n_files > kMaxGridY || (n_files > 0 && (!files || !rows))) return fail(ctx, MCR_EINVAL, "bad file list");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_csv_stage with summaries in flight");
    ctx->img.staged = false;
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        int held = 0;
        for (int i = 0; i < n_files; ++i) {
            if (!files[i]) return fail(ctx, MCR_EINVAL, "file %d is NULL", i);
            if (files[i]->owner) {
                if (files[i]->owner != ctx || files[i]->gen != ctx->img.gen)
                    return fail(ctx, MCR_EINVAL, "csv: file %d was read by an earlier call whose images are gone; open it again", i);
                ++held;
            }
        }
        if (held && held != n_files) return fail(ctx, MCR_EINVAL, "csv: files read by the library and caller images cannot share a call");
        const bool table = n_files > 0 && files[0]->table;
        for (int i = 0; i < n_files; ++i) {
            if (files[i]->table != table) return fail(ctx, MCR_EINVAL, "csv: table files and chain files cannot share a call");
            if (table && files[i]->tflags)
                return table_fallback(ctx, files[i]->im.path.empty() ? "file " + std::to_string(i) : files[i]->im.path,
                                      table_flag_text(files[i]->tflags), files[i]->twhere);
        }
        ctx->img.table = table;
        ctx->img.files.assign((size_t)n_files, mcr_ctx::FileImage::File());
        if (!held) {                                           // caller images: into the pinned buffer, one upload
            size_t total = 0;
            for (int i = 0; i < n_files; ++i) { ctx->img.files[(size_t)i].img = total; total = align_up(total + files[i]->im.len, 256); }
            if (total > kCsvTextMax) return fail(ctx, MCR_EINVAL, "csv: the files of one call hold %zu bytes; the limit is 4 GiB", total);
            const int rc = ctx->img.rewrite(ctx, pq_stage_bytes(total), total, 0);
            if (rc) return rc;
            for (int i = 0; i < n_files; ++i)
                if (files[i]->im.len) memcpy(ctx->img.pin.as<char>() + ctx->img.files[(size_t)i].img, files[i]->im.bytes, files[i]->im.len);
            if (total) HIP_TRY(ctx, hipMemcpyAsync(ctx->img.dev.p, ctx->img.pin.p, total, hipMemcpyHostToDevice, st));
        }
        std::vector<csv::FileDesc> desc((size_t)n_files);
        std::vector<uint32_t> chunk_file;
        uint32_t slot0 = 0;
        for (int i = 0; i < n_files; ++i) {
            mcr_ctx::FileImage::File& c = ctx->img.files[(size_t)i];
            const csv::Image& im = files[i]->im;
            if (held) c.img = files[i]->img;
            c.len = im.len; c.body = im.body; c.ncols = (int)im.names.size(); c.path = im.path;
            desc[(size_t)i] = csv::FileDesc{(uint32_t)c.img, (uint32_t)(c.img + c.body), (uint32_t)(c.img + c.len), (uint32_t)c.ncols,
                                            (uint32_t)chunk_file.size(), slot0};
            slot0 += (uint32_t)c.ncols;
            chunk_file.insert(chunk_file.end(), (c.len + csv::kChunk - 1) / csv::kChunk, (uint32_t)i);
        }
        const uint32_t n_chunks = (uint32_t)chunk_file.size();
        ctx->img.row0.assign((size_t)n_files + 1, 0u);
        if (n_chunks) {
            // (the tables below are this call's own to fill: it stamps staged_gen when they are whole)
            csv::FileDesc* d_desc = nullptr;                  // first: the decoders find the descriptors at img.tab itself
            uint32_t *d_cfile = nullptr, *d_cnt = nullptr, *d_first = nullptr, *d_row0 = nullptr;
            int rc = carve(ctx, ctx->img.tab, [&](Carve& cv) {
                d_desc = cv.take<csv::FileDesc>(desc.size());
                d_cfile = cv.take<uint32_t>(n_chunks);
                d_cnt = cv.take<uint32_t>(n_chunks);
                d_first = cv.take<uint32_t>((size_t)n_chunks + 1);
                d_row0 = cv.take<uint32_t>((size_t)n_files + 1);
            });
            if (rc) return rc;
            ctx->img.row0_off = (size_t)((char*)d_row0 - ctx->img.tab.as<char>());
            HIP_TRY(ctx, hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(csv::FileDesc), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_cfile, chunk_file.data(), (size_t)n_chunks * 4, hipMemcpyHostToDevice, st));
            const char* text = ctx->img.dev.as<const char>();
            auto lines = [&](bool write) {                    // count pass, then the write pass into img.rows
                const auto kern = table ? (write ? csv::k_csv_lines<true, true> : csv::k_csv_lines<false, true>)
                                        : (write ? csv::k_csv_lines<true, false> : csv::k_csv_lines<false, false>);
                LAUNCH(ctx, K_CSV_LINES, kern, dim3(n_chunks), dim3(csv::kLinesNT), 0, text, (const csv::FileDesc*)d_desc,
                       (const uint32_t*)d_cfile, d_cnt, (const uint32_t*)d_first, write ? ctx->img.rows.as<uint32_t>() : nullptr);
                return (int)MCR_OK;
            };
            rc = lines(false);
            if (rc) return rc;
            LAUNCH(ctx, K_CSV_SCAN, csv::k_csv_scan, dim3(1), dim3(1024), 0, (const uint32_t*)d_cnt, n_chunks, d_first,
                   (const csv::FileDesc*)d_desc, (uint32_t)n_files, d_row0);
            HIP_TRY(ctx, hipMemcpyAsync(ctx->img.row0.data(), d_row0, ((size_t)n_files + 1) * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            const uint32_t total_rows = ctx->img.row0[(size_t)n_files];
            if (total_rows) {
                rc = ctx->img.rows.reserve(ctx, (size_t)total_rows * 4 + 256);
                if (rc) return rc;
                rc = lines(true);
                if (rc) return rc;
            }
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        prof_resolve(ctx);
        for (int i = 0; i < n_files; ++i) rows[i] = (int64_t)(ctx->img.row0[(size_t)i + 1] - ctx->img.row0[(size_t)i]);
        for (int i = 0; table && i < n_files; ++i)
            if (rows[i] == 0) return table_fallback(ctx, csv_file_name(ctx, (size_t)i), "no data rows", files[i]->im.body);
        ctx->img.staged = true;
        ctx->img.staged_gen = ctx->img.gen;
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "csv: host allocation failed: %s", e.what()); }
    return MCR_OK;
}

int mcr_csv_decode(mcr_ctx* ctx, const int* columns, int n_cols, int64_t max_rows, double* out_dev, int64_t stride_file,
                   int64_t stride_row, int64_t stride_col, int64_t* hard)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (hard) *hard = 0;
    if (n_cols < 0 || max_rows < 0 || (n_cols > 0 && !columns) || stride_file < 0 || stride_row < 0 || stride_col < 0)
        return fail(ctx, MCR_EINVAL, "bad argument");
    if (!ctx->img.is_staged()) return fail(ctx, MCR_EINVAL, "csv: no staged files (call mcr_csv_stage first)");
    if (ctx->img.table) return fail(ctx, MCR_EINVAL, "csv: the staged files are table CSVs (mcr_csv_decode_table reads them)");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_csv_decode with summaries in flight");
    try {
        const size_t nf = ctx->img.files.size();
        std::vector<int> slots;
        int64_t rows_eff = 0;
        for (size_t f = 0; f < nf; ++f) {
            const int nc = ctx->img.files[f].ncols;
            const size_t s0 = slots.size();
            slots.insert(slots.end(), (size_t)nc, -1);
            for (int k = 0; k < n_cols; ++k) {
                const int rc = claim_slot(ctx, slots, s0, nc, f, columns[f * (size_t)n_cols + (size_t)k], k);
                if (rc) return rc;
            }
            rows_eff = std::max(rows_eff, std::min<int64_t>(max_rows, (int64_t)(ctx->img.row0[f + 1] - ctx->img.row0[f])));
        }
        if (rows_eff == 0 || n_cols == 0) return MCR_OK;
        if (!out_dev) return fail(ctx, MCR_EINVAL, "out_dev is NULL");
        hipStream_t st = ctx->stream;
        const char* tb = ctx->img.tab.as<const char>();          // as mcr_csv_stage carved it: descriptors first
        unsigned long long h_err = ~0ull;
        std::vector<csv::HardField> list;
        int* d_slots = nullptr;
        int rc = hard_pass(ctx, list, &h_err, [&](Carve& cv) { d_slots = cv.take<int>(slots.size()); },
                           [&] { HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, st)); return (int)MCR_OK; },
                           [&](csv::HardField* d_hard, uint32_t cap, uint32_t* d_count, unsigned long long* d_err) {
            csv::ParseArgs a{ctx->img.dev.as<const char>(), (const csv::FileDesc*)tb, ctx->img.rows.as<const uint32_t>(),
                             (const uint32_t*)(tb + ctx->img.row0_off), d_slots, ctx->pow5.as<const uint64_t>(), (long long)max_rows, out_dev,
                             (long long)stride_file, (long long)stride_row, (long long)stride_col, d_hard, cap, d_count, d_err};
            LAUNCH(ctx, K_CSV_PARSE, csv::k_csv_parse, dim3((unsigned)((rows_eff + csv::kParseWaves - 1) / csv::kParseWaves), (unsigned)nf),
                   dim3(csv::kParseWaves * 64), 0, a);
            return (int)MCR_OK;
        });
        if (rc) return rc;
        const char* pin = ctx->img.pin.as<const char>();
        if (h_err != ~0ull) {
            const size_t f = (size_t)(h_err >> 44);
            const unsigned long long row = (h_err >> 4) & ((1ull << 40) - 1);
            const mcr_ctx::FileImage::File& c = ctx->img.files[f];
            if ((h_err & 15) == csv::kErrQuote)
                return fail(ctx, MCR_EINVAL, "%s: data row %llu: quoted fields are not supported", csv_file_name(ctx, f).c_str(), row);
            uint32_t start = 0;
            HIP_TRY(ctx, hipMemcpy(&start, ctx->img.rows.as<const uint32_t>() + ctx->img.row0[f] + row, 4, hipMemcpyDeviceToHost));
            size_t fields = 1;
            for (size_t i = start; i < c.img + c.len && pin[i] != '\n'; ++i) fields += pin[i] == ',';
            return fail(ctx, MCR_EINVAL, "%s: data row %llu has %zu fields, header has %d", csv_file_name(ctx, f).c_str(), row, fields, c.ncols);
        }
        std::vector<long long> idx(list.size());              // the host finishes them: strtod on the pinned image
        std::vector<double> val(list.size());
        for (size_t i = 0; i < list.size(); ++i) {
            const csv::HardField& h = list[i];
            if (!csv::finish_field(pin + h.off, h.len, &val[i])) {
                int col = 0;
                size_t base = 0;
                for (size_t s = 0; s < h.file; ++s) base += (size_t)ctx->img.files[s].ncols;
                while (col < ctx->img.files[h.file].ncols && slots[base + (size_t)col] != (int)h.slot) ++col;
                return fail(ctx, MCR_EINVAL, "%s: data row %u, column %d: could not convert string to float: '%.*s'",
                            csv_file_name(ctx, h.file).c_str(), h.row, col, (int)std::min<uint32_t>(h.len, 200u), pin + h.off);
            }
            idx[i] = (long long)h.file * stride_file + (long long)h.row * stride_row + (long long)h.slot * stride_col;
        }
        rc = patch_values(ctx, out_dev, idx, val);
        if (rc) return rc;
        if (hard) *hard = (int64_t)list.size();
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "csv: host allocation failed: %s", e.what()); }
    return MCR_OK;
}

int mcr_csv_decode_table(mcr_ctx* ctx, const int* columns, int n_cols, const int* id_columns, int64_t max_rows, double* out_dev,
                         int64_t stride_file, int64_t stride_row, int64_t stride_col, int64_t* ids_dev, uint8_t* all_int, int64_t* hard)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (hard) *hard = 0;
    if (n_cols < 0 || max_rows < 0 || (n_cols > 0 && !columns) || !id_columns || stride_file < 0 || stride_row < 0 || stride_col < 0)
        return fail(ctx, MCR_EINVAL, "bad argument");
    if (!ctx->img.is_staged() || !ctx->img.table)
        return fail(ctx, MCR_EINVAL, "csv: no staged table files (call mcr_csv_open_table_paths and mcr_csv_stage first)");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_csv_decode_table with summaries in flight");
    try {
        const size_t nf = ctx->img.files.size();
        const bool packed = stride_file == 0 && stride_col == 0;
        std::vector<int> slots;
        std::vector<csv::TableOut> outs(nf);
        int64_t rows_eff = 0, at = 0, id_at = 0;
        bool any_col = false, any_id = false;
        for (size_t f = 0; f < nf; ++f) {
            const int nc = ctx->img.files[f].ncols;
            const size_t s0 = slots.size();
            slots.insert(slots.end(), (size_t)nc, -1);
            int used = 0;
            for (int k = 0; k < n_cols; ++k) {
                const int c = columns[f * (size_t)n_cols + (size_t)k];
                if (c == -1) continue;
                const int rc = claim_slot(ctx, slots, s0, nc, f, c, k);
                if (rc) return rc;
                used = k + 1;
            }
            for (int w = 0; w < 2; ++w) {
                const int c = id_columns[2 * f + (size_t)w];
                if (c == -1) continue;
                const int rc = claim_slot(ctx, slots, s0, nc, f, c, w ? csv::kSlotDraw : csv::kSlotChain);
                if (rc) return rc;
                any_id = true;
            }
            for (int c = 0; c < nc; ++c)
                if (slots[s0 + (size_t)c] == -1)
                    return fail(ctx, MCR_EINVAL, "csv: column %d of %s is neither requested nor an id column (a table is read whole)", c, csv_file_name(ctx, f).c_str());
            const int64_t rows = std::min<int64_t>(max_rows, (int64_t)(ctx->img.row0[f + 1] - ctx->img.row0[f]));
            csv::TableOut& o = outs[f];
            o.rows = rows; o.sr = packed ? 1 : stride_row; o.sc = packed ? rows : stride_col;
            o.base = packed ? at : (int64_t)f * stride_file;
            o.ids = id_at;
            at += (int64_t)used * rows; id_at += 2 * rows;
            any_col |= used > 0;
            rows_eff = std::max(rows_eff, rows);
        }
        if (rows_eff == 0 || nf == 0) return MCR_OK;
        if (any_col && !out_dev) return fail(ctx, MCR_EINVAL, "out_dev is NULL");
        if (any_id && !ids_dev) return fail(ctx, MCR_EINVAL, "ids_dev is NULL");
        if (n_cols > 0 && !all_int) return fail(ctx, MCR_EINVAL, "all_int is NULL");
        hipStream_t st = ctx->stream;
        const char* tb = ctx->img.tab.as<const char>();          // as mcr_csv_stage carved it: descriptors first
        unsigned long long h_err = ~0ull;
        std::vector<csv::HardField> list;
        std::vector<uint8_t> flags(2 * slots.size());       // all_int, then neg_zero
        int* d_slots = nullptr;
        csv::TableOut* d_outs = nullptr;
        unsigned char* d_flags = nullptr;
        int rc = hard_pass(ctx, list, &h_err,
                           [&](Carve& cv) { d_slots = cv.take<int>(slots.size()); d_outs = cv.take<csv::TableOut>(nf); d_flags = cv.take<unsigned char>(flags.size()); },
                           [&] {
            HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_outs, outs.data(), nf * sizeof(csv::TableOut), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(d_flags, 1, slots.size(), st));
            HIP_TRY(ctx, hipMemsetAsync(d_flags + slots.size(), 0, slots.size(), st));
            return (int)MCR_OK;
        },
                           [&](csv::HardField* d_hard, uint32_t cap, uint32_t* d_count, unsigned long long* d_err) {
            csv::TableArgs a{ctx->img.dev.as<const char>(), (const csv::FileDesc*)tb, ctx->img.rows.as<const uint32_t>(),
                             (const uint32_t*)(tb + ctx->img.row0_off), d_slots, ctx->pow5.as<const uint64_t>(), d_outs, out_dev, (long long*)ids_dev,
                             d_flags, d_flags + slots.size(), d_hard, cap, d_count, d_err};
            LAUNCH(ctx, K_CSV_TABLE_PARSE, csv::k_csv_table_parse, dim3((unsigned)((rows_eff + csv::kParseWaves - 1) / csv::kParseWaves), (unsigned)nf),
                   dim3(csv::kParseWaves * 64), 0, a);
            HIP_TRY(ctx, hipMemcpyAsync(flags.data(), d_flags, flags.size(), hipMemcpyDeviceToHost, st));
            return (int)MCR_OK;
        });
        if (rc) return rc;
        const char* pin = ctx->img.pin.as<const char>();
        if (h_err != ~0ull) {                                  // the first byte that leaves the subset: the host reader's file
            const size_t off = (size_t)(h_err >> 4);
            size_t f = 0;
            while (f + 1 < nf && ctx->img.files[f + 1].img <= off) ++f;
            const mcr_ctx::FileImage::File& c = ctx->img.files[f];
            const int kind = (int)(h_err & 15);
            size_t ls = off, le = off;                         // the line around it
            while (ls > c.img && pin[ls - 1] != '\n') --ls;
            while (le < c.img + c.len && pin[le] != '\n') ++le;
            bool blank = true, cr = false;
            for (size_t i = ls; i < le; ++i) {
                blank = blank && (pin[i] == ' ' || (pin[i] >= '\t' && pin[i] <= '\r'));
                cr = cr || (pin[i] == '\r' && i + 1 < le);
            }
            if (le == c.img + c.len && le > ls && pin[le - 1] == '\r') cr = true;     // a "\r" that ends the file
            size_t fe = off;                                   // the field that starts at `off` (a quoted one fails the grammar first)
            while (fe < le && pin[fe] != ',') ++fe;
            const void* q = kind == csv::kTabErrQuote ? nullptr : memchr(pin + off, '"', fe - off);
            if (q) return table_fallback(ctx, csv_file_name(ctx, f), "a '\"'", (size_t)((const char*)q - pin) - c.img);
            const char* what = kind == csv::kTabErrQuote ? "a '\"'"
                : cr ? "a carriage return without a line feed"
                : blank ? "a whitespace-only line"
                : kind == csv::kTabErrFields ? "a row whose field count differs from the header's"
                : kind == csv::kTabErrBigInt ? "an integer literal above 2^53"
                : kind == csv::kTabErrIdField ? "a non-integer literal in an id column"
                : "a field outside the number grammar";
            return table_fallback(ctx, csv_file_name(ctx, f), what, off - c.img);
        }
        std::vector<size_t> slot_base(nf, 0);
        bool unsign = false;
        for (size_t f = 1; f < nf; ++f) slot_base[f] = slot_base[f - 1] + (size_t)ctx->img.files[f - 1].ncols;
        std::vector<long long> idx(list.size());              // the host finishes them: strtod on the pinned image
        std::vector<double> val(list.size());
        for (size_t i = 0; i < list.size(); ++i) {
            const csv::HardField& h = list[i];
            if (!csv::finish_field(pin + h.off, h.len, &val[i]))      // (cannot happen: the device checked the grammar)
                return table_fallback(ctx, csv_file_name(ctx, h.file), "a field outside the number grammar", h.off - ctx->img.files[h.file].img);
            const csv::TableOut& o = outs[h.file];
            idx[i] = o.base + (long long)h.row * o.sr + (long long)h.slot * o.sc;
        }
        rc = patch_values(ctx, out_dev, idx, val);
        if (rc) return rc;
        for (size_t f = 0; f < nf && n_cols > 0; ++f) {
            for (int k = 0; k < n_cols; ++k) all_int[f * (size_t)n_cols + (size_t)k] = 0;
            for (int c = 0; c < ctx->img.files[f].ncols; ++c) {
                const int k = slots[slot_base[f] + (size_t)c];
                if (k < 0) continue;
                all_int[f * (size_t)n_cols + (size_t)k] = flags[slot_base[f] + (size_t)c];
                if (flags[slot_base[f] + (size_t)c] && flags[slots.size() + slot_base[f] + (size_t)c] && outs[f].rows > 0) {   // an int64 column: no -0
                    const csv::TableOut& o = outs[f];
                    LAUNCH(ctx, K_CSV_UNSIGN_ZERO, csv::k_csv_unsign_zero, dim3((unsigned)((o.rows + 255) / 256)), dim3(256), 0,
                           out_dev + o.base + (long long)k * o.sc, o.sr, o.rows);
                    unsign = true;
                }
            }
        }
        if (unsign) {
            HIP_TRY(ctx, hipStreamSynchronize(st));
            prof_resolve(ctx);
        }
        if (hard) *hard = (int64_t)list.size();
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "csv: host allocation failed: %s", e.what()); }
    return MCR_OK;
}

}  // extern "C"

// ---- chain-list JSON ingest (replaces json.loads + np.asarray of the JSON-zip reader, src/mcmc_ref/convert.py:78-102)

// An indexed document.  The caller keeps `bytes` alive and unchanged; the device holds a copy and every token's offset.
struct mcr_json {
    mcr_ctx* ctx = nullptr; const char* bytes = nullptr; size_t len = 0;
    DevBuf d_text;                           // the text, padded to whole chunks
    DevBuf d_tok; uint32_t n_tok = 0;
    std::vector<json::Chain> chains;
    ~mcr_json() { if (ctx) hipSetDevice(ctx->device); }      // (the members free themselves behind this)
};

namespace {
// The text of the element that starts at `off`, for a message: up to the next ',' or ']', at most 48 bytes.
std::string json_excerpt(const mcr_json* f, size_t off)
{
    size_t e = off;
    while (e < f->len && e - off < 48 && f->bytes[e] != ',' && f->bytes[e] != ']') ++e;
    std::string s(f->bytes + off, e - off);
    for (char& c : s) if ((unsigned char)c < 0x20) c = ' ';
    return s;
}
}  // namespace

extern "C" {

int mcr_json_open(mcr_ctx* ctx, const void* bytes, size_t len, mcr_json** out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if ((!bytes && len) || !out) return fail(ctx, MCR_EINVAL, "NULL argument");
    if (len >= ((size_t)1 << 32)) return fail(ctx, MCR_EINVAL, "json: the document holds %zu bytes; the limit is 4 GiB", len);
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_json_open with summaries in flight");
    if (len == 0) return fail(ctx, MCR_EFALLBACK, "json: the document is empty (byte 0)");
    try {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        std::unique_ptr<mcr_json> f(new mcr_json());
        f->ctx = ctx; f->bytes = (const char*)bytes; f->len = len;
        const uint32_t n_chunks = (uint32_t)((len + json::kChunk - 1) / json::kChunk);
        int rc = f->d_text.reserve(ctx, (size_t)n_chunks * json::kChunk);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(f->d_text.p, bytes, len, hipMemcpyHostToDevice, st));
        // scratch: chunk counts | in_string | first | sfirst (n_chunks + 1 each) | first backslash
        const size_t o_in = align_up((size_t)n_chunks * sizeof(json::ChunkCount), 256), w = align_up(((size_t)n_chunks + 1) * 4, 256),
                     o_first = o_in + w, o_sfirst = o_first + w, o_bsl = o_sfirst + w;
        rc = ctx->parse_scratch.reserve(ctx, o_bsl + 256);
        if (rc) return rc;
        char* ax = ctx->parse_scratch.as<char>();
        json::ChunkCount* d_cnt = (json::ChunkCount*)ax;
        uint32_t *d_in = (uint32_t*)(ax + o_in), *d_first = (uint32_t*)(ax + o_first), *d_sfirst = (uint32_t*)(ax + o_sfirst),
                 *d_bsl = (uint32_t*)(ax + o_bsl);
        const char* text = f->d_text.as<const char>();
        HIP_TRY(ctx, hipMemsetAsync(d_bsl, 0xFF, 4, st));
        LAUNCH(ctx, K_JSON_INDEX, json::k_json_index<false>, dim3(n_chunks), dim3(json::kIndexNT), 0, text, (uint32_t)len, d_cnt, d_bsl,
               (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
               (uint32_t*)nullptr);
        LAUNCH(ctx, K_JSON_SCAN, json::k_json_scan, dim3(1), dim3(1024), 0, (const json::ChunkCount*)d_cnt, n_chunks, d_in, d_first, d_sfirst);
        uint32_t bsl = 0, n_tok = 0, n_skel = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&bsl, d_bsl, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&n_tok, d_first + n_chunks, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&n_skel, d_sfirst + n_chunks, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (bsl != json::kNoOffset) { prof_resolve(ctx); return fail(ctx, MCR_EFALLBACK, "json: a backslash (byte %u): escapes take the host reader", bsl); }
        std::vector<uint32_t> skel((size_t)n_skel * 2);
        if (n_tok) {
            rc = f->d_tok.reserve(ctx, (size_t)n_tok * 4);
            // the skeleton borrows the row starts' buffer: whatever mcr_csv_stage left there is gone, and a decode says so
            if (!rc) rc = ctx->img.rewrite(ctx, 0, 0, (size_t)n_skel * 8 + 256);
            if (rc) return rc;
            uint32_t* d_skel = ctx->img.rows.as<uint32_t>();
            LAUNCH(ctx, K_JSON_INDEX, json::k_json_index<true>, dim3(n_chunks), dim3(json::kIndexNT), 0, text, (uint32_t)len, d_cnt, d_bsl,
                   (const uint32_t*)d_in, (const uint32_t*)d_first, (const uint32_t*)d_sfirst, f->d_tok.as<uint32_t>(), d_skel, d_skel + n_skel);
            if (n_skel) HIP_TRY(ctx, hipMemcpyAsync(skel.data(), d_skel, (size_t)n_skel * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        prof_resolve(ctx);
        f->n_tok = n_tok;
        size_t where = 0;
        const char* why = json::walk(f->bytes, len, skel.data(), skel.data() + n_skel, n_skel, f->chains, &where);
        if (*why) return fail(ctx, MCR_EFALLBACK, "json: %s (byte %zu)", why, where);
        *out = f.release();
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "json: host allocation failed: %s", e.what()); }
    return MCR_OK;
}

void mcr_json_close(mcr_json* f) { delete f; }
int mcr_json_num_chains(const mcr_json* f) { return f ? (int)f->chains.size() : -1; }
int mcr_json_num_keys(const mcr_json* f, int chain)
{
    return (f && chain >= 0 && chain < (int)f->chains.size()) ? (int)f->chains[(size_t)chain].keys.size() : -1;
}
const char* mcr_json_key(const mcr_json* f, int chain, int k)
{
    return mcr_json_num_keys(f, chain) > k && k >= 0 ? f->chains[(size_t)chain].keys[(size_t)k].c_str() : nullptr;
}
int64_t mcr_json_length(const mcr_json* f, int chain, int k)
{
    return mcr_json_num_keys(f, chain) > k && k >= 0 ? (int64_t)f->chains[(size_t)chain].arrays[(size_t)k].count : -1;
}

int mcr_parse_json_number(const char* text, size_t len, double* value, int* is_int)
{
    if ((!text && len) || !value || !is_int) return MCR_EINVAL;
    uint64_t bits = 0;
    bool integer = false;
    const int rc = json::json_token(text, len, csv::kPow5, &bits, &integer);
    *is_int = integer;
    if (rc == csv::kNumDecided) { memcpy(value, &bits, 8); return 0; }
    if (rc == csv::kNumHard) return json::finish_token(text, len, value) ? 1 : MCR_EINVAL;
    return rc == csv::kNumBigInt ? MCR_EFALLBACK : MCR_EINVAL;
}

int mcr_json_decode(mcr_ctx* ctx, const mcr_json* f, const int* arrays, int n_params, int64_t n_draws, double* out_dev,
                    int64_t stride_c, int64_t stride_n, int64_t stride_p, uint8_t* all_int, int64_t* hard)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (hard) *hard = 0;
    if (!f || f->ctx != ctx || n_params < 0 || n_draws < 0 || (n_params > 0 && (!arrays || !all_int)) || stride_c < 0 || stride_n < 0 ||
        stride_p < 0)
        return fail(ctx, MCR_EINVAL, "bad argument");
    if (!ctx->order.empty()) return fail(ctx, MCR_EINVAL, "mcr_json_decode with summaries in flight");
    try {
        const size_t n_chains = f->chains.size();
        std::vector<json::ArrayDesc> descs;
        std::vector<size_t> desc_of((size_t)n_params * n_chains, SIZE_MAX);      // [c * n_params + p] -> descs index
        uint64_t n_values = 0;
        for (size_t c = 0; c < n_chains; ++c) {
            const json::Chain& ch = f->chains[c];
            std::vector<int> slot(ch.keys.size(), -1);
            for (int p = 0; p < n_params; ++p) {
                const int k = arrays[c * (size_t)n_params + (size_t)p];
                if (k < 0 || k >= (int)ch.keys.size()) return fail(ctx, MCR_EINVAL, "json: chain %zu has no key %d", c, k);
                if (slot[(size_t)k] >= 0) return fail(ctx, MCR_EINVAL, "json: key %d of chain %zu is requested twice", k, c);
                if ((int64_t)ch.arrays[(size_t)k].count < n_draws)
                    return fail(ctx, MCR_EINVAL, "json: chain %zu, key %d holds %u values, %lld are requested", c, k, ch.arrays[(size_t)k].count,
                                (long long)n_draws);
                slot[(size_t)k] = p;
            }
            for (size_t k = 0; k < ch.keys.size(); ++k) {       // every element of the document is checked, the selected ones stored
                const json::Array& a = ch.arrays[k];
                if (!a.count) continue;
                const int p = slot[k];
                if (p >= 0) desc_of[c * (size_t)n_params + (size_t)p] = descs.size();
                descs.push_back(json::ArrayDesc{a.tok0, a.count, p >= 0 ? (uint32_t)n_draws : 0u, (uint32_t)n_values,
                                                p >= 0 ? (long long)c * stride_c + (long long)p * stride_p : -1ll});
                n_values += a.count;
            }
        }
        for (size_t i = 0; i < (size_t)n_params * n_chains; ++i) all_int[i] = 1;
        if (n_values == 0) return MCR_OK;
        if (n_params > 0 && n_draws > 0 && !out_dev) return fail(ctx, MCR_EINVAL, "out_dev is NULL");
        hipStream_t st = ctx->stream;
        const size_t n_arrays = descs.size();
        unsigned long long h_err = ~0ull;
        std::vector<json::HardToken> list;
        std::vector<uint32_t> not_int(n_arrays);
        json::ArrayDesc* d_descs = nullptr;
        uint32_t* d_ni = nullptr;
        int rc = hard_pass(ctx, list, &h_err, [&](Carve& cv) { d_descs = cv.take<json::ArrayDesc>(n_arrays); d_ni = cv.take<uint32_t>(n_arrays); },
                           [&] {
            HIP_TRY(ctx, hipMemcpyAsync(d_descs, descs.data(), n_arrays * sizeof(json::ArrayDesc), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemsetAsync(d_ni, 0, n_arrays * 4, st));
            return (int)MCR_OK;
        },
                           [&](json::HardToken* d_hard, uint32_t cap, uint32_t* d_count, unsigned long long* d_err) {
            json::ParseArgs a{f->d_text.as<const char>(), f->d_tok.as<const uint32_t>(), d_descs, (uint32_t)n_arrays, (uint32_t)n_values,
                              ctx->pow5.as<const uint64_t>(), out_dev, (long long)stride_n, d_ni, d_hard, cap, d_count, d_err};
            LAUNCH(ctx, K_JSON_PARSE, json::k_json_parse, dim3((unsigned)((n_values + json::kParseNT - 1) / json::kParseNT)), dim3(json::kParseNT),
                   0, a);
            HIP_TRY(ctx, hipMemcpyAsync(not_int.data(), d_ni, n_arrays * 4, hipMemcpyDeviceToHost, st));
            return (int)MCR_OK;
        });
        if (rc) return rc;
        if (h_err != ~0ull) {
            const size_t off = (size_t)(h_err >> 4);
            if ((h_err & 15) == json::kErrBigInt)
                return fail(ctx, MCR_EFALLBACK, "json: the integer literal '%s' (byte %zu) is beyond 2^53", json_excerpt(f, off).c_str(), off);
            return fail(ctx, MCR_EFALLBACK, "json: the array element '%s' (byte %zu) is not a number", json_excerpt(f, off).c_str(), off);
        }
        std::vector<long long> idx(list.size());              // the host finishes them: strtod on the caller's image
        std::vector<double> val(list.size());
        for (size_t i = 0; i < list.size(); ++i) {
            const json::HardToken& h = list[i];
            if (!json::finish_token(f->bytes + h.off, h.len, &val[i]))
                return fail(ctx, MCR_EFALLBACK, "json: the array element '%s' (byte %u) is not a number", json_excerpt(f, h.off).c_str(), h.off);
            idx[i] = descs[h.array].base + (long long)h.v * stride_n;
        }
        rc = patch_values(ctx, out_dev, idx, val);
        if (rc) return rc;
        for (size_t i = 0; i < desc_of.size(); ++i)
            if (desc_of[i] != SIZE_MAX) all_int[i] = not_int[desc_of[i]] ? 0 : 1;
        if (hard) *hard = (int64_t)list.size();
    } catch (const std::exception& e) { return fail(ctx, MCR_ENOMEM, "json: host allocation failed: %s", e.what()); }
    return MCR_OK;
}

}  // extern "C"
