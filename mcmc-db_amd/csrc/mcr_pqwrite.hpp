// mcr_pqwrite.hpp -- device tensor -> Parquet draws file.
//
// The reference writes its draws with `pq.write_table(table, draws_path)` (src/mcmc_ref/convert.py:64).  This file is
// the replacement for that step, the mirror of mcr_parquet.hpp and written against the same published formats
// (parquet.thrift; Thrift compact protocol; Snappy format description; RLE / bit-packing hybrid):
//
//   device: k_pqw_encode   one workgroup per data page: the page's rows of one column through an element stride ->
//                          physical type (checked) -> definition levels + PLAIN values -> ONE raw Snappy stream in the
//                          page's worst-case slot; compressed size and min / max into the page's record
//           k_pqw_compact  slots + the host-built headers / footer -> one contiguous file image
//   host  : page headers, column chunk / row group / file metadata (Thrift compact protocol writer), statistics, and
//           a scalar restatement of the page compressor (mcr_parquet_write_host) that shares the token emission.
//
// Written: flat schemas of OPTIONAL INT32 / INT64 / DOUBLE leaves without nulls, data pages v1, PLAIN values, RLE
// levels, SNAPPY.  No dictionary pages.
//
// Matches are found at ELEMENT granularity.  Every element i gets a distance d[i] (in elements) to an equal earlier
// element of its page, or 0: d = 1 when the element equals its predecessor (constant runs, the `chain` column),
// otherwise the latest earlier element in the same slot of a hash table of element positions when its value is equal
// (discrete columns, `draw`, which repeats its chain's sequence).  The token stream follows from d alone: a maximal
// run of d == 0 is one literal, a maximal run of equal d > 0 is one copy at offset d * element size, cut into pieces
// of at most 64 bytes.  (Element i of such a run equals element i - d by construction, so the copy is exact, also
// where it overlaps itself.)  Distinct doubles have d == 0 everywhere: the page is one long literal, which is what
// k_pq_snappy copies at 16 bytes per lane.  Because the runs are a function of d, positions and sizes come out of
// workgroup scans and the tokens are written in parallel; the result does not depend on scheduling: hash slots
// are updated with atomicMax on (position, fingerprint), lookups are separated from updates by barriers.
// LDS of k_pqw_encode: 32 KiB table + 16 KiB d + 13 KiB of step values, small tables and scan buffers = 61 KiB,
// two workgroups per CU (160 KiB); the values themselves are not kept -- they are read again (L2) where needed.
#pragma once
#include "mcr_parquet.hpp"

#include <algorithm>
#include <cstdio>

namespace mcr {
namespace pqw {

constexpr int kPageRows = 8192;            // MCR_PQW_PAGE_ROWS: 64 KiB of 8-byte values
constexpr i64 kRowGroupRows = 1048576;     // MCR_PQW_ROW_GROUP_ROWS
constexpr int kNT = 256;                   // threads of k_pqw_encode
constexpr int kHashBits = 13;              // 8192 slots of (position + 1) << 16 | fingerprint
constexpr u32 kMaxOffset = 65535;          // copies carry 2-byte offsets at most (tag types 1 and 2)

enum : int { SRC_F64 = 0, SRC_I64 = 1, SRC_SEQ = 2 };

struct ColDev { const void* src; i64 stride, seq_div, seq_mod; int src_kind, type; };
struct PageW { int col; u32 nrows; i64 row0; u64 slot_off; };
struct PageRec { u32 comp_size, has_nan; u64 min_key, max_key; };     // keys: order-preserving unsigned images
struct Seg { u64 src_off, dst_off; u32 len, from_blob; };

#define MCR_HD __host__ __device__ inline

// ---- shared by the kernel and the host restatement --------------------------------------------------------------
MCR_HD u32 uvarint_len(u32 v) { u32 n = 1; while (v >= 0x80) { v >>= 7; ++n; } return n; }
MCR_HD u32 put_uvarint(unsigned char* p, u32 v)
{
    u32 n = 0;
    while (v >= 0x80) { p[n++] = (unsigned char)(v | 0x80); v >>= 7; }
    p[n++] = (unsigned char)v;
    return n;
}
MCR_HD u32 elem_size(int type) { return type == pq::T_INT32 ? 4u : 8u; }
// definition levels of n defined values of an OPTIONAL leaf: 4-byte length, then one RLE run "value 1, n times"
MCR_HD u32 level_block_len(u32 n) { return 4 + uvarint_len(n << 1) + 1; }
MCR_HD u32 put_level_block(unsigned char* p, u32 n)
{
    const u32 body = uvarint_len(n << 1) + 1;
    p[0] = (unsigned char)body; p[1] = 0; p[2] = 0; p[3] = 0;
    const u32 k = put_uvarint(p + 4, n << 1);
    p[4 + k] = 1;
    return 4 + body;
}
MCR_HD u32 literal_header_len(u32 len)
{
    const u32 n = len - 1;
    return n < 60 ? 1u : n < 256 ? 2u : n < 65536 ? 3u : n < (1u << 24) ? 4u : 5u;
}
MCR_HD u32 put_literal_header(unsigned char* p, u32 len)
{
    const u32 n = len - 1, h = literal_header_len(len);
    if (h == 1) { p[0] = (unsigned char)(n << 2); return 1; }
    p[0] = (unsigned char)((58 + h) << 2);
    for (u32 b = 0; b + 1 < h; ++b) p[1 + b] = (unsigned char)(n >> (8 * b));
    return h;
}
// one copy of len bytes (4 <= len <= 64, 1 <= off <= 65535)
MCR_HD u32 copy_len(u32 len, u32 off) { return (len <= 11 && off < 2048) ? 2u : 3u; }
MCR_HD u32 put_copy(unsigned char* p, u32 len, u32 off)
{
    if (len <= 11 && off < 2048) {
        p[0] = (unsigned char)(1 | ((len - 4) << 2) | ((off >> 8) << 5)); p[1] = (unsigned char)off;
        return 2;
    }
    p[0] = (unsigned char)(2 | ((len - 1) << 2)); p[1] = (unsigned char)off; p[2] = (unsigned char)(off >> 8);
    return 3;
}
// a run of `bytes` (a multiple of the element size) at one offset: pieces of 64 bytes and a rest of at least 4
MCR_HD u32 copy_run_len(u32 bytes, u32 off) { const u32 r = bytes & 63; return 3 * (bytes >> 6) + (r ? copy_len(r, off) : 0); }
MCR_HD u32 put_copy_run(unsigned char* p, u32 bytes, u32 off)
{
    u32 n = 0;
    for (u32 k = bytes >> 6; k; --k) n += put_copy(p + n, 64, off);
    if (bytes & 63) n += put_copy(p + n, bytes & 63, off);
    return n;
}
MCR_HD u32 run_len(u32 d, u32 elems, u32 es, u32 lvl)      // encoded size of one run; lvl: level bytes in front (first literal)
{
    if (d == 0) { const u32 b = elems * es + lvl; return literal_header_len(b) + b; }
    return copy_run_len(elems * es, d * es);
}
// worst case of a page's stream: preamble, and (Snappy's own bound) a tag byte per six payload bytes
MCR_HD u32 slot_bytes(u32 uncomp) { return (32 + uncomp + uncomp / 6 + 15) & ~15u; }

MCR_HD u64 hash_mul(u64 bits) { return bits * 0x9E3779B97F4A7C15ull; }

// Element `row` of the column in its physical type (the low 4 bytes for INT32).  false: an f64 source value that is
// no integer, or a value outside the target's range.
MCR_HD bool convert(const ColDev& c, i64 row, u64* bits)
{
    i64 iv;
    if (c.src_kind == SRC_F64) {
        const double v = ((const double*)c.src)[row * c.stride];
        if (c.type == pq::T_DOUBLE) { __builtin_memcpy(bits, &v, 8); return true; }
        if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) { *bits = 0; return false; }   // NaN fails too
        iv = (i64)v;
        if ((double)iv != v) { *bits = 0; return false; }
    } else if (c.src_kind == SRC_I64) iv = ((const i64*)c.src)[row * c.stride];
    else iv = (row / c.seq_div) % c.seq_mod;
    if (c.type == pq::T_INT32) {
        if (iv < -2147483648ll || iv > 2147483647ll) { *bits = 0; return false; }
        *bits = (u64)(u32)(int)iv;
        return true;
    }
    *bits = (u64)iv;
    return true;
}
// order-preserving unsigned image of a value (doubles: the usual sign flip; NaN never gets here)
MCR_HD u64 order_key(int type, u64 bits)
{
    if (type == pq::T_DOUBLE) return (bits >> 63) ? ~bits : bits ^ 0x8000000000000000ull;
    const i64 v = type == pq::T_INT32 ? (i64)(int)(u32)bits : (i64)bits;
    return (u64)v ^ 0x8000000000000000ull;
}
MCR_HD bool is_nan_bits(u64 bits) { return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// ---- device -------------------------------------------------------------------------------------------------------
// Inclusive scan of one u32 per thread over the workgroup (Hillis-Steele in LDS), left in out[0 .. kNT).  REVERSE
// scans from the last thread down.
template <bool REVERSE, class Op>
__device__ __forceinline__ void block_scan(u32 v, u32* buf /* 2 * kNT */, u32* out, Op op)
{
    const int idx = REVERSE ? kNT - 1 - (int)threadIdx.x : (int)threadIdx.x;
    int cur = 0;
    buf[idx] = v;
    __syncthreads();
    for (int o = 1; o < kNT; o <<= 1) {
        u32 x = buf[cur * kNT + idx];
        if (idx >= o) x = op(buf[cur * kNT + idx - o], x);
        buf[(cur ^ 1) * kNT + idx] = x;
        cur ^= 1;
        __syncthreads();
    }
    out[threadIdx.x] = buf[cur * kNT + idx];
    __syncthreads();
}

// One workgroup per data page.
__global__ __launch_bounds__(kNT) void k_pqw_encode(const ColDev* __restrict__ cols, const PageW* __restrict__ pages,
                                                    unsigned char* __restrict__ slots, PageRec* __restrict__ recs,
                                                    unsigned long long* __restrict__ err_row)
{
    __shared__ u32 tab[kPageRows];                  // hash table of element positions; afterwards the literal elements' output positions
    __shared__ unsigned short dist[kPageRows];
    __shared__ u64 s_val[2][kNT + 1];               // a step's values behind the last value of the step before it
    __shared__ u32 s_buf[2 * kNT], s_next[kNT], s_prev[kNT], s_pos[kNT];
    __shared__ u32 s_subA[2][kNT], s_subB[2][kNT];
    __shared__ u64 s_min, s_max;
    __shared__ u32 s_nan;
    const PageW pg = pages[blockIdx.x];
    const ColDev col = cols[pg.col];
    const int tid = threadIdx.x;
    const u32 n = pg.nrows, es = elem_size(col.type);
    unsigned char* const slot = slots + pg.slot_off;

    for (int k = tid; k < kPageRows; k += kNT) tab[k] = 0u;
    s_subA[0][tid] = 0u; s_subB[0][tid] = 0u;
    if (tid == 0) { s_min = ~0ull; s_max = 0ull; s_nan = 0u; }
    __syncthreads();

    // ---- A. d[i], kNT elements per step ----
    // tab holds the latest position of every slot from the steps before this one.  Inside a step, s_subA gets the last
    // lane of every (small) slot and s_subB the last of the others: a lane's candidate in its own step is the s_subB lane
    // when that is in front of it, which finds the partner of a value that occurs twice in a step.  Every table is
    // read and updated on different sides of a barrier; the step's small tables are cleared one step ahead.
    u64 kmin = ~0ull, kmax = 0ull; u32 nan = 0;
    for (u32 base = 0, par = 0; base < n; base += kNT, par ^= 1) {
        const u32 i = base + tid;
        const bool act = i < n;
        u64 bits = 0; u32 h = 0, hs = 0, fp = 0, e1 = 0;
        if (act) {
            if (!convert(col, pg.row0 + i, &bits)) atomicMin(&err_row[pg.col], (unsigned long long)(pg.row0 + i));
            if (col.type == pq::T_DOUBLE && is_nan_bits(bits)) nan = 1;
            else { const u64 key = order_key(col.type, bits); kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax; }
            const u64 m = hash_mul(bits);
            h = (u32)(m >> (64 - kHashBits)); fp = (u32)(m >> 32) & 0xFFFFu; hs = (u32)(m >> 24) & (kNT - 1);
            e1 = tab[h];
            s_val[par][1 + tid] = bits;
            atomicMax(&s_subA[par][hs], ((u32)(tid + 1) << 16) | fp);
        }
        __syncthreads();
        s_subA[par ^ 1][tid] = 0u; s_subB[par ^ 1][tid] = 0u;
        if (act) {
            atomicMax(&tab[h], ((i + 1) << 16) | fp);
            if ((s_subA[par][hs] >> 16) != (u32)(tid + 1)) atomicMax(&s_subB[par][hs], ((u32)(tid + 1) << 16) | fp);
        }
        __syncthreads();
        if (act) {
            u32 d = 0;
            if (i > 0 && s_val[par][tid] == bits) d = 1;
            else {
                const u32 eb = s_subB[par][hs];
                const u32 lane = (eb >> 16) - 1;                    // (eb == 0: no lane)
                if (eb != 0 && lane < (u32)tid && (eb & 0xFFFFu) == fp && s_val[par][1 + lane] == bits) d = (u32)tid - lane;
                else if ((e1 >> 16) != 0 && (e1 & 0xFFFFu) == fp) {
                    const u32 pos = (e1 >> 16) - 1;                 // in a step before this one: pos < i
                    u64 other;
                    convert(col, pg.row0 + pos, &other);
                    if (other == bits) d = i - pos;
                }
            }
            if (d * es > kMaxOffset) d = 0;
            dist[i] = (unsigned short)d;
            if (tid == kNT - 1) s_val[par ^ 1][0] = bits;
        }
    }
    atomicMin(&s_min, kmin); atomicMax(&s_max, kmax);
    if (nan) atomicOr(&s_nan, 1u);
    __syncthreads();

    // ---- B. runs: thread t owns the elements [lo, hi) ----
    const u32 E = (n + kNT - 1) / kNT;
    const u32 lo = min(n, (u32)tid * E), hi = min(n, lo + E);
    const u32 lvl = level_block_len(n), pre = uvarint_len(lvl + n * es);
    auto is_start = [&](u32 i) { return i == 0 || dist[i] != dist[i - 1]; };
    u32 first = n, last = 0;
    for (u32 i = lo; i < hi; ++i) if (is_start(i)) { if (first == n) first = i; last = i; }
    block_scan<true>(first, s_buf, s_next, [](u32 a, u32 b) { return a < b ? a : b; });     // first start at or behind my range
    block_scan<false>(last, s_buf, s_prev, [](u32 a, u32 b) { return a > b ? a : b; });     // last start up to my range
    const u32 after = tid + 1 < kNT ? s_next[tid + 1] : n;           // end of the run that is open at hi
    // f(start, end) for every run that starts in [lo, hi)
    auto for_runs = [&](auto&& f) {
        if (first >= hi) return;
        u32 s = first;
        for (u32 i = first + 1; i < hi; ++i) if (dist[i] != dist[i - 1]) { f(s, i); s = i; }
        f(s, after);
    };
    u32 mine = 0;
    for_runs([&](u32 s, u32 e) { mine += run_len(dist[s], e - s, es, s == 0 ? lvl : 0u); });
    block_scan<false>(mine, s_buf, s_pos, [](u32 a, u32 b) { return a + b; });
    u32 pos = pre + s_pos[tid] - mine;
    if (tid == 0) put_uvarint(slot, lvl + n * es);
    if (tid == kNT - 1) {
        PageRec r; r.comp_size = pre + s_pos[tid]; r.has_nan = s_nan; r.min_key = s_min; r.max_key = s_max;
        recs[blockIdx.x] = r;
    }
    // ---- C. tokens; tab[i] = output position of literal element i ----
    for_runs([&](u32 s, u32 e) {
        const u32 d = dist[s], own = min(e, hi);
        if (d == 0) {
            pos += put_literal_header(slot + pos, (e - s) * es + (s == 0 ? lvl : 0u));
            if (s == 0) pos += put_level_block(slot + pos, n);
            for (u32 j = s; j < own; ++j) tab[j] = pos + (j - s) * es;
            pos += (e - s) * es;
        } else {
            pos += put_copy_run(slot + pos, (e - s) * es, d * es);
            for (u32 j = s; j < own; ++j) tab[j] = ~0u;
        }
    });
    __syncthreads();
    {   // the elements in front of my first start belong to a run of an earlier thread
        const u32 lead_end = min(first, hi);
        if (lo < lead_end) {
            const u32 s = s_prev[tid - 1];               // (tid > 0: element 0 is a start)
            const bool lit = dist[s] == 0;
            const u32 b = tab[s];
            for (u32 j = lo; j < lead_end; ++j) tab[j] = lit ? b + (j - s) * es : ~0u;
        }
    }
    __syncthreads();
    for (u32 i = tid; i < n; i += kNT) {
        const u32 p = tab[i];
        if (p == ~0u) continue;
        u64 bits;
        convert(col, pg.row0 + i, &bits);
        if (es == 8) __builtin_memcpy(slot + p, &bits, 8);
        else { const u32 w = (u32)bits; __builtin_memcpy(slot + p, &w, 4); }
    }
}

// len bytes from src to dst by a workgroup of 256 threads, in 16-byte stores where dst allows.
__device__ __forceinline__ void wg_copy(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src, u32 len)
{
    const u32 tid = threadIdx.x;
    const u32 head = min(len, (16u - (u32)((uintptr_t)dst & 15)) & 15);
    if (tid < head) dst[tid] = src[tid];
    const u32 nv = (len - head) >> 4;
    for (u32 v = tid; v < nv; v += 256) {
        uint4 x;
        __builtin_memcpy(&x, src + head + 16 * (size_t)v, 16);      // the source is at any byte offset
        *(uint4*)(dst + head + 16 * (size_t)v) = x;
    }
    const u32 done = head + 16 * nv;
    if (tid < len - done) dst[done + tid] = src[done + tid];
}

// One workgroup per segment of the file image: a page's stream from its slot, or host-built bytes from the blob.
__global__ __launch_bounds__(256) void k_pqw_compact(const Seg* __restrict__ segs, const unsigned char* __restrict__ slots,
                                                     const unsigned char* __restrict__ blob, unsigned char* __restrict__ image)
{
    const Seg sg = segs[blockIdx.x];
    wg_copy(image + sg.dst_off, (sg.from_blob ? blob : slots) + sg.src_off, sg.len);
}

// ---- host ---------------------------------------------------------------------------------------------------------
// The scalar restatement of k_pqw_encode: d from one sequential pass (every earlier element is visible to the hash
// table), the same run rule, the same token emission.  Appends the stream to `out`.  Returns the first row that does
// not convert, or -1.
inline i64 encode_page_host(const ColDev& col, const PageW& pg, std::vector<unsigned char>& out, PageRec& rec)
{
    const u32 n = pg.nrows, es = elem_size(col.type), lvl = level_block_len(n);
    std::vector<u64> v(n);
    std::vector<u32> d(n, 0), tab((size_t)1 << kHashBits, 0);
    rec.has_nan = 0; rec.min_key = ~0ull; rec.max_key = 0;
    for (u32 i = 0; i < n; ++i) {
        if (!convert(col, pg.row0 + i, &v[i])) return pg.row0 + i;
        if (col.type == pq::T_DOUBLE && is_nan_bits(v[i])) rec.has_nan = 1;
        else { const u64 k = order_key(col.type, v[i]); rec.min_key = std::min(rec.min_key, k); rec.max_key = std::max(rec.max_key, k); }
        const u32 h = (u32)(hash_mul(v[i]) >> (64 - kHashBits));
        if (i > 0 && v[i - 1] == v[i]) d[i] = 1;
        else if (tab[h] && v[tab[h] - 1] == v[i]) d[i] = i - (tab[h] - 1);
        if (d[i] * es > kMaxOffset) d[i] = 0;
        tab[h] = i + 1;
    }
    const size_t at = out.size();
    out.resize(at + slot_bytes(lvl + n * es));
    unsigned char* p = out.data() + at;
    u32 pos = put_uvarint(p, lvl + n * es);
    for (u32 s = 0; s < n;) {
        u32 e = s + 1;
        while (e < n && d[e] == d[s]) ++e;
        if (d[s] == 0) {
            pos += put_literal_header(p + pos, (e - s) * es + (s == 0 ? lvl : 0u));
            if (s == 0) pos += put_level_block(p + pos, n);
            for (u32 j = s; j < e; ++j, pos += es) memcpy(p + pos, &v[j], es);       // little-endian host
        } else pos += put_copy_run(p + pos, (e - s) * es, d[s] * es);
        s = e;
    }
    rec.comp_size = pos;
    out.resize(at + pos);
    return -1;
}

// Thrift compact protocol writer (the mirror of pq::Thrift)
struct ThriftW {
    std::vector<unsigned char>& b;
    std::vector<int> stack; int last = 0;
    explicit ThriftW(std::vector<unsigned char>& out) : b(out) {}
    void varint(u64 v) { while (v >= 0x80) { b.push_back((unsigned char)(v | 0x80)); v >>= 7; } b.push_back((unsigned char)v); }
    void zigzag(i64 v) { varint(((u64)v << 1) ^ (u64)(v >> 63)); }
    void field(int id, int type)
    {
        const int delta = id - last;
        if (delta > 0 && delta <= 15) b.push_back((unsigned char)((delta << 4) | type));
        else { b.push_back((unsigned char)type); zigzag(id); }
        last = id;
    }
    void i32(int id, i64 v) { field(id, 5); zigzag(v); }
    void i64f(int id, i64 v) { field(id, 6); zigzag(v); }
    void bytes(const void* s, size_t n) { varint(n); b.insert(b.end(), (const unsigned char*)s, (const unsigned char*)s + n); }
    void binary(int id, const void* s, size_t n) { field(id, 8); bytes(s, n); }
    void str(int id, const std::string& s) { binary(id, s.data(), s.size()); }
    void list(int id, int etype, size_t n)
    {
        field(id, 9);
        if (n < 15) b.push_back((unsigned char)((n << 4) | etype));
        else { b.push_back((unsigned char)(0xF0 | etype)); varint(n); }
    }
    void begin() { stack.push_back(last); last = 0; }                 // a struct as list element or after field(id, 12)
    void begin(int id) { field(id, 12); begin(); }
    void end() { b.push_back(0); last = stack.back(); stack.pop_back(); }
};

struct ColSpec { std::string name; int type; };
struct PagePlan { int col, rg; u32 nrows; i64 row0; u32 uncomp; };
struct Layout {
    std::vector<unsigned char> blob;      // "PAR1", every page header, footer + length + "PAR1"
    std::vector<Seg> segs;                // in file order
    size_t image_bytes = 0;
};

inline std::string created_by(int version)
{
    char s[64];
    snprintf(s, sizeof s, "mcmc-ref-hip version %d.%d.%d", version / 10000, version / 100 % 100, version % 100);
    return s;
}

// Pages in file order: row group, column, page.
inline void plan_pages(int n_cols, const int* types, i64 rows, i64 rg_rows, std::vector<PagePlan>& pages)
{
    int rg = 0;
    for (i64 r0 = 0; r0 < rows; r0 += rg_rows, ++rg) {
        const i64 r1 = std::min(rows, r0 + rg_rows);
        for (int c = 0; c < n_cols; ++c)
            for (i64 p0 = r0; p0 < r1; p0 += kPageRows) {
                const u32 n = (u32)std::min<i64>(kPageRows, r1 - p0);
                pages.push_back(PagePlan{c, rg, n, p0, level_block_len(n) + n * elem_size(types[c])});
            }
    }
}

// Upper bound of the image for the pages' worst-case streams (the device image is carved before the sizes are known).
inline size_t image_bound(const std::vector<ColSpec>& cols, const std::vector<PagePlan>& pages)
{
    size_t names = 0;
    for (const ColSpec& c : cols) names += c.name.size();
    const size_t n_rg = pages.empty() ? 0 : (size_t)pages.back().rg + 1;
    size_t b = 256 + cols.size() * 48 + 2 * names + n_rg * (64 + cols.size() * 160 + 2 * names);
    for (const PagePlan& p : pages) b += 48 + slot_bytes(p.uncomp);
    return b;
}

// value of a key as the `type`'s PLAIN bytes, with the zero rule of doubles (min: -0.0, max: +0.0)
inline size_t stat_bytes(int type, u64 key, bool is_min, unsigned char* out)
{
    if (type == pq::T_DOUBLE) {
        u64 bits = (key >> 63) ? key ^ 0x8000000000000000ull : ~key;
        if ((bits << 1) == 0) bits = is_min ? 0x8000000000000000ull : 0ull;
        memcpy(out, &bits, 8);
        return 8;
    }
    const u64 bits = key ^ 0x8000000000000000ull;
    memcpy(out, &bits, 8);
    return type == pq::T_INT32 ? 4 : 8;
}

// Headers, offsets and the footer from the pages' records.  slot_off[k]: where page k's stream lies (device: in the
// slot buffer).  The segments alternate blob pieces and payloads, in file order.
inline void build_layout(const std::vector<ColSpec>& cols, const std::vector<PagePlan>& pages, const std::vector<PageRec>& recs,
                         const std::vector<u64>& slot_off, i64 rows, int version, Layout& L)
{
    std::vector<unsigned char>& blob = L.blob;
    size_t file_off = 0;
    auto blob_seg = [&](size_t from) {
        const size_t len = blob.size() - from;
        L.segs.push_back(Seg{(u64)from, (u64)file_off, (u32)len, 1u});
        file_off += len;
    };
    blob.insert(blob.end(), {'P', 'A', 'R', '1'});
    size_t pending = 0;                       // blob bytes not yet in a segment
    struct ChunkInfo { i64 first_off = 0, comp = 0, uncomp = 0, values = 0; u64 kmin = ~0ull, kmax = 0; bool nan = false; };
    const int n_cols = (int)cols.size(), n_rg = pages.empty() ? 0 : pages.back().rg + 1;
    std::vector<ChunkInfo> chunks((size_t)n_rg * n_cols);
    for (size_t k = 0; k < pages.size(); ++k) {
        const PagePlan& p = pages[k];
        ChunkInfo& ch = chunks[(size_t)p.rg * n_cols + p.col];
        const size_t h0 = blob.size();
        ThriftW t(blob);
        t.begin();
        t.i32(1, pq::PAGE_DATA); t.i32(2, p.uncomp); t.i32(3, recs[k].comp_size);
        t.begin(5);
        t.i32(1, p.nrows); t.i32(2, pq::ENC_PLAIN); t.i32(3, pq::ENC_RLE); t.i32(4, pq::ENC_RLE);
        t.end();
        t.end();
        const size_t hlen = blob.size() - h0;
        if (ch.values == 0) ch.first_off = (i64)(file_off + (h0 - pending));
        ch.values += p.nrows; ch.comp += (i64)hlen + recs[k].comp_size; ch.uncomp += (i64)hlen + p.uncomp;
        ch.kmin = std::min(ch.kmin, recs[k].min_key); ch.kmax = std::max(ch.kmax, recs[k].max_key); ch.nan |= recs[k].has_nan != 0;
        blob_seg(pending);
        pending = blob.size();
        L.segs.push_back(Seg{slot_off[k], (u64)file_off, recs[k].comp_size, 0u});
        file_off += recs[k].comp_size;
    }
    // footer
    const size_t f0 = blob.size();
    ThriftW t(blob);
    t.begin();
    t.i32(1, 1);
    t.list(2, 12, cols.size() + 1);
    t.begin(); t.str(4, "schema"); t.i32(5, (i64)cols.size()); t.end();
    for (const ColSpec& c : cols) { t.begin(); t.i32(1, c.type); t.i32(3, 1 /* OPTIONAL */); t.str(4, c.name); t.end(); }
    t.i64f(3, rows);
    t.list(4, 12, (size_t)n_rg);
    for (int g = 0; g < n_rg; ++g) {
        i64 total_u = 0, total_c = 0, g_rows = 0;
        for (int c = 0; c < n_cols; ++c) { const ChunkInfo& ch = chunks[(size_t)g * n_cols + c]; total_u += ch.uncomp; total_c += ch.comp; g_rows = ch.values; }
        t.begin();
        t.list(1, 12, (size_t)n_cols);
        for (int c = 0; c < n_cols; ++c) {
            const ChunkInfo& ch = chunks[(size_t)g * n_cols + c];
            t.begin();
            t.i64f(2, 0);
            t.begin(3);
            t.i32(1, cols[c].type);
            t.list(2, 5, 2); t.zigzag(pq::ENC_PLAIN); t.zigzag(pq::ENC_RLE);
            t.list(3, 8, 1); t.bytes(cols[c].name.data(), cols[c].name.size());
            t.i32(4, pq::CODEC_SNAPPY);
            t.i64f(5, ch.values); t.i64f(6, ch.uncomp); t.i64f(7, ch.comp); t.i64f(9, ch.first_off);
            t.begin(12);
            t.i64f(3, 0);
            if (!ch.nan) {
                unsigned char sb[8];
                size_t sn = stat_bytes(cols[c].type, ch.kmax, false, sb); t.binary(5, sb, sn);
                sn = stat_bytes(cols[c].type, ch.kmin, true, sb); t.binary(6, sb, sn);
            }
            t.end();
            t.end();
            t.end();
        }
        t.i64f(2, total_u); t.i64f(3, g_rows); t.i64f(5, chunks[(size_t)g * n_cols].first_off); t.i64f(6, total_c);
        t.field(7, 4); t.zigzag(g);
        t.end();
    }
    t.str(6, created_by(version));
    t.list(7, 12, cols.size());
    for (size_t c = 0; c < cols.size(); ++c) { t.begin(); t.begin(1); t.end(); t.end(); }      // TYPE_ORDER: min_value / max_value are meaningful
    t.end();
    const u32 flen = (u32)(blob.size() - f0);
    unsigned char le[4]; memcpy(le, &flen, 4);
    blob.insert(blob.end(), le, le + 4);
    blob.insert(blob.end(), {'P', 'A', 'R', '1'});
    blob_seg(pending);
    L.image_bytes = file_off;
}

}  // namespace pqw
}  // namespace mcr
