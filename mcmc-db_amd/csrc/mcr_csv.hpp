// mcr_csv.hpp -- CmdStan chain CSV text -> draw tensor (replaces the DictReader / float() loop of
// src/mcmc_ref/cmdstan_generate.py:13-29 on the way into the statistics).
//
//   parse_field     one decimal field -> binary64 bits, Eisel-Lemire as published (Lemire 2021; Mushtak & Lemire 2023,
//                   no fallback): correctly rounded or reported as HARD, never guessed.  __host__ __device__: the CPU
//                   tests run the text the kernels run.
//   k_csv_lines     line index: every workgroup scans kChunk bytes of one file for data-row starts (count pass, then a
//                   write pass behind k_csv_scan's prefix sums).
//   k_csv_parse     one wavefront per data row: 64-byte batches, a ballot on ',' gives the field boundaries, a running
//                   popcount the column, each lane that owns a selected field parses it.
//   open_image      host: header, body offset and column names of a file image.
//   table mode      plain table CSVs by pyarrow.csv.read_csv's rules, as far as they are certified: strict_number (the
//                   strict number grammar), k_csv_lines<., true> (every non-empty line is a row), k_csv_table_parse,
//                   open_table_image.  What leaves the subset is reported, never guessed: the host reader decides.
//   finish_field    host: the float() grammar (no underscores) + strtod for the fields the device reported hard.
#pragma once

#include <hip/hip_runtime.h>

#include <clocale>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <locale.h>
#include <string>
#include <vector>

#include "mcr_pow5.h"

namespace mcr { namespace csv {

typedef uint64_t u64;
typedef uint32_t u32;

constexpr int kChunk = 16384;          // bytes of text per k_csv_lines workgroup (MCR_CSV_CHUNK)
constexpr int kLinesNT = 256;          // x 64 bytes per thread
constexpr int kParseWaves = 4;         // rows per k_csv_parse workgroup
constexpr int kSigDigits = 19;         // decimal digits that always fit a u64
static_assert(kLinesNT * 64 == kChunk, "line index geometry");

constexpr u64 kInfBits = 0x7FF0000000000000ull;

struct U128 { u64 hi, lo; };

__host__ __device__ inline U128 mul_64x64(u64 a, u64 b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return U128{__umul64hi(a, b), a * b};
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    return U128{(u64)(p >> 64), (u64)p};
#endif
}

__host__ __device__ inline int clz_64(u64 x)   // x != 0
{
#ifdef __HIP_DEVICE_COMPILE__
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// The bits of the binary64 nearest to w * 10^q (ties to even), w < 2^64.  `pow5` = kPow5 in this address space.
__host__ __device__ inline u64 eisel_lemire(u64 w, long long q, const u64* pow5)
{
    if (w == 0 || q < kPow5QMin) return 0;
    if (q > kPow5QMax) return kInfBits;
    const int lz = clz_64(w);
    w <<= lz;
    const u64* e = pow5 + 2 * (q - kPow5QMin);
    U128 pr = mul_64x64(w, e[0]);
    if ((pr.hi & 0x1FF) == 0x1FF) {                    // the 55 bits needed are not settled by the first product
        const U128 s = mul_64x64(w, e[1]);
        pr.lo += s.hi;
        if (s.hi > pr.lo) ++pr.hi;
    }
    const int upper = (int)(pr.hi >> 63), shift = upper + 9;
    u64 m = pr.hi >> shift;
    int p2 = (int)(((217706ll * q) >> 16) + 63) + upper - lz + 1023;
    if (p2 <= 0) {                                      // subnormal
        if (-p2 + 1 >= 64) return 0;
        m >>= -p2 + 1;
        m += m & 1;
        m >>= 1;
        return m;                                       // m == 2^52: the smallest normal, exponent field 1
    }
    if (pr.lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == pr.hi) m &= ~1ull;   // exact tie: to even
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) { m = 1ull << 52; ++p2; }
    m &= ~(1ull << 52);
    if (p2 >= 0x7FF) return kInfBits;
    return m | ((u64)p2 << 52);
}

__host__ __device__ inline bool field_ws(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// [ws] [+-] digits [. digits] [eE [+-] digits] [ws], at least one digit.  0: *bits is float(text); 1: HARD -- other
// text (inf, nan, underscores, an empty field, ...) or more than 19 significant digits whose two bracketing
// 19-digit values round differently.  `p` may point to device or host memory.
__host__ __device__ inline int parse_field(const char* p, size_t n, const u64* pow5, u64* bits)
{
    size_t i = 0, e = n;
    while (i < e && field_ws(p[i])) ++i;
    while (e > i && field_ws(p[e - 1])) --e;
    bool neg = false;
    if (i < e && (p[i] == '-' || p[i] == '+')) { neg = p[i] == '-'; ++i; }
    u64 w = 0;
    int nd = 0;
    long long q = 0;
    bool any = false, tail = false;
    for (; i < e; ++i) {
        const unsigned d = (unsigned)(p[i] - '0');
        if (d > 9) break;
        any = true;
        if (nd < kSigDigits) { if (w | d) { w = w * 10 + d; ++nd; } }
        else { ++q; tail |= d != 0; }
    }
    if (i < e && p[i] == '.') {
        for (++i; i < e; ++i) {
            const unsigned d = (unsigned)(p[i] - '0');
            if (d > 9) break;
            any = true;
            if (nd < kSigDigits) { if (w | d) { w = w * 10 + d; ++nd; } --q; }
            else tail |= d != 0;
        }
    }
    if (!any) return 1;
    if (i < e && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < e && (p[i] == '-' || p[i] == '+')) { eneg = p[i] == '-'; ++i; }
        if (i >= e || (unsigned)(p[i] - '0') > 9) return 1;
        long long ex = 0;
        for (; i < e; ++i) {
            const unsigned d = (unsigned)(p[i] - '0');
            if (d > 9) break;
            if (ex < 1000000000000ll) ex = ex * 10 + d;
        }
        q += eneg ? -ex : ex;
    }
    if (i != e) return 1;
    u64 b = eisel_lemire(w, q, pow5);
    if (tail && eisel_lemire(w + 1, q, pow5) != b) return 1;   // the dropped digits decide: the host finishes it
    *bits = b | ((u64)neg << 63);
    return 0;
}

constexpr u64 kMaxExactInt = 1ull << 53;   // integer literals above it leave the certified subset (pyarrow refuses the mix)
constexpr int kNumDecided = 0, kNumHard = 1, kNumNotNumber = -1, kNumBigInt = -2;   // strict_number

// The strict number grammar of the table CSV and the JSON reader (json::json_token adds what is JSON's own):
// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? and nothing around it -> the double pyarrow.csv gives the field.
// kNumDecided: *bits is the value; kNumHard: the dropped digits decide the rounding (the host finishes it);
// kNumNotNumber: outside the grammar; kNumBigInt: an integer literal above 2^53.  *is_int: no fraction and no
// exponent; -0 keeps its sign (bits of -0.0).  Like pyarrow, 1e400 is inf and 1e-400 is 0.
__host__ __device__ inline int strict_number(const char* t, size_t m, const u64* pow5, u64* bits, bool* is_int)
{
    *is_int = false;
    size_t k = (m && t[0] == '-') ? 1 : 0;
    if (k >= m || (unsigned)(t[k] - '0') > 9) return kNumNotNumber;
    const size_t d0 = k;
    u64 mag = 0;
    if (t[k] == '0') ++k;
    else for (; k < m && (unsigned)(t[k] - '0') <= 9; ++k) if (k - d0 < 17) mag = mag * 10 + (u64)(t[k] - '0');
    const size_t int_digits = k - d0;
    bool integer = true;
    if (k < m && t[k] == '.') {
        integer = false;
        const size_t f0 = ++k;
        while (k < m && (unsigned)(t[k] - '0') <= 9) ++k;
        if (k == f0) return kNumNotNumber;
    }
    if (k < m && (t[k] == 'e' || t[k] == 'E')) {
        integer = false;
        ++k;
        if (k < m && (t[k] == '+' || t[k] == '-')) ++k;
        const size_t x0 = k;
        while (k < m && (unsigned)(t[k] - '0') <= 9) ++k;
        if (k == x0) return kNumNotNumber;
    }
    if (k != m) return kNumNotNumber;
    *is_int = integer;
    if (integer && (int_digits > 16 || mag > kMaxExactInt)) return kNumBigInt;      // 17 digits: at least 10^16 > 2^53
    return parse_field(t, m, pow5, bits) == 0 ? kNumDecided : kNumHard;
}

// ---- device side ------------------------------------------------------------------------------------------------

struct FileDesc {       // absolute byte offsets into the call's text buffer (all files back to back, 256-byte aligned)
    u32 img, body, end; // image start, first byte after the header line, image end
    u32 ncols;          // header fields
    u32 chunk0;         // first k_csv_lines workgroup of this file
    u32 slot0;          // first entry of this file's column -> output slot table
};
struct HardField { u32 file, row, slot, off, len; };

constexpr int kErrFields = 1, kErrQuote = 2;   // low bits of the error key (file << 44 | row << 4 | kind), smallest wins

__device__ inline bool blank_ws(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// Is the line that starts at `s` a data row: not a comment, not whitespace only.
__device__ inline bool data_row(const char* text, u32 s, u32 end)
{
    if (text[s] == '#') return false;
    while (s < end && blank_ws(text[s])) ++s;
    return s < end && text[s] != '\n';
}

// Table mode: every line is a data row unless it is empty ("\n" or "\r\n" right at its start).
__device__ inline bool table_row(const char* text, u32 s, u32 end)
{
    if (text[s] == '\n') return false;
    return !(text[s] == '\r' && s + 1 < end && text[s + 1] == '\n');
}

template <int NT> __device__ inline u32 block_scan_excl(u32 v, u32* sh, u32* total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const u32 add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const u32 incl = sh[t];
    *total = sh[NT - 1];
    __syncthreads();
    return incl - v;
}

// Every '\n' at p, body - 1 <= p < end - 1, starts a line at p + 1 (the header's own newline starts the first one), and
// the thread that holds the newline owns that line.  WRITE = false: counts[chunk] = data rows owned by the chunk;
// WRITE = true: their start offsets go to rowtab[chunk_first[chunk] ...] in text order.  TABLE: table_row decides.
template <bool WRITE, bool TABLE = false>
__global__ __launch_bounds__(kLinesNT) void k_csv_lines(const char* __restrict__ text, const FileDesc* __restrict__ files,
                                                        const u32* __restrict__ chunk_file, u32* __restrict__ counts,
                                                        const u32* __restrict__ chunk_first, u32* __restrict__ rowtab)
{
    __shared__ u32 sh[kLinesNT];
    const u32 k = blockIdx.x;
    const FileDesc f = files[chunk_file[k]];
    const u32 pos0 = f.img + (k - f.chunk0) * (u32)kChunk + threadIdx.x * 64u;
    u64 starts = 0;                                    // bit j: the newline at pos0 + j starts a data row
    if (f.body < f.end && pos0 < f.end - 1 && pos0 + 64 > f.body - 1) {
        const uint4* src = reinterpret_cast<const uint4*>(text + pos0);      // pos0 is 64-byte aligned
        for (int v = 0; v < 4; ++v) {
            const uint4 q = src[v];
            const u32 wds[4] = {q.x, q.y, q.z, q.w};
            for (int j = 0; j < 4; ++j) {
                const u32 x = wds[j] ^ 0x0A0A0A0Au;
                if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) continue;  // no '\n' in these four bytes
                for (int b = 0; b < 4; ++b) {
                    const u32 p = pos0 + v * 16 + j * 4 + b;
                    if (((wds[j] >> (8 * b)) & 0xFF) == '\n' && p + 1 >= f.body && p + 1 < f.end &&
                        (TABLE ? table_row(text, p + 1, f.end) : data_row(text, p + 1, f.end)))
                        starts |= 1ull << (v * 16 + j * 4 + b);
                }
            }
        }
    }
    const u32 mine = (u32)__popcll(starts);
    u32 total;
    const u32 before = block_scan_excl<kLinesNT>(mine, sh, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) counts[k] = total;
    } else {
        u32 at = chunk_first[k] + before;
        for (u64 m = starts; m; m &= m - 1) rowtab[at++] = pos0 + (u32)__ffsll((long long)m);   // ffs is 1-based: p + 1
    }
}

// chunk_first = exclusive prefix sums of counts (n_chunks + 1 entries), file_row0[f] = first row of file f (n_files + 1).
__global__ __launch_bounds__(1024) void k_csv_scan(const u32* __restrict__ counts, u32 n_chunks, u32* __restrict__ chunk_first,
                                                   const FileDesc* __restrict__ files, u32 n_files, u32* __restrict__ file_row0)
{
    __shared__ u32 sh[1024];
    u32 carry = 0;
    for (u32 base = 0; base < n_chunks; base += 1024) {
        const u32 i = base + threadIdx.x;
        u32 total;
        const u32 ex = block_scan_excl<1024>(i < n_chunks ? counts[i] : 0, sh, &total);
        if (i < n_chunks) chunk_first[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) chunk_first[n_chunks] = carry;
    __syncthreads();
    for (u32 f = threadIdx.x; f <= n_files; f += 1024)
        file_row0[f] = f < n_files ? chunk_first[files[f].chunk0] : carry;
}

struct ParseArgs {
    const char* text; const FileDesc* files; const u32* rowtab; const u32* file_row0; const int* slots; const u64* pow5;
    long long max_rows; double* out; long long sf, sr, sc;
    HardField* hard; u32 hard_cap; u32* hard_count; unsigned long long* err;
};

// One wavefront per data row (blockIdx.y = file).  Lane l of a batch looks at byte pos + l; the batch of a row's first
// field starts one byte early, at the newline in front of the row, which stands in for that field's leading comma.
__global__ __launch_bounds__(kParseWaves * 64) void k_csv_parse(const ParseArgs a)
{
    const u32 fi = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kParseWaves + (threadIdx.x >> 6);
    const u32 r0 = a.file_row0[fi];
    const long long rows = (long long)(a.file_row0[fi + 1] - r0);
    if (row >= rows || row >= a.max_rows) return;
    const FileDesc f = a.files[fi];
    const int* slot = a.slots + f.slot0;
    u32 pos = a.rowtab[r0 + (u32)row] - 1;
    int col = -1;
    bool first = true;
    for (;;) {
        const u32 at = pos + lane;
        const char c = at < f.end ? a.text[at] : '\n';
        u64 comma = __ballot(c == ','), nl = __ballot(c == '\n'), quote = __ballot(c == '"');
        if (first) { comma |= 1; nl &= ~1ull; quote &= ~1ull; first = false; }
        const u64 term = nl & (0 - nl);                 // the row's terminator, if it is in this batch
        const u64 inrow = term ? term - 1 : ~0ull;
        comma &= inrow;
        if (quote & inrow) {
            if (lane == 0) atomicMin(a.err, ((unsigned long long)fi << 44) | ((unsigned long long)row << 4) | kErrQuote);
            return;
        }
        if ((comma >> lane) & 1) {
            const int mycol = col + 1 + __popcll(comma & ((1ull << lane) - 1));
            const int k = mycol < (int)f.ncols ? slot[mycol] : -1;
            if (k >= 0) {
                const u32 s = at + 1;
                const u64 after = (comma | term) & ~((2ull << lane) - 1);
                u32 e;
                if (after) e = pos + (u32)__ffsll((long long)after) - 1;
                else for (e = pos + 64; e < f.end && a.text[e] != ',' && a.text[e] != '\n'; ++e) {}
                u64 bits = 0;
                if (parse_field(a.text + s, e - s, a.pow5, &bits) == 0) {
                    a.out[(long long)fi * a.sf + row * a.sr + (long long)k * a.sc] = __longlong_as_double((long long)bits);
                } else {
                    const u32 h = atomicAdd(a.hard_count, 1u);
                    if (h < a.hard_cap) a.hard[h] = HardField{fi, (u32)row, (u32)k, s, e - s};
                }
            }
        }
        col += __popcll(comma);
        if (term) break;
        pos += 64;
    }
    if (col + 1 != (int)f.ncols && lane == 0)
        atomicMin(a.err, ((unsigned long long)fi << 44) | ((unsigned long long)row << 4) | kErrFields);
}

// out[idx[i]] = val[i]: the fields the host finished.
__global__ void k_csv_patch(double* __restrict__ out, const long long* __restrict__ idx, const double* __restrict__ val, u32 n)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[idx[i]] = val[i];
}

// ---- table mode ---------------------------------------------------------------------------------------------------

// Why a table leaves the certified subset: low bits of the error key (byte offset << 4 | kind), smallest offset wins.
constexpr int kTabErrFields = 1, kTabErrQuote = 2, kTabErrField = 3, kTabErrBigInt = 4, kTabErrIdField = 5;
constexpr int kSlotChain = -2, kSlotDraw = -3;   // slot table entries of the id columns (>= 0: a parameter's output column)

struct TableOut {       // where file f's values go
    long long base, sr, sc;     // out[base + row * sr + k * sc]
    long long ids;              // ids[ids + which * rows + row], which = 0 chain, 1 draw
    long long rows;             // rows of the file that are parsed
};
struct TableArgs {
    const char* text; const FileDesc* files; const u32* rowtab; const u32* file_row0; const int* slots; const u64* pow5;
    const TableOut* outs; double* out; long long* ids;
    unsigned char *all_int, *neg_zero;      // [slot0 + header column]: start 1 / 0; neg_zero: the integer literal -0 occurs
    HardField* hard; u32 hard_cap; u32* hard_count; unsigned long long* err;
};

// k_csv_parse's geometry (one wavefront per row, 64-byte batches, the lane at a field's leading comma parses it) by the
// table rules: EVERY field has to be a number of the strict grammar, a "\r" in front of the row's "\n" belongs to the
// line end, id columns are stored as int64, and a literal with a fraction or an exponent clears its column's all_int byte
// (every lane stores the same 0).  Anything else sets the error key and the host reader gets the file.
__global__ __launch_bounds__(kParseWaves * 64) void k_csv_table_parse(const TableArgs a)
{
    const u32 fi = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kParseWaves + (threadIdx.x >> 6);
    const TableOut o = a.outs[fi];
    if (row >= o.rows) return;
    const u32 r0 = a.file_row0[fi];
    const FileDesc f = a.files[fi];
    const int* slot = a.slots + f.slot0;
    const u32 start = a.rowtab[r0 + (u32)row];
    u32 pos = start - 1;
    int col = -1;
    bool first = true;
    for (;;) {
        const u32 at = pos + lane;
        const char c = at < f.end ? a.text[at] : '\n';
        u64 comma = __ballot(c == ','), nl = __ballot(c == '\n'), quote = __ballot(c == '"');
        if (first) { comma |= 1; nl &= ~1ull; quote &= ~1ull; first = false; }
        const u64 term = nl & (0 - nl);                 // the row's terminator, if it is in this batch
        const u64 inrow = term ? term - 1 : ~0ull;
        comma &= inrow;
        quote &= inrow;                                 // (the fields around it are still parsed: an earlier reason wins)
        if (quote && lane == 0) atomicMin(a.err, ((unsigned long long)(pos + (u32)__ffsll((long long)quote) - 1) << 4) | kTabErrQuote);
        if ((comma >> lane) & 1) {
            const int mycol = col + 1 + __popcll(comma & ((1ull << lane) - 1));
            if (mycol < (int)f.ncols) {
                const int k = slot[mycol];
                const u32 s = at + 1;
                const u64 after = (comma | term) & ~((2ull << lane) - 1);
                u32 e;
                if (after) e = pos + (u32)__ffsll((long long)after) - 1;
                else for (e = pos + 64; e < f.end && a.text[e] != ',' && a.text[e] != '\n'; ++e) {}
                u32 n = e - s;
                if (n && e < f.end && a.text[e] == '\n' && a.text[e - 1] == '\r') --n;     // "\r\n" ends the row
                u64 bits = 0;
                bool is_int = false;
                const int rc = strict_number(a.text + s, n, a.pow5, &bits, &is_int);
                if (rc < 0) {
                    const int kind = rc == kNumBigInt ? kTabErrBigInt : kTabErrField;
                    atomicMin(a.err, ((unsigned long long)s << 4) | kind);
                } else if (k >= 0) {
                    if (!is_int) a.all_int[f.slot0 + mycol] = 0;
                    else if (bits == 1ull << 63) a.neg_zero[f.slot0 + mycol] = 1;
                    if (rc == kNumDecided) {
                        a.out[o.base + row * o.sr + (long long)k * o.sc] = __longlong_as_double((long long)bits);
                    } else {
                        const u32 h = atomicAdd(a.hard_count, 1u);
                        if (h < a.hard_cap) a.hard[h] = HardField{fi, (u32)row, (u32)k, s, n};
                    }
                } else if (!is_int) {                   // (an integer literal is never hard)
                    atomicMin(a.err, ((unsigned long long)s << 4) | kTabErrIdField);
                } else {
                    a.ids[o.ids + (k == kSlotDraw ? o.rows : 0) + row] = (long long)__longlong_as_double((long long)bits);
                }
            }
        }
        col += __popcll(comma);
        if (term) break;
        pos += 64;
    }
    if (col + 1 != (int)f.ncols && lane == 0) atomicMin(a.err, ((unsigned long long)start << 4) | kTabErrFields);
}

// out[i * stride] = +0.0 where it is -0.0, i < n: a column of integer literals only is one pyarrow types int64, which
// has no negative zero, so the resident draws of such a column carry none either.
__global__ void k_csv_unsign_zero(double* __restrict__ out, long long stride, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && __double_as_longlong(out[i * stride]) == (long long)(1ull << 63)) out[i * stride] = 0.0;
}

// ---- host side --------------------------------------------------------------------------------------------------

struct Image {
    const char* bytes = nullptr; size_t len = 0;
    size_t body = 0;                     // first byte after the header line (== len: no data rows)
    std::vector<std::string> names;      // raw header fields, whitespace stripped; empty: no header line at all
    std::string path;                    // for messages ("" for a caller's image)
};

inline bool py_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// The first line that does not start with '#' is the header (cmdstan_generate.py:16-20); its fields are split on ','.
inline void open_image(Image& im, const char* bytes, size_t len)
{
    im.bytes = bytes; im.len = len; im.body = len; im.names.clear();
    size_t s = 0;
    while (s < len) {
        const char* nl = (const char*)memchr(bytes + s, '\n', len - s);
        const size_t e = nl ? (size_t)(nl - bytes) : len;
        if (bytes[s] != '#') {
            for (size_t a = s;;) {
                const char* cm = (const char*)memchr(bytes + a, ',', e - a);
                size_t b = cm ? (size_t)(cm - bytes) : e, x = a, y = b;
                while (x < y && py_space(bytes[x])) ++x;
                while (y > x && py_space(bytes[y - 1])) --y;
                im.names.emplace_back(bytes + x, y - x);
                if (!cm) break;
                a = b + 1;
            }
            im.body = nl ? e + 1 : len;
            return;
        }
        s = nl ? e + 1 : len;
    }
}

// Table mode: header conditions that leave the certified subset (MCR_CSV_T_*).
constexpr int kTabBom = 1, kTabDupName = 2, kTabEmptyName = 4, kTabHdrQuote = 8, kTabHdrCr = 16, kTabNoHeader = 32;

// pyarrow.csv.read_csv's header: the first non-empty line ("\n" and "\r\n" lines are skipped), split on ',', the names
// raw.  Returns the kTab* flags; *where = byte offset of the first flagged condition.
inline int open_table_image(Image& im, const char* bytes, size_t len, size_t* where)
{
    im.bytes = bytes; im.len = len; im.body = len; im.names.clear();
    *where = 0;
    int flags = 0;
    if (len >= 3 && (unsigned char)bytes[0] == 0xEF && (unsigned char)bytes[1] == 0xBB && (unsigned char)bytes[2] == 0xBF) flags |= kTabBom;
    size_t s = 0;
    while (s < len && (bytes[s] == '\n' || (bytes[s] == '\r' && s + 1 < len && bytes[s + 1] == '\n'))) s += bytes[s] == '\n' ? 1 : 2;
    if (s >= len) return flags | kTabNoHeader;
    const char* nl = (const char*)memchr(bytes + s, '\n', len - s);
    size_t e = nl ? (size_t)(nl - bytes) : len;
    im.body = nl ? e + 1 : len;
    if (nl && e > s && bytes[e - 1] == '\r') --e;
    auto flag = [&](int bit, size_t at) { if (!flags) *where = at; flags |= bit; };
    if (const void* q = memchr(bytes + s, '"', e - s)) flag(kTabHdrQuote, (size_t)((const char*)q - bytes));
    if (const void* r = memchr(bytes + s, '\r', e - s)) flag(kTabHdrCr, (size_t)((const char*)r - bytes));
    for (size_t a = s;;) {
        const char* cm = (const char*)memchr(bytes + a, ',', e - a);
        const size_t b = cm ? (size_t)(cm - bytes) : e;
        std::string name(bytes + a, b - a);
        if (name.empty()) flag(kTabEmptyName, a);
        else for (const std::string& x : im.names) if (x == name) { flag(kTabDupName, a); break; }
        im.names.push_back(std::move(name));
        if (!cm) break;
        a = b + 1;
    }
    return flags;
}

// A field the parser left: Python float()'s grammar without underscores -- a decimal, or signed inf / infinity / nan
// in any case -- converted by strtod in the C locale.  false: float() would raise ValueError.
inline bool finish_field(const char* p, size_t n, double* out)
{
    size_t i = 0, e = n;
    while (i < e && py_space(p[i])) ++i;
    while (e > i && py_space(p[e - 1])) --e;
    const std::string s(p + i, e - i);
    size_t k = 0;
    if (k < s.size() && (s[k] == '+' || s[k] == '-')) ++k;
    auto word = [&](const char* w) {
        const size_t m = strlen(w);
        if (s.size() - k != m) return false;
        for (size_t j = 0; j < m; ++j) if ((s[k + j] | 0x20) != w[j]) return false;
        return true;
    };
    bool ok = word("inf") || word("infinity") || word("nan");
    if (!ok) {
        size_t j = k, digits = 0;
        while (j < s.size() && s[j] >= '0' && s[j] <= '9') { ++j; ++digits; }
        if (j < s.size() && s[j] == '.') { ++j; while (j < s.size() && s[j] >= '0' && s[j] <= '9') { ++j; ++digits; } }
        ok = digits > 0;
        if (ok && j < s.size() && (s[j] == 'e' || s[j] == 'E')) {
            ++j;
            if (j < s.size() && (s[j] == '+' || s[j] == '-')) ++j;
            size_t ed = 0;
            while (j < s.size() && s[j] >= '0' && s[j] <= '9') { ++j; ++ed; }
            ok = ed > 0;
        }
        ok = ok && j == s.size();
    }
    if (!ok) return false;
    static locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    *out = c_locale ? strtod_l(s.c_str(), nullptr, c_locale) : strtod(s.c_str(), nullptr);
    return true;
}

}}  // namespace mcr::csv
