// mcr_csvwrite.hpp -- device columns -> CSV text: the other direction of mcr_csv.hpp.
//
// The reference's `mcmc-ref draws` writes its table with `pyarrow.csv.write_csv` (src/mcmc_ref/cli.py:100-127).  This
// file produces the same bytes from columns in device memory (the addressing of mcr_pq_column):
//
//   device: k_csvw_format   one workgroup per tile of kTileFields fields of the row-major field sequence: every field
//                           once through the shortest-digits conversion into registers, lengths at their row-major
//                           index in LDS, one block scan, the tile's text assembled in LDS and stored with 16-byte
//                           writes into the tile's worst-case slot; the tile's byte count
//           k_csvw_scan     tile sizes -> 64-bit offsets (one workgroup; not hot)
//           k_csvw_compact  slots -> one contiguous text image
//           k_select_rows   stable compaction: the rows whose chain id is in a list, in file order
//   host  : the header line, and mcr_csv_write_host, which walks the same tiles with the same formatter.
//
// Field grammar (what pyarrow prints for float64 / int64 without nulls): nan | [-]inf | [-]0 | the SHORTEST digits
// d1..dn that read back to the value (the closest such string), v = d1.d2..dn x 10^e, written positionally when
// -6 <= e <= 9 and as d1[.d2..dn]e[+-]E otherwise; integers in plain decimal.  At most 25 bytes.
//
// Shortest digits: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020), integer arithmetic only: three
// 64 x 128-bit products against g(k) of mcr_pow10.h (indexed per lane, so the table is read through a pointer
// with vector loads), no dependence between fields.
// LDS of k_csvw_format: 52 KiB text + 8 KiB lengths / offsets + 3 KiB scan = 63 KiB, two workgroups per CU (160 KiB).
#pragma once
#include "mcr_csv.hpp"
#include "mcr_pow10.h"
#include "mcr_pqwrite.hpp"

namespace mcr {
namespace csvw {

constexpr int kTileFields = 2048;          // MCR_CSVW_TILE_FIELDS
constexpr int kNT = pqw::kNT;              // threads of k_csvw_format (pqw::block_scan is written for this many)
constexpr int kPerThread = kTileFields / kNT;
constexpr int kFieldMax = 26;              // the longest field (25 bytes: -0.00000ddddddddddddddddd) and its separator
constexpr int kSelectNT = 256;             // MCR_SELECT_BLOCK_ROWS: one row per thread of k_select_rows
static_assert(kTileFields % kNT == 0 && (kTileFields * kFieldMax) % 16 == 0, "tile geometry");

enum : int { HEADER_QUOTED = 0, HEADER_PLAIN = 1, HEADER_NONE = 2 };
enum : int { KIND_NUM = 0, KIND_INT = 1, KIND_INF = 2, KIND_NAN = 3 };

using pqw::ColDev;

// A field before it is text.  NUM: m x 10^k, m without trailing zeros, n digits.  INT: the magnitude m (zeros of either
// sign included), n digits.
struct Dec { u64 m; short k; unsigned char n, tag; };     // tag: kind | negative << 7
MCR_HD int dec_kind(const Dec& d) { return d.tag & 0x7F; }
MCR_HD u32 dec_neg(const Dec& d) { return d.tag >> 7; }

MCR_HD int count_digits(u64 m)             // m < 10^19
{
    int n = 1;
    for (u64 p = 10; n < 19 && m >= p; p *= 10) ++n;
    return n;
}

MCR_HD Dec dec_int(i64 v)
{
    const bool neg = v < 0;
    const u64 m = neg ? 0 - (u64)v : (u64)v;
    return Dec{m, 0, (unsigned char)count_digits(m), (unsigned char)(KIND_INT | (neg ? 0x80 : 0))};
}

// y = floor(g * cp / 2^128) with the sticky bit of what was shifted out (g = ghi 2^64 + glo)
MCR_HD u64 round_to_odd(u64 ghi, u64 glo, u64 cp)
{
    const csv::U128 x = csv::mul_64x64(glo, cp), y = csv::mul_64x64(ghi, cp);
    const u64 y0 = y.lo + x.hi, y1 = y.hi + (y0 < y.lo ? 1 : 0);
    return y1 | (y0 > 1 ? 1 : 0);
}

// The shortest decimal of a binary64 (Schubfach).  `pow10` = kPow10 in this address space.
MCR_HD Dec dec_double(u64 bits, const uint64_t* pow10)
{
    const unsigned char sign = (unsigned char)((bits >> 63) << 7);
    const u64 frac = bits & 0x000FFFFFFFFFFFFFull;
    const int be = (int)((bits >> 52) & 0x7FF);
    if (be == 0x7FF) return Dec{0, 0, 0, (unsigned char)(frac ? KIND_NAN : (KIND_INF | sign))};
    if (be == 0 && frac == 0) return Dec{0, 0, 1, (unsigned char)(KIND_INT | sign)};
    u64 c, m;
    int q, k;
    bool small_int = false;
    if (be != 0) {
        c = frac | 0x0010000000000000ull;
        q = be - 1075;
        small_int = q <= 0 && q > -53 && (c & ((1ull << -q) - 1)) == 0;      // an integer below 2^53: its own digits
    } else { c = frac; q = -1074; }
    if (small_int) { m = c >> -q; k = 0; }
    else {
        const bool even = (c & 1) == 0;
        const bool lower_closer = frac == 0 && be > 1;
        const u64 cbl = 4 * c - 2 + (lower_closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
        k = (q * 1262611 - (lower_closer ? 524031 : 0)) >> 22;                // floor(log10(2^q)) or floor(log10(3/4 2^q))
        const int h = q + ((-k * 1741647) >> 19) + 1;                        // q + floor(log2(10^-k)) + 1, in 1 .. 4
        const uint64_t* g = pow10 + 2 * (-k - kPow10KMin);
        const u64 ghi = g[0], glo = g[1];
        const u64 vbl = round_to_odd(ghi, glo, cbl << h), vb = round_to_odd(ghi, glo, cb << h), vbr = round_to_odd(ghi, glo, cbr << h);
        const u64 lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
        const u64 s = vb >> 2;
        bool done = false;
        if (s >= 10) {                                                       // one digit fewer, when exactly one candidate is inside
            const u64 sp = s / 10;
            const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
            if (up_in != wp_in) { m = sp + (wp_in ? 1 : 0); k += 1; done = true; }
        }
        if (!done) {
            const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
            if (u_in != w_in) m = s + (w_in ? 1 : 0);
            else {                                                           // both or none: the closer one, ties to even
                const u64 mid = 4 * s + 2;
                m = s + ((vb > mid || (vb == mid && (s & 1))) ? 1 : 0);
            }
        }
    }
    for (u64 t = m / 10; t * 10 == m; t = m / 10) { m = t; ++k; }             // (m != 0)
    return Dec{m, (short)k, (unsigned char)count_digits(m), (unsigned char)(KIND_NUM | sign)};
}

MCR_HD bool dec_positional(int e) { return e >= -6 && e <= 9; }

// Bytes of the field's text.
MCR_HD u32 dec_len(const Dec& d)
{
    const int kind = dec_kind(d);
    const u32 neg = dec_neg(d), n = d.n;
    if (kind == KIND_INT) return neg + n;
    if (kind == KIND_INF) return neg + 3;
    if (kind == KIND_NAN) return 3;
    const int e = d.k + (int)n - 1;
    if (dec_positional(e)) return neg + (e < 0 ? 1 + (u32)-e + n : d.k >= 0 ? n + (u32)d.k : n + 1);
    const int ae = e < 0 ? -e : e;
    return neg + n + (n > 1 ? 1 : 0) + 2 + (ae >= 100 ? 3 : ae >= 10 ? 2 : 1);
}

// The n digits of m, digit i at out[i], or one further when i >= dot, with the point at out[dot] (dot >= n: no point).
MCR_HD void put_digits(unsigned char* out, u64 m, int n, int dot)
{
    if (dot < n) out[dot] = '.';
    int i = n - 1;
    for (; (m >> 32) != 0; --i) { const u64 t = m / 10; out[i + (i >= dot ? 1 : 0)] = (unsigned char)('0' + (u32)(m - t * 10)); m = t; }
    for (u32 w = (u32)m; i >= 0; --i) { const u32 t = w / 10; out[i + (i >= dot ? 1 : 0)] = (unsigned char)('0' + (w - t * 10)); w = t; }
}

// Writes the dec_len(d) bytes of the field.
MCR_HD void dec_put(const Dec& d, unsigned char* out)
{
    const int kind = dec_kind(d), n = d.n;
    if (kind == KIND_NAN) { out[0] = 'n'; out[1] = 'a'; out[2] = 'n'; return; }
    if (dec_neg(d)) *out++ = '-';
    if (kind == KIND_INF) { out[0] = 'i'; out[1] = 'n'; out[2] = 'f'; return; }
    if (kind == KIND_INT) { put_digits(out, d.m, n, n); return; }
    const int e = d.k + n - 1;
    if (dec_positional(e)) {
        if (e < 0) {                                  // 0.000ddd
            out[0] = '0'; out[1] = '.';
            for (int z = 0; z < -e - 1; ++z) out[2 + z] = '0';
            put_digits(out + 1 - e, d.m, n, n);
        } else if (d.k >= 0) {                        // ddd000
            put_digits(out, d.m, n, n);
            for (int z = 0; z < d.k; ++z) out[n + z] = '0';
        } else put_digits(out, d.m, n, e + 1);        // dd.ddd
        return;
    }
    put_digits(out, d.m, n, 1);
    out += n + (n > 1 ? 1 : 0);
    out[0] = 'e'; out[1] = e < 0 ? '-' : '+';
    const u32 ae = (u32)(e < 0 ? -e : e);
    put_digits(out + 2, ae, ae >= 100 ? 3 : ae >= 10 ? 2 : 1, 3);
}

// Field (row, col) of the source.  false: an f64 source declared integer holds a value that is none.
MCR_HD bool field_dec(const ColDev& c, i64 row, const uint64_t* pow10, Dec* d)
{
    u64 bits;
    const bool ok = pqw::convert(c, row, &bits);
    *d = c.type == pq::T_DOUBLE ? dec_double(bits, pow10) : dec_int((i64)bits);
    return ok;
}

// ---- tiles of the row-major field sequence ----------------------------------------------------------------------
// n_cols <= kTileFields: R = kTileFields / n_cols whole rows per tile.  Wider tables: a row is cut into `parts` tiles.
struct Tiling { int n_cols, R, parts; };
struct Tile { i64 row0; int nr, col0, nc; };
MCR_HD Tiling make_tiling(int n_cols)
{
    if (n_cols <= kTileFields) return Tiling{n_cols, kTileFields / n_cols, 1};
    return Tiling{n_cols, 1, (n_cols + kTileFields - 1) / kTileFields};
}
MCR_HD i64 tile_count(const Tiling& g, i64 rows) { return g.parts == 1 ? (rows + g.R - 1) / g.R : rows * g.parts; }
MCR_HD Tile tile_at(const Tiling& g, i64 rows, i64 t)
{
    if (g.parts == 1) { const i64 r0 = t * g.R; return Tile{r0, (int)(rows - r0 < g.R ? rows - r0 : g.R), 0, g.n_cols}; }
    const int c0 = (int)(t % g.parts) * kTileFields;
    return Tile{t / g.parts, 1, c0, g.n_cols - c0 < kTileFields ? g.n_cols - c0 : kTileFields};
}
// worst case of a tile's text, 16-byte aligned
MCR_HD u32 slot_bytes(const Tiling& g)
{
    const u32 f = g.parts == 1 ? (u32)(g.R * g.n_cols) : (u32)kTileFields;
    return (f * kFieldMax + 15) & ~15u;
}

// ---- device -------------------------------------------------------------------------------------------------------
struct FormatArgs {
    const ColDev* cols; Tiling tiling;
    i64 first, count;          // the call's rows [first, first + count) of the row list
    const i64* rows_dev;       // the row list, or null for the identity
    i64 src_rows;              // rows of the source: the bound of the list's entries
    const uint64_t* pow10;
    unsigned char* slots; u32* sizes;
    unsigned long long* err;   // [0]: first list position with a row outside the source; [1]: first field (position * n_cols + column) that is no integer
};

__global__ __launch_bounds__(kNT) void k_csvw_format(const FormatArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_text[kTileFields * kFieldMax];
    __shared__ u32 s_off[kTileFields];               // lengths (separator included), then exclusive offsets
    __shared__ u32 s_buf[2 * kNT], s_sum[kNT];
    const int tid = threadIdx.x;
    const Tile tl = tile_at(a.tiling, a.count, blockIdx.x);
    const u32 nr = (u32)tl.nr, nc = (u32)tl.nc, nf = nr * nc;

    // work item j = column * nr + row: consecutive lanes read consecutive rows of one column
    Dec dec[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const u32 j = (u32)tid + (u32)i * kNT;
        dec[i] = Dec{0, 0, 1, KIND_INT};
        if (j < nf) {
            const u32 c = j / nr, r = j - c * nr;
            const i64 pos = a.first + tl.row0 + r;
            i64 row = pos;
            if (a.rows_dev) {
                row = a.rows_dev[pos];
                if (row < 0 || row >= a.src_rows) { atomicMin(&a.err[0], (unsigned long long)pos); row = -1; }
            }
            if (row >= 0 && !field_dec(a.cols[tl.col0 + c], row, a.pow10, &dec[i]))
                atomicMin(&a.err[1], (unsigned long long)pos * (unsigned long long)a.tiling.n_cols + (unsigned long long)(tl.col0 + c));
            s_off[r * nc + c] = dec_len(dec[i]) + 1;
        }
    }
    __syncthreads();
    // exclusive offsets: thread t owns the row-major fields [t * kPerThread, (t + 1) * kPerThread)
    u32 mine = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) { const u32 f = (u32)tid * kPerThread + i; if (f < nf) mine += s_off[f]; }
    pqw::block_scan<false>(mine, s_buf, s_sum, [](u32 x, u32 y) { return x + y; });
    const u32 total = s_sum[kNT - 1];
    u32 at = s_sum[tid] - mine;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const u32 f = (u32)tid * kPerThread + i;
        if (f < nf) { const u32 len = s_off[f]; s_off[f] = at; at += len; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const u32 j = (u32)tid + (u32)i * kNT;
        if (j < nf) {
            const u32 c = j / nr, r = j - c * nr;
            unsigned char* p = s_text + s_off[r * nc + c];
            dec_put(dec[i], p);
            p[dec_len(dec[i])] = tl.col0 + (int)c == a.tiling.n_cols - 1 ? '\n' : ',';
        }
    }
    __syncthreads();
    uint4* dst = (uint4*)(a.slots + (size_t)blockIdx.x * slot_bytes(a.tiling));       // (total <= the slot's bytes, both of 16-byte grain)
    for (u32 v = tid; v < (total + 15) / 16; v += kNT) dst[v] = ((const uint4*)s_text)[v];
    if (tid == 0) a.sizes[blockIdx.x] = total;
}

// offs[0 .. n] = exclusive prefix sums of sizes[0 .. n), 64-bit.  One workgroup.
__global__ __launch_bounds__(256) void k_csvw_scan(const u32* __restrict__ sizes, i64 n, u64* __restrict__ offs)
{
    __shared__ u64 s_part[256];
    const i64 per = (n + 255) / 256, lo = min(n, (i64)threadIdx.x * per), hi = min(n, lo + per);
    u64 sum = 0;
    for (i64 k = lo; k < hi; ++k) sum += sizes[k];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 acc = 0;
        for (int t = 0; t < 256; ++t) { const u64 v = s_part[t]; s_part[t] = acc; acc += v; }
        offs[n] = acc;
    }
    __syncthreads();
    u64 acc = s_part[threadIdx.x];
    for (i64 k = lo; k < hi; ++k) { offs[k] = acc; acc += sizes[k]; }
}

// One workgroup per tile: its text from the slot to its place in the image.
__global__ __launch_bounds__(256) void k_csvw_compact(const unsigned char* __restrict__ slots, u32 slot_stride, const u32* __restrict__ sizes,
                                                      const u64* __restrict__ offs, unsigned char* __restrict__ image)
{
    pqw::wg_copy(image + offs[blockIdx.x], slots + (size_t)blockIdx.x * slot_stride, sizes[blockIdx.x]);
}

// Stable compaction of the rows whose chain id is in `list`.  EMIT = false: counts[block] = the block's selected rows;
// EMIT = true (after k_csvw_scan of the counts): the rows' indices at offs[block] onwards, in order.
template <bool EMIT>
__global__ __launch_bounds__(kSelectNT) void k_select_rows(const i64* __restrict__ chain, i64 M, const i64* __restrict__ list, int n_list,
                                                           u32* __restrict__ counts, const u64* __restrict__ offs, i64* __restrict__ rows_out)
{
    __shared__ u32 s_buf[2 * kSelectNT], s_pos[kSelectNT];
    const i64 i = (i64)blockIdx.x * kSelectNT + threadIdx.x;
    u32 hit = 0;
    if (i < M) {
        const i64 v = chain[i];
        for (int k = 0; k < n_list; ++k) hit |= list[k] == v ? 1u : 0u;
    }
    pqw::block_scan<false>(hit, s_buf, s_pos, [](u32 x, u32 y) { return x + y; });
    if (!EMIT) { if (threadIdx.x == kSelectNT - 1) counts[blockIdx.x] = s_pos[kSelectNT - 1]; }
    else if (hit) rows_out[offs[blockIdx.x] + s_pos[threadIdx.x] - 1] = i;
}
static_assert(kSelectNT == pqw::kNT, "pqw::block_scan is written for this many threads");

// ---- host ---------------------------------------------------------------------------------------------------------
// The header line.  QUOTED: every name in double quotes, an inner quote doubled (what pyarrow writes by default).
inline void put_header(const std::vector<std::string>& names, int mode, std::vector<unsigned char>& out)
{
    if (mode == HEADER_NONE) return;
    for (size_t c = 0; c < names.size(); ++c) {
        if (c) out.push_back(',');
        if (mode == HEADER_QUOTED) out.push_back('"');
        for (const char ch : names[c]) { if (mode == HEADER_QUOTED && ch == '"') out.push_back('"'); out.push_back((unsigned char)ch); }
        if (mode == HEADER_QUOTED) out.push_back('"');
    }
    out.push_back('\n');
}

// The scalar restatement of k_csvw_format over all tiles: appends the text to `out`.  bad_pos / bad_field as the
// kernel's error words.
inline void format_host(const ColDev* cols, const Tiling& g, i64 count, const i64* rows, i64 src_rows, std::vector<unsigned char>& out,
                        unsigned long long* err)
{
    const i64 nt = tile_count(g, count);
    unsigned char buf[kFieldMax];
    for (i64 t = 0; t < nt; ++t) {
        const Tile tl = tile_at(g, count, t);
        for (int r = 0; r < tl.nr; ++r)
            for (int c = 0; c < tl.nc; ++c) {
                const i64 pos = tl.row0 + r;
                i64 row = rows ? rows[pos] : pos;
                if (row < 0 || row >= src_rows) { err[0] = std::min(err[0], (unsigned long long)pos); row = -1; }
                Dec d{0, 0, 1, KIND_INT};
                if (row >= 0 && !field_dec(cols[tl.col0 + c], row, kPow10, &d))
                    err[1] = std::min(err[1], (unsigned long long)pos * (unsigned long long)g.n_cols + (unsigned long long)(tl.col0 + c));
                const u32 len = dec_len(d);
                dec_put(d, buf);
                buf[len] = tl.col0 + c == g.n_cols - 1 ? '\n' : ',';
                out.insert(out.end(), buf, buf + len + 1);
            }
    }
}

}  // namespace csvw
}  // namespace mcr
