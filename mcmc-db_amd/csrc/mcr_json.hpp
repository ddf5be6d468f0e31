// mcr_json.hpp -- chain-list JSON text, [ {param: [draws...], ...}, ... ], -> draw tensor (replaces the
// json.loads + np.asarray of the JSON-zip reader, src/mcmc_ref/convert.py:78-102, on the way into the statistics).
//
//   json_token      one array element -> binary64 bits: csv::strict_number (the strict number grammar, then Eisel-Lemire:
//                   correctly rounded or HARD) with JSON's whitespace, NaN / Infinity and unsigned integer zero.  __host__ __device__: the CPU tests run the kernels' text.
//   k_json_index    structural index: every workgroup scans kChunk bytes for [ ] { } : , outside strings.  The count
//                   pass counts under both quote states at the chunk's start; k_json_scan picks the true one from the
//                   chunks' quote parities and forms the prefix sums; the write pass stores tok[] (every token's
//                   offset) and the skeleton (the non-comma tokens: their index in tok[] and their offset).
//   k_json_parse    one thread per array element between tok[a + v] and tok[a + v + 1].
//   walk            host: the document's skeleton against the text -- chains, keys, arrays and their lengths.
#pragma once

#include "mcr_csv.hpp"

namespace mcr { namespace json {

using csv::u32;
using csv::u64;

constexpr int kChunk = csv::kChunk;    // bytes of text per k_json_index workgroup (MCR_JSON_CHUNK)
constexpr int kIndexNT = 256;          // x 64 bytes per thread
constexpr int kParseNT = 256;          // array elements per k_json_parse workgroup (MCR_JSON_PARSE_BLOCK)
static_assert(kIndexNT * 64 == kChunk, "structural index geometry");

constexpr u32 kNoOffset = 0xFFFFFFFFu;
__host__ __device__ inline bool json_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

__host__ __device__ inline bool token_is(const char* p, size_t n, const char* w, size_t m)
{
    if (n != m) return false;
    for (size_t j = 0; j < m; ++j) if (p[j] != w[j]) return false;
    return true;
}

// [ws] -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? [ws] -> float(json.loads(text)): csv::strict_number and its
// csv::kNum* codes, with what is JSON's own.  The whitespace around the token is trimmed; exactly NaN / Infinity /
// -Infinity are kNumHard too (the host finishes them); kNumNotNumber: json.loads would refuse it or give something
// else than a number; an integer literal has no negative zero.
__host__ __device__ inline int json_token(const char* p, size_t n, const u64* pow5, u64* bits, bool* is_int)
{
    size_t i = 0, e = n;
    while (i < e && json_ws(p[i])) ++i;
    while (e > i && json_ws(p[e - 1])) --e;
    const char* t = p + i;
    const size_t m = e - i;
    if (m && (t[0] == 'N' || t[0] == 'I' || (m > 1 && t[1] == 'I'))) {
        *is_int = false;
        return token_is(t, m, "NaN", 3) || token_is(t, m, "Infinity", 8) || token_is(t, m, "-Infinity", 9) ? csv::kNumHard : csv::kNumNotNumber;
    }
    const int rc = csv::strict_number(t, m, pow5, bits, is_int);
    if (*is_int && rc == csv::kNumDecided && *bits == 1ull << 63) *bits = 0;
    return rc;
}

// ---- device side ------------------------------------------------------------------------------------------------

struct ChunkCount { u32 quotes, even, odd; };   // tokens | skeleton tokens << 16, the chunk starting outside / inside a string

// The 64 bytes at pos0 (64-byte aligned; bytes at or past `len` do not count): bit j of *quote / *tok / *comma / *bsl is
// set when byte pos0 + j is a '"' / one of [ ] { } : , / a ',' / a backslash.
__host__ __device__ inline void classify64(const char* __restrict__ text, u32 pos0, u32 len, u64* quote, u64* tok, u64* comma, u64* bsl)
{
    u64 q = 0, s = 0, c = 0, b = 0;
    if (pos0 < len) {
        const uint4* src = reinterpret_cast<const uint4*>(text + pos0);     // the buffer is padded to whole chunks
        for (int v = 0; v < 4; ++v) {
            const uint4 x = src[v];
            const u32 wds[4] = {x.x, x.y, x.z, x.w};
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < 4; ++k) {
                    const u32 ch = (wds[j] >> (8 * k)) & 0xFF, up = ch | 0x20;    // '[' | 0x20 == '{', ']' | 0x20 == '}'
                    const int bit = v * 16 + j * 4 + k;
                    q |= (u64)(ch == '"') << bit;
                    c |= (u64)(ch == ',') << bit;
                    s |= (u64)(ch == ',' || ch == ':' || up == '{' || up == '}') << bit;
                    b |= (u64)(ch == '\\') << bit;
                }
        }
        const u32 left = len - pos0;
        if (left < 64) { const u64 valid = (1ull << left) - 1; q &= valid; s &= valid; c &= valid; b &= valid; }
    }
    *quote = q; *tok = s; *comma = c; *bsl = b;
}

// bit j = parity of bits 0 .. j of x: after an even number of quotes a byte lies outside a string
__host__ __device__ inline u64 prefix_xor(u64 x)
{
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
    return x;
}

// WRITE = false: counts[chunk] and *first_bsl = the offset of the document's first backslash.  WRITE = true: with the
// chunk's true starting state in_string[chunk] and the prefix sums packed in first[chunk] (tokens) / sfirst[chunk]
// (skeleton tokens), tok[] gets every token's offset and skel_idx[] / skel_off[] the non-comma tokens, in text order.
template <bool WRITE>
__global__ __launch_bounds__(kIndexNT) void k_json_index(const char* __restrict__ text, u32 len, ChunkCount* __restrict__ counts,
                                                         u32* __restrict__ first_bsl, const u32* __restrict__ in_string,
                                                         const u32* __restrict__ first, const u32* __restrict__ sfirst,
                                                         u32* __restrict__ tok, u32* __restrict__ skel_idx, u32* __restrict__ skel_off)
{
    __shared__ u32 sh[kIndexNT];
    const u32 k = blockIdx.x;
    const u32 pos0 = k * (u32)kChunk + threadIdx.x * 64u;
    u64 quote, st, comma, bsl;
    classify64(text, pos0, len, &quote, &st, &comma, &bsl);
    u32 total_q;
    const u32 q_before = csv::block_scan_excl<kIndexNT>((u32)__popcll(quote), sh, &total_q);
    u64 inside = prefix_xor(quote);                       // relative to a chunk that starts outside a string
    if (q_before & 1) inside = ~inside;
    if (!WRITE) {
        if (bsl) atomicMin(first_bsl, pos0 + (u32)__ffsll((long long)bsl) - 1);
        const u64 even = st & ~inside, odd = st & inside;
        u32 total_e, total_o;
        csv::block_scan_excl<kIndexNT>((u32)__popcll(even) | ((u32)__popcll(even & ~comma) << 16), sh, &total_e);
        csv::block_scan_excl<kIndexNT>((u32)__popcll(odd) | ((u32)__popcll(odd & ~comma) << 16), sh, &total_o);
        if (threadIdx.x == 0) counts[k] = ChunkCount{total_q, total_e, total_o};
    } else {
        if (in_string[k]) inside = ~inside;
        const u64 mine = st & ~inside;
        u32 total;
        const u32 before = csv::block_scan_excl<kIndexNT>((u32)__popcll(mine) | ((u32)__popcll(mine & ~comma) << 16), sh, &total);
        u32 at = first[k] + (before & 0xFFFF), sat = sfirst[k] + (before >> 16);
        for (u64 m = mine; m; m &= m - 1) {
            const u32 bit = (u32)__ffsll((long long)m) - 1;
            if (!((comma >> bit) & 1)) { skel_idx[sat] = at; skel_off[sat] = pos0 + bit; ++sat; }
            tok[at++] = pos0 + bit;
        }
    }
}

// in_string[k] = parity of the quotes in front of chunk k; first / sfirst = exclusive prefix sums (n_chunks + 1 entries)
// of the token and skeleton-token counts each chunk has under that state.  A chunk holds at most 2^14 tokens, so the
// packed halves of ChunkCount::even / odd cannot carry into each other.
__global__ __launch_bounds__(1024) void k_json_scan(const ChunkCount* __restrict__ counts, u32 n_chunks, u32* __restrict__ in_string,
                                                    u32* __restrict__ first, u32* __restrict__ sfirst)
{
    __shared__ u32 sh[1024];
    u32 carry_q = 0, carry_t = 0, carry_s = 0;
    for (u32 base = 0; base < n_chunks; base += 1024) {
        const u32 i = base + threadIdx.x;
        const ChunkCount c = i < n_chunks ? counts[i] : ChunkCount{0, 0, 0};
        u32 total;
        const u32 qb = carry_q + csv::block_scan_excl<1024>(c.quotes & 1, sh, &total);
        carry_q += total;
        const u32 pk = (qb & 1) ? c.odd : c.even;
        const u32 tb = csv::block_scan_excl<1024>(pk & 0xFFFF, sh, &total);
        const u32 t_total = total;
        const u32 sb = csv::block_scan_excl<1024>(pk >> 16, sh, &total);
        if (i < n_chunks) { in_string[i] = qb & 1; first[i] = carry_t + tb; sfirst[i] = carry_s + sb; }
        carry_t += t_total;
        carry_s += total;
    }
    if (threadIdx.x == 0) { in_string[n_chunks] = carry_q & 1; first[n_chunks] = carry_t; sfirst[n_chunks] = carry_s; }
}

// One non-empty array of the document: its '[' is token tok0, element v lies between tokens tok0 + v and tok0 + v + 1.
// Elements v < limit are stored at out[base + v * stride_n]; the others, and every element of an array with base < 0,
// are only checked against the grammar.  first = elements of the arrays in front of it.
struct ArrayDesc { u32 tok0, count, limit, first; long long base; };
struct HardToken { u32 array, v, off, len; };

struct ParseArgs {
    const char* text; const u32* tok; const ArrayDesc* arrays; u32 n_arrays; u32 n_values; const u64* pow5;
    double* out; long long stride_n;
    u32* not_int;                        // [n_arrays]: set when a stored element is not an integer literal
    HardToken* hard; u32 hard_cap; u32* hard_count;
    unsigned long long* err;             // smallest (offset << 4 | kind) of the tokens outside the certified subset
};
constexpr int kErrToken = 1, kErrBigInt = 2;

__global__ __launch_bounds__(kParseNT) void k_json_parse(const ParseArgs a)
{
    const u64 g64 = (u64)blockIdx.x * kParseNT + threadIdx.x;
    if (g64 >= a.n_values) return;
    const u32 g = (u32)g64;
    u32 lo = 0, hi = a.n_arrays;                          // the last array with first <= g (none is empty)
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (a.arrays[mid].first <= g) lo = mid; else hi = mid;
    }
    const ArrayDesc d = a.arrays[lo];
    const u32 v = g - d.first;
    const u32 s = a.tok[d.tok0 + v] + 1, e = a.tok[d.tok0 + v + 1];
    u64 bits = 0;
    bool is_int = false;
    const int rc = json_token(a.text + s, e - s, a.pow5, &bits, &is_int);
    if (rc == csv::kNumNotNumber) { atomicMin(a.err, ((unsigned long long)s << 4) | kErrToken); return; }
    if (d.base < 0 || v >= d.limit) return;
    if (rc == csv::kNumBigInt) { atomicMin(a.err, ((unsigned long long)s << 4) | kErrBigInt); return; }
    if (!is_int) a.not_int[lo] = 1;
    if (rc == csv::kNumDecided) {
        a.out[d.base + (long long)v * a.stride_n] = __longlong_as_double((long long)bits);
    } else {
        const u32 h = atomicAdd(a.hard_count, 1u);
        if (h < a.hard_cap) a.hard[h] = HardToken{lo, v, s, e - s};
    }
}

// ---- host side --------------------------------------------------------------------------------------------------

struct Array { u32 tok0, count; };      // token index of the '[', elements
struct Chain { std::vector<std::string> keys; std::vector<Array> arrays; };   // document order

// A token the device reported hard: the value json.loads gives it.
inline bool finish_token(const char* p, size_t n, double* out)
{
    size_t i = 0, e = n;
    while (i < e && json_ws(p[i])) ++i;
    while (e > i && json_ws(p[e - 1])) --e;
    if (token_is(p + i, e - i, "NaN", 3)) { *out = __builtin_nan(""); return true; }
    if (token_is(p + i, e - i, "Infinity", 8)) { *out = __builtin_inf(); return true; }
    if (token_is(p + i, e - i, "-Infinity", 9)) { *out = -__builtin_inf(); return true; }
    return csv::finish_field(p + i, e - i, out);
}

// Walks the skeleton (n_skel non-comma tokens: idx[] their index among all tokens, off[] their byte offset) against the
// text.  Returns "" and fills `chains`, or the first reason the document is outside the certified subset, with *where =
// its byte offset.  Between two skeleton tokens lie idx[j + 1] - idx[j] - 1 commas and otherwise only what this walk
// accepts, so every byte outside the arrays' elements is checked here.
inline const char* walk(const char* text, size_t len, const u32* idx, const u32* off, size_t n_skel, std::vector<Chain>& chains,
                        size_t* where)
{
    chains.clear();
    auto skip_ws = [&](size_t p, size_t e) { while (p < e && json_ws(text[p])) ++p; return p; };
    auto fail_at = [&](size_t p, const char* why) { *where = p; return why; };
    size_t j = 0;
    if (n_skel == 0 || text[off[0]] != '[' || skip_ws(0, off[0]) != off[0]) return fail_at(0, "the top level is not an array");
    // gap(j, commas): the text between skeleton tokens j and j + 1 is whitespace around exactly `commas` commas
    auto gap = [&](size_t a, u32 commas) {
        if (idx[a + 1] - idx[a] - 1 != commas) return false;
        size_t p = skip_ws(off[a] + 1, off[a + 1]);
        if (commas) { if (p >= off[a + 1] || text[p] != ',') return false; p = skip_ws(p + 1, off[a + 1]); }
        return p == off[a + 1];
    };
    if (n_skel < 2) return fail_at(off[0], "the top-level array is not closed");
    if (text[off[1]] == ']') return fail_at(off[0], gap(0, 0) ? "the top-level array is empty" : "the top-level array does not hold objects");
    j = 1;
    for (;;) {                                            // skeleton token j should open a chain
        if (text[off[j]] != '{' || !gap(j - 1, chains.empty() ? 0 : 1)) return fail_at(off[j], "the top-level array does not hold objects");
        chains.emplace_back();
        Chain& ch = chains.back();
        for (bool first_member = true;; first_member = false) {
            if (j + 1 >= n_skel) return fail_at(off[j], "an object is not closed");
            if (text[off[j + 1]] == '}') {
                if (!gap(j, 0)) return fail_at(off[j] + 1, "a member is not a key and a flat array");
                ++j;
                break;
            }
            // [ws , ] ws "key" ws :
            if (text[off[j + 1]] != ':' || idx[j + 1] - idx[j] - 1 != (first_member ? 0u : 1u))
                return fail_at(off[j] + 1, "a member is not a key and a flat array");
            const size_t colon = off[j + 1];
            size_t p = skip_ws(off[j] + 1, colon);
            if (!first_member) { if (p >= colon || text[p] != ',') return fail_at(p, "a member is not a key and a flat array"); p = skip_ws(p + 1, colon); }
            if (p >= colon || text[p] != '"') return fail_at(p, "a member is not a key and a flat array");
            const char* close = (const char*)memchr(text + p + 1, '"', colon - p - 1);
            if (!close || skip_ws((size_t)(close - text) + 1, colon) != colon) return fail_at(p, "a member is not a key and a flat array");
            std::string key(text + p + 1, (size_t)(close - text) - p - 1);
            for (const char c : key) if ((unsigned char)c < 0x20) return fail_at(p, "a key holds a control character");
            for (const std::string& k : ch.keys) if (k == key) return fail_at(p, "an object holds a key twice");
            // : ws [ elements ]
            if (j + 3 >= n_skel || text[off[j + 2]] != '[' || !gap(j + 1, 0) || text[off[j + 3]] != ']')
                return fail_at(colon + 1, "a member's value is not a flat array");
            const bool blank = skip_ws(off[j + 2] + 1, off[j + 3]) == off[j + 3];
            ch.keys.push_back(std::move(key));
            ch.arrays.push_back(Array{idx[j + 2], blank ? 0u : idx[j + 3] - idx[j + 2]});
            j += 3;
        }
        if (j + 1 >= n_skel) return fail_at(off[j], "the top-level array is not closed");
        if (text[off[j + 1]] == ']') {
            if (!gap(j, 0)) return fail_at(off[j] + 1, "the top-level array does not hold objects");
            ++j;
            break;
        }
        ++j;
    }
    if (j + 1 != n_skel || skip_ws(off[j] + 1, len) != len) return fail_at(off[j] + 1, "text follows the top-level array");
    return "";
}

}}  // namespace mcr::json
