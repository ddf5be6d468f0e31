"""Shared by test_parquet_write_cpu.py and test_parquet_write_gpu.py: the columns the Parquet writer is tried on, what a
written file must look like to pyarrow and to the project's own footer parser, and a plain Snappy token walker.

A column here is (name, physical type, numpy array of float64 / int64) or (name, type, ("seq", div, mod)); `write`
is a function (columns, rows, row_group_rows) -> bytes of the file: mcr_parquet_write_host or Context.write_parquet."""
from __future__ import annotations

import ctypes as C
import io
import struct

import numpy as np

INT32, INT64, DOUBLE = 1, 2, 5
PAGE_ROWS = 8192                       # MCR_PQW_PAGE_ROWS (asserted against the header by the CPU test)
INT64_MAX = (1 << 63) - 1
ES = {INT32: 4, INT64: 8, DOUBLE: 8}
NP = {INT32: np.int32, INT64: np.int64, DOUBLE: np.float64}


def expected_values(col, rows: int) -> np.ndarray:
    """The column as the file must hold it (the physical type's numpy array)."""
    _name, type_, src = col
    if isinstance(src, tuple):
        _seq, div, mod = src
        return ((np.arange(rows, dtype=np.int64) // div) % mod).astype(NP[type_])
    a = np.asarray(src)[:rows]
    return a.astype(NP[type_]) if type_ != DOUBLE else a


def uvarint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def level_block(n: int) -> bytes:
    """Definition levels of n defined values: 4-byte length, one RLE run (n << 1, value 1)."""
    body = uvarint(n << 1) + b"\x01"
    return struct.pack("<I", len(body)) + body


def snappy_walk(payload: bytes):
    """Decodes a raw Snappy stream token by token: (uncompressed bytes, [("lit", length) | ("copy", tag, offset, length)]).
    Asserts what the writer promises: tags 0, 1 and 2 only, copies of at most 64 bytes, 1 <= offset <= min(produced, 65535)."""
    pos, shift, ulen = 0, 0, 0
    while True:
        b = payload[pos]
        pos += 1
        ulen |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out, tokens = bytearray(), []
    while pos < len(payload):
        tag = payload[pos]
        kind = tag & 3
        if kind == 0:
            n = tag >> 2
            pos += 1
            if n >= 60:
                nb = n - 59
                n = int.from_bytes(payload[pos:pos + nb], "little")
                pos += nb
            n += 1
            assert pos + n <= len(payload), "literal runs past the stream"
            out += payload[pos:pos + n]
            pos += n
            tokens.append(("lit", n))
            continue
        assert kind in (1, 2), "a 4-byte-offset copy"
        if kind == 1:
            length, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | payload[pos + 1]
            pos += 2
        else:
            length, off = (tag >> 2) + 1, payload[pos + 1] | (payload[pos + 2] << 8)
            pos += 3
        assert 1 <= off <= min(len(out), 65535) and length <= 64, (off, length, len(out))
        for _ in range(length):
            out.append(out[-off])
        tokens.append(("copy", kind, off, length))
    assert len(out) == ulen, "preamble differs from the decoded length"
    return bytes(out), tokens


def copy_tokens(nbytes: int, off: int) -> list:
    """The pieces one run of equal distance is cut into: 64-byte copies, then the rest (tag 1 where it fits)."""
    out = [("copy", 2, off, 64)] * (nbytes // 64)
    rest = nbytes % 64
    if rest:
        out.append(("copy", 1 if rest <= 11 and off < 2048 else 2, off, rest))
    return out


def pages_of(lib, image: bytes):
    """[(column, payload bytes, uncompressed size, values, first row)] from the project's own footer / page-header parser."""
    buf = C.create_string_buffer(image, len(image))
    h = C.c_void_p()
    assert lib.mcr_parquet_open(None, buf, len(image), C.byref(h)) == 0, lib.mcr_last_error(None)
    try:
        out = []
        info = (C.c_int64 * 10)()
        for k in range(lib.mcr_parquet_num_pages(h)):
            assert lib.mcr_parquet_page_info(h, k, info) == 0
            col, kind, enc, codec, off, csz, usz, nv, row0, dic = list(info)
            assert (kind, enc, codec, dic) == (0, 0, 1, -1)            # data page v1, PLAIN, SNAPPY, no dictionary
            out.append((col, image[off:off + csz], usz, nv, row0))
        return out
    finally:
        lib.mcr_parquet_close(h)


def check_file(lib, image: bytes, cols, rows: int, row_group_rows: int = 0):
    """Everything a written file must satisfy; returns {column name: [token list per page]}."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    rg = row_group_rows or 1048576
    table = pq.read_table(io.BytesIO(image))
    want = [expected_values(c, rows) for c in cols]
    assert table.column_names == [c[0] for c in cols]
    for f, c in zip(table.schema, cols):
        assert f.nullable and f.type == {INT32: pa.int32(), INT64: pa.int64(), DOUBLE: pa.float64()}[c[1]], f
    for c, w in zip(cols, want):
        got = table[c[0]].to_numpy()
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), c[0]
    md = pq.ParquetFile(io.BytesIO(image)).metadata
    assert md.num_rows == rows and md.created_by.startswith("mcmc-ref-hip version ")
    assert [md.row_group(g).num_rows for g in range(md.num_row_groups)] == [min(rg, rows - r) for r in range(0, rows, rg)]
    for g in range(md.num_row_groups):
        for k, (c, w) in enumerate(zip(cols, want)):
            cc = md.row_group(g).column(k)
            part = w[g * rg:(g + 1) * rg]
            assert cc.compression == "SNAPPY" and tuple(cc.encodings) == ("PLAIN", "RLE") and cc.num_values == len(part)
            st = cc.statistics
            assert st is not None and st.null_count == 0
            if c[1] == DOUBLE and np.isnan(part).any():
                assert not st.has_min_max
                continue
            assert st.has_min_max and st.min == part.min() and st.max == part.max(), (c[0], st.min, st.max)
            if c[1] == DOUBLE:                                           # the zero rule: min -0.0, max +0.0
                assert st.min != 0 or np.signbit(st.min)
                assert st.max != 0 or not np.signbit(st.max)
    # the pages, from our own parser: geometry, and payloads that inflate to levels + PLAIN values
    codec = pa.Codec("snappy")
    tokens: dict = {c[0]: [] for c in cols}
    pages = pages_of(lib, image)
    assert len(pages) == sum(-(-min(rg, rows - r) // PAGE_ROWS) for r in range(0, rows, rg)) * len(cols)
    for col, payload, usz, nv, row0 in pages:
        c, w = cols[col], want[col]
        plain = level_block(nv) + w[row0:row0 + nv].tobytes()
        assert usz == len(plain)
        assert codec.decompress(payload, usz).to_pybytes() == plain, (c[0], row0)
        mine, toks = snappy_walk(payload)
        assert mine == plain
        tokens[c[0]].append(toks)
    return tokens


def distinct(n: int, type_: int, seed: int = 0) -> np.ndarray:
    """n distinct values of the type's source array (int64 for the integer types)."""
    rng = np.random.default_rng(seed)
    if type_ == DOUBLE:
        return rng.normal(size=n)
    return (rng.permutation(n).astype(np.int64) * 7919 + 11) % (2 ** 31 - 1)


def token_edge_cases():
    """[(id, column, rows, expected tokens of the page(s))]: one column each.

    Literal lengths are a multiple of the element size, plus the level block in a page's first literal, so the tag
    boundaries (1 / 2 / 3 / 4 tag bytes at lengths 60|61, 256|257, 65536|65537) are met from both sides with the nearest
    lengths there are: exactly 60 and 256 and the next length up in a second literal (behind one repeated element),
    65535 and 65544 in a first literal.  Copy offsets are multiples of the element size too: 2040 | 2048 | 2056 (INT64) and
    2044 | 2048 | 2052 (INT32) around the switch from tag 1 to tag 2."""
    cases = []
    lvl = lambda n: len(level_block(n))      # noqa: E731
    # first literal of a page: the level block + n distinct values
    for type_, n in ((INT32, 13), (INT32, 14), (INT64, 6), (INT64, 7), (INT32, 62), (INT32, 63), (DOUBLE, 31), (DOUBLE, 32),
                     (INT64, 8191), (DOUBLE, 8192), (INT32, 8192)):
        cases.append((f"first-literal-{type_}-{n}", ("v", type_, distinct(n, type_, n)), n, [[("lit", lvl(n) + n * ES[type_])]]))
    # second literal: [a, a, k distinct] -> lit(level block + a), copy(a), lit(k values)
    for type_, k in ((INT32, 14), (INT32, 15), (INT32, 16), (INT64, 7), (INT64, 8), (INT32, 63), (INT32, 64), (INT32, 65),
                     (INT64, 32), (DOUBLE, 33), (INT64, 8190)):
        es, n = ES[type_], k + 2
        body = distinct(k + 1, type_, 100 + k)
        a = np.concatenate([body[:1], body])
        cases.append((f"second-literal-{type_}-{k}", ("v", type_, a), n,
                      [[("lit", lvl(n) + es), ("copy", 1, es, es), ("lit", k * es)]]))
    # constant runs: one literal element, then one overlapping copy at offset = element size, cut at 64 bytes
    for type_ in (INT64, INT32):
        for n in (7, 8, 9, 64, 65, 1000):
            es = ES[type_]
            cases.append((f"constant-{type_}-{n}", ("v", type_, np.full(n, 42, dtype=np.int64)), n,
                          [[("lit", lvl(n) + es)] + copy_tokens((n - 1) * es, es)]))
    # x, c ... c, x: the second x is one element copied from `dist` elements back
    for type_, dists in ((INT64, (255, 256, 257, 8191)), (INT32, (511, 512, 513, 8191))):
        for dist in dists:
            es, n = ES[type_], dist + 1
            a = np.full(n, 5, dtype=np.int64)
            a[0] = a[-1] = 123456789
            off = dist * es
            cases.append((f"repeat-{type_}-{off}", ("v", type_, a), n,
                          [[("lit", lvl(n) + 2 * es)] + copy_tokens((dist - 2) * es, es) + copy_tokens(es, off)]))
    # the same value one page apart (65536 bytes for 8-byte elements): never a match, pages stand alone
    for type_ in (INT64, DOUBLE):
        n = PAGE_ROWS + 1
        a = distinct(n, type_, 7)
        a[-1] = a[0]
        cases.append((f"repeat-{type_}-next-page", ("v", type_, a), n, [[("lit", lvl(PAGE_ROWS) + PAGE_ROWS * 8)], [("lit", lvl(1) + 8)]]))
    return cases


def special_doubles() -> np.ndarray:
    """-0.0, denormals, the extremes, infinities and NaNs with payloads."""
    bits = np.array([0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF,
                     0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001,
                     0x7FF0000000000123, 0x3FF0000000000000], dtype=np.uint64)
    return bits.view(np.float64)
