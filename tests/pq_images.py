"""A byte-level Parquet image builder for the reader's tests (test_parquet_images_cpu.py / _gpu.py): files no writer
here emits, composed element by element -- Thrift compact structs, Snappy streams from an explicit token plan, RLE /
bit-packed hybrid runs from an explicit run plan, pages and column chunks laid out by hand.

Plain Python and numpy; nothing is imported from the project or from pyarrow.  The builder computes what every page
must decode to with executors of its own (`snappy`, `hybrid_values`), so an image comes with its expected values and
with the page table the project's host parser has to report; pyarrow confirms both in the CPU test before an image
is decoded on a GPU.

The constants of k_pq_snappy / k_pq_decode that the case catalogues below aim at are named here once (BATCH, IN_WIN,
LOOKAHEAD, RING, REACH, FLUSH, DECODE_THREADS); a change to the kernel's shows which cases must move."""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

from pqwrite_cases import level_block, uvarint

# ---- format constants (parquet.thrift) -----------------------------------------------------------------------------
INT32, INT64, FLOAT, DOUBLE = 1, 2, 4, 5
NP = {INT32: np.dtype("<i4"), INT64: np.dtype("<i8"), FLOAT: np.dtype("<f4"), DOUBLE: np.dtype("<f8")}
PLAIN, PLAIN_DICT, RLE, BIT_PACKED, RLE_DICT = 0, 2, 3, 4, 8
NONE, SNAPPY = 0, 1
DATA, INDEX, DICT, DATA_V2 = 0, 1, 2, 3

# ---- the kernels' constants (mcr_parquet.hpp) ------------------------------------------------------------------------
BATCH = 64                 # input bytes one k_pq_snappy step looks at (one per lane)
IN_WIN = 4096              # kInWin: the LDS input window
LOOKAHEAD = 136            # the window is refilled when ip + 136 > win + kInWin
RING = 32768               # kRing: the LDS output ring
BATCH_OUT = 64 * 64 + 64   # kBatchOut
REACH = RING - BATCH_OUT   # 28608: the farthest copy offset served from the ring
FLUSH = 8192               # kFlush: ring -> global in pieces of this size
DECODE_THREADS = 256       # k_pq_decode's workgroup


def rnd(n: int, seed: int) -> bytes:
    """n incompressible bytes: every output byte of a Snappy case is a visible bit."""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- Thrift compact protocol writer ----------------------------------------------------------------------------------
# A struct is a list of (id, type, value).  Types: "bool" "i8" "i16" "i32" "i64" "double" "binary" "list" "set" "map"
# "struct".  list / set value: (element type, [values]); map value: (key type, value type, [(k, v)]); struct value: a
# field list.  Fields are written in list order; a field whose id is not 1..15 above the previous one takes the long
# form (delta 0 + zigzag id), and `long_ids` forces the long form everywhere.
TT = {"bool": 1, "i8": 3, "i16": 4, "i32": 5, "i64": 6, "double": 7, "binary": 8, "list": 9, "set": 10, "map": 11, "struct": 12}


def zigzag(v: int) -> bytes:
    return uvarint((v << 1) ^ (v >> 63) if v < 0 else v << 1)


def t_value(type_: str, v, long_ids: bool, in_container: bool = False) -> bytes:
    if type_ == "bool":
        return bytes([1 if v else 2]) if in_container else b""
    if type_ == "i8":
        return struct.pack("<b", v)
    if type_ in ("i16", "i32", "i64"):
        return zigzag(int(v))
    if type_ == "double":
        return struct.pack("<d", v)
    if type_ == "binary":
        v = v.encode() if isinstance(v, str) else bytes(v)
        return uvarint(len(v)) + v
    if type_ in ("list", "set"):
        et, items = v
        head = bytes([(len(items) << 4) | TT[et]]) if len(items) < 15 else bytes([0xF0 | TT[et]]) + uvarint(len(items))
        return head + b"".join(t_value(et, x, long_ids, True) for x in items)
    if type_ == "map":
        kt, vt, items = v
        if not items:
            return b"\x00"
        return uvarint(len(items)) + bytes([(TT[kt] << 4) | TT[vt]]) + b"".join(
            t_value(kt, k, long_ids, True) + t_value(vt, x, long_ids, True) for k, x in items)
    if type_ == "struct":
        return t_struct(v, long_ids)
    raise ValueError(type_)


def t_struct(fields, long_ids: bool = False) -> bytes:
    out, last = bytearray(), 0
    for fid, type_, v in fields:
        code = (1 if v else 2) if type_ == "bool" else TT[type_]
        delta = fid - last
        if not long_ids and 0 < delta <= 15:
            out.append((delta << 4) | code)
        else:
            out.append(code)
            out += zigzag(fid)
        out += t_value(type_, v, long_ids)
        last = fid
    out.append(0)
    return bytes(out)


def unknown_fields(base: int = 100):
    """One unknown field of every Thrift type (containers of bools, of structs and of containers among them), at ids no
    Parquet struct uses: what Thrift::skip has to walk."""
    inner = [(1, "i32", -7), (2, "bool", True), (3, "binary", b"xyz"), (9, "list", ("i64", [1, -2, 3 << 40]))]
    return [
        (base + 0, "bool", True), (base + 1, "bool", False), (base + 2, "i8", -3), (base + 3, "i16", -300),
        (base + 4, "i32", 1 << 30), (base + 5, "i64", -(1 << 62)), (base + 6, "double", -0.5),
        (base + 7, "binary", b"\x00\xffunknown"), (base + 8, "binary", b""),
        (base + 9, "list", ("struct", [inner] * 16)),                        # 16 elements: the long list header
        (base + 10, "list", ("bool", [True, False, True])),                 # bools in a container are one byte each
        (base + 11, "list", ("list", [("i32", [1, 2]), ("i32", []), ("bool", [False])])),
        (base + 12, "set", ("i32", [5, 6, 7])), (base + 13, "set", ("binary", [b"a", b""])),
        (base + 14, "map", ("binary", "struct", [(b"k1", inner), (b"k2", [])])),
        (base + 15, "map", ("bool", "bool", [(True, False), (False, True)])),
        (base + 16, "map", ("i32", "list", [(1, ("double", [1.5, 2.5]))])),
        (base + 17, "map", ("i32", "i32", [])),                              # an empty map is one zero byte
        (base + 18, "struct", [(1, "struct", [(15, "struct", inner)]), (200, "bool", False)]),
        (base + 300, "i32", 0),                                              # a two-byte zigzag id
    ]


STRUCTS = ("FileMetaData", "SchemaElement", "RowGroup", "ColumnChunk", "ColumnMetaData", "PageHeader", "DataPageHeader",
           "DataPageHeaderV2", "DictionaryPageHeader", "Statistics")


@dataclass
class Opts:
    """How the Thrift structs of one file are written.  `extras` maps a struct name to unknown fields injected behind
    its first own field (so the next own field's header has to come back from the unknown id)."""
    long_ids: bool = False
    extras: dict = field(default_factory=dict)

    def struct(self, name: str, fields) -> bytes:
        fields = [f for f in fields if f is not None]
        extra = self.extras.get(name, [])
        return t_struct(fields[:1] + list(extra) + fields[1:], self.long_ids)

    def fields(self, name: str, fields):
        """The field list (for a struct nested as a value) with the extras in place."""
        fields = [f for f in fields if f is not None]
        return fields[:1] + list(self.extras.get(name, [])) + fields[1:]


# ---- Snappy from a token plan ----------------------------------------------------------------------------------------
def lit_header(n: int, nb=None) -> bytes:
    """Tag of an n-byte literal; nb = None takes the minimal form, nb = 0 the inline length, 1..4 that many extra bytes."""
    assert n >= 1
    if nb is None:
        nb = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
    if nb == 0:
        assert n <= 60
        return bytes([(n - 1) << 2])
    assert n - 1 < 1 << (8 * nb)
    return bytes([(59 + nb) << 2]) + (n - 1).to_bytes(nb, "little")


def copy_bytes(tag: int, off: int, n: int) -> bytes:
    if tag == 1:
        assert 4 <= n <= 11 and 0 <= off < 2048
        return bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    assert 1 <= n <= 64
    if tag == 2:
        assert 0 <= off < 65536
        return bytes([2 | ((n - 1) << 2)]) + off.to_bytes(2, "little")
    assert tag == 3 and 0 <= off < 1 << 32
    return bytes([3 | ((n - 1) << 2)]) + off.to_bytes(4, "little")


def tags_for(off: int, n: int):
    """The copy tags that can express (offset, length)."""
    return [t for t in (1, 2, 3) if (t != 1 or (4 <= n <= 11 and off < 2048)) and (t != 2 or off < 65536)]


def snappy(tokens, pad_seed: int = 0, preamble=None, check: bool = True):
    """(stream, output) of a token plan: ("lit", bytes[, nb]) | ("copy", tag, offset, length), emitted exactly as given.
    The output is padded to a multiple of 8 with one final literal.  `preamble` overrides the length varint and
    `check = False` lets a plan be wrong on purpose (the refusal cases); the output then stops at the bad element."""
    out, body = bytearray(), bytearray()
    tokens = list(tokens)
    ok = True
    for k, tok in enumerate(tokens):
        if tok[0] == "lit":
            data, nb = tok[1], (tok[2] if len(tok) > 2 else None)
            body += lit_header(len(data), nb) + data
            out += data
        elif tok[0] == "raw":                      # bytes put into the stream as they are (damaged elements)
            body += tok[1]
            ok = False
        else:
            _c, tag, off, n = tok
            body += copy_bytes(tag, off, n)
            if ok and 1 <= off <= len(out):
                if off >= n:
                    out += out[len(out) - off:len(out) - off + n]
                else:
                    for _ in range(n):
                        out.append(out[-off])
            else:
                assert not check, (k, tok, len(out))
                ok = False
    if ok and len(out) % 8:
        data = rnd(8 - len(out) % 8, 7000 + pad_seed)
        body += lit_header(len(data)) + data
        out += data
    pre = uvarint(len(out)) if preamble is None else preamble
    return bytes(pre) + bytes(body), bytes(out)


def filler(n_values: int, type_: int, seed: int):
    """(values, plan): a page of a constant, as one literal and overlapping copies -- brings a column to its file's rows."""
    es = NP[type_].itemsize
    v = np.full(n_values, 1000 + seed % 97, dtype=NP[type_])
    data = v.tobytes()
    toks, left = [("lit", data[:es])], len(data) - es
    while left > 0:
        toks.append(("copy", 2, es, min(64, left)))
        left -= min(64, left)
    return v, toks


# ---- RLE / bit-packed hybrid from a run plan ---------------------------------------------------------------------------
def pack_bits(values, bw: int, n_bytes: int) -> bytes:
    acc = 0
    for k, v in enumerate(values):
        assert 0 <= v < (1 << bw) or (bw == 0 and v == 0), (v, bw)
        acc |= int(v) << (k * bw)
    return acc.to_bytes(max(n_bytes, (len(values) * bw + 7) // 8), "little")[:n_bytes]


def hybrid(runs, bw: int) -> bytes:
    """Bytes of a run plan at bit width bw (without the width byte): ("rle", count, value) |
    ("packed", values[, groups[, "cut"]]).  A packed run is padded with zeros to its groups; "cut" drops the padding
    bytes behind the last used value (legal for the last run of a page)."""
    out = bytearray()
    for run in runs:
        if run[0] == "rle":
            count, value = run[1], run[2]
            out += uvarint(count << 1) + int(value).to_bytes((bw + 7) // 8, "little")
        else:
            values = list(run[1])
            groups = run[2] if len(run) > 2 and run[2] is not None else (len(values) + 7) // 8
            assert len(values) <= groups * 8
            n_bytes = groups * bw
            if len(run) > 3 and run[3] == "cut":
                n_bytes = (len(values) * bw + 7) // 8
            out += uvarint((groups << 1) | 1) + pack_bits(values, bw, n_bytes)
    return bytes(out)


def hybrid_values(runs, n: int):
    """The first n values a run plan stands for (padding of a packed run counts where another run follows it)."""
    out = []
    for k, run in enumerate(runs):
        if run[0] == "rle":
            out += [run[2]] * run[1]
        else:
            values = list(run[1])
            groups = run[2] if len(run) > 2 and run[2] is not None else (len(values) + 7) // 8
            out += values + [0] * (groups * 8 - len(values))
    assert len(out) >= n, (len(out), n)
    return out[:n]


def levels_v1(runs) -> bytes:
    body = hybrid(runs, 1)
    return struct.pack("<I", len(body)) + body


# ---- pages, chunks, files --------------------------------------------------------------------------------------------
@dataclass
class Page:
    kind: int                      # DATA, DATA_V2, DICT or INDEX
    num_values: int
    encoding: int
    body: bytes                    # v1: levels + values; v2: values; dictionary: entries -- before compression
    stream: bytes | None = None    # the Snappy stream standing for `body` (None: the page is stored as it is)
    def_levels: bytes = b""        # v2 only: in front of the values, never compressed
    is_compressed: bool | None = None     # v2 field 7; None leaves it out (it defaults to true)
    def_encoding: int = RLE
    crc: bool = False
    stats: bool = False
    pad: int = 0                   # bytes of an unknown binary field in the page header: shifts where the payload lands
    uncompressed_size: int | None = None  # override of the header's figure (refusal cases)


@dataclass
class Chunk:
    codec: int
    pages: list
    dict_offset: str = "set"       # "set" | "absent" (data_page_offset points at the dictionary page) | "zero"


@dataclass
class Column:
    name: str
    type: int
    optional: bool
    chunks: list
    values: np.ndarray | None      # what the column must decode to (None: a refusal case)
    doc: str = ""


def page_bytes(pg: Page, codec: int, opts: Opts):
    """(header, payload) of one page."""
    stored = pg.stream if pg.stream is not None else pg.body
    payload = pg.def_levels + stored
    usize = len(pg.def_levels) + len(pg.body) if pg.uncompressed_size is None else pg.uncompressed_size
    st = opts.fields("Statistics", [(3, "i64", 0), (5, "binary", b"\x09" * 8), (6, "binary", b"\x01" * 8)]) if pg.stats else None
    if pg.kind == DATA:
        sub = (5, "struct", opts.fields("DataPageHeader", [
            (1, "i32", pg.num_values), (2, "i32", pg.encoding), (3, "i32", pg.def_encoding), (4, "i32", RLE),
            (5, "struct", st) if st else None]))
    elif pg.kind == DATA_V2:
        sub = (8, "struct", opts.fields("DataPageHeaderV2", [
            (1, "i32", pg.num_values), (2, "i32", 0), (3, "i32", pg.num_values), (4, "i32", pg.encoding),
            (5, "i32", len(pg.def_levels)), (6, "i32", 0),
            (7, "bool", pg.is_compressed) if pg.is_compressed is not None else None,
            (8, "struct", st) if st else None]))
    elif pg.kind == DICT:
        sub = (7, "struct", opts.fields("DictionaryPageHeader", [(1, "i32", pg.num_values), (2, "i32", pg.encoding), (3, "bool", False)]))
    else:
        sub = (6, "struct", [])                    # IndexPageHeader: empty
    crc = zlib.crc32(payload)
    hdr = opts.struct("PageHeader", [
        (1, "i32", pg.kind), (2, "i32", usize), (3, "i32", len(payload)),
        (4, "i32", crc - (1 << 32) if crc >= 1 << 31 else crc) if pg.crc else None,
        (90, "binary", b"\xAA" * pg.pad) if pg.pad else None, sub])
    return hdr, payload


def build_file(columns, opts: Opts | None = None, created_by: str = "pq_images (hand-built)"):
    """(image, page table): the file of `columns` (all with the same chunk row counts) and the rows ParquetFile.pages()
    must report for it, in its keys (INDEX pages are walked over, not listed)."""
    opts = opts or Opts()
    out = bytearray(b"PAR1")
    table = []
    n_rg = len(columns[0].chunks)
    assert all(len(c.chunks) == n_rg for c in columns)
    rgs, total_rows = [], 0
    first_row = [0] * len(columns)
    for g in range(n_rg):
        ccs, rg_rows, rg_bytes = [], None, 0
        for ci, col in enumerate(columns):
            ch = col.chunks[g]
            start = len(out)
            dict_at = data_at = None
            dict_idx, values, usum, encs = -1, 0, 0, []
            for pg in ch.pages:
                hdr, payload = page_bytes(pg, ch.codec, opts)
                at = len(out)
                out += hdr + payload
                usum += len(hdr) + len(pg.def_levels) + len(pg.body)
                if pg.kind == DICT and dict_at is None:
                    dict_at = at
                if pg.kind in (DATA, DATA_V2) and data_at is None:
                    data_at = at
                if pg.kind == INDEX:
                    continue
                if pg.kind == DICT:
                    dict_idx = len(table)
                encs.append(pg.encoding)
                table.append(dict(column=ci, kind=pg.kind, encoding=pg.encoding, codec=ch.codec, payload_offset=at + len(hdr),
                                  compressed_size=len(payload),
                                  uncompressed_size=len(pg.def_levels) + len(pg.body) if pg.uncompressed_size is None else pg.uncompressed_size,
                                  num_values=pg.num_values,
                                  first_row=first_row[ci] + values if pg.kind != DICT else 0,
                                  dictionary_page=dict_idx if pg.kind != DICT else -1))
                if pg.kind != DICT:
                    values += pg.num_values
            first_row[ci] += values
            assert rg_rows in (None, values), (col.name, values, rg_rows)
            rg_rows = values
            dict_field = (11, "i64", dict_at) if dict_at is not None else None
            if ch.dict_offset != "set":            # old writers: no dictionary_page_offset (or 0), data_page_offset at the first page
                data_at = dict_at if dict_at is not None else data_at
                dict_field = (11, "i64", 0) if ch.dict_offset == "zero" else None
            meta = opts.fields("ColumnMetaData", [
                (1, "i32", col.type), (2, "list", ("i32", sorted(set(encs + [RLE])))), (3, "list", ("binary", [col.name])),
                (4, "i32", ch.codec), (5, "i64", values), (6, "i64", usum), (7, "i64", len(out) - start),
                (9, "i64", data_at if data_at is not None else start),
                dict_field])
            ccs.append(opts.fields("ColumnChunk", [(2, "i64", start), (3, "struct", meta)]))
            rg_bytes += len(out) - start
        rgs.append(opts.fields("RowGroup", [(1, "list", ("struct", ccs)), (2, "i64", rg_bytes), (3, "i64", rg_rows)]))
        total_rows += rg_rows
    schema = [opts.fields("SchemaElement", [(4, "binary", "schema"), (5, "i32", len(columns))])]
    for col in columns:
        schema.append(opts.fields("SchemaElement", [(1, "i32", col.type), (3, "i32", 1 if col.optional else 0), (4, "binary", col.name)]))
    footer = opts.struct("FileMetaData", [
        (1, "i32", 1), (2, "list", ("struct", schema)), (3, "i64", total_rows), (4, "list", ("struct", rgs)), (6, "binary", created_by)])
    out += footer + struct.pack("<I", len(footer)) + b"PAR1"
    return bytes(out), table


# ---- column makers ---------------------------------------------------------------------------------------------------
def snappy_column(name: str, tokens, rows: int, doc: str, type_: int = INT64, pad: int = 0, v2: bool = False, seed: int = 0) -> Column:
    """A REQUIRED PLAIN Snappy column whose first page is the token plan (its output ARE the values) and whose second
    page, a constant, brings it to `rows`."""
    stream, body = snappy(tokens, pad_seed=seed)
    es = NP[type_].itemsize
    assert len(body) % es == 0 and len(body) // es <= rows, (name, len(body), rows)
    vals = np.frombuffer(body, dtype=NP[type_])
    kind = DATA_V2 if v2 else DATA
    pages = [Page(kind, len(vals), PLAIN, body, stream, pad=pad)]
    if len(vals) < rows:
        fv, ftoks = filler(rows - len(vals), type_, seed)
        fstream, fbody = snappy(ftoks)
        assert fbody == fv.tobytes()
        pages.append(Page(kind, len(fv), PLAIN, fbody, fstream))
        vals = np.concatenate([vals, fv])
    return Column(name, type_, False, [Chunk(SNAPPY, pages)], vals, doc)


def dict_entries(n: int, type_: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if type_ in (FLOAT, DOUBLE):
        v = rng.normal(size=n).astype(NP[type_])
        v[0] = -0.0
        return v
    info = np.iinfo(NP[type_])
    v = rng.integers(info.min, info.max, n, dtype=NP[type_], endpoint=True)
    v[0] = info.min
    return v


def dict_column(name: str, type_: int, entries: np.ndarray, page_runs, doc: str, codec: int = NONE, optional: bool = False,
                v2: bool = False, plain_tail: np.ndarray | None = None, enc: int = RLE_DICT,
                dict_offset: str = "set", seed: int = 0) -> Column:
    """A dictionary-encoded column: page_runs is [(bit width, run plan, values in the page)] per data page; plain_tail
    adds a PLAIN page behind them (the writer's fallback)."""
    dbody = entries.tobytes()
    comp = codec == SNAPPY
    pages = [Page(DICT, len(entries), PLAIN_DICT if enc == PLAIN_DICT else PLAIN, dbody,
                  raw_stream(dbody, seed) if comp else None)]
    vals = []
    for k, (bw, runs, n) in enumerate(page_runs):
        idx = hybrid_values(runs, n)
        vals.append(entries[np.asarray(idx, dtype=np.int64)])
        body = bytes([bw]) + hybrid(runs, bw)
        pages.append(data_page(body, n, enc, optional, comp, v2, seed + k))
    if plain_tail is not None:
        pages.append(data_page(plain_tail.astype(NP[type_]).tobytes(), len(plain_tail), PLAIN, optional, comp, v2, seed + 99))
        vals.append(plain_tail.astype(NP[type_]))
    return Column(name, type_, optional, [Chunk(codec, pages, dict_offset)], np.concatenate(vals), doc)


def raw_stream(data: bytes, seed: int = 0) -> bytes:
    """A Snappy stream for bytes that are not the subject of a case (levels, dictionaries, run bytes), of any length:
    literals of mixed sizes, and a copy wherever the next bytes repeat the ones 8 back."""
    rng = np.random.default_rng(seed)
    body, i = bytearray(), 0
    while i < len(data):
        n = min(int(rng.integers(1, 70)), len(data) - i)
        if i >= 8 and data[i:i + min(n, 64)] == data[i - 8:i - 8 + min(n, 64)]:
            n = min(n, 64)
            body += copy_bytes(2, 8, n)
        else:
            body += lit_header(n) + data[i:i + n]
        i += n
    return uvarint(len(data)) + bytes(body)


def data_page(values_body: bytes, n: int, enc: int, optional: bool, comp: bool, v2: bool, seed: int = 0, level_runs=None,
              is_compressed=None) -> Page:
    """A data page of an all-defined column: level_runs defaults to one RLE run."""
    runs = level_runs if level_runs is not None else [("rle", n, 1)]
    if v2:
        lv = hybrid(runs, 1) if optional else b""
        store = comp and is_compressed is not False
        return Page(DATA_V2, n, enc, values_body, raw_stream(values_body, seed) if store else None, def_levels=lv,
                    is_compressed=is_compressed)
    body = ((level_block(n) if level_runs is None else levels_v1(runs)) if optional else b"") + values_body
    return Page(DATA, n, enc, body, raw_stream(body, seed) if comp else None)
