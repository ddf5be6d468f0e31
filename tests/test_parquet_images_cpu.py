"""Hand-built Parquet images (pq_images.py, pq_image_cases.py) on the host: the builder is honest and the project's
footer / page-header parser agrees with it.  No GPU.

For every image that test_parquet_images_gpu.py decodes: `pq.read_table` returns exactly the values the builder
intended (bit patterns), `pa.Codec("snappy")` inflates every compressed page to the builder's bytes, and
`ParquetFile(img).pages()` is the page table the builder laid out.  pyarrow is the reference reader here as it is in
test_parquet_cpu.py (the reference's `pq.read_table`, src/mcmc_ref/store.py:79-95).

Of the three doubtful cases, pyarrow 25 reads two -- an INDEX page between data pages (dict_mixed: index_page_between)
and an RLE level run whose count exceeds the values left (levels: lv_rle_count_beyond_*) -- and refuses one, which is
therefore in neither test file: a bit-packed run of definition LEVELS cut short of the groups its header declares
("Number of decoded rep / def levels do not match num_values in page header").  The cut-short last run of dictionary
INDICES is read by pyarrow and stays (dict_widths: last_group_*_used_cut)."""
from __future__ import annotations

import io

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_image_cases as cases
from mcmc_ref_hip._ffi import McrError
from mcmc_ref_hip.parquet import ParquetFile
from pq_images import (DATA, DATA_V2, DICT, DOUBLE, NONE, PLAIN, SNAPPY, Chunk, Column, Page, build_file, copy_bytes,
                       hybrid, hybrid_values, lit_header, snappy, t_struct, unknown_fields, uvarint)

ARROW = {1: pa.int32(), 2: pa.int64(), 4: pa.float32(), 5: pa.float64()}


def check_image(img: bytes, table, cols):
    """The three gates of the module docstring for one image."""
    t = pq.read_table(io.BytesIO(img))
    assert t.column_names == [c.name for c in cols]
    for f, c in zip(t.schema, cols):
        assert f.type == ARROW[c.type] and f.nullable == c.optional, c.name
    for c in cols:
        col = t[c.name]
        assert col.null_count == 0, c.name
        got = col.to_numpy()
        assert got.dtype == c.values.dtype and got.tobytes() == c.values.tobytes(), (c.name, c.doc)
    with ParquetFile(img) as f:
        assert f.num_rows == len(cols[0].values)
        assert f.column_names == [c.name for c in cols] and f.column_types == [c.type for c in cols]
        assert f.pages() == table
    codec = pa.Codec("snappy")
    it = iter(table)
    for g in range(len(cols[0].chunks)):                                # the table is in file order: row group, then column
        for c in cols:
            ch = c.chunks[g]
            for pg in ch.pages:
                if pg.kind not in (DATA, DATA_V2, DICT):
                    continue
                row = next(it)
                assert row["kind"] == pg.kind and row["codec"] == ch.codec
                if pg.stream is not None:
                    assert ch.codec == SNAPPY
                    at = row["payload_offset"] + len(pg.def_levels)
                    stored = img[at:row["payload_offset"] + row["compressed_size"]]
                    assert stored == pg.stream
                    assert codec.decompress(stored, len(pg.body)).to_pybytes() == pg.body, (c.name, c.doc)
                else:
                    assert img[row["payload_offset"]:row["payload_offset"] + row["compressed_size"]] == pg.def_levels + pg.body
    assert next(it, None) is None


@pytest.mark.parametrize("name", ["snappy_small", "snappy_big", "dict_widths", "dict_runs", "dict_mixed", "two_row_groups", "levels",
                                  "host_wide_schema", "host_unknown_everywhere_long_ids"])
def test_gpu_images_are_what_the_builder_says(name):
    """Every image of the GPU test: confirmed against pyarrow and the host parser before it travels."""
    check_image(*cases.gpu_files()[name])


def test_every_case_names_its_target():
    """Each column's doc names the constant or branch it aims at, and the names are unique within a file."""
    for name, (_img, _tab, cols) in cases.gpu_files().items():
        assert len({c.name for c in cols}) == len(cols), name
        if not name.startswith(("host_", "two_row")):
            assert all(len(c.doc) > 20 for c in cols), name


def test_case_lists_hold_what_the_kernels_constants_ask_for():
    """The catalogue against the kernel constants it was derived from (BATCH, REACH, RING, FLUSH): a changed constant
    shows here which names must move."""
    from pq_images import FLUSH, REACH, RING
    small = {c.name for c in cases.snappy_small()[2]}
    big = {c.name for c in cases.snappy_big()[2]}
    for L in (1, 59, 60, 61, 62, 63, 64, 65, 255, 256, 257):
        assert f"lit{L}" in small
    for L in (65535, 65536, 65537):
        assert f"lit{L}" in big
    for off in (REACH - 1, REACH, REACH + 1, RING - 1, RING, RING + 1, 65535):
        assert {f"far_off{off}_tag2", f"far_off{off}_tag3"} <= big
    assert {"far_off65536_tag3", "far_off100000_tag3"} <= big and "far_off65536_tag2" not in big
    assert (REACH, RING, FLUSH) == (28608, 32768, 8192)
    for off in (1, 2, 3, 4, 7, 8, 63, 64, 65):
        assert {f"copy_off{off}_tag{t}" for t in (1, 2, 3)} <= small
    for r in range(16):
        assert {f"lone{L}_op{r}" for L in (60, 64, 65, 200)} <= small
        assert {f"window_edge_pad{r}", f"window_mixed_pad{r}"} <= big
    for s in range(59, 64):
        assert {f"straddle_{k}_at{s}" for k in ("lit1", "lit2", "lit3", "lit4", "lit5", "copy1", "copy2", "copy3")} <= small
    widths = {c.name for c in cases.dict_widths()}
    assert {f"bw{bw}_dict{dn}" for bw in range(33) for dn in (1, 2, 3, 300)} <= widths
    assert {f"full_dict_w{w}" for w in range(13)} <= widths and {f"last_group_{u}_used" for u in range(1, 8)} <= widths
    # the output sizes of the FLUSH cases are what their names say
    sizes = {c.name: len(c.chunks[0].pages[0].body) for c in cases.snappy_small()[2] if c.name.startswith("out")}
    assert sizes == {"out8": 8, "out16": 16, "out8184": FLUSH - 8, "out8192": FLUSH, "out8200_copy": FLUSH + 8, "out8200_lit": FLUSH + 8,
                     "out8200_lone": FLUSH + 8}
    # streams longer than one input window really are
    for c in cases.snappy_big()[2]:
        if c.name.startswith("window_"):
            assert len(c.chunks[0].pages[0].stream) > 2 * 4096, c.name


def test_kernel_constants_the_cases_are_built_from():
    """The constants named in pq_images.py against the header they were read from: a change there must move the cases."""
    import re
    from pathlib import Path
    from pq_images import BATCH, DECODE_THREADS, FLUSH, IN_WIN, LOOKAHEAD, REACH, RING
    src = (Path(__file__).resolve().parents[1] / "mcmc-db_amd" / "csrc" / "mcr_parquet.hpp").read_text()
    assert re.search(r"constexpr int kRing = (\d+), kInWin = (\d+), kFlush = (\d+);", src).groups() == (str(RING), str(IN_WIN), str(FLUSH))
    assert "constexpr int kBatchOut = 64 * 64 + 64;" in src and REACH == RING - (BATCH * 64 + 64)
    assert f"(i64)ip + {LOOKAHEAD} > win + kInWin" in src
    assert f"__launch_bounds__({DECODE_THREADS}) void k_pq_decode" in src and f"__launch_bounds__({BATCH}) void k_pq_snappy" in src


def test_builder_primitives():
    """The Snappy, hybrid and Thrift writers byte by byte on examples small enough to check by hand."""
    assert lit_header(1) == b"\x00" and lit_header(60) == bytes([59 << 2]) and lit_header(61) == bytes([60 << 2, 60])
    assert lit_header(256) == bytes([60 << 2, 255]) and lit_header(257) == bytes([61 << 2, 0, 1])
    assert lit_header(65536) == bytes([61 << 2, 255, 255]) and lit_header(65537) == bytes([62 << 2, 0, 0, 1])
    assert lit_header(10, 2) == bytes([61 << 2, 9, 0]) and lit_header(70, 4) == bytes([63 << 2, 69, 0, 0, 0])
    assert copy_bytes(1, 0x234, 7) == bytes([1 | (3 << 2) | (2 << 5), 0x34])
    assert copy_bytes(2, 0x1234, 64) == bytes([2 | (63 << 2), 0x34, 0x12])
    assert copy_bytes(3, 100000, 1) == bytes([3]) + (100000).to_bytes(4, "little")
    stream, out = snappy([("lit", b"abc"), ("copy", 3, 3, 10), ("copy", 1, 13, 4), ("lit", b"xyzw!", 2)])
    assert out[:22] == b"abc" + b"abcabcabca" + b"abca" + b"xyzw!" and len(out) == 24
    assert stream[0] == 24 and pa.Codec("snappy").decompress(stream, 24).to_pybytes() == out
    runs = [("rle", 3, 5), ("packed", [0, 1, 2, 3, 4, 5, 6, 7]), ("rle", 8192, 1), ("packed", [7, 7, 7])]
    b = hybrid(runs, 3)
    assert b[:2] == bytes([6, 5]) and b[2] == 3 and b[3:6] == bytes([0b10001000, 0b11000110, 0b11111010])   # the format's own example
    assert b[6:10] == uvarint(16384) + b"\x01" and len(uvarint(16384)) == 3 and b[10:] == bytes([3, 0xFF, 0x01, 0])
    assert hybrid([("packed", [7, 7, 7], None, "cut")], 3) == bytes([3, 0xFF, 0x01])
    assert hybrid_values(runs, 8206) == [5] * 3 + [0, 1, 2, 3, 4, 5, 6, 7] + [1] * 8192 + [7, 7, 7]
    assert hybrid([("rle", 4, 0x01020304)], 32) == bytes([8, 4, 3, 2, 1]) and hybrid([("rle", 4, 0)], 0) == bytes([8])
    assert t_struct([(1, "i32", 1), (3, "bool", True), (4, "bool", False)]) == bytes([0x15, 2, 0x21, 0x12, 0])
    assert t_struct([(1, "i32", 1)], long_ids=True) == bytes([0x05, 2, 2, 0])
    assert t_struct([(100, "i32", -1), (2, "binary", b"ab")]) == bytes([0x05, 200, 1, 1, 0x08, 4, 2, 97, 98, 0])
    assert t_struct([(1, "list", ("bool", [True, False]))]) == bytes([0x19, 0x21, 1, 2, 0])
    assert t_struct([(1, "map", ("i32", "bool", [(1, True)]))]) == bytes([0x1B, 1, 0x51, 2, 1, 0])
    assert len({f[1] for f in unknown_fields()}) == 11                 # every Thrift type the compact protocol has


@pytest.mark.parametrize("name", sorted(cases.host_images()))
def test_thrift_shapes_the_writers_here_never_produce(name):
    """Long-form field ids throughout, one unknown field of every Thrift type (maps, sets, nested lists, bools in
    containers, a list of 16 structs) in each of FileMetaData, SchemaElement, RowGroup, ColumnChunk, ColumnMetaData,
    PageHeader, DataPageHeader, DataPageHeaderV2, DictionaryPageHeader and Statistics, a schema of 20 columns (long
    list header), page headers with crc and statistics: Thrift::field / skip / list_header."""
    img, table, cols = cases.host_images()[name]
    check_image(img, table, cols)
    kinds = {p["kind"] for p in table}
    assert kinds == {DATA, DATA_V2, DICT}                              # every page-header struct is in every image


def test_dictionary_page_found_without_its_offset():
    """ColumnMetaData without dictionary_page_offset whose data_page_offset is the dictionary page, and
    dictionary_page_offset = 0: `m.dict_off > 0 && m.dict_off < m.data_off` must fall back to data_page_offset."""
    img, table, cols = cases.dict_mixed_file()
    md = pq.ParquetFile(io.BytesIO(img)).metadata
    by_name = {c.name: k for k, c in enumerate(cols)}
    for name, want in (("no_dict_offset_2", None), ("zero_dict_offset_5", 0)):
        k = by_name[name]
        cm = md.row_group(0).column(k)
        assert (cm.dictionary_page_offset or 0) == (want or 0) and not (want is None and cm.has_dictionary_page)
        mine = [p for p in table if p["column"] == k]
        assert mine[0]["kind"] == DICT and all(p["dictionary_page"] == table.index(mine[0]) for p in mine[1:])
        assert cm.data_page_offset < mine[0]["payload_offset"]         # it points at the dictionary page's header


def test_null_images_hold_one_null_where_the_builder_put_it():
    for name, img, at in cases.null_images():
        col = pq.read_table(io.BytesIO(img))["x"]
        assert col.null_count == 1 and not col[at].is_valid and len(col) == cases.NULL_ROWS, name
        ParquetFile(img).close()                                       # the host does not look at level bytes


def test_refusal_images_pass_the_host_and_fail_pyarrow():
    """The device refusals' images are sound up to the damaged element: open() takes them (the damage is in page
    payloads, which the host never decodes) and pyarrow refuses every one."""
    for name, img, _msg, guard in cases.refusal_images():
        assert "k_pq_" in guard, name
        ParquetFile(img).close()
        with pytest.raises(Exception):
            pq.read_table(io.BytesIO(img))


def test_bit_packed_definition_levels_are_refused_by_name():
    """A v1 page of an OPTIONAL column with the deprecated BIT_PACKED definition levels has no 4-byte length in front of
    its levels; decoded as RLE it would misread them.  pyarrow reads the page; open() refuses it and names the encoding.
    The same header on a REQUIRED column (no level bytes at all) stays readable."""
    img, vals = cases.bit_packed_levels_image()
    assert pq.read_table(io.BytesIO(img))["x"].to_numpy().tobytes() == vals.tobytes()
    with pytest.raises(McrError, match="BIT_PACKED"):
        ParquetFile(img)
    pg = Page(DATA, len(vals), PLAIN, vals.tobytes(), def_encoding=4)
    img2, table = build_file([Column("x", DOUBLE, False, [Chunk(NONE, [pg])], vals)])
    assert pq.read_table(io.BytesIO(img2))["x"].to_numpy().tobytes() == vals.tobytes()
    with ParquetFile(img2) as f:
        assert f.pages() == table
    pg = Page(DATA, len(vals), PLAIN, b"\xFF\xFF\xFF" + vals.tobytes(), def_encoding=9)
    with pytest.raises(McrError, match="encoding 9"):
        ParquetFile(build_file([Column("x", DOUBLE, True, [Chunk(NONE, [pg])], vals)])[0])
