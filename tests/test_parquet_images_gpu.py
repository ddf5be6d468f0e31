"""k_pq_snappy and k_pq_decode on hand-built Parquet images no writer here emits (pq_images.py, pq_image_cases.py):
`read_columns` equals pyarrow's reading of the same image in bits, for whole files and for column subsets.

pyarrow is the reference reader (the reference's `pq.read_table`, src/mcmc_ref/store.py:79-95);
test_parquet_images_cpu.py has confirmed every image against it and against the host parser.  One case is one column
and its `doc` names what it aims at; the kernel constants the cases are built from are pq_images.BATCH (64 input bytes
per step), IN_WIN (kInWin 4096) with LOOKAHEAD 136, RING (kRing 32768), REACH (kRing - kBatchOut = 28608), FLUSH
(8192) and DECODE_THREADS (256).  All comparisons are bit-exact.

Not here, as pyarrow refuses it: a bit-packed run of definition levels cut short of its declared groups (see the CPU
module).  "The last element ending at lane 0 of its batch" is read as the earliest end there is, lane 1 -- an element
is at least two bytes (snappy_small: last_ends_lane1)."""
from __future__ import annotations

import io

import numpy as np
import pyarrow.parquet as pq
import pytest

import pq_image_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip._ffi import Context
    c = Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def wide(col):
    """A pyarrow / builder column as read_columns returns it: integers as int64, floats as float64."""
    col = np.asarray(col)
    return col.astype(np.int64) if np.issubdtype(col.dtype, np.integer) else col.astype(np.float64)


def check(ctx, file, columns=None):
    """read_columns against pyarrow and against the builder's own values; a failure names every wrong case and its aim."""
    from mcmc_ref_hip.parquet import read_columns
    img, _table, cols = file
    by_name = {c.name: c for c in cols}
    names = list(columns) if columns is not None else [c.name for c in cols]
    got = read_columns(ctx, img, columns)
    assert list(got) == names
    t = pq.read_table(io.BytesIO(img), columns=names)
    wrong = []
    for n in names:
        exp = wide(t[n].to_numpy())
        assert got[n].dtype == exp.dtype and got[n].shape == exp.shape, n
        if not (np.array_equal(bits(got[n]), bits(exp)) and np.array_equal(bits(got[n]), bits(wide(by_name[n].values)))):
            first = int(np.flatnonzero(bits(got[n]) != bits(exp))[0])
            wrong.append(f"{n} (first wrong row {first}): {by_name[n].doc}")
    assert not wrong, f"{len(wrong)} of {len(names)} cases differ from pyarrow:\n" + "\n".join(wrong)
    return got


def subsets(cols):
    names = [c.name for c in cols]
    return [names[::7][::-1], list(dict.fromkeys(names[-3:] + names[:2])), [names[len(names) // 2]]]


def test_snappy_elements_batches_and_copies(ctx):
    """snappy_small: literal lengths and header forms, lone literals at every output residue, elements whose header
    straddles a BATCH, copies at offsets 1..65 x lengths 1..64 through every tag, independent (4a) and in-order (4b)
    copies against the batch's output position, outputs around FLUSH, the last element's lane."""
    file = cases.snappy_small()
    check(ctx, file)
    for sub in subsets(file[2]):
        check(ctx, file, sub)


def test_snappy_windows_long_literals_and_far_copies(ctx):
    """snappy_big: literals of 65 535 | 65 536 | 65 537 bytes, streams of several IN_WIN refills with the payload swept
    over all 16 alignments, and 64-byte copies at REACH - 1 | REACH | REACH + 1, RING - 1 | RING | RING + 1, 65 535,
    65 536 and 100 000 whose source spans a FLUSH mark."""
    file = cases.snappy_big()
    check(ctx, file)
    for sub in subsets(file[2]):
        check(ctx, file, sub)


def test_dictionary_bit_widths(ctx):
    """dict_widths: every bit width 0..32 over dictionaries of 1, 2, 3 and 300 entries, dictionaries of exactly 2^w
    entries, last groups with 1..7 values used, RLE values of 1..4 bytes, all four physical types -- into the natural
    outputs (i64 for the integer types, f64 for the others) and, for the integer columns, into f64 as well."""
    from mcmc_ref_hip import parquet
    from mcmc_ref_hip._ffi import MCR_PQ_F64, DeviceBuffer
    file = cases.dict_widths_file()
    check(ctx, file)
    for sub in subsets(file[2]):
        check(ctx, file, sub)
    img, _table, cols = file
    ints = [c for c in cols if c.values.dtype.kind == "i"]
    with parquet.ParquetFile(img, ctx) as f:
        M = f.num_rows
        buf = DeviceBuffer(ctx, len(ints) * M * 8)
        try:
            parquet.decode(ctx, [(f, f.index(c.name), MCR_PQ_F64, buf.ptr.value + j * M * 8) for j, c in enumerate(ints)])
            got = buf.download(np.float64, len(ints) * M).reshape(len(ints), M)
        finally:
            buf.free()
    t = pq.read_table(io.BytesIO(img), columns=[c.name for c in ints])
    for j, c in enumerate(ints):
        assert np.array_equal(bits(got[j]), bits(t[c.name].to_numpy().astype(np.float64))), (c.name, c.doc)


def test_dictionary_run_lengths(ctx):
    """dict_runs: bit-packed runs of 1, 2, 31, 32, 33 groups and RLE runs of 1, 2, 255, 256, 257, 8191, 8192 alternating
    (run headers of 1, 2 and 3 varint bytes, 248 | 256 | 264 values against DECODE_THREADS)."""
    file = cases.dict_runs_file()
    check(ctx, file)
    check(ctx, file, [file[2][3].name, file[2][0].name])


def test_dictionary_chunks_pages_and_offsets(ctx):
    """dict_mixed and two_row_groups: fallback to PLAIN pages, compressed and stored dictionary pages, PLAIN_DICTIONARY,
    chunks without dictionary_page_offset or with 0, an INDEX page between data pages, a dictionary per row group."""
    for file in (cases.dict_mixed_file(), cases.two_row_groups_file()):
        check(ctx, file)
        for sub in subsets(file[2]):
            check(ctx, file, sub)


def test_definition_levels_of_other_writers(ctx):
    """levels: several RLE runs, bit-packed all-ones groups and mixes on v1 and v2 pages with num_values % 8 == 3 (the zero
    padding must not read as a null), an RLE count beyond the values left, v2 pages with is_compressed false / absent /
    true under a Snappy chunk."""
    file = cases.levels_file()
    check(ctx, file)
    for sub in subsets(file[2]):
        check(ctx, file, sub)


def test_thrift_shapes_decode(ctx):
    """Long-form ids and unknown fields of every Thrift type in every struct, and a 20-column schema: the page table the
    host hands the kernels is still right."""
    for name in ("unknown_everywhere_long_ids", "wide_schema"):
        file = cases.host_images()[name]
        check(ctx, file)
        check(ctx, file, [file[2][-1].name, file[2][0].name])


def test_a_null_at_each_position_of_a_partial_group_is_refused(ctx):
    """One real null in the last bit-packed level group (7 of 8 used), at each of its positions, v1 and v2: the existing
    "null values" refusal through `m = (1 << (cnt - g * 8)) - 1`."""
    from mcmc_ref_hip._ffi import McrError
    from mcmc_ref_hip.parquet import read_columns
    for name, img, _at in cases.null_images():
        with pytest.raises(McrError, match="null values"):
            read_columns(ctx, img)
    check(ctx, cases.two_row_groups_file())


def test_device_refusals_leave_the_context_sound(ctx):
    """Damaged elements the kernels reject by an explicit comparison before any load or store depends on the bad value
    (pq_image_cases.refusal_images cites the guard beside each): the existing message, and the next good call returns
    the bits of a fresh context."""
    from mcmc_ref_hip._ffi import Context, McrError
    from mcmc_ref_hip.parquet import read_columns
    good = cases.dict_mixed_file()
    with Context(0) as fresh_ctx:
        fresh = read_columns(fresh_ctx, good[0])
    for name, img, message, _guard in cases.refusal_images():
        with pytest.raises(McrError, match=message):
            read_columns(ctx, img)
        got = read_columns(ctx, good[0])
        assert list(got) == list(fresh), name
        for n in fresh:
            assert got[n].dtype == fresh[n].dtype and np.array_equal(bits(got[n]), bits(fresh[n])), (name, n)
    check(ctx, good)
