"""The Parquet writer's file format, without a GPU: mcr_parquet_write_host shares headers, footer, levels, statistics
and the Snappy token emission with the device writer (its match finder is the scalar restatement).  Every file is
read back by pyarrow, its pages are found with the project's own footer parser, inflated with pyarrow's Snappy and
walked token by token (tests/pqwrite_cases.py)."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import pqwrite_cases as W
from pqwrite_cases import DOUBLE, INT32, INT64

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def ffi():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mcr_build", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from mcmc_ref_hip import _ffi
    return _ffi


def host_columns(ffi, cols):
    return [ffi.pq_sequence(n, t, s[1], s[2]) if isinstance(s, tuple) else ffi.pq_column(n, t, s) for n, t, s in cols]


def write_host(ffi, cols, rows, row_group_rows=0) -> bytes:
    with ffi.write_parquet_host(host_columns(ffi, cols), rows, row_group_rows) as image:
        assert image.pages >= len(cols)
        return image.tobytes()


def test_geometry_constants_match_the_header(ffi):
    header = (ROOT / "include" / "mcmcref_hip.h").read_text()
    assert int(re.search(r"#define MCR_PQW_PAGE_ROWS (\d+)", header).group(1)) == W.PAGE_ROWS == ffi.MCR_PQW_PAGE_ROWS
    assert int(re.search(r"#define MCR_PQW_ROW_GROUP_ROWS (\d+)", header).group(1)) == 1048576 == ffi.MCR_PQW_ROW_GROUP_ROWS


@pytest.mark.parametrize("row_group_rows", [0, 5000, W.PAGE_ROWS, W.PAGE_ROWS + 1])
def test_a_draws_table_reads_back_with_schema_bits_metadata_and_statistics(ffi, row_group_rows):
    rng = np.random.default_rng(3)
    C_, N = 4, W.PAGE_ROWS // 2 + 1
    rows = C_ * N
    x = rng.normal(size=(3, rows))                          # a [P][M] matrix: rows of a column are `P` apart when transposed
    xt = np.ascontiguousarray(x.T)
    cols = [("chain", INT64, np.repeat(np.arange(C_, dtype=np.int64), N)), ("draw", INT64, np.tile(np.arange(N, dtype=np.int64), C_)),
            ("a", DOUBLE, x[0]), ("b_interleaved", DOUBLE, xt[:, 1]), ("every_third", DOUBLE, rng.normal(size=3 * rows)[::3]),
            ("k", INT64, rng.integers(-2, 3, rows).astype(np.float64)), ("k32", INT32, rng.integers(-2, 3, rows)),
            ("sorted", DOUBLE, np.sort(rng.normal(size=rows))), ("const", DOUBLE, np.full(rows, 2.5)),
            ("chain_seq", INT32, ("seq", N, W.INT64_MAX)), ("draw_seq", INT64, ("seq", 1, N)), ("row", INT32, ("seq", 1, W.INT64_MAX)),
            ("zeros", INT32, ("seq", 1, 1))]
    image = write_host(ffi, cols, rows, row_group_rows)
    tokens = W.check_file(ffi.load_library(), image, cols, rows, row_group_rows)
    if row_group_rows == 0:                                 # distinct doubles are one literal per page; constants nearly vanish
        assert [len(t) for t in tokens["a"]] == [1] * len(tokens["a"])
        assert sum(len(t) for t in tokens["const"]) < rows // 7
        assert any(tok[0] == "copy" and tok[2] == N * 8 for t in tokens["draw"] for tok in t)      # draw repeats its chain's sequence


def test_special_doubles_keep_their_bits_and_the_statistics_rules(ffi):
    lib = ffi.load_library()
    sp = W.special_doubles()
    finite = sp[~np.isnan(sp)]
    cols = [("with_nan", DOUBLE, sp), ("tail", DOUBLE, np.resize(finite, len(sp))),
            ("zeros_mixed", DOUBLE, np.resize(np.array([0.0, -0.0]), len(sp))), ("neg_zero", DOUBLE, np.full(len(sp), -0.0)),
            ("below_zero", DOUBLE, np.resize(np.array([-1.0, -0.0]), len(sp))), ("above_zero", DOUBLE, np.resize(np.array([1.0, 0.0]), len(sp)))]
    image = write_host(ffi, cols, len(sp))
    W.check_file(lib, image, cols, len(sp))
    import io

    import pyarrow.parquet as pq
    md = pq.ParquetFile(io.BytesIO(image)).metadata.row_group(0)
    st = {md.column(k).path_in_schema: md.column(k).statistics for k in range(len(cols))}
    assert not st["with_nan"].has_min_max
    for name in ("zeros_mixed", "neg_zero"):
        assert np.signbit(st[name].min) and st[name].min == 0 and not np.signbit(st[name].max) and st[name].max == 0
    assert st["below_zero"].min == -1.0 and st["below_zero"].max == 0 and not np.signbit(st["below_zero"].max)
    assert st["above_zero"].max == 1.0 and st["above_zero"].min == 0 and np.signbit(st["above_zero"].min)


def test_integer_extremes(ffi):
    i64 = np.array([-2 ** 63, 2 ** 63 - 1, 0, -1, 1], dtype=np.int64)
    i32 = np.array([-2 ** 31, 2 ** 31 - 1, 0, -1, 1], dtype=np.int64)
    f = np.array([-2.0 ** 63, 2.0 ** 53, -0.0, -1.0, 2.0 ** 62])
    cols = [("i64", INT64, i64), ("i32", INT32, i32), ("f_as_i64", INT64, f), ("f_as_i32", INT32, i32.astype(np.float64))]
    W.check_file(ffi.load_library(), write_host(ffi, cols, 5), cols, 5)


@pytest.mark.parametrize("case", W.token_edge_cases(), ids=lambda c: c[0])
def test_token_edges(ffi, case):
    _id, col, rows, want = case
    tokens = W.check_file(ffi.load_library(), write_host(ffi, [col], rows), [col], rows)
    assert tokens[col[0]] == want


def test_the_walker_itself_refuses_what_the_writer_must_not_emit():
    ok = W.uvarint(8) + bytes([7 << 2]) + b"abcdefgh"
    assert W.snappy_walk(ok) == (b"abcdefgh", [("lit", 8)])
    far = W.uvarint(12) + bytes([7 << 2]) + b"abcdefgh" + bytes([3 | (3 << 2), 8, 0, 0, 0])          # tag 3: 4-byte offset
    with pytest.raises(AssertionError):
        W.snappy_walk(far)
    before = W.uvarint(12) + bytes([7 << 2]) + b"abcdefgh" + bytes([2 | (3 << 2), 9, 0])              # offset 9 > 8 produced
    with pytest.raises(AssertionError):
        W.snappy_walk(before)


REJECTED = [
    ("not-an-integer", [("x", INT64, np.array([1.0, 2.0, 1.5, 0.5]))], 4, ("'x'", "row 2")),
    ("int32-range", [("a", INT32, np.zeros(3)), ("y", INT32, np.array([0.0, 2.0 ** 31, 3e10]))], 3, ("'y'", "row 1")),
    ("int32-range-i64", [("y", INT32, np.array([0, -2 ** 31 - 1], dtype=np.int64))], 2, ("'y'", "row 1")),
    ("int64-range", [("z", INT64, np.array([2.0 ** 63]))], 1, ("'z'", "row 0")),
    ("nan-as-int", [("z", INT64, np.array([0.0, 1.0, np.nan]))], 3, ("'z'", "row 2")),
    ("second-page", [("w", INT64, np.concatenate([np.zeros(W.PAGE_ROWS + 5), [0.25]]))], W.PAGE_ROWS + 6, ("'w'", f"row {W.PAGE_ROWS + 5}")),
    ("no-rows", [("x", DOUBLE, np.zeros(1))], 0, ("row count",)),
    ("too-many-rows", [("x", INT32, ("seq", 1, 1))], 2 ** 31, ("row count",)),
    ("empty-name", [("", DOUBLE, np.zeros(1))], 1, ("empty name",)),
    ("duplicate-name", [("x", DOUBLE, np.zeros(1)), ("x", DOUBLE, np.zeros(1))], 1, ("duplicate", "'x'")),
    ("float-type", [("x", 4, np.zeros(1))], 1, ("type 4",)),
    ("byte-array-type", [("x", 6, np.zeros(1))], 1, ("type 6",)),
    ("int-source-as-double", [("x", DOUBLE, np.zeros(1, dtype=np.int64))], 1, ("'x'", "integer source")),
    ("sequence-as-double", [("x", DOUBLE, ("seq", 1, 1))], 1, ("'x'", "integer source")),
    ("sequence-div", [("x", INT32, ("seq", 0, 1))], 1, ("'x'", "seq_div")),
]


@pytest.mark.parametrize("case", REJECTED, ids=lambda c: c[0])
def test_rejections_name_what_is_wrong(ffi, case):
    _id, cols, rows, words = case
    with pytest.raises(ffi.McrError) as err:
        write_host(ffi, cols, rows)
    assert err.value.code == ffi.MCR_EINVAL
    for w in words:
        assert w in err.value.message, err.value.message


def test_no_columns_and_null_arguments(ffi):
    import ctypes as C
    lib = ffi.load_library()
    out = C.c_void_p()
    assert lib.mcr_parquet_write_host(None, None, 0, 1, 0, C.byref(out)) == ffi.MCR_EINVAL
    arr, _keep = ffi._pq_columns([ffi.pq_column("x", DOUBLE, np.zeros(2))], host=True)
    assert lib.mcr_parquet_write_host(None, arr, 1, 2, 0, None) == ffi.MCR_EINVAL
    assert lib.mcr_parquet_write_host(None, arr, 1, 2, -1, C.byref(out)) == ffi.MCR_EINVAL
    assert lib.mcr_parquet_write_dev(None, arr, 1, 2, 0, C.byref(out)) == ffi.MCR_EINVAL       # the device form needs a context
    assert lib.mcr_pq_image_size(None) == 0 and lib.mcr_pq_image_pages(None) == -1 and lib.mcr_pq_image_data(None) is None
    lib.mcr_pq_image_free(None)


def test_host_writer_is_deterministic_and_files_feed_the_host_footer_parser(ffi):
    rng = np.random.default_rng(5)
    cols = [("chain", INT64, np.repeat(np.arange(4, dtype=np.int64), 300)), ("x", DOUBLE, rng.normal(size=1200))]
    a, b = write_host(ffi, cols, 1200, 500), write_host(ffi, cols, 1200, 500)
    assert a == b and a[:4] == b"PAR1" and a[-4:] == b"PAR1"
    pages = W.pages_of(ffi.load_library(), a)
    assert [(p[0], p[3], p[4]) for p in pages] == [(0, 500, 0), (1, 500, 0), (0, 500, 500), (1, 500, 500), (0, 200, 1000), (1, 200, 1000)]


def test_convert_files_refuses_an_unknown_writer(tmp_path):
    from mcmc_ref_hip import convert
    with pytest.raises(ValueError, match="writer must be 'auto' or 'host'"):
        convert.convert_files([], tmp_path, tmp_path, writer="device")
