"""Draws Parquet files written on the GPU: Context.write_parquet (mcr_parquet_write_dev) and the `writer` of
convert_files.  Every image is read by pyarrow (schema, bits, metadata, statistics), by the project's own device
decoder (the path mcr_summarize_files takes), found page by page with the project's footer parser, inflated with
pyarrow's Snappy and walked token by token, and written twice for byte identity (tests/pqwrite_cases.py)."""
from __future__ import annotations

import io
import json
import zipfile
from pathlib import Path

import numpy as np
import pytest

import pqwrite_cases as W
from pqwrite_cases import DOUBLE, INT32, INT64

pytestmark = pytest.mark.gpu
R = W.PAGE_ROWS


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    assert _ffi.MCR_PQW_PAGE_ROWS == R
    with _ffi.Context(0) as c:
        yield c


def write_dev(ctx, cols, rows, row_group_rows=0, strides=None) -> bytes:
    """cols as in pqwrite_cases; strides: {name: element stride} (the source is spread out accordingly), and
    {"interleave": [names]} puts those columns into one row-major [rows][P] matrix."""
    from mcmc_ref_hip import _ffi
    strides = strides or {}
    inter = [c for c in cols if c[0] in strides.get("interleave", ())]
    bufs, dev = [], []
    try:
        mat = None
        if inter:
            m = np.stack([np.asarray(c[2], dtype=np.float64)[:rows] for c in inter], axis=1)
            mat = _ffi.DeviceBuffer(ctx, m.nbytes).upload(m)
            bufs.append(mat)
        for name, type_, src in cols:
            if isinstance(src, tuple):
                dev.append(_ffi.pq_sequence(name, type_, src[1], src[2]))
                continue
            a = np.asarray(src)[:rows]
            kind = _ffi.MCR_PQW_F64 if a.dtype == np.float64 else _ffi.MCR_PQW_I64
            if mat is not None and any(name == c[0] for c in inter):
                k = [c[0] for c in inter].index(name)
                dev.append(_ffi.pq_column(name, type_, mat.ptr.value + 8 * k, len(inter), kind))
                continue
            s = strides.get(name, 1)
            wide = np.full(rows * s, 77, dtype=a.dtype)
            wide[::s] = a
            bufs.append(_ffi.DeviceBuffer(ctx, wide.nbytes).upload(wide))
            dev.append(_ffi.pq_column(name, type_, bufs[-1], s, kind))
        out = []
        for _ in range(2):
            with ctx.write_parquet(dev, rows, row_group_rows) as image:
                out.append(image.tobytes())
        assert out[0] == out[1], "the same columns gave different bytes"
        return out[0]
    finally:
        for b in bufs:
            b.free()


def check_own_decoder(ctx, image: bytes, cols, rows):
    from mcmc_ref_hip import parquet
    got = parquet.read_columns(ctx, image)
    for c in cols:
        want = W.expected_values(c, rows)
        if c[1] == DOUBLE:
            assert got[c[0]].view(np.uint64).tobytes() == want.view(np.uint64).tobytes(), c[0]
        else:
            assert np.array_equal(got[c[0]], want.astype(np.int64)), c[0]


def matrix_columns(rows: int, seed: int):
    """Six columns per file, every source kind and data kind of the matrix, by turns."""
    rng = np.random.default_rng(seed)
    N = R // 2 + 1
    chain = (np.arange(rows, dtype=np.int64) // N)
    draw = (np.arange(rows, dtype=np.int64) % N)
    five = rng.choice(np.array([-1.5, 0.0, 2.0, 1e300, 3.25]), rows)
    five_int = rng.integers(-2, 3, rows)
    a = [("chain", INT64, chain), ("draw", INT64, draw), ("normal", DOUBLE, rng.normal(size=rows)),
         ("five_as_int", INT64, five_int.astype(np.float64)), ("sorted", DOUBLE, np.sort(rng.normal(size=rows))),
         ("zeros", INT32, ("seq", 1, 1))]
    b = [("chain_seq", INT32, ("seq", N, W.INT64_MAX)), ("draw_seq", INT64, ("seq", 1, N)), ("row", INT64, ("seq", 1, W.INT64_MAX)),
         ("five", DOUBLE, five), ("const", DOUBLE, np.full(rows, -0.0)), ("five32", INT32, five_int.astype(np.int64))]
    c = [("draw32", INT32, draw), ("const_int", INT64, np.full(rows, 7.0)), ("normal", DOUBLE, rng.normal(size=rows)),
         ("sorted_int", INT64, np.sort(rng.integers(-10 ** 12, 10 ** 12, rows))), ("chain_f", INT32, chain.astype(np.float64)),
         ("special", DOUBLE, np.resize(W.special_doubles(), rows))]
    return [a, b, c]


ROWS = [1, 2, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3]


@pytest.mark.parametrize("rows", ROWS)
def test_edge_matrix(ctx, rows):
    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    for k, cols in enumerate(matrix_columns(rows, rows)):
        rgr = [0, R, R + 1][(ROWS.index(rows) + k) % 3]
        f64 = [c[0] for c in cols if not isinstance(c[2], tuple) and np.asarray(c[2]).dtype == np.float64]
        strides = [{}, {cols[0][0]: 3, cols[3][0]: 3, cols[4][0]: 3}, {"interleave": f64}][(k + rows) % 3]
        image = write_dev(ctx, cols, rows, rgr, strides)
        W.check_file(lib, image, cols, rows, rgr)
        check_own_decoder(ctx, image, cols, rows)


def test_every_stride_and_row_group_size_on_one_shape(ctx):
    from mcmc_ref_hip import _ffi
    lib = _ffi.load_library()
    rows = R + 1
    cols = matrix_columns(rows, 9)[0]
    f64 = [c[0] for c in cols if not isinstance(c[2], tuple) and np.asarray(c[2]).dtype == np.float64]
    images = {}
    for rgr in (0, R, R + 1):
        for tag, strides in (("1", {}), ("3", {c[0]: 3 for c in cols}), ("P", {"interleave": f64})):
            images[rgr, tag] = write_dev(ctx, cols, rows, rgr, strides)
            W.check_file(lib, images[rgr, tag], cols, rows, rgr)
        assert images[rgr, "1"] == images[rgr, "3"] == images[rgr, "P"]           # the bytes depend on the values alone
    check_own_decoder(ctx, images[R, "P"], cols, rows)


@pytest.mark.parametrize("case", W.token_edge_cases(), ids=lambda c: c[0])
def test_token_edges(ctx, case):
    from mcmc_ref_hip import _ffi
    _id, col, rows, want = case
    tokens = W.check_file(_ffi.load_library(), write_dev(ctx, [col], rows), [col], rows)
    assert tokens[col[0]] == want


def test_size_conditions(ctx):
    """From the format, not from a measurement: a page of distinct doubles is one literal behind its header, level
    block and preamble (<= 8 bytes a row + 64 a page); a constant column is 3 bytes per 64-byte copy = 0.375 bytes a row
    (<= 0.5 a row + 64 a page)."""
    import pyarrow.parquet as pq
    rows = 2 * R + 3
    rng = np.random.default_rng(2)
    cols = [("distinct", DOUBLE, rng.normal(size=rows)), ("const", DOUBLE, np.full(rows, 1.25)), ("const_seq", INT64, ("seq", 1, 1))]
    image = write_dev(ctx, cols, rows)
    md = pq.ParquetFile(io.BytesIO(image)).metadata.row_group(0)
    pages = -(-rows // R)
    assert md.column(0).total_compressed_size <= 8 * rows + 64 * pages
    assert md.column(1).total_compressed_size <= 0.5 * rows + 64 * pages
    assert md.column(2).total_compressed_size <= 0.5 * rows + 64 * pages


def test_default_row_groups(ctx):
    import pyarrow.parquet as pq
    from mcmc_ref_hip import _ffi
    rows = _ffi.MCR_PQW_ROW_GROUP_ROWS + 5
    x = np.random.default_rng(4).normal(size=rows)
    buf = _ffi.DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        with ctx.write_parquet([_ffi.pq_sequence("row", INT64), _ffi.pq_column("x", DOUBLE, buf, 1, _ffi.MCR_PQW_F64)], rows) as image:
            assert image.pages == 2 * (rows // R + 1)
            data = image.tobytes()
    finally:
        buf.free()
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    assert [md.row_group(g).num_rows for g in range(md.num_row_groups)] == [_ffi.MCR_PQW_ROW_GROUP_ROWS, 5]
    t = pq.read_table(io.BytesIO(data))
    assert np.array_equal(t["row"].to_numpy(), np.arange(rows)) and t["x"].to_numpy().tobytes() == x.tobytes()


REJECTED = [
    ("not-an-integer", ("x", INT64, np.array([1.0, 2.0, 1.5, 0.5])), ("'x'", "row 2")),
    ("int32-range", ("y", INT32, np.array([0.0, 2.0 ** 31, 3e10])), ("'y'", "row 1")),
    ("int64-range", ("z", INT64, np.array([2.0 ** 63])), ("'z'", "row 0")),
    ("i64-into-int32", ("y", INT32, np.array([5, 2 ** 31], dtype=np.int64)), ("'y'", "row 1")),
    ("sequence-into-int32", ("s", INT32, ("seq", 1, W.INT64_MAX)), None),
    ("second-page", ("w", INT64, np.concatenate([np.zeros(R + 5), [0.25, 0.5]])), ("'w'", f"row {R + 5}")),
]


@pytest.mark.parametrize("case", REJECTED, ids=lambda c: c[0])
def test_conversion_failures_name_column_and_first_row(ctx, case):
    from mcmc_ref_hip import _ffi
    _id, col, words = case
    rows = len(col[2]) if not isinstance(col[2], tuple) else 5
    if words is None:                                   # a row number fits INT32 for every row count the call accepts
        write_dev(ctx, [col], rows)
        return
    with pytest.raises(_ffi.McrError) as err:
        write_dev(ctx, [("ok", DOUBLE, np.zeros(rows)), col], rows)
    assert err.value.code == _ffi.MCR_EINVAL
    for w in words:
        assert w in err.value.message, err.value.message


def test_argument_errors(ctx):
    from mcmc_ref_hip import _ffi
    buf = _ffi.DeviceBuffer(ctx, 64)
    try:
        col = _ffi.pq_column("x", DOUBLE, buf, 1, _ffi.MCR_PQW_F64)
        for cols, rows in (([col], 0), ([col], 2 ** 31), ([col, col], 4), ([_ffi.pq_column("", DOUBLE, buf, 1, _ffi.MCR_PQW_F64)], 4),
                           ([_ffi.pq_column("x", 4, buf, 1, _ffi.MCR_PQW_F64)], 4), ([_ffi.pq_column("x", DOUBLE, buf, 0, _ffi.MCR_PQW_F64)], 4),
                           ([_ffi.pq_column("x", DOUBLE, buf, 1, _ffi.MCR_PQW_I64)], 4)):
            with pytest.raises(_ffi.McrError) as err:
                ctx.write_parquet(cols, rows)
            assert err.value.code == _ffi.MCR_EINVAL
    finally:
        buf.free()


# ---- through the public interface -----------------------------------------------------------------------------------
def table_csv(C_=4, N=250, ids=("chain", "draw"), seed=0) -> bytes:
    rng = np.random.default_rng(seed)
    head = [*ids, "a", "count", "b"]
    lines = [",".join(head)]
    for c in range(C_):
        for n in range(N):
            row = {"chain": str(c), "draw": str(n), "a": "%.17g" % rng.normal(), "count": str(int(rng.integers(0, 50))),
                   "b": "%.17g" % rng.normal()}
            lines.append(",".join(row[h] for h in head))
    return ("\n".join(lines) + "\n").encode()


def json_archive(path: Path, C_=4, N=250, seed=1) -> Path:
    rng = np.random.default_rng(seed)
    chains = [{"mu": rng.normal(size=N).tolist(), "count": rng.integers(0, 9, N).tolist(), "tau": rng.normal(size=N).tolist()}
              for _ in range(C_)]
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr("model.json", json.dumps(chains))
    return path


def convert_both(ctx, tmp_path, jobs, force=True, writers=("auto", "host")):
    from mcmc_ref_hip import convert
    outs = []
    for w in writers:
        out = tmp_path / f"out_{w}_{len(list(tmp_path.iterdir()))}"
        (out / "draws").mkdir(parents=True)
        (out / "meta").mkdir()
        outs.append((out, convert.convert_files(jobs, out / "draws", out / "meta", force=force, context=ctx, writer=w)))
    return outs


def test_convert_files_writes_on_the_device_and_both_writers_agree(ctx, tmp_path):
    import pyarrow.parquet as pq
    csv = tmp_path / "t.csv"
    csv.write_bytes(table_csv())
    jobs = [(csv, "csv_model"), (json_archive(tmp_path / "j.json.zip"), "json_model")]
    (_, auto), (_, host) = convert_both(ctx, tmp_path, jobs)
    for a, h in zip(auto, host):
        assert not isinstance(a, Exception) and not isinstance(h, Exception), (a, h)
        ta, th = pq.read_table(a.draws_path), pq.read_table(h.draws_path)
        assert ta.schema.equals(th.schema) and ta.equals(th)
        assert str(ta.schema.field("count").type) == "int64" and ta.num_rows == 1000
        assert a.meta_path.read_text() == h.meta_path.read_text()
        assert pq.ParquetFile(a.draws_path).metadata.created_by.startswith("mcmc-ref-hip")
        assert pq.ParquetFile(h.draws_path).metadata.created_by.startswith("parquet-cpp")
    # the project's own file reader gives the same statistics from either file, exactly
    for a, h in zip(auto, host):
        (info_a, ra), (info_h, rh) = ctx.summarize_files([str(a.draws_path)]), ctx.summarize_files([str(h.draws_path)])
        assert info_a == info_h
        for key in ra:
            assert np.array_equal(ra[key], rh[key], equal_nan=True), key


@pytest.mark.parametrize("ids", [(), ("chain",), ("draw",)], ids=lambda i: "+".join(i) or "none")
def test_missing_bookkeeping_columns_are_appended_as_int32(ctx, tmp_path, ids):
    import pyarrow as pa
    import pyarrow.parquet as pq
    csv = tmp_path / "t.csv"
    csv.write_bytes(table_csv(1 if "chain" not in ids else 4, 40, ids, seed=3))
    (_, (a,)), (_, (h,)) = convert_both(ctx, tmp_path, [(csv, "m")])
    ta, th = pq.read_table(a.draws_path), pq.read_table(h.draws_path)
    assert pq.ParquetFile(a.draws_path).metadata.created_by.startswith("mcmc-ref-hip")
    assert ta.schema.equals(th.schema) and ta.equals(th)
    missing = [n for n in ("chain", "draw") if n not in ids]
    assert ta.column_names == [*ids, "a", "count", "b", *missing]
    assert all(ta.schema.field(n).type == pa.int32() for n in missing)
    assert a.meta_path.read_text() == h.meta_path.read_text()


def test_a_failed_quality_gate_writes_nothing_on_either_route(ctx, tmp_path):
    csv = tmp_path / "t.csv"
    csv.write_bytes(table_csv())                       # 1000 draws: `ndraws_is_10k` fails
    for out, res in convert_both(ctx, tmp_path, [(csv, "m")], force=False):
        assert isinstance(res[0], ValueError) and "quality checks failed" in str(res[0])
        assert list((out / "draws").iterdir()) == [] and list((out / "meta").iterdir()) == []


def test_the_environment_variable_selects_pyarrow_and_an_unknown_writer_raises(ctx, tmp_path, monkeypatch):
    import pyarrow.parquet as pq
    from mcmc_ref_hip import convert
    csv = tmp_path / "t.csv"
    csv.write_bytes(table_csv(4, 30))
    monkeypatch.setenv("MCMC_REF_HIP_WRITER", "arrow")
    (_, (a,)), = convert_both(ctx, tmp_path, [(csv, "m")], writers=("auto",))
    assert pq.ParquetFile(a.draws_path).metadata.created_by.startswith("parquet-cpp")
    monkeypatch.delenv("MCMC_REF_HIP_WRITER")
    with pytest.raises(ValueError, match="writer must be 'auto' or 'host'"):
        convert.convert_files([(csv, "m")], tmp_path, tmp_path, context=ctx, writer="device")


def test_write_draws_dev_writes_the_file(ctx, tmp_path):
    import pyarrow.parquet as pq
    from mcmc_ref_hip import _ffi, parquet
    x = np.arange(12, dtype=np.float64).reshape(3, 4)           # [rows][P]
    buf = _ffi.DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        cols = [_ffi.pq_sequence("draw", INT32)] + [_ffi.pq_column(f"p{k}", DOUBLE, buf.ptr.value + 8 * k, 4, _ffi.MCR_PQW_F64) for k in range(4)]
        size = parquet.write_draws_dev(ctx, tmp_path / "d.parquet", cols, 3)
    finally:
        buf.free()
    assert size == (tmp_path / "d.parquet").stat().st_size
    t = pq.read_table(tmp_path / "d.parquet")
    assert t.column_names == ["draw", "p0", "p1", "p2", "p3"] and np.array_equal(t["p2"].to_numpy(), x[:, 2])
