"""Draws exported as CSV on the GPU: Context.write_csv (mcr_csv_write_dev), Context.select_rows, reference.export_draws
and the `draws` command.  The device image equals the host image (mcr_csv_write_host) and pyarrow.csv.write_csv of the
same table, byte for byte (tests/csvwrite_cases.py); there are no tolerances."""
from __future__ import annotations

import io

import numpy as np
import pytest

import csvwrite_cases as W
import ragged_cases
from conftest import GOLDEN
from csvwrite_cases import DOUBLE, INT64

pytestmark = pytest.mark.gpu
MODELS = ("radon_pooled", "wells_data-wells_dist")


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    assert _ffi.MCR_CSVW_TILE_FIELDS == W.F and _ffi.MCR_SELECT_BLOCK_ROWS == W.SELECT_BLOCK
    with _ffi.Context(0) as c:
        yield c


class Uploaded:
    """The columns of csvwrite_cases in device memory, strides kept: views of one array share its upload."""

    def __init__(self, ctx, cols):
        from mcmc_ref_hip import _ffi
        self.bufs, self.columns, bases = [], [], {}
        for name, type_, src in cols:
            if isinstance(src, tuple):
                self.columns.append(_ffi.pq_sequence(name, type_, src[1], src[2]))
                continue
            a = np.asarray(src)
            base = a if a.base is None else a.base
            while base.base is not None:
                base = base.base
            if id(base) not in bases:
                self.bufs.append(_ffi.DeviceBuffer(ctx, max(base.nbytes, 8)).upload(base))
                bases[id(base)] = (self.bufs[-1], base)
            buf, base = bases[id(base)]
            kind = _ffi.MCR_PQW_F64 if a.dtype == np.float64 else _ffi.MCR_PQW_I64
            stride = a.strides[0] // 8 if a.size else 1
            self.columns.append(_ffi.pq_column(name, type_, buf.ptr.value + (a.ctypes.data - base.ctypes.data), stride, kind))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def write_dev(ctx, cols, rows, row_index=None, header="quoted") -> bytes:
    with Uploaded(ctx, cols) as up, ctx.write_csv(up.columns, rows, row_index, header) as image:
        return image.tobytes()


@pytest.mark.parametrize("n_cols", W.N_COLS)
def test_device_equals_host_and_pyarrow(ctx, n_cols):
    for rows in W.rows_for(n_cols):
        cols, rows = W.table_case(n_cols, rows)
        got = write_dev(ctx, cols, rows)
        assert got == W.write_host(cols, rows), rows
        assert got == W.expected(cols, rows), rows
    cols, rows = W.table_case(n_cols, W.rows_for(n_cols)[-1])
    for name, index in W.row_lists(rows).items():
        got = write_dev(ctx, cols, rows, index, "none")
        assert got == W.write_host(cols, rows, index, "none") == W.expected(cols, rows, index, "none"), name


def test_every_field_length_in_one_tile(ctx):
    cols, rows = W.length_class_columns()
    assert len(cols) * rows <= W.F
    got = write_dev(ctx, cols, rows, header="plain")
    assert got == W.write_host(cols, rows, header="plain") == W.expected(cols, rows, header="plain")
    assert {len(f) for line in got.split(b"\n")[1:-1] for f in line.split(b",")} == set(range(1, 26))


def test_edges_and_integers(ctx):
    x = np.array(W.EDGES + [-v for v in W.EDGES])
    i = np.resize(np.array(W.INT_EDGES, dtype=np.int64), x.size)
    cols = [("v", DOUBLE, x), ("i", INT64, i)]
    assert write_dev(ctx, cols, x.size) == W.expected(cols, x.size)
    from mcmc_ref_hip import _ffi
    bad = np.arange(600, dtype=np.float64)
    bad[[411, 500]] = 0.25
    with pytest.raises(_ffi.McrError, match=r"column 'frac', row 411 .*not an integer"):
        write_dev(ctx, [("v", DOUBLE, bad), ("frac", INT64, bad)], 600)
    with pytest.raises(_ffi.McrError, match=r"entry 2 of the row list"):
        write_dev(ctx, cols, x.size, np.array([0, 1, x.size, -1], dtype=np.int64))


def test_workspace_limit_writes_row_ranges(ctx):
    rows, n_cols = 3000, 40
    cols, rows = W.table_case(n_cols, rows)
    whole = write_dev(ctx, cols, rows)
    ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 1 << 20))      # the worst-case text alone is 3 000 x 40 x 26 bytes, 2.98 MiB
    ctx.profile(True)
    ctx.profile_reset()
    try:
        ranged = write_dev(ctx, cols, rows)
        launches = ctx.profile_get()["k_csvw_format"]["launches"]
        listed = write_dev(ctx, cols, rows, np.arange(rows, dtype=np.int64)[::-1].copy())
    finally:
        ctx.profile(False)
        ctx.profile_reset()
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 8 << 30))
    assert launches >= 3                                              # one launch per row range
    assert ranged == whole == W.expected(cols, rows)
    assert listed == W.expected(cols, rows, np.arange(rows)[::-1])


def test_same_bytes_twice_and_after_a_summary(ctx):
    from mcmc_ref_hip import synth
    cols, rows = W.table_case(7, 900)
    with Uploaded(ctx, cols) as up:
        def once():
            with ctx.write_csv(up.columns, rows) as image:
                return image.tobytes()
        first = once()
        assert once() == first
        ctx.summarize(synth.c1_model(4, 500, 3, seed=5), "pcn")           # the lane's workspace is carved anew, perhaps grown
        assert once() == first
    assert first == W.expected(cols, rows)


def select(ctx, chain: np.ndarray, chains) -> np.ndarray:
    from mcmc_ref_hip import _ffi
    buf = _ffi.DeviceBuffer(ctx, max(chain.nbytes, 8)).upload(chain)
    try:
        out, n = ctx.select_rows(buf, chain.size, chains)
        try:
            return out.download(np.int64, n) if n else np.zeros(0, dtype=np.int64)
        finally:
            out.free()
    finally:
        buf.free()


@pytest.mark.parametrize("chains", [[0], [3], [1, 2], [2, 1, 1], [], [7]])
def test_select_rows(ctx, chains):
    chain = np.repeat(np.arange(4, dtype=np.int64), 250)
    for M in (1000, W.SELECT_BLOCK - 1, W.SELECT_BLOCK, W.SELECT_BLOCK + 1, 1):
        c = chain[:: max(1000 // M, 1)][:M].copy() if M < 1000 else chain
        assert np.array_equal(select(ctx, c, chains), np.flatnonzero(np.isin(c, chains))), M


@pytest.mark.parametrize("pattern", ["ordered", "shuffled"])
def test_select_rows_ragged(ctx, pattern):
    chain, _draw = ragged_cases.id_columns(1337, pattern)
    for chains in ([0, 2], [3], [1, 1, 5]):
        assert np.array_equal(select(ctx, chain, chains), np.flatnonzero(np.isin(chain, chains)))


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from mcmc_ref_hip.store import DataStore
    root = tmp_path_factory.mktemp("csvw_store")
    (root / "draws").mkdir()
    for name in MODELS:
        (root / "draws" / f"{name}.draws.parquet").write_bytes((GOLDEN / "parquet" / f"{name}.draws.parquet").read_bytes())
    return DataStore(local_root=root, packaged_root=root / "none"), root


def arrow_csv(store, model, params, chains) -> bytes:
    import pyarrow.csv as pacsv
    from mcmc_ref_hip import reference
    sink = io.BytesIO()
    data = reference.draws(model, params=params, chains=chains, return_="arrow", store=store)
    pacsv.write_csv(data.read_all() if hasattr(data, "read_all") else data, sink)      # (write_csv takes a table, not a reader)
    return sink.getvalue()


@pytest.mark.parametrize("model", MODELS)
def test_export_draws_csv(ctx, store, model):
    import pyarrow.parquet as pq
    from mcmc_ref_hip import reference
    st, root = store
    names = [n for n in pq.read_schema(root / "draws" / f"{model}.draws.parquet").names if n not in ("chain", "draw")]
    for params in (None, [names[-1], names[0]]):
        for chains in (None, [0, 2], []):
            exp = arrow_csv(st, model, params, chains)
            for writer in ("auto", "host"):
                sink = io.BytesIO()
                reference.export_draws(model, sink, params=params, chains=chains, store=st, context=ctx, writer=writer)
                assert sink.getvalue() == exp, (params, chains, writer)
    assert exp.count(b"\n") == 1                                # chains = []: the header alone


@pytest.mark.parametrize("model", MODELS)
def test_export_draws_parquet(ctx, store, model, tmp_path):
    import pyarrow.parquet as pq
    from mcmc_ref_hip import reference
    st, _root = store
    reference.export_draws(model, tmp_path / "out.parquet", format_="parquet", store=st, context=ctx)
    table = reference.draws(model, return_="arrow", store=st)
    table = table.read_all() if hasattr(table, "read_all") else table
    got = pq.read_table(tmp_path / "out.parquet")
    assert got.equals(table)
    assert b"mcmc-ref-hip" in pq.ParquetFile(tmp_path / "out.parquet").metadata.created_by.encode()      # the device writer's file


def test_plain_header_reads_back_on_the_device(ctx, store, tmp_path):
    from mcmc_ref_hip import convert, parquet
    _st, root = store
    cols = parquet.read_columns(ctx, root / "draws" / "radon_pooled.draws.parquet")
    names = [n for n in cols if n not in ("chain", "draw")]
    assert all(np.all(cols[n] != np.trunc(cols[n])) for n in names)          # no column the reader would type int64
    table = [(n, DOUBLE if n in names else INT64, cols[n]) for n in cols]
    rows = cols["chain"].size
    with Uploaded(ctx, table) as up:
        parquet.write_csv_dev(ctx, tmp_path / "t.csv", up.columns, rows, header="plain")
    got = convert.read_csv_dev(tmp_path / "t.csv", context=ctx)
    assert got is not None
    d, fbuf, int_columns = got
    try:
        assert d.params == names and not any(int_columns)
        back = fbuf.download(np.float64, len(names) * rows).reshape(len(names), rows)
        assert np.array_equal(back.view(np.uint64), np.stack([cols[n] for n in names]).view(np.uint64))
    finally:
        d.free()
        fbuf.free()


def test_draws_command(store, tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mcmc_ref_hip import cli
    st, root = store
    monkeypatch.setenv("MCMC_REF_LOCAL_ROOT", str(root))
    out = tmp_path / "f.csv"
    r = CliRunner().invoke(cli.main, ["draws", "radon_pooled", "--params", "sigma,beta_0", "--chains", "0,1", "--output", str(out)])
    assert r.exit_code == 0, r.output
    exp = arrow_csv(st, "radon_pooled", ["sigma", "beta_0"], [0, 1])
    assert out.read_bytes() == exp
    r = CliRunner().invoke(cli.main, ["draws", "radon_pooled", "--params", "sigma,beta_0", "--chains", "0,1"])
    assert r.exit_code == 0, r.output
    assert r.stdout_bytes == exp
