"""No error path of the Python readers leaves device memory allocated.

A proxy stands in for `ctx.lib`: it forwards every attribute to the real library, keeps the set of live pointers of
mcr_dev_alloc / mcr_dev_free, and can make the k-th call among mcr_dev_alloc, mcr_memcpy_h2d and mcr_memcpy_d2h answer
MCR_ENOMEM without calling through -- a return code on the host; nothing is launched and nothing on the device fails.
Every path runs clean first (the live set is back at the baseline once the caller has freed what it was given), then
with k = 1, 2, ... until a run ends without the injection firing: the call raises McrError (or the ValueError
value_errors() makes of it) and the live set is back at the baseline.  convert_files is the one path whose contract is
to report a job's failure as that job's result and to send a job the device reader fails on to the host reader: there
a run that swallows the injected failure is accepted, and the live set is checked all the same.

Files: 4 chains x 8 draws x 2 parameters each, written here."""
from __future__ import annotations

import io
import json
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CHAINS, DRAWS, CAP = 4, 8, 64
M = CHAINS * DRAWS


class CountingLib:
    """The library with its memory calls counted: `live` holds the pointers allocated and not freed through it."""
    COUNTED = ("mcr_dev_alloc", "mcr_memcpy_h2d", "mcr_memcpy_d2h")

    def __init__(self, real):
        self.real, self.live, self.calls, self.fail_at, self.fired = real, set(), 0, None, False
        for name in self.COUNTED:
            setattr(self, name, self._counted(name))

    def __getattr__(self, name):
        return getattr(self.real, name)

    def arm(self, k):
        self.calls, self.fail_at, self.fired = 0, k, False

    def _counted(self, name):
        from mcmc_ref_hip import _ffi
        entry = getattr(self.real, name)

        def call(handle, *args):
            self.calls += 1
            if self.calls == self.fail_at:
                self.fired = True
                return _ffi.MCR_ENOMEM
            rc = entry(handle, *args)
            if name == "mcr_dev_alloc" and rc == _ffi.MCR_OK:
                self.live.add(args[1]._obj.value)
            return rc
        return call

    def mcr_dev_free(self, handle, ptr):
        self.live.discard(ptr.value)
        return self.real.mcr_dev_free(handle, ptr)


@pytest.fixture(scope="module")
def real_ctx():
    from mcmc_ref_hip import _ffi
    with _ffi.Context(0) as c:
        yield c


@pytest.fixture()
def ctx(real_ctx):
    real_ctx.lib = CountingLib(real_ctx.lib)
    yield real_ctx
    real_ctx.lib = real_ctx.lib.real


def sweep(ctx, call, release=lambda got: None, swallows: bool = False) -> list:
    """The clean run, then the runs with the k-th counted call failing: [(k, raised, live pointers above the baseline)]
    of the runs in which the injection fired.  The caller asserts; `release` frees what a run that returns was given."""
    from mcmc_ref_hip import _ffi
    lib, base = ctx.lib, set(ctx.lib.live)
    lib.arm(None)
    release(call())
    assert lib.live == base, f"the clean run leaves {len(lib.live - base)} allocation(s)"
    seen = []
    for k in range(1, CAP + 1):
        lib.arm(k)
        try:
            got = call()
        except (_ffi.McrError, ValueError):
            assert lib.fired, f"k = {k}: raised without the injection"
            raised = True
        else:
            release(got)
            raised = False
            if not lib.fired:
                lib.arm(None)
                return seen
        lib.arm(None)
        seen.append((k, raised, len(lib.live - base)))
        base = set(lib.live)                                    # (a leak is counted once, at its own k)
        assert raised or swallows, f"k = {k}: the call returned although the injected failure fired"
    pytest.fail(f"the path makes more than {CAP} counted calls")


def check(ctx, call, release=lambda got: None, swallows: bool = False):
    seen = sweep(ctx, call, release, swallows)
    print("injected (k, raised, leaked):", seen)
    assert seen, "the injection never fired: the path makes no counted call"
    assert [k for k, _raised, leaked in seen if leaked] == [], seen


def free_all(owners):
    for o in owners:
        o.free()


def draws_columns(seed: int, shuffled: bool):
    rng = np.random.default_rng(seed)
    chain, draw = np.repeat(np.arange(CHAINS, dtype=np.int64), DRAWS), np.tile(np.arange(DRAWS, dtype=np.int64), CHAINS)
    order = rng.permutation(M) if shuffled else np.arange(M)
    return chain[order], draw[order], rng.standard_normal(M), rng.standard_normal(M)


def write_parquet(path, seed: int, shuffled: bool):
    from mcmc_ref_hip import _ffi
    chain, draw, a, b = draws_columns(seed, shuffled)
    cols = [_ffi.pq_column("chain", _ffi.MCR_PQ_INT64, chain), _ffi.pq_column("draw", _ffi.MCR_PQ_INT64, draw),
            _ffi.pq_column("a", _ffi.MCR_PQ_DOUBLE, a), _ffi.pq_column("b", _ffi.MCR_PQ_DOUBLE, b)]
    with _ffi.write_parquet_host(cols, M) as image:
        path.write_bytes(image.view)
    return path


def write_csv(path, seed: int, shuffled: bool, with_draw: bool = True):
    chain, draw, a, b = draws_columns(seed, shuffled)
    head = "chain,draw,a,b" if with_draw else "chain,a,b"
    rows = [f"{c},{d},{x!r},{y!r}" if with_draw else f"{c},{x!r},{y!r}"
            for c, d, x, y in zip(chain.tolist(), draw.tolist(), a.tolist(), b.tolist())]
    path.write_text("\n".join([head, *rows]) + "\n")
    return path


def write_json_zip(path, seed: int):
    _chain, _draw, a, b = draws_columns(seed, False)
    doc = [{"a": a[c * DRAWS:(c + 1) * DRAWS].tolist(), "b": b[c * DRAWS:(c + 1) * DRAWS].tolist()} for c in range(CHAINS)]
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr("draws.json", json.dumps(doc))
    return path


def test_context_upload_and_upload_sims(ctx):
    check(ctx, lambda: ctx.upload(np.zeros((2, CHAINS, DRAWS))), lambda t: t.free())
    check(ctx, lambda: ctx.upload_sims(np.zeros((1, 2, CHAINS, DRAWS))), lambda t: t.free())


def test_summarize_chains_of_a_host_array(ctx):
    x = np.random.default_rng(1).standard_normal((2, M))
    check(ctx, lambda: ctx.summarize_chains(x, [8, 8, 9, 7]))


def test_write_csv_with_a_host_row_index_and_select_rows(ctx):
    from mcmc_ref_hip import _ffi
    chain, _draw, a, _b = draws_columns(2, False)
    col, ids = _ffi.DeviceBuffer(ctx, M * 8).upload(a), _ffi.DeviceBuffer(ctx, M * 8).upload(chain)
    try:
        columns = [_ffi.pq_column("a", _ffi.MCR_PQ_DOUBLE, col, 1, _ffi.MCR_PQW_F64)]
        check(ctx, lambda: ctx.write_csv(columns, M, row_index=np.arange(0, M, 3)), lambda image: image.close())
        check(ctx, lambda: ctx.select_rows(ids, M, [0, 2]), lambda got: got[0].free())
    finally:
        free_all([col, ids])


def test_read_draws_many_with_a_file_whose_rows_need_the_gather(ctx, tmp_path):
    from mcmc_ref_hip import parquet
    paths = [write_parquet(tmp_path / "ordered.parquet", 3, False), write_parquet(tmp_path / "shuffled.parquet", 4, True)]
    got = parquet.read_draws_many(ctx, paths)
    chain, draw = draws_columns(4, True)[:2]
    want = [np.stack(draws_columns(3, False)[2:]), np.stack(draws_columns(4, True)[2:])[:, np.lexsort((draw, chain))]]
    assert all(np.array_equal(d.to_host(), w) and d.tensor is not None for d, w in zip(got, want))
    assert got[0].buf.ptr.value != got[1].buf.ptr.value
    free_all(got)
    check(ctx, lambda: parquet.read_draws_many(ctx, paths), free_all)


def test_read_columns(ctx, tmp_path):
    from mcmc_ref_hip import parquet
    path = write_parquet(tmp_path / "shuffled.parquet", 5, True)
    check(ctx, lambda: parquet.read_columns(ctx, path))


def test_csv_table_decode_through_read_csv_many_dev(ctx, tmp_path):
    from mcmc_ref_hip import convert
    paths = [write_csv(tmp_path / "nodraw.csv", 6, False, with_draw=False), write_csv(tmp_path / "shuffled.csv", 7, True)]

    def release(got):
        for d, fbuf, *_rest in got:
            d.free()
            fbuf.free()

    got = convert.read_csv_many_dev(paths, ctx)
    chain, draw = draws_columns(7, True)[:2]
    assert np.array_equal(got[0][0].to_host(), np.stack(draws_columns(6, False)[2:]))
    assert np.array_equal(got[1][0].to_host(), np.stack(draws_columns(7, True)[2:])[:, np.lexsort((draw, chain))])
    assert np.array_equal(got[1][1].download(np.float64, 2 * M).reshape(2, M), np.stack(draws_columns(7, True)[2:]))
    release(got)
    check(ctx, lambda: convert.read_csv_many_dev(paths, ctx), release)


def test_read_json_zip_dev(ctx, tmp_path):
    from mcmc_ref_hip import convert
    path = write_json_zip(tmp_path / "m.json.zip", 8)
    check(ctx, lambda: convert.read_json_zip_dev(path, context=ctx), lambda got: got[1].free())


@pytest.mark.parametrize("writer", ["auto", "host"])
def test_convert_files_of_a_csv_and_a_json_zip(ctx, tmp_path, writer):
    from mcmc_ref_hip import convert
    jobs = [(write_csv(tmp_path / "c.csv", 9, True), "c"), (write_json_zip(tmp_path / "j.json.zip", 10), "j")]

    def call():
        got = convert.convert_files(jobs, tmp_path, tmp_path, force=True, context=ctx, writer=writer)
        assert all(isinstance(r, (convert.ConvertResult, Exception)) for r in got), got
        return got

    assert all(isinstance(r, convert.ConvertResult) for r in call())
    check(ctx, call, swallows=True)


def test_export_draws_to_csv_with_a_chain_selection(ctx, tmp_path):
    from mcmc_ref_hip import reference
    from mcmc_ref_hip.store import DataStore
    (tmp_path / "draws").mkdir()
    write_parquet(tmp_path / "draws" / "m.draws.parquet", 11, True)
    store = DataStore(local_root=tmp_path, packaged_root=tmp_path / "none")
    check(ctx, lambda: reference.export_draws("m", io.BytesIO(), chains=[0, 2], store=store, context=ctx, writer="device"))
