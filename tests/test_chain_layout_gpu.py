"""The device row order (mcr_chain_layout_dev, mcr_gather_rows_order_dev; csrc/mcr_layout.hpp) against
np.lexsort((draw, chain)) -- the order of the reference's `_chains_from_table` (src/mcmc_ref/convert.py:150-161;
tests/test_layout_refs_cpu.py shows the two agree).  Order, chain ids and counts exactly; gathered draws bit for bit."""
from __future__ import annotations

import ctypes as C
import io
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import ragged_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

SPAN = int(re.search(r"#define MCR_LAYOUT_SPAN (\d+)", (ROOT / "include" / "mcmcref_hip.h").read_text()).group(1))
SIZES = [0, 1, 2, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 1, 70001]      # 70 001: row numbers beyond 16 bits
PATTERNS = ("ordered", "reversed", "shuffled", "interleaved", "single", "duplicates")
SENTINEL = -7


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip._ffi import Context
    c = Context(0)
    yield c
    c.close()


def layout(ctx, chain, draw, cap=256):
    """(rc, order as the call left the buffer, ids, counts, in_order) of one mcr_chain_layout_dev call."""
    from mcmc_ref_hip._ffi import DeviceBuffer
    M = int(chain.size)
    ids_dev = DeviceBuffer(ctx, max(2 * M * 8, 8))
    order_dev = DeviceBuffer(ctx, max(M * 8, 8))
    try:
        if M:
            ids_dev.upload(np.concatenate([chain, draw]).astype(np.int64))
            order_dev.upload(np.full(M, SENTINEL, dtype=np.int64))
        ids, counts = np.zeros(max(cap, 1), dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int64)
        n, in_order = C.c_int(-1), C.c_int(-1)
        ip = C.POINTER(C.c_int64)
        rc = ctx.lib.mcr_chain_layout_dev(ctx.handle, ids_dev.ptr, C.c_void_p(ids_dev.ptr.value + M * 8), M, order_dev.ptr,
                                          ids.ctypes.data_as(ip), counts.ctypes.data_as(ip), cap, C.byref(n),
                                          C.byref(in_order))
        order = order_dev.download(np.int64, M) if M else np.zeros(0, dtype=np.int64)
        return rc, order, ids[:max(n.value, 0)], counts[:max(n.value, 0)], in_order.value
    finally:
        ids_dev.free()
        order_dev.free()


def expect(chain, draw):
    ids, counts = np.unique(chain, return_counts=True)
    order = np.lexsort((draw, chain))
    return order, ids, counts, bool(np.array_equal(order, np.arange(chain.size)))


def check(ctx, chain, draw, cap=256):
    rc, order, ids, counts, in_order = layout(ctx, chain, draw, cap)
    assert rc == 0, ctx.lib.mcr_last_error(ctx.handle)
    e_order, e_ids, e_counts, e_in = expect(chain, draw)
    assert in_order == int(e_in)
    assert np.array_equal(ids, e_ids) and np.array_equal(counts, e_counts)
    if e_in:
        assert np.all(order == SENTINEL)                    # no sort ran, the buffer is untouched
    else:
        assert np.array_equal(order, e_order)
    return e_order


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", SIZES)
def test_order_ids_counts(ctx, M, pattern):
    chain, draw = ragged_cases.id_columns(M, pattern)
    check(ctx, chain, draw)


def test_negative_ids(ctx):
    rng = np.random.default_rng(11)
    chain = rng.integers(-9, -2, size=5000).astype(np.int64)
    draw = rng.integers(-700, 300, size=5000).astype(np.int64)
    check(ctx, chain, draw)


def test_wide_ids_take_several_passes(ctx):
    rng = np.random.default_rng(12)
    chain = rng.choice(np.array([-5, 0, 2**40], dtype=np.int64), size=SPAN + 77)
    draw = rng.integers(0, 2**20 + 1, size=chain.size).astype(np.int64)
    draw[3] = 2**20
    check(ctx, chain, draw)                                 # 41 + 21 key bits: eight passes, a shift of 21


def test_draws_alone_fill_the_key(ctx):
    draw = np.array([2**63 - 1, -2**63, 0, 5, -1], dtype=np.int64)     # 64 bits of draw range, one chain: the shift is 64
    check(ctx, np.zeros(5, dtype=np.int64), draw)


def test_many_chains_and_the_cap(ctx):
    from mcmc_ref_hip._ffi import MCR_EINVAL
    rng = np.random.default_rng(13)
    chain = np.concatenate([np.arange(300), rng.integers(0, 300, size=1500)]).astype(np.int64)
    chain = chain[rng.permutation(chain.size)]
    draw = rng.integers(0, 40, size=chain.size).astype(np.int64)
    check(ctx, chain, draw, cap=300)
    rc, *_ = layout(ctx, chain, draw, cap=256)
    assert rc == MCR_EINVAL
    check(ctx, np.sort(chain), np.zeros(chain.size, dtype=np.int64), cap=300)       # ... and in order, without a sort
    rc, *_ = layout(ctx, np.sort(chain), np.zeros(chain.size, dtype=np.int64), cap=299)
    assert rc == MCR_EINVAL


def test_many_tables_in_one_round_trip(ctx):
    from mcmc_ref_hip._ffi import DeviceBuffer
    cols = [ragged_cases.id_columns(M, pattern, seed=3) for M, pattern in
            ((0, "ordered"), (1, "ordered"), (SPAN + 1, "ordered"), (300, "shuffled"), (70001, "ordered"), (257, "duplicates"),
             (4, "reversed"), (3 * SPAN, "single"))]
    cols.append((np.arange(300, dtype=np.int64), np.zeros(300, dtype=np.int64)))          # in order, more chains than cap
    flat = np.concatenate([np.concatenate([c, d]) for c, d in cols])
    buf = DeviceBuffer(ctx, flat.nbytes).upload(flat)
    try:
        tables, off = [], 0
        for c, d in cols:
            tables.append((buf.ptr.value + off * 8, buf.ptr.value + (off + c.size) * 8, c.size))
            off += 2 * c.size
        got = ctx.chain_layout_many(tables, cap=256)
    finally:
        buf.free()
    for (c, d), g in zip(cols, got):
        _order, e_ids, e_counts, e_in = expect(c, d)
        if not e_in or e_ids.size > 256:
            assert g is None
        else:
            assert np.array_equal(g[0], e_ids) and np.array_equal(g[1], e_counts)
    assert [g is None for g in got] == [False, False, False, True, False, True, True, True, True]


def wide_table(seed=14, M=3000, P=3):
    rng = np.random.default_rng(seed)
    chain = rng.choice(np.array([-2**62, 0, 2**62], dtype=np.int64), size=M)
    draw = rng.permutation(M).astype(np.int64)
    cols = {"chain": chain, "draw": draw}
    cols.update({f"p{j}": rng.normal(size=M) for j in range(P)})
    return pa.table(cols)


def image(table) -> bytes:
    buf = io.BytesIO()
    pq.write_table(table, buf)
    return buf.getvalue()


def test_more_than_64_key_bits_falls_back(ctx):
    from mcmc_ref_hip._ffi import MCR_EFALLBACK
    from mcmc_ref_hip.convert import table_to_tensor
    from mcmc_ref_hip.parquet import read_draws
    t = wide_table()
    chain, draw = t["chain"].to_numpy(), t["draw"].to_numpy()
    rc, *_ = layout(ctx, chain, draw)
    assert rc == MCR_EFALLBACK                              # 64 bits of chain range + 12 of draw range
    d = read_draws(ctx, image(t))                           # ... and the reader sorts on the host instead
    try:
        x, counts = table_to_tensor(t, ["p0", "p1", "p2"])
        assert np.array_equal(d.counts, counts) and np.array_equal(d.chain_ids, np.unique(chain))
        assert np.array_equal(d.to_host().view(np.int64), x.view(np.int64))
    finally:
        d.free()


@pytest.mark.parametrize("M,P", [(1, 1), (257, 3), (SPAN + 1, 2), (70001, 2)])
def test_gather_is_bit_equal(ctx, M, P):
    from mcmc_ref_hip._ffi import DeviceBuffer
    rng = np.random.default_rng(M)
    chain, draw = ragged_cases.id_columns(M, "shuffled", seed=1)
    x = rng.normal(size=(P, M))
    x[0, 0] = -0.0
    x[-1, -1] = np.nan
    bufs = [DeviceBuffer(ctx, 2 * M * 8), DeviceBuffer(ctx, P * M * 8), DeviceBuffer(ctx, P * M * 8)]
    try:
        bufs[0].upload(np.concatenate([chain, draw]))
        bufs[1].upload(x)
        got = ctx.chain_layout(bufs[0].ptr, C.c_void_p(bufs[0].ptr.value + M * 8), M)
        _ids, order, _counts = got
        e_order = np.lexsort((draw, chain))
        if order is None:
            assert np.array_equal(e_order, np.arange(M))
            return
        try:
            ctx.gather_rows_order(bufs[1].ptr, P, M, order.ptr, bufs[2].ptr)
        finally:
            order.free()
        out = bufs[2].download(np.float64, P * M).reshape(P, M)
        assert np.array_equal(out.view(np.int64), x[:, e_order].view(np.int64))
    finally:
        for b in bufs:
            b.free()


def test_gather_refuses_an_order_out_of_range(ctx):
    from mcmc_ref_hip._ffi import MCR_EINVAL, DeviceBuffer, McrError
    M = 300
    bufs = [DeviceBuffer(ctx, M * 8), DeviceBuffer(ctx, M * 8), DeviceBuffer(ctx, M * 8)]
    try:
        order = np.arange(M, dtype=np.int64)
        order[17] = M
        bufs[0].upload(order)
        bufs[1].upload(np.zeros(M))
        with pytest.raises(McrError) as ei:
            ctx.gather_rows_order(bufs[1].ptr, 1, M, bufs[0].ptr, bufs[2].ptr)
        assert ei.value.code == MCR_EINVAL
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("pattern", ["shuffled", "interleaved", "ordered"])
def test_read_draws_many_on_a_shuffled_file(ctx, pattern):
    from mcmc_ref_hip.convert import table_to_tensor
    from mcmc_ref_hip.parquet import read_draws_many
    tables = []
    for k, M in enumerate((4100, 257)):
        chain, draw = ragged_cases.id_columns(M, pattern, seed=k)
        rng = np.random.default_rng(M)
        tables.append(pa.table({"chain": chain, "a": rng.normal(size=M), "draw": draw, "b": rng.normal(size=M)}))
    ctx.profile(True)
    ctx.profile_reset()
    try:
        got = read_draws_many(ctx, [image(t) for t in tables])
        prof = ctx.profile_get()
    finally:
        ctx.profile(False)
    try:
        assert "k_layout_scan" in prof                       # the layout came from the device
        assert ("k_layout_scatter" in prof) == (pattern != "ordered")
        for d, t in zip(got, tables):
            x, counts = table_to_tensor(t, ["a", "b"])
            assert d.params == ["a", "b"]
            assert np.array_equal(d.counts, counts) and np.array_equal(d.chain_ids, np.unique(t["chain"].to_numpy()))
            assert np.array_equal(d.to_host().view(np.int64), x.view(np.int64))
    finally:
        for d in got:
            d.free()
