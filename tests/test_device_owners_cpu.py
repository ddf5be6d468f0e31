"""Who owns the Python layer's device memory, counted: every owner is a context manager whose free() may be called
again, an arena lives as long as its maker or a view holds it, contextlib.ExitStack.pop_all() hands a buffer on alive,
and the records' close() frees exactly their own buffers.  No GPU and no library: the `ctx` here is a fake whose `lib`
has the four memory calls only, backed by a dict."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import pytest

from mcmc_ref_hip import _ffi, convert, parquet


class FakeLib:
    """mcr_dev_alloc / mcr_dev_free / mcr_memcpy_h2d / mcr_memcpy_d2h over a dict {address: bytearray}; `frees` counts
    the frees of every address, `fail_h2d` makes the next uploads answer MCR_ENOMEM."""

    def __init__(self):
        self.live, self.frees, self.next, self.fail_h2d = {}, {}, 4096, False

    def mcr_dev_alloc(self, _handle, nbytes, out):
        out._obj.value = self.next
        self.live[self.next] = bytearray(max(int(nbytes), 1))
        self.next += (max(int(nbytes), 1) + 4095) // 4096 * 4096 + 4096
        return _ffi.MCR_OK

    def mcr_dev_free(self, _handle, ptr):
        self.frees[ptr.value] = self.frees.get(ptr.value, 0) + 1
        del self.live[ptr.value]                                # KeyError: freed twice, or never allocated
        return _ffi.MCR_OK

    def _block(self, addr):
        base = max(a for a in self.live if a <= addr)
        return self.live[base], addr - base

    def mcr_memcpy_h2d(self, _handle, dptr, hptr, nbytes):
        if self.fail_h2d:
            return _ffi.MCR_ENOMEM
        block, off = self._block(dptr.value)
        block[off:off + nbytes] = C.string_at(hptr, nbytes)
        return _ffi.MCR_OK

    def mcr_memcpy_d2h(self, _handle, hptr, dptr, nbytes):
        block, off = self._block(dptr.value)
        C.memmove(hptr, bytes(block[off:off + nbytes]), nbytes)
        return _ffi.MCR_OK

    def mcr_last_error(self, _handle):
        return b"fake: out of memory"


class FakeContext:
    handle = C.c_void_p(1)
    _check = _ffi.Context._check
    upload = _ffi.Context.upload
    upload_sims = _ffi.Context.upload_sims
    ragged_tensor = _ffi.Context.ragged_tensor

    def __init__(self):
        self.lib = FakeLib()


@pytest.fixture()
def ctx():
    c = FakeContext()
    yield c
    assert c.lib.live == {}, "a test left device memory allocated"


def test_with_frees_once_and_free_is_idempotent(ctx):
    with _ffi.DeviceBuffer(ctx, 64) as buf:
        addr = buf.ptr.value
        assert list(ctx.lib.live) == [addr]
        buf.upload(np.arange(8.0))
        assert np.array_equal(buf.download(np.float64, 8), np.arange(8.0))
    assert ctx.lib.live == {} and ctx.lib.frees == {addr: 1}
    buf.free()
    buf.free()
    assert ctx.lib.frees == {addr: 1} and not buf.ptr


@pytest.mark.parametrize("make", [
    lambda ctx: _ffi.DeviceTensor(ctx, _ffi.DeviceBuffer(ctx, 64), (_ffi.MCR_F64, 2, 2, 2, 2, 1, 4)),
    lambda ctx: _ffi.DeviceSims(ctx, _ffi.DeviceBuffer(ctx, 64), (_ffi.MCR_F64, 1, 2, 2, 2, 8, 2, 1, 4)),
    lambda ctx: parquet.DeviceDraws(None, _ffi.DeviceBuffer(ctx, 64), ["a"], np.zeros(1, np.int64), np.full(1, 8)),
    lambda ctx: ctx.upload(np.zeros((2, 2, 2))),
    lambda ctx: ctx.upload_sims(np.zeros((1, 2, 2, 2))),
], ids=["DeviceTensor", "DeviceSims", "DeviceDraws", "Context.upload", "Context.upload_sims"])
def test_every_owner_is_a_context_manager(ctx, make):
    with make(ctx) as owner:
        assert len(ctx.lib.live) == 1
    assert ctx.lib.live == {} and list(ctx.lib.frees.values()) == [1]
    owner.free()
    assert list(ctx.lib.frees.values()) == [1]


def test_an_arena_lives_until_its_last_view_and_its_share_are_freed(ctx):
    with _ffi.DeviceArena(ctx, 256) as arena:
        a, b = arena.view(0, 64), arena.view(64, 64)
        shared = b.share()
        assert shared.ptr.value == b.ptr.value and shared.nbytes == 64
    assert len(ctx.lib.live) == 1                                # the maker let go; three views hold it
    with a:
        pass
    a.free()                                                     # again: harmless, and counts once
    assert len(ctx.lib.live) == 1
    b.free()
    assert len(ctx.lib.live) == 1                                # the share of b still holds it
    shared.free()
    assert ctx.lib.live == {} and list(ctx.lib.frees.values()) == [1]
    arena.free()
    assert list(ctx.lib.frees.values()) == [1]


def test_an_arena_without_views_frees_itself(ctx):
    with _ffi.DeviceArena(ctx, 0) as arena:
        assert len(ctx.lib.live) == 1
    assert ctx.lib.live == {}
    arena = _ffi.DeviceArena(ctx, 32)
    view = arena.view(0, 32)
    view.free()
    assert len(ctx.lib.live) == 1                                # the maker still holds it
    arena.free()
    assert ctx.lib.live == {}


def test_an_arena_whose_maker_fails_goes_with_the_views_of_its_stack(ctx):
    with pytest.raises(RuntimeError):
        with contextlib.ExitStack() as stack, _ffi.DeviceArena(ctx, 64) as arena:
            stack.enter_context(arena.view(0, 32))
            stack.enter_context(arena.view(32, 32))
            raise RuntimeError("after two views")
    assert ctx.lib.live == {} and list(ctx.lib.frees.values()) == [1]


def test_pop_all_hands_a_buffer_out_alive(ctx):
    def make(fail: bool):
        with contextlib.ExitStack() as stack:
            kept = stack.enter_context(_ffi.DeviceBuffer(ctx, 16))
            stack.enter_context(_ffi.DeviceBuffer(ctx, 16)).free()       # scratch, done with before the hand-over
            if fail:
                raise RuntimeError("before the hand-over")
            stack.pop_all()
        return kept

    with pytest.raises(RuntimeError):
        make(True)
    assert ctx.lib.live == {}
    kept = make(False)
    assert list(ctx.lib.live) == [kept.ptr.value]
    kept.upload(np.arange(2.0))
    kept.free()


def test_a_failing_upload_leaves_nothing_allocated(ctx):
    ctx.lib.fail_h2d = True
    with pytest.raises(_ffi.McrError):
        ctx.upload(np.zeros((2, 2, 2)))
    with pytest.raises(_ffi.McrError):
        ctx.upload_sims(np.zeros((1, 2, 2, 2)))
    with pytest.raises(_ffi.McrError):
        convert._upload_draws(ctx, np.zeros((2, 5)), np.array([2, 3]), 2)       # the ragged upload
    with pytest.raises(_ffi.McrError):
        convert._upload_draws(ctx, np.zeros((2, 6)), np.array([3, 3]), 2)
    assert ctx.lib.live == {} and len(ctx.lib.frees) == 4
    ctx.lib.fail_h2d = False
    with convert._upload_draws(ctx, np.zeros((2, 5)), np.array([2, 3]), 2) as t:
        assert t.chain_off.tolist() == [0, 2, 5] and len(ctx.lib.live) == 1


def test_each_record_closes_exactly_its_own_buffers_once(ctx):
    other = _ffi.DeviceBuffer(ctx, 8)                            # somebody else's: no record may touch it
    with _ffi.DeviceArena(ctx, 128) as values, _ffi.DeviceArena(ctx, 128) as ids:
        table = _ffi.CsvTable(["a"], values.view(0, 64), np.zeros(1, bool), (ids.view(0, 64), None), 0, ["chain", "a"])
    names, buf, ints, (chain, draw), hard, header = table       # positional, as every caller unpacks it
    assert table.values is buf and table.ids == (chain, None) and draw is None and hard == 0
    assert len(ctx.lib.live) == 3
    table.close()
    table.close()
    assert list(ctx.lib.live) == [other.ptr.value]

    with _ffi.DeviceArena(ctx, 64) as arena:
        fbuf = arena.view(0, 64)
    rec = convert.CsvDraws(parquet.DeviceDraws(None, fbuf.share(), ["a"], np.zeros(1, np.int64), np.full(1, 8)), fbuf, [False],
                           ["a"], (None, None))
    d, file_order, int_columns, header, got_ids = rec
    assert rec.draws is d and rec.file_order is file_order and rec[:3] == (d, fbuf, [False])
    assert len(ctx.lib.live) == 2
    rec.close()
    rec.close()
    assert list(ctx.lib.live) == [other.ptr.value]

    class Image:
        closed = 0

        def close(self):
            self.closed += 1

    image = Image()
    entry = convert._Prepared(["a"], 1, 8, np.full(1, 8), image=image, tensor=ctx.upload(np.zeros((1, 1, 8))))
    assert len(ctx.lib.live) == 2
    entry.close()
    entry.close()
    assert list(ctx.lib.live) == [other.ptr.value] and image.closed == 2        # (an image's close() is idempotent itself)
    convert._Prepared([], 0, 0, np.zeros(0), table=object(), x=np.zeros((0, 0))).close()     # a host job owns nothing
    other.free()
    assert sorted(ctx.lib.frees.values()) == [1] * len(ctx.lib.frees)
