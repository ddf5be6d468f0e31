"""Strided and non-contiguous draw tensors on every summarize path.

The C ABI takes any element strides (stride_c, stride_n, stride_p) (include/mcmcref_hip.h, "Conventions").  After
ingest the pipeline sees the same f64 [P][M] data whatever the layout, so every view must give the SAME BITS as the
contiguous [P][C][N] call on the same data and dtype -- every field, q_lo and the truncation lags included -- on the
host path, `summarize_dev`, `enqueue` / `wait_one` and `summarize_models`, and agree with `oracle.summarize` on the view
itself (the oracle reads strides: tests/test_strides_cpu.py).  No shape here reaches the FFT tier (N <= 16384), whose
pair assignment depends on how parameters share a chunk.

What decides the path (mcr_api.hip): `plan_chunks` consumes [P][C][N] in place (ignoring the stride of an axis of
length 1); everything else is ingested chunk by chunk into X[P][M] f64 by `k_ingest_transpose` (stride_p == 1,
stride_n != 1, more than one parameter in the chunk) or `k_ingest_rows` (anything else), each reading parameter
p0 + p of chunk p0.  `mcr_moments_dev` uses `k_moments_rows` for row-contiguous views (stride_n == 1, stride_c == N;
pstride = stride_p) and `k_moments_cols` for every other view.  `mcr_summarize` uploads parameter-separable host
tensors of at least 8 MB in pieces.
"""
from __future__ import annotations

import ctypes
import math
from contextlib import contextmanager

import numpy as np
import pytest

from test_hip_parity import check_summary
from test_strides_cpu import contiguous_pcn, natural, random_draws, strided, view_cases

pytestmark = pytest.mark.gpu

KEYS = ("mean", "std", "median", "rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "lag_bulk", "lag_tail",
        "q", "q_lo")
DTYPES = [np.float64, np.float32]
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


class _At:
    """What a DeviceTensor reads of its buffer: the address of the view's first element."""

    def __init__(self, ptr: int):
        self.ptr = ctypes.c_void_p(ptr)


@contextmanager
def on_device(ctx, view: np.ndarray, layout: str, base: np.ndarray):
    """The view as a DeviceTensor: its base uploaded whole, the view's byte offset added to the address, its strides
    passed as they are."""
    from mcmc_ref_hip import _ffi
    off = view.__array_interface__["data"][0] - base.ctypes.data
    assert 0 <= off < base.nbytes and off % base.itemsize == 0
    buf = _ffi.DeviceBuffer(ctx, base.nbytes).upload(base)
    try:
        yield _ffi.DeviceTensor(ctx, _At(buf.ptr.value + off), _ffi.tensor_args(view, layout))
    finally:
        buf.free()


def assert_same_bits(got: dict, ref: dict, what):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k)


def contiguous_call(ctx, view, layout):
    return ctx.summarize(contiguous_pcn(view, layout), "pcn", min_chains=1)


STATS = ("mean", "std", "median", "q")


def check_oracle(got: dict, oracle, view, layout, params, what, keys=None):
    """check_summary on the parameters `params` of the view (the oracle reads the view's strides); keys: only these
    fields (the others as the oracle has them)."""
    params = sorted(set(params))
    sub = np.take(view, params, axis=layout.index("p"))
    exp = oracle.summarize(sub, layout, min_chains=1)
    mine = {k: got[k][params] for k in KEYS if k != "q_lo"}
    if keys is not None:
        mine = {k: (mine[k] if k in keys else exp[k]) for k in mine}
    check_summary(mine, exp, what=what)


def find_chunk_limit(ctx, t, P: int) -> int:
    """Lowers the workspace limit until a call on t is cut into >= 3 chunks with a remainder; returns the chunk size
    (the caller restores the limit)."""
    limit = 1 << 30
    while True:
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, limit))
        per_chunk = ctx.params_per_chunk(t)
        if -(-P // per_chunk) >= 3 and P % per_chunk:
            return per_chunk
        limit //= 2
        assert limit >= 1 << 16, per_chunk


# ---------------------------------------------------------------------------------------------------------------------
# every view: host pointer and device pointer give the contiguous bits and the oracle's values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_view_gives_the_contiguous_bits(ctx, oracle, dtype):
    C, N, P = 4, 300, 6
    x = random_draws(P, C, N, seed=21)
    for name, layout, strides, offset in view_cases(C, N, P):
        v, base = strided(x, layout, strides, offset, dtype)
        ref = contiguous_call(ctx, v, layout)
        got = ctx.summarize(v, layout, min_chains=1)
        assert_same_bits(got, ref, ("host", name))
        with on_device(ctx, v, layout, base) as t:
            assert_same_bits(ctx.summarize(t, min_chains=1), ref, ("dev", name))
        # every chain of the stride_n == 0 view is constant: its diagnostics differ from the oracle's whatever the
        # layout (test_constant_chains_of_distinct_values_vs_oracle); the bits above pin them to the contiguous call
        check_oracle(got, oracle, v, layout, range(P), name, keys=STATS if strides[1] == 0 else None)


@pytest.mark.xfail(strict=True, reason="constant half-chains get a within-chain variance of exactly 0 (rhat = inf); "
                                       "the reference's _variance of equal values is a rounding residue (finite rhat)")
def test_constant_chains_of_distinct_values_vs_oracle(ctx, oracle):
    """Known discrepancy, not a stride effect (the contiguous tensor shows it): every chain constant, the chains at
    different values.  The kernels detect constant half-chains on the rank codes and take their variance as 0, so
    split-R-hat is inf.  The reference's `_variance` sums the half's equal z values left to right, and for a half of
    150 draws sum / n is in general not the value itself: the within variance is a residue of ~1e-33 and R-hat a
    finite ~1e14 (test_constant_halves_of_a_chain_that_is_not_constant holds halves short enough for an exact sum)."""
    C, N, P = 4, 300, 6
    x = np.broadcast_to(random_draws(P, C, 1, seed=21), (P, C, N))
    x = np.ascontiguousarray(x)
    check_summary(ctx.summarize(x, "pcn", min_chains=1), oracle.summarize(x, "pcn", min_chains=1), what="constant chains")


def test_rolling_window_and_models_of_mixed_layouts(ctx):
    """enqueue / wait_one with up to MCR_MAX_INFLIGHT calls of different layouts, dtypes and shapes outstanding, and one
    summarize_models call with every model in a different layout."""
    from mcmc_ref_hip import _ffi
    views = []
    for k, (C, N, P) in enumerate(((4, 300, 6), (3, 129, 70), (5, 64, 2))):
        x = random_draws(P, C, N, seed=30 + k)
        for dtype in DTYPES:
            for name, layout, strides, offset in view_cases(C, N, P):
                v, base = strided(x, layout, strides, offset, dtype)
                views.append(((C, N, P, np.dtype(dtype).name, name), v, layout, base, contiguous_call(ctx, v, layout)))
    rng = np.random.default_rng(5)
    order = rng.permutation(len(views))
    bufs = [on_device(ctx, v, layout, base) for _, v, layout, base, _ in views]
    ts = [b.__enter__() for b in bufs]
    try:
        delivered = []
        for i in order:
            if ctx.inflight >= _ffi.MCR_MAX_INFLIGHT:
                delivered.append(ctx.wait_one())
            ctx.enqueue(ts[i], min_chains=1)
        while ctx.inflight:
            delivered.append(ctx.wait_one())
        assert len(delivered) == len(views) and ctx.wait_one() is None
        for i, b in zip(order, delivered):
            assert_same_bits(b.result(), views[i][4], ("rolling", views[i][0]))
        pick = order[:24]
        outs = ctx.summarize_models([ts[i] for i in pick], min_chains=1)
        for i, r in zip(pick, outs):
            assert_same_bits(r, views[i][4], ("models", views[i][0]))
    finally:
        for b in bufs:
            b.__exit__(None, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# ingest tile edges (64 x 64 transpose tiles, 256-draw rows) and the in-place shortcuts
# ---------------------------------------------------------------------------------------------------------------------
def ingest_views(kernel: str, C: int, N: int, P: int, alt: int):
    """A layout that goes through k_ingest_transpose (stride_p == 1, stride_n != 1) or k_ingest_rows."""
    if kernel == "transpose":
        return ("cnp", natural("cnp", C, N, P)) if alt % 2 == 0 else ("ncp", natural("ncp", C, N, P, gap={"c": 1}))
    return ("pcn", natural("pcn", C, N, P, gap={"n": 3}, step=2)) if alt % 2 == 0 else \
        ("pnc", natural("pnc", C, N, P, gap={"n": 7}))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ingest_tile_edges(ctx, oracle, dtype):
    NS = (1, 2, 63, 64, 65, 255, 257, 4097)
    PS = (1, 2, 63, 64, 65, 130)
    CS = (1, 2, 4, 7)
    for i, N in enumerate(NS):
        for j, P in enumerate(PS):
            C = CS[(i + j) % len(CS)]
            x = random_draws(P, C, N, seed=100 * i + j)
            ref = None
            for kernel in ("transpose", "rows"):
                layout, strides = ingest_views(kernel, C, N, P, i + j)
                v, _ = strided(x, layout, strides, 0, dtype)
                if ref is None:
                    ref = contiguous_call(ctx, v, layout)
                got = ctx.summarize(v, layout, min_chains=1)
                assert_same_bits(got, ref, (kernel, layout, C, N, P))
                if (i + j) % 3 == 0:
                    check_oracle(got, oracle, v, layout, (0, P // 2, P - 1), (kernel, layout, C, N, P))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmax_chains(ctx, oracle, dtype):
    C, N, P = 256, 65, 65
    x = random_draws(P, C, N, seed=256)
    ref = None
    for kernel in ("transpose", "rows"):
        layout, strides = ingest_views(kernel, C, N, P, 0)
        v, base = strided(x, layout, strides, 0, dtype)
        if ref is None:
            ref = contiguous_call(ctx, v, layout)
        got = ctx.summarize(v, layout, min_chains=1)
        assert_same_bits(got, ref, (kernel, C))
        with on_device(ctx, v, layout, base) as t:
            assert_same_bits(ctx.summarize(t, min_chains=1), ref, ("dev", kernel, C))
        check_oracle(got, oracle, v, layout, (0, 63, 64), (kernel, C))


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_shortcuts_ignore_the_stride_of_a_unit_axis(ctx, oracle, dtype):
    """plan_chunks reads [P][C][N] in place and skips the stride test of an axis of length 1."""
    cases = [
        ((3, 8, 1), (1, 7, 8)),             # N == 1, stride_n != 1
        ((3, 1, 500), (999, 1, 500)),       # C == 1, stride_c != N
        ((1, 4, 300), (300, 1, 12345)),     # P == 1, any stride_p
        ((1, 4, 300), (300, 1, 0)),
    ]
    for (P, C, N), strides in cases:
        x = random_draws(P, C, N, seed=P * 1000 + C * 10 + N)
        v, base = strided(x, "pcn", strides, 0, dtype)
        ref = contiguous_call(ctx, v, "pcn")
        got = ctx.summarize(v, "pcn", min_chains=1)
        assert_same_bits(got, ref, ("host", (P, C, N), strides))
        with on_device(ctx, v, "pcn", base) as t:
            assert_same_bits(ctx.summarize(t, min_chains=1), ref, ("dev", (P, C, N), strides))
        check_oracle(got, oracle, v, "pcn", range(P), ((P, C, N), strides))


# ---------------------------------------------------------------------------------------------------------------------
# chunk edges: parameter p0 + p of chunk p0 (k_ingest_* with p0 > 0)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["transpose", "rows"])
def test_chunked_views_at_every_chunk_edge(ctx, oracle, kernel, dtype):
    C, N, P = 4, 1000, 37
    x = random_draws(P, C, N, seed=37)
    layout, strides = ingest_views(kernel, C, N, P, 0)
    v, base = strided(x, layout, strides, 0, dtype)
    ref = contiguous_call(ctx, v, layout)
    with on_device(ctx, v, layout, base) as t:
        whole = ctx.summarize(t, min_chains=1)
        assert_same_bits(whole, ref, "unchunked")
        try:
            n = find_chunk_limit(ctx, t, P)
            chunked_dev = ctx.summarize(t, min_chains=1)
            chunked_host = ctx.summarize(v, layout, min_chains=1)
        finally:
            ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 8 << 30))
    assert_same_bits(chunked_dev, whole, ("dev", n))
    assert_same_bits(chunked_host, whole, ("host", n))
    edges = [p for k in range(n, P, n) for p in (k - 1, k)]
    check_oracle(chunked_dev, oracle, v, layout, [0, P - 1] + edges, (kernel, "chunks of", n))


# ---------------------------------------------------------------------------------------------------------------------
# host piece upload (separable tensors of >= 8 MB)
# ---------------------------------------------------------------------------------------------------------------------
def test_host_piece_upload_of_padded_views(ctx, oracle):
    C, N, P = 4, 10000, 30
    x = random_draws(P, C, N, seed=8)
    for layout, strides in (("pcn", natural("pcn", C, N, P, gap={"c": 5})),       # stride_p > C*N
                            ("pnc", natural("pnc", C, N, P))):
        v, base = strided(x, layout, strides, 0, np.float64)
        assert (P - 1) * strides[2] * 8 >= 8 << 20
        got = ctx.summarize(v, layout)
        with on_device(ctx, v, layout, base) as t:
            dev = ctx.summarize(t)
        assert_same_bits(got, dev, (layout, "pieces vs device"))
        assert_same_bits(got, ctx.summarize(contiguous_pcn(v, layout), "pcn"), (layout, "pieces vs contiguous"))
        check_oracle(got, oracle, v, layout, (0, P - 1), (layout, "pieces"))


# ---------------------------------------------------------------------------------------------------------------------
# mcr_moments_dev against an exactly rounded reference
# ---------------------------------------------------------------------------------------------------------------------
def moment_slice_starts(M: int, P: int, es: int, rows: bool) -> list[int]:
    """First pooled draw of every slice of k_moments_rows / k_moments_cols (mcr_moments_dev's choice of S)."""
    if rows:
        vec = 16 // es
        S = max(1, min(-(-4096 // P), -(-M // (256 * vec * 4))))
        per = -(-M // S)
        per = -(-per // vec) * vec
    else:
        S = max(1, min(-(-2048 // -(-P // 64)), -(-M // 64), 65535))
        per = -(-M // S)
    return list(range(0, M, per))


def exact_moments(x_pcn: np.ndarray):
    """Per parameter: the mean rounded once from its exact value (math.fsum), and sqrt(fsum((x - mean)^2) / M)."""
    P = x_pcn.shape[0]
    mean, std = np.empty(P), np.empty(P)
    for p in range(P):
        v = x_pcn[p].reshape(-1).astype(np.float64)
        m0 = math.fsum(v) / v.size
        m = m0 + math.fsum(v - m0) / v.size
        mean[p] = m
        std[p] = math.sqrt(math.fsum((v - m) ** 2) / v.size)
    return mean, std


def assert_moments(mean, std, ref_mean, ref_std, what, k: float = 1.0):
    """Within the rounding of the mean itself (one ulp of |mean| on either side) plus a few ulp of the spread: the
    streaming kernels' bound (mcr_kernels.hpp, above k_moments_rows), however far the mean lies from the spread."""
    for p in range(len(ref_mean)):
        tol_m = k * (2 * np.spacing(abs(ref_mean[p])) + 16 * EPS * ref_std[p])
        assert abs(mean[p] - ref_mean[p]) <= tol_m, (what, p, "mean", mean[p], ref_mean[p])
        assert abs(std[p] - ref_std[p]) <= k * 16 * EPS * ref_std[p], (what, p, "std", std[p], ref_std[p])


@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_of_row_and_column_views(ctx, dtype):
    """Mean 1e6, spread 1, and an outlying draw (+20) at the start of every slice of both kernels, P around 64."""
    C, N, P = 4, 1000, 65
    M = C * N
    rng = np.random.default_rng(64)
    x = 1e6 + rng.normal(size=(P, C, N))
    starts = set()
    for es in (4, 8):
        for rows in (True, False):
            starts.update(moment_slice_starts(M, P, es, rows))
    for r in starts:
        x[:, r // N, r % N] = 1e6 + 20.0
    x = x.astype(dtype)
    ref_mean, ref_std = exact_moments(x)
    views = [  # (name, layout, strides, offset, row-contiguous)
        ("pcn", "pcn", natural("pcn", C, N, P), 0, True),
        ("pcn padded params", "pcn", natural("pcn", C, N, P, gap={"c": 3}), 0, True),
        ("pcn offset 1", "pcn", natural("pcn", C, N, P), 1, True),
        ("pcn offset 3 padded params", "pcn", natural("pcn", C, N, P, gap={"c": 1}), 3, True),
        ("cnp", "cnp", natural("cnp", C, N, P), 0, False),
        ("npc", "npc", natural("npc", C, N, P), 0, False),
        ("cpn", "cpn", natural("cpn", C, N, P), 0, False),
        ("pcn padded chains", "pcn", natural("pcn", C, N, P, gap={"n": 5}), 0, False),
        ("cnp param subset", "cnp", (N * (2 * P + 1), 2 * P + 1, 2), 1, False),
    ]
    got = {}
    for name, layout, strides, offset, rows in views:
        assert rows == (strides[1] == 1 and strides[0] == N), name
        v, base = strided(x, layout, strides, offset, dtype)
        with on_device(ctx, v, layout, base) as t:
            got[name] = ctx.moments(t)
        assert_moments(*got[name], ref_mean, ref_std, name)
    for name in got:
        assert_moments(*got[name], *got["pcn"], (name, "vs pcn"), k=2.0)


# ---------------------------------------------------------------------------------------------------------------------
# element offsets past 2^31
# ---------------------------------------------------------------------------------------------------------------------
def test_element_offsets_past_2_31(ctx, oracle):
    """Two blocks of f32 draws 2^31 + 64 elements apart in one 8.6 GB allocation, read as
      (a) [P][C][N] with stride_p = 2^31 + 64: k_ingest_rows, and k_moments_rows with pstride = stride_p;
      (b) C = 2 chains with stride_c = 2^31 + 64 over [N][P] blocks: k_ingest_transpose and k_moments_cols.
    Every index of those kernels is a 64-bit product; a 32-bit one would read the wrong block or fault."""
    from mcmc_ref_hip import _ffi
    S = (1 << 31) + 64
    C, N, P = 4, 1000, 2
    rng = np.random.default_rng(31)
    blocks = [(rng.normal(size=C * N) * (1 + k) + 3 * k).astype(np.float32) for k in range(2)]
    buf = _ffi.DeviceBuffer(ctx, (S + C * N) * 4)
    try:
        for k, b in enumerate(blocks):
            ctx._check(ctx.lib.mcr_memcpy_h2d(ctx.handle, ctypes.c_void_p(buf.ptr.value + k * S * 4),
                                              b.ctypes.data_as(ctypes.c_void_p), b.nbytes))
        at = _At(buf.ptr.value)
        a = _ffi.DeviceTensor(ctx, at, (_ffi.MCR_F32, C, N, P, N, 1, S))
        a_host = np.stack([b.reshape(C, N) for b in blocks])                       # [P][C][N]
        b_t = _ffi.DeviceTensor(ctx, at, (_ffi.MCR_F32, 2, C * N // 4, 4, S, 4, 1))
        b_host = np.stack([b.reshape(C * N // 4, 4) for b in blocks])              # [C][N][P]
        for what, t, host, layout in (("a", a, a_host, "pcn"), ("b", b_t, b_host, "cnp")):
            got = ctx.summarize(t, min_chains=1)
            ref = contiguous_call(ctx, host, layout)
            assert_same_bits(got, ref, what)
            P_ = host.shape[layout.index("p")]
            check_oracle(got, oracle, host, layout, range(P_), what)
            mean, std = ctx.moments(t)
            assert_moments(mean, std, *exact_moments(contiguous_pcn(host, layout)), what)
    finally:
        buf.free()
