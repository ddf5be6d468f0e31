"""The Stan-convention diagnostics on the device (libmcmcref_std.so: the summary pipeline on the kept draws, k_mcs_series,
k_mcs_walk) against the host definition mcs_diagnostics_host, at the smallest shapes at which a path changes: the case list
of test_std_refs_cpu, the edges of the first lag block and of the 512-draw blocks, walks that leave the first block, the
LDS / global switch of the walk kernel, odd N, every layout and dtype route, chunking and batching, and the main library's
summarize before and after on one device.

Tolerances: device and host run the same sums in the same order but differ in the inverse normal CDF, log10 and sqrt by an
ulp or two, so they are held to 1e-9 relative (the project's gate), not to bits; the lags must be equal, and every case's
margin -- how far the bulk walk's decisions were from a tie -- is at least 1e-7, far above those differences.  Between
the device's own routes no tolerance applies: the bits are equal.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import math

import numpy as np
import pytest

import std_cases as sc

pytestmark = pytest.mark.gpu

EXTRA = [(2, 1022, (("iid", 501), ("ar0.9", 502), ("ties", 503))),          # N = 2 * 512 - 2 (+ 2 is on the case list)
         (4, 2000, (("ar0.99", 504), ("shifted", 505), ("ar0.9", 506)))]    # walks that leave the first block of lags
SHAPES = sc.shapes() + EXTRA


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std():
    from mcmc_ref_hip import standard
    return standard


@functools.lru_cache(maxsize=None)
def host_of(C_: int, N: int, cases: tuple) -> dict:
    from mcmc_ref_hip import standard
    return standard.diagnostics_host(sc.tensor_of(C_, N, cases), basic=True)


def agree(got: dict, want: dict, where) -> None:
    """The device's answers [P] against the host's."""
    for p in range(len(want["rhat"])):
        sc.same(sc.at(got, p), sc.at(want, p), (where, p))
        m = float(want["margin"][p])
        if not math.isnan(m):
            assert m >= sc.MARGIN_MIN and sc.close(float(got["margin"][p]), m, 1e-6), (where, p, m)
        else:
            assert math.isnan(got["margin"][p]), (where, p)


@pytest.mark.parametrize("C_,N,cases", SHAPES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_device_matches_the_host(std, ctx, C_, N, cases):
    x = sc.tensor_of(C_, N, cases)
    want = host_of(C_, N, cases)
    got = std.diagnostics(x, "pcn", basic=True, context=ctx)
    agree(got, want, (C_, N))
    if (C_, N) == (4, 2000):
        assert want["lag_bulk"][0] > 256 and want["lag_bulk"][1] >= 1000 - 6 and want["lag_mean"][0] > 256


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 40])
def test_edge_rules_on_the_device(std, ctx, N):
    rng = np.random.default_rng(N)
    x = np.stack([rng.standard_normal((3, N)), np.full((3, N), 0.1), (rng.random((3, N)) < 0.5) * 1.0])
    want = std.diagnostics_host(x, basic=True)
    got = std.diagnostics(x, "pcn", basic=True, context=ctx)
    for p in range(3):
        sc.same(sc.at(got, p), sc.at(want, p), (N, p))
    assert all(math.isnan(got[k][1]) for k in sc.DOUBLES) and all(got[k][1] == -1 for k in sc.LAGS)
    if N < 8:
        assert all(np.isnan(got[k]).all() for k in ("ess_bulk", "ess_tail", "ess_mean")) and (got["lag_bulk"] == -1).all()
    else:
        assert math.isnan(got["ess_q95"][2]) and not math.isnan(got["ess_q05"][2]) and not math.isnan(got["ess_bulk"][0])


@pytest.mark.parametrize("delta", [0, 1])
def test_lds_global_switch(std, ctx, delta):
    from mcmc_ref_hip import _sabi
    n = _sabi.MCS_LDS_DRAWS + delta
    x = np.random.default_rng(n).standard_normal((2, 1, 2 * n))
    x[1] = np.round(x[1], 2)
    agree(std.diagnostics(x, "pcn", basic=True, context=ctx), std.diagnostics_host(x, basic=True), n)


def test_many_parameters(std, ctx):
    x = np.random.default_rng(65).standard_normal((65, 2, 34))
    agree(std.diagnostics(x, "pcn", basic=True, context=ctx), std.diagnostics_host(x, basic=True), 65)


# ---- the same bits on every route ------------------------------------------------------------------------------------------

def limit_for(std, ctx, C_: int, N: int, P: int, chunk: int) -> int:
    """The smallest workspace limit under which a call of this shape takes `chunk` parameters at a time."""
    def per(nbytes: int) -> int:
        std.set_workspace_limit(nbytes, ctx)
        try:
            return std.params_per_chunk(C_, N, P, basic=True, strides=(N * P, P, 1), context=ctx)
        except Exception:                                           # one parameter does not fit yet
            return 0
    lo, hi = 1, 1 << 30
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if per(mid) >= chunk else (mid, hi)
    assert per(hi) == chunk
    return hi


@pytest.mark.parametrize("N", [200, 201])
def test_same_bits_on_every_route(std, ctx, N):
    P, C_ = 9, 3
    rng = np.random.default_rng(N)
    x = np.stack([sc.ar1(rng, C_, N, phi) for phi in (0.0, 0.5, 0.9, -0.5, 0.0, 0.7, 0.3, 0.95, 0.0)])
    x[4] = np.round(x[4], 1)
    x = x.astype(np.float32).astype(np.float64)                    # representable in f32: the f32 routes see the same draws
    base = std.diagnostics(x, "pcn", basic=True, context=ctx)      # even N: in place
    agree(base, std.diagnostics_host(x, basic=True), N)
    want = sc.bits(base)

    def check(got, where):
        assert sc.bits(got) == want, where

    for p in range(P):                                              # alone against its place in the batch
        one = std.diagnostics(x[p:p + 1], "pcn", basic=True, context=ctx)
        assert sc.bits(one) == sc.bits({k: v[p:p + 1] for k, v in base.items()}), p
    rev = std.diagnostics(x[::-1].copy(), "pcn", basic=True, context=ctx)
    check({k: v[::-1] for k, v in rev.items()}, "reversed")
    cnp = np.ascontiguousarray(x.transpose(1, 2, 0))
    check(std.diagnostics(cnp, "cnp", basic=True, context=ctx), "cnp")
    check(std.diagnostics(np.ascontiguousarray(x.transpose(2, 0, 1)), "npc", basic=True, context=ctx), "npc")
    wide = np.zeros((P, C_, 2 * N))
    wide[:, :, ::2] = x
    check(std.diagnostics(wide[:, :, ::2], "pcn", basic=True, context=ctx), "strided view")
    pad = np.zeros((C_, N, P + 2))
    pad[:, :, :P] = cnp
    check(std.diagnostics(pad[:, :, :P], "cnp", basic=True, context=ctx), "padded cnp")
    check(std.diagnostics(x.astype(np.float32), "pcn", basic=True, context=ctx), "f32 pcn")
    check(std.diagnostics(cnp.astype(np.float32), "cnp", basic=True, context=ctx), "f32 cnp")
    with ctx.upload(x, "pcn") as t:                                 # the device entry on a tensor of the context's
        check(std.diagnostics(t, basic=True, context=ctx), "device pcn")
    with ctx.upload(cnp.astype(np.float32), "cnp") as t:
        check(std.diagnostics(t, basic=True, context=ctx), "device f32 cnp")
    plain = std.diagnostics(x, "pcn", context=ctx)                  # without the raw series: the other outputs keep their bits
    assert sc.bits(plain) == {k: want[k] for k in plain} and not set(plain) & set(std.BASIC_OUTPUTS)
    try:
        for chunk in (1, 4):
            std.set_workspace_limit(limit_for(std, ctx, C_, N, P, chunk), ctx)
            check(std.diagnostics(cnp, "cnp", basic=True, context=ctx), ("chunks of", chunk, "cnp"))
            check(std.diagnostics(x, "pcn", basic=True, context=ctx), ("chunks of", chunk, "pcn"))
    finally:
        std.set_workspace_limit(1 << 30, ctx)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_usable(std, ctx):
    from mcmc_ref_hip import _ffi
    x = sc.tensor_of(2, 16, (("iid", 1), ("ar0.9", 2)))
    base = std.diagnostics(x, "pcn", basic=True, context=ctx)
    h = std._handle(ctx)
    ptr, none = np.ascontiguousarray(x).ctypes.data_as(C.c_void_p), [None] * 15
    #            dtype C  N   P  sc  sn sp  flags
    for args, cause in (((7, 2, 16, 2, 16, 1, 32, 0), "dtype"),
                        ((0, 0, 16, 2, 16, 1, 32, 0), ">= 1"),
                        ((0, 2, 16, 0, 16, 1, 32, 0), ">= 1"),
                        ((0, 2, 1, 2, 1, 1, 2, 0), "N >= 2"),
                        ((0, 2, (1 << 20) + 1, 2, 16, 1, 32, 0), "MCS_MAX_DRAWS"),
                        ((0, 4096, 1 << 19, 2, 16, 1, 32, 0), "2^31"),
                        ((0, 2, 16, 2, -16, 1, 32, 0), "stride"),
                        ((0, 2, 16, 2, 16, -1, 32, 0), "stride"),
                        ((0, 2, 16, 2, 16, 1, -32, 0), "stride"),
                        ((0, 2, 16, 2, 16, 1, 32, 2), "MCS_WANT_BASIC")):
        for entry in (h.lib.mcs_diagnostics, h.lib.mcs_diagnostics_dev):
            assert entry(h.handle, ptr, *args, *none) == _ffi.MCR_EINVAL, cause
            assert cause in h.lib.mcs_last_error(h.handle).decode(), (cause, h.lib.mcs_last_error(h.handle))
    assert h.lib.mcs_diagnostics(h.handle, None, 0, 2, 16, 2, 16, 1, 32, 0, *none) == _ffi.MCR_EINVAL
    assert "NULL" in h.lib.mcs_last_error(h.handle).decode()
    assert h.lib.mcs_diagnostics(None, ptr, 0, 2, 16, 2, 16, 1, 32, 0, *none) == _ffi.MCR_EINVAL
    assert h.lib.mcs_set_workspace_limit(h.handle, 0) == _ffi.MCR_EINVAL
    assert h.lib.mcs_kernel_ms(h.handle, None, 3) == _ffi.MCR_EINVAL
    try:
        std.set_workspace_limit(64, ctx)
        with pytest.raises(_ffi.McrError, match="workspace") as e:
            std.diagnostics(x, "pcn", context=ctx)
        assert e.value.code == _ffi.MCR_ENOMEM
    finally:
        std.set_workspace_limit(1 << 30, ctx)
    bad = x.copy()
    bad[1, 0, 3] = math.nan
    with pytest.raises(_ffi.McrError, match="non-finite") as e:
        std.diagnostics(bad, "pcn", context=ctx)
    assert e.value.code == _ffi.MCR_ENONFINITE
    assert sc.bits(std.diagnostics(x, "pcn", basic=True, context=ctx)) == sc.bits(base)


# ---- beside the main library ---------------------------------------------------------------------------------------------------

def test_call_order_with_summarize(std, ctx):
    """summarize of the main library before and after on the same device and tensor: both give the bits of a fresh state."""
    from mcmc_ref_hip import _ffi
    x = sc.tensor_of(4, 2000, EXTRA[1][2])
    with _ffi.Context(0) as fresh:                                  # a context that has run nothing, and its own mcs handle
        d_first = sc.bits(std.diagnostics(x, "pcn", basic=True, context=fresh))
        s_after = sc.bits(fresh.summarize(x, "pcn"))
    with _ffi.Context(0) as fresh:
        s_first = sc.bits(fresh.summarize(x, "pcn"))
    assert s_first == s_after
    with ctx.upload(x, "pcn") as t:
        for _ in range(2):
            assert sc.bits(ctx.summarize(t)) == s_first
            assert sc.bits(std.diagnostics(t, basic=True, context=ctx)) == d_first
        assert sc.bits(ctx.summarize(t)) == s_first


def test_python_layer_and_command(std, ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli
    x = sc.tensor_of(4, 2000, EXTRA[1][2])[:2, :, :120]
    std.profile(True, ctx)
    try:
        r = std.diagnostics(x, "pcn", basic=True, context=ctx)
        ms = std.kernel_ms(ctx)
        assert set(ms) == {"pipe", "series", "walk"} and all(0.0 < v < 1000.0 for v in ms.values())
    finally:
        std.profile(False, ctx)
    std.diagnostics(x, "pcn", context=ctx)
    assert set(std.kernel_ms(ctx).values()) == {0.0}                # the last call was not timed
    path = tmp_path / "draws.csv"
    rows = ["chain,draw,mu,tau"] + [f"{c},{t},{float(x[0, c, t])!r},{float(x[1, c, t])!r}" for c in range(4) for t in range(120)]
    path.write_text("\n".join(rows) + "\n")
    res = CliRunner().invoke(cli.main, ["std-diagnostics", str(path), "--basic", "--json"])
    assert res.exit_code == 0, res.output
    out = json.loads(res.output)
    for i, name in enumerate(("mu", "tau")):
        assert out[name] == {k: float(v[i]) for k, v in r.items()}
    res = CliRunner().invoke(cli.main, ["std-diagnostics", str(path), "--params", "tau"])
    assert res.exit_code == 0 and "ess_bulk" in res.output and "tau" in res.output and "ess_mean" not in res.output
    assert std.diagnostics_file(path, params=["mu"], context=ctx)["mu"]["rhat"] == r["rhat"][0]
