"""Batch means, the long-run covariance, the mean test and the multivariate ESS on the device (libmcmcref_bm.so: k_bm_time /
k_bm_tile / k_bm_mean / k_bm_finish / k_bm_pool / k_bm_pooled, and the main library's covariance, Cholesky factor and solve
through the new call path) against the host definitions -- in bits -- and against the long double reference of
test_batchmeans_refs_cpu, at the smallest shapes at which a path changes: the lane, row and block edges of the tree, both
routes, every layout and alignment, chunking, profiling, and the Cholesky block edges.

The device and the host compile the arithmetic from one text without fused multiply-add, so no tolerance applies between
them.  End to end the gate is test_batchmeans_refs_cpu's 1e-9 relative on its well-conditioned cases.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from test_batchmeans_refs_cpu import (BITS_B, CAL_P, E2E_P, RTOL, ar1, bits, calibration_host, calibration_pairs, check_mean_test,
                                      close, e2e_case, restate_batch_means, spd)

pytestmark = pytest.mark.gpu

SHAPES = tuple((C_, P) for P in (1, 63, 64, 65, 130) for C_ in (1, 3))
CORPUS = Path(__file__).parent / "golden" / "corpus"


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bm():
    from mcmc_ref_hip import batchmeans
    return batchmeans


def draws(seed: int, P: int, C_: int, N: int, dtype=np.float64) -> np.ndarray:
    """[P][C][N]: noise of very different sizes around a large offset, so that an order of summation shows in the bits."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((P, C_, N)) * 10.0 ** rng.integers(-3, 4, (P, 1, 1)) + 7.0).astype(dtype)


class _At:
    """A device address inside a buffer: what DeviceTensor needs of a buffer."""

    def __init__(self, buf, offset: int):
        self.ptr = C.c_void_p(buf.ptr.value + offset)


def same(a: dict, b: dict) -> bool:
    return a["a"] == b["a"] and a["b"] == b["b"] and bits(a["bm"]) == bits(b["bm"]) and bits(a["mu"]) == bits(b["mu"])


def layouts(x: np.ndarray):
    """(name, array or view, layout) of the layouts of one [P][C][N] tensor; every one holds the same draws."""
    P, C_, N = x.shape
    yield "pcn", x, "pcn"
    yield "cnp", np.ascontiguousarray(x.transpose(1, 2, 0)), "cnp"
    padded = np.full((P, C_, N + 5), np.nan, dtype=x.dtype)          # a padded row stride: rows start at odd elements too
    padded[:, :, :N] = x
    yield "padded", padded[:, :, :N], "pcn"
    thin = np.full((P, C_, 2 * N), np.nan, dtype=x.dtype)            # stride_n = 2
    thin[:, :, ::2] = x
    yield "thinned", thin[:, :, ::2], "pcn"
    cpn = np.full((C_, P + 2, N), np.nan, dtype=x.dtype)             # chains outermost, a padded parameter stride
    cpn[:, :P, :] = x.transpose(1, 0, 2)
    yield "cpn", cpn[:, :P, :], "cpn"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("b", BITS_B)
def test_batch_means_in_bits(bm, ctx, b, dtype):
    """Every b at N = 3 b + r0, r0 in {0, 1, b - 1}, over the (C, P) of SHAPES in turn and every layout, against the host
    definition; the first shape of every b also against the numpy restatement."""
    from mcmc_ref_hip._device import DeviceBuffer, DeviceTensor
    i = BITS_B.index(b)
    for j, r0 in enumerate(sorted({0, 1, b - 1})):
        C_, P = SHAPES[(3 * i + j) % len(SHAPES)]
        N = 3 * b + r0
        x = draws(1000 * b + r0, P, C_, N, dtype)
        want = bm.batch_means_host(x, batch=b, r=1)
        if j == 0:
            rb, rm = restate_batch_means(x, "pcn", b)
            assert bits(want["bm"]) == bits(rb) and bits(want["mu"]) == bits(rm), (b, r0)
        for name, y, layout in layouts(x):
            got = bm.batch_means(y, layout, batch=b, r=1, context=ctx)
            assert same(got, want), (b, r0, C_, P, name)
        if C_ == 3:                                              # stride_c = 0: one chain three times
            rep = np.broadcast_to(x[:, :1, :], x.shape)
            assert same(bm.batch_means(rep, batch=b, r=1, context=ctx), bm.batch_means_host(rep, batch=b, r=1)), (b, r0, "rep")
        # the tensor 0 and 8 bytes past a 16-byte boundary, through the entry that takes a device tensor
        for off in (0, 8):
            with DeviceBuffer(ctx, x.nbytes + 16) as buf:
                ctx._check(ctx.lib.mcr_memcpy_h2d(ctx.handle, C.c_void_p(buf.ptr.value + off), x.ctypes.data_as(C.c_void_p), x.nbytes))
                t = DeviceTensor(ctx, _At(buf, off), (0 if dtype == np.float64 else 1, C_, N, P, N, 1, C_ * N))
                assert same(bm.batch_means(t, batch=b, r=1, context=ctx), want), (b, r0, off)


def test_dtype_codes():
    from mcmc_ref_hip import _abi
    assert (_abi.MCR_F64, _abi.MCR_F32) == (0, 1)


def test_alone_chunked_repeated_and_profiled(bm, ctx):
    x = draws(7, 130, 3, 3 * 99 + 5)
    cnp = np.ascontiguousarray(x.transpose(1, 2, 0))
    want = bm.batch_means_host(x, batch=99, r=3)
    whole = bm.batch_means(x, batch=99, r=3, context=ctx)
    assert same(whole, want)
    for p in (0, 64, 129):                                       # a parameter alone, on both routes
        one = bm.batch_means(x[p:p + 1], batch=99, r=3, context=ctx)
        assert bits(one["bm"]) == bits(whole["bm"][p:p + 1]) and bits(one["mu"]) == bits(whole["mu"][p:p + 1]), p
        one = bm.batch_means(cnp[:, :, p:p + 1], "cnp", batch=99, r=3, context=ctx)
        assert bits(one["bm"]) == bits(whole["bm"][p:p + 1]) and bits(one["mu"]) == bits(whole["mu"][p:p + 1]), p
    try:
        bm.set_workspace_limit(40 * 72, context=ctx)             # 9 batch sums = 72 bytes a parameter: 4 chunks of 39
        bm.profile(True, context=ctx)
        for y, layout, ran, idle in ((x, "pcn", "time", "tile"), (cnp, "cnp", "tile", "time")):
            for _ in range(2):
                assert same(bm.batch_means(y, layout, batch=99, r=3, context=ctx), want), layout
                ms = bm.kernel_ms(context=ctx)
                assert ms[ran] > 0 and ms["mean"] > 0 and ms[idle] == 0 and ms["pool"] == 0, (layout, ms)
        bm.set_workspace_limit(64, context=ctx)                  # not even one parameter
        from mcmc_ref_hip._abi import MCR_ENOMEM, McrError
        with pytest.raises(McrError) as exc:
            bm.batch_means(x, batch=99, r=3, context=ctx)
        assert exc.value.code == MCR_ENOMEM and "limit" in exc.value.message
    finally:
        bm.profile(False, context=ctx)
        bm.set_workspace_limit(1 << 30, context=ctx)
    assert same(bm.batch_means(x, batch=99, r=3, context=ctx), want)          # the handle is usable after the error
    assert not any(bm.kernel_ms(context=ctx).values())                        # an untimed call reads 0
    from mcmc_ref_hip._abi import MCR_EINVAL, McrError
    with pytest.raises(McrError) as exc:
        bm.batch_means(x, batch=x.shape[2] + 1, r=1, context=ctx)
    assert exc.value.code == MCR_EINVAL and "outside [1, N" in exc.value.message
    assert same(bm.batch_means(cnp, "cnp", batch=99, r=3, context=ctx), want)


def test_finish_and_pool_in_bits(bm, ctx):
    """k_bm_finish and k_bm_pool against their host forms, with parameters dropped at the first, a middle and the last
    index; k_bm_pooled against the tensor itself."""
    rng = np.random.default_rng(3)
    P = 67
    g = rng.standard_normal((P, 2 * P))
    cb, cb3 = g @ g.T, (g * 1.1) @ g.T
    mur, mua = rng.standard_normal(P), rng.standard_normal(P)
    host = bm._Host()
    with contextlib.ExitStack() as stack:
        dev = bm._Dev(ctx, stack)
        up = lambda a: dev.buf(a.size).upload(a)  # noqa: E731
        for r, b, A, A3 in ((1, 5, 40, 0), (3, 6, 40, 121), (3, 3, 2, 6), (1, 4, 1, 0)):
            got = dev.get(dev.finish(up(cb), up(cb3) if r == 3 else None, P, b, A, A3, r), P * P)
            assert bits(got) == bits(host.finish(cb, cb3 if r == 3 else None, P, b, A, A3, r).ravel()), (r, b, A)
        d_sr, d_sa, d_mur, d_mua = up(cb), up(cb3 + np.eye(P)), up(mur), up(mua)
        for drop in ((), (0,), (33,), (P - 1,), (0, 33, P - 1)):
            scale = rng.uniform(0.5, 2.0, P)
            scale[list(drop)] = 0.0
            for two in (True, False):
                hv, hd, hz, hn = host.pool(cb, mur, 900, cb3 + np.eye(P) if two else None, mua if two else None, 1700, P, scale, 1e-3)
                v, d, z, n = dev.pool(d_sr, d_mur, 900, d_sa if two else None, d_mua if two else None, 1700, P, scale, 1e-3)
                assert n == hn == P - len(drop), drop
                assert bits(dev.get(v, n * n)) == bits(hv.ravel()) and bits(dev.get(d, n)) == bits(hd) and bits(dev.get(z, n)) == bits(hz), (drop, two)
        assert dev.pool(d_sr, d_mur, 9, d_sa, d_mua, 7, P, np.zeros(P), 0.0)[3] == 0
        for dtype in (np.float64, np.float32):
            x = draws(5, 5, 3, 77, dtype)
            for layout in ("pcn", "cnp", "ncp"):
                t = dev.tensor(np.ascontiguousarray(x.transpose(["pcn".index(a) for a in layout])), layout)
                assert bits(dev.get(dev.pooled(t), x.size)) == bits(x.astype(np.float64).ravel()), (dtype, layout)


@pytest.mark.parametrize("P", E2E_P)
def test_end_to_end_against_long_double(bm, ctx, P):
    """mean_shift_test and multi_ess through mcr_covariance_dev, mcrx_cholesky_dev and mcrx_solve_lower_dev: P_live at the
    block edges of the factorisation; one parameter is dropped by its scale."""
    ref, act, scale, b_ref, b_act, want = e2e_case(P)
    got = bm.mean_shift_test(ref, act, scale=scale, r=3, context=ctx, batch_ref=b_ref, batch_act=b_act)
    check_mean_test(got, want, P)
    host = bm.mean_shift_test_host(ref, act, scale=scale, r=3, batch_ref=b_ref, batch_act=b_act)
    assert got["info"] == host["info"] and got["dof"] == host["dof"] and close(got["p_value"], host["p_value"])
    m = bm.multi_ess(np.ascontiguousarray(ref.transpose(1, 2, 0)), "cnp", batch=b_ref, r=3, scale=scale, context=ctx)
    assert m["p_live"] == P and m["info_sigma"] == 0 and m["info_lambda"] == 0 and close(m["mess"], want["mess_ref"])
    mh = bm.multi_ess_host(ref, batch=b_ref, r=3, scale=scale)
    assert np.abs(m["ess_bm"] - mh["ess_bm"]).max() <= RTOL * np.abs(mh["ess_bm"]).max()
    assert np.abs(m["mcse_mean"] - mh["mcse_mean"]).max() <= RTOL * np.abs(mh["mcse_mean"]).max()
    assert bits(m["mu"]) == bits(mh["mu"])


def test_findings_on_the_device(bm, ctx):
    rng = np.random.default_rng(5)
    mix = np.linalg.cholesky(spd(3, 5.0, seed=1))
    x, y = ar1(rng, mix, 4, 60, 0.3), ar1(rng, mix, 5, 48, 0.3)
    t = bm.mean_shift_test(x[:, :1], y, r=1, context=ctx, batch_ref=60, batch_act=4, mess=False)      # A < 2: NaN
    assert t["info"] == 1 and math.isnan(t["T"]) and math.isnan(t["p_value"]) and np.isnan(t["shift"]).all()
    t = bm.mean_shift_test(x, x, r=3, context=ctx, batch_ref=6, batch_act=6, mess=False)
    assert t["info"] == 0 and t["T"] == 0.0 and t["p_value"] == 1.0 and not t["z"].any()
    lr = bm.long_run_covariance(x, batch=6, r=3, context=ctx)
    lh = bm.long_run_covariance_host(x, batch=6, r=3)
    assert lr["info"] == lh["info"] == 0 and bits(lr["mu"]) == bits(lh["mu"])
    assert np.abs(lr["sigma"] - lh["sigma"]).max() <= RTOL * np.abs(lh["sigma"]).max()
    with pytest.raises(ValueError, match="divisible by 3"):
        bm.mean_shift_test(x, y, r=3, context=ctx, batch_ref=10)


def test_calibration_pairs_on_the_device(bm, ctx):
    """The first ten pairs of the CPU calibration give the host's p-values (the counting is the CPU test's)."""
    for i in range(10):
        ref, act, scale = calibration_pairs()[i]
        want = calibration_host(i)
        got = bm.mean_shift_test(ref, act, scale=scale, r=3, context=ctx)
        assert got["info"] == 0 and got["dof"] == CAL_P and close(got["p_value"], want["p_value"]), (i, got["p_value"], want["p_value"])
        assert close(got["mess_ref"], want["mess_ref"]) and close(got["mess_act"], want["mess_act"]), i


def test_validate_mean_shift_on_a_corpus_model(ctx):
    from mcmc_ref_hip.convert import table_to_tensor
    from mcmc_ref_hip.store import DataStore
    from mcmc_ref_hip.validate import validate_mean_shift
    store = DataStore(local_root=CORPUS, packaged_root=CORPUS / "none")
    table = store.open_draws("arma-arma11").read_all()
    params = [c for c in table.column_names if c not in ("chain", "draw")]
    x, counts = table_to_tensor(table, params)
    chains = len(counts)
    same_draws = {p: x[i] for i, p in enumerate(params)}
    res = validate_mean_shift("arma-arma11", same_draws, chains, p_min=0.01, store=store, context=ctx)
    assert res.passed and res.test["T"] == 0.0 and res.p_value == 1.0 and res.test["dof"] == len(params) and not res.failures
    moved = dict(same_draws)
    moved[params[1]] = x[1] + 0.5 * x[1].std()
    res = validate_mean_shift("arma-arma11", moved, chains, p_min=0.01, store=store, context=ctx)
    assert not res.passed and len(res.failures) == 1 and res.failures[0].startswith("mean_shift.p=") and res.failures[0].endswith("< 0.01")
    assert res.p_value < 1e-6 and abs(res.test["z"][params[1]]) > 5 and res.test["singular"] is None
    assert validate_mean_shift("arma-arma11", moved, chains, store=store, context=ctx).passed           # no p_min: information only
    with pytest.raises(ValueError, match="chains of equal length"):
        validate_mean_shift("arma-arma11", same_draws, 7, store=store, context=ctx)
