"""Simulation-based calibration on the GPU (mcr_sbc_ranks, mcr_sbc_ranks_dev; mcr_sbc.hpp).

* The counts EQUAL and mean / sd equal in BITS to the host routine mcr_sbc_ranks_host (tests/test_sbc_refs_cpu.py holds
  that one to numpy and to long-double references): at both sides of every wave (64), pair-row (128), block (1024) and
  register-path (4096) edge of the row length, with 1, 7 and 9 parameters and 1, 5 and 33 simulations (four rows per
  workgroup: every remainder), odd L (every other row off a 16-byte boundary), a device tensor one double off.
* One answer on every route: the tensor read in place ("spcn"), the ingest copy ("scnp", "cspn", a thinned view), f32
  against the widened f64, the host and the device entry, any workspace chunking.
* Only the intended kernels run; errors leave the context usable and the outputs as stated; empty shapes.
* The conjugate-normal model, sbc_files and the command end to end on the device.
"""
from __future__ import annotations

import ctypes as C
import json
import types

import numpy as np
import pytest

from test_sbc_refs_cpu import check_against_references, check_conjugate, edge_sample, write_simulations

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049, 4097]
BATCHES = [(1, 1), (5, 7), (33, 9)]                            # (S, P)
KEYS = ("n_less", "n_equal", "mean", "sd")


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sbc_mod():
    from mcmc_ref_hip import sbc
    return sbc


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()


def bits(r: dict) -> dict:
    """A rank call's result, the floats as their bit patterns (NaN compares equal to itself)."""
    out = {k: np.ascontiguousarray(r[k]).tolist() for k in ("n_less", "n_equal")}
    out.update({k: np.ascontiguousarray(r[k], dtype=np.float64).view(np.int64).tolist() for k in ("mean", "sd")})
    out["n_draws"] = r["n_draws"]
    return out


def chains(L: int) -> int:
    return next(c for c in (4, 3, 1) if L % c == 0)


def as_layout(x4: np.ndarray, layout: str) -> np.ndarray:
    """[S][P][C][N] as a C-contiguous array whose axes are `layout`."""
    return np.ascontiguousarray(np.transpose(x4, ["spcn".index(a) for a in layout]))


def off_by_one(ctx, ffi, x4: np.ndarray):
    """The simulations in device memory, the first draw one double behind the allocation's start."""
    buf = ffi.DeviceBuffer(ctx, x4.nbytes + 8).upload(np.concatenate([[0.0], x4.reshape(-1)]))
    view = types.SimpleNamespace(ptr=C.c_void_p(buf.ptr.value + 8))
    return buf, ffi.DeviceSims(ctx, view, ffi.tensor4_args(x4, "spcn"))


# ---- shapes, inputs and routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("SP", BATCHES, ids=lambda sp: f"S{sp[0]}P{sp[1]}")
@pytest.mark.parametrize("L", LENGTHS)
def test_bits_on_every_route(ctx, ffi, L, SP):
    S, P = SP
    x, t = edge_sample(S, P, L, seed=S)
    host = ffi.sbc_ranks_host(x, t)
    if L <= 129:                                                          # (the CPU tests hold the host routine at every length)
        check_against_references(host, x, t)
    want = bits(host)
    x4 = x.reshape(S, P, chains(L), -1)
    assert bits(ctx.sbc_ranks(x4, t)) == want                             # in place, the host entry
    dev = ctx.upload_sims(x4)
    buf, shifted = off_by_one(ctx, ffi, x4)
    try:
        assert ctx.sbc_sims_per_chunk(dev) == S
        assert bits(ctx.sbc_ranks(dev, t)) == want                        # in place, the device entry
        assert bits(ctx.sbc_ranks(shifted, t)) == want                    # rows off a 16-byte boundary
    finally:
        dev.free()
        buf.free()
    for layout in ("scnp", "cspn"):                                       # the ingest copy
        assert bits(ctx.sbc_ranks(as_layout(x4, layout), t, layout)) == want, layout
    d2 = ctx.upload_sims(as_layout(x4, "scnp"), "scnp")
    try:
        assert bits(ctx.sbc_ranks(d2, t)) == want
    finally:
        d2.free()


@pytest.mark.parametrize("L", [1, 65, 1025, 4097])
def test_f32_is_the_widened_f64(ctx, ffi, L):
    x, t = edge_sample(5, 7, L, seed=3)
    x32 = x.astype(np.float32)
    t = np.where(np.abs(t) > 1e6, t, x32.astype(np.float64)[:, :, 0])      # truths that f32 draws can equal
    want = bits(ffi.sbc_ranks_host(x32.astype(np.float64), t))
    x4 = x32.reshape(5, 7, chains(L), -1)
    for layout in ("spcn", "scnp"):
        assert bits(ctx.sbc_ranks(as_layout(x4, layout), t, layout)) == want, layout
    d = ctx.upload_sims(x4)
    try:
        assert ctx.sbc_sims_per_chunk(d) == 5 and bits(ctx.sbc_ranks(d, t)) == want
    finally:
        d.free()


@pytest.mark.parametrize("thin", [2, 3])
def test_thinning_is_a_larger_stride(ctx, ffi, thin):
    S, P, Cn, N = 5, 7, 3, 343
    x, t = edge_sample(S, P, Cn * N, seed=thin)
    x4 = x.reshape(S, P, Cn, N)
    kept = np.ascontiguousarray(x4[..., ::thin])
    want = bits(ffi.sbc_ranks_host(kept.reshape(S, P, -1), t))
    assert want["n_draws"] == Cn * -(-N // thin)
    assert bits(ctx.sbc_ranks(x4, t, thin=thin)) == want
    assert bits(ctx.sbc_ranks(as_layout(x4, "scnp"), t, "scnp", thin=thin)) == want
    assert bits(ctx.sbc_ranks(x4[..., ::thin], t)) == want                 # the same view, made by numpy
    d = ctx.upload_sims(x4)
    try:
        assert bits(ctx.sbc_ranks(d, t, thin=thin)) == want
    finally:
        d.free()


def test_a_row_does_not_depend_on_its_batch(ctx, ffi):
    x, t = edge_sample(33, 9, 1025, seed=8)
    x4 = x.reshape(33, 9, 1, -1)
    whole = ctx.sbc_ranks(x4, t)
    for s, p in ((0, 0), (7, 3), (32, 8)):
        one = ctx.sbc_ranks(x4[s:s + 1, p:p + 1], t[s:s + 1, p:p + 1])    # (a view of one row, at its own address)
        for k in KEYS:
            assert np.array_equal(one[k][0, 0], whole[k][s, p], equal_nan=True), (s, p, k)


# ---- launches ---------------------------------------------------------------------------------------------------------------------
OTHER_KERNELS = ("k_ingest", "k_moments", "k_moments_final", "k_tile_sort", "k_merge", "k_order_stats", "k_rank_z", "k_fold_merge",
                 "k_finalize", "k_splitters", "k_bucket_merge", "k_weight_prepare", "k_weighted_moments", "k_weighted_combine",
                 "k_wq_blocks", "k_wq_pick", "k_chain_moments", "k_acf_mean")


def test_only_the_intended_kernels_run(ctx, ffi):
    x, t = edge_sample(33, 9, 2049)
    x4 = x.reshape(33, 9, 3, -1)
    ctx.profile(True)
    try:
        for draws in (x4, None):
            d = ctx.upload_sims(x4) if draws is None else draws
            ctx.profile_reset()
            ctx.sbc_ranks(d, t)
            prof = ctx.profile_get()
            if draws is None:
                d.free()
            assert prof["k_sbc_ranks"]["launches"] == 1, prof
            for name in OTHER_KERNELS:
                assert name not in prof, name
        ctx.profile_reset()
        ctx.sbc_ranks(as_layout(x4, "scnp"), t, "scnp")
        prof = ctx.profile_get()
        assert prof["k_sbc_ranks"]["launches"] == 1 and prof["k_ingest"]["launches"] == 1, prof     # (the simulations lie along z)
        assert set(prof) == {"k_sbc_ranks", "k_ingest"}, prof
    finally:
        ctx.profile(False)


# ---- the workspace limit ---------------------------------------------------------------------------------------------------------
def test_workspace_chunks_of_simulations(ffi):
    S, P, L = 9, 7, 20001                                                # (the smallest limit is 1 MiB: a copy must exceed it)
    x, t = edge_sample(S, P, L, seed=2)
    want = bits(ffi.sbc_ranks_host(x, t))
    y = as_layout(x.reshape(S, P, 1, L), "scnp")
    one = P * L * 8                                                      # a simulation's ingest copy
    with ffi.Context(0) as small:
        dev = small.upload_sims(y, "scnp")
        inplace = small.upload_sims(x.reshape(S, P, 1, L))
        small.profile(True)
        for per in (1, 2, S - 1):
            small._check(small.lib.mcr_set_workspace_limit(small.handle, per * one))
            assert small.sbc_sims_per_chunk(dev) == per == small.sbc_sims_per_chunk(y, "scnp")
            assert small.sbc_sims_per_chunk(inplace) == S                # no copy: nothing to fit
            for draws in (dev, y):                                       # the device and the host entry
                small.profile_reset()
                assert bits(small.sbc_ranks(draws, t, "scnp")) == want, per
                prof = small.profile_get()
                assert prof["k_sbc_ranks"]["launches"] == prof["k_ingest"]["launches"] == -(-S // per), (per, prof)
            assert bits(small.sbc_ranks(inplace, t)) == want
        small.profile(False)
        small._check(small.lib.mcr_set_workspace_limit(small.handle, one - 8))
        for call in (lambda: small.sbc_sims_per_chunk(dev), lambda: small.sbc_ranks(dev, t), lambda: small.sbc_ranks(y, t, "scnp")):
            with pytest.raises(ffi.McrError) as e:
                call()
            assert e.value.code == ffi.MCR_ENOMEM and "one simulation needs" in e.value.message
        assert bits(small.sbc_ranks(inplace, t)) == want                 # in place still runs
        dev.free()
        inplace.free()


# ---- errors and empty shapes ---------------------------------------------------------------------------------------------------
def test_nonfinite_draws_are_counted_and_the_rest_written(ctx, ffi):
    x, t = edge_sample(5, 7, 300, seed=4)
    ok = ctx.sbc_ranks(x.reshape(5, 7, 3, -1), t)
    bad = x.copy()
    bad[1, 0, 7], bad[1, 0, 8], bad[4, 6, 299] = np.nan, -np.inf, np.inf
    clean = np.ones((5, 7), dtype=bool)
    clean[1, 0] = clean[4, 6] = False
    for layout in ("spcn", "scnp"):
        rc, got = ctx.sbc_ranks_rc(as_layout(bad.reshape(5, 7, 3, -1), layout), t, layout)
        assert rc == ffi.MCR_ENONFINITE and "3 non-finite" in ctx.lib.mcr_last_error(ctx.handle).decode()
        for k in KEYS:
            assert np.array_equal(got[k][clean], ok[k][clean]), (layout, k)
        assert got["n_less"][1, 0] == (bad[1, 0] < t[1, 0]).sum() and got["n_less"][4, 6] == (bad[4, 6] < t[4, 6]).sum()
        assert np.isnan(got["mean"][1, 0]) and np.isnan(got["sd"][4, 6])
    with pytest.raises(ffi.McrError) as e:
        ctx.sbc_ranks(bad.reshape(5, 7, 3, -1), t)
    assert e.value.code == ffi.MCR_ENONFINITE
    assert bits(ctx.sbc_ranks(x.reshape(5, 7, 3, -1), t)) == bits(ok)


def test_refusals_leave_the_outputs_and_the_context(ctx, ffi):
    x, t = edge_sample(5, 7, 300, seed=4)
    x4 = x.reshape(5, 7, 3, -1)
    base = bits(ctx.sbc_ranks(x4, t))
    dev = ctx.upload_sims(x4)
    try:
        for v in (np.nan, np.inf, -np.inf):
            tb = t.copy()
            tb[3, 2] = v
            for draws in (x4, dev):
                rc, got = ctx.sbc_ranks_rc(draws, tb)
                assert rc == ffi.MCR_EINVAL and "truth[3][2]" in ctx.lib.mcr_last_error(ctx.handle).decode()
                assert (got["n_less"] == -1).all() and (got["n_equal"] == -1).all()              # the sentinels
                assert np.isnan(got["mean"]).all() and np.isnan(got["sd"]).all()
                assert bits(ctx.sbc_ranks(draws, t)) == base
        arrs, out = ffi._sbc_arrays(5, 7)
        targs = list(ffi.tensor4_args(x4, "spcn"))
        for at, v in ((1, -1), (2, -1), (3, -1), (4, -1), (5, -1), (6, -1), (7, -1), (8, -1), (1, 1 << 31), (0, 7)):
            a = list(targs)
            a[at] = v
            rc = ctx.lib.mcr_sbc_ranks_dev(ctx.handle, dev.buf.ptr, *a, ffi._as_dp(t), C.byref(out))
            assert rc == ffi.MCR_EINVAL, (at, v)
        assert ctx.lib.mcr_sbc_ranks_dev(ctx.handle, dev.buf.ptr, targs[0], 1, 1 << 16, 1 << 15, 1, 0, 1 << 15, 1, 0, ffi._as_dp(t),
                                         C.byref(out)) == ffi.MCR_EINVAL                         # C * N = 2^31
        assert ctx.lib.mcr_sbc_ranks_dev(ctx.handle, dev.buf.ptr, *targs, ffi._as_dp(t), None) == ffi.MCR_EINVAL
        assert ctx.lib.mcr_sbc_ranks_dev(ctx.handle, dev.buf.ptr, *targs, None, C.byref(out)) == ffi.MCR_EINVAL
        assert (arrs["n_less"] == -1).all() and np.isnan(arrs["mean"]).all()
        t3 = ctx.upload(x4[0], "pcn")
        ctx.enqueue(t3, min_chains=2)                                                   # a summary in flight
        rc, _ = ctx.sbc_ranks_rc(dev, t)
        assert rc == ffi.MCR_EINVAL and "in flight" in ctx.lib.mcr_last_error(ctx.handle).decode()
        ctx.wait()
        t3.free()
        assert bits(ctx.sbc_ranks(dev, t)) == base
    finally:
        dev.free()


def test_empty_shapes(ctx, ffi):
    r = ctx.sbc_ranks(np.empty((3, 2, 4, 0)), np.zeros((3, 2)))
    assert r["n_draws"] == 0 and not r["n_less"].any() and not r["n_equal"].any() and np.isnan(r["mean"]).all() and np.isnan(r["sd"]).all()
    assert ctx.sbc_ranks(np.empty((0, 2, 1, 5)), np.empty((0, 2)))["n_less"].shape == (0, 2)
    assert ctx.sbc_ranks(np.empty((2, 0, 1, 5)), np.empty((2, 0)))["mean"].shape == (2, 0)
    assert ctx.sbc_sims_per_chunk(np.empty((0, 2, 1, 5))) == 0 and ctx.sbc_sims_per_chunk(np.empty((3, 2, 4, 0))) == 0
    with pytest.raises(ValueError):
        ctx.sbc_ranks(np.zeros((2, 2, 5)), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ctx.sbc_ranks(np.zeros((2, 2, 1, 5)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        ctx.sbc_ranks(np.zeros((2, 2, 1, 5)), np.zeros((2, 2)), thin=0)
    t3 = ctx.upload(np.zeros((2, 1, 5)))                                  # one simulation's tensor is not S of them,
    sims = ctx.upload_sims(np.zeros((2, 2, 1, 5)))                        # and S of them are not one tensor
    try:
        with pytest.raises(ValueError):
            ctx.sbc_ranks(t3, np.zeros((2, 2)))
        for call in (ctx.hdi, ctx.pareto_khat, ctx.autocorr):
            with pytest.raises(ValueError):
                call(sims)
        with pytest.raises(ValueError):
            ffi.DeviceSims(ctx, sims.buf, t3.targs)
        assert isinstance(sims, ffi.DeviceSims) and not isinstance(sims, ffi.DeviceTensor) and sims.shape_scnp == (2, 1, 5, 2)
    finally:
        t3.free()
        sims.free()
    # S == 0 reads nothing: a NULL draws pointer is no error; the plan refuses what the call refuses
    arrs, out = ffi._sbc_arrays(1, 1)
    assert ctx.lib.mcr_sbc_ranks_dev(ctx.handle, None, ffi.MCR_F64, 0, 1, 5, 2, 10, 5, 1, 5, None, C.byref(out)) == ffi.MCR_OK
    v = C.c_int64(-7)
    assert ctx.lib.mcr_sbc_plan(ctx.handle, ffi.MCR_F64, 1 << 31, 1, 5, 2, 10, 5, 1, 5, C.byref(v)) == ffi.MCR_EINVAL
    assert ctx.lib.mcr_sbc_plan(ctx.handle, ffi.MCR_F64, -1, 1, 5, 2, 10, 5, 1, 5, C.byref(v)) == ffi.MCR_EINVAL and v.value == -7
    assert ctx.lib.mcr_sbc_plan(ctx.handle, ffi.MCR_F32, (1 << 31) - 1, 1, (1 << 31) - 2, 1, (1 << 31) - 2, 0, 1, 0, C.byref(v)) == ffi.MCR_ENOMEM


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_conjugate_normal_on_the_device(ctx, sbc_mod):
    check_conjugate(sbc_mod, ctx)
    check_conjugate(sbc_mod, ctx, lambda x: (np.ascontiguousarray(x.transpose(0, 2, 1))[:, None], "scnp"))


def test_files_and_the_command(ctx, ffi, sbc_mod, tmp_path, monkeypatch):
    from click.testing import CliRunner

    from mcmc_ref_hip import cli

    paths, table, x, truth = write_simulations(tmp_path)
    r = sbc_mod.sbc_files(paths, table, context=ctx, bins=5)
    assert r.names == ("mu", "tau") and r.n_draws == 24 and np.array_equal(r.ranks, (x < truth[..., None]).sum(-1))
    want = ffi.sbc_ranks_host(x, truth)
    assert np.array_equal(r.z_score, (want["mean"] - truth) / want["sd"])
    thin = sbc_mod.sbc_files(paths, {"mu": truth[:, 0], "tau": truth[:, 1]}, params=["tau"], context=ctx, bins=4, thin=2)
    assert thin.names == ("tau",) and np.array_equal(thin.ranks[:, 0], (x[:, 1, ::2] < truth[:, 1, None]).sum(-1))
    monkeypatch.setattr(ffi, "default_context", lambda: ctx)
    args = ["sbc", "--truth", str(table), "--bins", "5", "--format", "json"] + [str(p) for p in paths]
    res = CliRunner().invoke(cli.main, args)
    assert res.exit_code == 0, res.output
    doc = json.loads(res.output)
    assert doc["simulations"] == 3 and doc["draws"] == 24 and doc["failures"] == []
    assert doc["params"]["mu"]["p"] == pytest.approx(float(r.pvalue[0])) and doc["params"]["tau"]["dof"] == 4
    res = CliRunner().invoke(cli.main, args[:-3] + ["--p-min", "1.1"] + args[-3:])
    assert res.exit_code == 1 and len(json.loads(res.output)["failures"]) == 2
    res = CliRunner().invoke(cli.main, ["sbc", "--truth", str(table), "--params", "mu"] + [str(p) for p in paths])
    assert res.exit_code == 0 and "chi2" in res.output and "tau" not in res.output.split("\n", 1)[1]
