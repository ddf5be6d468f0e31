"""Importance-weighted summaries on the GPU (mcr_weighted_summary, mcr_weighted_summary_dev; mcr_weighted.hpp).

* Every output in BITS against the host routine mcr_weighted_host (tests/test_weighted_refs_cpu.py holds that one to
  numpy and to exact references) for linear weights: at both sides of every block (1024), tile (4096) and position-width
  (65 535) edge, with 1, 3 and 9 parameters (xcd_map deals them in groups of 8), odd M (every other row off a 16-byte
  boundary) and a device tensor that starts on and off one.
* One answer on every route: any workspace chunking, host / device entry, a strided view, f32 against the widened f64,
  any order of the parameters.
* Log weights: the returned weights fed back as linear ones give the same bits; against numpy on the host's exp the
  quantile VALUES are equal (under the margin precondition of the CPU tests) and the floats agree within 1e-9.
* Only the intended kernels run, k_weight_prepare once per call; errors leave the context usable; empty shapes; the file
  function, the command and validate_weighted end to end.
"""
from __future__ import annotations

import ctypes as C
import json
import types

import numpy as np
import pytest

from test_weighted_refs_cpu import GATE, QS, check_floats, numpy_quantiles, real_sample, threshold_margin, tied_sample

pytestmark = pytest.mark.gpu

FLOATS = ("mean", "sd", "mean_se")
SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65_535, 65_536, 65_537, 200_000]


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()


def as_bits(a) -> list:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).tolist()


def bits(r: dict) -> dict:
    out = {k: as_bits(r[k]) for k in FLOATS + ("quantiles",)}
    out.update({k: as_bits([r[k]]) for k in ("ess", "weight_sum")})
    return out


def rows(b: dict, sel) -> dict:
    """The bits of the parameters `sel` of a batch."""
    return {k: ([v[p] for p in sel] if k in FLOATS + ("quantiles",) else v) for k, v in b.items()}


def chains_of(x: np.ndarray) -> np.ndarray:
    """[P][M] -> [P][C][N] with 4 chains where M allows, else one."""
    P, M = x.shape
    return x.reshape(P, 4, M // 4) if M % 4 == 0 else x.reshape(P, 1, M)


def sample(M: int, P: int, seed: int = 0, offset: bool = True):
    """P parameters of M draws -- every third one heavily tied, with `offset` one at 1e8 -- and real weights with zeros."""
    rng = np.random.default_rng(1000 + seed + M)
    x = rng.standard_normal((P, M))
    x[::3] = np.round(x[::3] * 4.0) / 4.0 + 0.0                        # (+ 0.0: no -0.0, whose sign the sort does not keep)
    if P > 1 and offset:
        x[1] += 1e8
    w = np.exp(2.0 * rng.standard_normal(M))
    w[rng.random(M) < 0.1] = 0.0
    w[0] = 1.0
    return x, w


def host_bits(ffi, x: np.ndarray, w: np.ndarray, qs=QS) -> dict:
    per = [ffi.weighted_host(row, weights=w, quantiles=qs) for row in x]
    out = {k: as_bits([r[k] for r in per]) for k in FLOATS}
    out["quantiles"] = [as_bits(r["quantiles"]) for r in per]
    out.update({k: as_bits([per[0][k]]) for k in ("ess", "weight_sum")})
    return out


def offset_tensor(ffi, ctx, x3: np.ndarray, pad: int):
    """x3 in device memory behind `pad` doubles: a tensor that starts 8 * pad bytes behind a 256-byte boundary."""
    flat = np.concatenate([np.zeros(pad), x3.reshape(-1)])
    buf = ffi.DeviceBuffer(ctx, max(flat.nbytes, 8)).upload(flat)
    view = types.SimpleNamespace(ptr=C.c_void_p(buf.ptr.value + 8 * pad))
    return ffi.DeviceTensor(ctx, view, ffi.tensor_args(x3, "pcn")), buf


# ---- bits against the host routine -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_bits_against_the_host_routine(ctx, ffi, M):
    x, w = sample(M, 9)
    want = host_bits(ffi, x, w)
    nine = bits(ctx.weighted_summary(chains_of(x), weights=w, quantiles=QS))
    assert nine == want, M
    for P in (1, 3):                                                   # fewer than a group of 8, alone
        assert bits(ctx.weighted_summary(chains_of(x[:P]), weights=w, quantiles=QS)) == rows(want, range(P)), (M, P)
    for pad in (0, 1):                                                 # the device entry, on and off a 16-byte boundary
        t, buf = offset_tensor(ffi, ctx, chains_of(x), pad)
        try:
            assert bits(ctx.weighted_summary(t, weights=w, quantiles=QS)) == want, (M, pad)
        finally:
            buf.free()


@pytest.mark.parametrize("M", SIZES)
def test_integer_weights_and_tied_draws_equal_numpy(ctx, M):
    xs, ws = zip(*(tied_sample(M, seed) for seed in (1, 2, 3)))
    w = ws[0]
    x = np.stack(xs)
    got = ctx.weighted_summary(chains_of(x), weights=w, quantiles=QS)
    for p in range(3):
        assert np.array_equal(got["quantiles"][p], numpy_quantiles(x[p], w, QS)), (M, p)
    assert got["weight_sum"] == w.sum() and got["ess"] == w.sum() ** 2 / (w * w).sum()


# ---- one answer on every route -----------------------------------------------------------------------------------------------
def test_chunking_and_entries_give_the_same_bits(ctx, ffi):
    P, M = 5, 65_537                                                    # 32-bit positions, an odd M
    x, w = sample(M, P)
    x3 = chains_of(x)
    want = host_bits(ffi, x, w)
    assert bits(ctx.weighted_summary(x3, weights=w, quantiles=QS)) == want
    with ffi.Context(0) as small:
        ts = small.upload(x3)
        assert small.weighted_params_per_chunk(ts, len(QS)) == P
        limits = {}
        for mib in range(1, 24):
            small._check(small.lib.mcr_set_workspace_limit(small.handle, mib << 20))
            try:
                limits.setdefault(small.weighted_params_per_chunk(ts, len(QS)), mib)
            except ffi.McrError:
                continue
        assert {1, 2} <= set(limits), limits
        small.profile(True)
        for per in (1, 2):
            small._check(small.lib.mcr_set_workspace_limit(small.handle, limits[per] << 20))
            assert small.weighted_params_per_chunk(ts, len(QS)) == per
            small.profile_reset()
            assert bits(small.weighted_summary(ts, weights=w, quantiles=QS)) == want, per          # the device entry
            prof = small.profile_get()
            chunks = -(-P // per)
            assert prof["k_weight_prepare"]["launches"] == 1, prof                                 # once per call
            assert prof["k_weighted_moments"]["launches"] == 2 * chunks and prof["k_wq_pick"]["launches"] == chunks, prof
            assert bits(small.weighted_summary(x3, weights=w, quantiles=QS)) == want, per          # the host entry
        small.profile(False)
        ts.free()


def test_layouts_strides_and_f32(ctx, ffi):
    P, M = 4, 5000
    x, w = sample(M, P)
    x3 = chains_of(x)
    want = host_bits(ffi, x, w)
    cnp = np.ascontiguousarray(x3.transpose(1, 2, 0))                  # the ingest pass
    assert bits(ctx.weighted_summary(cnp, "cnp", weights=w, quantiles=QS)) == want
    wide = np.zeros((4, 2 * (M // 4), P + 3))                          # a strided cnp view: every other draw, 4 of 7 columns
    wide[:, ::2, 1:P + 1] = cnp
    assert bits(ctx.weighted_summary(wide[:, ::2, 1:P + 1], "cnp", weights=w, quantiles=QS)) == want
    x32 = x3.astype(np.float32)
    widened = bits(ctx.weighted_summary(x32.astype(np.float64), weights=w, quantiles=QS))
    assert widened == host_bits(ffi, x32.astype(np.float64).reshape(P, M), w)
    assert bits(ctx.weighted_summary(x32, weights=w, quantiles=QS)) == widened
    assert bits(ctx.weighted_summary(np.ascontiguousarray(x32.transpose(1, 2, 0)), "cnp", weights=w, quantiles=QS)) == widened
    t = ctx.upload(x32)
    try:
        assert bits(ctx.weighted_summary(t, weights=w, quantiles=QS)) == widened
    finally:
        t.free()


def test_the_order_of_the_parameters_changes_no_bit(ctx):
    x, w = sample(4097, 9)
    base = bits(ctx.weighted_summary(chains_of(x), weights=w, quantiles=QS))
    perm = np.random.default_rng(5).permutation(9)
    assert bits(ctx.weighted_summary(chains_of(x[perm]), weights=w, quantiles=QS)) == rows(base, perm)
    same = bits(ctx.weighted_summary(chains_of(np.repeat(x[4:5], 9, axis=0)), weights=w, quantiles=QS))
    assert same == rows(base, [4] * 9)


# ---- log weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,seed", [(5000, 12), (40_000, 13)])
def test_log_weights(ctx, M, seed):
    x0, w = real_sample(M, seed)
    assert threshold_margin(x0, w, QS[2:5]) >= 1e-9                    # from the reference alone (the CPU tests' seeds)
    x = np.stack([x0, -x0])                                            # (mirrored: the prefixes 1 - c against the same q)
    lw = np.log(w) + 700.0                                             # a shift no exp of the raw values would survive
    got = ctx.weighted_summary(chains_of(x), log_weights=lw, quantiles=QS, return_weights=True)
    wd = got["weights"]
    assert wd.shape == (M,) and wd.max() == 1.0 and np.allclose(wd, w / w.max(), rtol=1e-12, atol=0)
    again = ctx.weighted_summary(chains_of(x), weights=wd, quantiles=QS, return_weights=True)
    assert bits(again) == bits(got) and as_bits(again["weights"]) == as_bits(wd)          # pinned to the linear route
    wh = np.exp(lw - lw.max())                                         # the host's exp
    for p in range(2):
        assert np.array_equal(got["quantiles"][p], numpy_quantiles(x[p], wh, QS)), p
    check_floats({**{k: got[k][0] for k in FLOATS}, "ess": got["ess"], "weight_sum": got["weight_sum"]}, x[0], wh)
    assert got["mean"][1] == pytest.approx(-got["mean"][0], abs=GATE * got["sd"][0]) and got["sd"][1] == pytest.approx(got["sd"][0], rel=GATE)
    t = ctx.upload(chains_of(x))                                       # the device entry returns its weights from device memory
    try:
        dev = ctx.weighted_summary(t, log_weights=lw, quantiles=QS, return_weights=True)
        assert bits(dev) == bits(got) and as_bits(dev["weights"]) == as_bits(wd)
    finally:
        t.free()


def test_minus_infinity_is_a_zero_weight(ctx):
    x, w = real_sample(3000, 35)
    lw = np.log(w)
    lw[::3] = -np.inf
    w[::3] = 0.0
    got = ctx.weighted_summary(x.reshape(1, 1, -1), log_weights=lw, quantiles=QS, return_weights=True)
    assert (got["weights"][::3] == 0.0).all() and np.array_equal(got["quantiles"][0], numpy_quantiles(x, w, QS))
    assert bits(ctx.weighted_summary(x.reshape(1, 1, -1), weights=got["weights"], quantiles=QS)) == bits(got)


# ---- equal weights ---------------------------------------------------------------------------------------------------------------
def test_equal_weights_agree_with_summarize(ctx):
    x, _ = sample(20_000, 4, offset=False)
    x3 = chains_of(x)
    got = ctx.weighted_summary(x3, weights=np.full(20_000, 0.125), quantiles=QS)
    ref = ctx.summarize(x3)
    for p in range(4):
        scale = max(ref["std"][p], abs(ref["mean"][p]))
        assert abs(got["mean"][p] - ref["mean"][p]) <= GATE * scale and abs(got["sd"][p] - ref["std"][p]) <= GATE * ref["std"][p]
        assert np.array_equal(got["quantiles"][p], np.quantile(x[p], QS, method="inverted_cdf"))
    assert got["ess"] == pytest.approx(20_000, rel=GATE)


# ---- launches ---------------------------------------------------------------------------------------------------------------------
OTHER_KERNELS = ("k_rank_z", "k_fold_merge", "k_acov_seg", "k_acov_more", "k_acov_long", "k_diag", "k_diag_combine2",
                 "k_diag_long_scan", "k_fft", "k_chain_moments", "k_nested_combine", "k_pareto_fit", "k_psis_column",
                 "k_psis_weights", "k_hdi_window", "k_hdi_pick", "k_acf_mean", "k_acf_products")


def test_only_the_intended_kernels_run(ctx):
    x, w = sample(65_536, 3)
    x3 = chains_of(x)
    ctx.profile(True)
    ctx.profile_reset()
    ctx.weighted_summary(x3, weights=w)
    prof = ctx.profile_get()
    ctx.profile_reset()
    none = ctx.weighted_summary(x3, weights=w, quantiles=())
    bare = ctx.profile_get()
    ctx.profile(False)
    want = {"k_weight_prepare": 1, "k_weighted_moments": 2, "k_weighted_combine": 2, "k_wq_blocks": 1, "k_wq_pick": 1, "k_tile_sort": 1}
    assert {k: prof[k]["launches"] for k in want} == want, prof
    for name in OTHER_KERNELS:
        assert name not in prof and name not in bare, name
    assert "k_wq_blocks" not in bare and "k_wq_pick" not in bare and bare["k_weighted_moments"]["launches"] == 2
    assert none["quantiles"].shape == (3, 0)
    assert as_bits(none["mean"]) == as_bits(ctx.weighted_summary(x3, weights=w)["mean"])


# ---- errors and empty shapes ---------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, ffi):
    x, w = sample(4096, 2)
    x3 = chains_of(x)
    base = bits(ctx.weighted_summary(x3, weights=w))

    def still_works():
        assert bits(ctx.weighted_summary(x3, weights=w)) == base

    bad = x3.copy()
    bad[1, 2, 5] = np.nan
    with pytest.raises(ffi.McrError) as e:
        ctx.weighted_summary(bad, weights=w)
    assert e.value.code == ffi.MCR_ENONFINITE
    still_works()
    t = ctx.upload(x3)
    try:
        texts = {}
        for name, v, log in (("nan", np.nan, False), ("inf", np.inf, False), ("negative", -1.0, False), ("log nan", np.nan, True),
                             ("log inf", np.inf, True)):
            wb = w.copy()
            wb[77] = v
            for entry, d in (("host", x3), ("dev", t)):
                with pytest.raises(ffi.McrError) as e:
                    ctx.weighted_summary(d, **({"log_weights": wb} if log else {"weights": wb}))
                assert e.value.code == ffi.MCR_EINVAL, (name, entry)
                texts.setdefault(name, set()).add(e.value.message)
            still_works()
        for entry, d in (("host", x3), ("dev", t)):
            for kw in ({"weights": np.zeros(4096)}, {"log_weights": np.full(4096, -np.inf)}):
                with pytest.raises(ffi.McrError, match="no entry is positive") as e:
                    ctx.weighted_summary(d, **kw)
                assert e.value.code == ffi.MCR_EINVAL, entry
        assert all(len(s) == 1 for s in texts.values()), texts          # one text on both entries
        still_works()
        # nothing is written to the outputs of a refused call
        mean, qs = np.full(2, 7.0), np.full(6, 7.0)
        ess, s1 = C.c_double(7.0), C.c_double(7.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        out = ffi.Weighted(mean=dp(mean), quantiles=dp(qs), ess=C.pointer(ess), weight_sum=C.pointer(s1))
        wb = w.copy()
        wb[5] = -2.0
        pr = np.array([0.05, 0.5, 0.95])
        rc = ctx.lib.mcr_weighted_summary(ctx.handle, x3.ctypes.data_as(C.c_void_p), *ffi.tensor_args(x3, "pcn"),
                                          wb.ctypes.data_as(C.c_void_p), 0, dp(pr), 3, C.byref(out))
        assert rc == ffi.MCR_EINVAL and (mean == 7.0).all() and (qs == 7.0).all() and ess.value == 7.0 and s1.value == 7.0
        still_works()
        ctx.enqueue(t)                                                  # a summary in flight
        with pytest.raises(ffi.McrError, match="summaries in flight") as e:
            ctx.weighted_summary(t, weights=w)
        assert e.value.code == ffi.MCR_EINVAL
        ctx.wait()
        assert bits(ctx.weighted_summary(t, weights=w)) == base
    finally:
        t.free()
    for kw in ({}, {"weights": w, "log_weights": w}, {"weights": w[:-1]}, {"weights": w, "quantiles": [0.5] * 17},
               {"weights": w, "quantiles": [1.5]}):
        with pytest.raises(ValueError):
            ctx.weighted_summary(x3, **kw)
    still_works()


def test_empty_shapes(ctx):
    empty = ctx.weighted_summary(np.empty((2, 4, 0)), weights=np.empty(0))                 # M == 0
    assert all(np.isnan(empty[k]).all() and empty[k].shape == (2,) for k in FLOATS)
    assert np.isnan(empty["quantiles"]).all() and empty["quantiles"].shape == (2, 3)
    assert np.isnan(empty["ess"]) and np.isnan(empty["weight_sum"]) and empty["n_draws"] == 0
    none = ctx.weighted_summary(np.empty((0, 4, 10)), weights=np.ones(40))                 # P == 0
    assert all(none[k].shape == (0,) for k in FLOATS) and none["quantiles"].shape == (0, 3)


# ---- Python, the command and validate_weighted ----------------------------------------------------------------------------------
def test_chains_of_unequal_lengths_are_pooled(ctx, ffi):
    from mcmc_ref_hip import diagnostics
    x, w = real_sample(1000, 41)
    cuts = [0, 100, 350, 351, 1000]
    chains = [x[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    got = diagnostics.weighted_summary(chains, weights=w, quantiles=QS, context=ctx)
    want = ffi.weighted_host(x, weights=w, quantiles=QS)
    assert all(got[k] == want[k] for k in FLOATS + ("ess", "weight_sum")) and np.array_equal(got["quantiles"], want["quantiles"])
    assert got["n_draws"] == 1000
    with pytest.raises(ValueError):
        diagnostics.weighted_summary(chains, weights=w[:-1], context=ctx)
    with pytest.raises(ValueError, match="not weights"):
        diagnostics.weighted_summary(chains, weights=-w, context=ctx)


def test_file_function_and_command(ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli
    from mcmc_ref_hip.convert import weighted_summary_file
    rng = np.random.default_rng(8)
    n = 500
    a, b = rng.normal(2.0, 1.0, 4 * n), rng.exponential(1.0, 4 * n)
    lw = 0.5 * (a - 2.0) - 0.3 * b
    path = tmp_path / "approx.csv"
    lines = ["chain,draw,a,lw,b"] + [f"{i // n},{i % n},{float(a[i])!r},{float(lw[i])!r},{float(b[i])!r}" for i in range(4 * n)]
    path.write_text("\n".join(lines) + "\n")
    x = np.stack([a, b]).reshape(2, 1, -1)
    sm = ctx.psis(lw.reshape(1, 1, -1))
    by_hand = ctx.weighted_summary(x, log_weights=sm["log_weights"][0])
    got = weighted_summary_file(path, log_weights="lw", context=ctx)
    assert list(got["params"]) == ["a", "b"] and got["n_draws"] == 4 * n
    assert got["khat"] == float(sm["khat"][0]) and got["khat_threshold"] == sm["khat_threshold"] and got["ess"] == by_hand["ess"]
    for i, name in enumerate(("a", "b")):
        assert got["params"][name] == {"mean": by_hand["mean"][i], "sd": by_hand["sd"][i], "mean_se": by_hand["mean_se"][i],
                                       "q5": by_hand["quantiles"][i, 0], "q50": by_hand["quantiles"][i, 1],
                                       "q95": by_hand["quantiles"][i, 2]}
    raw = weighted_summary_file(path, log_weights="lw", params=["b"], quantiles=(0.25,), psis=False, context=ctx)
    plain = ctx.weighted_summary(x[1:], log_weights=lw, quantiles=(0.25,))
    assert "khat" not in raw and raw["params"] == {"b": {"mean": plain["mean"][0], "sd": plain["sd"][0],
                                                         "mean_se": plain["mean_se"][0], "q25": plain["quantiles"][0, 0]}}
    with pytest.raises(ValueError, match="Unknown"):
        weighted_summary_file(path, log_weights="nope", context=ctx)
    res = CliRunner().invoke(cli.main, ["weighted-summary", str(path), "--log-weights", "lw", "--format", "json"])
    assert res.exit_code == 0, res.output
    assert json.loads(res.output) == got
    res = CliRunner().invoke(cli.main, ["weighted-summary", str(path), "--log-weights", "lw", "--params", "b"])
    assert res.exit_code == 0 and "mean_se" in res.output and "q50" in res.output and "khat" in res.output, res.output
    assert f"{got['params']['b']['mean']:.6g}" in res.output and "\na " not in res.output
    res = CliRunner().invoke(cli.main, ["weighted-summary", str(path), "--weights", "b", "--quantile", "0.5", "--no-psis"])
    assert res.exit_code == 0 and "khat" not in res.output, res.output
    res = CliRunner().invoke(cli.main, ["weighted-summary", str(path)])
    assert res.exit_code != 0 and "exactly one" in res.output
    res = CliRunner().invoke(cli.main, ["weighted-summary", str(path), "--log-weights", "lw", "--quantile", "1.5"])
    assert res.exit_code != 0 and "[0, 1]" in res.output


def test_validate_weighted_brings_shifted_draws_back(ctx, tmp_path):
    """Reference draws a ~ N(2, 1), b ~ N(-1, 0.5^2); `actual` is the reference with a shifted by half its sd, and the
    weights are the exact log ratio of the two Gaussians: the weighted mean / std gate passes, the unweighted one fails."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    from mcmc_ref_hip.validate import validate, validate_weighted
    (tmp_path / "draws").mkdir()
    (tmp_path / "meta").mkdir()
    rng = np.random.default_rng(9)
    ref = {"a": rng.normal(2.0, 1.0, 4000), "b": rng.normal(-1.0, 0.5, 4000)}
    pq.write_table(pa.table({"chain": np.repeat(np.arange(4), 1000), "draw": np.tile(np.arange(1000), 4), **ref}),
                   tmp_path / "draws" / "gauss.draws.parquet")
    (tmp_path / "meta" / "gauss.meta.json").write_text(json.dumps({"diagnostics": {}}))
    store = DataStore(local_root=tmp_path, packaged_root=tmp_path / "none")
    delta = 0.5
    actual = {"a": ref["a"] + delta, "b": ref["b"]}
    lw = ((actual["a"] - 2.0 - delta) ** 2 - (actual["a"] - 2.0) ** 2) / 2.0        # log N(y; 2, 1) - log N(y; 2.5, 1)
    assert not validate("gauss", actual, store=store, context=ctx).passed
    for psis in (True, False):
        res = validate_weighted("gauss", actual, lw, psis=psis, store=store, context=ctx)
        assert res.passed and res.failures == [] and res.compare.passed, res.failures
        assert (res.khat is not None) == psis and 1000 < res.ess < 4000
        assert set(res.stats) == {"a", "b"} and set(res.stats["a"]) == {"mean", "std", "mean_se", "q5", "q50", "q95"}
        assert abs(res.stats["a"]["mean"] - 2.0) < 5 * res.stats["a"]["mean_se"] + 0.05
        assert abs(res.stats["a"]["q50"] - 2.0) < 0.1
    gated = validate_weighted("gauss", actual, lw, khat_max=-10.0, ess_min=1e9, store=store, context=ctx)
    assert not gated.passed and gated.compare.passed and len(gated.failures) == 2
    assert gated.failures[0].startswith("khat=") and "> -10.0" in gated.failures[0]
    assert gated.failures[1].startswith("ess=") and "< 1000000000.0" in gated.failures[1]
    flat = validate_weighted("gauss", actual, np.zeros(4000), psis=False, store=store, context=ctx)      # equal weights: the shift stays
    assert not flat.passed and flat.ess == pytest.approx(4000)
    with pytest.raises(ValueError):
        validate_weighted("gauss", {"a": actual["a"], "b": actual["b"][:-1]}, lw, store=store, context=ctx)
