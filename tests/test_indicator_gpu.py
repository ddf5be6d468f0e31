"""The indicator ESS on the device (libmcmcref_iess.so: k_pack_time / k_pack_tile / k_lag) against the host definition
mci_indicator_ess_host -- ESS in bits, truncation lag and count exactly -- and against the reference's fixture, at the
smallest shapes at which a path changes: the word edges of the packing, the lag block, the LDS / global switch of the lag
kernel, every pack route, every request count, chunking and batching.  Every case carries a parameter with ties.

The device and the host compile the arithmetic from one text without fused multiply-add, so no tolerance applies between
them; against the fixture the gates are those of test_indicator_refs_cpu (lag exact where unflagged, ESS 1e-9).
"""
from __future__ import annotations

import ctypes as C
import json
import math

import numpy as np
import pytest

from test_indicator_refs_cpu import LB, case_bits, close, fixture_cases, long_walk_cases, restate

pytestmark = pytest.mark.gpu

INF = float("inf")
PROBS = (0.05, 0.5, 0.95)


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ind():
    from mcmc_ref_hip import indicator
    return indicator


def draws(seed: int, P: int, C_: int, N: int, phi: float = 0.7) -> np.ndarray:
    """[P][C][N] AR(1) draws; parameter 0 is rounded to halves, so it is full of ties (and of draws equal to a threshold)."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(P, C_, N))
    x = e.copy()
    for t in range(1, N):
        x[:, :, t] = phi * x[:, :, t - 1] + e[:, :, t]
    x[0] = np.round(x[0] * 2) / 2
    return x


def quantile_requests(x: np.ndarray, probs=PROBS):
    """lower = -inf and upper [P][K] = the pooled quantiles of every parameter of x [P][C][N]."""
    return -INF, np.quantile(x.reshape(x.shape[0], -1), probs, axis=1).T.copy()


def same(a: dict, b: dict) -> bool:
    return (np.array_equal(a["ess"].view(np.int64), b["ess"].view(np.int64)) and np.array_equal(a["trunc"], b["trunc"])
            and np.array_equal(a["ones"], b["ones"]))


def agree(ind, ctx, x, lower, upper, layout="pcn"):
    """The device's answer, after holding it to the host definition."""
    got = ind.indicator_ess(x, lower, upper, layout, ctx)
    exp = ind.indicator_ess_host(x, lower, upper, layout)
    assert same(got, exp), (x.shape, layout, got, exp)
    return got


@pytest.mark.parametrize("N", [63, 64, 65, 127, 128, 129, LB - 1, LB, LB + 1, 2 * LB + 1])
def test_word_and_block_edges(ind, ctx, N):
    for C_ in (1, 2, 3, 4, 5):
        x = draws(100 * N + C_, 3, C_, N, phi=0.9)
        lo, hi = quantile_requests(x)
        r = agree(ind, ctx, x, lo, hi)
        for p in (0, 2):
            for k in range(3):
                exp = restate((x[p] <= hi[p, k]).astype(np.int64))
                assert (int(r["trunc"][p, k]), int(r["ones"][p, k])) == exp[1:] and close(float(r["ess"][p, k]), exp[0])


def test_long_walks(ind, ctx):
    """Persistent chains around the lag block (two of them truncate beyond the first block), and no negative lag at all."""
    truncs = {}
    for name, bits in long_walk_cases().items():
        r = agree(ind, ctx, bits.astype(np.float64)[None], 0.5, INF)
        exp = restate(bits)
        assert (int(r["trunc"][0, 0]), int(r["ones"][0, 0])) == exp[1:] and close(float(r["ess"][0, 0]), exp[0]), name
        truncs[name] = exp[1]
    assert truncs["n775_c1"] > LB and truncs["n775_c2"] > LB
    n = 2 * LB + 1
    level = np.stack([np.ones(n), np.zeros(n)])[None]              # constant at two levels: A == 0 at every lag
    r = agree(ind, ctx, level, 0.5, INF)
    assert (float(r["ess"][0, 0]), int(r["trunc"][0, 0]), int(r["ones"][0, 0])) == (2.0 * n, n, n)


@pytest.mark.parametrize("K", [1, 3, 31, 32])
def test_request_counts(ind, ctx, K):
    x = draws(K, 2, 2, 130)
    probs = [(j + 1) / (K + 1) for j in range(K)]
    lo, hi = quantile_requests(x, probs)
    a = agree(ind, ctx, x, lo, hi)
    b = agree(ind, ctx, np.ascontiguousarray(x.transpose(1, 2, 0)), lo, hi, "cnp")
    assert same(a, b)
    if K >= 3:                                                      # a request has the same bits alone
        one = agree(ind, ctx, x, -INF, hi[:, 2:3])
        assert np.array_equal(one["ess"][:, 0].view(np.int64), a["ess"][:, 2].view(np.int64))


@pytest.mark.parametrize("P", [1, 7, 65])
def test_parameter_contiguous_route(ind, ctx, P):
    x = draws(P, P, 3, 131)
    lo, hi = quantile_requests(x)
    a = agree(ind, ctx, x, lo, hi)
    b = agree(ind, ctx, np.ascontiguousarray(x.transpose(1, 2, 0)), lo, hi, "cnp")
    assert same(a, b)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_lds_global_switch(ind, ctx, delta):
    """C (ceil(N / 64) + 1) = MCI_LDS_WORDS - 1, + 0, + 1 words with one chain of iid draws (the walk is short), and three
    chains just past the limit."""
    from mcmc_ref_hip import _iabi
    words = _iabi.MCI_LDS_WORDS + delta
    N = 64 * (words - 1) - 5
    assert (N + 63) // 64 + 1 == words and N <= _iabi.MCI_MAX_DRAWS
    x = np.random.default_rng(words).normal(size=(1, 1, N))
    r = agree(ind, ctx, x, -INF, 0.3)
    assert 0 < r["trunc"][0, 0] < 64 and r["ones"][0, 0] == int((x <= 0.3).sum())
    if delta == 1:
        per = words // 3 + 1
        y = np.random.default_rng(5).normal(size=(1, 3, 64 * (per - 1) - 7))
        assert 3 * per > _iabi.MCI_LDS_WORDS
        agree(ind, ctx, y, -0.2, 0.9)


def test_routes_entries_and_dtypes_agree(ind, ctx):
    x = draws(11, 7, 3, 200)
    lo, hi = quantile_requests(x)
    base = agree(ind, ctx, x, lo, hi)                               # stride_n == 1: the ballot route
    assert same(base, agree(ind, ctx, np.ascontiguousarray(x.transpose(1, 2, 0)), lo, hi, "cnp"))      # stride_p == 1
    assert same(base, agree(ind, ctx, np.ascontiguousarray(x.transpose(2, 0, 1)), lo, hi, "npc"))      # neither
    wide = np.zeros((7, 3, 400))
    wide[:, :, ::2] = x
    assert same(base, agree(ind, ctx, wide[:, :, ::2], lo, hi))     # a strided view: stride_n == 2
    pad = np.zeros((3, 200, 9))
    pad[:, :, :7] = x.transpose(1, 2, 0)
    assert same(base, agree(ind, ctx, pad[:, :, :7], lo, hi, "cnp"))
    # f32 draws are widened exactly: the same answer as the widened f64 tensor, on both routes
    x32 = x.astype(np.float32)
    lo32, hi32 = quantile_requests(x32.astype(np.float64))
    w = agree(ind, ctx, x32.astype(np.float64), lo32, hi32)
    assert same(w, ind.indicator_ess(x32, lo32, hi32, "pcn", ctx))
    assert same(w, ind.indicator_ess(np.ascontiguousarray(x32.transpose(1, 2, 0)), lo32, hi32, "cnp", ctx))
    # the device entry on a tensor of the context's, against the host entry
    with ctx.upload(x, "pcn") as t:
        assert same(base, ind.indicator_ess(t, lo, hi, context=ctx))
    with ctx.upload(np.ascontiguousarray(x32.transpose(1, 2, 0)), "cnp") as t:
        assert same(w, ind.indicator_ess(t, lo32, hi32, context=ctx))


def test_alone_in_a_batch_and_under_every_chunking(ind, ctx):
    x = draws(23, 5, 2, 200)
    lo, hi = quantile_requests(x)
    base = agree(ind, ctx, x, lo, hi)
    for p in range(5):                                              # alone against its place in the batch
        one = ind.indicator_ess(x[p:p + 1], lo, hi[p:p + 1], "pcn", ctx)
        assert all(np.array_equal(one[k][0], base[k][p]) for k in ("trunc", "ones"))
        assert np.array_equal(one["ess"][0].view(np.int64), base["ess"][p].view(np.int64))
    rev = ind.indicator_ess(x[::-1].copy(), lo, hi[::-1].copy(), "pcn", ctx)
    assert same({k: v[::-1] for k, v in rev.items()}, base)
    try:
        limits = {}
        for nbytes in range(512, 8192, 128):
            ind.set_workspace_limit(nbytes, ctx)
            try:
                limits.setdefault(ind.params_per_chunk(2, 200, 5, 3, context=ctx), nbytes)
            except Exception:                                       # one parameter does not fit yet
                continue
        assert {1, 2, 5} <= set(limits), limits
        for chunk in (1, 2, 5):
            ind.set_workspace_limit(limits[chunk], ctx)
            assert ind.params_per_chunk(2, 200, 5, 3, context=ctx) == chunk
            assert same(base, ind.indicator_ess(x, lo, hi, "pcn", ctx))
            assert same(base, ind.indicator_ess(np.ascontiguousarray(x.transpose(1, 2, 0)), lo, hi, "cnp", ctx))
    finally:
        ind.set_workspace_limit(1 << 30, ctx)


def test_fixture_on_the_device(ind, ctx):
    for c in fixture_cases():
        bits = case_bits(c)
        r = agree(ind, ctx, bits.astype(np.float64)[None], 0.5, INF)
        trunc = int(r["trunc"][0, 0])
        if not c["flagged"]:
            assert trunc == c["trunc"], c["name"]
        if trunc == c["trunc"]:
            assert close(float(r["ess"][0, 0]), c["ess"]), c["name"]


def test_edges_on_the_device(ind, ctx):
    r = agree(ind, ctx, np.array([[[1.0], [0.0], [1.0]]]), 0.5, INF)                    # n < 2
    assert math.isnan(r["ess"][0, 0]) and (r["trunc"][0, 0], r["ones"][0, 0]) == (-1, 2)
    x = np.arange(24, dtype=np.float64).reshape(1, 3, 8)
    x[0, 1, 3] = math.nan
    r = agree(ind, ctx, x, [-INF, 100.0, 5.0, 5.0, 2.0], [INF, INF, 5.0, 4.0, 9.0])
    assert r["ones"].tolist() == [[23, 0, 0, 0, 7]] and r["trunc"][0, 1:4].tolist() == [0] * 3      # (the NaN draw is a 0)
    assert r["ess"][0, 1:4].tolist() == [24.0] * 3
    hand = agree(ind, ctx, np.array([[[1.0, 1, 1, 0, 0, 0]]]), 0.5, INF)
    assert hand["trunc"][0, 0] == 3 and close(float(hand["ess"][0, 0]), 30 / 11)


def test_errors_leave_the_handle_usable(ind, ctx):
    from mcmc_ref_hip import _ffi
    x = draws(3, 2, 2, 100)
    lo, hi = quantile_requests(x)
    base = agree(ind, ctx, x, lo, hi)
    h = ind._handle(ctx)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
    flat, many = np.ascontiguousarray(x), np.zeros(2 * 33)
    for args, cause in (((0, 2, 100, 2, 100, 1, 200, dp(many), dp(many), 33), "MCI_MAX_REQUESTS"),
                        ((0, 2, 100, 2, 100, 1, 200, dp(many), dp(many), 0), "MCI_MAX_REQUESTS"),
                        ((7, 2, 100, 2, 100, 1, 200, dp(many), dp(many), 1), "dtype"),
                        ((0, 2, 100, 2, 100, -1, 200, dp(many), dp(many), 1), "stride"),
                        ((0, 2, (1 << 20) + 1, 2, 100, 1, 200, dp(many), dp(many), 1), "MCI_MAX_DRAWS"),
                        ((0, 4096, 1 << 19, 2, 100, 1, 200, dp(many), dp(many), 1), "2^31")):
        rc = h.lib.mci_indicator_ess(h.handle, flat.ctypes.data_as(C.c_void_p), *args, None, None, None)
        assert rc == _ffi.MCR_EINVAL and cause in h.lib.mci_last_error(h.handle).decode(), (cause, h.lib.mci_last_error(h.handle))
    bad = hi.copy()
    bad[1, 1] = math.nan
    with pytest.raises(_ffi.McrError, match="NaN"):
        ind.indicator_ess(x, lo, bad, "pcn", ctx)
    with pytest.raises(ValueError):
        ind.indicator_ess(x, lo, np.zeros((2, 33)), "pcn", ctx)
    try:
        ind.set_workspace_limit(64, ctx)
        with pytest.raises(_ffi.McrError, match="workspace") as e:
            ind.indicator_ess(x, lo, hi, "pcn", ctx)
        assert e.value.code == _ffi.MCR_ENOMEM
    finally:
        ind.set_workspace_limit(1 << 30, ctx)
    assert same(base, ind.indicator_ess(x, lo, hi, "pcn", ctx))


def test_python_layer(ind, ctx):
    x = draws(31, 3, 4, 250)
    q = ind.ess_quantile(x, PROBS, "pcn", ctx)
    want = np.quantile(x.reshape(3, -1), PROBS, axis=1).T
    assert np.array_equal(q["thresholds"], want)                   # numpy's linear quantiles, in bits
    for p in range(3):
        for k in range(3):
            exp = restate((x[p] <= want[p, k]).astype(np.int64))
            assert int(q["trunc"][p, k]) == exp[1] and close(float(q["ess"][p, k]), exp[0])
    assert np.array_equal(q["tail_min"], np.minimum(q["ess"][:, 0], q["ess"][:, 2]))
    with ctx.upload(x, "pcn") as t:                                 # a tensor of the context's gives the same
        qd = ind.ess_quantile(t, PROBS, context=ctx)
    assert np.array_equal(qd["ess"], q["ess"]) and np.array_equal(qd["thresholds"], q["thresholds"])
    loc = ind.ess_local(x, 4, "pcn", ctx)
    edges = np.quantile(x.reshape(3, -1), [0.25, 0.5, 0.75], axis=1).T
    assert np.array_equal(loc["edges"], edges) and loc["ess"].shape == (3, 4)
    for p in range(3):
        lo = np.concatenate([[-INF], edges[p]])
        hi = np.concatenate([edges[p], [INF]])
        for j in range(4):
            exp = restate(((x[p] > lo[j]) & (x[p] <= hi[j])).astype(np.int64))
            assert int(loc["trunc"][p, j]) == exp[1] and close(float(loc["ess"][p, j]), exp[0])
    assert np.array_equal(loc["efficiency"], loc["ess"] / 1000.0)
    ind.profile(True, ctx)
    try:
        ind.indicator_ess(x, -INF, want, "pcn", ctx)
        ms = ind.kernel_ms(ctx)
        assert set(ms) == {"pack", "lag"} and all(0.0 < v < 1000.0 for v in ms.values())
    finally:
        ind.profile(False, ctx)


def test_command(ind, ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli
    x = draws(41, 2, 4, 120)
    path = tmp_path / "draws.csv"
    rows = ["chain,draw,mu,tau"] + [f"{c},{t},{float(x[0, c, t])!r},{float(x[1, c, t])!r}" for c in range(4) for t in range(120)]
    path.write_text("\n".join(rows) + "\n")
    res = CliRunner().invoke(cli.main, ["ess-quantile", str(path), "--probs", "0.1", "--probs", "0.9", "--local", "4", "--format", "json"])
    assert res.exit_code == 0, res.output
    out = json.loads(res.output)
    q = ind.ess_quantile(x, (0.1, 0.9), "pcn", ctx)
    loc = ind.ess_local(x, 4, "pcn", ctx)
    for i, name in enumerate(("mu", "tau")):
        assert out[name]["q_0.1"] == q["thresholds"][i, 0] and out[name]["ess_q_0.9"] == q["ess"][i, 1]
        assert out[name]["ess_tail_min"] == q["tail_min"][i]
        assert [out[name][f"eff_local_{j}"] for j in range(4)] == loc["efficiency"][i].tolist()
    res = CliRunner().invoke(cli.main, ["ess-quantile", str(path), "--params", "tau"])
    assert res.exit_code == 0 and "ess_tail_min" in res.output and "tau" in res.output and "mu " not in res.output
    res = CliRunner().invoke(cli.main, ["ess-quantile", str(path), "--probs", "1.5"])
    assert res.exit_code != 0 and "inside (0, 1)" in res.output
