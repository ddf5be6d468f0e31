"""The rank-ECDF test of include/mcmcref_recdf.h on the device: every output of `rankecdf.rank_ecdf` has the bits of the
host definition `rank_ecdf_host` -- the counts are integers and every minimum is exact, so there is no tolerance -- at
the smallest shapes at which the kernels can go wrong: chains of 1, 63 .. 65, 255, 257 and 1 000 draws (the 16-byte loads'
peeled first and left-over last draw, rows that start 8 bytes off), 1, 2, 5, 64 chains and one more than a count
workgroup's tile, 2, 3, 64, 65 and 1 024 points (the search's power-of-two padding, the most thresholds), batches cut
into three chunks and more, both layouts, f32, views, a thin stride, an odd base offset, heavy ties and a constant
column.  The null sample equals the host's in bits under every chunking; a NaN is refused and the handle lives on; calls
of other entries in between change nothing.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("counts", "pooled", "tied", "u", "kmin", "dev", "g", "chain")
TOP = 1 << 40
SIMS = dict(sims=16, seed=5)          # a small null sample: the statistics are what these tests compare


@pytest.fixture(scope="module")
def recdf():
    from mcmc_ref_hip import rankecdf
    return rankecdf


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def bits(r: dict, p=None) -> dict:
    return {k: (np.asarray(r[k]) if p is None else np.asarray(r[k][p])).tobytes() for k in KEYS}


def same(got: dict, want: dict, where) -> None:
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k)
        assert g.tobytes() == w.tobytes(), (where, k, g, w)
    for k in ("pvalue", "reject", "thin", "n", "points"):
        assert np.array_equal(got[k], want[k]), (where, k)


def limit_for(ask, want: int) -> int:
    """The smallest workspace limit under which ask(limit) >= want (ask is monotone and does no device work)."""
    lo, hi = 1, TOP
    assert ask(hi) >= want
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ask(mid) >= want:
            hi = mid
        else:
            lo = mid
    return hi


def chunked(recdf, ctx, ask_name: str, args: tuple, want: int):
    """Sets the limit under which the plan `ask_name` gives `want` per chunk; returns that plan's answer."""
    from mcmc_ref_hip._abi import McrError

    def ask(limit: int) -> int:
        recdf.set_workspace_limit(limit, ctx)
        try:
            return getattr(recdf, ask_name)(*args, context=ctx)
        except McrError:
            return 0
    recdf.set_workspace_limit(limit_for(ask, want), ctx)
    return getattr(recdf, ask_name)(*args, context=ctx)


# ---- shapes -----------------------------------------------------------------------------------------------------------------

NS = (1, 63, 64, 65, 255, 257, 1000)
CS = (1, 2, 5, 64, "past")
KS = (2, 3, 64, 65, 1024)


def shapes() -> list:
    from mcmc_ref_hip import rankecdf
    out = []
    for i, n in enumerate(NS):
        for j in range(5):
            C_, K = CS[(i + j) % 5], KS[(i + 2 * j) % 5]
            if C_ == "past":
                C_ = rankecdf.chain_tile(1 << 30, n, K) + 1
            if 2 <= K <= C_ * n:
                out.append((C_, n, K))
    out += [(7, 255, 1024), (97, 63, 64), (13, 257, 1024), (64, 65, 1024), (5, 1000, 1024), (64, 1, 64), (2, 1, 2)]
    return sorted(set(out))


def test_shape_list(recdf):
    got = shapes()
    assert {n for _, n, _ in got} == set(NS) and {K for *_, K in got} == set(KS) and {1, 2, 5, 64} <= {C_ for C_, *_ in got}
    past = [(C_, n, K) for C_, n, K in got if C_ == recdf.chain_tile(1 << 30, n, K) + 1]
    assert len(past) >= 5 and any(K == 1024 for *_, K in past)
    assert any((C_ * n) % K for C_, n, K in got) and len(got) <= 40


@pytest.mark.parametrize("C_,n,K", shapes())
def test_device_equals_host(recdf, ctx, C_, n, K):
    x = np.random.default_rng(1000 * C_ + 10 * n + K).standard_normal((3, C_, n))
    want = recdf.rank_ecdf_host(x, points=K, **SIMS)
    same(recdf.rank_ecdf(x, "pcn", points=K, context=ctx, **SIMS), want, "host array")
    assert np.all(want["tied"] == 0)
    with ctx.upload(x, "pcn") as t:
        same(recdf.rank_ecdf(t, points=K, context=ctx, **SIMS), want, "device tensor")


# ---- routes -------------------------------------------------------------------------------------------------------------------

P, C5, N5, K5 = 9, 5, 257, 65


@pytest.fixture(scope="module")
def batch():
    return np.random.default_rng(77).standard_normal((P, C5, N5))


@pytest.fixture(scope="module")
def batch_host(recdf, batch):
    return recdf.rank_ecdf_host(batch, points=K5, **SIMS)


def test_layouts_dtypes_and_views(recdf, ctx, batch, batch_host):
    cnp = np.ascontiguousarray(batch.transpose(1, 2, 0))
    same(recdf.rank_ecdf(cnp, "cnp", points=K5, context=ctx, **SIMS), batch_host, "cnp")
    f32 = batch.astype(np.float32)
    want32 = recdf.rank_ecdf_host(f32, points=K5, **SIMS)
    same(recdf.rank_ecdf(f32, "pcn", points=K5, context=ctx, **SIMS), want32, "f32 pcn")
    same(recdf.rank_ecdf(np.ascontiguousarray(f32.transpose(1, 2, 0)), "cnp", points=K5, context=ctx, **SIMS), want32, "f32 cnp")
    wide = np.random.default_rng(78).standard_normal((P, C5 + 1, 2 * N5 + 3))
    wide[:, 1:, 3:3 + N5] = batch
    same(recdf.rank_ecdf(wide[:, 1:, 3:3 + N5], "pcn", points=K5, context=ctx, **SIMS), batch_host, "a view")
    long = np.random.default_rng(79).standard_normal((P, C5, 3 * N5 - 1))                 # 770 = 3 * 256 + 2 draws, every third kept
    want = recdf.rank_ecdf_host(long, points=K5, thin=3, **SIMS)
    got = recdf.rank_ecdf(long, "pcn", points=K5, thin=3, context=ctx, **SIMS)
    assert (got["thin"], got["n"]) == (3, N5)
    same(got, want, "thin")
    with ctx.upload(long, "pcn") as t:
        same(recdf.rank_ecdf(t, points=K5, thin=3, context=ctx, **SIMS), want, "thin, device tensor")


def test_an_odd_base_offset(recdf, ctx, batch, batch_host):
    """Contiguous f64 is read in place: with the tensor one double into its allocation every row that started 16-byte
    aligned starts 8 bytes off and the other way round."""
    from mcmc_ref_hip import _ffi
    from mcmc_ref_hip._device import DeviceArena, DeviceTensor
    flat = np.concatenate([[123.0], batch.ravel()])
    with DeviceArena(ctx, flat.nbytes) as arena:
        arena.buf.upload(flat)
        with arena.view(8, batch.nbytes) as view:
            t = DeviceTensor(ctx, view, (_ffi.MCR_F64, C5, N5, P, N5, 1, C5 * N5))
            same(recdf.rank_ecdf(t, points=K5, context=ctx, **SIMS), batch_host, "offset 8")
    for n in (64, 65):
        x = np.random.default_rng(n).standard_normal((2, 3, n))
        flat = np.concatenate([[5.0], x.ravel()])
        with DeviceArena(ctx, flat.nbytes) as arena:
            arena.buf.upload(flat)
            with arena.view(8, x.nbytes) as view:
                t = DeviceTensor(ctx, view, (_ffi.MCR_F64, 3, n, 2, n, 1, 3 * n))
                same(recdf.rank_ecdf(t, points=16, context=ctx, **SIMS), recdf.rank_ecdf_host(x, points=16, **SIMS), n)


@pytest.mark.parametrize("K", [2, 65, 1024])
def test_ties_and_a_constant_column(recdf, ctx, K):
    rng = np.random.default_rng(K)
    x = rng.integers(-3, 4, (4, 5, 257)).astype(np.float64)
    x[1] = 0.25                                                         # constant
    x[2] = np.where(rng.random((5, 257)) < 0.5, -0.0, 0.0)             # signed zeros tie
    x[3, 2] = 7.0                                                       # one constant chain above the others
    want = recdf.rank_ecdf_host(x, points=K, **SIMS)
    got = recdf.rank_ecdf(x, "pcn", points=K, context=ctx, **SIMS)
    same(got, want, K)
    assert np.all(got["counts"][1] == 257) and got["tied"][1] == K - 1 and np.all(got["counts"][2] == 257)
    assert got["tied"][0] > 0 or K == 2
    if K == 2:
        assert got["chain"][3] == 2
    else:                                                               # more points than distinct values: the tied chains' counts
        assert got["g"][3] == 0.0 and got["chain"][3] == 0              # leave the support (u = 0) and the first of them is named
        assert 0.0 < got["u"][3, 2] < 1e-200


# ---- alone, in a batch, under every chunking -------------------------------------------------------------------------------------

def test_alone_in_a_batch_and_chunked(recdf, ctx, batch, batch_host):
    try:
        whole = recdf.rank_ecdf(batch, "pcn", points=K5, context=ctx, **SIMS)
        same(whole, batch_host, "whole")
        for p in (0, 4, 8):
            alone = recdf.rank_ecdf(batch[p:p + 1], "pcn", points=K5, context=ctx, **SIMS)
            assert bits(alone, 0) == bits(whole, p), p
        for per in (1, 2, 3, 4):                                        # 9, 5, 3 and 3 chunks
            assert chunked(recdf, ctx, "params_per_chunk", (C5, N5, P, K5), per) == per
            same(recdf.rank_ecdf(batch, "pcn", points=K5, context=ctx, **SIMS), batch_host, per)
        f32 = batch.astype(np.float32)                                  # the copy's route has a plan of its own
        assert chunked(recdf, ctx, "params_per_chunk", (C5, N5, P, K5, np.float32), 3) == 3
        same(recdf.rank_ecdf(f32, "pcn", points=K5, context=ctx, **SIMS), recdf.rank_ecdf_host(f32, points=K5, **SIMS), "f32 chunks")
    finally:
        recdf.set_workspace_limit(1 << 32, ctx)
    assert recdf.params_per_chunk(C5, N5, 1, K5, context=ctx) == 1


# ---- the null sample ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_,n,K,S", [(4, 250, 32, 300), (2, 65, 64, 33)])
def test_null_sample_equals_the_host(recdf, ctx, C_, n, K, S):
    want = recdf.null_sample_host(C_, n, K, S, seed=11)
    try:
        got = recdf.null_sample(C_, n, K, S, seed=11, context=ctx)
        assert got.tobytes() == want.tobytes()
        assert recdf.null_sample(C_, n, K, S, seed=11, context=ctx) is got          # cached on the context
        for per in (S // 3, 7):                                         # three chunks and a ragged last one; many
            recdf.clear_null_cache(ctx)
            assert chunked(recdf, ctx, "sims_per_chunk", (C_, n, K, S), per) == per
            assert recdf.null_sample(C_, n, K, S, seed=11, context=ctx).tobytes() == want.tobytes(), per
    finally:
        recdf.set_workspace_limit(1 << 32, ctx)
    assert recdf.null_sample(C_, n, K, S, seed=12, context=ctx).tobytes() == recdf.null_sample_host(C_, n, K, S, seed=12).tobytes()


def test_pvalues_against_the_device_null(recdf, ctx):
    x = np.random.default_rng(31).standard_normal((6, 4, 250))
    x[3, 1] += 1.0
    got = recdf.rank_ecdf(x, "pcn", points=32, sims=300, seed=11, context=ctx)
    g0 = recdf.null_sample_host(4, 250, 32, 300, seed=11)
    want = (1 + (g0[None, :] <= got["g"][:, None]).sum(axis=1)) / 301.0
    assert np.array_equal(got["pvalue"], want) and got["reject"][3] and got["chain"][3] == 1
    assert np.array_equal(got["reject"], want <= 0.05)


# ---- refusals, order, thinning by the ESS, the times -------------------------------------------------------------------------------

def test_nan_is_refused_and_the_handle_lives_on(recdf, ctx, batch, batch_host):
    from mcmc_ref_hip._abi import MCR_EINVAL, MCR_ENONFINITE, McrError
    for bad in (np.nan, np.inf):
        y = batch.copy()
        y[4, 2, 100] = bad
        with pytest.raises(McrError) as exc:
            recdf.rank_ecdf(y, "pcn", points=K5, context=ctx, **SIMS)
        assert exc.value.code == MCR_ENONFINITE
        same(recdf.rank_ecdf(batch, "pcn", points=K5, context=ctx, **SIMS), batch_host, "after the refusal")
    with pytest.raises(ValueError, match="points"):
        recdf.rank_ecdf(batch, "pcn", points=1025, context=ctx)
    h = recdf.RECDF.handle(ctx)
    assert h.lib.mce_null_sample(h.handle, 2, 8, 4, 0, 0, None) == MCR_EINVAL
    same(recdf.rank_ecdf(batch, "pcn", points=K5, context=ctx, **SIMS), batch_host, "after EINVAL")


def test_order_of_calls(recdf, ctx, batch, batch_host):
    from mcmc_ref_hip import standard
    with ctx.upload(batch, "pcn") as t:
        same(recdf.rank_ecdf(t, points=K5, context=ctx, **SIMS), batch_host, "first")
        std0 = standard.diagnostics(t, context=ctx)
        same(recdf.rank_ecdf(t, points=K5, context=ctx, **SIMS), batch_host, "after standard.diagnostics")
        sum0 = ctx.summarize(t)
        same(recdf.rank_ecdf(t, points=K5, context=ctx, **SIMS), batch_host, "after summarize")
        std1, sum1 = standard.diagnostics(t, context=ctx), ctx.summarize(t)
    for k in std0:
        assert np.asarray(std0[k]).tobytes() == np.asarray(std1[k]).tobytes(), k
    for k in ("mean", "std", "rhat", "ess_bulk", "ess_tail", "q"):
        assert np.asarray(sum0[k]).tobytes() == np.asarray(sum1[k]).tobytes(), k


def test_thin_by_the_ess_and_kernel_times(recdf, ctx):
    rng = np.random.default_rng(41)
    e = rng.standard_normal((2, 4, 4000))
    x = np.empty_like(e)
    x[..., 0] = e[..., 0]
    for i in range(1, 4000):
        x[..., i] = 0.9 * x[..., i - 1] + np.sqrt(0.19) * e[..., i]
    ess = ctx.summarize(x, "pcn")["ess_bulk"]
    stride = int(np.ceil(16000 / ess.min()))
    assert 5 <= stride <= 40                                             # theory: (1 + 0.9) / (1 - 0.9) = 19
    got = recdf.rank_ecdf(x, "pcn", points=32, thin="ess", context=ctx, **SIMS)
    assert got["thin"] == stride and got["n"] == -(-4000 // stride) and got["points"] == 32
    same(got, recdf.rank_ecdf_host(x, points=32, thin=stride, **SIMS), "ess")
    capped = recdf.rank_ecdf(x, "pcn", thin="ess", context=ctx, **SIMS)   # 100 points: n >= 200, a stride of at most 20
    assert capped["points"] == 100 and capped["thin"] == min(stride, 20) and capped["n"] >= 200
    recdf.profile(True, ctx)
    try:
        recdf.rank_ecdf(x, "pcn", points=32, context=ctx, **SIMS)
        ms = recdf.kernel_ms(ctx)
        assert list(ms) == ["fill", "pipe", "count", "stat"] and ms["fill"] == 0.0 and min(ms["pipe"], ms["count"], ms["stat"]) > 0.0
        recdf.clear_null_cache(ctx)
        recdf.null_sample(4, 250, 32, 64, seed=1, context=ctx)
        assert min(recdf.kernel_ms(ctx).values()) > 0.0
    finally:
        recdf.profile(False, ctx)
    assert sum(recdf.kernel_ms(ctx).values()) == 0.0
