"""The benchmark's workloads at full size, every call path against the CPU oracle.

A plain `bench.py` run checks one result: the last pipelined call of the C1 model (phi <= 0.95, so tier 3 of the ESS
lags never runs).  The other workloads it used to check on every run -- sticky chains through k_tier3, the D sweep with
its result-buffer ring, the whole corpus batch, the lone and host-memory calls -- run only under `--full`.  This file
holds the same paths at the same sizes in the suite.  Every result of every call is compared either with the oracle
(`test_hip_parity.check_summary`: truncation lags and quantiles exact, the rest to 1e-9) or bit for bit with a result
that was.

`python tests/test_workloads_gpu.py` runs the oracle-only preconditions of these tests on a host without a GPU.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

from test_hip_parity import check_summary

pytestmark = pytest.mark.gpu

C, N = 4, 10000                     # the C1 shape: 4 chains x 10 000 draws
QS = (0.05, 0.5, 0.95)
ORACLE_THREADS = 16
INFLIGHT = 8                        # = MCR_MAX_INFLIGHT: the window of the headline loop
KEYS = ("mean", "std", "median", "rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "lag_bulk", "lag_tail",
        "q", "q_lo")

# k_tier3's stage geometry (mcr_diag.hpp: kLag2, kLongGroup, kT3StageGroups, t3_stage_first).  Tier 3 takes the lags
# [256, n) of the pairs still undecided at lag 255 in groups of 256 lags; the groups are walked in stages of 2, 6, 8, 8, ...
# groups, one stage for chains of at most 8 groups.  n is the chain length the ESS kernels see: N (whole chains).
LAG2, LONG_GROUP, T3_STAGE_GROUPS = 256, 256, 8


def t3_stage_first(st: int, groups: int) -> int:
    if groups <= T3_STAGE_GROUPS:
        return 0 if st == 0 else groups
    return 0 if st == 0 else (2 if st == 1 else T3_STAGE_GROUPS * (st - 1))


def t3_stage_lags(n: int, stages: int = 3) -> list[tuple[int, int]]:
    """[first lag, end lag) of the first `stages` stages of k_tier3 on chains of n draws."""
    groups = (n - LAG2 + LONG_GROUP - 1) // LONG_GROUP
    out = []
    for st in range(stages):
        a, b = t3_stage_first(st, groups), min(t3_stage_first(st + 1, groups), groups)
        out.append((LAG2 + LONG_GROUP * a, min(LAG2 + LONG_GROUP * b, n)))
    return out


def deciding_lags(exp) -> np.ndarray:
    """The lag of the first negative rho of every (parameter, kind) pair: the reference's walk accumulated `lag_*` terms
    (lags 1 .. lag_*) and stopped at the next lag; the tier whose lags hold it decides the pair."""
    return np.concatenate([exp["lag_bulk"], exp["lag_tail"]]) + 1


def stage_census(exp, n: int = N) -> dict:
    L = deciding_lags(exp)
    out = {"pairs": int(L.size), "below_64": int((L < 64).sum()), "tier2": int(((L >= 64) & (L < LAG2)).sum()),
           "tier3": int((L >= LAG2).sum())}
    for st, (a, b) in enumerate(t3_stage_lags(n)):
        out[f"stage{st} [{a}, {b})"] = int(((L >= a) & (L < b)).sum())
    return out


def assert_tier3_workload(census: dict, every_stage: bool):
    """What test_sticky_chains_through_k_tier3 claims about its data, from the oracle alone."""
    assert census["tier3"] >= 100, census
    if every_stage:
        assert all(v > 0 for k, v in census.items() if k.startswith("stage")), census
        assert census["below_64"] > 0 and census["tier2"] > 0, census


def assert_differ_everywhere(e1, e2):
    """Two oracle results of the same shape that differ in every field of every parameter (q_lo aside: a function of
    the shape alone)."""
    for k in KEYS[:-1]:
        assert np.all(e1[k] != e2[k]), (k, np.flatnonzero(e1[k] != e2[k]))


def sticky_model(P: int = 100, seed: int = 99) -> np.ndarray:
    """bench.leg_sticky's model: every parameter AR(1) with phi = 0.99 (integrated autocorrelation time ~ 200 draws),
    means 0 .. P - 1."""
    from scipy.signal import lfilter
    phi = 0.99
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -phi], rng.normal(size=(P, C, N)) * np.sqrt(1 - phi * phi), axis=2)
    x += np.arange(P)[:, None, None]
    return x


def mixed_phi_model(P: int = 100, seed: int = 8) -> np.ndarray:
    """AR(1) parameters with phi = 1 - logspace(-1, -3.5) (0.9 .. 0.9997) in a random order: pairs decided by tier 1,
    tier 2 and the first three k_tier3 stages sit side by side in one call."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    phi = rng.permutation(1.0 - np.logspace(-1, -3.5, P))
    e = rng.normal(size=(P, C, N))
    x = np.empty((P, C, N))
    for p in range(P):
        x[p] = lfilter([1.0], [1.0, -phi[p]], e[p] * np.sqrt(1 - phi[p] ** 2), axis=1)
    return x


def oracle_of(orc, x) -> dict:
    return orc.summarize_mt(x, "pcn", threads=ORACLE_THREADS)


def expected_q_lo(M: int) -> np.ndarray:
    """floor((M - 1) q): the order statistic below each quantile (mcmcref_hip.h)."""
    return np.array([math.floor((M - 1) * q) for q in QS], dtype=np.int64)


def assert_oracle(got, exp, M: int, what: str):
    check_summary(got, exp, what=what)
    assert np.array_equal(got["q_lo"], expected_q_lo(M)), (what, got["q_lo"])


def assert_same_bits(got, ref, what: str):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k)


def rolling_window(ctx, tensors, on_result, reuse: bool = True) -> int:
    """The headline loop: enqueue tensors[k] in order with at most INFLIGHT calls outstanding (wait_one delivers the
    oldest).  reuse: call k writes into the buffers delivered by call k - INFLIGHT (Context.enqueue(bufs=...)).
    on_result(k, result) sees each call's result when it is delivered, before its buffers are handed on.  Returns the
    number of calls that reused buffers."""
    ring, delivered, reused = [], 0, 0

    def deliver():
        nonlocal delivered
        b = ctx.wait_one()
        on_result(delivered, b.result())
        delivered += 1
        b.arrays["q_lo"][:] = -1        # a function of the shape: alternating tensors cannot show it stale, this can
        return b

    for t in tensors:
        if ctx.inflight >= INFLIGHT:
            b = deliver()
            if reuse:
                ring.append(b)
        r = ring.pop() if ring else None
        got = ctx.enqueue(t, quantiles=QS, bufs=r)
        if r is not None:
            assert got is r, "enqueue allocated new buffers instead of reusing the delivered ones"
            reused += 1
    while ctx.inflight:
        deliver()
    assert delivered == len(tensors) and ctx.wait_one() is None
    return reused


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    assert _ffi.MCR_MAX_INFLIGHT == INFLIGHT
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def c1(oracle):
    from mcmc_ref_hip import synth
    x = synth.c1_model(C, N, 100, seed=4711)
    return x, oracle_of(oracle, x)


@pytest.fixture(scope="module")
def sticky(oracle):
    x = sticky_model()
    return x, oracle_of(oracle, x)


@pytest.fixture(scope="module")
def mixed(oracle):
    x = mixed_phi_model()
    return x, oracle_of(oracle, x)


def test_c1_full_size_host_lone_and_rolling_window(ctx, c1):
    """The headline workload (BASELINE config 1, 4 x 10 000 x 100 f64) on every call path, against the oracle on all
    100 parameters: the host-memory call (32 MB: uploaded in pieces that overlap the lanes' kernels), the lone
    device-resident call (forks onto the lane's second stream) and 24 calls of the headline's rolling window (8 in
    flight over the lanes, delivered buffers reused).  Mirrors bench.py's headline and --full leg_call_latency."""
    x, exp = c1
    M = C * N
    host = ctx.summarize(x, "pcn", quantiles=QS)
    assert_oracle(host, exp, M, "c1 host")
    t = ctx.upload(x, "pcn")
    try:
        lone = ctx.summarize(t, quantiles=QS)
        assert_same_bits(lone, host, "c1 lone")
        reused = rolling_window(ctx, [t] * 24, lambda k, r: assert_same_bits(r, host, f"c1 window call {k}"))
        assert reused == 24 - INFLIGHT
    finally:
        t.free()


def test_result_ring_reuse_cannot_hide_stale_fields(ctx, c1, sticky):
    """Context.enqueue(bufs=...) writes a call's results into the arrays of an earlier, delivered call: a field the
    library failed to rewrite would keep the earlier call's value, unseen while consecutive calls agree.  Two models of
    the same shape whose oracle results differ in every field of every parameter (the C1 model and bench.leg_sticky's
    phi = 0.99 model) go through one ring in blocks of 8, so every reused buffer (call k takes call k - 8's) and every
    result slot held the OTHER model last; each delivery must equal the oracle of its own model.  q_lo depends on the
    shape alone, so it is overwritten with -1 before each reuse instead.  Only same-shape reuse is in play:
    enqueue allocates fresh buffers whenever P, the number of quantiles or `diagnostics` differ.  Mirrors the result
    ring of bench.py's headline loop and --full leg_d_sweep."""
    (xa, ea), (xb, eb) = c1, sticky
    assert_differ_everywhere(ea, eb)
    M = C * N
    ta, tb = ctx.upload(xa, "pcn"), ctx.upload(xb, "pcn")
    try:
        order = [(k // INFLIGHT) % 2 for k in range(4 * INFLIGHT)]
        exps = (ea, eb)
        reused = rolling_window(ctx, [(ta, tb)[i] for i in order],
                                lambda k, r: assert_oracle(r, exps[order[k]], M, f"ring call {k} model {order[k]}"))
        assert reused == 3 * INFLIGHT
    finally:
        ta.free(); tb.free()


def test_sticky_chains_through_k_tier3(ctx, oracle, sticky, mixed, monkeypatch):
    """Tier 3 of the ESS lags at full size: (a) bench.leg_sticky's model (phi = 0.99: ~115 of 200 pairs undecided at
    lag 255, walks to lag ~1 200) and (b) a mixed-phi model whose pairs end in tier 1, tier 2 and each of k_tier3's first
    three stages, side by side.  Preconditions from the oracle alone, then for each model, against the oracle:
      * a lone call (forked), and the same call profiled: ONE k_tier3 launch (counted as k_acov_long), neither the
        round-by-round scans (k_diag_long_scan) nor the FFT tier;
      * 16 pipelined calls on the default 4 lanes in blocks of 4, (a) and (b) alternating on every lane, so each lane's
        per-pair stage words (reset by k_diag_combine for every call) see another pair list on every call;
      * a context made with MCR_FORK=0;
      * a workspace limit that splits the 100 parameters into >= 3 chunks: one k_tier3 launch per chunk.
    Mirrors bench.py --full leg_sticky."""
    from mcmc_ref_hip import _ffi
    (xa, ea), (xb, eb) = sticky, mixed
    assert_tier3_workload(stage_census(ea), every_stage=False)
    assert_tier3_workload(stage_census(eb), every_stage=True)
    M, P = C * N, xa.shape[0]
    monkeypatch.setenv("MCR_FORK", "0")
    plain = _ffi.Context(0)
    monkeypatch.delenv("MCR_FORK")
    ts = [ctx.upload(xa, "pcn"), ctx.upload(xb, "pcn")]
    exps = (ea, eb)
    try:
        lone = []
        for i, t in enumerate(ts):
            r = ctx.summarize(t, quantiles=QS)
            assert_oracle(r, exps[i], M, f"tier3 lone {i}")
            lone.append(r)
            ctx.profile(True)
            try:
                ctx.profile_reset()
                r = ctx.summarize(t, quantiles=QS)
                prof = ctx.profile_get()
            finally:
                ctx.profile(False)
            assert_same_bits(r, lone[i], f"tier3 profiled {i}")
            assert prof.get("k_acov_long", {}).get("launches") == 1 and "k_diag_long_scan" not in prof and "k_fft" not in prof, prof

        order = [(k // 4) % 2 for k in range(16)]
        rolling_window(ctx, [ts[i] for i in order],
                       lambda k, r: assert_same_bits(r, lone[order[k]], f"tier3 pipelined call {k} model {order[k]}"))

        for i, t in enumerate(ts):
            r = plain.summarize(_ffi.DeviceTensor(plain, t.buf, t.targs), quantiles=QS)
            assert_same_bits(r, lone[i], f"tier3 MCR_FORK=0 {i}")

        try:
            limit = 1 << 30
            while True:
                ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, limit))
                per_chunk = ctx.params_per_chunk(ts[0])
                if -(-P // per_chunk) >= 3:
                    break
                limit //= 2
                assert limit >= 1 << 20, per_chunk
            chunks = -(-P // per_chunk)
            for i, t in enumerate(ts):
                r = ctx.summarize(t, quantiles=QS)
                assert_same_bits(r, lone[i], f"tier3 {chunks} chunks {i}")
                ctx.profile(True)
                try:
                    ctx.profile_reset()
                    r = ctx.summarize(t, quantiles=QS)
                    prof = ctx.profile_get()
                finally:
                    ctx.profile(False)
                assert_same_bits(r, lone[i], f"tier3 {chunks} chunks profiled {i}")
                assert prof.get("k_acov_long", {}).get("launches") == chunks and "k_diag_long_scan" not in prof, (chunks, prof)
        finally:
            ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 8 << 30))
    finally:
        for t in ts:
            t.free()
        plain.close()


@pytest.mark.parametrize("P", [1000, 10])
def test_d_sweep_host_lone_and_pipelined(ctx, oracle, P):
    """bench.py --full leg_d_sweep's extremes against the oracle on every parameter: D = 1000 (320 MB, the host call
    uploads it in 4 pieces, one per lane) and D = 10 (3.2 MB: one upload, the lanes mostly idle).  The host call, the
    lone device-resident call and the last of a 12-call rolling window (8 in flight, delivered buffers reused) match
    the oracle; every call of the window is bit-identical to the host call."""
    from mcmc_ref_hip import synth
    x = synth.c1_model(C, N, P, seed=4711)
    exp = oracle_of(oracle, x)
    M = C * N
    host = ctx.summarize(x, "pcn", quantiles=QS)
    assert_oracle(host, exp, M, f"D={P} host")
    t = ctx.upload(x, "pcn")
    try:
        lone = ctx.summarize(t, quantiles=QS)
        assert_oracle(lone, exp, M, f"D={P} lone")
        assert_same_bits(lone, host, f"D={P} lone")
        res = []

        def on_result(k, r):
            assert_same_bits(r, host, f"D={P} window call {k}")
            res.append(r)
        reused = rolling_window(ctx, [t] * 12, on_result)
        assert reused == 12 - INFLIGHT
        assert_oracle(res[-1], exp, M, f"D={P} last pipelined")
    finally:
        t.free()


def test_corpus_batch_every_parameter(ctx, oracle):
    """BASELINE config 2 device-resident (bench.py --full leg_corpus_device): the 57 packaged model shapes, same-shape
    models concatenated into one tensor per shape and enqueued pass after pass with at most MCR_MAX_INFLIGHT calls in
    flight; every delivered call matches the oracle on all 460 parameters.  Then the same tensors, and the 57 models
    one by one, through Context.summarize_models (one C call)."""
    from mcmc_ref_hip import corpus
    models = corpus.synthetic_corpus(seed=4711)
    assert len(models) == 57 and sum(a.shape[0] for _, a in models) == 460
    groups = {}
    for i, (_, arr) in enumerate(models):
        groups.setdefault(arr.shape[1:], []).append(i)
    bigs = [np.concatenate([models[i][1] for i in members], axis=0) for members in groups.values()]
    exps = [oracle_of(oracle, b) for b in bigs]
    Ms = [b.shape[1] * b.shape[2] for b in bigs]
    ts = [ctx.upload(b, "pcn") for b in bigs]
    mts = []
    try:
        G = len(ts)
        rolling_window(ctx, ts * 6, lambda k, r: assert_oracle(r, exps[k % G], Ms[k % G], f"corpus call {k}"),
                       reuse=False)
        for g, r in enumerate(ctx.summarize_models(ts, quantiles=QS)):
            assert_oracle(r, exps[g], Ms[g], f"summarize_models group {g}")
        # model i is the slice [p0, p0 + P_i) of its group's tensor
        where = {}
        for g, members in enumerate(groups.values()):
            p0 = 0
            for i in members:
                where[i] = (g, p0, p0 + models[i][1].shape[0])
                p0 += models[i][1].shape[0]
        mts = [ctx.upload(a, "pcn") for _, a in models]
        for i, r in enumerate(ctx.summarize_models(mts, quantiles=QS)):
            g, a, b = where[i]
            exp = {k: v[a:b] for k, v in exps[g].items()}
            assert_oracle(r, exp, Ms[g], f"summarize_models model {i} {models[i][0]}")
    finally:
        for t in ts + mts:
            t.free()


if __name__ == "__main__":           # the oracle-only preconditions, on any host
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root), str(root / "mcmc-db_amd")]
    from mcmc_ref_hip import synth
    from oracle import oracle as orc
    orc.build()
    print("k_tier3 stages on chains of", N, "draws:", t3_stage_lags(N, 5))
    ea, eb = oracle_of(orc, sticky_model()), oracle_of(orc, mixed_phi_model())
    for name, e, every in (("sticky phi = 0.99", ea, False), ("mixed phi", eb, True)):
        cen = stage_census(e)
        print(name, cen, "max deciding lag", int(deciding_lags(e).max()))
        assert_tier3_workload(cen, every_stage=every)
    assert_differ_everywhere(oracle_of(orc, synth.c1_model(C, N, 100, seed=4711)), ea)
    print("preconditions hold")
