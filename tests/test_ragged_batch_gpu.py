"""Batched ragged-chain summaries (mcr_summarize_chains_enqueue / _dev, mcr_plan_chunks_chains) against the oracle per
parameter -- truncation lags, q_lo and every integer output exactly, floating-point outputs to 1e-9, pooled mean / std /
quantiles / median against oracle.stats -- and, bit for bit, against one mcr_diagnose_chains call per parameter: the same
kernels run per (parameter, kind) pair whatever the batch.  The one exception is a call whose listed pairs outnumber
its FFT slots ("Ragged batches and device row order"): pairs beyond the slots take the direct rounds, which
agree with the FFT to ~1e-14, so that case is held to the oracle alone.  Inputs: tests/ragged_cases.py."""
from __future__ import annotations

import numpy as np
import pytest

import ragged_cases
from conftest import rel_close

pytestmark = pytest.mark.gpu

QS = (0.05, 0.5, 0.95)
TOL = 1e-9
FLOATS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "median")
DIAG_KERNELS = ("k_rank_z", "k_fold_merge", "k_acov_seg", "k_acov_more", "k_diag", "k_diag_combine2", "k_acov_long",
                "k_diag_long_scan", "k_fft")


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip._ffi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_nofft():
    from mcmc_ref_hip._ffi import Context
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MCR_FFT", "0")
        c = Context(0)
    yield c
    c.close()


_EXPECTED: dict = {}


def expected(oracle, name):
    """(x, counts, min_chains, per-parameter oracle diagnostics, per-parameter oracle stats), computed once per case."""
    if name not in _EXPECTED:
        x, counts = ragged_cases.make(name)
        mc = ragged_cases.RAGGED[name][3]
        _EXPECTED[name] = (x, counts, mc, [oracle.diag(ragged_cases.chains_of(row, counts), mc) for row in x],
                           [oracle.stats(row, QS) for row in x])
    return _EXPECTED[name]


def assert_oracle(r, diags, stats, tag):
    for p, (d, s) in enumerate(zip(diags, stats)):
        assert int(r["lag_bulk"][p]) == d["lag_bulk"] and int(r["lag_tail"][p]) == d["lag_tail"], (tag, p, d)
        for k in FLOATS:
            assert rel_close(float(r[k][p]), d[k], TOL), (tag, p, k, float(r[k][p]), d[k])
        assert rel_close(float(r["mean"][p]), s["mean"], TOL) and rel_close(float(r["std"][p]), s["std"], TOL), (tag, p)
        for j, q in enumerate(QS):
            assert rel_close(float(r["q"][p][j]), s[f"q{int(q * 100)}"], TOL), (tag, p, q)
        assert [int(v) for v in r["q_lo"]] == s["_q_lo"], (tag, p)


def assert_per_parameter(ctx, r, x, counts, mc, tag):
    """Bit for bit what mcr_diagnose_chains gives for each parameter on its own."""
    for p, row in enumerate(x):
        one = ctx.diagnose_chains(ragged_cases.chains_of(row, counts), min_chains=mc)
        for k in FLOATS:
            a, b = np.float64(r[k][p]), np.float64(one[k])
            assert a.view(np.int64) == b.view(np.int64) or (np.isnan(a) and np.isnan(b)), (tag, p, k, a, b)
        assert int(r["lag_bulk"][p]) == one["lag_bulk"] and int(r["lag_tail"][p]) == one["lag_tail"], (tag, p)


def same_bits(a: dict, b: dict, tag=""):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape, (tag, k)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (tag, k)


@pytest.mark.parametrize("name", [n for n in ragged_cases.RAGGED if n != "random_walks"])
def test_batch_against_oracle_and_per_parameter_calls(ctx, oracle, name):
    x, counts, mc, diags, stats = expected(oracle, name)
    r = ctx.summarize_chains(x, counts, min_chains=mc, quantiles=QS)
    assert_oracle(r, diags, stats, name)
    assert_per_parameter(ctx, r, x, counts, mc, name)


@pytest.mark.parametrize("fft", [True, False])
def test_long_ragged_chains(ctx, ctx_nofft, oracle, fft):
    c = ctx if fft else ctx_nofft
    x, counts, mc, diags, stats = expected(oracle, "random_walks")
    c.profile(True)
    c.profile_reset()
    try:
        r = c.summarize_chains(x, counts, min_chains=mc, quantiles=QS)
        prof = c.profile_get()
    finally:
        c.profile(False)
    assert ("k_fft" in prof) == fft, prof
    assert_oracle(r, diags, stats, f"random_walks fft={fft}")
    assert_per_parameter(c, r, x, counts, mc, f"random_walks fft={fft}")     # enough FFT slots for all six pairs


def test_more_listed_pairs_than_fft_slots(ctx, oracle):
    """A workspace limit that leaves the FFT tier two slots: the other listed pairs take the direct rounds in the same
    call.  Oracle tolerance only (see the module docstring)."""
    x, counts, mc, diags, stats = expected(oracle, "random_walks")
    assert sum(d["lag_bulk"] >= 256 for d in diags) + sum(d["lag_tail"] >= 256 for d in diags) > 2
    ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 36 << 20))
    ctx.profile(True)
    ctx.profile_reset()
    try:
        r = ctx.summarize_chains(x, counts, min_chains=mc, quantiles=QS)
        prof = ctx.profile_get()
    finally:
        ctx.profile(False)
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 8 << 30))
    assert "k_fft" in prof and "k_acov_long" in prof, prof
    assert_oracle(r, diags, stats, "random_walks, two FFT slots")


def test_strided_parameters_take_the_ingest_pass(ctx, oracle):
    from mcmc_ref_hip._ffi import DeviceBuffer
    x, counts, mc, diags, stats = expected(oracle, "small")
    P, M = x.shape
    padded = np.full((P, M + 3), np.nan)
    padded[:, :M] = x
    lone = ctx.summarize_chains(x, counts, min_chains=mc, quantiles=QS)
    buf = DeviceBuffer(ctx, padded.nbytes).upload(padded)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        t = ctx.ragged_tensor(buf, counts, P, stride_p=M + 3)
        r = ctx.summarize(t, min_chains=mc, quantiles=QS)
        prof = ctx.profile_get()
    finally:
        ctx.profile(False)
        buf.free()
    assert "k_ingest" in prof
    same_bits(r, lone, "stride_p = M + 3")
    assert_oracle(r, diags, stats, "stride_p = M + 3")


def test_chunk_edge(ctx, oracle):
    from mcmc_ref_hip._ffi import DeviceBuffer
    P = 7
    base, counts = ragged_cases.make("seg_switch_ar95")
    rng = np.random.default_rng(77)
    x = np.ascontiguousarray(np.concatenate([base, base[::-1] * 0.5, rng.normal(size=(1, base.shape[1]))])[:P])
    whole = ctx.summarize_chains(x, counts, min_chains=4, quantiles=QS)
    buf = DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        t = ctx.ragged_tensor(buf, counts, P)
        limit = 8 << 20
        while True:
            ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, limit))
            per_chunk = ctx.params_per_chunk(t)
            if per_chunk < P:
                break
            limit //= 2
        assert 1 < per_chunk < P, (limit, per_chunk)
        r = ctx.summarize(t, min_chains=4, quantiles=QS)
    finally:
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, 8 << 30))
        buf.free()
    same_bits(r, whole, f"{per_chunk} parameters per chunk")
    d = oracle.diag(ragged_cases.chains_of(x[P - 1], counts), 4)         # a parameter of the last, partial chunk
    assert int(r["lag_bulk"][P - 1]) == d["lag_bulk"] and rel_close(float(r["ess_bulk"][P - 1]), d["ess_bulk"], TOL)


def test_ragged_and_rectangular_calls_in_flight_together(ctx):
    from mcmc_ref_hip._ffi import DeviceBuffer
    x, counts = ragged_cases.make("seg_switch_iid")
    rect = np.random.default_rng(3).normal(size=(4, 4, 500))
    lone_ragged = ctx.summarize_chains(x, counts, quantiles=QS)
    t_rect = ctx.upload(rect, "pcn")
    buf = DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        lone_rect = ctx.summarize(t_rect, quantiles=QS)
        t_ragged = ctx.ragged_tensor(buf, counts, x.shape[0])
        pending = [ctx.enqueue(t_rect, quantiles=QS), ctx.enqueue(t_ragged, quantiles=QS),
                   ctx.enqueue(t_rect, quantiles=QS), ctx.enqueue(t_ragged, quantiles=QS)]
        ctx.wait()
        for k, b in enumerate(pending):
            same_bits(b.result(), lone_ragged if k % 2 else lone_rect, f"call {k}")
    finally:
        t_rect.free()
        buf.free()


def test_nan_in_one_parameter(ctx):
    from mcmc_ref_hip._ffi import MCR_ENONFINITE, McrError
    x, counts = ragged_cases.make("small")
    good = ctx.summarize_chains(x, counts, quantiles=QS)
    bad = x.copy()
    bad[2, 57] = np.nan
    with pytest.raises(McrError) as ei:
        ctx.summarize_chains(bad, counts, quantiles=QS)
    assert ei.value.code == MCR_ENONFINITE
    same_bits(ctx.summarize_chains(x, counts, quantiles=QS), good, "after the NaN call")


def test_acceptance_matches_diagnose_chains(ctx):
    from mcmc_ref_hip._ffi import MCR_EINVAL, MCR_EMINCHAINS, MCR_EMINCHAINS_ARG, McrError
    x, counts = ragged_cases.make("two_chains")
    for kw, code in ((dict(min_chains=4), MCR_EMINCHAINS), (dict(min_chains=0), MCR_EMINCHAINS_ARG)):
        with pytest.raises(McrError) as ei:
            ctx.summarize_chains(x, counts, **kw)
        assert ei.value.code == code
        with pytest.raises(McrError) as ej:
            ctx.diagnose_chains(ragged_cases.chains_of(x[0], counts), **kw)
        assert ej.value.code == code
    many = np.ones(257, dtype=np.int64)
    with pytest.raises(McrError) as ei:
        ctx.summarize_chains(np.zeros((1, 257)), many, min_chains=1)
    assert ei.value.code == MCR_EINVAL
    r = ctx.summarize_chains(np.zeros((2, 0)), np.zeros(4, dtype=np.int64), min_chains=4, quantiles=QS)     # M == 0
    assert np.isnan(r["mean"]).all() and np.isnan(r["rhat"]).all() and not r["lag_bulk"].any()


def test_stats_only_launches_no_diagnostics_kernel(ctx, oracle):
    x, counts, mc, _diags, stats = expected(oracle, "seg_switch_iid")
    ctx.profile(True)
    try:
        ctx.profile_reset()
        r = ctx.summarize_chains(x, counts, min_chains=mc, quantiles=QS, diagnostics=False)
        prof = ctx.profile_get()
        ctx.profile_reset()
        ctx.summarize_chains(x, counts, min_chains=mc, quantiles=QS)
        prof_diag = ctx.profile_get()
    finally:
        ctx.profile(False)
    assert "k_tile_sort" in prof and not [k for k in DIAG_KERNELS if k in prof], prof
    assert "k_acov_seg" in prof_diag and "k_fold_merge" in prof_diag
    for p, s in enumerate(stats):
        assert rel_close(float(r["mean"][p]), s["mean"], TOL) and rel_close(float(r["std"][p]), s["std"], TOL)
        for j, q in enumerate(QS):
            assert rel_close(float(r["q"][p][j]), s[f"q{int(q * 100)}"], TOL)
    assert np.isnan(r["rhat"]).all()
