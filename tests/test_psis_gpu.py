"""PSIS and PSIS-LOO on the GPU (mcr_psis, mcr_psis_dev, k_psis_column, k_psis_weights).

* Every output -- khat, ndraws_tail, lppd, elpd, p_loo and every log weight in time order, so that a wrong scatter shows --
  against the longdouble reference of tests/test_psis_refs_cpu.py under the project's gate, at the sizes where a path
  changes: the tail rules (1 .. 26, 225 / 226), one and two sort tiles (4096 / 4097), 16- against 32-bit positions
  (65535 .. 65537), past the bucket path (600 000), both sides of the LDS tail (8192 / 8193 of 20 000).
* In bits: alone against any place in a batch, host against device entry, layouts and a strided view, three workspace
  chunks, f32 against the widened f64, negate on v against -v, with and without weights.
* The device against mcr_psis_host; only the sort stage and the two new kernels run; errors leave the context usable;
  ragged chains are pooled; Context.loo, loo_file, loo_compare_files and the `loo` command.

Worst error seen on an MI355X over all gated cases: see DESIGN.md section 7 (the module prints it when it closes its context).
"""
from __future__ import annotations

import json
import math

import numpy as np
import pytest

from test_psis_refs_cpu import (DISTS, GATE, assert_reference_agrees, check, lse, psis_reference, same, tied_tail,
                                values)

pytestmark = pytest.mark.gpu

WORST = {"err": 0.0, "where": ""}
REFS: dict = {}                                              # the longdouble reference of a column, computed once


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()
    print(f"\nPSIS: worst error against longdouble {WORST['err']:.3e} ({WORST['where']})")


def call(ctx, x3, negate=False, r_eff=None, tails=None, weights=True, layout="pcn"):
    """Every output of mcr_psis / mcr_psis_dev (Context.psis and Context.loo each return a part)."""
    return ctx._psis_call(x3, layout, negate, r_eff, tails, weights)


def bits(r: dict) -> dict:
    out = {k: np.ascontiguousarray(r[k], dtype=np.float64).view(np.int64).tolist() for k in ("khat", "lppd", "elpd", "p_loo")}
    out["ndraws_tail"] = r["ndraws_tail"].tolist()
    if "log_weights" in r:
        out["log_weights"] = np.ascontiguousarray(r["log_weights"]).view(np.int64).tolist()
    return out


def scalars(b: dict) -> dict:
    return {k: v for k, v in b.items() if k != "log_weights"}


def part(b: dict, lo: int, hi: int) -> dict:
    return {k: v[lo:hi] for k, v in b.items()}


def chains_of(x: np.ndarray) -> np.ndarray:
    """[P][M] -> [P][C][N] with 4 chains where M allows, else one."""
    P, M = x.shape
    return x.reshape(P, 4, M // 4) if M % 4 == 0 else x.reshape(P, 1, M)


def sample(M: int, P: int, first: int = 0) -> np.ndarray:
    """P columns of M values, the distributions in turn from DISTS[first]; column p is values(dist, M, seed = 10 + p)."""
    return np.stack([values(DISTS[(first + p) % len(DISTS)], M, seed=10 + p) for p in range(P)])


def reference(col: np.ndarray, key, negate: bool, tail=None, r_eff=None) -> dict:
    k = (key, bool(negate), tail, r_eff)
    if k not in REFS:
        kw = {} if r_eff is None else {"r_eff": float(r_eff)}
        REFS[k] = assert_reference_agrees(col, k, negate=negate, ndraws_tail=tail, **kw)
    return REFS[k]


def gate(got: dict, x: np.ndarray, key, negate: bool, tails=None, r_eff=None):
    """Every output of every column of x[P][M] against the longdouble reference."""
    P = x.shape[0]
    for p in range(P):
        tail = None if tails is None else int(np.broadcast_to(tails, P)[p])
        r = None if r_eff is None else float(np.broadcast_to(r_eff, P)[p])
        ref = reference(x[p], (key, p), negate, tail, r)
        col = {k: got[k][p] for k in ("khat", "ndraws_tail", "lppd", "elpd", "p_loo")}
        if "log_weights" in got:
            col["log_weights"] = got["log_weights"][p]
        e = check(col, ref, (key, p, negate))
        if e > WORST["err"]:
            WORST["err"], WORST["where"] = e, f"{key} p={p} negate={negate}"
    print(f"{key} negate={negate}: worst error so far {WORST['err']:.3e}")


# ---- against longdouble --------------------------------------------------------------------------------------------------

SIZES = [1, 4, 5, 9, 10, 24, 25, 26, 225, 226, 4096, 4097, 65535, 65536, 65537]


@pytest.mark.parametrize("M", SIZES)
def test_sizes_against_longdouble(ctx, M):
    P = 3
    x = sample(M, P, first=SIZES.index(M))
    for negate in (False, True):
        got = call(ctx, chains_of(x), negate)
        assert got["log_weights"].shape == (P, M)
        gate(got, x, f"M = {M}", negate)
        if not negate:
            assert np.isnan(got["lppd"]).all() and np.isnan(got["elpd"]).all() and np.isnan(got["p_loo"]).all()
    assert got["khat_threshold"] == (1.0 - 1.0 / math.log10(M) if M > 1 else float("-inf"))


def test_past_the_bucket_path(ctx):
    x = values("normal3", 600_000, seed=3).reshape(1, -1)
    for negate in (False, True):
        gate(call(ctx, chains_of(x), negate), x, "M = 600000", negate)


def test_every_distribution(ctx):
    x = sample(20_000, len(DISTS))
    for negate in (False, True):
        got = call(ctx, chains_of(x), negate)
        gate(got, x, "nine distributions", negate)
    k = dict(zip(DISTS, call(ctx, chains_of(x))["khat"]))
    assert k["normal"] < 0.5 and k["cauchy5"] > 1.0 and k["constant"] == float("inf"), k


def test_both_sides_of_the_lds_tail(ctx, ffi):
    assert ffi.MCR_PARETO_LDS_TAIL == 8192
    x = sample(20_000, 2, first=2)                            # t3 and 5 Cauchy
    tails = np.array([8192, 8193], dtype=np.int64)
    for negate in (False, True):
        got = call(ctx, chains_of(x), negate, tails=tails)
        gate(got, x, "tails 8192 / 8193", negate, tails=tails)
        base = bits(got)
        for p in range(2):
            alone = bits(call(ctx, chains_of(x[p:p + 1]), negate, tails=tails[p:p + 1]))
            assert alone == part(base, p, p + 1), (negate, p)
    assert call(ctx, chains_of(x), tails=tails)["ndraws_tail"][0] == 8192
    other = call(ctx, chains_of(x[:1]), tails=8193)            # the same column from global memory
    gate(other, x[:1], "tail 8193 of column 0", False, tails=8193)


def test_r_eff_and_explicit_tails(ctx, ffi):
    x = sample(20_000, 3)
    r = [1.0, 0.5, 0.1]
    got = call(ctx, chains_of(x), True, r_eff=r)
    gate(got, x, "r_eff", True, r_eff=r)
    want = [ffi.psis_tail_length(20_000, v) for v in r]
    assert want == [425, 600, 1342]
    assert bits(got) == bits(call(ctx, chains_of(x), True, tails=want))
    assert bits(call(ctx, chains_of(x), True, r_eff=1.0)) == bits(call(ctx, chains_of(x), True))
    small = call(ctx, chains_of(x), tails=[1, 4, 5])
    assert small["khat"][0] == small["khat"][1] == float("inf") and np.isfinite(small["khat"][2])
    gate(small, x, "tails 1 / 4 / 5", False, tails=[1, 4, 5])
    with pytest.raises(ValueError, match="not both"):
        ctx.psis(chains_of(x), r_eff=1.0, ndraws_tail=5)


def test_tied_values_get_equal_weights(ctx):
    v = tied_tail()
    x = np.stack([v, np.round(values("normal", v.size, seed=4), 1)])
    got = call(ctx, chains_of(x))
    gate(got, x, "ties", False)
    s = np.sort(v)
    for val in (s[-19], s[-7]):
        w = got["log_weights"][0][v == val]
        assert w.size >= 3 and np.all(w == w[0])
    for p in range(2):                                         # a weight is a function of the value alone
        order = np.argsort(x[p], kind="stable")
        w, xs = got["log_weights"][p][order], x[p][order]
        assert np.all(np.diff(w) >= 0.0) and np.all(np.diff(w)[np.diff(xs) == 0.0] == 0.0)


# ---- one order of summation ---------------------------------------------------------------------------------------------

def test_place_in_the_batch_changes_no_bit(ctx):
    x = sample(5000, 9)
    for negate in (False, True):
        base = bits(call(ctx, chains_of(x), negate))
        for p in range(9):
            assert bits(call(ctx, chains_of(x[p:p + 1]), negate)) == part(base, p, p + 1), p
        nine = bits(call(ctx, chains_of(np.repeat(x[3:4], 9, axis=0)), negate))     # one column at each of nine places
        assert all(nine[k] == base[k][3:4] * 9 for k in base)


def test_routes_give_the_same_bits(ctx, ffi):
    P, M = 9, 65_536
    x = sample(M, P)
    x3 = chains_of(x)
    base = bits(call(ctx, x3, True))
    assert scalars(bits(call(ctx, x3, True, weights=False))) == scalars(base)          # with and without the weights
    t = ctx.upload(x3)
    try:
        assert bits(call(ctx, t, True)) == base                        # device entry: the weights in device memory
        assert scalars(bits(call(ctx, t, True, weights=False))) == scalars(base)
        assert ctx.psis_params_per_chunk(t) == P == ctx.psis_params_per_chunk(t, host_weights=True)
        cnp = np.ascontiguousarray(x3.transpose(1, 2, 0))              # the ingest pass
        assert bits(call(ctx, cnp, True, layout="cnp")) == base
        wide = np.zeros((P, 4, 2 * (M // 4)))                          # a strided view: every other draw of a wider array
        wide[:, :, ::2] = x3
        assert bits(call(ctx, wide[:, :, ::2], True)) == base
        with ffi.Context(0) as small:                                  # at least three workspace chunks
            ts = small.upload(x3)
            for mib4 in range(4, 256):
                small._check(small.lib.mcr_set_workspace_limit(small.handle, mib4 << 18))
                try:
                    per = small.psis_params_per_chunk(ts, host_weights=True)
                except ffi.McrError:
                    continue
                break
            print(f"{mib4 / 4} MiB workspace: {per} of {P} columns per chunk")
            assert 1 <= per <= 3 and small.psis_params_per_chunk(ts) >= per
            per_dev = small.psis_params_per_chunk(ts)
            small.profile(True)
            small.profile_reset()
            assert bits(call(small, ts, True)) == base
            prof = small.profile_get()
            assert prof["k_psis_column"]["launches"] == -(-P // per_dev) == prof["k_psis_weights"]["launches"]     # one per chunk
            small.profile_reset()
            assert bits(call(small, x3, True)) == base                 # the host entry: its chunks hold the weights too
            assert small.profile_get()["k_psis_column"]["launches"] == -(-P // per)
            small.profile(False)
            ts.free()
    finally:
        t.free()


def test_negation_and_f32(ctx):
    x = sample(20_000, len(DISTS))
    x3 = chains_of(x)
    loo = bits(call(ctx, x3, True))
    neg = bits(call(ctx, -x3, False))                                  # negate = 1 on v against negate = 0 on -v
    assert loo["khat"] == neg["khat"] and loo["ndraws_tail"] == neg["ndraws_tail"] and loo["log_weights"] == neg["log_weights"]
    x32 = x3.astype(np.float32)
    for negate in (False, True):
        want = bits(call(ctx, x32.astype(np.float64), negate))
        assert bits(call(ctx, x32, negate)) == want
        assert bits(call(ctx, np.ascontiguousarray(x32.transpose(1, 2, 0)), negate, layout="cnp")) == want
        t = ctx.upload(x32)
        try:
            assert bits(call(ctx, t, negate)) == want
        finally:
            t.free()


def test_device_against_the_host_routine(ctx, ffi):
    for M, P in ((26, 3), (4097, 3), (65_537, 2)):
        x = sample(M, P, first=1)
        for negate in (False, True):
            got = call(ctx, chains_of(x), negate)
            for p in range(P):
                host = ffi.psis_host(x[p], negate=negate)
                assert int(got["ndraws_tail"][p]) == host["ndraws_tail"]
                for k in ("khat", "lppd", "elpd", "p_loo"):
                    assert same(float(got[k][p]), host[k]), (M, p, k, got[k][p], host[k])
                d = np.abs(got["log_weights"][p] - host["log_weights"])
                assert np.all(d <= GATE * np.maximum(1.0, np.abs(host["log_weights"]))), (M, p, d.max())


def test_only_the_intended_kernels_run(ctx):
    x3 = chains_of(sample(65_536, 3))
    for weights in (True, False):
        ctx.profile(True)
        ctx.profile_reset()
        call(ctx, x3, True, weights=weights)
        prof = ctx.profile_get()
        ctx.profile(False)
        assert prof["k_psis_column"]["launches"] == 1 and prof["k_tile_sort"]["launches"] == 1
        assert prof.get("k_psis_weights", {"launches": 0})["launches"] == (1 if weights else 0)
        for name in ("k_rank_z", "k_fold_merge", "k_acov_seg", "k_acov_more", "k_acov_long", "k_diag", "k_diag_combine2",
                     "k_diag_long_scan", "k_fft", "k_chain_moments", "k_nested_combine", "k_pareto_fit", "k_hdi_window"):
            assert name not in prof or prof[name]["launches"] == 0, name


# ---- branches and errors -------------------------------------------------------------------------------------------------

def test_empty_shapes(ctx):
    empty = call(ctx, np.empty((2, 4, 0)), True)                        # M == 0
    assert all(np.isnan(empty[k]).all() and empty[k].shape == (2,) for k in ("khat", "lppd", "elpd", "p_loo"))
    assert empty["ndraws_tail"].tolist() == [0, 0] and empty["log_weights"].shape == (2, 0)
    none = call(ctx, np.empty((0, 4, 10)), True)                        # P == 0
    assert all(none[k].shape == (0,) for k in ("khat", "lppd", "elpd", "p_loo", "ndraws_tail")) and none["log_weights"].shape == (0, 40)
    one = ctx.psis(np.array([[[3.5]]]))
    assert one["log_weights"].tolist() == [[0.0]] and one["khat"][0] == float("inf") and one["ndraws_tail"][0] == 0


def test_errors_leave_the_context_usable(ctx, ffi):
    x3 = chains_of(sample(4096, 2))
    base = bits(call(ctx, x3, True))

    def still_works():
        assert bits(call(ctx, x3, True)) == base

    with pytest.raises(ffi.McrError, match=r"ndraws_tail\[1\] = 0") as e:
        ctx.psis(x3, ndraws_tail=[7, 0])
    assert e.value.code == ffi.MCR_EINVAL
    still_works()
    for bad_r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ffi.McrError, match=r"r_eff\[1\]") as e:
            ctx.loo(x3, r_eff=[1.0, bad_r])
        assert e.value.code == ffi.MCR_EINVAL
    still_works()
    for bad_value in (np.nan, np.inf, -np.inf):                         # a log ratio of -inf is refused like the others
        bad = x3.copy()
        bad[1, 2, 5] = bad_value
        for fn in (ctx.psis, ctx.loo):
            with pytest.raises(ffi.McrError) as e:
                fn(bad)
            assert e.value.code == ffi.MCR_ENONFINITE
        still_works()
    t = ctx.upload(x3)
    try:
        ctx.enqueue(t)                                                  # a summary in flight
        with pytest.raises(ffi.McrError, match="summaries in flight") as e:
            ctx.psis(t)
        assert e.value.code == ffi.MCR_EINVAL
        ctx.wait()
        assert bits(call(ctx, t, True)) == base
    finally:
        t.free()
    still_works()


# ---- Python, files and the command ---------------------------------------------------------------------------------------

def test_ragged_chains_are_pooled(ctx, ffi):
    from mcmc_ref_hip import diagnostics
    x = values("t3", 1000, seed=5)
    cuts = [0, 100, 350, 351, 1000]
    chains = [x[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    pooled = ctx.psis(x.reshape(1, 1, -1))
    one = diagnostics.psis_log_weights(chains, context=ctx)
    assert np.array_equal(one["log_weights"], pooled["log_weights"][0]) and one["khat"] == pooled["khat"][0]
    assert one["ndraws_tail"] == 95 and one["khat_threshold"] == 1.0 - 1.0 / 3.0 and one["min_ss"] == pooled["min_ss"][0]
    assert diagnostics.psis_log_weights(chains, ndraws_tail=40, context=ctx)["ndraws_tail"] == 40
    assert diagnostics.psis_log_weights(chains, r_eff=0.25, context=ctx)["ndraws_tail"] == 190
    buf = ffi.DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        ragged = ctx.ragged_tensor(buf, np.diff(cuts), 1)
        assert bits(call(ctx, ragged)) == bits(call(ctx, x.reshape(1, 1, -1)))
        assert ctx.loo(ragged)["elpd_loo"] == ctx.loo(x.reshape(1, 1, -1))["elpd_loo"]
    finally:
        buf.free()


def loo_model(P: int = 40, C: int = 4, N: int = 250, seed: int = 2, spread: float = 0.3) -> np.ndarray:
    """[P][C][N] pointwise log-likelihoods of P normal observations under C N posterior draws of their mean."""
    rng = np.random.default_rng(seed)
    y = rng.normal(size=P)
    mu = rng.normal(scale=spread, size=C * N)
    return (-0.5 * ((y[:, None] - mu[None, :]) ** 2 + math.log(2.0 * math.pi))).reshape(P, C, N)


def test_loo_totals(ctx, ffi):
    ll = loo_model()
    got = ctx.loo(ll)
    P = ll.shape[0]
    refs = [reference(ll[p].reshape(-1), ("loo model", p), True) for p in range(P)]
    elpd = [r["elpd"] for r in refs]
    assert same(got["elpd_loo"], math.fsum(elpd)) and same(got["p_loo"], math.fsum(r["p_loo"] for r in refs))
    assert same(got["lppd"], math.fsum(r["lppd"] for r in refs)) and same(got["se"], math.sqrt(P * np.var(elpd)))
    assert got["n_obs"] == P and got["n_draws"] == 1000 and sum(got["khat_counts"]) == P
    assert got["khat_counts"] == [int(np.count_nonzero((got["khat"] > a) & (got["khat"] <= b)))
                                  for a, b in ((-np.inf, 0.5), (0.5, 0.7), (0.7, 1.0), (1.0, np.inf))]
    assert got["elpd_loo"] == math.fsum(got["elpd_i"]) and got["elpd_loo"] < got["lppd"] and got["p_loo"] > 0.0
    for p in range(P):
        check({"khat": got["khat"][p], "ndraws_tail": got["ndraws_tail"][p], "elpd": got["elpd_i"][p], "lppd": got["lppd_i"][p],
               "p_loo": got["p_loo_i"][p]}, refs[p], ("loo pointwise", p))
    lean = ctx.loo(ll, pointwise=False)
    assert "elpd_i" not in lean and lean["elpd_loo"] == got["elpd_loo"] and lean["khat_counts"] == got["khat_counts"]
    assert ctx.loo(np.ascontiguousarray(ll.transpose(1, 2, 0)), "cnp")["elpd_loo"] == got["elpd_loo"]
    # the weights of psis on the negated log-likelihoods are the LOO weights: elpd_i is their weighted log mean
    w = ctx.psis(-ll)["log_weights"]
    for p in (0, P - 1):
        assert same(float(lse((w[p] + ll[p].reshape(-1)).astype(np.longdouble))), got["elpd_i"][p])


def write_table(path, ll: np.ndarray, extra: bool = True):
    P, C, N = ll.shape
    with path.open("w") as f:
        f.write("chain,draw," + ("mu," if extra else "") + ",".join(f"log_lik[{p + 1}]" for p in range(P)) + "\n")
        for i in range(C * N):
            row = [str(i // N), str(i % N)] + (["0.5"] if extra else []) + [repr(float(ll[p, i // N, i % N])) for p in range(P)]
            f.write(",".join(row) + "\n")


def test_loo_files_and_command(ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli, convert
    a, b = loo_model(P=12, N=100), loo_model(P=12, N=100, spread=1.0)
    pa, pb = tmp_path / "a.csv", tmp_path / "b.csv"
    write_table(pa, a)
    write_table(pb, b, extra=False)
    ra, rb = ctx.loo(a), ctx.loo(b)
    fa = convert.loo_file(pa, context=ctx)
    assert fa["names"] == [f"log_lik[{p + 1}]" for p in range(12)] and fa["elpd_loo"] == ra["elpd_loo"] and fa["n_obs"] == 12
    assert np.array_equal(fa["khat"], ra["khat"])
    assert convert.loo_file(pa, params=["log_lik[2]", "mu"], context=ctx)["n_obs"] == 1
    with pytest.raises(ValueError, match="no column starts with"):
        convert.loo_file(pa, prefix="nope", context=ctx)
    cmp_ = convert.loo_compare_files(pa, pb, context=ctx)
    diff = ra["elpd_i"] - rb["elpd_i"]
    assert cmp_["elpd_diff"] == math.fsum(diff) and cmp_["se_diff"] == math.sqrt(12 * float(np.var(diff)))
    assert cmp_["elpd_diff"] > 0.0                                     # the tighter posterior predicts better
    short = tmp_path / "short.csv"
    write_table(short, b[:11], extra=False)
    with pytest.raises(ValueError, match="12 and 11 observations"):
        convert.loo_compare_files(pa, short, context=ctx)
    res = CliRunner().invoke(cli.main, ["loo", str(pa), "--format", "json", "--pointwise"])
    assert res.exit_code == 0, res.output
    out = json.loads(res.output)
    assert out["elpd_loo"] == ra["elpd_loo"] and out["se"] == ra["se"] and out["khat_counts"] == ra["khat_counts"]
    assert out["n_obs"] == 12 and out["n_draws"] == 400 and out["pointwise"]["log_lik[3]"]["elpd"] == float(ra["elpd_i"][2])
    res = CliRunner().invoke(cli.main, ["loo", str(pa), "--against", str(pb)])
    assert res.exit_code == 0 and f"elpd_diff {cmp_['elpd_diff']:.6g}" in res.output and f"elpd_loo {ra['elpd_loo']:.6g}" in res.output
    res = CliRunner().invoke(cli.main, ["loo", str(pa), "--against", str(pb), "--format", "json"])
    assert res.exit_code == 0 and json.loads(res.output)["against"]["elpd_loo"] == rb["elpd_loo"]
    res = CliRunner().invoke(cli.main, ["loo", str(pa), "--pointwise"])
    assert res.exit_code == 0 and "log_lik[12]" in res.output and "khat" in res.output
    res = CliRunner().invoke(cli.main, ["loo", str(pa), "--prefix", "nope"])
    assert res.exit_code != 0 and "no column starts with" in res.output
    res = CliRunner().invoke(cli.main, ["loo", str(pa), "--against", str(short)])
    assert res.exit_code != 0 and "observations" in res.output
