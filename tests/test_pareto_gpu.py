"""Pareto k-hat on the GPU (mcr_pareto_khat, mcr_pareto_khat_dev, k_pareto_fit).

* Every output against tests/test_pareto_refs_cpu.py's reference in longdouble: |got - ref| <= 1e-9 max(1, |ref|); NaN,
  +inf and the tail lengths exactly.  Shapes: the smallest at which a path changes (the t < 5 rule, the switch of the
  default tail length, one / two sort tiles, 16- against 32-bit positions, past the bucket path) and the kernel's own
  edges (lanes without an exceedance, one and two rounds of the workgroup, both sides of MCR_PARETO_LDS_TAIL).
* One order of summation: alone or at any place in a batch, host / device entry, either layout, a strided view, any
  workspace chunking, f32 against the widened f64, x against 4 x, the left tail against the right tail of -x -- in bits.
* Only the sort stage and k_pareto_fit run.  Branches, errors that leave the context usable, the Python functions,
  validate(khat_max=) and the `pareto-khat` command.

Worst error seen on an MI355X over all gated cases: see DESIGN.md section 7 (the test prints it).
"""
from __future__ import annotations

import json
import math

import numpy as np
import pytest

from test_pareto_refs_cpu import (DISTS, constant_right_tail, draws, err_of, pareto_reference, same, ties_at_cutoff)

pytestmark = pytest.mark.gpu

KEYS = ("khat", "khat_left", "khat_right")
WORST = {"err": 0.0, "where": ""}


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()
    print(f"\nPareto k-hat: worst error against longdouble {WORST['err']:.3e} ({WORST['where']})")


def bits(r: dict) -> dict:
    out = {k: np.ascontiguousarray(r[k], dtype=np.float64).view(np.int64).tolist() for k in KEYS}
    out["ndraws_tail"] = r["ndraws_tail"].tolist()
    return out


def chains_of(x: np.ndarray) -> np.ndarray:
    """[P][M] -> [P][C][N] with 4 chains where M allows, else one."""
    P, M = x.shape
    return x.reshape(P, 4, M // 4) if M % 4 == 0 else x.reshape(P, 1, M)


def gate(got: dict, x: np.ndarray, what: str, tails=None):
    """Every output of every parameter of x[P][M] against the longdouble reference."""
    for p in range(x.shape[0]):
        ref = pareto_reference(x[p], None if tails is None else int(np.broadcast_to(tails, x.shape[0])[p]), np.longdouble)
        assert int(got["ndraws_tail"][p]) == ref["ndraws_tail"], (what, p, got["ndraws_tail"][p], ref)
        for k in KEYS:
            g, r = float(got[k][p]), ref[k]
            e = err_of(g, r)
            if e > WORST["err"]:
                WORST["err"], WORST["where"] = e, f"{what} p={p} {k}"
            assert same(g, r), (what, p, k, g, r)
    print(f"{what}: worst error so far {WORST['err']:.3e}")


def sample(M: int, P: int, first: int = 0) -> np.ndarray:
    """P parameters of M draws, the distributions in turn from DISTS[first]."""
    return np.stack([draws(DISTS[(first + p) % len(DISTS)], M, seed=10 + p) for p in range(P)])


# ---- against longdouble --------------------------------------------------------------------------------------------------

SHAPES = [(9, 2), (10, 2), (11, 2), (225, 2), (226, 2), (4096, 3), (4097, 3), (65535, 3), (65536, 3), (600_000, 1)]


@pytest.mark.parametrize("M,P", SHAPES)
def test_shapes_against_longdouble(ctx, M, P):
    x = sample(M, P, first=SHAPES.index((M, P)))
    got = ctx.pareto_khat(chains_of(x))
    gate(got, x, f"M = {M}")
    assert got["khat_threshold"] == 1.0 - 1.0 / math.log10(M)


def test_every_distribution(ctx):
    x = sample(20_000, len(DISTS))
    got = ctx.pareto_khat(chains_of(x))
    gate(got, x, "five distributions")
    k = dict(zip(DISTS, got["khat"]))
    assert k["normal"] < 0.3 and k["cauchy"] > 0.8, k                 # light and heavy tails are told apart
    assert got["min_ss"][DISTS.index("normal")] == 10.0 ** (1.0 / (1.0 - max(0.0, k["normal"])))


TAILS = [5, 63, 64, 65, 255, 256, 257, 8192, 8193]


def test_explicit_tail_lengths(ctx, ffi):
    """Lanes without an exceedance (5, 63), one wave exactly (64), a second round of lanes (65), the workgroup's 16 waves
    and grid points (255 .. 257), both sides of the LDS tail -- as nine parameters with nine lengths in one call, and alone."""
    assert ffi.MCR_PARETO_LDS_TAIL == 8192
    x = sample(20_000, len(TAILS), first=1)
    tails = np.array(TAILS, dtype=np.int64)
    got = ctx.pareto_khat(chains_of(x), ndraws_tail=tails)
    gate(got, x, "explicit tails", tails)
    assert got["ndraws_tail"].tolist() == TAILS
    base = bits(got)
    for lo, hi in ((0, 1), (0, 8), (8, 9), (7, 9)):                    # P = 1, 8 and the two sides of the LDS tail alone
        part = bits(ctx.pareto_khat(chains_of(x[lo:hi]), ndraws_tail=tails[lo:hi]))
        assert all(part[k] == base[k][lo:hi] for k in base), (lo, hi)
    one = ctx.pareto_khat(chains_of(x), ndraws_tail=257)              # a scalar serves every parameter
    assert one["ndraws_tail"].tolist() == [257] * len(TAILS) and bits(one)["khat"][6] == base["khat"][6]


def test_cap_at_half_the_draws(ctx):
    x = sample(4096, 2, first=2)
    a, b = ctx.pareto_khat(chains_of(x), ndraws_tail=2048), ctx.pareto_khat(chains_of(x), ndraws_tail=2049)
    assert a["ndraws_tail"].tolist() == [2048, 2048] == b["ndraws_tail"].tolist() and bits(a) == bits(b)
    gate(a, x, "ndraws_tail = M / 2", 2048)
    odd = sample(4097, 1)
    assert ctx.pareto_khat(chains_of(odd), ndraws_tail=10 ** 9)["ndraws_tail"].tolist() == [2048]


def test_r_eff(ctx, ffi):
    x = sample(20_000, 3)
    r = ctx.pareto_khat(chains_of(x), r_eff=[1.0, 0.5, 0.1])
    want = [ffi.pareto_tail_length(20_000, v) for v in (1.0, 0.5, 0.1)]
    assert r["ndraws_tail"].tolist() == want == [425, 600, 1342]
    assert bits(r) == bits(ctx.pareto_khat(chains_of(x), ndraws_tail=want))
    assert bits(ctx.pareto_khat(chains_of(x), r_eff=1.0)) == bits(ctx.pareto_khat(chains_of(x)))
    with pytest.raises(ValueError, match="not both"):
        ctx.pareto_khat(chains_of(x), r_eff=1.0, ndraws_tail=5)


# ---- one order of summation ---------------------------------------------------------------------------------------------

def test_place_in_the_batch_changes_no_bit(ctx):
    x = sample(5000, 9)
    base = bits(ctx.pareto_khat(chains_of(x)))
    for p in range(9):
        alone = bits(ctx.pareto_khat(chains_of(x[p:p + 1])))
        assert all(alone[k][0] == base[k][p] for k in base), p
    same_nine = bits(ctx.pareto_khat(chains_of(np.repeat(x[3:4], 9, axis=0))))     # one parameter at each of nine places
    assert all(same_nine[k] == [base[k][3]] * 9 for k in base)


def test_routes_give_the_same_bits(ctx, ffi):
    P, M = 9, 65_536
    x = sample(M, P)
    x3 = chains_of(x)
    base = bits(ctx.pareto_khat(x3))
    t = ctx.upload(x3)
    try:
        assert bits(ctx.pareto_khat(t)) == base                         # device entry
        assert ctx.pareto_params_per_chunk(t) == P
        cnp = np.ascontiguousarray(x3.transpose(1, 2, 0))               # the ingest pass
        assert bits(ctx.pareto_khat(cnp, "cnp")) == base
        wide = np.zeros((P, 4, 2 * (M // 4)))                           # a strided view: every other draw of a wider array
        wide[:, :, ::2] = x3
        assert bits(ctx.pareto_khat(wide[:, :, ::2])) == base
        with ffi.Context(0) as small:                                   # at least three workspace chunks
            ts = small.upload(x3)
            for mib4 in range(4, 256):
                small._check(small.lib.mcr_set_workspace_limit(small.handle, mib4 << 18))
                try:
                    per = small.pareto_params_per_chunk(ts)
                except ffi.McrError:
                    continue
                break
            print(f"{mib4 / 4} MiB workspace: {per} of {P} parameters per chunk")
            assert 1 <= per <= 3
            small.profile(True)
            small.profile_reset()
            assert bits(small.pareto_khat(ts)) == base
            assert small.profile_get()["k_pareto_fit"]["launches"] == -(-P // per)      # one launch per chunk
            small.profile(False)
            assert bits(small.pareto_khat(x3)) == base
            ts.free()
    finally:
        t.free()


def test_scaling_negation_and_f32(ctx):
    x = sample(20_000, len(DISTS))
    x3 = chains_of(x)
    base = bits(ctx.pareto_khat(x3))
    assert bits(ctx.pareto_khat(4.0 * x3)) == base                      # a power of two scales nothing
    neg = bits(ctx.pareto_khat(-x3))                                    # the left tail is the right tail of -x
    assert neg["khat_left"] == base["khat_right"] and neg["khat_right"] == base["khat_left"] and neg["khat"] == base["khat"]
    x32 = x3.astype(np.float32)
    want = bits(ctx.pareto_khat(x32.astype(np.float64)))
    assert bits(ctx.pareto_khat(x32)) == want
    assert bits(ctx.pareto_khat(np.ascontiguousarray(x32.transpose(1, 2, 0)), "cnp")) == want
    t = ctx.upload(x32)
    try:
        assert bits(ctx.pareto_khat(t)) == want
    finally:
        t.free()


def test_only_the_intended_kernels_run(ctx):
    x3 = chains_of(sample(65_536, 3))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.pareto_khat(x3)
    prof = ctx.profile_get()
    ctx.profile(False)
    assert prof["k_pareto_fit"]["launches"] == 1 and prof["k_tile_sort"]["launches"] == 1
    for name in ("k_rank_z", "k_fold_merge", "k_acov_seg", "k_acov_more", "k_acov_long", "k_diag", "k_diag_combine2",
                 "k_diag_long_scan", "k_fft", "k_chain_moments", "k_nested_combine"):
        assert name not in prof or prof[name]["launches"] == 0, name


# ---- branches and errors -------------------------------------------------------------------------------------------------

def test_branches(ctx):
    inf = float("inf")
    M = 1000
    x = np.stack([np.full(M, 2.5), constant_right_tail(M), ties_at_cutoff(M), -ties_at_cutoff(M)])
    got = ctx.pareto_khat(chains_of(x))
    gate(got, x, "branches")
    assert all(np.isnan(got[k][0]) for k in KEYS)                        # a constant parameter
    assert np.isnan(got["khat_right"][1]) and np.isfinite(got["khat_left"][1]) and got["khat"][1] == got["khat_left"][1]
    assert got["khat_right"][2] == inf and np.isfinite(got["khat_left"][2]) and got["khat"][2] == inf      # xstar == 0
    assert got["khat_left"][3] == inf
    assert np.isnan(got["min_ss"][0]) and got["min_ss"][2] == inf
    empty = ctx.pareto_khat(np.empty((2, 4, 0)))                        # M == 0
    assert all(np.isnan(empty[k]).all() and empty[k].shape == (2,) for k in KEYS) and empty["ndraws_tail"].tolist() == [0, 0]
    none = ctx.pareto_khat(np.empty((0, 4, 10)))                        # P == 0
    assert all(none[k].shape == (0,) for k in KEYS + ("ndraws_tail", "min_ss"))


def test_errors_leave_the_context_usable(ctx, ffi):
    x3 = chains_of(sample(4096, 2))
    base = bits(ctx.pareto_khat(x3))

    def still_works():
        assert bits(ctx.pareto_khat(x3)) == base

    with pytest.raises(ffi.McrError, match=r"ndraws_tail\[1\] = 0") as e:
        ctx.pareto_khat(x3, ndraws_tail=[7, 0])
    assert e.value.code == ffi.MCR_EINVAL
    still_works()
    bad = x3.copy()
    bad[1, 2, 5] = np.nan
    with pytest.raises(ffi.McrError) as e:
        ctx.pareto_khat(bad)
    assert e.value.code == ffi.MCR_ENONFINITE
    still_works()
    bad[1, 2, 5] = np.inf
    with pytest.raises(ffi.McrError) as e:
        ctx.pareto_khat(bad)
    assert e.value.code == ffi.MCR_ENONFINITE
    still_works()
    t = ctx.upload(x3)
    try:
        ctx.enqueue(t)                                                  # a summary in flight
        with pytest.raises(ffi.McrError, match="summaries in flight") as e:
            ctx.pareto_khat(t)
        assert e.value.code == ffi.MCR_EINVAL
        ctx.wait()
        assert bits(ctx.pareto_khat(t)) == base
    finally:
        t.free()
    still_works()


# ---- Python, validate and the command ------------------------------------------------------------------------------------

def test_ragged_chains_are_pooled(ctx, ffi):
    from mcmc_ref_hip import diagnostics
    x = draws("t2", 1000, seed=5)
    cuts = [0, 100, 350, 351, 1000]
    chains = [x[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    pooled = ctx.pareto_khat(x.reshape(1, 1, -1))
    assert diagnostics.pareto_khat(chains, context=ctx) == pooled["khat"][0]
    detail = diagnostics.pareto_khat_detail(chains, context=ctx)
    assert detail == {"khat": pooled["khat"][0], "khat_left": pooled["khat_left"][0], "khat_right": pooled["khat_right"][0],
                      "min_ss": pooled["min_ss"][0], "ndraws_tail": 95, "khat_threshold": 1.0 - 1.0 / 3.0}
    assert diagnostics.pareto_khat_detail(chains, ndraws_tail=40, context=ctx)["ndraws_tail"] == 40
    assert diagnostics.pareto_khat_detail(chains, r_eff=0.25, context=ctx)["ndraws_tail"] == 190
    buf = ffi.DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        ragged = ctx.ragged_tensor(buf, np.diff(cuts), 1)
        assert bits(ctx.pareto_khat(ragged)) == bits(pooled)
    finally:
        buf.free()


def test_validate_gates_on_khat_only_when_asked(ctx, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    from mcmc_ref_hip.validate import validate
    (tmp_path / "draws").mkdir()
    (tmp_path / "meta").mkdir()
    rng = np.random.default_rng(9)
    pq.write_table(pa.table({"chain": np.repeat(np.arange(4), 1000), "draw": np.tile(np.arange(1000), 4),
                             "a": rng.normal(size=4000), "b": rng.normal(size=4000)}), tmp_path / "draws" / "tails.draws.parquet")
    (tmp_path / "meta" / "tails.meta.json").write_text(json.dumps({"diagnostics": {}}))
    store = DataStore(local_root=tmp_path, packaged_root=tmp_path / "none")
    actual = {"a": rng.normal(size=4000), "b": rng.standard_cauchy(size=4000)}
    free = validate("tails", actual, store=store, context=ctx)
    assert free.passed == free.compare.passed and free.failures == list(free.compare.failures)
    assert set(free.khat_ref) == set(free.khat_actual) == {"a", "b"}
    assert max(free.khat_ref.values()) < 0.5 and free.khat_actual["a"] < 0.5 and free.khat_actual["b"] > 0.7, free
    assert free.khat_actual["b"] == ctx.pareto_khat(actual["b"].reshape(1, 1, -1))["khat"][0]
    gated = validate("tails", actual, store=store, context=ctx, khat_max=0.7)
    extra = [f for f in gated.failures if f not in free.failures]
    assert not gated.passed and len(extra) == 1 and extra[0].startswith("b.khat_actual=") and extra[0].endswith("> 0.7")
    # a gate so wide that mean and std pass: the k-hat threshold alone decides
    wide = validate("tails", actual, tolerance=1e12, store=store, context=ctx)
    assert wide.passed and wide.khat_actual == free.khat_actual
    wide_gated = validate("tails", actual, tolerance=1e12, store=store, context=ctx, khat_max=0.7)
    assert not wide_gated.passed and [f.split("=")[0] for f in wide_gated.failures] == ["b.khat_actual"]
    uneven = validate("tails", {"a": actual["a"], "b": actual["b"][:-1]}, store=store, context=ctx)     # no joint draws needed
    assert uneven.khat_actual["a"] == free.khat_actual["a"]


def test_pareto_khat_command(ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli
    C, N = 4, 250
    x = np.stack([draws("normal", C * N, seed=2), draws("cauchy", C * N, seed=2)])
    path = tmp_path / "draws.csv"
    with path.open("w") as f:
        f.write("chain,draw,light,heavy\n")
        for i in range(C * N):
            f.write(f"{i // N},{i % N},{float(x[0, i])!r},{float(x[1, i])!r}\n")
    want = ctx.pareto_khat(x.reshape(2, 1, -1))
    res = CliRunner().invoke(cli.main, ["pareto-khat", str(path), "--format", "json"])
    assert res.exit_code == 0, res.output
    out = json.loads(res.output)
    assert set(out) == {"light", "heavy"} and set(out["light"]) == {"khat", "khat_left", "khat_right", "ndraws_tail", "min_ss"}
    for i, name in enumerate(("light", "heavy")):
        assert out[name]["ndraws_tail"] == 95
        for k in KEYS + ("min_ss",):
            assert out[name][k] == float(want[k][i]), (name, k)
    res = CliRunner().invoke(cli.main, ["pareto-khat", str(path), "--params", "heavy", "--tail-draws", "50"])
    assert res.exit_code == 0 and "khat_left" in res.output and "light" not in res.output
    assert f"{float(ctx.pareto_khat(x[1].reshape(1, 1, -1), ndraws_tail=50)['khat'][0]):.6g}" in res.output
    res = CliRunner().invoke(cli.main, ["pareto-khat", str(path), "--params", "nope"])
    assert res.exit_code != 0 and "Unknown parameter" in res.output
    res = CliRunner().invoke(cli.main, ["pareto-khat", str(path), "--tail-draws", "0"])
    assert res.exit_code != 0 and "must be >= 1" in res.output
