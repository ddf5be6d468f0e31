"""Highest-density intervals on the GPU (mcr_hdi, mcr_hdi_dev, k_hdi_window, k_hdi_pick).

* Every output against tests/test_hdi_refs_cpu.py's numpy reference: `index` exactly, `lo` / `hi` with ==.  There is no
  tolerance because the definition leaves no rounding choice open.  Shapes: the smallest at which a path changes -- fewer
  draws than a wave, a workgroup's thread count +-1 windows, MCR_HDI_SLICE -1 / +0 / +1 and two slices + 1 windows (even
  and odd offsets: the wide and the plain loads; odd M: a parameter whose keys start off a 16-byte boundary), and the sort
  plan's switches of tests/test_pareto_gpu.py.  The tied generator is among the parameters of every case.
* One answer on every route: alone or at any place in a batch, host / device entry, either layout, a strided view, any
  workspace chunking, f32 against the widened f64, x against 4 x, x against -x -- in bits, `index` exactly.
* Only the sort stage and the two new kernels run.  Errors that leave the context usable, empty shapes, the Python
  functions, the `hdi` command and validate(hdi_prob=, hdi_tol=).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
from pathlib import Path

import numpy as np
import pytest

from test_hdi_refs_cpu import GENERATORS, draws, hdi_reference, windows

pytestmark = pytest.mark.gpu

KEYS = ("lo", "hi", "index")
NT = 256                                                     # threads of a k_hdi_window workgroup


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()


def bits(r: dict) -> dict:
    out = {k: np.ascontiguousarray(r[k], dtype=np.float64).view(np.int64).tolist() for k in ("lo", "hi")}
    out["index"] = np.asarray(r["index"]).tolist()
    return out


def chains_of(x: np.ndarray) -> np.ndarray:
    """[P][M] -> [P][C][N] with 4 chains where M allows, else one."""
    P, M = x.shape
    return x.reshape(P, 4, M // 4) if M % 4 == 0 else x.reshape(P, 1, M)


def sample(M: int, P: int, first: int = 3) -> np.ndarray:
    """P parameters of M draws, the generators in turn from GENERATORS[first] (3: the tied one first)."""
    return np.stack([draws(GENERATORS[(first + p) % len(GENERATORS)], M, seed=10 + p) for p in range(P)])


def gate(got: dict, x: np.ndarray, probs, what: str):
    """Every output of every parameter of x[P][M] and every probability against the numpy reference: exactly."""
    probs = list(np.atleast_1d(probs))
    for p in range(x.shape[0]):
        for j, q in enumerate(probs):
            lo, hi, idx = hdi_reference(x[p], q)
            g = tuple(np.asarray(got[k]).reshape(x.shape[0], -1)[p, j] for k in KEYS)
            assert int(g[2]) == idx, (what, p, q, g, (lo, hi, idx))
            if idx < 0:
                assert math.isnan(g[0]) and math.isnan(g[1])
            else:
                assert g[0] == lo and g[1] == hi, (what, p, q, g, (lo, hi, idx))


# ---- against numpy --------------------------------------------------------------------------------------------------------

PROBS3 = [0.94, 0.5, 0.1]


@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65])
def test_few_draws(ctx, M):
    x = sample(M, 3)
    gate(ctx.hdi(chains_of(x), prob=PROBS3), x, PROBS3, f"M = {M}")


def at_half(W: int, odd: bool) -> int:
    """The M whose prob = 0.5 call has W windows: 2 W (inc = W), or the odd 2 W - 1 (inc = W - 1)."""
    M = 2 * W - 1 if odd else 2 * W
    assert windows(M, 0.5) == W
    return M


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("W", [NT - 1, NT, NT + 1])
def test_a_workgroup_of_windows(ctx, W, odd):
    M = at_half(W, odd)
    x = sample(M, 3)
    gate(ctx.hdi(chains_of(x), prob=[0.5, 0.94]), x, [0.5, 0.94], f"W = {W}, M = {M}")


def slice_edges(ffi):
    S = ffi.MCR_HDI_SLICE
    return [S - 1, S, S + 1, 2 * S + 1]


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("edge", range(4))
def test_slice_edges(ctx, ffi, edge, odd):
    """One slice less a window, one slice, a second slice of one window, a third slice of one window -- with an even and
    an odd offset (wide and plain loads), and with odd M three parameters whose keys start on and off a 16-byte boundary."""
    W = slice_edges(ffi)[edge]
    M = at_half(W, odd)
    x = sample(M, 3)
    got = ctx.hdi(chains_of(x), prob=[0.5, 0.9])
    gate(got, x, [0.5, 0.9], f"W = {W}, M = {M}")
    if edge >= 2:                                                       # the narrowest window is the last: a slice of ONE window
        inc = M - W
        gaps = np.ones(M - 1)
        gaps[M - 2] = 0.5                                               # only the last window holds the last gap
        y = np.concatenate([[0.0], np.cumsum(gaps)])                    # (multiples of 0.5: exact)
        y = np.stack([x[0], np.random.default_rng(1).permutation(y)])
        r = ctx.hdi(chains_of(y), prob=0.5)
        assert r["index"][1] == W - 1 and r["hi"][1] - r["lo"][1] == inc - 0.5
        gate(r, y, 0.5, f"W = {W}: the last window")


SHAPES = [(4096, 3), (4097, 3), (65535, 3), (65536, 3), (600_000, 1)]


@pytest.mark.parametrize("M,P", SHAPES)
def test_sort_plan_switches(ctx, M, P):
    x = sample(M, P)
    gate(ctx.hdi(chains_of(x), prob=PROBS3), x, PROBS3, f"M = {M}")


def test_every_generator(ctx):
    x = sample(20_000, len(GENERATORS), first=0)
    got = ctx.hdi(chains_of(x))                                         # the default: 0.94, [P] arrays
    assert got["prob"] == 0.94 and all(got[k].shape == (len(GENERATORS),) for k in KEYS)
    gate(got, x, 0.94, "five generators")
    e = GENERATORS.index("exponential")
    q3, q97 = np.quantile(x[e], [0.03, 0.97])
    assert got["lo"][e] < q3 and got["hi"][e] < q97
    half = ctx.hdi(chains_of(x), prob=0.5)
    b = GENERATORS.index("bimodal")
    assert -4.0 < half["lo"][b] < half["hi"][b] < 0.0                   # on the heavier mode
    assert half["index"][GENERATORS.index("constant")] == 0


# ---- probabilities ----------------------------------------------------------------------------------------------------------

def test_probabilities_in_one_call(ctx, ffi):
    x = sample(5000, 4)
    x3 = chains_of(x)
    single = {}

    def one(q):
        if q not in single:
            single[q] = bits(ctx.hdi(x3, prob=q))
        return single[q]

    sixteen = [0.94, 0.5, 0.03, 0.999, 0.5, 0.25, 0.9, 0.89, 0.0001, 0.75, 0.6, 0.94, 0.3333, 0.8, 0.95, 0.4]
    assert len(sixteen) == ffi.MCR_HDI_MAX_PROBS
    for probs in ([0.7], [0.94, 0.5], sixteen):                         # unsorted, with repeats
        got = ctx.hdi(x3, prob=probs)
        assert all(got[k].shape == (4, len(probs)) for k in KEYS) and list(got["prob"]) == probs
        gate(got, x, probs, f"{len(probs)} probabilities")
        b = bits(got)
        for j, q in enumerate(probs):
            assert all([row[j] for row in b[k]] == one(q)[k] for k in KEYS), (probs, j)


# ---- one answer on every route ----------------------------------------------------------------------------------------------

def test_place_in_the_batch_changes_no_bit(ctx):
    x = sample(5001, 9)                                                 # odd M: the keys of every other parameter start off 16 bytes
    probs = [0.5, 0.94]
    base = bits(ctx.hdi(chains_of(x), prob=probs))
    for p in range(9):
        alone = bits(ctx.hdi(chains_of(x[p:p + 1]), prob=probs))
        assert all(alone[k][0] == base[k][p] for k in KEYS), p
    eight = bits(ctx.hdi(chains_of(x[:8]), prob=probs))
    assert all(eight[k] == base[k][:8] for k in KEYS)
    same_nine = bits(ctx.hdi(chains_of(np.repeat(x[3:4], 9, axis=0)), prob=probs))        # one parameter at each of nine places
    assert all(same_nine[k] == [base[k][3]] * 9 for k in KEYS)


def test_routes_give_the_same_bits(ctx, ffi):
    P, M = 9, 65_536
    probs = [0.5, 0.94]
    x = sample(M, P)
    x3 = chains_of(x)
    got = ctx.hdi(x3, prob=probs)
    gate(got, x, probs, "routes")
    base = bits(got)
    t = ctx.upload(x3)
    try:
        assert bits(ctx.hdi(t, prob=probs)) == base                     # device entry
        assert ctx.hdi_params_per_chunk(t, 2) == P
        cnp = np.ascontiguousarray(x3.transpose(1, 2, 0))               # the ingest pass
        assert bits(ctx.hdi(cnp, "cnp", prob=probs)) == base
        wide = np.zeros((P, 4, 2 * (M // 4)))                           # a strided view: every other draw of a wider array
        wide[:, :, ::2] = x3
        assert bits(ctx.hdi(wide[:, :, ::2], prob=probs)) == base
        with ffi.Context(0) as small:                                   # 1, 2 and 3 parameters per workspace chunk
            ts = small.upload(x3)
            limits = {}
            for mib in range(1, 16):                                    # (a parameter needs ~1.6 MiB: no count is stepped over)
                small._check(small.lib.mcr_set_workspace_limit(small.handle, mib << 20))
                try:
                    limits.setdefault(small.hdi_params_per_chunk(ts, 2), mib)
                except ffi.McrError:
                    continue
            assert {1, 2, 3} <= set(limits), limits
            small.profile(True)
            for per in (1, 2, 3):
                small._check(small.lib.mcr_set_workspace_limit(small.handle, limits[per] << 20))
                assert small.hdi_params_per_chunk(ts, 2) == per
                small.profile_reset()
                assert bits(small.hdi(ts, prob=probs)) == base, per
                prof = small.profile_get()
                chunks = -(-P // per)
                assert prof["k_hdi_window"]["launches"] == chunks and prof["k_hdi_pick"]["launches"] == chunks, (per, prof)
            small.profile(False)
            assert bits(small.hdi(x3, prob=probs)) == base              # the host entry in chunks
            ts.free()
    finally:
        t.free()


def test_scaling_negation_and_f32(ctx):
    x = sample(20_001, len(GENERATORS), first=0)
    x3 = chains_of(x)
    probs = [0.5, 0.94]
    base = ctx.hdi(x3, prob=probs)
    four = ctx.hdi(4.0 * x3, prob=probs)                                # a power of two moves no comparison
    assert four["index"].tolist() == base["index"].tolist()
    assert np.array_equal(four["lo"], 4.0 * base["lo"]) and np.array_equal(four["hi"], 4.0 * base["hi"])
    free = [i for i, g in enumerate(GENERATORS) if g in ("normal", "exponential", "bimodal")]      # tie-free input
    neg = ctx.hdi(-x3[free], prob=probs)                                # mirrored: the same windows from the other end
    M = x.shape[1]
    inc = np.array([int(math.floor(q * M)) for q in probs])
    assert np.array_equal(neg["lo"], -base["hi"][free]) and np.array_equal(neg["hi"], -base["lo"][free])
    assert np.array_equal(neg["index"], (M - 1) - (base["index"][free] + inc))
    x32 = x3.astype(np.float32)
    want = bits(ctx.hdi(x32.astype(np.float64), prob=probs))
    assert bits(ctx.hdi(x32, prob=probs)) == want
    assert bits(ctx.hdi(np.ascontiguousarray(x32.transpose(1, 2, 0)), "cnp", prob=probs)) == want
    t = ctx.upload(x32)
    try:
        assert bits(ctx.hdi(t, prob=probs)) == want
    finally:
        t.free()


def test_only_the_intended_kernels_run(ctx):
    x3 = chains_of(sample(65_536, 3))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.hdi(x3, prob=PROBS3)
    prof = ctx.profile_get()
    ctx.profile(False)
    assert prof["k_hdi_window"]["launches"] == 1 and prof["k_hdi_pick"]["launches"] == 1 and prof["k_tile_sort"]["launches"] == 1
    for name in ("k_rank_z", "k_fold_merge", "k_acov_seg", "k_acov_more", "k_acov_long", "k_diag", "k_diag_combine2",
                 "k_diag_long_scan", "k_fft", "k_chain_moments", "k_nested_combine", "k_pareto_fit"):
        assert name not in prof or prof[name]["launches"] == 0, name


# ---- errors and empty shapes ---------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(ctx, ffi):
    x3 = chains_of(sample(4096, 2))
    base = bits(ctx.hdi(x3))

    def still_works():
        assert bits(ctx.hdi(x3)) == base

    bad = x3.copy()
    for v in (np.nan, np.inf, -np.inf):
        bad[1, 2, 5] = v
        with pytest.raises(ffi.McrError) as e:
            ctx.hdi(bad)
        assert e.value.code == ffi.MCR_ENONFINITE
        still_works()
    for q in (0.0, 1.0, -0.1, float("nan"), [0.5, 1.5], [], [0.5] * 17):
        with pytest.raises(ffi.McrError) as e:
            ctx.hdi(x3, prob=q)
        assert e.value.code == ffi.MCR_EINVAL, q
    still_works()
    t = ctx.upload(x3)
    try:
        ctx.enqueue(t)                                                  # a summary in flight
        with pytest.raises(ffi.McrError, match="summaries in flight") as e:
            ctx.hdi(t)
        assert e.value.code == ffi.MCR_EINVAL
        ctx.wait()
        assert bits(ctx.hdi(t)) == base
        pr = np.array([0.94])
        out = ffi.Hdi()                                                 # (rejected before anything is written)
        for fn, ptr in ((ctx.lib.mcr_hdi, x3.ctypes.data_as(C.c_void_p)), (ctx.lib.mcr_hdi_dev, t.buf.ptr)):
            targs = list(ffi.tensor_args(x3, "pcn"))
            targs[5] = -targs[5]                                        # a negative draw stride
            with pytest.raises(ffi.McrError, match="negative strides") as e:
                ctx._check(fn(ctx.handle, ptr, *targs, pr.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(out)))
            assert e.value.code == ffi.MCR_EINVAL
    finally:
        t.free()
    still_works()


def test_empty_shapes(ctx):
    empty = ctx.hdi(np.empty((2, 4, 0)), prob=[0.5, 0.94])              # M == 0
    assert empty["index"].tolist() == [[-1, -1], [-1, -1]] and np.isnan(empty["lo"]).all() and np.isnan(empty["hi"]).all()
    none = ctx.hdi(np.empty((0, 4, 10)), prob=[0.5, 0.94])              # P == 0
    assert all(none[k].shape == (0, 2) for k in KEYS)
    assert all(ctx.hdi(np.empty((0, 4, 10)))[k].shape == (0,) for k in KEYS)


# ---- Python, the command and validate --------------------------------------------------------------------------------------------

def test_chains_of_unequal_lengths_are_pooled(ctx, ffi):
    from mcmc_ref_hip import diagnostics
    x = draws("exponential", 1000, seed=5)
    cuts = [0, 100, 350, 351, 1000]
    chains = [x[a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    for q in (0.94, 0.5):
        lo, hi, _ = hdi_reference(x, q)
        assert diagnostics.hdi(chains, q, context=ctx) == (lo, hi)
    assert diagnostics.hdi(chains, context=ctx) == hdi_reference(x, 0.94)[:2]
    with pytest.raises(ValueError):
        diagnostics.hdi(chains, 1.0, context=ctx)
    buf = ffi.DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        ragged = ctx.ragged_tensor(buf, np.diff(cuts), 1)
        assert bits(ctx.hdi(ragged, prob=[0.94, 0.5])) == bits(ctx.hdi(x.reshape(1, 1, -1), prob=[0.94, 0.5]))
    finally:
        buf.free()


CORPUS_FILE = Path(__file__).parent / "golden" / "corpus" / "draws" / "arma-arma11.draws.parquet"


def test_hdi_file_and_command(ctx):
    import pyarrow.parquet as pq
    from click.testing import CliRunner
    from mcmc_ref_hip import cli
    from mcmc_ref_hip.convert import hdi_file
    table = pq.read_table(CORPUS_FILE)
    names = [c for c in table.column_names if c not in ("chain", "draw")]
    cols = {n: table.column(n).to_numpy() for n in names}
    want = {n: {f"hdi_{k}_{q:g}": v for q in (0.5, 0.94) for k, v in zip(("lo", "hi"), hdi_reference(cols[n], q))} for n in names}
    assert hdi_file(CORPUS_FILE, prob=(0.5, 0.94), context=ctx) == want
    assert hdi_file(CORPUS_FILE, params=names[:1], context=ctx) == {names[0]: {k: v for k, v in want[names[0]].items() if k.endswith("0.94")}}
    res = CliRunner().invoke(cli.main, ["hdi", str(CORPUS_FILE), "--prob", "0.5", "--prob", "0.94", "--format", "json"])
    assert res.exit_code == 0, res.output
    assert json.loads(res.output) == want
    res = CliRunner().invoke(cli.main, ["hdi", str(CORPUS_FILE), "--params", names[1]])
    assert res.exit_code == 0 and "hdi_lo_0.94" in res.output and names[1] in res.output and names[0] + " " not in res.output
    assert f"{want[names[1]]['hdi_hi_0.94']:.6g}" in res.output
    res = CliRunner().invoke(cli.main, ["hdi", str(CORPUS_FILE), "--params", "nope"])
    assert res.exit_code != 0 and "Unknown parameter" in res.output
    res = CliRunner().invoke(cli.main, ["hdi", str(CORPUS_FILE), "--prob", "1.0"])
    assert res.exit_code != 0 and "inside (0, 1)" in res.output


def test_validate_sees_mass_in_the_wrong_place(ctx, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    from mcmc_ref_hip.validate import validate
    (tmp_path / "draws").mkdir()
    (tmp_path / "meta").mkdir()
    rng = np.random.default_rng(9)
    ref = {"a": rng.normal(size=4000), "b": rng.exponential(size=4000)}
    pq.write_table(pa.table({"chain": np.repeat(np.arange(4), 1000), "draw": np.tile(np.arange(1000), 4), **ref}),
                   tmp_path / "draws" / "skew.draws.parquet")
    (tmp_path / "meta" / "skew.meta.json").write_text(json.dumps({"diagnostics": {}}))
    store = DataStore(local_root=tmp_path, packaged_root=tmp_path / "none")
    kw = dict(store=store, context=ctx, tolerance=1e12)                 # mean and std pass: the HDI alone decides
    plain = validate("skew", ref, **kw)                                 # without the options: today's result
    assert plain.passed and plain.hdi_ref == {} and plain.hdi_actual == {}
    same = validate("skew", ref, hdi_tol=0.05, **kw)                    # a sample against itself
    assert same.passed and same.hdi_ref == same.hdi_actual
    assert same.hdi_ref == {p: hdi_reference(ref[p], 0.94)[:2] for p in ref}
    for f in dataclasses.fields(plain):                                 # every other field is what it is without the options
        if f.name not in ("hdi_ref", "hdi_actual", "compare"):
            assert getattr(same, f.name) == getattr(plain, f.name), f.name
    assert same.compare.failures == plain.compare.failures
    half = validate("skew", ref, hdi_prob=0.5, **kw)                    # information only
    assert half.passed and half.hdi_actual == {p: hdi_reference(ref[p], 0.5)[:2] for p in ref}
    med = float(np.median(ref["b"]))
    mirrored = {"a": ref["a"], "b": 2.0 * med - ref["b"]}               # the same median, the mass on the other side
    assert np.median(mirrored["b"]) == pytest.approx(med, abs=1e-12)
    free = validate("skew", mirrored, **kw)
    assert free.passed and free.hdi_ref == {}
    gated = validate("skew", mirrored, hdi_tol=0.05, **kw)
    assert not gated.passed and len(gated.failures) == 1 and gated.failures[0].startswith("b.hdi_offset="), gated.failures
    assert gated.hdi_actual["a"] == gated.hdi_ref["a"] and gated.hdi_actual["b"] == hdi_reference(mirrored["b"], 0.94)[:2]
    uneven = validate("skew", {"a": ref["a"], "b": ref["b"][:-1]}, hdi_tol=0.05, **kw)        # no joint draws needed
    assert uneven.hdi_actual["a"] == same.hdi_actual["a"] and uneven.hdi_actual["b"] == hdi_reference(ref["b"][:-1], 0.94)[:2]
