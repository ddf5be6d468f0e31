"""The f64 tile sort on 64-bit records, its order check and its fallback to (key, position) pairs.

`k_tile_sort` sorts a tile of 4096 f64 draws as records -- the draw with its low 12 mantissa bits replaced by its tile slot --,
rebuilds the exact keys, checks that they ascend, and sorts the tile as (key, position) pairs after all when they do not: when
draws of one tile agree in their upper 52 bits and their low bits order them against their slots.  Every test here takes the
per-draw gate of test_rank_codes_gpu.py (ranks exactly, z to 1e-13, the median in bits) through `mcr_diagnose_chains`, and
counts the tiles that fell back (`mcr_tile_fallback_count`) against the host model of tests/test_tile_records_cpu.py: none for
ordinary draws, and exactly the constructed ones otherwise.

Pooled lengths: 4095 (one partial tile), 4096, 4097 (a last tile of ONE draw), 8191 (a last tile of 4095 draws), 8192 + 37 and
40000 (the benchmark's).  A tile is 4096 consecutive pooled draws; `chains_of` cuts the pooled array into three ragged chains.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_hip_parity import TIGHT, check_summary, close
from test_rank_codes_gpu import check_ranks_and_z
from test_rank_refs_cpu import b_iid, b_signed_zero, chains_of, median_of, same_bits
from test_tile_records_cpu import fallback_tiles, record_sorted

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = (4095, 4096, 4097, 8192 + 37, 40000)
ULP1 = 2.0 ** -52             # the spacing of doubles in [1, 2)


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def tiles_of(M) -> list[int]:
    return [min(TILE, M - b) for b in range(0, M, TILE)]


def run(ctx, x, what, oracle=None) -> int:
    """The per-draw gate on one pooled array; returns how many of its tiles fell back."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    chains = chains_of(x)
    before = ctx.tile_fallback_count()
    got = ctx.diagnose_chains(chains, min_chains=2, debug=True)
    fell = ctx.tile_fallback_count() - before
    med = check_ranks_and_z(got, x, what)
    assert same_bits(got["median"], med), (what, "median", got["median"], med)
    if oracle is not None:
        exp = oracle.diag(chains, 2)
        for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
            assert close(got[k], exp[k], TIGHT), (what, k, got[k], exp[k])
        assert (got["lag_bulk"], got["lag_tail"]) == (exp["lag_bulk"], exp["lag_tail"]), what
    print(f"\n{what}: {fell} of {len(tiles_of(len(x)))} tiles fell back, the host model says {fallback_tiles(x)}")
    assert fell == fallback_tiles(x), what
    return fell


def low_bit_ladder(M, seed, descending=False):
    """1 + j 2^-52 for a permutation j of 0 .. M-1: the upper 52 bits agree within blocks of 4096 values."""
    j = np.arange(M)[::-1] if descending else np.random.default_rng([seed, M]).permutation(M)
    return 1.0 + j.astype(np.float64) * ULP1


@pytest.mark.parametrize("M", SIZES)
def test_ordinary_draws_stay_on_the_record_path(ctx, oracle, M):
    """iid normal draws, and draws rounded to two decimals (ties: equal keys are sorted by slot, which is an order)."""
    assert run(ctx, b_iid(M, seed=61), f"iid M={M}", oracle) == 0
    assert run(ctx, np.round(b_iid(M, seed=62), 2) + 0.0, f"round2 M={M}", oracle) == 0


@pytest.mark.parametrize("M", SIZES + (8191,))
def test_low_bit_ladder_falls_back_in_every_tile(ctx, M):
    """Every tile with two draws or more holds draws that tie in their upper 52 bits against their slots (a random permutation
    leaves 37 draws of three blocks in slot order with probability < 1e-30); a tile of one draw has nothing to check."""
    expect = sum(1 for n in tiles_of(M) if n >= 2)
    assert run(ctx, low_bit_ladder(M, 63), f"ladder M={M}") == expect
    assert run(ctx, -low_bit_ladder(M, 64), f"negative ladder M={M}") == expect
    if M <= TILE:       # the true order exactly opposite to the slot order
        assert run(ctx, low_bit_ladder(M, 0, descending=True), f"descending ladder M={M}") == 1


def test_one_fallback_tile_among_record_tiles(ctx, oracle):
    M = 40000
    x = b_iid(M, seed=65)
    x[3 * TILE:4 * TILE] = low_bit_ladder(TILE, 66, descending=True)                    # inside the iid range
    assert run(ctx, x, "one ladder tile of ten", oracle) == 1
    x = b_iid(M, seed=67)
    x[9 * TILE:] = 1.0 + np.arange(M - 9 * TILE)[::-1] * ULP1                           # the partial last tile alone
    assert run(ctx, x, "the partial tile of ten", oracle) == 1


def plant_pair(x, tile, s):
    """Make the draws at sorted slots s - 1 | s of `tile` tie in their upper 52 bits, with the low bits against the record
    order (slot order for positive draws, reverse slot order for negative ones)."""
    lo = tile * TILE
    t = x[lo:lo + TILE]
    order = np.argsort(t, kind="stable")
    a, b = sorted((int(order[s - 1]), int(order[s])))                  # tile slots, a < b
    bits = np.float64(t[order[s - 1]]).view(np.uint64) & ~np.uint64(0xFFF)
    small, large = sorted(((bits | np.uint64(0x800)).view(np.float64), (bits | np.uint64(0x801)).view(np.float64)))
    first, second = (a, b) if small > 0 else (b, a)                     # the record order of the two
    t[first], t[second] = large, small
    keys, slots = record_sorted(t)
    assert [int(slots[s - 1]), int(slots[s])] == [first, second] and keys[s - 1] > keys[s]
    assert np.flatnonzero(keys[1:] < keys[:-1]).tolist() == [s - 1]


@pytest.mark.parametrize("s,where", [(16 * 37, "lane boundary"), (1024 * 2, "wave boundary"), (16 * 100 + 5, "inside a lane"),
                                     (TILE - 16, "the last lane's boundary")])
def test_one_misordered_pair(ctx, s, where):
    """Two draws that the record sort leaves at the sorted slots s - 1 | s in the wrong order: inside one lane's 16 registers,
    across two lanes (seen only by the check through the LDS), across two waves.  Tiles 0 and 2 of three stay records."""
    x = b_iid(8192 + 37, seed=68)
    plant_pair(x, 1, s)
    assert run(ctx, x, f"pair at the {where}") == 1


def test_denormals_that_differ_in_their_low_bits(ctx):
    for M in (4097, 8192 + 37):
        rng = np.random.default_rng([69, M])
        x = rng.permutation(M).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], size=M) + 0.0
        assert np.count_nonzero(x) == M - 1 and np.abs(x).max() < 2.3e-308
        assert run(ctx, x, f"denormals M={M}") >= 1
    x = b_iid(4096, seed=70) * 1e-310                                  # denormals with all 52 bits in use: ordinary draws
    run(ctx, x, "denormal iid")                                        # (the host model decides: their upper bits are 2^-32 apart)


@pytest.mark.parametrize("M", (4096, 8192 + 37, 40000))
def test_signed_zeros_share_one_rank(ctx, oracle, M):
    """-0.0 and +0.0 are one tie run (check_ranks_and_z), and the zero median keeps the sign of the time order's middle zeros."""
    x = b_signed_zero(M, seed=71)
    assert np.signbit(x[x == 0.0]).any() and not np.signbit(x[x == 0.0]).all() and median_of(x) == 0.0
    assert run(ctx, x, f"signed zeros M={M}", oracle) == 0
    y = b_iid(M, seed=72)
    y[::7] = 0.0
    y[3::14] = -0.0
    assert run(ctx, y, f"signed zeros among iid M={M}") == 0


def test_f32_draws_widened_by_the_tile_sort(ctx, monkeypatch):
    """f32 tensors on the f64 kernels (MCR_F32_RECORDS=0): the widened draws have 29 zero low bits, so no tile falls back, and
    every output equals the one of the same draws handed over as f64, in bits."""
    from mcmc_ref_hip import _ffi
    monkeypatch.setenv("MCR_F32_RECORDS", "0")
    wide = _ffi.Context(0)
    monkeypatch.delenv("MCR_F32_RECORDS")
    try:
        rng = np.random.default_rng(73)
        for C, N in ((3, 1365), (4, 2048 + 10), (4, 10000)):
            x = rng.normal(size=(2, C, N)).astype(np.float32)
            x[1] = np.round(x[1], 1)
            x[1, :, ::5] = -0.0
            got = wide.summarize(x, "pcn", min_chains=2)
            ref = wide.summarize(x.astype(np.float64), "pcn", min_chains=2)
            for k in got:
                assert np.array_equal(got[k], ref[k], equal_nan=True), (C, N, k)
        assert wide.tile_fallback_count() == 0
    finally:
        wide.close()


@pytest.mark.parametrize("C,N", [(17, 241), (2, 4095), (4, 10000)])
def test_moments_of_record_and_fallback_tiles_against_the_oracle(ctx, oracle, C, N):
    """Mean and std come from the tile sort's own moment passes (the rebuilt keys in registers, or the pair sort's): `summarize`
    against the oracle for a last tile of one draw (4097), of 4094 draws (8190) and the benchmark's 40000, one parameter on
    the record path and one whose every tile with two draws falls back.

    The ladder's spread is a few thousand ulps of its mean, and the reference's std is `sqrt(mean((x - m)^2))` about a mean m
    that is rounded to a double: off by up to half an ulp, which adds (m - mu)^2 to the variance, up to (ulp / 2 / std)^2 / 2
    of the std (2e-8 at M = 8190; the kernels' moment records carry what rounding left of the mean).  That term is the
    reference's own error and is added to the 1e-9 for the ladder's std; every other field keeps 1e-9."""
    M = C * N
    x = np.stack([3.0 + 0.5 * b_iid(M, seed=75), low_bit_ladder(M, 76)]).reshape(2, C, N)
    before = ctx.tile_fallback_count()
    got = ctx.summarize(x, "pcn", min_chains=2)
    assert ctx.tile_fallback_count() - before == fallback_tiles(x[1].reshape(-1)) == sum(1 for n in tiles_of(M) if n >= 2)
    exp = oracle.summarize(x, "pcn", min_chains=2)
    one = lambda d, p: {k: np.asarray(v)[p:p + 1] for k, v in d.items()}
    check_summary(one(got, 0), one(exp, 0), what=f"moments M={M}, records")
    sd = float(exp["std"][1])
    ref_err = 0.5 * (np.spacing(float(exp["mean"][1])) / 2 / sd) ** 2
    print(f"\nmoments M={M}: ladder std {got['std'][1]!r} against {sd!r}, the reference's own bound {ref_err:.2e}")
    assert close(got["std"][1], sd, TIGHT + ref_err), (M, got["std"][1], sd, ref_err)
    g1, e1 = one(got, 1), one(exp, 1)
    g1["std"] = e1["std"]
    check_summary(g1, e1, what=f"moments M={M}, pairs")


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_non_finite_draws_are_still_refused(ctx, poison):
    from mcmc_ref_hip import _ffi
    x = b_iid(2 * 8229, seed=74).reshape(2, 3, 2743)
    ref = ctx.summarize(x, "pcn", min_chains=2)
    bad = x.copy()
    bad[1, 1, 1500] = poison
    with pytest.raises(_ffi.McrError) as e:
        ctx.summarize(bad, "pcn", min_chains=2)
    assert e.value.code == _ffi.MCR_ENONFINITE
    again = ctx.summarize(x, "pcn", min_chains=2)
    for k in ref:
        assert np.array_equal(again[k], ref[k], equal_nan=True), k
