"""Every draw's average rank and z, exactly, on every sort and fold path.

R-hat, bulk / tail ESS and the truncation lags are functions of one integer per draw, the code `s + e` of its tie run `[s, e)`
in the pooled ascending order -- once for the draws, once for `|x - median|`.  The kernels that produce the codes (tile sort,
pairwise merges, run samples and splitters, bucket merge, the fold merge with its block-edge tie completion, the rank kernel of
the merge-pass path) are compared elsewhere through the final statistics at 1e-9, a gate that a draw half a rank off, or two
neighbouring ranks swapped, passes at the benchmark and stress shapes.  Here `mcr_diagnose_chains` -- the same pipeline with one
f64 parameter -- hands back the decoded codes of every draw in time order, and they are compared with the plain numpy reference
of tests/test_rank_refs_cpu.py:

* `rank_bulk`, `rank_tail` equal `(code + 1) / 2` exactly, no tolerance; a failure names the first offending pooled positions,
  their sorted positions modulo the tile (4096) and the fold block (4032), their tie runs and the codes got / expected;
* the median equals the reference's in bits;
* `z_bulk`, `z_tail` equal `NormalDist().inv_cdf` of the reference's rank to 1e-13 relative (the gate of
  `test_unit_vectors_ragged_api` for the same quantity), and z is strictly increasing in the code over the codes present, which
  the constant-window test of the autocovariance kernel relies on;
* up to 70 000 pooled draws, R-hat / ESS of the same call agree with the oracle to 1e-9 and the lags exactly.

The debug decode clamps a code above 2M - 1 to 2M - 1 (it bounds the z-table read), so a code that no kernel ever wrote shows up
as rank M or as whatever the buffer held; the exact comparison catches either.

The pooled lengths sit on each side of every switch of the sort plan, the inputs are the builders of test_rank_refs_cpu.py (whose
CPU tests check that each really has the tie runs, medians and zeros it is named for), and the chains are ragged, so a draw's
time-order position, sorted position and chain-local index all differ.  The case list is fixed at import: nothing is skipped
or filtered at run time, and the last test counts the cases.

The second test ties the multi-parameter routes (`summarize` on f64 `pcn`, f64 `cnp` and f32 `pcn`, the packed-record sort) to the
route checked per draw: bit-identical diagnostics for five parameters of different kinds in one tensor.
"""
from __future__ import annotations

import time

import numpy as np
import pytest

from test_hip_parity import TIGHT, close
from test_rank_refs_cpu import (CASES, N_CASES, ALL_M, SIDE_M, STAIR_M, STAIR_L, EVERY_M_KINDS, SIDE_KINDS, b_iid, b_round1,
                                b_signed_zero, b_sym_between, b_sym_in_run, b_underflow, build, chains_of, fold, median_of,
                                rank_codes, same_bits, z_of_codes)

pytestmark = pytest.mark.gpu

ORACLE_MAX_M = 70000          # as test_f32_records_equal_the_widened_path draws the line
Z_RTOL = 1e-13


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def describe_rank_errors(x, got_rank, exp_codes, what, limit=6) -> str:
    """First few draws whose rank is wrong: pooled position, sorted position (stable) modulo 4096 and 4032, tie run [s, e),
    got / expected code."""
    got_codes = np.rint(2.0 * got_rank - 1.0).astype(np.int64)
    bad = np.flatnonzero(got_rank != (exp_codes + 1) / 2)
    order = np.argsort(x, kind="stable")
    spos = np.empty(len(x), dtype=np.int64)
    spos[order] = np.arange(len(x))
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    run_len = cnt[inv.reshape(-1)]
    lines = [f"{what}: {bad.size} of {len(x)} draws with a wrong rank; first {min(limit, bad.size)}:"]
    for i in bad[:limit]:
        s = (exp_codes[i] - run_len[i]) // 2
        lines.append(f"  pooled {i}: sorted {spos[i]} (mod 4096 = {spos[i] % 4096}, mod 4032 = {spos[i] % 4032}), run [{s}, "
                     f"{s + run_len[i]}) (s mod 4096 = {s % 4096}, mod 4032 = {s % 4032}; last mod 4096 = "
                     f"{(s + run_len[i] - 1) % 4096}, mod 4032 = {(s + run_len[i] - 1) % 4032}), value {x[i]!r}, code got "
                     f"{got_codes[i]} expected {exp_codes[i]}")
    return "\n".join(lines)


def check_ranks_and_z(got, x, what):
    """The per-draw gate.  Returns the reference median (the caller compares it, last)."""
    M = len(x)
    f, med = fold(x)
    for name, v in (("bulk", x), ("tail", f)):
        codes = rank_codes(v)
        rank = np.concatenate(got[f"rank_{name}"])
        assert rank.shape == (M,)
        if not np.array_equal(rank, (codes + 1) / 2):
            pytest.fail(describe_rank_errors(v, rank, codes, f"{what} rank_{name}"), pytrace=False)
        z, zref = np.concatenate(got[f"z_{name}"]), z_of_codes(codes, M)
        err = np.abs(z - zref)
        worst = int(np.argmax(err - Z_RTOL * np.abs(zref)))
        assert np.all(err <= Z_RTOL * np.abs(zref)), (what, f"z_{name}", worst, z[worst], zref[worst], int(codes[worst]))
        u, first = np.unique(codes, return_index=True)
        zu = z[first]
        assert np.array_equal(zu[np.searchsorted(u, codes)], z), (what, f"z_{name}: one code, two z")
        assert np.all(np.diff(zu) > 0), (what, f"z_{name} not strictly increasing in the code",
                                         u[:-1][np.diff(zu) <= 0][:4].tolist())
    return med


@pytest.mark.parametrize("M,kind", CASES, ids=[f"{M}-{k}" for M, k in CASES])
def test_ranks_and_z_of_every_draw(ctx, oracle, M, kind):
    """Ranks, z, the statistics against the oracle, and last the median in bits.

    `const` (every chain constant at ONE value) is not the known constant-halves discrepancy that test_strides_gpu.py pins:
    every z is exactly 0 (code M is the centre of the table), all sums are exact, and kernels and oracle agree (R-hat 1.0).

    The median of `signed_zero` is a zero whose sign `statistics.median` takes from the time order of the +-0 draws (it sorts
    stably); the order statistics look it up there, since the sort keeps no order among equal draws.
    """
    x = build(M, kind)
    chains = chains_of(x)
    what = f"M={M} {kind}"
    t0 = time.perf_counter()
    got = ctx.diagnose_chains(chains, min_chains=2, debug=True)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\n{what}: {ms:.1f} ms; median {got['median']!r} rhat {got['rhat']!r} ess {got['ess_bulk']!r} / {got['ess_tail']!r} "
          f"lags {got['lag_bulk']} / {got['lag_tail']}")
    check_diagnosis(got, x, chains, oracle, what)


def check_diagnosis(got, x, chains, oracle, what):
    """A diagnose_chains(debug=True) result of the pooled draws x in `chains`: the per-draw gate, the statistics against the
    oracle up to ORACLE_MAX_M pooled draws, and last the median in bits (tests/call_families.py shares this gate)."""
    med = check_ranks_and_z(got, x, what)
    if len(x) <= ORACLE_MAX_M:
        exp = oracle.diag(chains, 2)
        print(f"{what}: oracle rhat {exp['rhat']!r} ess {exp['ess_bulk']!r} / {exp['ess_tail']!r} lags {exp['lag_bulk']} / "
              f"{exp['lag_tail']}")
        for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
            assert close(got[k], exp[k], TIGHT), (what, k, got[k], exp[k])
        assert (got["lag_bulk"], got["lag_tail"]) == (exp["lag_bulk"], exp["lag_tail"]), what
    assert same_bits(got["median"], med), (what, "median", got["median"], med)


ROUTE_M = (40000, 65536, 400000)      # the benchmark shape, the first length with 32-bit positions, the stress shape
ROUTE_KEYS = ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "lag_bulk", "lag_tail", "median")


def route_tensor(M):
    """[P = 5][C = 4][N = M / 4], float64 values that float32 holds exactly: five parameters of different kinds and seeds."""
    rows = [b_iid(M, seed=21), b_round1(M, seed=22), b_sym_in_run(M, seed=23), b_sym_between(M, seed=24), b_iid(M, seed=25)]
    x = np.stack(rows).astype(np.float32).astype(np.float64).reshape(5, 4, M // 4)
    return x + 0.0


@pytest.mark.parametrize("M", ROUTE_M)
def test_summarize_routes_equal_the_checked_route_in_bits(ctx, M):
    x = route_tensor(M)
    P = x.shape[0]
    per_param = []
    for p in range(P):
        got = ctx.diagnose_chains(list(x[p]), min_chains=2, debug=True)
        med = check_ranks_and_z(got, x[p].reshape(-1), f"route M={M} p={p}")
        assert same_bits(got["median"], med), (M, p, "median", got["median"], med)
        per_param.append(got)
    assert len({g["median"] for g in per_param}) >= 3 and len({g["rhat_bulk"] for g in per_param}) == P     # they do differ
    routes = {"f64 pcn": ctx.summarize(x, "pcn", min_chains=2),
              "f64 cnp": ctx.summarize(np.ascontiguousarray(np.transpose(x, (1, 2, 0))), "cnp", min_chains=2),
              "f32 pcn": ctx.summarize(x.astype(np.float32), "pcn", min_chains=2)}
    diffs = []
    for name, r in routes.items():
        for p in range(P):
            for k in ROUTE_KEYS:
                a, b = r[k][p], per_param[p][k]
                same = int(a) == int(b) if k.startswith("lag") else same_bits(float(a), float(b))
                if not same:
                    diffs.append((name, p, k, a, b))
    print(f"\nroutes M={M}: {len(diffs)} fields differ", diffs[:10])
    assert not diffs, diffs[:10]


@pytest.mark.parametrize("C,N", [(3, 21), (3, 1365), (4, 1024), (4, 10000), (4, 16384), (3, 43691), (4, 100000)])
def test_sign_of_a_zero_median_on_every_route(ctx, C, N):
    """A median made of +-0 draws has the sign `statistics.median` gives it (a stable sort: the middle zeros of the time order),
    whatever order the sort leaves equal draws in: `summarize` on f64 `pcn`, f64 `cnp` (the ingest buffer), f32 `pcn` (packed
    records) and without diagnostics (the order-statistics launch of its own), for odd and even pooled lengths on each side
    of the 16-bit positions.  Ten parameters with differently placed signs; both signs must occur among the medians."""
    M = C * N
    x = np.stack([b_signed_zero(M, seed=40 + p) for p in range(10)]).reshape(10, C, N)
    ref = [median_of(x[p].reshape(-1)) for p in range(10)]
    assert all(m == 0.0 for m in ref) and len({bool(np.signbit(m)) for m in ref}) == 2
    routes = {"f64 pcn": ctx.summarize(x, "pcn", min_chains=2),
              "f64 cnp": ctx.summarize(np.ascontiguousarray(np.transpose(x, (1, 2, 0))), "cnp", min_chains=2),
              "f32 pcn": ctx.summarize(x.astype(np.float32), "pcn", min_chains=2),
              "f64 pcn, no diagnostics": ctx.summarize(x, "pcn", min_chains=2, diagnostics=False),
              "f32 pcn, no diagnostics": ctx.summarize(x.astype(np.float32), "pcn", min_chains=2, diagnostics=False)}
    for name, r in routes.items():
        got = [float(v) for v in r["median"]]
        assert all(same_bits(g, m) for g, m in zip(got, ref)), (name, got, ref)


@pytest.mark.parametrize("M", [4, 64, 4096, 40000, 65536, 131072, 600000])
@pytest.mark.parametrize("negative_zero", [False, True])
def test_median_that_underflows_to_zero_keeps_the_sign_of_the_sum(ctx, M, negative_zero):
    """Even M, the draw below the middle is -5e-324 and the draw above it a zero of either sign: the median is -0.0 by the
    rounding of (-5e-324 + 0) / 2, not a zero draw, so the time-order look-up of a zero median must leave it alone.  f64
    routes (f32 cannot hold the draw): ragged chains, `pcn`, `cnp`, and without diagnostics."""
    x = b_underflow(M, negative_zero)
    assert same_bits(median_of(x), -0.0)
    got = {"ragged": ctx.diagnose_chains(chains_of(x), min_chains=2)["median"]}
    t = np.stack([x, b_underflow(M, not negative_zero, seed=16)]).reshape(2, 4, M // 4)
    got["pcn"] = ctx.summarize(t, "pcn", min_chains=2)["median"]
    got["cnp"] = ctx.summarize(np.ascontiguousarray(np.transpose(t, (1, 2, 0))), "cnp", min_chains=2)["median"]
    got["pcn, no diagnostics"] = ctx.summarize(t, "pcn", min_chains=2, diagnostics=False)["median"]
    for name, m in got.items():
        assert all(same_bits(float(v), -0.0) for v in np.atleast_1d(m)), (name, m)


def test_case_count():
    """The parametrisation, counted, so that a later edit cannot thin it silently."""
    assert len(CASES) == len(set(CASES)) == N_CASES == 408
    assert len(ALL_M) == 27 and len(SIDE_M) == 18 and len(STAIR_M) == 15 and len(STAIR_L) == 11
    per_kind = {}
    for M, k in CASES:
        per_kind[k] = per_kind.get(k, 0) + 1
    assert len(EVERY_M_KINDS) == 5 and all(per_kind[k] == 27 for k in EVERY_M_KINDS) and per_kind["sym_between"] == 13
    assert all(per_kind[k] == 18 for k in SIDE_KINDS)
    assert sum(per_kind[f"stair{L}"] for L in STAIR_L) == 134 and min(per_kind[f"stair{L}"] for L in STAIR_L) == 9
    assert len(ROUTE_M) == 3
