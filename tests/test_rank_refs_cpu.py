"""The per-draw reference of the rank path, pinned on the CPU, and the inputs of tests/test_rank_codes_gpu.py.

Everything the diagnostics compute is a function of one integer per draw: the code `n2 = s + e` of the draw's tie run `[s, e)` in
the pooled ascending order (average rank `(n2 + 1) / 2`, `z = Phi^-1((rank - 0.5) / M)`), once for the draws and once for
`|x - median|`.  This file states those codes in plain numpy, independent of the C oracle and of the kernels:

* `rank_codes(x)`       the exact integer code of every draw (`-0.0` and `+0.0` tie, as `==` makes them in the reference);
* `fold(x)`             `statistics.median`'s rule and `np.abs(x - med)`: the reference's two IEEE operations;
* `z_of_codes(c, M)`    `statistics.NormalDist().inv_cdf`, the reference's own call, on the distinct codes.

The tests hold them to the oracle bit for bit and to a literal transcription of the reference's semantics
(`scipy.stats.rankdata(method="average")`, `statistics.median`), and check that every input builder produces what its name
says -- a tie run longer than a tile, a median inside a run, both signs of zero in one run, ... -- so that the GPU file, which
imports the builders and the case list from here, cannot quietly test something easier.
"""
from __future__ import annotations

import statistics

import numpy as np
import pytest

# ---------------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------------


def rank_codes(x) -> np.ndarray:
    """Code s + e (int64) of every draw's tie run [s, e) in the ascending order of x."""
    x = np.asarray(x, dtype=np.float64)
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)      # -0.0 == +0.0: one value
    e = np.cumsum(cnt, dtype=np.int64)
    s = e - cnt
    return (s + e)[inv.reshape(-1)].astype(np.int64)


def median_of(x) -> float:
    """statistics.median: the middle draw of the sorted array, or (a + b) / 2 of the two middle draws."""
    s = np.sort(np.asarray(x, dtype=np.float64), kind="stable")      # as sorted(): equal draws (-0.0, +0.0) keep their order
    m = s.size
    return float(s[m // 2]) if m % 2 else float((s[m // 2 - 1] + s[m // 2]) / 2)


def fold(x) -> tuple[np.ndarray, float]:
    x = np.asarray(x, dtype=np.float64)
    med = median_of(x)
    return np.abs(x - med), med


_ZCACHE: dict = {"M": None, "z": None}     # z of the codes already evaluated for the last M (bulk and tail share most)


def z_of_codes(codes, M: int) -> np.ndarray:
    """z of every code: NormalDist().inv_cdf(((n2 + 1) / 2 - 0.5) / M), evaluated once per distinct code."""
    codes = np.asarray(codes, dtype=np.int64)
    if _ZCACHE["M"] != M:
        _ZCACHE["M"], _ZCACHE["z"] = M, np.full(2 * M, np.nan)
    tab = _ZCACHE["z"]
    u = np.unique(codes)
    assert u.size == 0 or (u[0] >= 1 and u[-1] <= 2 * M - 1)
    inv = statistics.NormalDist().inv_cdf
    for n2 in u[np.isnan(tab[u])].tolist():
        tab[n2] = inv(((n2 + 1) / 2 - 0.5) / M)
    return tab[codes]


def same_bits(a: float, b: float) -> bool:
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# Inputs.  Every builder returns the pooled draws (float64, length M) for a seed; `chains_of` cuts them into ragged chains.
# ---------------------------------------------------------------------------------------------------------------------


def chains_of(x) -> list[np.ndarray]:
    """Three ragged chains of about M/2, M/3 and the rest, each with at least two draws, so that the time-order position, the
    sorted position and the chain-local index of a draw all differ.  Six draws are the least three such chains hold: the
    pooled lengths 4 and 5 are cut into two chains (M/2 and the rest)."""
    M = len(x)
    cuts = [M // 2, M // 2 + M // 3] if M >= 6 else [M // 2]
    out = np.split(np.asarray(x), cuts)
    assert all(len(c) >= 2 for c in out) and sum(len(c) for c in out) == M
    return out


def _rng(M, seed):
    return np.random.default_rng([seed, M])


def b_iid(M, seed=1):
    return _rng(M, seed).normal(size=M)


def _round1(rng, M):
    x = rng.normal(size=M)
    x[rng.random(size=M) < 0.55] *= 0.01       # these round to zero
    return np.round(x, 1) + 0.0                # (+ 0.0: the rounding's own negative zeros made positive)


def b_round1(M, seed=2):
    """Standard normal draws rounded to one decimal, 55 % of them shrunk to zero first: ~60 values whose tie runs hold M/55
    draws and fewer, and one run (the zeros, 57 % of the draws) that is longer than a tile as soon as M has two tiles.  The
    median lies in that run, so the folded draws have it too."""
    return _round1(_rng(M, seed), M)


def b_two(M, seed=3):
    x = (_rng(M, seed).normal(size=M) > 0.3).astype(np.float64)
    x[0], x[-1] = 1.0, 0.0                     # both values at any M
    return x


def b_const(M, seed=4):
    return np.full(M, 0.25)


def b_sym_in_run(M, seed=5):
    """Integer-valued, roughly symmetric about a median that lies inside a tie run (a run of folded zeros); the counts on the
    two sides of the median differ.  Seeds are tried in order until the median condition holds (it does at once for M >= 63)."""
    for k in range(1000):
        x = np.round(3.0 * _rng(M, seed + 100 * k).normal(size=M)) + 0.0
        med = median_of(x)
        if np.count_nonzero(x == med) >= 2:
            return x
    raise AssertionError("no seed gives a median inside a tie run")


def b_sym_between(M, seed=6):
    """Even M, integer-valued: M/2 draws at -1, -2, ... and M/2 at 1, 2, ...: the median 0 lies halfway between -1 and 1, and
    the folded values of the two sides tie (med - a == b - med) with different counts on each side."""
    assert M % 2 == 0
    rng = _rng(M, seed)
    a = np.round(2.0 * np.abs(rng.normal(size=M // 2)))
    b = np.round(2.0 * np.abs(rng.normal(size=M // 2)))
    a[0] = b[0] = 0.0
    return rng.permutation(np.concatenate([-(1.0 + a), 1.0 + b]))


def b_staircase(M, L, seed=7):
    """Sorted order = runs of exactly L equal draws (values 0, 0.5, 1, ...; a shorter last run if L does not divide M), the
    positions permuted.  Needs M >= 4 L."""
    assert M >= 4 * L
    return _rng(M, seed + L).permutation((np.arange(M) // L) * 0.5)


def b_signed_zero(M, seed=8):
    """b_round1 with every zero given a random sign."""
    rng = _rng(M, seed)
    x = _round1(rng, M)
    zeros = np.flatnonzero(x == 0.0)
    if zeros.size < 2:                         # tiny M: two zeros by hand
        zeros = np.array([0, M - 1])
        x[zeros] = 0.0
    sign = rng.integers(0, 2, size=zeros.size)
    sign[0], sign[-1] = 0, 1                   # both signs at any M
    x[zeros] = np.where(sign == 1, -0.0, 0.0)
    return x


def b_one_sided(M, seed=14):
    """exp() of b_round1: heavy ties on the lattice e^(k / 10), which no reflection about the median (1.0, inside the run of
    e^0) maps onto itself, so every folded tie run but the zeros holds draws from ONE side of the median.  (Every other tied
    input here is a uniform lattice around its median, whose folded runs are all two-sided.)  At a fold-block edge such a run
    continues in one of the two merged halves only."""
    return np.exp(_round1(_rng(M, seed), M))


def b_underflow(M, negative_zero, seed=15):
    """Even M: exactly M/2 draws below zero, the largest of them -5e-324, one zero (of the given sign) as the draw at M/2 and
    positive draws above it.  The median (-5e-324 + 0) / 2 underflows and rounds to even: -0.0 by arithmetic, whatever the sign
    of the zero -- a zero median that is not a zero draw."""
    assert M % 2 == 0 and M >= 4
    rng = _rng(M, seed)
    lower = -1.0 - np.abs(rng.normal(size=M // 2))
    upper = 1.0 + np.abs(rng.normal(size=M // 2))
    lower[0], upper[0] = -5e-324, (-0.0 if negative_zero else 0.0)
    return rng.permutation(np.concatenate([lower, upper]))


def b_ascending(M, seed=9):
    return np.sort(_rng(M, seed).normal(size=M))


def b_descending(M, seed=10):
    return np.sort(_rng(M, seed).normal(size=M))[::-1].copy()


def b_disjoint(M, seed=11):
    """Each chain of `chains_of` a value range of its own, descending from chain to chain: sorted runs never overlap."""
    x = _rng(M, seed).normal(size=M)
    cuts = [M // 2, M // 2 + M // 3] if M >= 6 else [M // 2]
    parts = np.split(np.tanh(x), cuts)         # every draw in (-1, 1)
    return np.concatenate([p - 4.0 * i for i, p in enumerate(parts)])


def b_subnormal(M, seed=12):
    """Small integer multiples of 5e-324: subnormal keys, exactly representable subnormal differences in the fold."""
    k = np.round(4.0 * _rng(M, seed).normal(size=M))
    return k * 5e-324 + 0.0                    # (+ 0.0: no negative zeros; those are b_signed_zero's subject)


def b_huge(M, seed=13):
    return _rng(M, seed).normal(size=M) * 1e300


STAIR_L = (2, 3, 63, 64, 65, 4031, 4032, 4033, 4096, 4097, 8193)

# Pooled lengths: each side of every switch in the sort plan, the sort stage, the fold launch and the order statistics.
#   4, 5                       the smallest arrays the ragged cut takes (two chains of >= 2 draws), even and odd
#   63, 64, 65                 one wavefront; the stride of the regular samples (every 64th draw of a run)
#   4031, 4032, 4033           one fold workgroup owns 4096 - 64 = 4032 outputs
#   4095, 4096, 4097           one sort tile (4096 draws): a partial tile, a full one, a full one and a single draw
#   8064, 8065                 two fold workgroups exactly, and a third with one output
#   12288                      three full tiles
#   40000                      the benchmark shape (4 x 10 000)
#   65535, 65536               16-bit -> 32-bit positions (limit 65535): the line-wise code scatter ends, the order
#                              statistics leave the fold kernel
#   65536, 65537               16 tiles (the most the bucket partition takes as runs) -> 9 runs of 8192 pre-merged pairwise,
#                              samples taken from the merged runs
#   131072, 131073             runs of 8192 -> 16384
#   262144, 262145             runs of 16384 -> 32768
#   400000                     the stress shape (4 x 100 000)
#   524288, 524289             16 runs x 32768 / 64 = 8192 samples is the most that fits: bucket partition -> full merge
#                              passes and the separate rank kernel
#   600001, 1200000            well inside the merge-pass path, odd and even
ALL_M = (4, 5, 63, 64, 65, 4031, 4032, 4033, 4095, 4096, 4097, 8064, 8065, 12288, 40000, 65535, 65536, 65537, 131072,
         131073, 262144, 262145, 400000, 524288, 524289, 600001, 1200000)
# b_iid, b_round1, b_sym_in_run, b_signed_zero and b_one_sided run at every M (b_sym_between at every even one).
# b_two, b_const, b_ascending, b_descending, b_disjoint, b_subnormal, b_huge: one M on each side of every switch above
SIDE_M = (5, 64, 65, 4032, 4033, 4096, 4097, 8064, 8065, 65535, 65536, 65537, 131072, 131073, 262144, 262145, 524288,
          524289)
# b_staircase: every L at every M >= 4 L of this list, which again has both sides of every switch that such an M
# can reach (L = 8193 starts at 65535)
STAIR_M = (260, 4032, 4033, 4096, 4097, 16388, 40000, 65535, 65536, 65537, 131073, 262144, 262145, 524288, 524289)

EVERY_M_KINDS = {"iid": b_iid, "round1": b_round1, "sym_in_run": b_sym_in_run, "signed_zero": b_signed_zero,
                 "one_sided": b_one_sided}
SIDE_KINDS = {"two": b_two, "const": b_const, "ascending": b_ascending, "descending": b_descending,
              "disjoint": b_disjoint, "subnormal": b_subnormal, "huge": b_huge}


def build_cases() -> list[tuple[int, str]]:
    """(M, kind) of every GPU case, M-major.  A kind that cannot be built for an M is left out here, explicitly."""
    cases = [(M, k) for M in ALL_M for k in EVERY_M_KINDS]
    cases += [(M, "sym_between") for M in ALL_M if M % 2 == 0]           # the median halfway between two draws: even M
    cases += [(M, k) for M in SIDE_M for k in SIDE_KINDS]
    cases += [(M, f"stair{L}") for M in STAIR_M for L in STAIR_L if M >= 4 * L]
    return sorted(cases, key=lambda c: c[0])


CASES = build_cases()
N_CASES = 27 * 5 + 13 + 18 * 7 + 134            # 408


def build(M: int, kind: str) -> np.ndarray:
    if kind.startswith("stair"):
        return b_staircase(M, int(kind[5:]))
    if kind == "sym_between":
        return b_sym_between(M)
    return {**EVERY_M_KINDS, **SIDE_KINDS}[kind](M)


# ---------------------------------------------------------------------------------------------------------------------
# Properties of an input, from the reference alone
# ---------------------------------------------------------------------------------------------------------------------


def run_lengths(x) -> np.ndarray:
    return np.unique(np.asarray(x, dtype=np.float64), return_counts=True)[1]


def cross_side_share(x) -> float:
    """Share of the folded draws that sit in a tie run holding draws from both sides of the median."""
    f, med = fold(x)
    side = np.sign(np.asarray(x) - med)
    _, inv = np.unique(f, return_inverse=True)
    inv = inv.reshape(-1)
    below = np.bincount(inv, weights=(side < 0)) > 0
    above = np.bincount(inv, weights=(side > 0)) > 0
    return float(np.mean((below & above)[inv]))


# ---------------------------------------------------------------------------------------------------------------------
# Tests
# ---------------------------------------------------------------------------------------------------------------------

SMALL_M = (4, 5, 7, 63, 64, 65, 260, 1001, 4097, 40001)


def small_inputs():
    for M in SMALL_M:
        for k in list(EVERY_M_KINDS) + list(SIDE_KINDS):
            yield M, k
        if M % 2 == 0:
            yield M, "sym_between"
        for L in STAIR_L:
            if M >= 4 * L:
                yield M, f"stair{L}"


SMALL = list(small_inputs())


def transcribed_ranks(chains):
    """`_rank_normalize`'s ranks: the average 1-based rank over a run of `==` values in the pooled ascending order."""
    from scipy.stats import rankdata
    return rankdata(np.concatenate([np.asarray(c, dtype=np.float64) for c in chains]), method="average")


def transcribed_fold(chains):
    """`_fold_chains`: med = statistics.median(flat); abs(v - med) per draw, in Python floats."""
    flat = [float(v) for c in chains for v in c]
    med = statistics.median(flat)
    return np.array([abs(v - med) for v in flat]), med


@pytest.mark.parametrize("M,kind", SMALL)
def test_helpers_equal_oracle_and_transcription(oracle, M, kind):
    x = build(M, kind)
    chains = chains_of(x)
    f, med = fold(x)
    # the oracle, bit for bit
    of, omed = oracle.fold(chains)
    assert same_bits(med, omed)
    assert np.array_equal(f.view(np.int64), np.concatenate(of).view(np.int64))
    for v in (x, f):
        cut = chains_of(v)
        oz, orank = oracle.rank_normalize(cut)
        codes = rank_codes(v)
        assert np.array_equal((codes + 1) / 2, np.concatenate(orank))
        assert np.array_equal(z_of_codes(codes, M).view(np.int64), np.concatenate(oz).view(np.int64))
        # the reference's semantics, transcribed
        assert np.array_equal((codes + 1) / 2, transcribed_ranks(cut))
    tf, tmed = transcribed_fold(chains)
    assert same_bits(med, tmed)
    assert np.array_equal(f.view(np.int64), tf.view(np.int64))
    # z is strictly increasing in the code
    u = np.unique(np.concatenate([rank_codes(x), rank_codes(f)]))
    assert np.all(np.diff(z_of_codes(u, M)) > 0)


@pytest.mark.parametrize("M", [4, 64, 4096, 40000])
@pytest.mark.parametrize("negative_zero", [False, True])
def test_median_that_underflows_to_zero(oracle, M, negative_zero):
    x = b_underflow(M, negative_zero)
    s = np.sort(x)
    assert np.count_nonzero(x < 0) == M // 2 and s[M // 2 - 1] == -5e-324 and s[M // 2] == 0.0 and s[M // 2 + 1] >= 1.0
    assert bool(np.signbit(x[x == 0.0][0])) == negative_zero
    med = median_of(x)
    assert same_bits(med, -0.0) and same_bits(statistics.median([float(v) for v in x]), -0.0)
    assert same_bits(oracle.fold(chains_of(x))[1], -0.0)


def test_rank_codes_by_hand():
    assert rank_codes([3.0, 1.0, 2.0]).tolist() == [5, 1, 3]
    assert rank_codes([0.0, -0.0, 1.0, -1.0, 0.0]).tolist() == [5, 5, 9, 1, 5]      # run [1, 4): 1 + 4
    assert rank_codes(np.full(7, 2.5)).tolist() == [7] * 7                            # one run of M: every code is M
    assert fold([4.0, 1.0, 3.0, 2.0])[1] == 2.5 and fold([5.0, 1.0, 3.0])[1] == 3.0
    assert fold([-0.0, 0.0, 1.0, -1.0])[0].tolist() == [0.0, 0.0, 1.0, 1.0]


def test_case_list_is_complete():
    assert len(CASES) == len(set(CASES)) == N_CASES
    for k in EVERY_M_KINDS:
        assert sorted(M for M, kk in CASES if kk == k) == sorted(ALL_M)
    assert sorted(M for M, kk in CASES if kk == "sym_between") == [M for M in ALL_M if M % 2 == 0]
    for k in SIDE_KINDS:
        assert sorted(M for M, kk in CASES if kk == k) == sorted(SIDE_M)
    for L in STAIR_L:
        assert sorted(M for M, kk in CASES if kk == f"stair{L}") == [M for M in STAIR_M if M >= 4 * L] != []


@pytest.mark.parametrize("M", ALL_M)
def test_every_m_builders_do_what_they_say(M):
    x = b_iid(M)
    assert np.unique(x).size == M and np.unique(fold(x)[0]).size >= M - 1           # all distinct (odd M: one folded 0)
    x = b_round1(M)
    assert not np.any(np.signbit(x[x == 0.0]))
    if M >= 8065:
        assert run_lengths(x).max() > 4096 and run_lengths(fold(x)[0]).max() > 4096
    x = b_sym_in_run(M)
    f, med = fold(x)
    assert np.array_equal(x, np.round(x)) and np.count_nonzero(x == med) >= 2 and np.count_nonzero(f == 0.0) >= 2
    if M >= 63:
        assert cross_side_share(x) >= 0.30
        below, above = np.count_nonzero(x == med - 1), np.count_nonzero(x == med + 1)
        assert below > 0 and above > 0 and below != above                            # the two sides are not mirror images
    if M % 2 == 0:
        x = b_sym_between(M)
        s = np.sort(x)
        f, med = fold(x)
        assert np.array_equal(x, np.round(x)) and s[M // 2 - 1] == -1.0 and s[M // 2] == 1.0 and med == 0.0
        assert cross_side_share(x) >= 0.30 and f.min() == 1.0
    x = b_signed_zero(M)
    z = x[x == 0.0]
    assert np.any(np.signbit(z)) and not np.all(np.signbit(z))                       # one run holds both signs of zero
    assert np.array_equal(rank_codes(x), rank_codes(x + 0.0))
    if M >= 8065:
        assert run_lengths(x).max() > 4096
    x = b_one_sided(M)
    f, med = fold(x)
    if M >= 63:
        assert med == 1.0 and np.count_nonzero(f == 0.0) >= 2 and cross_side_share(x) == 0.0
        for side in (x < med, x > med):                                              # tie runs of either side alone
            longest = run_lengths(f[side]).max()
            assert longest >= 2 and (M < 400000 or longest > 4096)


@pytest.mark.parametrize("M", SIDE_M)
def test_side_builders_do_what_they_say(M):
    assert np.unique(b_two(M)).size == 2
    assert np.all(rank_codes(b_const(M)) == M)
    a, d = b_ascending(M), b_descending(M)
    assert np.all(np.diff(a) > 0) and np.all(np.diff(d) < 0)
    parts = chains_of(b_disjoint(M))
    assert all(parts[i].min() > parts[i + 1].max() for i in range(len(parts) - 1))
    x = b_subnormal(M)
    tiny = np.finfo(np.float64).tiny
    assert np.all(np.abs(x) < tiny) and 2 <= np.unique(x).size <= 40
    assert np.all(fold(x)[0] < tiny)
    x = b_huge(M)
    assert np.all(np.isfinite(x)) and np.abs(x).max() > 1e300 and np.all(np.isfinite(fold(x)[0]))


@pytest.mark.parametrize("L", STAIR_L)
def test_staircase_runs_have_length_l(L):
    for M in (m for m in STAIR_M if m >= 4 * L):
        x = b_staircase(M, L)
        cnt = run_lengths(x)
        assert np.all(cnt[:-1] == L) and cnt[-1] == (M % L or L) and cnt.size >= 4
        assert not np.array_equal(x, np.sort(x))
