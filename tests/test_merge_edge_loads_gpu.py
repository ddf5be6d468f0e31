"""The edge neighbours of the fold and bucket merges, at the shapes where their loads can go wrong.

A fold workgroup (4032 outputs of the `|x - median|` order) and a bucket-merge workgroup (one bucket of the pooled order) decide
from the element just before and just behind their block in every run whether their first / last tie run goes on outside.  The
kernels load those neighbours together with the gather, from an index clamped into the array, whether the neighbour exists or
not, and compare after the merge.  A clamped load that is not ignored, a neighbour taken from the wrong run or the wrong
parameter, or a flag that stays set gives draws at a block edge a wrong tie run -- half a rank, which the statistics' 1e-9 gates
do not see.  So every case here compares the rank code and z of EVERY draw exactly (the debug hand-back of
`mcr_diagnose_chains` and the gate of tests/test_rank_codes_gpu.py) and the summary (`q`, `median`, `lag_*`, R-hat, ESS) with
the oracle.

Each fixture states on the CPU, from the sorted data alone, the configuration it is there for -- no draw below the median, a tie
run across output 4032 of the folded order from one run only, a bucket piece that starts at the first or ends at the last draw
of its tile, a tie run cut by a bucket in some tiles and not in others (by a numpy model of the sample partition) -- so that it
cannot quietly test something easier.  Those statements run inside the GPU tests, before the device is asked anything.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_hip_parity import TIGHT, check_summary, close
from test_rank_codes_gpu import ROUTE_KEYS, check_ranks_and_z
from test_rank_refs_cpu import b_iid, b_round1, chains_of, fold, median_of, same_bits

pytestmark = pytest.mark.gpu

TILE, FOLD_BLOCK = 4096, 4032


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def rng_of(*key):
    return np.random.default_rng(list(key))


def check_one_parameter(ctx, oracle, x, chains, what, min_chains=2):
    """Ranks and z of every draw, the diagnostics against the oracle, the median in bits.  Returns the kernel's result."""
    got = ctx.diagnose_chains(chains, min_chains=min_chains, debug=True)
    med = check_ranks_and_z(got, x, what)
    exp = oracle.diag(chains, min_chains)
    for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
        assert close(got[k], exp[k], TIGHT), (what, k, got[k], exp[k])
    assert (got["lag_bulk"], got["lag_tail"]) == (exp["lag_bulk"], exp["lag_tail"]), what
    assert same_bits(got["median"], med), (what, "median", got["median"], med)
    return got


def check_tensor(ctx, oracle, x, what, per_param):
    """`summarize` of [P][C][N], f64 or f32, against the oracle on the same tensor (q bit-exact, median, lags) and against
    `per_param`, the per-draw checked results of the same chains, in bits, which ties the per-parameter offsets down."""
    for name, t in (("pcn", x), ("cnp", np.ascontiguousarray(np.transpose(x, (1, 2, 0))))):
        got = ctx.summarize(t, name, min_chains=2)
        check_summary(got, oracle.summarize(t, name, min_chains=2), what=f"{what} {name}")
        if per_param is not None:
            for p, ref in enumerate(per_param):
                for k in ROUTE_KEYS:
                    same = int(got[k][p]) == int(ref[k]) if k.startswith("lag") else same_bits(float(got[k][p]), float(ref[k]))
                    assert same, (what, name, p, k, got[k][p], ref[k])


# ---------------------------------------------------------------------------------------------------------------------
# Fold: no neighbour on a side
# ---------------------------------------------------------------------------------------------------------------------


def b_median_at_end(M, top, seed=61):
    """More than half the draws are one value at the bottom (top: at the top) of the sample, the others distinct."""
    rng = rng_of(seed, M)
    n_eq = M // 2 + M // 8 + 1
    x = np.concatenate([np.zeros(n_eq), 1.0 + rng.permutation(M - n_eq)])
    x = rng.permutation(x)
    return (-x if top else x) + 0.0


@pytest.mark.parametrize("top", [False, True], ids=["median_is_min", "median_is_max"])
@pytest.mark.parametrize("M", [5000, 9000])
def test_fold_without_draws_on_one_side_of_the_median(ctx, oracle, M, top):
    """s = #(x < med) = 0: the run that is walked downwards is empty (na = 0, abase = -1) and every neighbour index of it is
    clamped; the mirror has no draw above the median, and the run of folded zeros crosses every block edge."""
    x = b_median_at_end(M, top)
    med = median_of(x)
    if top:
        assert med == x.max() and np.count_nonzero(x > med) == 0 and np.count_nonzero(x == med) > M // 2
    else:
        assert med == x.min() and np.count_nonzero(x < med) == 0 and np.count_nonzero(x == med) > M // 2
    assert M > FOLD_BLOCK
    check_one_parameter(ctx, oracle, x, chains_of(x), f"M={M} top={top}")


@pytest.mark.parametrize("kind", ["iid", "round1"])
@pytest.mark.parametrize("M", [4032, 4033])
def test_fold_block_that_ends_both_runs(ctx, oracle, M, kind):
    """M = 4032: exactly one block, which ends both runs (ai1 = na, bi1 = nb: both neighbours behind it are clamped away);
    M = 4033: the second block has one output and one run is exhausted in front of it."""
    x = b_iid(M, seed=62) if kind == "iid" else b_round1(M, seed=63)
    assert (M + FOLD_BLOCK - 1) // FOLD_BLOCK == (1 if M == 4032 else 2)
    check_one_parameter(ctx, oracle, x, chains_of(x), f"M={M} {kind}")


@pytest.mark.parametrize("x", [[1.0, 2.0], [2.0, 2.0], [3.0, 1.0, 2.0], [1.0, 1.0, 2.0], [2.0, 1.0, 2.0]],
                         ids=["2-distinct", "2-equal", "3-distinct", "3-low-tie", "3-high-tie"])
def test_fold_of_two_and_three_draws(ctx, oracle, x):
    """M = 2 and M = 3 (one chain): every neighbour index is clamped on at least one side."""
    x = np.asarray(x)
    check_one_parameter(ctx, oracle, x, [x], f"x={x.tolist()}", min_chains=1)


# ---------------------------------------------------------------------------------------------------------------------
# Fold: a tie run across a block edge, from one run, the other, both, or none
# ---------------------------------------------------------------------------------------------------------------------


def b_fold_edge(M, tie, seed=64):
    """Even M, median exactly 0, M/2 draws on each side; the folded order is 10, 10, 12, 13, 14, ... (index t holds t + 10,
    from the draws below the median -- run A -- at odd t and from those above -- run B -- at even t), except at every block
    edge E = 4032, 8064 < M:
      "A":    indices E - 1 and E hold one value, both from run A;       "B": both from run B;
      "both": indices E - 2 .. E + 1 hold one value, two from each run;  "none": nothing (the neighbours exist and differ)."""
    assert M % 2 == 0
    val = np.arange(M, dtype=np.float64) + 10.0
    val[1] = 10.0
    side = (np.arange(M) % 2 == 0)                      # True: run B (x > med)
    side[0], side[1] = False, True
    edges = [E for E in (FOLD_BLOCK, 2 * FOLD_BLOCK) if E < M]
    fixed = np.zeros(M, dtype=bool)
    fixed[:2] = True
    for E in edges:
        if tie in ("A", "B"):
            val[E] = val[E - 1]
            side[E - 1:E + 1] = tie == "B"
        elif tie == "both":
            val[E - 2:E + 2] = val[E - 2]
            side[E - 2:E + 2] = [False, False, True, True]
        fixed[E - 4:E + 4] = True
    free = np.flatnonzero(~fixed)
    excess = int(side.sum()) - M // 2                   # balance the runs far from the edges
    flip = [i for i in free if side[i] == (excess > 0)][:abs(excess)]
    side[flip] = ~side[flip]
    x = np.where(side, val, -val)
    return rng_of(seed, M).permutation(x)


@pytest.mark.parametrize("tie", ["A", "B", "both", "none"])
@pytest.mark.parametrize("M", [4040, 8064, 8070])
def test_fold_tie_run_across_a_block_edge(ctx, oracle, M, tie):
    x = b_fold_edge(M, tie)
    f, med = fold(x)
    assert same_bits(med, 0.0) and np.count_nonzero(x < med) == M // 2 == np.count_nonzero(x > med)
    fs = np.sort(f)
    edges = [E for E in (FOLD_BLOCK, 2 * FOLD_BLOCK) if E < M]
    assert edges == {4040: [4032], 8064: [4032], 8070: [4032, 8064]}[M]
    for E in edges:
        v = fs[E]
        in_a, in_b = np.count_nonzero(x == -v), np.count_nonzero(x == v)
        if tie == "none":
            assert fs[E - 1] < v < fs[E + 1] and fs[E - 2] < fs[E - 1]        # the neighbours exist; no tie at the edge
        else:
            assert fs[E - 1] == v and (in_a, in_b) == {"A": (2, 0), "B": (0, 2), "both": (2, 2)}[tie]
            assert fs[E - 3] < v and (E + 2 >= M or fs[E + 2] > v)
    chains = list(x.reshape(2, M // 2))                                       # C = 2
    check_one_parameter(ctx, oracle, x, chains, f"M={M} tie={tie}")


# ---------------------------------------------------------------------------------------------------------------------
# Bucket merge.  A numpy model of the partition by regular sampling (k sorted runs, every 64th order statistic of each, a
# splitter at every D-th sample of the strict order (value, run, position)) tells where each bucket's pieces start and end.
# ---------------------------------------------------------------------------------------------------------------------


def bucket_cuts(x):
    """(sorted runs, cut[B + 1][k]): bucket b takes [cut[b][t], cut[b + 1][t]) of sorted run t."""
    M = len(x)
    R = TILE
    while (M + R - 1) // R > 16:
        R *= 2
    k = (M + R - 1) // R
    runs = [np.sort(x[t * R:(t + 1) * R]) for t in range(k)]
    D = (4096 - 64 - 79 * k) // 64
    samples = sorted((r[64 * j + 63], t, 64 * j + 63) for t, r in enumerate(runs) for j in range(len(r) // 64))
    B = max(1, (len(samples) + D - 1) // D)
    cut = np.zeros((B + 1, k), dtype=np.int64)
    cut[B] = [len(r) for r in runs]
    for b in range(1, B):
        v, ts, pos = samples[b * D - 1]
        for t, r in enumerate(runs):
            cut[b, t] = pos + 1 if t == ts else np.searchsorted(r, v, side="right" if t < ts else "left")
    assert np.all(np.diff(cut, axis=0) >= 0) and np.all(np.diff(cut, axis=0).sum(axis=1) <= 4032)
    return runs, cut


def edge_ties(runs, cut, b):
    """For the cut in front of bucket b >= 1: per run, does the bucket's first value also end the run's previous piece?"""
    first = min(r[c] for r, c in zip(runs, cut[b]) if c < len(r))
    return [bool(c > 0 and r[c - 1] == first) for r, c in zip(runs, cut[b])]


def b_bucket_shared_ties(M, seed=65):
    """round(20 z): ~120 values, every one of them in every tile, tie runs of up to ~80 draws per tile."""
    return np.round(20.0 * rng_of(seed, M).normal(size=M)) + 0.0


def b_bucket_apart(M, seed=66):
    """Tile 0 holds integers in [-100, 20], tile 1 integers in [18, 150], a short third tile (if any) integers in [-100, -60]:
    the middle bucket takes tile 0 up to its last draw and tile 1 from its first, the first bucket all of the short tile."""
    rng = rng_of(seed, M)
    parts = [np.round(rng.uniform(-100, 20, size=min(M, TILE))), np.round(rng.uniform(18, 150, size=min(M - TILE, TILE)))]
    if M > 2 * TILE:
        parts.append(np.round(rng.uniform(-100, -60, size=M - 2 * TILE)))
    return np.concatenate(parts) + 0.0


def assert_bucket_configuration(x, kind):
    M = len(x)
    runs, cut = bucket_cuts(x)
    B, k = cut.shape[0] - 1, cut.shape[1]
    assert k == (M + TILE - 1) // TILE and B >= 3
    if kind == "shared":
        # some bucket cut goes through a tie run in some tiles and not in others
        mixed = [b for b in range(1, B) if len(set(edge_ties(runs, cut, b))) == 2]
        assert mixed, "no bucket edge with a tie run cut in some tiles only"
    else:
        starts = [(b, t) for b in range(1, B) for t in range(k) if cut[b, t] == 0 and cut[b + 1, t] > 0]
        ends = [(b, t) for b in range(B - 1) for t in range(k) if cut[b + 1, t] == len(runs[t]) and cut[b, t] < len(runs[t])]
        assert starts, "no bucket after the first whose piece starts at the first draw of a tile"
        assert ends, "no bucket before the last whose piece ends at the last draw of a tile"
        if M % TILE:
            assert any(t == k - 1 for _, t in ends), "the short last tile does not end inside an inner bucket"
            assert len(runs[-1]) == M % TILE
        assert any(any(edge_ties(runs, cut, b)) for b in range(1, B))


BUCKET_CASES = [(8192, "shared"), (12288, "shared"), (8192, "apart"), (12288, "apart"), (10000, "apart"), (10000, "shared")]


def build_bucket(M, kind):
    return b_bucket_shared_ties(M) if kind == "shared" else b_bucket_apart(M)


@pytest.mark.parametrize("M,kind", BUCKET_CASES, ids=[f"{M}-{k}" for M, k in BUCKET_CASES])
def test_bucket_edges(ctx, oracle, M, kind):
    """2 and 3 tiles, several buckets; M = 10000 has a short last tile (1808 draws).  The chains are equal-length halves, so
    the pooled (tile) order is the order of the array."""
    x = build_bucket(M, kind)
    assert_bucket_configuration(x, kind)
    check_one_parameter(ctx, oracle, x, list(x.reshape(2, M // 2)), f"M={M} {kind}")


@pytest.mark.parametrize("M", [8192, 12288])
def test_three_parameters_all_equal_next_to_all_distinct(ctx, oracle, M):
    """P = 3: a tied parameter, an all-equal one (every neighbour equals the edge value, in every tile) and an all-distinct
    one (no neighbour does) in one tensor: a neighbour read at another parameter's offset changes one of them."""
    rows = [build_bucket(M, "shared"), np.full(M, 0.25), rng_of(67, M).permutation(M).astype(np.float64)]
    assert_bucket_configuration(rows[0], "shared")
    assert np.unique(rows[1]).size == 1 and np.unique(rows[2]).size == M
    x = np.stack(rows).reshape(3, 2, M // 2)
    per_param = [check_one_parameter(ctx, oracle, x[p].reshape(-1), list(x[p]), f"M={M} p={p}") for p in range(3)]
    check_tensor(ctx, oracle, x, f"M={M} P=3", per_param)


# ---------------------------------------------------------------------------------------------------------------------
# 32-bit positions and the f32-record route
# ---------------------------------------------------------------------------------------------------------------------


def fold_edge_ties(x):
    """Block edges of the folded order that a tie run crosses."""
    fs = np.sort(fold(x)[0])
    return [E for E in range(FOLD_BLOCK, len(x), FOLD_BLOCK) if fs[E - 1] == fs[E]]


def test_positions_of_32_bits(ctx, oracle):
    """M = 2 x 35 000 = 70 000 >= 65 536, P = 2: the `u32` position instantiations of both kernels (nine pre-merged runs of
    8192 draws), tied draws, so that tie runs cross bucket cuts and fold block edges."""
    M = 70000
    rows = [b_bucket_shared_ties(M, seed=68), b_round1(M, seed=69)]
    for r in rows:
        runs, cut = bucket_cuts(r)
        assert len(runs) == 9 and any(any(edge_ties(runs, cut, b)) for b in range(1, cut.shape[0] - 1))
        assert len(fold_edge_ties(r)) >= 4
    x = np.stack(rows).reshape(2, 2, M // 2)
    per_param = [check_one_parameter(ctx, oracle, x[p].reshape(-1), list(x[p]), f"M={M} p={p}") for p in range(2)]
    check_tensor(ctx, oracle, x, f"M={M} P=2", per_param)


@pytest.mark.parametrize("M", [8070, 12288])
def test_f32_records(ctx, oracle, M):
    """An f32 tensor takes the packed-record kernels (`k_bucket_merge32`, the fold merge on records).  Integer-valued draws
    that f32 holds exactly, with ties at bucket cuts and at fold block edges: the f32 summary equals the oracle's on the f32
    tensor, and in bits the f64 route whose draws are checked one by one."""
    rows = [b_bucket_shared_ties(M, seed=70), b_fold_edge(M, "both"), np.full(M, -3.0), b_bucket_apart(M, seed=71)]
    for r in rows:
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r)
    runs, cut = bucket_cuts(rows[0])
    assert any(any(edge_ties(runs, cut, b)) for b in range(1, cut.shape[0] - 1)) and fold_edge_ties(rows[0])
    assert fold_edge_ties(rows[1])
    x = np.stack(rows).reshape(4, 2, M // 2)
    per_param = [check_one_parameter(ctx, oracle, x[p].reshape(-1), list(x[p]), f"M={M} p={p}") for p in range(4)]
    check_tensor(ctx, oracle, x.astype(np.float32), f"f32 M={M}", per_param)
