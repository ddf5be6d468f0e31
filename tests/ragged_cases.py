"""Inputs shared by the ragged-chain tests (test_layout_refs_cpu.py, test_ragged_batch_gpu.py, test_ragged_routes_gpu.py):
draws [P][M] of P parameters whose chains differ in length, regenerated from a seed, and small id columns for the row
order.  No GPU, no library: numpy only."""
from __future__ import annotations

import numpy as np

# name: (P, chain lengths, kind, min_chains)
RAGGED = {
    "one_draw_chain": (3, [7, 1, 6, 5, 9], "iid", 4),            # odd lengths, a chain of one draw
    "four_short": (3, [9, 7, 8, 11], "iid", 4),
    "two_chains": (1, [5, 3], "iid", 2),                         # a shortest chain of 3 draws: nh = 1, rhat NaN
    "small": (5, [40, 30, 35, 40], "iid", 4),
    "seg_switch_iid": (3, [1300, 1025, 1100, 2049], "iid", 4),   # staged prefix crosses 1024: 2048-draw segments, tier 2
    "seg_switch_ar95": (3, [1300, 1025, 1100, 2049], "ar0.95", 4),
    "sticky_ar995": (2, [1500, 1400, 1450, 1350], "ar0.995", 4),  # oracle lags >= 256: tier 3 with two parameters
    "random_walks": (3, [21000, 17500, 30000], "rw", 1),         # n >= 16 384: the long-chain rounds and the FFT tier
}
SEEDS = {"sticky_ar995": 8}      # chosen so that three of its four (parameter, kind) walks pass lag 256 and one stops in tier 2
REFERENCE_CASES = ("one_draw_chain", "four_short", "two_chains")   # small enough for the pure-Python reference


def make(name: str):
    """(x [P][M] float64, counts int64) of a RAGGED case."""
    P, lengths, kind, _mc = RAGGED[name]
    rng = np.random.default_rng(SEEDS.get(name, sorted(RAGGED).index(name) + 20240))
    rows = []
    for _p in range(P):
        parts = []
        for n in lengths:
            e = rng.normal(size=n)
            if kind == "iid":
                parts.append(e)
            elif kind == "rw":
                parts.append(np.cumsum(e) * 0.01)
            else:
                phi = float(kind[2:])
                v = np.empty(n)
                acc = e[0] / np.sqrt(1.0 - phi * phi)
                for i in range(n):
                    acc = phi * acc + e[i] if i else acc
                    v[i] = acc
                parts.append(v)
        rows.append(np.concatenate(parts))
    return np.ascontiguousarray(np.stack(rows)), np.asarray(lengths, dtype=np.int64)


def chains_of(row: np.ndarray, counts) -> list[list[float]]:
    off = np.concatenate([[0], np.cumsum(counts)])
    return [row[off[c]:off[c + 1]].tolist() for c in range(len(counts))]


def reference_order(chain, draw) -> list[int]:
    """Row numbers in the order in which `_chains_from_table` (src/mcmc_ref/convert.py:150-161) emits a parameter's
    values: rows bucketed by int(chain) as they come, the buckets walked in ascending chain id, each bucket sorted by
    its draw index with Python's stable sort."""
    buckets: dict[int, list[tuple[int, int]]] = {}
    for row, (c, d) in enumerate(zip(chain, draw)):
        buckets.setdefault(int(c), []).append((int(d), row))
    out: list[int] = []
    for c in sorted(buckets):
        out.extend(row for _d, row in sorted(buckets[c], key=lambda t: t[0]))
    return out


def id_columns(M: int, pattern: str, seed: int = 0):
    """(chain, draw) int64 columns of M rows: `pattern` in ordered / reversed / shuffled / interleaved / single /
    duplicates.  Four chains of unequal length unless the pattern says otherwise."""
    rng = np.random.default_rng(seed + M)
    cuts = np.sort(rng.integers(0, M + 1, size=3)) if M else np.zeros(3, dtype=np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [M]]))
    chain = np.repeat(np.arange(4, dtype=np.int64), counts)
    draw = np.concatenate([np.arange(n, dtype=np.int64) for n in counts]) if M else np.zeros(0, dtype=np.int64)
    if pattern == "ordered":
        return chain, draw
    if pattern == "reversed":
        return chain[::-1].copy(), draw[::-1].copy()
    if pattern == "shuffled":
        p = rng.permutation(M)
        return chain[p], draw[p]
    if pattern == "interleaved":                      # draw-major: all chains' draw 0, then draw 1, ...
        p = np.lexsort((chain, draw))
        return chain[p], draw[p]
    if pattern == "single":
        p = rng.permutation(M)
        return np.full(M, 3, dtype=np.int64), np.arange(M, dtype=np.int64)[p]
    if pattern == "duplicates":                       # few distinct (chain, draw) pairs: ties keep file order
        return rng.integers(0, 3, size=M).astype(np.int64), rng.integers(0, 5, size=M).astype(np.int64)
    raise ValueError(pattern)
