"""Host reference of the f64 tile sort's records (mcr_kernels.hpp, k_tile_sort), and what the kernel relies on.

A record is the draw with its low 12 mantissa bits replaced by its tile slot, compared AS A DOUBLE; the 12 bits wait in a side
array by slot.  The kernel relies on three facts, checked here on random doubles of every magnitude, denormals and +-0:

* the record order never contradicts the draws' order where their upper 52 bits differ: sorting a tile by record and putting
  the low bits back yields an ascending tile unless two draws that TIE in their upper 52 bits come out against their low bits;
* record + low bits give the draw back, bit for bit (denormals and both zeros included), and the slot with it;
* live records are finite, never NaN, and pairwise distinct as doubles -- what makes a compare-exchange by minimum and maximum
  a permutation -- and the +inf pad sorts behind all of them.

`fallback_tiles` is the model of the kernel's decision that tests/test_tile_records_gpu.py counts against.
"""
from __future__ import annotations

import numpy as np

TILE = 4096
LOW = np.uint64(0xFFF)


def records_of(tile: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(records as float64, low bits as uint16) of up to 4096 finite draws; slot e = index."""
    bits = np.ascontiguousarray(tile, dtype=np.float64).view(np.uint64)
    slots = np.arange(bits.size, dtype=np.uint64)
    return ((bits & ~LOW) | slots).view(np.float64), (bits & LOW).astype(np.uint16)


def rebuild(rec: np.ndarray, low: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(keys, slots) of records in any order; `low` is indexed by slot."""
    bits = np.ascontiguousarray(rec, dtype=np.float64).view(np.uint64)
    slots = (bits & LOW).astype(np.int64)
    return ((bits & ~LOW) | low[slots].astype(np.uint64)).view(np.float64), slots


def record_sorted(tile: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The tile's keys and slots in record order."""
    rec, low = records_of(tile)
    with np.errstate(all="ignore"):
        order = np.argsort(rec, kind="stable")
    return rebuild(rec[order], low)


def falls_back(tile: np.ndarray) -> bool:
    keys, _ = record_sorted(tile)
    return bool(np.any(keys[1:] < keys[:-1]))


def fallback_tiles(x: np.ndarray) -> int:
    """How many 4096-draw tiles of the pooled draws x the kernel sorts as (key, position) pairs after all."""
    x = np.asarray(x, dtype=np.float64)
    return sum(falls_back(x[b:b + TILE]) for b in range(0, x.size, TILE))


def _doubles(rng, n):
    """Finite doubles of every exponent and sign, denormals, both zeros, and clusters that tie in their upper 52 bits."""
    any_bits = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    x = any_bits.view(np.float64).copy()
    x[~np.isfinite(x)] = 1.5
    x[: n // 8] = (rng.integers(0, 2 ** 52, size=n // 8, dtype=np.uint64)).view(np.float64)          # denormals
    x[n // 8: n // 4] *= -1.0
    x[n // 4: n // 4 + 8] = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, -2.0 ** -1022, 1.7976931348623157e308, -1.7976931348623157e308]
    k = n // 2
    x[k: k + 64] = (np.float64(3.25).view(np.uint64) + rng.permutation(64).astype(np.uint64)).view(np.float64)
    x[k + 64: k + 128] = -(np.float64(1e-320).view(np.uint64) + rng.permutation(64).astype(np.uint64)).view(np.float64)
    return rng.permutation(x)


def test_record_and_low_bits_give_the_draw_back():
    rng = np.random.default_rng(81)
    for n in (1, 37, 4095, 4096):
        x = _doubles(rng, max(n, 512))[:n]
        rec, low = records_of(x)
        assert np.isfinite(rec).all()
        keys, slots = rebuild(rec, low)
        assert np.array_equal(keys.view(np.uint64), x.view(np.uint64)) and np.array_equal(slots, np.arange(n))
        p = rng.permutation(n)
        keys, slots = rebuild(rec[p], low)
        assert np.array_equal(keys.view(np.uint64), x[p].view(np.uint64)) and np.array_equal(slots, p)


def test_live_records_are_distinct_doubles_below_the_pad():
    rng = np.random.default_rng(82)
    for trial in range(8):
        x = _doubles(rng, TILE)
        x[0] = (0.0, -0.0)[trial % 2]                       # the one slot whose record can be a zero
        rec, _ = records_of(x)
        assert np.unique(rec).size == TILE                  # np.unique compares as doubles: -0.0 == +0.0 would merge
        assert np.all(rec < np.inf) and not np.isnan(rec).any()
        lo, hi = np.minimum(rec[:-1], rec[1:]), np.maximum(rec[:-1], rec[1:])
        both = np.sort(np.stack([rec[:-1], rec[1:]]).view(np.uint64), axis=0)
        assert np.array_equal(np.sort(np.stack([lo, hi]).view(np.uint64), axis=0), both)      # min / max: the operands' own bits


def test_record_order_is_the_draws_order_up_to_ties_in_the_upper_52_bits():
    rng = np.random.default_rng(83)
    for trial in range(8):
        x = _doubles(rng, TILE)
        rec, _ = records_of(x)
        up = x.view(np.uint64) & ~LOW
        i, j = rng.integers(0, TILE, size=(2, 200000))
        differ = up[i] != up[j]
        # (+-0 tie as draws and as upper bits alike; a draw pair whose upper bits differ never ties)
        assert np.array_equal((x[i] < x[j])[differ], (rec[i] < rec[j])[differ])
        keys, slots = record_sorted(x)
        assert sorted(slots.tolist()) == list(range(TILE))
        wrong = np.flatnonzero(keys[1:] < keys[:-1])
        ku = keys.view(np.uint64) & ~LOW
        assert np.all(ku[wrong] == ku[wrong + 1])           # every descent is inside a run of equal upper bits
        assert falls_back(x) == (wrong.size > 0)


def test_what_falls_back_and_what_does_not():
    rng = np.random.default_rng(84)
    iid = rng.normal(size=40000)
    assert fallback_tiles(iid) == 0
    assert fallback_tiles(np.round(iid, 2) + 0.0) == 0                  # equal keys in slot order ascend (weakly)
    z = iid.copy(); z[::3] = 0.0; z[1::6] = -0.0
    assert fallback_tiles(z) == 0                                       # -0.0 before +0.0 or after: equal
    ladder = 1.0 + rng.permutation(40000) * 2.0 ** -52
    assert fallback_tiles(ladder) == 10 and fallback_tiles(-ladder) == 10
    asc = 1.0 + np.arange(4096) * 2.0 ** -52
    assert fallback_tiles(asc) == 0 and fallback_tiles(asc[::-1]) == 1  # low bits with the slots / against them
    assert fallback_tiles(-asc) == 0 and fallback_tiles(-asc[::-1]) == 1    # (negative records descend with their slots, as their draws do here)
    assert record_sorted(-asc)[1].tolist() == list(range(4095, -1, -1))
    assert fallback_tiles(np.array([3.0])) == 0
    f32 = rng.normal(size=8229).astype(np.float32).astype(np.float64)
    f32[:100] = f32[100:200]
    assert fallback_tiles(f32) == 0                                     # widened f32: the low 29 bits are zero
    den = rng.permutation(4097) * 5e-324
    assert fallback_tiles(den) == 1 and fallback_tiles(den[:4096][np.argsort(den[:4096])]) == 0
