"""The lag-edge fixture (golden/lag_edge_cases.json, lag_edge_cases.py) against the C oracle, on any host.

Every recipe rebuilds to the recorded bytes; the oracle puts its first negative rho of the bulk ESS at the recorded F
(`lag_bulk + 1 == F`) and its `lag_tail` at the recorded value, with |rho| >= 1e-6 at F and F - 1, far outside the guard
band; and the fixture holds every (route, C, F) of lag_edge_cases.TABLE, each at a chain length of its route -- the
condition that keeps test_lag_edges_gpu.py from silently missing a seam.

Oracle time per case (one thread, measured with `python tests/test_lag_edges_cpu.py`, which prints them): short under
0.005 s, one_stage under 0.01 s, segments 0.01 .. 0.04 s, long 0.03 .. 0.05 s, multi_stage 0.06 .. 0.21 s, long_round_end
(2 x 56 003 draws, F = 16 383 .. 16 385) 2.3, 2.6 and 2.0 s -- under the 10 s above which the fixture would have to carry
the oracle's results, so both tests compute them (the three long cases side by side on three threads: 2.9 s).
"""
from __future__ import annotations

import numpy as np
import pytest

import lag_edge_cases as lec

CASES = lec.load()
GROUPS = lec.groups(CASES)
ORACLE_THREADS = 16


def group_id(key) -> str:
    return f"{key[0]}-C{key[1]}-N{key[2]}"


@pytest.fixture(scope="module")
def tensors():
    return {key: lec.tensor(cases) for key, cases in GROUPS.items()}


def test_fixture_covers_every_route_chain_count_and_hand_over_lag():
    have = {(c["route"], c["C"], c["F"]) for c in CASES}
    want = {(route, C, F) for route, (_n, counts, targets) in lec.TABLE.items() for C in counts for F in targets}
    assert want <= have, sorted(want - have)
    assert len(CASES) == len(have), "a (route, C, F) twice"
    for c in CASES:
        lo, hi = lec.TABLE[c["route"]][0]
        assert lo <= c["N"] <= hi, c
    # the table itself: the hand-over lags of the kernels' constants, one lag to either side
    assert lec.around(64) == (63, 64, 65)
    assert set(lec.TABLE["short"][2]) == {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257}
    assert set(lec.TABLE["segments"][2]) == set(lec.TABLE["short"][2]) | {511, 512, 513, 767, 768, 769}
    assert set(lec.TABLE["one_stage"][2]) == {511, 512, 513, 767, 768, 769}
    assert set(lec.TABLE["multi_stage"][2]) == {767, 768, 769, 2303, 2304, 2305, 4351, 4352, 4353}
    assert set(lec.TABLE["long"][2]) == {255, 256, 257, 511, 512, 513}
    assert set(lec.TABLE["long_round_end"][2]) == {16383, 16384, 16385}


def test_builder_stays_in_range_and_separates_chains_and_seeds():
    e = lec.noise(3, 1, 4096)
    assert e.min() >= -1.0 and e.max() < 1.0 and abs(e.mean()) < 0.05
    assert not np.array_equal(e, lec.noise(3, 0, 4096)) and not np.array_equal(e, lec.noise(4, 1, 4096))
    w = lec.triangle(40, 10, 0)
    assert w[0] == 1.0 and w[5] == -1.0 and w[10] == 1.0 and np.array_equal(w[:10], w[10:20])
    assert 0 <= lec.phase(7, 2, 13) < 13
    x = lec.build(3, 500, 37, 5, 0.5)
    assert x.shape == (3, 500) and np.abs(x).max() < 1.5 and np.unique(x).size == x.size      # no ties


@pytest.mark.parametrize("key", list(GROUPS), ids=group_id)
def test_recipes_rebuild_to_the_recorded_bytes(tensors, key):
    for case, x in zip(GROUPS[key], tensors[key]):
        assert lec.sha256(x) == case["sha256"], case


@pytest.mark.parametrize("key", list(GROUPS), ids=group_id)
def test_oracle_lags_are_the_recorded_ones(oracle, tensors, key):
    exp = oracle.summarize_mt(tensors[key], "pcn", threads=ORACLE_THREADS, min_chains=1)
    for p, case in enumerate(GROUPS[key]):
        assert int(exp["lag_bulk"][p]) + 1 == case["F"], case
        assert int(exp["lag_tail"][p]) == case["lag_tail"], case


@pytest.mark.parametrize("key", list(GROUPS), ids=group_id)
def test_rho_at_the_decision_is_outside_the_guard_band(oracle, tensors, key):
    for case, x in zip(GROUPS[key], tensors[key]):
        z = np.stack(oracle.rank_normalize(list(x))[0])
        before, at = lec.rho(z, (case["F"] - 1, case["F"]))
        assert before >= lec.RHO_FLOOR and at <= -lec.RHO_FLOOR, (case, before, at)


if __name__ == "__main__":           # the oracle's time per case, on any host
    import sys
    import time
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root)]
    from oracle import oracle as orc
    orc.build()
    for case in CASES:
        x = lec.draws_of(case)[None]
        t0 = time.perf_counter()
        o = orc.summarize(x, "pcn", min_chains=1)
        dt = time.perf_counter() - t0
        print(f"{case['route']:15s} C={case['C']} N={case['N']:6d} F={case['F']:6d} lag_tail={int(o['lag_tail'][0]):6d} oracle {dt:6.3f} s")
