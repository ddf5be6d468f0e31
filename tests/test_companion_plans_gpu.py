"""The chunk plans of the companion libraries do not move: for every shape of tests/golden/companion_plans.json and every
parameters-per-chunk value a workspace limit can yield, the smallest limit in bytes that yields it is the recorded one,
byte for byte.  The table was recorded on the device at the commit it names, before the plans of mci_api.hip and
mcs_api.hip were put on the shared carving and fitting tools; the plan is monotone in the limit and does no device work,
so each edge is found by bisection.  libmcmcref_bm.so has no plan entry: test_alone_chunked_repeated_and_profiled pins its
arithmetic.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import load_json

TOP = 1 << 40          # a limit under which every shape here fits whole


def ask(case: dict, limit: int, ctx) -> int:
    """Parameters per chunk of the case's shape under `limit` bytes; 0 when not even one parameter fits."""
    from mcmc_ref_hip import indicator, standard
    from mcmc_ref_hip._abi import McrError
    C_, N, P = case["C"], case["N"], case["P"]
    try:
        if case["library"] == "mci":
            indicator.set_workspace_limit(limit, ctx)
            return indicator.params_per_chunk(C_, N, P, case["K"], np.float64, ctx)
        standard.set_workspace_limit(limit, ctx)
        return standard.params_per_chunk(C_, N, P, np.float64, case["basic"], tuple(case["strides"]), ctx)
    except McrError:
        return 0


def smallest_limits(case: dict, ctx) -> list[list[int]]:
    """[parameters per chunk, the smallest limit that yields it], ascending, for every value above 0 a limit yields."""
    steps, top = [], ask(case, TOP, ctx)
    have, lo = ask(case, 1, ctx), 1
    assert have == 0 and top >= 1
    while have < top:
        hi = TOP                                        # ask(lo) == have < ask(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if ask(case, mid, ctx) > have:
                hi = mid
            else:
                lo = mid
        have, lo = ask(case, hi, ctx), hi
        steps.append([have, hi])
    return steps


@pytest.mark.gpu
def test_smallest_limits_are_the_recorded_ones():
    from mcmc_ref_hip import _ffi
    table = load_json("companion_plans.json")
    assert len(table["cases"]) == 5
    with _ffi.Context(0) as ctx:
        for case in table["cases"]:
            got = smallest_limits(case, ctx)
            assert got == case["steps"], (case, got)
            assert [s[0] for s in got][-1] == case["P"]
