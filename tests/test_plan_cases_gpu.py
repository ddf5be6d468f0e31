"""The planning calls (mcr_plan_chunks, mcr_plan_chunks_chains, mcr_nested_plan, mcr_sliced_plan) against recorded
answers: tests/golden/plan_cases.json holds, per call shape, workspace limits with the units per chunk and the return code
the library gave for them when the file was made -- the full count, 1, values strictly between and MCR_ENOMEM wherever a
limit of at least 1 MiB (the smallest mcr_set_workspace_limit accepts) reaches them.  Planning launches nothing; every row
must come out exactly as recorded."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import load_json

pytestmark = pytest.mark.gpu

DEFAULT_LIMIT = 8 << 30
GOLDEN = load_json("plan_cases.json")


def plan(ctx, call: str, args: dict) -> tuple[int, int]:
    """(return code, units per chunk) of one planning call under the context's current workspace limit."""
    L, v = ctx.lib, C.c_int64(-1)
    if call == "plan_chunks":
        rc = L.mcr_plan_chunks(ctx.handle, args["C"], args["N"], args["P"], args["sc"], args["sn"], args["sp"],
                               args["diagnostics"], C.byref(v))
    elif call == "plan_chunks_chains":
        off = np.ascontiguousarray(args["chain_off"], dtype=np.int64)
        rc = L.mcr_plan_chunks_chains(ctx.handle, off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1, args["P"],
                                      args["diagnostics"], C.byref(v))
    elif call == "nested_plan":
        rc = L.mcr_nested_plan(ctx.handle, args["dtype"], args["C"], args["N"], args["P"], args["sc"], args["sn"],
                               args["sp"], args["K"], C.byref(v))
    elif call == "sliced_plan":
        rc = L.mcr_sliced_plan(ctx.handle, args["Mr"], args["Ma"], args["P"], args["K"], C.byref(v))
    else:
        raise ValueError(call)
    return int(rc), int(v.value)


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip._ffi import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_plans_equal_the_record(ctx, name):
    case = GOLDEN["cases"][name]
    assert case["rows"]
    try:
        for row in case["rows"]:
            ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, row["limit"]))
            rc, units = plan(ctx, case["call"], case["args"])
            print(name, row["limit"], "->", rc, units, "recorded", row["rc"], row["units"])
            assert rc == row["rc"], (name, row, rc, units)
            if rc == 0:
                assert units == row["units"], (name, row, units)
    finally:
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, DEFAULT_LIMIT))
