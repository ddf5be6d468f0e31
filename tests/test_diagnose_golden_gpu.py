"""mcr_diagnose_chains against a record of its own results: tests/golden/diagnose_cases.json holds, per case, the
floating-point results as 64-bit integer views, the truncation lags, and a SHA-256 of each per-draw debug array (z and
decoded rank of every draw, bulk and tail, in pooled order; the arrays themselves would not fit a fixture).  The draws
come from fixed seeds here, so the fixture holds results only.  Every case must come out bit for bit as recorded: the
entry shares the host path of the batched ragged calls, and tests/test_ragged_batch_gpu.py compares those two with each
other -- this file is what holds both to what the library gave before they were joined.

Cases: every chain set of unit_vectors.json that runs, the first parameter of each small case of ragged_cases.py, a
single chain, 4097 pooled draws (one more than a sort tile), 65 535 and 65 536 pooled draws (16-bit and 32-bit
positions), a shortest chain one past the FFT threshold with and without the FFT tier, an empty pool, and the return
codes of tables the entry refuses."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

import ragged_cases
from conftest import load_json

pytestmark = pytest.mark.gpu

FLOATS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "median")
LAGS = ("lag_bulk", "lag_tail")
DEBUG = ("z_bulk", "z_tail", "rank_bulk", "rank_tail")
UNIT = load_json("unit_vectors.json")


def normal_chains(seed: int, lengths) -> list[np.ndarray]:
    rng = np.random.default_rng(seed)
    return [rng.normal(size=n) for n in lengths]


def walk_chains(seed: int, lengths) -> list[np.ndarray]:
    """Random walks: both kinds pass lag 256, so chains past the FFT threshold take the FFT tier."""
    rng = np.random.default_rng(seed)
    return [np.cumsum(rng.normal(size=n)) * 0.01 for n in lengths]


def cases() -> dict:
    """name -> (chains, min_chains, engine); engine "fft" is the default context, "direct" one made under MCR_FFT=0."""
    out = {}
    for name, rec in UNIT.items():
        if name.startswith("_"):
            continue
        for key, mc in (("min4", 4), ("min1", 1)):
            if not isinstance(rec[key]["rhat"], dict):                # (a dict there: the reference raises)
                out[f"unit-{name}-{key}"] = (rec["chains"], mc, "fft")
    for name, (_P, _lengths, _kind, mc) in ragged_cases.RAGGED.items():
        if name != "random_walks":
            x, counts = ragged_cases.make(name)
            out[f"ragged-{name}"] = (ragged_cases.chains_of(x[0], counts), mc, "fft")
    out["single_chain"] = (normal_chains(1, [100]), 1, "fft")
    out["tile_plus_one"] = (normal_chains(2, [1366, 1365, 1366]), 2, "fft")
    out["pool_65535"] = (normal_chains(3, [16384, 16383, 16384, 16384]), 4, "fft")
    out["pool_65536"] = (normal_chains(4, [16384, 16384, 16384, 16384]), 4, "fft")
    out["fft_threshold-fft"] = (walk_chains(5, [16385, 16400]), 2, "fft")
    out["fft_threshold-direct"] = (walk_chains(5, [16385, 16400]), 2, "direct")
    out["empty_pool"] = ([[], []], 2, "fft")
    return out


CASES = cases()
GOLDEN = load_json("diagnose_cases.json")


def record(ctx, chains, mc) -> dict:
    """The full result of diagnose_chains(debug=True) in the fixture's form."""
    r = ctx.diagnose_chains(chains, mc, debug=True)
    rec = {k: int(np.float64(r[k]).view(np.int64)) for k in FLOATS}
    rec.update({k: int(r[k]) for k in LAGS})
    for k in DEBUG:
        flat = np.concatenate([np.asarray(a, dtype="<f8") for a in r[k]]) if r[k] else np.zeros(0, dtype="<f8")
        rec[k] = {"n": int(flat.size), "sha256": hashlib.sha256(flat.tobytes()).hexdigest()}
    return rec


@pytest.fixture(scope="module")
def engines():
    from mcmc_ref_hip import _ffi
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MCR_FFT", "0")
        direct = _ffi.Context(0)
    fft = _ffi.Context(0)
    yield {"fft": fft, "direct": direct}
    fft.close()
    direct.close()


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_equal_the_record_in_bits(engines, name):
    chains, mc, engine = CASES[name]
    got, exp = record(engines[engine], chains, mc), GOLDEN["cases"][name]
    print(name, got)
    assert got == exp, (name, {k: (got[k], exp[k]) for k in exp if got.get(k) != exp[k]})


def test_empty_pool_is_nan(engines):
    r = engines["fft"].diagnose_chains([[], []], 2, debug=True)
    assert all(np.isnan(r[k]) for k in FLOATS) and (r["lag_bulk"], r["lag_tail"]) == (0, 0)


def test_fft_threshold_case_reaches_tier_three():
    exp = GOLDEN["cases"]["fft_threshold-fft"]
    assert min(exp["lag_bulk"], exp["lag_tail"]) >= 255, exp          # both pairs listed: the FFT tier serves them


def raw_call(ctx, off, min_chains: int, n_chains: int | None = None) -> int:
    """mcr_diagnose_chains on the table `off` as it stands (the wrapper always builds one that starts at 0)."""
    from mcmc_ref_hip._ffi import SummaryBuffers
    off = np.ascontiguousarray(off, dtype=np.int64)
    pooled = np.linspace(0.0, 1.0, max(int(off.max(initial=0)), 1))
    bufs = SummaryBuffers(1, 0)
    nc = len(off) - 1 if n_chains is None else n_chains
    return int(ctx.lib.mcr_diagnose_chains(ctx.handle, pooled.ctypes.data_as(C.POINTER(C.c_double)),
                                           off.ctypes.data_as(C.POINTER(C.c_int64)), nc, min_chains,
                                           C.byref(bufs.struct), None, None, None, None))


def test_refused_tables(engines):
    from mcmc_ref_hip._ffi import MCR_EINVAL, MCR_OK, McrError
    ctx = engines["fft"]
    with pytest.raises(McrError) as ei:                               # min_chains = 0 is not legal
        ctx.diagnose_chains([], 0)
    assert ei.value.code == GOLDEN["empty_list_min_chains_0_rc"]
    assert raw_call(ctx, [0, 10, 20, 30, 40], 4) == MCR_OK
    assert raw_call(ctx, [1, 10, 20, 30, 40], 4) == MCR_EINVAL        # draws in front of chain 0 belong to no chain
    assert raw_call(ctx, [0, 10, 8, 30, 40], 4) == MCR_EINVAL         # decreasing
    assert raw_call(ctx, np.arange(258) * 2, 4) == MCR_EINVAL         # 257 chains
    assert raw_call(ctx, [0, 10, 20, 30, 40], 4) == MCR_OK            # the context stays usable
