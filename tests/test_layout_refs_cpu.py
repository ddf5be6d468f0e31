"""What the device row order and the batched ragged-chain calls are tested against, pinned on the CPU.

* np.lexsort((draw, chain)) -- the expression the GPU tests compare mcr_chain_layout_dev with -- IS the order in which
  the reference's `_chains_from_table` (src/mcmc_ref/convert.py:150-161) emits values: checked against a pure-Python
  restatement of that function's bookkeeping (ragged_cases.reference_order), duplicated (chain, draw) pairs included.
* The oracle (oracle.diag) equals mcmc_ref.diagnostics on the small ragged cases (tests/golden/ragged_cases.json,
  recorded from the imported reference), and the ragged inputs have the properties their GPU cases are named for."""
from __future__ import annotations

import math

import numpy as np
import pytest

import ragged_cases
from conftest import load_json, same_float

PATTERNS = ("ordered", "reversed", "shuffled", "interleaved", "single", "duplicates")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", [0, 1, 2, 7, 255, 257, 1000])
def test_lexsort_is_the_reference_order(M, pattern):
    chain, draw = ragged_cases.id_columns(M, pattern)
    assert np.lexsort((draw, chain)).tolist() == ragged_cases.reference_order(chain, draw)


def test_lexsort_is_the_reference_order_wide_ids():
    rng = np.random.default_rng(5)
    chain = rng.choice(np.array([-5, 0, 2**40], dtype=np.int64), size=500)
    draw = rng.integers(-3, 2**20, size=500).astype(np.int64)
    draw[::7] = draw[0]                                   # ties inside a chain
    assert np.lexsort((draw, chain)).tolist() == ragged_cases.reference_order(chain, draw)
    ids, counts = np.unique(chain, return_counts=True)    # the reference walks sorted(buckets): ascending ids
    assert ids.tolist() == sorted(set(chain.tolist())) and counts.sum() == 500


def _dec(v):
    return math.nan if v is None else float(v)


@pytest.mark.parametrize("name", ragged_cases.REFERENCE_CASES)
def test_oracle_equals_reference_on_small_ragged_cases(oracle, name):
    x, counts = ragged_cases.make(name)
    mc = ragged_cases.RAGGED[name][3]
    exp = load_json("ragged_cases.json")[name]
    assert len(exp) == x.shape[0]
    for row, e in zip(x, exp):
        got = oracle.diag(ragged_cases.chains_of(row, counts), mc)
        for k in ("rhat", "ess_bulk", "ess_tail"):
            assert same_float(got[k], _dec(e[k])), (name, k, got[k], e[k])


def test_one_draw_chain_case_has_nan_ess_and_finite_rhat(oracle):
    x, counts = ragged_cases.make("one_draw_chain")
    assert 1 in counts.tolist()
    for row in x:
        d = oracle.diag(ragged_cases.chains_of(row, counts), 4)
        assert math.isnan(d["ess_bulk"]) and math.isnan(d["ess_tail"]) and math.isfinite(d["rhat"])


def test_two_chain_case_has_nan_rhat(oracle):
    x, counts = ragged_cases.make("two_chains")
    d = oracle.diag(ragged_cases.chains_of(x[0], counts), 2)
    assert math.isnan(d["rhat"]) and math.isfinite(d["ess_bulk"])


def _lags(oracle, name):
    x, counts = ragged_cases.make(name)
    mc = ragged_cases.RAGGED[name][3]
    out = []
    for row in x:
        d = oracle.diag(ragged_cases.chains_of(row, counts), mc)
        out += [d["lag_bulk"], d["lag_tail"]]
    return out


def test_sticky_cases_reach_the_tiers_they_are_named_for(oracle):
    assert max(_lags(oracle, "seg_switch_iid")) < 64                 # decided by tier 1
    assert max(_lags(oracle, "seg_switch_ar95")) >= 64               # tier 2 (lags 64 .. 255)
    lags = _lags(oracle, "sticky_ar995")
    assert max(lags) >= 256                                          # tier 3
    assert sum(l >= 256 for l in lags) >= 2                          # ... for more than one (parameter, kind) pair
    assert max(_lags(oracle, "random_walks")) >= 256


NEW_SYMBOLS = ("mcr_summarize_chains_enqueue", "mcr_summarize_chains_dev", "mcr_plan_chunks_chains",
               "mcr_chain_layout_dev", "mcr_chain_layout_many_dev", "mcr_gather_rows_order_dev")


def test_the_library_exports_the_ragged_and_layout_symbols():
    """Declared in the header, bound by _ffi and exported by the built library (no GPU needed to load it)."""
    import ctypes
    import importlib.util
    import re

    from conftest import ROOT
    from mcmc_ref_hip import _ffi
    spec = importlib.util.spec_from_file_location("mcr_build", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(str(mod.build()))
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mcmcref_hip.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _ffi.SYMBOLS and hasattr(lib, name), name
    span = int(re.search(r"#define MCR_LAYOUT_SPAN (\d+)", (ROOT / "include" / "mcmcref_hip.h").read_text()).group(1))
    assert span >= 256 and span % 256 == 0            # whole rounds of a 256-thread workgroup


def test_ragged_tensor_describes_the_chains():
    """Context.ragged_tensor's bookkeeping (offsets, shortest chain, stride) without a device."""
    from mcmc_ref_hip import _ffi
    t = _ffi.Context.ragged_tensor(None, buf=None, counts=[7, 1, 6], P=3)
    assert t.chain_off.tolist() == [0, 7, 8, 14] and t.chain_off.dtype == np.int64
    assert t.targs == (_ffi.MCR_F64, 3, 1, 3, 0, 1, 14)
    assert _ffi.Context.ragged_tensor(None, None, [4, 2], 2, stride_p=9).targs[6] == 9
