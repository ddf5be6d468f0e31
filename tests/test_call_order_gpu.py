"""Every entry behind every other on one context, in bits.

Every device buffer the library owns belongs to the context, grows through one rule, never shrinks and is never cleared
between calls: each call carves its own layout out of what the call before it left.  A kernel that reads a word its own
call never wrote -- a pad lane, a partial last tile, a counter "the last kernel re-initialised", a position array carved 16
bits wide over 32-bit entries -- is right on a quiet context and wrong behind another predecessor.  Memory from a first
hipMalloc is typically zero, so a family's own tests on a context that only ever saw that family cannot show it.

The families, their inputs and their references are tests/call_families.py (held honest without a GPU by
test_call_families_cpu.py).  Here:

a. `want(family, size)` is the family's call on a context of its own, held ONCE to the family's reference at the family's
   own gate; two fresh contexts agree in bits (no float path uses floating-point atomics), which is what lets everything
   below compare with `==`.  There is no tolerance in this file.  The baseline call runs on a context whose library
   notes every entry asked of it, as do the libraries of its two companion handles (mci_*, mcb_*: one handle per
   Context, with buffers of its own that only grow): the entries a family declares (the CPU test places every entry of
   the four ABI tables by these declarations) are the entries its run reaches, no more and no fewer.
b. With one lane (MCR_LANES=1: every call shares one workspace), for every predecessor A: two rounds over all families B of
   A at its large size, then B at its small size.  The first round grows the buffers; from the second on nothing
   reallocates, so B's carve lies in what A just used -- that round proves the ordered pair (A, B), and (B, A) small ->
   large with it.  The last test counts the pairs: F x F.
c. Every family behind every refused call (call_families.REFUSED), then the refusal's own family at its large size.
d. Default lanes: four summaries in flight fill every lane's workspace, then every synchronous family lands on the lane the
   last summary left current.  Again for the chain that crosses three handles in one call (mean_shift_test), the Gaussian
   check and the factorisation, at both sizes, and with a Gaussian check refused while the summaries are in flight.
e. summarize, diagnose_chains and nested_rhat at small, large, small with 25 other pooled lengths summarized in between:
   the cache of z tables (24 entries) evicts and rebuilds the table of the small length.

A failure names (predecessor, successor, round, first differing output field).  Nothing is skipped or filtered at run time.
"""
from __future__ import annotations

import collections

import numpy as np
import pytest

import call_families as F

pytestmark = pytest.mark.gpu

FAMILY = pytest.mark.parametrize("family", F.FAMILIES, ids=F.NAMES)
PAIRS: collections.Counter = collections.Counter()           # (predecessor, successor) -> second rounds that passed
Z_TABLES = 24                                                # kMaxZTabs of mcr_api.hip
OWN_BINDING = {"mcr_parquet_open", "mcr_parquet_close"}      # parquet.ParquetFile asks the library itself, not the context's


def fresh_context():
    from mcmc_ref_hip import _ffi
    return _ffi.Context(0)


ABI_PREFIXES = ("mcr_", "mcrx_", "mci_", "mcb_")              # the four ABI tables: _abi, _xabi, _iabi, _babi


class Recording:
    """A library (the context's, or a companion handle's), noting in `asked` the name of every entry asked of it."""

    def __init__(self, lib, asked: set):
        self.lib, self.asked = lib, asked

    def __getattr__(self, name):
        if name.startswith(ABI_PREFIXES):
            self.asked.add(name)
        return getattr(self.lib, name)


def companions(ctx) -> list:
    """The context's handles of the two companion libraries, made now if this context has none yet."""
    from mcmc_ref_hip import batchmeans, indicator
    return [indicator._handle(ctx), batchmeans._handle(ctx)]


_WANT: dict = {}


def want(family, size: str):
    """The family's call on a context of its own: made once, held to the family's reference once, never changed."""
    key = (family.name, size)
    if key not in _WANT:
        from mcmc_ref_hip import _xabi
        left_out = {s for symbols in F.NOT_IN_THE_MATRIX.values() for s in symbols}
        with fresh_context() as c:
            asked: set = set()
            owners = [c] + companions(c)                      # every library a run can reach hangs off one of these
            libs = [o.lib for o in owners]
            _xabi.bind(c.lib)                                 # (gaussian binds at first use: that is no call of an entry)
            for o in owners:
                o.lib = Recording(o.lib, asked)
            try:
                got = family.run(c, family.inputs(size))
            finally:
                for o, lib in zip(owners, libs):
                    o.lib = lib
            undeclared = asked - set(family.symbols) - left_out
            assert not undeclared, f"{family.name} reaches entries it does not declare: {sorted(undeclared)}"
            unreached = set(family.symbols) - asked - OWN_BINDING
            assert not unreached, f"{family.name} declares entries its run does not reach: {sorted(unreached)}"
            family.check(family.inputs(size), got, c)
        _WANT[key] = got
    return _WANT[key]


@pytest.fixture(scope="module")
def wants():
    """Every baseline, made before any test sets MCR_LANES."""
    return {(f.name, size): want(f, size) for f in F.FAMILIES for size in F.SIZES}


def same(got, expected, *what):
    if got != expected:
        pytest.fail(f"{what}: differs from the fresh context in output field {F.first_difference(got, expected)!r}", pytrace=False)


# ---- a. baselines ------------------------------------------------------------------------------------------------------

@FAMILY
def test_two_fresh_contexts_agree_in_bits(family):
    """What lets every test below ask for bit equality with a fresh context; the first context's result passed the
    family's reference gate inside want()."""
    for size in F.SIZES:
        expected = want(family, size)
        with fresh_context() as c:
            same(family.run(c, family.inputs(size)), expected, family.name, size)


def test_companion_handles_belong_to_one_context():
    """The handles of libmcmcref_iess.so and libmcmcref_bm.so are per Context: a fresh context has a workspace and an
    upload buffer of its own there too, which is what makes want() a baseline for the mci_ and mcb_ families."""
    with fresh_context() as a, fresh_context() as b:
        for ha, hb, again in zip(companions(a), companions(b), companions(a)):
            assert ha is again and ha is not hb and ha.handle.value and hb.handle.value and ha.handle.value != hb.handle.value
            assert ha.device == a.device == hb.device


# ---- b. every ordered pair ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("predecessor", F.FAMILIES, ids=F.NAMES)
def test_every_successor_behind(predecessor, wants, monkeypatch):
    monkeypatch.setenv("MCR_LANES", "1")
    A = predecessor
    with fresh_context() as c:
        for rnd in (1, 2):
            for B in F.FAMILIES:
                same(A.run(c, A.inputs("large")), wants[A.name, "large"], A.name, "behind", B.name, "round", rnd)
                same(B.run(c, B.inputs("small")), wants[B.name, "small"], B.name, "behind", A.name, "round", rnd)
                if rnd == 2:
                    PAIRS[A.name, B.name] += 1


# ---- c. behind a refusal -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refusal", F.REFUSED, ids=[r.name for r in F.REFUSED])
def test_every_family_behind_a_refused_call(refusal, wants, monkeypatch):
    monkeypatch.setenv("MCR_LANES", "1")
    with fresh_context() as c:
        for B in F.FAMILIES:
            refusal.call(c)                                   # asserts the code and the message
            same(B.run(c, B.inputs("small")), wants[B.name, "small"], B.name, "behind the refused", refusal.name)
        own = F.BY_NAME[refusal.family]
        refusal.call(c)
        same(own.run(c, own.inputs("large")), wants[own.name, "large"], own.name, "large, behind the refused", refusal.name)


# ---- d. default lanes --------------------------------------------------------------------------------------------------

def test_default_lanes(wants):
    """A synchronous call runs on the lane the last summary left current (the shared-lane comment of mcr_ctx): here behind
    four large summaries that went through every lane."""
    first, second = F.BY_NAME["summarize"], F.BY_NAME["enqueue"]
    i = second.inputs("large")
    with fresh_context() as c:
        t = c.upload(i["x"], i["layout"])
        try:
            bufs = [c.enqueue(t) for _ in range(4)]
            c.wait()
        finally:
            t.free()
        for k, b in enumerate(bufs):
            same(F.pack(b.result()), wants[second.name, "large"], second.name, "in flight", k)
        for B in F.FAMILIES:
            if B is not second:
                same(B.run(c, B.inputs("small")), wants[B.name, "small"], B.name, "behind four summaries in flight")
        same(first.run(c, first.inputs("large")), wants[first.name, "large"], first.name, "large, behind every small call")
        for B in F.FAMILIES:
            same(B.run(c, B.inputs("small")), wants[B.name, "small"], B.name, "behind", first.name, "large, default lanes")


def test_cross_handle_chain_behind_summaries_in_flight(wants):
    """mean_shift_test's driver lives in another library and calls mcr_covariance_dev, mcrx_cholesky_dev and
    mcrx_solve_lower_dev on the main context: here on the lane the last of four large summaries left current, as do
    gaussian_check and linalg.  With summaries in flight the Gaussian check is refused before it touches a buffer, and
    the summaries deliver the bits they would have."""
    from mcmc_ref_hip import _ffi
    second = F.BY_NAME["enqueue"]
    chain = [F.BY_NAME[name] for name in ("mean_shift_test", "gaussian_check", "linalg")]
    i = second.inputs("large")
    with fresh_context() as c:
        t = c.upload(i["x"], i["layout"])
        try:
            bufs = [c.enqueue(t) for _ in range(4)]
            c.wait()
            for k, b in enumerate(bufs):
                same(F.pack(b.result()), wants[second.name, "large"], second.name, "in flight", k)
            for size in F.SIZES:
                for B in chain:
                    same(B.run(c, B.inputs(size)), wants[B.name, size], B.name, size, "behind four summaries in flight")
            bufs = [c.enqueue(t) for _ in range(4)]
            g = F.BY_NAME["gaussian_check"]
            with pytest.raises(_ffi.McrError) as refused:
                g.run(c, g.inputs("small"))
            assert refused.value.code == _ffi.MCR_EINVAL and "summaries in flight" in refused.value.message, refused.value.message
            c.wait()
        finally:
            t.free()
        for k, b in enumerate(bufs):
            same(F.pack(b.result()), wants[second.name, "large"], second.name, "in flight around a refused Gaussian check", k)
        for B in chain:
            same(B.run(c, B.inputs("small")), wants[B.name, "small"], B.name, "small, behind the second four summaries")


@pytest.mark.parametrize("N", [63, 64, 65, 128])
def test_indicator_zero_word_behind_a_larger_call(N, wants):
    """k_lag shifts a chain's last word -- zero by the pack kernels' promise -- into every lag product of the word before
    it.  At the family's small size (N = 129) the word before it holds one draw, so there the zero word enters at lags
    from 64 on only, past the truncation of its chains; at 63, 64 and 128 draws it enters at lag 1.  Behind the family's
    large call, whose words fill the workspace these calls pack into, and against the definition on the host in bits."""
    from mcmc_ref_hip import indicator
    from test_indicator_gpu import agree, draws, quantile_requests
    family = F.BY_NAME["indicator_ess"]
    with fresh_context() as c:
        for C_ in (1, 2, 5):
            same(family.run(c, family.inputs("large")), wants[family.name, "large"], family.name, "large, before", (C_, N))
            x = draws(100 * N + C_, 3, C_, N, phi=0.9)
            lo, hi = quantile_requests(x)
            agree(indicator, c, x, lo, hi)
            agree(indicator, c, np.ascontiguousarray(x.transpose(1, 2, 0)), lo, hi, "cnp")


# ---- e. the cache of z tables --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["summarize", "diagnose_chains", "nested_rhat"])
def test_small_large_small_across_an_eviction_of_the_z_table(name, wants):
    family = F.BY_NAME[name]
    tiny = [np.random.default_rng(600 + n).normal(size=(1, 2, n)) for n in range(8, 33)]
    assert len({x.size for x in tiny}) == 25 > Z_TABLES and family.pooled("small") not in {x.size for x in tiny}
    with fresh_context() as c:
        def others():
            return [F.pack(c.summarize(x, "pcn", min_chains=2)) for x in tiny]
        same(family.run(c, family.inputs("small")), wants[name, "small"], name, "small, first")
        first = others()
        same(family.run(c, family.inputs("large")), wants[name, "large"], name, "large, behind 25 pooled lengths")
        assert others() == first
        same(family.run(c, family.inputs("small")), wants[name, "small"], name, "small, its z table evicted and rebuilt")


# ---- the count ---------------------------------------------------------------------------------------------------------

def test_all_ordered_pairs_ran():
    """Counted, not assumed: every (predecessor, successor) passed its second round exactly once.  (Run the whole file.)"""
    n = len(F.FAMILIES)
    assert n == 29 and len(PAIRS) == n * n == 841, (len(PAIRS), sorted(set((a, b) for a in F.NAMES for b in F.NAMES) - set(PAIRS))[:5])
    assert set(PAIRS.values()) == {1}
    assert len(_WANT) == 2 * n                                # and every baseline passed its family's reference gate
