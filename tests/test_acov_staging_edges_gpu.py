"""Chain lengths at every edge of the autocovariance kernels' staged windows.

Tiers 1 and 2 of the diagnostics stage a segment of one chain plus a halo in the LDS: 1024-draw segments on 128 threads for
chains of up to 1024 draws (windows of 1104 and 1296 draws), 2048-draw segments on 256 threads beyond (2128 and 2320).  A
lane loads the rank codes of its window slots unconditionally, and a slot beyond the chain's end reads the last draw the
window has instead; nothing such a slot loaded may reach a result.  The lengths below lie on either side of a segment end,
of the ends of the 64-lag and 80-draw halo and of the tier-2 halo, and one leaves a single draw for the last segment; the
columns reach tier 2 and tier 3 and include a chain whose compare-mask windows are all equal.  Checked against the CPU oracle
with the gates of test_hip_parity.py: integer outputs and order statistics exact, floating-point outputs to 1e-9.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_hip_parity import TIGHT, check_summary, close

pytestmark = pytest.mark.gpu

SHORT = [3, 4, 63, 64, 65, 127, 128, 129, 1023, 1024]
LONG = [1025, 2047, 2048, 2049, 2111, 2112, 2127, 2128, 2129, 2319, 2320, 2321, 4096, 4097, 6145]
CMAX = 4


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def ar1(rng, phi, C, N):
    e = rng.normal(size=(C, N))
    x = np.empty((C, N))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x


_draws: dict[int, np.ndarray] = {}


def draws(N: int) -> np.ndarray:
    """[5][CMAX][N], made once per N; a test with C chains takes the first C of every column."""
    if N not in _draws:
        rng = np.random.default_rng(7000 + N)
        x = np.empty((5, CMAX, N))
        x[0] = rng.normal(size=(CMAX, N))
        x[1] = ar1(rng, 0.9, CMAX, N)
        x[2] = ar1(rng, 0.99, CMAX, N)                                   # tier 2 and, for the longer N, tier 3
        x[3] = (rng.normal(size=(CMAX, N)) > 0.3).astype(np.float64)     # two values
        x[4] = rng.normal(size=(CMAX, N))
        x.setflags(write=False)
        _draws[N] = x
    return _draws[N]


def tensor(N: int, C: int) -> np.ndarray:
    x = draws(N)[:, :C].copy()
    x[4, C - 1] = 0.25                                                   # constant in one chain: every code equals the window's reference
    return x


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("N", SHORT + LONG)
def test_chain_lengths_at_the_window_edges(ctx, oracle, N, C):
    x = tensor(N, C)
    check_summary(ctx.summarize(x, "pcn", min_chains=1), oracle.summarize(x, "pcn", min_chains=1), what=f"N={N} C={C}")


# ragged chains (one parameter per call): the shortest chain sets n, a longer one sets the staged length through its second
# half, and another ends inside the halo of the window that holds its last segment
@pytest.mark.parametrize("lens", [(2049, 2100, 4200, 2127), (1000, 1023, 1010), (2320, 2330, 4097, 6145)])
@pytest.mark.parametrize("phi", [0.0, 0.99])
def test_ragged_chains_that_end_inside_a_halo(ctx, oracle, lens, phi):
    rng = np.random.default_rng(sum(lens))
    chains = [list(ar1(rng, phi, 1, n)[0]) for n in lens]
    got, exp = ctx.diagnose_chains(chains, 2), oracle.diag(chains, 2)
    for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
        assert close(got[k], exp[k], TIGHT), (lens, phi, k, got[k], exp[k])
    assert (got["lag_bulk"], got["lag_tail"]) == (exp["lag_bulk"], exp["lag_tail"]), (lens, phi)


def test_lone_call_forks_and_pipelined_calls_do_not_same_bits(ctx):
    """A lone call of 2 M param-draws or more runs the two kinds as two launches (kind_sel 0 / 1), pipelined calls as one."""
    C, N, P = 4, 6145, 85
    x = np.concatenate([tensor(N, C)] * (P // 5))
    x = x + np.arange(P).reshape(P, 1, 1)                                # distinct columns
    t = ctx.upload(x, "pcn")
    lone = ctx.summarize(t, min_chains=1)
    bufs = [ctx.enqueue(t, min_chains=1) for _ in range(8)]
    ctx.wait()
    t.free()
    assert (lone["lag_bulk"] > 63).any()                                 # tier 2 ran
    for q in bufs:
        r = q.result()
        for k in lone:
            assert np.array_equal(lone[k], r[k], equal_nan=True), k
