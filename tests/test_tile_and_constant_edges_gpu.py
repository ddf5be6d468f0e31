"""Full and partial sort tiles with heavy ties, and constant chains / half-chains that span several autocovariance segments.

The tile sort hands a lane the draws `i * 256 + tid` of its tile, so which of a tile's equal draws comes first is a property of
that hand-out; nothing after the sort may depend on it (equal draws share one average rank), and a full tile takes a path
without the per-draw pad tests.  Tier 1 of the autocovariance tells a constant chain (or half) by comparing every rank code of
a window with one reference code of that window -- the chain's first draw, or draw `n // 2` for the second half -- in every
2048-draw segment separately.  Both are checked here against the CPU oracle with the gates of test_hip_parity.py: integer
outputs and order statistics exact, floating-point outputs to 1e-9 (fp64 on both sides).

Every parameter keeps at least three ordinary chains, so the within-chain variance is far from zero and the comparison with the
oracle is well conditioned (all half-chains constant is the known discrepancy of test_strides_gpu.py, not the subject here).
"""
from __future__ import annotations

import numpy as np
import pytest

from test_hip_parity import check_summary

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


# pooled lengths C * N around the 4096-draw tile: one partial tile, exactly one / two / four full tiles, full tiles plus a
# partial one, a partial tile of a single draw, and the benchmark's 40 000
@pytest.mark.parametrize("C,N", [(4, 1000), (4, 1024), (4, 2048), (2, 2048), (4, 4096), (4, 2500), (1, 4097), (3, 4097),
                                  (4, 10000)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tied_draws_in_full_and_partial_tiles(ctx, oracle, C, N, dtype):
    rng = np.random.default_rng(1000 * C + N)
    P = 6
    x = rng.normal(size=(P, C, N))
    x[1] = np.round(x[1], 1)                          # ~60 distinct values: every tile is mostly ties
    x[2] = np.round(x[2] * 4.0) / 4.0
    x[3] = (x[3] > 0.3).astype(np.float64)            # two values
    x[4] = np.round(np.cumsum(x[4], axis=-1), 0)      # sticky and tied
    x[5, :, ::2] = 0.5                                # half the draws of every tile equal, at alternating positions
    x = (x + 0.0).astype(dtype)                       # (+ 0.0: no negative zeros, whose order among equals is unspecified)
    check_summary(ctx.summarize(x, "pcn", min_chains=1), oracle.summarize(x, "pcn", min_chains=1),
                  what=f"ties {C}x{N} {np.dtype(dtype).name}")


@pytest.mark.parametrize("N", [1000, 2048, 4999, 5000, 6145])     # one segment of 1024-draw workgroups ... four of 2048
def test_constant_chains_and_halves_across_segments(ctx, oracle, N):
    rng = np.random.default_rng(N)
    C, h = 4, N // 2
    cases = []

    def case(fill):
        x = rng.normal(size=(C, N))
        fill(x[1])
        cases.append(x)

    def const(c): c[:] = 0.25
    def last_differs(c): c[:] = 0.25; c[2 * h - 1] = 3.0            # the last draw the split keeps
    def first_differs(c): c[:] = 0.25; c[0] = 3.0                    # the reference draw of the chain and the first half
    def half_ref_differs(c): c[:] = 0.25; c[h] = 3.0                 # the reference draw of the second half
    def mid_segment_differs(c): c[:] = 0.25; c[min(N - 1, 2048 + 7)] = -1.0
    def first_half_const(c): c[:h] = 0.25
    def second_half_const(c): c[h:] = 0.25
    def two_levels(c): c[:h] = 0.25; c[h:] = 0.75                    # both halves constant, the chain is not
    def before_half_differs(c): c[:] = 0.25; c[h - 1] = 3.0          # last draw of the first half

    for f in (const, last_differs, first_differs, half_ref_differs, mid_segment_differs, first_half_const,
              second_half_const, two_levels, before_half_differs):
        case(f)
    x = np.stack(cases)                                               # [P][C][N]
    check_summary(ctx.summarize(x, "pcn"), oracle.summarize(x, "pcn"), what=f"constant windows N={N}")
