"""Inputs shared by the lag-edge tests (test_lag_edges_cpu.py, test_lag_edges_gpu.py) and their generator
(golden/make_lag_edge_fixture.py): draws whose first negative rho sits at a chosen lag F, rebuilt from a recipe
(C, N, T, seed, amp) to the same bits on every machine.  No GPU, no library: numpy only, and of numpy only integer
arithmetic and the exactly rounded float64 operations (int -> float conversion, +, -, *, /): no libm, no numpy.random.

A chain is a triangle wave of integer period T and of an integer phase hashed from (seed, c), plus amp times a noise
term in [-1, 1) hashed from (seed, c, t) with the splitmix64 finaliser.  Rank-normalised, the wave's autocorrelation
crosses zero near T / 4 (and that of the folded draws near T / 8); the noise removes the ties and gives rho a finite slope
through zero, so the decision lies far outside the +-1e-10 guard band and is the tiers' own.

The hand-over lags below are the kernels' documented constants (mcr_diag.hpp: kLag1, kMoreBlocks, kLag2, kLongGroup,
t3_stage_first; mcr_api.hip: launch_diag's rounds); TABLE is the coverage the fixture must have.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "lag_edge_cases.json"

TIER2 = (64, 128, 192)          # first lags of tier 2's three 64-lag blocks
TIER3 = 256                     # first lag of tier 3
STAGES = (768, 2304, 4352)      # first lags of k_tier3's stages two to four (256 + 256 * (2, 8, 16) groups); 512 is a group seam
ROUND_END = 16384               # end of the first direct round of the listed route
RHO_FLOOR = 1e-6                # |rho| at F and F - 1 of every recipe: four decades outside the guard band


def around(*lags):
    return tuple(f for l in lags for f in (l - 1, l, l + 1))


# route: (chain lengths allowed, chain counts, F)
TABLE = {
    "short": ((600, 1024), (2, 4), around(*TIER2, TIER3)),                    # 128-thread k_acov_seg, one tier-3 stage
    "segments": ((4097, 6200), (2, 3), around(*TIER2, TIER3, 512, 768)),      # 2048-draw segments, several per chain
    "one_stage": ((2100, 2304), (2,), around(512, 768)),                      # k_tier3 with at most 8 groups
    "multi_stage": ((12000, 16384), (2,), around(*STAGES)),                   # k_tier3, stage after stage
    "long": ((16385, 17000), (2,), around(TIER3, 512)),                       # FFT / direct rounds
    "long_round_end": ((16385, 1 << 20), (2,), around(ROUND_END)),            # the first direct round's last and next lag
}

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _mix(z: np.ndarray) -> np.ndarray:
    """The splitmix64 finaliser on a uint64 array (the products wrap)."""
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def _chain_key(seed: int, c: int) -> np.ndarray:
    return _mix(np.array([seed], dtype=np.uint64) * _GOLDEN + np.array([c + 1], dtype=np.uint64))


def phase(seed: int, c: int, T: int) -> int:
    """floor(T u), u in [0, 1) the top 32 bits of the chain's key over 2^32: the phase moves with T instead of jumping."""
    return ((int(_chain_key(seed, c)[0]) >> 32) * T) >> 32


def noise(seed: int, c: int, N: int) -> np.ndarray:
    """N values in [-1, 1): the top 53 bits of a hash of (seed, c, t), over 2^52, minus one -- all exact."""
    t = np.arange(1, N + 1, dtype=np.uint64)
    h = _mix(_chain_key(seed, c) + t * _GOLDEN)
    return (h >> np.uint64(11)).astype(np.float64) / 4503599627370496.0 - 1.0


def triangle(N: int, T: int, ph: int) -> np.ndarray:
    """(2 |2u - T| - T) / T for u = (t + ph) mod T: an integer over T, one rounding."""
    u = (np.arange(N, dtype=np.int64) + ph) % T
    return (2 * np.abs(2 * u - T) - T).astype(np.float64) / float(T)


def build(C: int, N: int, T: int, seed: int, amp: float) -> np.ndarray:
    """[C][N] float64 draws of a recipe."""
    x = np.empty((C, N), dtype=np.float64)
    for c in range(C):
        x[c] = triangle(N, T, phase(seed, c, T)) + amp * noise(seed, c, N)
    return x


def sha256(x: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(x, dtype="<f8").tobytes()).hexdigest()


def load() -> list[dict]:
    return json.loads(FIXTURE.read_text())["cases"]


def draws_of(case: dict) -> np.ndarray:
    return build(case["C"], case["N"], case["T"], case["seed"], case["amp"])


def groups(cases) -> dict:
    """(route, C, N) -> its cases in file order: one tensor [P][C][N] per key."""
    out: dict = {}
    for c in cases:
        out.setdefault((c["route"], c["C"], c["N"]), []).append(c)
    return out


def tensor(cases) -> np.ndarray:
    x = np.stack([draws_of(c) for c in cases])
    x.setflags(write=False)
    return x


def rho(z: np.ndarray, lags) -> np.ndarray:
    """rho at `lags` of z[C][n] the way the reference's `_ess` / `_autocorr` define it: per chain the lagged products of
    the deviations from the chain's mean over n - lag, summed over the chains, over C var_hat."""
    C, n = z.shape
    mu = z.mean(axis=1, keepdims=True)
    W = np.mean(z.var(axis=1, ddof=1))
    B = n * np.sum((mu[:, 0] - mu.mean()) ** 2) / (C - 1) if C > 1 else 0.0
    vhat = (n - 1) / n * W + B / n
    d = z - mu
    return np.array([np.sum(d[:, :n - l] * d[:, l:]) / (n - l) for l in lags]) / (C * vhat)
