"""What the two test files of the Stan-convention diagnostics (include/mcmcref_std.h) share: the case list, fixed at import,
and a numpy restatement of the definition written from the header's text -- FFT autocovariances, scipy's rankdata and
ndtri -- that knows nothing of the library's summation order.
"""
from __future__ import annotations

import functools
import math
import warnings

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

RTOL = 1e-9                      # the project's gate for a floating output against a restatement of the same definition
MARGIN_MIN = 1e-7                # a bulk walk decided closer to a tie than this would make the exact-lag comparison empty
DOUBLES = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "rhat_basic", "ess_mean", "mcse_mean")
LAGS = ("lag_bulk", "lag_q05", "lag_q95", "lag_mean")

NS = (8, 9, 16, 510, 512, 514, 1023, 1026, 2000)
CS = (1, 2, 3, 5)
KINDS = ("iid", "ar-0.5", "ar0.9", "ar0.99", "ties", "shifted")


def ar1(rng, C: int, N: int, phi: float) -> np.ndarray:
    """C stationary AR(1) chains of N draws with unit innovations."""
    e = rng.standard_normal((C, N))
    y = np.empty_like(e)
    y[:, 0] = e[:, 0] / math.sqrt(1.0 - phi * phi)
    for i in range(1, N):
        y[:, i] = phi * y[:, i - 1] + e[:, i]
    return y


def chains_of(kind: str, C: int, N: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "iid":
        return rng.standard_normal((C, N))
    if kind.startswith("ar"):
        return ar1(rng, C, N, float(kind[2:]))
    if kind == "ties":
        return np.round(rng.standard_normal((C, N)), 1)
    if kind == "shifted":                          # one chain shifted by 3: the walks run to n - 5
        y = ar1(rng, C, N, -0.5)
        y[C - 1] += 3.0
        return y
    raise ValueError(kind)


def _case_list() -> list:
    out, seed = [], 20240
    for N in NS:
        for C in CS:
            for kind in KINDS:
                seed += 1
                if kind == "shifted" and C == 1:   # the split halves of one shifted chain are not shifted against each other
                    continue
                out.append((kind, C, N, seed))
    return out


CASES = _case_list()                               # (kind, C, N, seed)


def shapes() -> list:
    """The (C, N) of the case list, each with its cases: one tensor [P][C][N] per shape."""
    seen: dict = {}
    for kind, C, N, seed in CASES:
        seen.setdefault((C, N), []).append((kind, seed))
    return [(C, N, tuple(v)) for (C, N), v in seen.items()]


@functools.lru_cache(maxsize=None)
def tensor_of(C: int, N: int, cases: tuple) -> np.ndarray:
    x = np.stack([chains_of(kind, C, N, seed) for kind, seed in cases])
    x.setflags(write=False)
    return x


# ---- the restatement ----------------------------------------------------------------------------------------------------

def split(x: np.ndarray) -> np.ndarray:
    """[C][N] -> the split chains [2 C][n]; the middle draw of an odd chain is dropped."""
    C, N = x.shape
    n = N // 2
    return np.concatenate([np.stack([x[c, :n], x[c, N - n:]]) for c in range(C)])


def blom(v: np.ndarray) -> np.ndarray:
    r = rankdata(v.reshape(-1), method="average").reshape(v.shape)
    return ndtri((r - 0.375) / (v.size + 0.25))


def rhat_of(v: np.ndarray) -> float:
    m, n = v.shape
    if v.min() == v.max():
        return math.nan
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # (n = 1 has no within-chain variance: NaN is the answer)
        means, var = v.mean(axis=1), v.var(axis=1, ddof=1)
        return float(np.sqrt((n * means.var(ddof=1) / var.mean() + n - 1) / n))


def walk_of(v: np.ndarray) -> dict:
    """ESS, max_t, margin, tau and the rho the walk stored, of a series [m][n]."""
    m, n = v.shape
    nan = {"ess": math.nan, "lag": -1, "margin": math.nan, "tau": math.nan, "rho": None}
    if n < 4 or v.min() == v.max():
        return nan
    d = v - v.mean(axis=1, keepdims=True)
    f = np.fft.rfft(d, 2 * n, axis=1)
    g = (np.fft.irfft(f * np.conj(f), 2 * n, axis=1)[:, :n] / n).mean(axis=0)
    mean_var = g[0] * n / (n - 1)
    var_plus = g[0] + (v.mean(axis=1).var(ddof=1) if m > 1 else 0.0)
    if not var_plus > 0:
        return nan
    rho_all = 1.0 - (mean_var - g) / var_plus
    rho = np.zeros(n + 2)
    rho[0], rho[1] = 1.0, rho_all[1]
    t, re, ro = 0, 1.0, rho_all[1]
    margin = abs(re + ro)
    while t < n - 5 and re + ro > 0:
        t += 2
        re, ro = rho_all[t], rho_all[t + 1]
        margin = min(margin, abs(re + ro))
        if re + ro >= 0:
            rho[t], rho[t + 1] = re, ro
    max_t = t
    if re > 0:
        rho[max_t] = re
    for t in range(2, max_t - 1, 2):
        if rho[t] + rho[t + 1] > rho[t - 2] + rho[t - 1]:
            rho[t] = rho[t + 1] = (rho[t - 2] + rho[t - 1]) / 2
    S = m * n
    tau = max(-1.0 + 2.0 * rho[:max_t].sum() + rho[max_t], 1.0 / math.log10(S))
    return {"ess": S / tau, "lag": max_t, "margin": margin, "tau": tau, "rho": rho_all, "g": g}


def restate(x: np.ndarray) -> dict:
    """Every output of the definition for the chains [C][N] of one parameter."""
    s = split(np.asarray(x, dtype=np.float64))
    zb, zf = blom(s), blom(np.abs(s - np.median(s)))
    q05, q95 = np.quantile(s, [0.05, 0.95])
    wb, w05, w95, wm = walk_of(zb), walk_of((s <= q05) * 1.0), walk_of((s <= q95) * 1.0), walk_of(s)
    rb, rt = rhat_of(zb), rhat_of(zf)
    return {"rhat": max(rb, rt), "rhat_bulk": rb, "rhat_tail": rt, "ess_bulk": wb["ess"], "lag_bulk": wb["lag"],
            "margin": wb["margin"], "ess_q05": w05["ess"], "lag_q05": w05["lag"], "ess_q95": w95["ess"], "lag_q95": w95["lag"],
            "ess_tail": math.nan if math.isnan(w05["ess"]) or math.isnan(w95["ess"]) else min(w05["ess"], w95["ess"]),
            "rhat_basic": rhat_of(s), "ess_mean": wm["ess"], "lag_mean": wm["lag"],
            "mcse_mean": float(s.std(ddof=1)) / math.sqrt(wm["ess"]) if not math.isnan(wm["ess"]) else math.nan}


def close(a: float, b: float, rtol: float = RTOL) -> bool:
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b or abs(a - b) <= rtol * max(abs(a), abs(b))


def same(got: dict, want: dict, where) -> None:
    """`got` (scalars) against `want` at RTOL, the lags exactly."""
    for k in DOUBLES:
        assert close(float(got[k]), float(want[k])), (where, k, got[k], want[k])
    for k in LAGS:
        assert int(got[k]) == int(want[k]), (where, k, got[k], want[k])


def at(r: dict, p: int) -> dict:
    return {k: v[p] for k, v in r.items()}


def bits(r: dict) -> dict:
    """The outputs as bytes: equality of bits, NaN included."""
    return {k: np.ascontiguousarray(v).tobytes() for k, v in r.items() if isinstance(v, (np.ndarray, np.generic, float, int))}
