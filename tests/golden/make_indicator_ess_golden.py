#!/usr/bin/env python3
"""Writes tests/golden/indicator_ess_cases.json: small 0/1 chains with what the reference's own ESS rule says of them.

    python tests/golden/make_indicator_ess_golden.py --reference /path/to/reference/src

The reference's `mcmc_ref.diagnostics` is IMPORTED (nothing of it is copied): per case the file records the chains as
strings of 0 and 1, `_ess` of them, and the first lag at which `_autocorr` is negative (n when there is none, 0 when
var_hat is 0 and the rule never looks at a lag).  Python integers compute A(lag) of include/mcmcref_iess.h next to it: a
case in which A == 0 at a lag up to the truncation is flagged, because there the sign the reference sees is the sign of
a rounding error.

Cases: 10 shapes (C 1-4, N 5-500) x AR(1) with phi in {0, 0.5 rounded to halves (ties), 0.9} x the indicator x <= q at
the pooled 5 / 50 / 95 % quantiles, and N in {2, 3, 63, 64, 65, 127, 128, 129} x C in {1, 2, 3, 5} at the median.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

SHAPES = [(1, 5), (1, 100), (1, 500), (2, 50), (2, 500), (3, 33), (3, 200), (4, 5), (4, 250), (4, 500)]
PHIS = (0.0, 0.5, 0.9)
PROBS = (0.05, 0.5, 0.95)
EDGE_N = (2, 3, 63, 64, 65, 127, 128, 129)
EDGE_C = (1, 2, 3, 5)


def ar1(rng, C: int, N: int, phi: float) -> np.ndarray:
    e = rng.normal(size=(C, N))
    y = e.copy()
    for t in range(1, N):
        y[:, t] = phi * y[:, t - 1] + e[:, t]
    return np.round(y * 2) / 2 if phi == 0.5 else y


def integer_a(bits: list[list[int]], lag: int) -> int:
    n, total = len(bits[0]), 0
    for b in bits:
        k = sum(b)
        S = sum(b[i] * b[i + lag] for i in range(n - lag))
        total += n * n * S - n * k * (sum(b[:n - lag]) + sum(b[lag:])) + (n - lag) * k * k
    return total


def case(diag, name: str, y: np.ndarray, prob: float, phi: float) -> dict:
    q = float(np.quantile(y, prob))
    bits = [[int(v <= q) for v in row] for row in y]
    chains = [[float(v) for v in row] for row in bits]
    m, n = len(chains), len(chains[0])
    ess = diag._ess(chains)
    means = [sum(c) / n for c in chains]
    mean_total = sum(means) / m
    var_between = n * sum((mu - mean_total) ** 2 for mu in means) / (m - 1) if m > 1 else 0.0
    var_hat = (n - 1) / n * sum(diag._variance(c) for c in chains) / m + var_between / n
    trunc = 0 if var_hat == 0 else next((lag for lag in range(1, n) if diag._autocorr(chains, lag, var_hat) < 0), n)
    flagged = var_hat != 0 and any(integer_a(bits, lag) == 0 for lag in range(1, min(trunc, n - 1) + 1))
    return {"name": name, "C": m, "N": n, "phi": phi, "prob": prob, "chains": ["".join(map(str, b)) for b in bits],
            "ess": ess, "trunc": trunc, "flagged": bool(flagged)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("MCMC_REF_SRC"), help="the reference's src directory")
    ap.add_argument("--out", type=Path, default=Path(__file__).with_name("indicator_ess_cases.json"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or MCMC_REF_SRC) is needed: the directory that holds the mcmc_ref package")
    sys.path.insert(0, args.reference)
    from mcmc_ref import diagnostics as diag

    rng = np.random.default_rng(20211)
    cases = []
    for C, N in SHAPES:
        for phi in PHIS:
            y = ar1(rng, C, N, phi)
            for prob in PROBS:
                cases.append(case(diag, f"c{C}_n{N}_phi{phi:g}_q{prob:g}", y, prob, phi))
    for i, N in enumerate(EDGE_N):
        for j, C in enumerate(EDGE_C):
            phi = PHIS[(i + j) % 3]
            cases.append(case(diag, f"edge_c{C}_n{N}_phi{phi:g}", ar1(rng, C, N, phi), 0.5, phi))
    args.out.write_text(json.dumps({"cases": cases}, indent=0) + "\n")
    print(f"{len(cases)} cases, {sum(c['flagged'] for c in cases)} flagged, {args.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
