#!/usr/bin/env python3
"""Recipes for draws whose first negative rho of the bulk ESS sits at a chosen lag F: one per (route, C, F) of
tests/lag_edge_cases.py's TABLE, the lags at which one kernel of the ESS relay hands the walk to the next.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_lag_edge_fixture.py      (CPU only, a few minutes)
    ... make_lag_edge_fixture.py long_round_end multi_stage      (a dry run of the named routes: prints, writes nothing)

For each target the period T of `lag_edge_cases.build` is searched: a feedback step T <- T F / F(T) from T = 4 F, a
bisection between the nearest misses, then a scan of T +- 30, seed after seed, with the first negative lag taken from
FFT autocovariances (oracle/numpy_path.py, quick); a hit is then confirmed with the C oracle (`oracle.summarize(...)["lag_bulk"] + 1 == F`) and rejected when
|rho| at F or F - 1, computed from the oracle's z, is below 1e-6.  N is fixed per route; a target that no (T, seed)
reaches at amplitude 0.5 is tried at 0.25 and 0.125 (less noise: rho's lag-to-lag jitter shrinks against the wave's slope,
so F follows T more smoothly -- it matters near lag 16 384, where the slope is 1e-4 per lag), then at the route's further N
(ROUTE_N), and the fixture records what it took.  Emits lag_edge_cases.json: recipes only -- {route, C, N, T, seed, amp, F, lag_tail,
sha256 of the draws' bytes} -- the draws are rebuilt by the tests.
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.dont_write_bytecode = True
sys.path[:0] = [str(HERE.parents[1]), str(HERE.parent)]

import lag_edge_cases as lec  # noqa: E402
from oracle import numpy_path, oracle as orc  # noqa: E402

# chain lengths tried in turn, the first one first for every target: off the segment and group sizes, inside TABLE's ranges
ROUTE_N = {
    "short": (1021, 1000, 900),
    "segments": (6151, 6200, 5000),
    "one_stage": (2297, 2304, 2200),
    "multi_stage": (16001, 16384, 15000, 15500),
    "long": (16411, 16900),
    "long_round_end": (56003, 57000, 58000, 60000),
}
AMPS = (0.5, 0.25, 0.125)
SEEDS = 24
SCAN = 30


def first_negative(x: np.ndarray) -> int:
    """F of draws [C][N], by FFT."""
    z = numpy_path._rank_z(x.reshape(-1)).reshape(x.shape)
    return numpy_path._ess(z)[1] + 1


def confirm(C, N, T, seed, amp, F):
    """The recipe's fixture entry if the oracle puts the first negative rho at F with |rho| >= 1e-6 on either side."""
    x = lec.build(C, N, T, seed, amp)
    o = orc.summarize(x[None], "pcn", min_chains=1)
    if int(o["lag_bulk"][0]) + 1 != F:
        return None
    z = np.stack(orc.rank_normalize(list(x))[0])
    r = lec.rho(z, (F - 1, F))
    if not (r[0] >= lec.RHO_FLOOR and r[1] <= -lec.RHO_FLOOR):
        return None
    return dict(C=C, N=N, T=T, seed=seed, amp=amp, F=F, lag_tail=int(o["lag_tail"][0]), rho_before=float(r[0]),
                rho_at=float(r[1]), sha256=lec.sha256(x))


def search(C, N, F, amp):
    for seed in range(1, SEEDS + 1):
        seen = {}

        def f(T):
            if T not in seen:
                seen[T] = first_negative(lec.build(C, N, T, seed, amp))
            return seen[T]

        T = 4 * F
        for _ in range(12):                                   # the crude feedback step
            got = f(T)
            nxt = max(8, int(round(T * F / got)))
            if got == F or nxt in seen:
                break
            T = nxt
        for _ in range(24):                                   # bisect between the nearest miss on either side
            below = [t for t in seen if seen[t] < F]
            above = [t for t in seen if seen[t] > F]
            if F in seen.values() or not below or not above:
                break
            mid = (max(below, key=lambda t: (seen[t], t)) + min(above, key=lambda t: (seen[t], t))) // 2
            if mid in seen:
                break
            f(mid)
        best = min(seen, key=lambda t: (abs(seen[t] - F), t))
        for d in sorted(range(-SCAN, SCAN + 1), key=abs):
            Tc = best + d
            if Tc >= 8 and f(Tc) == F:
                rec = confirm(C, N, Tc, seed, amp, F)
                if rec is not None:
                    return rec
    return None


def main() -> None:
    orc.build()
    cases, notes = [], []
    only = sys.argv[1:]                                      # route names: a dry run of those routes, nothing written
    for route, (nrange, chain_counts, targets) in lec.TABLE.items():
        if only and route not in only:
            continue
        for C in chain_counts:
            for F in targets:
                t0 = time.perf_counter()
                rec = None
                for N, amp in [(N, a) for N in ROUTE_N[route] for a in AMPS]:      # a smaller amplitude before another N
                    assert nrange[0] <= N <= nrange[1]
                    rec = search(C, N, F, amp)
                    if rec is not None:
                        break
                if rec is None:
                    raise SystemExit(f"no recipe for {route} C={C} F={F}: widen ROUTE_N / AMPS / SEEDS")
                if (rec["N"], rec["amp"]) != (ROUTE_N[route][0], AMPS[0]):
                    notes.append(f"{route} C={C} F={F}: N={rec['N']} amp={rec['amp']}")
                print(f"{time.perf_counter() - t0:6.1f} s", route, rec, flush=True)
                rec.pop("rho_before"), rec.pop("rho_at")
                cases.append(dict(route=route, **rec))
    if only:
        return
    doc = {"_about": "recipes of tests/lag_edge_cases.py, written by make_lag_edge_fixture.py", "not_first_choice": notes,
           "cases": cases}
    (HERE / "lag_edge_cases.json").write_text(json.dumps(doc, indent=1) + "\n")
    print("not at the first N / amplitude:", notes or "none")


if __name__ == "__main__":
    main()
