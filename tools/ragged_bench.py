#!/usr/bin/env python3
"""Host-clock times of the routes that take tables with rows out of order or chains of unequal length:

  read_draws_many     a shuffled 4 x 10 000 x 100 draws file -> resident [P][M] tensor in (chain, draw) order
  summarize_files     (general route: file image + params) a ragged 4-chain file of 10 000 / 9 000 / 9 500 / 10 000 draws
                      x 100 parameters -> statistics + diagnostics
  compute_diagnostics convert._compute_diagnostics on the same ragged table

After a warm-up every route is timed in `windows` windows of `reps` calls (each call ends synchronised: it returns host
results); per route the median window's ms per call and the range over the windows.  With a library that has them, the
HIP-event time of the layout kernels of one read_draws_many call.  Run it from a checkout of the parent commit to get
the other side of the comparison (`--root`), alternating the two.  Prints one JSON object."""
from __future__ import annotations

import argparse
import io
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    root = Path(a.root).resolve()
    sys.path[:0] = [str(root), str(root / "mcmc-db_amd")]
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip import _ffi, convert, parquet

    P = 100
    rng = np.random.default_rng(5)

    def table(counts, shuffle):
        M = int(sum(counts))
        cols = {"chain": np.repeat(np.arange(len(counts), dtype=np.int64), counts),
                "draw": np.concatenate([np.arange(n, dtype=np.int64) for n in counts])}
        for j in range(P):
            cols[f"p{j}"] = rng.normal(size=M)
        if shuffle:
            perm = rng.permutation(M)
            cols = {k: v[perm] for k, v in cols.items()}
        return pa.table(cols)

    def image(t):
        buf = io.BytesIO()
        pq.write_table(t, buf)
        return buf.getvalue()

    names = [f"p{j}" for j in range(P)]
    shuffled = image(table([10000] * 4, True))
    ragged_t = table([10000, 9000, 9500, 10000], False)
    ragged = image(ragged_t)
    ctx = _ffi.Context(0)

    def r_read():
        for d in parquet.read_draws_many(ctx, [shuffled], [names]):
            d.free()

    def r_files():
        return parquet.summarize_files(ctx, [ragged], [names])

    def r_diag():
        return convert._compute_diagnostics(ragged_t, names, context=ctx)

    out = {"tag": a.tag, "root": root.name, "windows": a.windows, "reps": a.reps, "routes": {}}
    for name, fn in (("read_draws_many", r_read), ("summarize_files", r_files), ("compute_diagnostics", r_diag)):
        fn()
        fn()
        per_call = []
        for _w in range(a.windows):
            t0 = time.perf_counter()
            for _r in range(a.reps):
                fn()
            per_call.append((time.perf_counter() - t0) * 1e3 / a.reps)
        out["routes"][name] = {"ms_per_call_median": statistics.median(per_call), "min": min(per_call), "max": max(per_call),
                               "windows_ms": per_call}
    ctx.profile(True)
    ctx.profile_reset()
    r_read()
    prof = ctx.profile_get()
    ctx.profile(False)
    out["read_draws_many_kernels_ms"] = {k: v["total_ms"] for k, v in prof.items()
                                         if k.startswith("k_layout") or k.startswith("k_pq") or k == "k_gather_rows"}
    chk = r_files()[0]["p0"]
    out["check_p0"] = {k: chk[k] for k in ("mean", "rhat", "ess_bulk", "ess_tail")}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
