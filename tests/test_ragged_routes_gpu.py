"""The Python routes that take tables with chains of unequal length or rows out of order, end to end:
`parquet.summarize_files` (general route) and `convert.convert_files`.  A ragged model is ONE kernel pipeline for all
its parameters -- the tile sort is launched as often for six parameters as for two -- and its numbers are Backend.stats
on the pooled draws plus the oracle's diagnostics per parameter."""
from __future__ import annotations

import io
import math

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import ragged_cases
from conftest import rel_close

pytestmark = pytest.mark.gpu

TOL = 1e-9
QS = (0.05, 0.5, 0.95)
COUNTS = np.array([40, 30, 35, 40], dtype=np.int64)


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip._ffi import Context
    c = Context(0)
    yield c
    c.close()


def ragged_table(P: int, seed: int, shuffle: bool = False, inf_at=None):
    rng = np.random.default_rng(seed)
    M = int(COUNTS.sum())
    chain = np.repeat(np.arange(len(COUNTS), dtype=np.int64), COUNTS)
    draw = np.concatenate([np.arange(n, dtype=np.int64) for n in COUNTS])
    cols = {"chain": chain, "draw": draw}
    for j in range(P):
        cols[f"p{j}"] = rng.normal(size=M) + 0.1 * j
    if inf_at is not None:
        cols["p0"][inf_at] = np.inf
    if shuffle:
        perm = rng.permutation(M)
        cols = {k: v[perm] for k, v in cols.items()}
    return pa.table(cols)


def image(table) -> bytes:
    buf = io.BytesIO()
    pq.write_table(table, buf)
    return buf.getvalue()


def expected_entries(oracle, table, params, min_chains=4):
    """{param: Backend.stats + diagnostics} from the oracle, on the table put into (chain, draw) order."""
    order = np.lexsort((table["draw"].to_numpy(), table["chain"].to_numpy()))
    counts = np.unique(table["chain"].to_numpy(), return_counts=True)[1]
    out = {}
    for p in params:
        row = table[p].to_numpy()[order]
        s = oracle.stats(row, QS)
        d = oracle.diag(ragged_cases.chains_of(row, counts), min_chains)
        out[p] = {**{k: v for k, v in s.items() if not k.startswith("_")},
                  "rhat": d["rhat"], "ess_bulk": d["ess_bulk"], "ess_tail": d["ess_tail"]}
    return out


def assert_entries(got: dict, exp: dict):
    assert list(got) == list(exp)
    for p in exp:
        assert got[p].keys() == exp[p].keys(), p
        for k in exp[p]:
            assert rel_close(float(got[p][k]), float(exp[p][k]), TOL), (p, k, got[p][k], exp[p][k])


def test_summarize_files_sorts_a_ragged_model_once(ctx, oracle):
    from mcmc_ref_hip.parquet import summarize_files
    launches = {}
    for P in (2, 6):
        t = ragged_table(P, seed=P, shuffle=(P == 6))
        params = [f"p{j}" for j in range(P)]
        ctx.profile(True)
        ctx.profile_reset()
        try:
            got = summarize_files(ctx, [image(t)], [params], min_chains=4, quantiles=QS)
            prof = ctx.profile_get()
        finally:
            ctx.profile(False)
        launches[P] = prof["k_tile_sort"]["launches"]
        assert_entries(got[0], expected_entries(oracle, t, params))
    assert launches[2] == launches[6] == 1, launches         # one pipeline per model, however many parameters


def test_summarize_files_mixes_ragged_and_rectangular_models(ctx, oracle):
    from mcmc_ref_hip.parquet import summarize_files
    rng = np.random.default_rng(9)
    rect = pa.table({"chain": np.repeat(np.arange(4), 50), "draw": np.tile(np.arange(50), 4), "a": rng.normal(size=200)})
    ragged = ragged_table(3, seed=21)
    got = summarize_files(ctx, [image(rect), image(ragged), image(rect)], [["a"], ["p0", "p1", "p2"], ["a"]], quantiles=QS)
    assert_entries(got[0], expected_entries(oracle, rect, ["a"]))
    assert_entries(got[1], expected_entries(oracle, ragged, ["p0", "p1", "p2"]))
    assert got[2] == got[0]
    stats_only = summarize_files(ctx, [image(ragged)], [["p1"]], quantiles=QS, diagnostics=False)
    assert list(stats_only[0]["p1"]) == ["mean", "std", "q5", "q50", "q95"]
    assert rel_close(stats_only[0]["p1"]["mean"], got[1]["p1"]["mean"], TOL)


def write_csv(path, table):
    names = table.column_names
    cols = [table[n].to_numpy() for n in names]
    with open(path, "w") as fh:
        fh.write(",".join(names) + "\n")
        for i in range(table.num_rows):
            fh.write(",".join(repr(int(c[i])) if c.dtype.kind == "i" else repr(float(c[i])) for c in cols) + "\n")


def test_convert_files_mixes_rectangular_ragged_and_shuffled_inputs(ctx, oracle, tmp_path):
    from mcmc_ref_hip.convert import ConvertResult, convert_file, convert_files
    rng = np.random.default_rng(31)
    rect = pa.table({"chain": np.repeat(np.arange(4), 60), "draw": np.tile(np.arange(60), 4),
                     "a": rng.normal(size=240), "b": rng.normal(size=240)})
    tables = {"rect": rect, "ragged": ragged_table(3, seed=41), "inf": ragged_table(2, seed=42, inf_at=17),
              "shuffled": ragged_table(4, seed=43, shuffle=True), "rect2": rect}
    jobs = []
    for name, t in tables.items():
        write_csv(tmp_path / f"{name}.csv", t)
        jobs.append((tmp_path / f"{name}.csv", name))
    (tmp_path / "d").mkdir()
    (tmp_path / "m").mkdir()
    res = convert_files(jobs, tmp_path / "d", tmp_path / "m", force=True, context=ctx)
    assert [isinstance(r, ConvertResult) for r in res] == [True, True, False, True, True]
    assert isinstance(res[2], ValueError) and "non-finite" in str(res[2])            # the model with a non-finite draw fails alone
    (tmp_path / "d1").mkdir()
    (tmp_path / "m1").mkdir()
    for (path, name), r in zip(jobs, res):
        if name == "inf":
            with pytest.raises(ValueError):
                convert_file(path, name, tmp_path / "d1", tmp_path / "m1", force=True)
            continue
        one = convert_file(path, name, tmp_path / "d1", tmp_path / "m1", force=True)
        assert r.meta["diagnostics"] == one.meta["diagnostics"], name
        assert r.meta["n_chains"] == 4 and r.meta["n_draws_per_chain"] == (60 if name.startswith("rect") else 30)
        t = tables[name]
        params = [c for c in t.column_names if c not in ("chain", "draw")]
        exp = expected_entries(oracle, t, params, min_chains=1)
        for p in params:
            for k in ("rhat", "ess_bulk", "ess_tail"):
                g, e = r.meta["diagnostics"][p][k], exp[p][k]
                assert rel_close(float(g), float(e), TOL) or (math.isnan(g) and math.isnan(e)), (name, p, k, g, e)
