"""Simulation-based calibration without a GPU: the host routines against numpy, scipy and exact references.

* mcr_sbc_ranks_host: the counts EQUAL numpy's; mean and sd within 1e-9 (the project's gate for its extensions: relative
  for sd, for the mean in units of max(sd, |mean|)) of long-double / math.fsum references, draws at 1e8 included; truth
  equal to a draw, to several tied draws, below and above all of them, +-0.0 against -+0.0; every refusal; L = 0.
* mcr_chi2_sf against scipy.stats.chi2.sf within 1e-9 relative wherever scipy's value is >= 1e-300.
* mcr_sbc_uniformity against a numpy restatement of its definition, with bins that divide n_draws + 1 and that do not.
* sbc() through a stub context that calls the host routine: the tie recipe, the default bins, p_min, prior_sd, z and
  contraction; a conjugate-normal model end to end (a correct sampler passes, a too narrow and a biased one fail, and the
  ranks equal numpy's); sbc_files on three small Parquet files; the command's options.
tests/test_sbc_gpu.py holds the device to mcr_sbc_ranks_host bit for bit.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import re
from pathlib import Path

import numpy as np
import pytest

GATE = 1e-9
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sbc_mod():
    from mcmc_ref_hip import sbc
    return sbc


class HostContext:
    """What sbc() needs of a Context, on the host routine: any layout, thinning, the same result dict."""

    def __init__(self, ffi):
        self.ffi = ffi

    def sbc_ranks(self, draws, truth, layout="spcn", thin=1):
        x = np.transpose(np.asarray(draws), [layout.index(a) for a in "spcn"])[:, :, :, ::thin]
        return self.ffi.sbc_ranks_host(np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], x.shape[1], -1), truth)


def edge_sample(S: int, P: int, L: int, seed: int = 0):
    """draws [S][P][L] and truth [S][P] with every edge of the comparison: parameter 0 continuous, 1 at 1e8, 2 on a grid
    (heavily tied, truth on the grid); then single rows: truth equal to one draw, below all, above all, +0.0 among -0.0
    draws and -0.0 among +0.0 draws."""
    rng = np.random.default_rng(77 + seed + 1000 * L)
    x = rng.standard_normal((S, P, L))
    t = rng.standard_normal((S, P))
    if P > 1:
        x[:, 1] += 1e8
        t[:, 1] += 1e8
    if P > 2:
        x[:, 2] = np.round(x[:, 2] * 2.0) / 2.0
        t[:, 2] = np.round(t[:, 2] * 2.0) / 2.0
    if L:
        flat_x, flat_t = x.reshape(S * P, L), t.reshape(S * P)
        rows = list(range(0, S * P, max(1, (S * P) // 5)))[:5]
        for kind, r in enumerate(rows):
            if kind == 0:
                flat_t[r] = flat_x[r, L // 2]
            elif kind == 1:
                flat_t[r] = flat_x[r].min() - 1.0
            elif kind == 2:
                flat_t[r] = flat_x[r].max() + 1.0
            elif kind == 3:
                flat_x[r, ::2] = -0.0
                flat_t[r] = 0.0
            else:
                flat_x[r, ::2] = 0.0
                flat_t[r] = -0.0
    return x, t


def check_against_references(res: dict, x: np.ndarray, t: np.ndarray):
    """Counts equal numpy's; mean and sd within GATE of long-double references (math.fsum for the mean)."""
    S, P, L = x.shape
    assert res["n_draws"] == L
    assert np.array_equal(res["n_less"], (x < t[..., None]).sum(-1)) and np.array_equal(res["n_equal"], (x == t[..., None]).sum(-1))
    if L == 0:
        assert np.isnan(res["mean"]).all() and np.isnan(res["sd"]).all()
        return
    for s in range(S):
        for p in range(P):
            mean = math.fsum(x[s, p]) / L
            d = x[s, p].astype(np.longdouble) - np.longdouble(mean)
            sd = float(np.sqrt((d * d).sum() / L))
            assert abs(res["mean"][s, p] - mean) <= GATE * max(sd, abs(mean)), (s, p)
            assert abs(res["sd"][s, p] - sd) <= GATE * sd, (s, p)


# ---- symbols and the header ---------------------------------------------------------------------------------------------------
def test_symbols_and_header(ffi):
    lib = ffi.load_library()
    header = (ROOT / "include" / "mcmcref_hip.h").read_text()
    for name in ("mcr_sbc_ranks", "mcr_sbc_ranks_dev", "mcr_sbc_plan", "mcr_sbc_ranks_host", "mcr_sbc_uniformity", "mcr_chi2_sf"):
        assert name in ffi.SYMBOLS and hasattr(lib, name) and re.search(rf"\b{name}\(", header), name
    body = re.search(r"typedef struct mcr_sbc_out \{(.*?)\} mcr_sbc_out;", header, re.S).group(1)
    fields = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in ffi.Sbc._fields_] == ["n_less", "n_equal", "mean", "sd"]
    assert int(re.search(r"#define MCR_WEIGHTED_BLOCK (\d+)", header).group(1)) == ffi.MCR_WEIGHTED_BLOCK == 1024
    assert int(re.search(r"#define MCR_VERSION\s+(\d+)", header).group(1)) == lib.mcr_version() == 100


# ---- mcr_sbc_ranks_host ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 5000])
def test_host_ranks_against_numpy(ffi, L):
    x, t = edge_sample(3, 4, L)
    check_against_references(ffi.sbc_ranks_host(x, t), x, t)


def test_host_ties_and_extremes(ffi):
    x = np.array([[[1.0, 2.0, 2.0, 2.0, 3.0, -0.0, 0.0, -0.0]]])
    for truth, less, equal in ((2.0, 4, 3), (1.0, 3, 1), (-5.0, 0, 0), (9.0, 8, 0), (0.0, 0, 3), (-0.0, 0, 3), (2.5, 7, 0)):
        r = ffi.sbc_ranks_host(x, [[truth]])
        assert (int(r["n_less"][0, 0]), int(r["n_equal"][0, 0])) == (less, equal), truth


def test_host_empty_shapes(ffi):
    r = ffi.sbc_ranks_host(np.empty((3, 2, 0)), np.zeros((3, 2)))
    assert r["n_draws"] == 0 and not r["n_less"].any() and not r["n_equal"].any()
    assert np.isnan(r["mean"]).all() and np.isnan(r["sd"]).all() and r["mean"].shape == (3, 2)
    assert ffi.sbc_ranks_host(np.empty((0, 2, 5)), np.empty((0, 2)))["n_less"].shape == (0, 2)
    assert ffi.sbc_ranks_host(np.empty((2, 0, 5)), np.empty((2, 0)))["mean"].shape == (2, 0)


def test_host_refusals(ffi):
    lib = ffi.load_library()
    x = np.arange(12.0).reshape(2, 2, 3)
    dp = ffi._as_dp

    def call(xp, S, P, L, tp, out=True):
        arrs, o = ffi._sbc_arrays(2, 2)
        rc = lib.mcr_sbc_ranks_host(xp, S, P, L, tp, C.byref(o) if out else None)
        return rc, arrs

    good = np.ones((2, 2))
    assert call(dp(x), 2, 2, 3, dp(good))[0] == ffi.MCR_OK
    for bad in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[1, 0] = bad
        rc, arrs = call(dp(x), 2, 2, 3, dp(t))
        assert rc == ffi.MCR_EINVAL
        assert (arrs["n_less"] == -1).all() and (arrs["n_equal"] == -1).all() and np.isnan(arrs["mean"]).all()     # untouched
    for S, P, L in ((-1, 2, 3), (2, -1, 3), (2, 2, -1), (1 << 31, 1, 3), (1 << 16, 1 << 15, 3), (2, 2, (1 << 31) - 1)):
        assert call(dp(x), S, P, L, dp(good))[0] == ffi.MCR_EINVAL, (S, P, L)
    assert call(dp(x), 2, 2, 3, dp(good), out=False)[0] == ffi.MCR_EINVAL
    assert call(None, 2, 2, 3, dp(good))[0] == ffi.MCR_EINVAL
    assert call(dp(x), 2, 2, 3, None)[0] == ffi.MCR_EINVAL
    with pytest.raises(ValueError):
        ffi.sbc_ranks_host(x, np.ones((2, 3)))
    with pytest.raises(ValueError):
        ffi.sbc_ranks_host(x[0], np.ones((2, 2)))


def test_host_nonfinite_draws_are_counted_and_the_rest_written(ffi):
    lib = ffi.load_library()
    x, t = edge_sample(2, 3, 50)
    bad = x.copy()
    bad[1, 0, 7], bad[0, 2, 3] = np.nan, np.inf
    arrs, o = ffi._sbc_arrays(2, 3)
    assert lib.mcr_sbc_ranks_host(ffi._as_dp(bad), 2, 3, 50, ffi._as_dp(t), C.byref(o)) == ffi.MCR_ENONFINITE
    ok = ffi.sbc_ranks_host(x, t)
    clean = np.ones((2, 3), dtype=bool)
    clean[1, 0] = clean[0, 2] = False
    for k in ("n_less", "n_equal", "mean", "sd"):
        assert np.array_equal(arrs[k][clean], ok[k][clean]), k
    assert np.isnan(arrs["mean"][1, 0]) and arrs["n_less"][1, 0] == (bad[1, 0] < t[1, 0]).sum()
    with pytest.raises(ffi.McrError) as e:
        ffi.sbc_ranks_host(bad, t)
    assert e.value.code == ffi.MCR_ENONFINITE


# ---- mcr_chi2_sf -----------------------------------------------------------------------------------------------------------------
def test_chi2_sf_against_scipy(ffi):
    from scipy import stats

    worst, seen = 0.0, 0
    for dof in (1, 2, 3, 15, 19, 99, 999):
        for x in (0.0, 1e-3, 0.5, dof, 3 * dof, 50 * dof):
            ref = float(stats.chi2.sf(x, dof))
            if ref < 1e-300:
                continue
            err = abs(ffi.chi2_sf(x, dof) - ref) / ref
            worst, seen = max(worst, err), seen + 1
            assert err <= GATE, (x, dof, ffi.chi2_sf(x, dof), ref)
    print(f"mcr_chi2_sf: worst relative error {worst:.3g} over {seen} points")
    assert seen >= 30


def test_chi2_sf_closed_form_and_edges(ffi):
    for x in (0.0, 1e-3, 0.5, 2.0, 6.0, 100.0, 1000.0):
        assert ffi.chi2_sf(x, 2) == pytest.approx(math.exp(-x / 2), rel=GATE)
    assert ffi.chi2_sf(0.0, 7) == 1.0 and ffi.chi2_sf(math.inf, 7) == 0.0
    for x, dof in ((-1.0, 3), (1.0, 0), (1.0, -2), (math.nan, 3)):
        assert math.isnan(ffi.chi2_sf(x, dof))
    assert all(ffi.chi2_sf(a, 9) > ffi.chi2_sf(b, 9) for a, b in ((1, 2), (9, 10), (10, 11), (11, 12), (40, 50)))   # both branches


# ---- mcr_sbc_uniformity ---------------------------------------------------------------------------------------------------------
def numpy_uniformity(ranks: np.ndarray, L: int, B: int) -> dict:
    """The definition in mcmcref_hip.h, restated."""
    from scipy import stats

    S, P = ranks.shape
    bin_of = np.arange(L + 1) * B // (L + 1)
    expected = S * np.bincount(bin_of, minlength=B) / (L + 1)
    counts = np.stack([np.bincount(bin_of[ranks[:, p]], minlength=B) for p in range(P)])
    chi2 = ((counts - expected) ** 2 / expected).sum(1)
    cum = np.stack([np.cumsum(np.bincount(ranks[:, p], minlength=L + 1)) for p in range(P)])
    dev = np.abs(cum * (L + 1) - (np.arange(L + 1) + 1) * S).max(1) / (S * (L + 1))
    return {"counts": counts, "expected": expected, "chi2": chi2, "pvalue": stats.chi2.sf(chi2, B - 1), "ecdf_dev": dev}


@pytest.mark.parametrize("L,B", [(99, 20), (99, 7), (100, 20), (6, 7), (1, 2), (1000, 13), (5, 2)])
def test_uniformity_against_numpy(ffi, L, B):
    rng = np.random.default_rng(L * 31 + B)
    ranks = np.stack([rng.integers(0, L + 1, 500), np.minimum(rng.integers(0, L + 1, 500), rng.integers(0, L + 1, 500)),
                      np.full(500, L), np.zeros(500, dtype=np.int64)], axis=1)
    got, ref = ffi.sbc_uniformity(ranks, L, B), numpy_uniformity(ranks, L, B)
    assert np.array_equal(got["counts"], ref["counts"]) and got["counts"].sum(1).tolist() == [500] * 4
    assert np.allclose(got["expected"], ref["expected"], rtol=1e-15, atol=0) and got["expected"].sum() == pytest.approx(500, rel=1e-14)
    assert np.allclose(got["chi2"], ref["chi2"], rtol=1e-12, atol=0)
    assert np.allclose(got["ecdf_dev"], ref["ecdf_dev"], rtol=1e-15, atol=0)
    for a, b in zip(got["pvalue"], ref["pvalue"]):
        assert a == pytest.approx(b, rel=GATE) if b >= 1e-300 else a < 1e-299


@pytest.mark.parametrize("L,B", [(99, 20), (9, 10), (11, 4)])
def test_uniform_ranks_are_exactly_uniform(ffi, L, B):
    S = 3 * (L + 1)
    ranks = np.stack([np.arange(S) % (L + 1), (np.arange(S)[::-1] * 7) % (L + 1)], axis=1)
    got = ffi.sbc_uniformity(ranks, L, B)
    assert (got["chi2"] == 0.0).all() and (got["pvalue"] == 1.0).all() and (got["ecdf_dev"] == 0.0).all()


def test_uniformity_refusals(ffi):
    ranks = np.array([[0, 1], [2, 3]])
    assert ffi.sbc_uniformity(ranks, 3, 2)["counts"].tolist() == [[1, 1], [1, 1]]
    for L, B in ((3, 1), (3, 5), (3, 0), (2, 2), (-1, 2)):                # (L = 2: the rank 3 is out of range)
        with pytest.raises(ValueError):
            ffi.sbc_uniformity(ranks, L, B)
    with pytest.raises(ValueError):
        ffi.sbc_uniformity(np.array([[0, -1]]), 3, 2)
    with pytest.raises(ValueError):
        ffi.sbc_uniformity(np.empty((0, 2), dtype=np.int64), 3, 2)
    with pytest.raises(ValueError):
        ffi.sbc_uniformity(np.arange(4), 3, 2)


# ---- sbc() -------------------------------------------------------------------------------------------------------------------------
def test_default_bins(sbc_mod):
    assert [sbc_mod.default_bins(L) for L in (99, 100, 6, 11, 1, 399, 3999, 1000, 18)] == [20, 20, 7, 12, 2, 20, 20, 13, 19]


def test_sbc_ties_layouts_and_scores(ffi, sbc_mod):
    rng = np.random.default_rng(5)
    S, Cn, N, P = 40, 2, 30, 3
    x = np.round(rng.standard_normal((S, P, Cn, N)) * 2.0) / 2.0           # a grid: ties with the truth everywhere
    t = np.round(rng.standard_normal((S, P)) * 2.0) / 2.0
    ctx = HostContext(ffi)
    r = sbc_mod.sbc(x, t, context=ctx, seed=9, names=("a", "b", "c"))
    n_less, n_equal = (x.reshape(S, P, -1) < t[..., None]).sum(-1), (x.reshape(S, P, -1) == t[..., None]).sum(-1)
    u = np.random.default_rng(9).integers(0, n_equal + 1)
    assert np.array_equal(r.ranks, n_less + np.where(n_equal > 0, u, 0)) and r.n_tied == (n_equal > 0).sum() > S
    assert r.n_draws == 60 and r.bins == sbc_mod.default_bins(60) == 20 and r.dof == 19
    assert r.passed and r.failures == () and r.names == ("a", "b", "c")
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.bins = 3
    mean, sd = x.reshape(S, P, -1).mean(-1), x.reshape(S, P, -1).std(-1)
    assert np.allclose(r.z_score, (mean - t) / sd, rtol=1e-12, atol=1e-12)
    assert np.allclose(r.contraction, 1 - sd ** 2 / t.var(0), rtol=1e-12, atol=1e-12)
    r2 = sbc_mod.sbc(x, t, context=ctx, seed=9, prior_sd=[1.0, 2.0, 0.5], bins=5)
    assert np.allclose(r2.contraction, 1 - sd ** 2 / np.array([1.0, 4.0, 0.25]), rtol=1e-12, atol=1e-12) and r2.bins == 5
    assert r2.counts.shape == (P, 5) and r2.expected.shape == (5,) and r2.names == ("p0", "p1", "p2")
    # any layout and thinning are the same call on the same draws
    for layout in ("scnp", "cspn", "pscn"):
        y = np.ascontiguousarray(np.transpose(x, ["spcn".index(a) for a in layout]))
        assert np.array_equal(sbc_mod.sbc(y, t, layout=layout, context=ctx, seed=9).ranks, r.ranks), layout
    thin = sbc_mod.sbc(x, t, context=ctx, thin=4)
    assert thin.n_draws == 2 * 8 and np.array_equal(thin.ranks, sbc_mod.sbc(x[..., ::4], t, context=ctx).ranks)
    with pytest.raises(ValueError):
        sbc_mod.sbc(x, t, context=ctx, names=("a",))


def conjugate_normal(scale: float = 1.0, shift: float = 0.0, S: int = 1000, P: int = 4, L: int = 99, n: int = 10):
    """y_1..n ~ N(theta, 1), theta ~ N(0, 1): the posterior is N(ybar n / (n + 1), 1 / (n + 1)); `scale` and `shift` (in
    posterior sds) make the sampler wrong.  truth [S][P], draws [S][P][L]."""
    rng = np.random.default_rng(4711)
    theta = rng.standard_normal((S, P))
    ybar = theta + rng.standard_normal((S, P)) / np.sqrt(n)
    x = ybar[..., None] * n / (n + 1) + shift / np.sqrt(n + 1) + scale * rng.standard_normal((S, P, L)) / np.sqrt(n + 1)
    return theta, x


def check_conjugate(sbc_mod, context, layout_of=lambda x: (x[:, :, None, :], "spcn")):
    """The three assertions of the conjugate-normal model, on whatever context ranks the draws."""
    from scipy import stats

    out = {}
    for name, kw in (("correct", {}), ("narrow", {"scale": 0.8}), ("biased", {"shift": 0.3})):
        theta, x = conjugate_normal(**kw)
        draws, layout = layout_of(x)
        r = sbc_mod.sbc(draws, theta, layout=layout, bins=20, p_min=1e-3, context=context)
        ranks = (x < theta[..., None]).sum(-1)                               # numpy's side of the recipe
        assert np.array_equal(r.ranks, ranks) and r.n_tied == 0, name
        counts = np.stack([np.bincount(ranks[:, p] * 20 // 100, minlength=20) for p in range(4)])
        p_numpy = stats.chi2.sf(((counts - 50.0) ** 2 / 50.0).sum(1), 19)
        assert np.allclose(r.pvalue, p_numpy, rtol=1e-9, atol=1e-300), name
        print(f"conjugate normal, {name}: p = {r.pvalue}")
        out[name] = r
    assert out["correct"].pvalue.min() > 1e-3 and out["correct"].passed and out["correct"].failures == ()
    assert out["narrow"].pvalue.max() < 1e-6 and out["biased"].pvalue.max() < 1e-6
    for name in ("narrow", "biased"):
        r = out[name]
        assert not r.passed and len(r.failures) == 4
        assert r.failures[0] == f"p0.sbc_p={r.pvalue[0]:.3g} < 0.001"
    assert abs(np.mean(out["biased"].z_score)) > 0.2 > abs(np.mean(out["correct"].z_score))
    assert np.allclose(out["correct"].contraction.mean(0), 1 - (1 / 11) / 1.0, atol=0.1)
    return out


def test_conjugate_normal_end_to_end(ffi, sbc_mod):
    check_conjugate(sbc_mod, HostContext(ffi))


# ---- files and the command ------------------------------------------------------------------------------------------------------
def write_simulations(tmp_path, S: int = 3, M: int = 24):
    import pyarrow as pa
    import pyarrow.parquet as pq

    rng = np.random.default_rng(3)
    x = rng.standard_normal((S, 2, M))
    truth = rng.standard_normal((S, 2))
    paths = []
    for s in range(S):
        path = tmp_path / f"sim{s}.parquet"
        pq.write_table(pa.table({"chain": np.repeat(np.arange(2), M // 2), "draw": np.tile(np.arange(M // 2), 2),
                                 "mu": x[s, 0], "tau": x[s, 1]}), path)
        paths.append(path)
    table = tmp_path / "truth.csv"
    table.write_text("sim,tau,mu\n" + "".join(f"s{s},{float(truth[s, 1])!r},{float(truth[s, 0])!r}\n" for s in range(S)))
    return paths, table, x, truth


def host_file_ranks(ctx, paths, params, truth_of, thin):
    """sbc._file_ranks without a device: pyarrow decodes, the stub ranks."""
    import pyarrow.parquet as pq

    tabs = [pq.read_table(p) for p in paths]
    names = params or [n for n in tabs[0].column_names if n not in ("chain", "draw")]
    x = np.stack([np.stack([t.column(n).to_numpy() for n in names]) for t in tabs])
    truth = truth_of(names, len(paths))
    return names, truth, ctx.sbc_ranks(x[:, :, None, :], truth, "spcn", thin)


def test_sbc_files_through_the_stub(ffi, sbc_mod, tmp_path, monkeypatch):
    paths, table, x, truth = write_simulations(tmp_path)
    monkeypatch.setattr(sbc_mod, "_file_ranks", host_file_ranks)          # (the device reader runs in tests/test_sbc_gpu.py)
    r = sbc_mod.sbc_files(paths, table, context=HostContext(ffi), bins=5)
    assert r.names == ("mu", "tau") and r.n_draws == 24 and r.ranks.shape == (3, 2)
    assert np.array_equal(r.ranks, (x < truth[..., None]).sum(-1))
    by_name = sbc_mod.sbc_files(paths, {"mu": truth[:, 0], "tau": truth[:, 1], "other": [1, 2, 3]}, params=["tau"],
                                context=HostContext(ffi), bins=5, thin=2)
    assert by_name.names == ("tau",) and np.array_equal(by_name.ranks[:, 0], (x[:, 1, ::2] < truth[:, 1, None]).sum(-1))
    with pytest.raises(KeyError):
        sbc_mod.sbc_files(paths, {"mu": truth[:, 0]}, context=HostContext(ffi))
    with pytest.raises(ValueError):
        sbc_mod.sbc_files(paths, {"mu": [1.0], "tau": [1.0]}, context=HostContext(ffi))
    with pytest.raises(ValueError):
        sbc_mod.sbc_files([], table)


def test_command_options():
    from mcmc_ref_hip import cli

    cmd = cli.main.commands["sbc"]
    opts = {o for p in cmd.params for o in p.opts}
    assert {"--truth", "--thin", "--bins", "--p-min", "--params", "--format"} <= opts
    files = next(p for p in cmd.params if p.name == "files")
    assert files.nargs == -1 and files.required
    assert next(p for p in cmd.params if p.name == "truth").required
