"""The rank-ECDF test of include/mcmcref_recdf.h without a GPU: the pointwise table against exact rationals, the host
routine mce_rank_ecdf_host against a numpy restatement (sort, `<=`, sum) in bits, the null sample against a numpy
restatement of the hash recipe in bits, the test's rejection rates on fixed seeds, the mirror `_eabi` against the header
and the exports of libmcmcref_recdf.so, and the command.  The other four libraries export what they exported before.

Table: relative error <= 1e-9, the project's float gate, for every entry whose exact value is >= 1e-300.  Worst measured:
2.4e-16 at (24, 6, 4), 5.4e-16 at (60, 15, 7), 8.7e-16 at (400, 100, 16); 7.1e-15 against scipy.stats.hypergeom at
(4000, 1000, 100).

Rates (fixed seeds, host path, C = 4, n = 250, K = 32, S = 2000, alpha = 0.05), measured: iid 7.25 % rejected; chain 2
shifted by 0.3: 87.5 % rejected, chain == 2 in 94 %; chain 1 scaled by 1.5: 99.75 %; AR(0.9) unthinned 97 %; AR(0.9) at
thin=20 7.5 %.  The bounds are those of a numpy/scipy prototype of the definition with margins of at least 3 binomial
standard deviations.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import re
from fractions import Fraction

import numpy as np
import pytest

from test_abi_mirror_cpu import DECLARATION, ROOT, c_class, py_class
from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build of all libraries)
from test_indicator_refs_cpu import exported

HEADER = ROOT / "include" / "mcmcref_recdf.h"


@pytest.fixture(scope="module")
def recdf(built_lib):  # noqa: F811
    from mcmc_ref_hip import rankecdf
    return rankecdf


# ---- the table ----------------------------------------------------------------------------------------------------------

def exact_table(M: int, n: int, K: int) -> list:
    rows = []
    total = math.comb(M, n)
    for k in range(1, K):
        m = k * M // K
        pmf = [Fraction(math.comb(m, j) * math.comb(M - m, n - j), total) if j <= m and n - j <= M - m else Fraction(0)
               for j in range(n + 1)]
        low, acc = [], Fraction(0)
        for v in pmf:
            acc += v
            low.append(acc)
        high, acc = [], Fraction(0)
        for v in reversed(pmf):
            acc += v
            high.append(acc)
        high.reverse()
        rows.append([min(a, b) for a, b in zip(low, high)])
    return rows


@pytest.mark.parametrize("M,n,K", [(24, 6, 4), (60, 15, 7), (400, 100, 16)])
def test_table_against_exact_rationals(recdf, M, n, K):
    got, want = recdf.table(M, n, K), exact_table(M, n, K)
    assert got.shape == (K - 1, n + 1)
    worst, tiny = 0.0, Fraction(1, 10 ** 300)
    for k in range(K - 1):
        for j in range(n + 1):
            if want[k][j] >= tiny:
                assert got[k, j] > 0.0, (k, j)
                worst = max(worst, abs(float((Fraction(float(got[k, j])) - want[k][j]) / want[k][j])))
            elif want[k][j] == 0:
                assert got[k, j] == 0.0, (k, j)               # outside the support
    print(f"table ({M}, {n}, {K}): worst relative error {worst:.3g}")
    assert worst <= 1e-9


def test_table_against_scipy(recdf):
    stats = pytest.importorskip("scipy.stats")
    M, n, K = 4000, 1000, 100
    got, j, worst = recdf.table(M, n, K), np.arange(n + 1), 0.0
    for k in range(1, K):
        d = stats.hypergeom(M, k * M // K, n)
        want = np.minimum(d.cdf(j), d.sf(j - 1))
        ok = want >= 1e-300
        assert np.all(got[k - 1][ok] > 0.0)
        worst = max(worst, float(np.max(np.abs(got[k - 1][ok] - want[ok]) / want[ok])))
    print(f"table ({M}, {n}, {K}) against scipy: worst relative error {worst:.3g}")
    assert worst <= 1e-9


def test_worked_example(recdf):
    """The header's example, to the digits it prints."""
    x = np.array([[1.0, 2, 3, 4], [5, 6, 7, 8]])
    r = recdf.rank_ecdf_host(x, points=4, sims=10)
    assert r["counts"].tolist() == [[2, 4, 4], [0, 0, 2]] and r["pooled"].tolist() == [2, 4, 6] and r["tied"] == 0
    near = lambda v: pytest.approx(v, rel=1e-14, abs=0)                      # noqa: E731
    assert r["u"].tolist() == [near(1 / 70)] * 2 and r["kmin"].tolist() == [2, 2] and r["g"] == near(1 / 70) and r["chain"] == 0
    assert r["dev"].tolist() == [0.5, 0.5]
    tab = recdf.table(8, 4, 4)
    assert [tab[0, 2], tab[0, 0], tab[2, 4], tab[2, 2]] == [near(3 / 14)] * 4 and [tab[1, 0], tab[1, 4]] == [near(1 / 70)] * 2
    assert np.all(tab[0, 3:] == 0.0) and np.all(tab[2, :2] == 0.0)            # outside the support
    text = HEADER.read_text()
    for phrase in (f"{1 / 70:.15f}", "a[0] = 2, 4, 4, a[1] = 0, 0, 2", "END INWARD", "SAME BITS", "0x9E3779B97F4A7C15"):
        assert phrase in text, phrase


# ---- the host routine against the restatement -------------------------------------------------------------------------------

def restate(x: np.ndarray, K: int, tab: np.ndarray) -> dict:
    """One parameter x[C][n] by the definition in numpy: sort, `<=`, sum."""
    x = np.asarray(x, dtype=np.float64)
    C_, n = x.shape
    M = C_ * n
    s = np.sort(x.ravel())
    m = np.arange(1, K, dtype=np.int64) * M // K
    a = (x[:, :, None] <= s[m - 1][None, None, :]).sum(axis=1).astype(np.int64)          # [C][K-1]
    R = a.sum(axis=0)
    U = tab[np.arange(K - 1)[None, :], a]
    u = U.min(axis=1)
    return {"counts": a, "pooled": R, "tied": int((R != m).sum()), "u": u, "kmin": U.argmin(axis=1) + 1,
            "dev": np.abs(a * M - n * R[None, :]).max(axis=1) / float(n * M), "g": u.min(), "chain": int(u.argmin())}


KEYS = ("counts", "pooled", "tied", "u", "kmin", "dev", "g", "chain")


def same(got: dict, want: dict, where) -> None:
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (where, k)
        if g.dtype.kind == "f":
            assert g.tobytes() == w.astype(np.float64).tobytes(), (where, k, g, w)
        else:
            assert np.array_equal(g, w), (where, k, g, w)


def points_of(C_: int, n: int) -> list:
    M = C_ * n
    return sorted({K for K in (2, 3, M, n + 1) if 2 <= K <= min(M, 1024)})


def draws_of(kind: str, C_: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((C_, n))
    if kind == "ties":
        return rng.integers(-2, 3, (C_, n)).astype(np.float64)
    if kind == "constant":
        return np.full((C_, n), 0.25)
    if kind == "zeros":
        zeros = np.where(rng.random((C_, n)) < 0.5, -0.0, 0.0)
        return np.where(rng.random((C_, n)) < 0.2, rng.standard_normal((C_, n)), zeros)
    raise AssertionError(kind)


SHAPES = [(C_, n) for C_ in (1, 2, 4, 7) for n in (1, 5, 64, 250) if C_ * n >= 2]


def test_case_list():
    assert len(SHAPES) == 15 and any((C_ * n) % K for C_, n in SHAPES for K in points_of(C_, n))
    assert all(points_of(C_, n) for C_, n in SHAPES) and points_of(7, 250) == [2, 3, 251] and points_of(2, 5) == [2, 3, 6, 10]


@pytest.mark.parametrize("kind", ["normal", "ties", "constant", "zeros"])
@pytest.mark.parametrize("C_,n", SHAPES)
def test_host_matches_the_restatement(recdf, C_, n, kind):
    x = draws_of(kind, C_, n, 100 * C_ + n)
    for K in points_of(C_, n):
        tab = recdf.table(C_ * n, n, K)
        got, want = recdf.rank_ecdf_host(x, points=K, sims=3), restate(x, K, tab)
        same(got, want, (kind, C_, n, K))
        assert (got["thin"], got["n"], got["points"]) == (1, n, K)
        if kind == "constant":
            assert np.all(got["counts"] == n) and got["tied"] == K - 1
        if kind == "normal":
            assert got["tied"] == 0 and np.array_equal(got["pooled"], np.arange(1, K) * (C_ * n) // K)


def test_f32_input_is_widened(recdf):
    x = np.random.default_rng(8).standard_normal((3, 4, 65)).astype(np.float32)
    got = recdf.rank_ecdf_host(x, points=16, sims=3)
    tab = recdf.table(4 * 65, 65, 16)
    for p in range(3):
        same({k: got[k][p] for k in KEYS}, restate(x[p].astype(np.float64), 16, tab), p)


def test_thin_is_a_stride(recdf):
    x = np.random.default_rng(9).standard_normal((2, 3, 101))               # 101 = 7 * 14 + 3: N is no multiple of the stride
    got = recdf.rank_ecdf_host(x, points=10, thin=7, sims=3)
    kept = x[:, :, ::7]
    assert kept.shape[2] == 15 == -(-101 // 7) and (got["thin"], got["n"], got["points"]) == (7, 15, 10)
    tab = recdf.table(3 * 15, 15, 10)
    for p in range(2):
        same({k: got[k][p] for k in KEYS}, restate(kept[p], 10, tab), p)
    assert recdf.rank_ecdf_host(x, thin=7, sims=3)["points"] == 15           # the default: min(n, 100)


def test_refusals(recdf):
    from mcmc_ref_hip import _abi, _eabi
    lib = _eabi.load_recdf_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                  # noqa: E731
    x, out = np.arange(64.0), np.zeros(1)
    none = [None] * 8

    def refused(*args, cause):
        assert lib.mce_rank_ecdf_host(*args, None, *none) == _abi.MCR_EINVAL
        assert cause in lib.mce_last_error(None).decode(), lib.mce_last_error(None)

    refused(None, 2, 8, 4, cause="NULL")
    refused(dp(x), 0, 8, 4, cause=">= 1")
    refused(dp(x), 2, 0, 4, cause=">= 1")
    refused(dp(x), 2 ** 31 // 1024, 1024, 4, cause="2^31")
    refused(dp(x), 2, 8, 1, cause="points")
    refused(dp(x), 2, 8, 17, cause="points")
    refused(dp(x), 1, 2000, _eabi.MCE_MAX_POINTS + 1, cause="MCE_MAX_POINTS")
    assert lib.mce_rank_ecdf_host(dp(x), 2, 8, 16, None, *none) == _abi.MCR_OK          # every output may be NULL
    y = x.copy()
    for bad in (math.nan, math.inf, -math.inf):
        y[5] = bad
        with pytest.raises(_abi.McrError) as exc:
            recdf.rank_ecdf_host(y.reshape(2, 32), points=4, sims=3)
        assert exc.value.code == _abi.MCR_ENONFINITE
    assert lib.mce_table_host(8, 9, 4, dp(np.zeros(64))) == _abi.MCR_EINVAL
    assert lib.mce_null_sample_host(2, 8, 4, 0, 0, dp(out)) == _abi.MCR_EINVAL
    with pytest.raises(ValueError, match="points"):
        recdf.rank_ecdf_host(x.reshape(2, 32), points=65)
    # the entries that take a handle refuse a NULL one without touching a device
    assert lib.mce_set_workspace_limit(None, 1) == _abi.MCR_EINVAL and lib.mce_kernel_ms(None, dp(out), 4) == _abi.MCR_EINVAL
    assert lib.mce_rank_ecdf_dev(None, dp(x), 0, 2, 8, 1, 8, 1, 16, 4, *none) == _abi.MCR_EINVAL
    assert lib.mce_null_sample(None, 2, 8, 4, 10, 0, dp(out)) == _abi.MCR_EINVAL
    assert lib.mce_plan(None, 0, 2, 8, 1, 8, 1, 16, 4, None) == _abi.MCR_EINVAL
    assert lib.mce_version() == _eabi.MCE_VERSION


# ---- the null sample --------------------------------------------------------------------------------------------------------

def null_draws(C_: int, n: int, S: int, seed: int) -> np.ndarray:
    """y[S][C][n] by the header's recipe, in uint64 arithmetic."""
    G = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        z = np.full(S * C_ * n, seed, dtype=np.uint64) * G + np.arange(S * C_ * n, dtype=np.uint64) + G
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(S, C_, n)


@pytest.mark.parametrize("seed", [0, 7, 2 ** 63 + 5])
def test_null_sample_matches_the_recipe(recdf, seed):
    C_, n, K, S = 3, 17, 5, 50
    got = recdf.null_sample_host(C_, n, K, S, seed)
    y, tab = null_draws(C_, n, S, seed), recdf.table(C_ * n, n, K)
    want = np.array([restate(y[s], K, tab)["g"] for s in range(S)])
    assert got.tobytes() == want.tobytes()
    more = recdf.null_sample_host(C_, n, K, 2 * S, seed)
    assert more[:S].tobytes() == got.tobytes()                               # the prefix is stable
    assert recdf.null_sample_host(C_, n, K, S, seed + 1).tobytes() != got.tobytes()


# ---- the rates (fixed seeds) ---------------------------------------------------------------------------------------------------

RATES = dict(points=32, sims=2000, seed=0, alpha=0.05)


def ar1(rng, P: int, C_: int, N: int, phi: float) -> np.ndarray:
    e = rng.standard_normal((P, C_, N))
    z = np.empty_like(e)
    z[..., 0] = e[..., 0]
    for i in range(1, N):
        z[..., i] = phi * z[..., i - 1] + math.sqrt(1.0 - phi * phi) * e[..., i]
    return z


@pytest.fixture(scope="module")
def iid():
    return np.random.default_rng(1).standard_normal((400, 4, 250))


def test_iid_draws_are_rejected_at_the_level(recdf, iid):
    r = recdf.rank_ecdf_host(iid, **RATES)
    rate = float(r["reject"].mean())
    print("iid: rejected", rate)
    assert 0.02 <= rate <= 0.09
    assert np.all(r["tied"] == 0) and np.all((r["pvalue"] > 0) & (r["pvalue"] <= 1))


def test_a_shifted_chain_is_found(recdf, iid):
    x = iid.copy()
    x[:, 2] += 0.3
    r = recdf.rank_ecdf_host(x, **RATES)
    print("chain 2 shifted by 0.3: rejected", r["reject"].mean(), "chain == 2 in", (r["chain"] == 2).mean())
    assert r["reject"].mean() >= 0.70 and (r["chain"] == 2).mean() >= 0.85


def test_a_scaled_chain_is_rejected(recdf, iid):
    x = iid.copy()
    x[:, 1] *= 1.5
    r = recdf.rank_ecdf_host(x, **RATES)
    print("chain 1 scaled by 1.5: rejected", r["reject"].mean())
    assert r["reject"].mean() >= 0.95


def test_autocorrelated_chains_need_thinning(recdf):
    r = recdf.rank_ecdf_host(ar1(np.random.default_rng(2), 200, 4, 250, 0.9), **RATES)
    print("AR(0.9) unthinned: rejected", r["reject"].mean())
    assert r["reject"].mean() >= 0.80
    r = recdf.rank_ecdf_host(ar1(np.random.default_rng(3), 200, 4, 5000, 0.9), thin=20, **RATES)
    print("AR(0.9) at thin=20: rejected", r["reject"].mean())
    assert r["n"] == 250 and r["reject"].mean() <= 0.15


# ---- the mirror of the header, and the libraries' exports ---------------------------------------------------------------------

EDEFINE = re.compile(r"^[ \t]*#define[ \t]+(MCE_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)
EDECLARATION = re.compile(DECLARATION.pattern.replace("mcr_", "mce_"), re.M)


@pytest.fixture(scope="module")
def eheader() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_mirror_constants(eheader, recdf):
    from mcmc_ref_hip import _eabi
    defines = {k: int(v) for k, v in EDEFINE.findall(eheader)}
    mirrored = {k: v for k, v in vars(_eabi).items() if k.startswith("MCE_") and isinstance(v, int)}
    assert mirrored == defines and len(defines) == 10
    assert defines["MCE_MAX_POINTS"] == 1024 and defines["MCE_MAX_POINTS"] * 8 <= 8 * 1024      # the thresholds: <= 8 KB of LDS
    assert defines["MCE_HIST_BYTES"] + defines["MCE_MAX_POINTS"] * 8 <= 32 * 1024               # five workgroups per CU
    assert defines["MCE_HIST_BYTES"] // (4 * defines["MCE_MAX_POINTS"]) >= 1
    assert defines["MCE_KERNELS"] == len(_eabi.KERNEL_NAMES)
    assert "typedef" not in eheader and "struct" not in HEADER.read_text()
    assert recdf.chain_tile(4, 10000, 100) == 1 and recdf.chain_tile(4, 250, 32) == 4 and recdf.chain_tile(100, 63, 64) == 96
    assert recdf.chain_tile(64, 1, 1024) == 6


def test_mirror_functions_and_exports(eheader, built_lib):  # noqa: F811
    from mcmc_ref_hip import _eabi
    named = set(re.findall(r"\b(mce_[a-z0-9_]+)\s*\(", eheader))
    parsed = {m.group(2): (m.group(1), m.group(3)) for m in EDECLARATION.finditer(eheader)}
    assert named == set(parsed) == set(_eabi.ESYMBOLS) and len(named) == 15
    lib = _eabi.load_recdf_library()
    for name, (ret, params) in sorted(parsed.items()):
        restype, argtypes = _eabi.ESYMBOLS[name]
        params = [p for p in params.split(",") if p.strip() != "void"]
        assert [py_class(t) for t in argtypes] == [c_class(p) for p in params], name
        assert py_class(restype) == c_class(ret), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    outs = [p.split()[-1].lstrip("*") for p in parsed["mce_rank_ecdf_host"][1].split(",")[5:]]
    assert tuple(outs) == tuple(name for name, _, _ in _eabi.OUTPUTS)         # the order the Python layer passes them in
    for entry in ("mce_rank_ecdf", "mce_rank_ecdf_dev"):
        assert [p.split()[-1].lstrip("*") for p in parsed[entry][1].split(",")[10:]] == outs
    width = {"int32_t": "int32", "int64_t": "int64", "double": "float64"}
    kinds = [width[p.split()[0].rstrip("*")] for p in parsed["mce_rank_ecdf_host"][1].split(",")[5:]]
    assert kinds == [dtype for _, dtype, _ in _eabi.OUTPUTS]                   # pointers all look alike to c_class: the widths
    fifth = built_lib.with_name("libmcmcref_recdf.so")
    assert fifth.exists()
    assert exported(fifth) == named                                # mce_* and nothing else, whatever is linked in


def test_the_other_libraries_export_what_they_did(built_lib):  # noqa: F811
    from mcmc_ref_hip import _abi, _babi, _iabi, _sabi, _xabi
    assert exported(built_lib) == set(_abi.SYMBOLS) | set(_xabi.XSYMBOLS)
    assert exported(built_lib.with_name("libmcmcref_iess.so")) == set(_iabi.ISYMBOLS)
    assert exported(built_lib.with_name("libmcmcref_bm.so")) == set(_babi.BSYMBOLS)
    assert exported(built_lib.with_name("libmcmcref_std.so")) == set(_sabi.SSYMBOLS)
    for header in ("mcmcref_hip.h", "mcmcref_hip_ext.h", "mcmcref_iess.h", "mcmcref_bm.h", "mcmcref_std.h"):
        assert "mce_" not in (ROOT / "include" / header).read_text().lower()


def test_ffi_knows_nothing_of_the_companion():
    from mcmc_ref_hip import _eabi, _ffi, rankecdf
    assert not [k for k, v in vars(_ffi).items() if v is _eabi or v is rankecdf]
    assert not [k for k in vars(_ffi) if k.lower().startswith(("mce", "recdf", "rankecdf", "rank_ecdf"))]
    assert not set(_ffi.SYMBOLS) & set(_eabi.ESYMBOLS)


def test_build_lists_the_unit(built_lib):  # noqa: F811
    import importlib.util
    spec = importlib.util.spec_from_file_location("mcr_build_recdf", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.RECDF_UNITS == ("mce_api",) and mod.RECDF_OUT.name == "libmcmcref_recdf.so"
    assert len(mod.LIBRARIES) == 5 and mod.LIBRARIES[-1][1] == mod.UNITS + mod.RECDF_UNITS


# ---- the command ---------------------------------------------------------------------------------------------------------------

def test_the_command(recdf, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip.cli import main
    out = CliRunner().invoke(main, ["rank-ecdf", "--help"])
    assert out.exit_code == 0 and "--points" in out.output and "--thin" in out.output and "--sims" in out.output
    x = np.random.default_rng(4).standard_normal((2, 3, 40))
    x[1, 2] += 3.0
    csv = tmp_path / "draws.csv"
    with open(csv, "w") as f:
        f.write("chain,draw,a,b\n")
        for c in range(3):
            for i in range(40):
                f.write(f"{c},{i},{float(x[0, c, i])!r},{float(x[1, c, i])!r}\n")
    assert CliRunner().invoke(main, ["rank-ecdf", str(csv), "--points", "1", "--host"]).exit_code != 0
    assert CliRunner().invoke(main, ["rank-ecdf", str(csv), "--points", "500", "--host"]).exit_code != 0     # more than C n
    assert CliRunner().invoke(main, ["rank-ecdf", str(csv), "--thin", "0", "--host"]).exit_code != 0
    assert CliRunner().invoke(main, ["rank-ecdf", "no_such_file.csv"]).exit_code != 0
    args = ["--points", "8", "--sims", "200", "--seed", "3", "--host"]
    want = recdf.rank_ecdf_file(csv, points=8, sims=200, seed=3, host=True)
    assert list(want) == ["a", "b"] and want["b"]["reject"] and want["b"]["chain"] == 2
    direct = recdf.rank_ecdf_host(x, points=8, sims=200, seed=3)
    assert want["b"]["pvalue"] == direct["pvalue"][1] and want["b"]["max_diff"] == direct["dev"][1, 2]
    assert want["b"]["quantile"] == direct["kmin"][1, 2] / 8 and (want["a"]["n"], want["a"]["points"], want["a"]["thin"]) == (40, 8, 1)
    res = CliRunner().invoke(main, ["rank-ecdf", str(csv), "--json"] + args)
    assert res.exit_code == 0, res.output
    assert json.loads(res.output) == json.loads(json.dumps(want))
    res = CliRunner().invoke(main, ["rank-ecdf", str(csv), "--params", "b", "--thin", "2"] + args)
    assert res.exit_code == 0, res.output                          # a rejection is a result, not an error
    lines = res.output.splitlines()
    assert lines[0].split()[0] == "param" and {"pvalue", "reject", "chain", "quantile", "max_diff"} <= set(lines[0].split())
    assert len(lines) == 2 and lines[1].split()[0] == "b"
