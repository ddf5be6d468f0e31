"""The Stan-convention diagnostics of include/mcmcref_std.h without a GPU: the host routine mcs_diagnostics_host held to a
numpy restatement of the definition (std_cases.py: FFT autocovariances, scipy's rankdata and ndtri) over the whole case
list, the header's worked example to the digit, the edge rules, three sanity checks against theory, the refusals, and the
mirror `_sabi` against the header and the exports of libmcmcref_std.so.  The other three libraries export what they
exported before.

Tolerances: every floating output is held to 1e-9 relative, the project's gate for an output against a restatement of the
same definition (the two differ in summation order, FFT against direct products, and in the inverse normal CDF: errors
of 1e-13 and below).  The lags are integers and must be equal; that means something only while no decision of a walk is
within those errors of a tie, so every case must have margin >= 1e-7 (the smallest on this list is 1e-4).
"""
from __future__ import annotations

import ctypes as C
import math
import re

import numpy as np
import pytest

import std_cases as sc
from test_abi_mirror_cpu import DECLARATION, ROOT, c_class, py_class
from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build of all libraries)
from test_indicator_refs_cpu import exported

HEADER = ROOT / "include" / "mcmcref_std.h"


@pytest.fixture(scope="module")
def std(built_lib):  # noqa: F811
    from mcmc_ref_hip import standard
    return standard


# ---- the host routine against the restatement ---------------------------------------------------------------------------

def test_case_list():
    assert len(sc.CASES) == 9 * 4 * 6 - 9 and len(sc.shapes()) == 36
    assert {k for k, *_ in sc.CASES} == set(sc.KINDS) and {n for *_, n, _ in sc.CASES} == set(sc.NS)


@pytest.mark.parametrize("C_,N,cases", sc.shapes(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_host_matches_the_restatement(std, C_, N, cases):
    x = sc.tensor_of(C_, N, cases)
    got = std.diagnostics_host(x, basic=True)
    for p, (kind, seed) in enumerate(cases):
        want = sc.restate(x[p])
        where = (kind, C_, N, seed)
        if N // 2 >= 4:
            assert want["margin"] >= sc.MARGIN_MIN and got["margin"][p] >= sc.MARGIN_MIN, (where, want["margin"])
            assert sc.close(float(got["margin"][p]), want["margin"], 1e-6), where
            if kind == "shifted":
                assert want["lag_bulk"] >= N // 2 - 6, where       # the walk reached n - 5 (the first even lag there)
        else:
            assert math.isnan(want["margin"]) and math.isnan(got["margin"][p])
        sc.same(sc.at(got, p), want, where)


def test_worked_example(std):
    """The header's example, to the digits it prints."""
    x = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 1, 8, 2, 7, 3, 6, 4, 5.0]])
    w = sc.walk_of(sc.split(x))
    text = HEADER.read_text()
    assert np.allclose(w["g"][:4], [5.25, -0.5, 2.375, -1.3125], rtol=0, atol=1e-12)      # (an FFT: not to the bit)
    for v in (w["rho"][1], w["rho"][2], w["rho"][3], w["tau"], 1.0 / math.log10(16)):
        assert f"{v:.15f}" in text, v
    assert "gamma(1) = -0.5, gamma(2) = 2.375, gamma(3) = -1.3125" in text and "ess_mean = 16 / tau = 19.2, lag_mean = 2" in text
    assert (w["lag"], round(w["tau"] * 6, 12), round(w["margin"] * 12, 12)) == (2, 5.0, 1.0)
    got = std.diagnostics_host(x, basic=True)
    assert got["lag_mean"] == 2 and sc.close(got["ess_mean"], 19.2) and sc.close(got["mcse_mean"], x.std(ddof=1) / math.sqrt(19.2))
    # rank scores of the same chain: both halves hold each of the ranks' scores once -- equal means, R-hat below 1
    assert sc.close(got["rhat"], sc.restate(x)["rhat"]) and got["rhat"] < 1.0


# ---- edge rules -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7])
def test_short_chains_have_no_ess(std, N):
    x = np.random.default_rng(N).standard_normal((3, N))
    got = std.diagnostics_host(x, basic=True)
    for k in ("ess_bulk", "ess_tail", "ess_q05", "ess_q95", "ess_mean", "mcse_mean", "margin"):
        assert math.isnan(got[k]), k
    assert all(got[k] == -1 for k in sc.LAGS)
    want = sc.restate(x)
    for k in ("rhat", "rhat_bulk", "rhat_tail", "rhat_basic"):
        assert sc.close(got[k], want[k]), k
    assert math.isnan(got["rhat"]) == (N < 4)                     # n = 1: no within-chain variance


def test_constant_parameter_and_constant_indicator(std):
    got = std.diagnostics_host(np.full((2, 40), 0.1), basic=True)
    assert all(math.isnan(got[k]) for k in sc.DOUBLES) and all(got[k] == -1 for k in sc.LAGS)
    # half the draws tie at the maximum: the 95 % quantile is the maximum and its indicator is 1 everywhere
    x = (np.random.default_rng(5).random((4, 200)) < 0.5) * 1.0
    got, want = std.diagnostics_host(x, basic=True), sc.restate(x)
    assert math.isnan(got["ess_q95"]) and got["lag_q95"] == -1 and math.isnan(got["ess_tail"])
    assert not math.isnan(got["ess_q05"]) and not math.isnan(got["ess_bulk"])
    sc.same(got, want, "binary")


@pytest.mark.parametrize("C_,N", [(1, 9), (3, 17), (2, 1023)])
def test_odd_n_drops_the_middle_draw(std, C_, N):
    x = sc.chains_of("ar0.9", C_, N, 77)
    y = x.copy()
    y[:, N // 2] = np.linspace(-50.0, 50.0, C_)
    a, b = std.diagnostics_host(x, basic=True), std.diagnostics_host(y, basic=True)
    assert sc.bits(a) == sc.bits(b)                               # the middle draw takes part in nothing
    even = np.delete(x, N // 2, axis=1)                           # ... and the answer is the even-N one of the kept draws
    assert sc.bits(a) == sc.bits(std.diagnostics_host(even, basic=True))


def test_non_finite_draws_are_refused(std):
    from mcmc_ref_hip import _abi
    x = np.random.default_rng(3).standard_normal((2, 20))
    for bad in (math.nan, math.inf, -math.inf):
        y = x.copy()
        y[1, 3] = bad
        with pytest.raises(_abi.McrError) as exc:
            std.diagnostics_host(y)
        assert exc.value.code == _abi.MCR_ENONFINITE
    y = np.random.default_rng(3).standard_normal((2, 21))
    y[0, 10] = math.nan                                           # the middle draw of an odd chain is not even looked at
    assert not math.isnan(std.diagnostics_host(y)["ess_bulk"])


def test_basic_outputs_only_on_request(std):
    x = sc.chains_of("iid", 2, 64, 9)
    plain, basic = std.diagnostics_host(x), std.diagnostics_host(x, basic=True)
    assert set(basic) - set(plain) == set(std.BASIC_OUTPUTS)
    assert sc.bits(plain) == sc.bits({k: basic[k] for k in plain})


# ---- sanity against theory (fixed seeds) ------------------------------------------------------------------------------------
# Seeds chosen to hold with room: over seeds 1 .. 12 ess_bulk of the iid case ran from 3492 to 4162 (seed 1: 4039), ess_mean
# of the AR(0.9) case from 345 to 500 around the theory's 421 (seed 6: 425), R-hat of the shifted case from 1.42 to 1.44.

def test_iid_draws_have_about_s_effective_draws(std):
    got = std.diagnostics_host(np.random.default_rng(1).standard_normal((4, 1000)), basic=True)
    print("iid 4 x 1000: ess_bulk", got["ess_bulk"], "ess_mean", got["ess_mean"], "rhat", got["rhat"])
    assert abs(got["ess_bulk"] - 4000.0) <= 400.0 and got["rhat"] < 1.01


def test_ar1_ess_mean_is_near_theory(std):
    phi = 0.9
    got = std.diagnostics_host(sc.ar1(np.random.default_rng(6), 4, 2000, phi), basic=True)
    theory = 8000.0 * (1.0 - phi) / (1.0 + phi)
    print("AR(0.9) 4 x 2000: ess_mean", got["ess_mean"], "theory", theory)
    assert abs(got["ess_mean"] - theory) <= 0.25 * theory


def test_a_shifted_chain_is_flagged(std):
    got = std.diagnostics_host(sc.chains_of("shifted", 4, 1000, 1))
    print("one chain of 4 shifted by 3: rhat", got["rhat"])
    assert got["rhat"] > 1.2


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(std):
    from mcmc_ref_hip import _abi, _sabi
    lib = _sabi.load_std_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
    x, out = np.zeros(64), np.zeros(1)
    none = [None] * 15

    def refused(*args, cause):
        assert lib.mcs_diagnostics_host(*args, dp(out), *none[1:]) == _abi.MCR_EINVAL
        assert cause in lib.mcs_last_error(None).decode(), lib.mcs_last_error(None)

    refused(None, 2, 8, 0, cause="NULL")
    refused(dp(x), 0, 8, 0, cause=">= 1")
    refused(dp(x), 2, 1, 0, cause="N >= 2")
    refused(dp(x), 1, _sabi.MCS_MAX_DRAWS + 1, 0, cause="MCS_MAX_DRAWS")
    refused(dp(x), 2 ** 31 // 1024, 1024, 0, cause="2^31")
    refused(dp(x), 2, 8, 2, cause="MCS_WANT_BASIC")
    assert lib.mcs_diagnostics_host(dp(x + np.arange(64)), 2, 8, 1, *none) == _abi.MCR_OK      # every output may be NULL
    # the entries that take a handle refuse a NULL one without touching a device
    assert lib.mcs_set_workspace_limit(None, 1) == _abi.MCR_EINVAL and lib.mcs_kernel_ms(None, dp(out), 3) == _abi.MCR_EINVAL
    assert lib.mcs_diagnostics_dev(None, dp(x), 0, 2, 8, 1, 8, 1, 16, 0, *none) == _abi.MCR_EINVAL
    assert lib.mcs_plan(None, 0, 2, 8, 1, 8, 1, 16, 0, None) == _abi.MCR_EINVAL
    assert lib.mcs_version() == _sabi.MCS_VERSION


# ---- the mirror of the header, and the libraries' exports ---------------------------------------------------------------------

SDEFINE = re.compile(r"^[ \t]*#define[ \t]+(MCS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)
SDECLARATION = re.compile(DECLARATION.pattern.replace("mcr_", "mcs_"), re.M)


@pytest.fixture(scope="module")
def sheader() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_mirror_constants(sheader):
    from mcmc_ref_hip import _sabi
    defines = {k: int(v) for k, v in SDEFINE.findall(sheader)}
    mirrored = {k: v for k, v in vars(_sabi).items() if k.startswith("MCS_") and isinstance(v, int)}
    assert mirrored == defines and len(defines) == 9
    assert defines["MCS_MAX_DRAWS"] == 1 << 20 and defines["MCS_LAG_BLOCK"] == 256 and defines["MCS_LDS_DRAWS"] * 8 <= 60 * 1024
    assert defines["MCS_KERNELS"] == len(_sabi.KERNEL_NAMES)
    assert "typedef" not in sheader and "struct" not in HEADER.read_text()
    text = HEADER.read_text()
    for phrase in ("DEVIATION for odd N", "takes part in\n * NOTHING", "no package output pins it", "O(n^2)"):
        assert phrase in text, phrase


def test_mirror_functions_and_exports(sheader, built_lib):  # noqa: F811
    from mcmc_ref_hip import _sabi
    named = set(re.findall(r"\b(mcs_[a-z0-9_]+)\s*\(", sheader))
    parsed = {m.group(2): (m.group(1), m.group(3)) for m in SDECLARATION.finditer(sheader)}
    assert named == set(parsed) == set(_sabi.SSYMBOLS) and len(named) == 11
    lib = _sabi.load_std_library()
    for name, (ret, params) in sorted(parsed.items()):
        restype, argtypes = _sabi.SSYMBOLS[name]
        params = [p for p in params.split(",") if p.strip() != "void"]
        assert [py_class(t) for t in argtypes] == [c_class(p) for p in params], name
        assert py_class(restype) == c_class(ret), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype, name
    outs = [p.split()[-1].lstrip("*") for p in parsed["mcs_diagnostics_host"][1].split(",")[4:]]
    assert tuple(outs) == _sabi.DOUBLE_OUTPUTS + _sabi.INT_OUTPUTS            # the order the Python layer passes them in
    fourth = built_lib.with_name("libmcmcref_std.so")
    assert fourth.exists()
    assert exported(fourth) == named                               # mcs_* and nothing else, whatever is linked in


def test_the_other_libraries_export_what_they_did(built_lib):  # noqa: F811
    from mcmc_ref_hip import _abi, _babi, _iabi, _xabi
    assert exported(built_lib) == set(_abi.SYMBOLS) | set(_xabi.XSYMBOLS)
    assert len(_abi.SYMBOLS) == 143 and len(_xabi.XSYMBOLS) == 10
    assert exported(built_lib.with_name("libmcmcref_iess.so")) == set(_iabi.ISYMBOLS)
    assert exported(built_lib.with_name("libmcmcref_bm.so")) == set(_babi.BSYMBOLS)
    for header in ("mcmcref_hip.h", "mcmcref_hip_ext.h", "mcmcref_iess.h", "mcmcref_bm.h"):
        assert "mcs_" not in (ROOT / "include" / header).read_text().lower()


def test_ffi_knows_nothing_of_the_companion():
    from mcmc_ref_hip import _ffi, _sabi, standard
    assert not [k for k, v in vars(_ffi).items() if v is _sabi or v is standard]
    assert not [k for k in vars(_ffi) if k.lower().startswith(("mcs", "std_", "standard"))]
    assert not set(_ffi.SYMBOLS) & set(_sabi.SSYMBOLS)


def test_build_lists_the_unit(built_lib):  # noqa: F811
    import importlib.util
    spec = importlib.util.spec_from_file_location("mcr_build_std", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.STD_UNITS == ("mcs_api",) and mod.STD_OUT.name == "libmcmcref_std.so"
    assert mod.UNITS == ("mcr_api", "mcr_stats", "mcr_files", "mcr_comm")
