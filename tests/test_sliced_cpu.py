"""The sliced KS / Wasserstein check without a GPU: the direction recipe, the inputs of the separating-power test and the
C entry's NULL-context answer.

`separation_case` is the one statement of those inputs; tests/test_sliced_gpu.py imports it, so what is pinned here with
numpy + scipy is what goes through `validate()` and the CLI there.  `sliced_reference` is the statistic in numpy + scipy:
the projection as a matrix product (not the device's fixed-order fma chain: the thresholds sit a factor of 1.5 or more
away from the figures, rounding does not matter here)."""
from __future__ import annotations

import ctypes as C
import importlib.util

import numpy as np
import pytest

from conftest import ROOT

PARAMS = ("a", "b")
SLICED_K, SLICED_SEED = 16, 4711


def separation_case():
    """(reference [2][2000], wrong-correlation actual [2][2037], control [2][2037]): unit marginals everywhere,
    correlation +0.9 in the reference and the control, -0.9 in the actual.  One generator, drawn from in this order."""
    rng = np.random.default_rng(0)
    plus = np.linalg.cholesky(np.array([[1.0, 0.9], [0.9, 1.0]]))
    minus = np.linalg.cholesky(np.array([[1.0, -0.9], [-0.9, 1.0]]))
    ref = plus @ rng.normal(size=(2, 2000))
    actual = minus @ rng.normal(size=(2, 2037))
    control = plus @ rng.normal(size=(2, 2037))
    return ref, actual, control


def sliced_reference(ref, act, W, center):
    from scipy.stats import ks_2samp, wasserstein_distance
    zr, za = W @ (ref - center[:, None]), W @ (act - center[:, None])
    ks = np.array([ks_2samp(r, a).statistic for r, a in zip(zr, za)])
    w1 = np.array([wasserstein_distance(r, a) for r, a in zip(zr, za)])
    return ks, w1


@pytest.fixture(scope="module")
def ffi():
    spec = importlib.util.spec_from_file_location("mcr_build", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from mcmc_ref_hip import _ffi
    _ffi.load_library()
    return _ffi


def test_directions_are_unit_rows_of_the_standardised_space():
    from mcmc_ref_hip.validate import sliced_directions
    std = np.array([2.0, 0.0, 1e-3, np.nan, 5e4, np.inf, 1.0])
    W, live = sliced_directions(9, std)
    assert W.shape == (9, 7) and live.tolist() == [True, False, True, False, True, False, True]
    assert not W[:, ~live].any()                                   # weight 0 where std is 0 or not finite
    U = W[:, live] * std[live]
    assert np.allclose(np.linalg.norm(U, axis=1), 1.0, rtol=0, atol=8 * 2.0 ** -52)
    # the documented recipe, outside the package
    G = np.random.default_rng(4711).standard_normal((9, 4))
    want = G / np.linalg.norm(G, axis=1, keepdims=True) / std[live]
    assert np.array_equal(W[:, live], want)


def test_directions_depend_on_the_seed_alone():
    from mcmc_ref_hip.validate import sliced_directions
    std = np.array([1.0, 3.0, 0.5])
    a, _ = sliced_directions(16, std, seed=4711)
    b, _ = sliced_directions(16, std)
    c, _ = sliced_directions(16, std, seed=4712)
    assert a.tobytes() == b.tobytes()
    assert not np.array_equal(a, c)
    few, _ = sliced_directions(3, std)
    assert few.shape == (3, 3)
    none, live = sliced_directions(4, np.zeros(3))
    assert not none.any() and not live.any()
    empty, _ = sliced_directions(0, std)
    assert empty.shape == (0, 3)


def test_separating_power_of_the_statistic_on_the_gpu_tests_inputs():
    """The thresholds tests/test_sliced_gpu.py asserts through validate(), here on the host: every marginal KS < 0.1,
    largest sliced KS > 0.2 for the wrong correlation and < 0.1 for the control."""
    from scipy.stats import ks_2samp
    from mcmc_ref_hip.validate import sliced_directions
    ref, actual, control = separation_case()
    assert ref.shape == (2, 2000) and actual.shape == control.shape == (2, 2037)
    W, live = sliced_directions(SLICED_K, ref.std(axis=1), SLICED_SEED)
    assert live.all()
    center = ref.mean(axis=1)
    for other in (actual, control):
        marginal = max(ks_2samp(ref[i], other[i]).statistic for i in range(2))
        print("largest marginal KS", marginal)
        assert marginal < 0.1
    ks, w1 = sliced_reference(ref, actual, W, center)
    print("wrong correlation: largest sliced KS", ks.max(), "W1", w1.max())
    assert ks.max() > 0.2
    worst = W[int(np.argmax(ks))] * ref.std(axis=1)
    assert worst[0] * worst[1] > 0 and 1 / 3 < abs(worst[0] / worst[1]) < 3       # along a + b, where the variances differ
    ks, w1 = sliced_reference(ref, control, W, center)
    print("control: largest sliced KS", ks.max(), "W1", w1.max())
    assert ks.max() < 0.1


def test_null_context_is_einval(ffi):
    lib = ffi.load_library()
    x = np.zeros(4)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for entry in (lib.mcr_sliced_two_sample, lib.mcr_sliced_two_sample_dev):
        rc = entry(None, dp(x), 2, dp(x), 2, 2, dp(x), None, 1, dp(x), dp(x), None, None)
        assert rc == ffi.MCR_EINVAL
    v = C.c_int64(7)
    assert lib.mcr_sliced_plan(None, 2, 2, 2, 1, C.byref(v)) == ffi.MCR_EINVAL


def test_validate_cli_is_registered():
    from click.testing import CliRunner
    from mcmc_ref_hip.cli import main
    out = CliRunner().invoke(main, ["validate", "--help"])
    assert out.exit_code == 0
    for opt in ("--actual", "--tolerance", "--metrics", "--ks-max", "--w1-scaled-max", "--sliced", "--sliced-seed", "--sliced-ks-max",
                "--sliced-w1-max", "--format"):
        assert opt in out.output
