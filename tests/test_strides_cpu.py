"""Strided and non-contiguous draw tensors, the CPU side: the view builders the GPU stride tests share, the oracle's
stride reads, and `_ffi.tensor_args`.

The C ABI describes a draws tensor by element strides (stride_c, stride_n, stride_p) (include/mcmcref_hip.h,
"Conventions"), and callers hand over views: `x[:, warmup:, :]`, `x[:, ::k, :]`, `x[..., idx]`, permuted tensors.
tests/test_strides_gpu.py compares every such view with the contiguous [P][C][N] call and with `oracle.summarize` on the
view itself; this file shows that the oracle reads the views right and that `tensor_args` passes their strides through.
"""
from __future__ import annotations

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

LAYOUTS = ("pcn", "pnc", "cpn", "cnp", "npc", "ncp")
SLACK = 4096        # NaN elements behind every base: a read past a view's extent stays inside its allocation


def to_pcn(a: np.ndarray, layout: str) -> np.ndarray:
    """The [P][C][N] view of an array whose axes are `layout`."""
    return np.transpose(a, [layout.index(ax) for ax in "pcn"])


def contiguous_pcn(a: np.ndarray, layout: str) -> np.ndarray:
    return np.ascontiguousarray(to_pcn(a, layout))


def natural(layout: str, C: int, N: int, P: int, gap: dict | None = None, step: int = 1) -> tuple[int, int, int]:
    """(stride_c, stride_n, stride_p) of a [layout] array: the innermost axis has stride `step`, and gap[a] elements of
    padding follow every row of axis a ({"n": 3} in "pcn" pads the chains, {"c": 5} the parameters)."""
    dims, gap, s, st = {"c": C, "n": N, "p": P}, gap or {}, step, {}
    for a in reversed(layout):
        st[a] = s
        s = s * dims[a] + gap.get(a, 0)
    return st["c"], st["n"], st["p"]


def strided(x: np.ndarray, layout: str, strides, offset: int = 0, dtype=None):
    """x [P][C][N] written into a NaN-filled flat base at element `offset` with element strides (sc, sn, sp), returned as
    a read-only view whose axes are `layout`, and the base.  Elements the view does not cover stay NaN, so a kernel that
    reads one rejects the call (MCR_ENONFINITE) or returns NaN.  Zero strides alias: an aliased element keeps one of the
    values written to it, and the view is whatever the base then holds (compare with the view, not with x)."""
    dtype = np.dtype(dtype or x.dtype)
    P, C, N = x.shape
    sc, sn, sp = strides
    ext = (C - 1) * sc + (N - 1) * sn + (P - 1) * sp + 1 if x.size else 0
    base = np.full(offset + ext + SLACK, np.nan, dtype=dtype)
    es = dtype.itemsize
    shape, byte_strides = (P, C, N), (sp * es, sc * es, sn * es)
    as_strided(base[offset:], shape, byte_strides)[...] = x
    v = as_strided(base[offset:], shape, byte_strides, writeable=False)
    return np.transpose(v, ["pcn".index(a) for a in layout]), base


def view_cases(C: int, N: int, P: int):
    """(name, layout, (sc, sn, sp), offset) of the views the stride tests run: all six axis orders, padded chains and
    parameters, thinned draws, a warmup slice, a parameter subset, and zero strides."""
    cases = [(lay, lay, natural(lay, C, N, P), 0) for lay in LAYOUTS]
    W = 5
    cases += [
        ("pcn padded chains", "pcn", natural("pcn", C, N, P, gap={"n": 3}), 0),
        ("pcn padded params", "pcn", natural("pcn", C, N, P, gap={"c": 5}), 0),
        ("pnc padded params", "pnc", natural("pnc", C, N, P, gap={"n": 7}), 0),
        ("npc padded", "npc", natural("npc", C, N, P, gap={"c": 1, "p": 2}), 0),
        ("cpn padded", "cpn", natural("cpn", C, N, P, gap={"n": 1}), 0),
        ("pcn thinned x2", "pcn", natural("pcn", C, N, P, step=2), 0),
        ("cnp thinned x3", "cnp", (3 * N * P, 3 * P, 1), 0),                        # x[:, ::3, :]
        ("cnp warmup slice", "cnp", ((N + W) * P, P, 1), W * P),                    # x[:, W:, :]
        ("cnp param subset", "cnp", (N * (2 * P + 1), 2 * P + 1, 2), 1),            # x[..., 1::2]
        ("ncp offset", "ncp", natural("ncp", C, N, P), 3),
        ("sc=0 identical chains", "pcn", (0, 1, N), 0),
        ("sp=0 aliased params", "pcn", (N, 1, 0), 0),
        ("sn=0 constant chains", "cnp", (P, 0, 1), 0),
    ]
    return cases


def random_draws(P: int, C: int, N: int, seed: int) -> np.ndarray:
    """[P][C][N] draws of different location, scale and autocorrelation per parameter (some ties)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(P, C, N))
    x = np.cumsum(x * 0.3, axis=2) + x                      # mild autocorrelation
    x = x * 10.0 ** rng.integers(-2, 3, size=(P, 1, 1)) + rng.normal(size=(P, 1, 1)) * 5
    if P > 1:
        x[1] = np.round(x[1], 0)                            # ties
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the oracle reads strides (the GPU tests compare every view with oracle.summarize on the view itself)
# ---------------------------------------------------------------------------------------------------------------------
def _same_bits(a: dict, b: dict, what: str):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert x.shape == y.shape and np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oracle_on_a_view_equals_the_oracle_on_its_contiguous_copy(oracle, dtype):
    C, N, P = 4, 70, 3
    x = random_draws(P, C, N, seed=7)
    for name, layout, strides, offset in view_cases(C, N, P):
        v, _ = strided(x, layout, strides, offset, dtype)
        exp = oracle.summarize(contiguous_pcn(v, layout), "pcn", min_chains=1)
        got = oracle.summarize(v, layout, min_chains=1)
        _same_bits(got, exp, name)


def test_strided_builder_places_the_draws():
    from mcmc_ref_hip import _ffi
    C, N, P = 3, 5, 4
    x = random_draws(P, C, N, seed=1)
    for name, layout, strides, offset in view_cases(C, N, P):
        v, base = strided(x, layout, strides, offset)
        assert _ffi.tensor_args(v, layout)[4:] == strides, name
        assert v.__array_interface__["data"][0] - base.ctypes.data == offset * base.itemsize, name
        if 0 not in strides:
            assert np.array_equal(contiguous_pcn(v, layout), x), name
    # natural strides of the six orders are numpy's own
    for lay in LAYOUTS:
        a = np.empty([{"c": C, "n": N, "p": P}[ax] for ax in lay])
        st = {ax: a.strides[i] // 8 for i, ax in enumerate(lay)}
        assert natural(lay, C, N, P) == (st["c"], st["n"], st["p"]), lay


# ---------------------------------------------------------------------------------------------------------------------
# _ffi.tensor_args
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tensor_args_of_the_six_orders(layout, dtype):
    from mcmc_ref_hip import _ffi
    C, N, P = 3, 11, 5
    dims = {"c": C, "n": N, "p": P}
    a = np.zeros([dims[ax] for ax in layout], dtype=dtype)
    code = _ffi.MCR_F64 if dtype == np.float64 else _ffi.MCR_F32
    assert _ffi.tensor_args(a, layout) == (code, C, N, P, *natural(layout, C, N, P))
    # the same memory described in another axis order: the strides follow the axes, not their position
    for other in LAYOUTS:
        t = np.transpose(a, [layout.index(ax) for ax in other])
        assert _ffi.tensor_args(t, other) == (code, C, N, P, *natural(layout, C, N, P)), other


def test_tensor_args_of_sliced_views():
    from mcmc_ref_hip import _ffi
    C, Nf, P = 4, 100, 9
    x = np.zeros((C, Nf, P))                                        # Draws.to_numpy: [C][N][P]
    F = _ffi.MCR_F64
    assert _ffi.tensor_args(x[:, 20:, :], "cnp") == (F, C, 80, P, Nf * P, P, 1)         # warmup dropped
    assert _ffi.tensor_args(x[:, ::3, :], "cnp") == (F, C, 34, P, Nf * P, 3 * P, 1)     # thinned
    assert _ffi.tensor_args(x[..., 1::2], "cnp") == (F, C, Nf, 4, Nf * P, P, 2)         # parameter subset
    assert _ffi.tensor_args(x[1:3, 5:50:5, 2:8], "cnp") == (F, 2, 9, 6, Nf * P, 5 * P, 1)
    y = np.zeros((P, C, Nf), dtype=np.float32)                      # the Arrow layout [P][C][N]
    assert _ffi.tensor_args(y[:, :, 10:], "pcn") == (_ffi.MCR_F32, C, 90, P, Nf, 1, C * Nf)
    assert _ffi.tensor_args(y[::2, 1:, ::4], "pcn") == (_ffi.MCR_F32, C - 1, 25, 5, Nf, 4, 2 * C * Nf)
    t = np.transpose(y, (1, 2, 0))                                  # a permuted tensor, no copy
    assert _ffi.tensor_args(t, "cnp") == (_ffi.MCR_F32, C, Nf, P, Nf, 1, C * Nf)


def test_tensor_args_of_zero_stride_views():
    from mcmc_ref_hip import _ffi
    C, N, P = 4, 50, 3
    x = np.zeros((P, 1, N))
    F = _ffi.MCR_F64
    assert _ffi.tensor_args(np.broadcast_to(x, (P, C, N)), "pcn") == (F, C, N, P, 0, 1, N)        # identical chains
    y = np.zeros((1, C, N))
    assert _ffi.tensor_args(np.broadcast_to(y, (P, C, N)), "pcn") == (F, C, N, P, N, 1, 0)        # aliased parameters
    z = np.zeros((C, 1, P))
    assert _ffi.tensor_args(np.broadcast_to(z, (C, N, P)), "cnp") == (F, C, N, P, P, 0, 1)        # constant chains
    w = np.zeros(1)
    assert _ffi.tensor_args(as_strided(w, (C, N, P), (0, 0, 0)), "cnp") == (F, C, N, P, 0, 0, 0)


def test_tensor_args_rejects_negative_strides_and_bad_arguments():
    from mcmc_ref_hip import _ffi
    x = np.zeros((4, 10, 3))
    for v in (x[:, ::-1, :], x[::-1], x[..., ::-1], x[::-1, ::-1, ::-1]):
        with pytest.raises(ValueError, match="negative"):
            _ffi.tensor_args(v, "cnp")
    with pytest.raises(ValueError):
        _ffi.tensor_args(x[0], "cn")
    with pytest.raises(ValueError):
        _ffi.tensor_args(x, "ccn")
    with pytest.raises(TypeError):
        _ffi.tensor_args(x.astype(np.float16), "cnp")
