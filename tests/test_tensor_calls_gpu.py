"""What the five calls on one draw tensor share -- nested R-hat, Pareto k-hat, PSIS, HDI, autocorrelation -- through each
host and each device entry: a table over the ten entries, on 2 parameters x 8 chains x 64 draws (K = 2 superchains,
max_lag = 8, prob = 0.9).

* The refusals of the tensor, by raw ctypes: MCR_EINVAL with the one message, the caller's arrays as the caller filled
  them, and the next good call gives the bits of the first.  All of them are decided on the host from the arguments: no
  case hands over a bad pointer with an acceptable shape.  C = 4, N = 2^62 is the product that overflows int64.
* The two shapes beyond the limit through each mcr_*_plan: 0 parameters per chunk, MCR_OK.
* P == 0 and C * N == 0: MCR_OK, the documented fills, no launch.
* A short last chunk: 7 parameters, the workspace limit searched upward from its floor to an answer of
  *_params_per_chunk that does not divide 7, both entries against the unchunked bits (PSIS: the host entry with weights;
  nested: with the z table).  The limit has a floor of 1 MiB, and seven parameters of 4 096 pooled draws fit under it
  whole in every one of the calls (about 110 KB per parameter on the pooled order, a few KB in autocorrelation), so the
  chains of 512 draws are doubled until seven no longer fit at the floor: 8 x 1024, and 8 x 131 072 for autocorrelation.
* Alternation on one context, nested -> PSIS -> HDI -> autocorrelation -> Pareto -> nested: each call's bits are those
  of a fresh context (the context's two call buffers carry nothing from one call into the next).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CALLS = ("nested_rhat", "pareto_khat", "psis", "hdi", "autocorr")
LAG = 8
FILL, IFILL = -1234.5, -1234                                  # what the caller's arrays hold before a call
IDS = np.repeat(np.arange(2, dtype=np.int32), 4)             # K = 2 superchains of 4 chains
PROB = np.array([0.9])
EXTRA = {"nested_rhat": (IDS.ctypes.data_as(C.POINTER(C.c_int32)),), "pareto_khat": (None,), "psis": (0, None, None),
         "hdi": (PROB.ctypes.data_as(C.POINTER(C.c_double)), 1), "autocorr": (LAG, 0, 5.0)}
PLAN_EXTRA = {"nested_rhat": (2,), "pareto_khat": (), "psis": (0,), "hdi": (1,), "autocorr": (LAG,)}
PLAN = {"nested_rhat": "mcr_nested_plan", "pareto_khat": "mcr_pareto_plan", "psis": "mcr_psis_plan", "hdi": "mcr_hdi_plan",
        "autocorr": "mcr_autocorr_plan"}
LAST_KERNEL = {"nested_rhat": "k_nested_combine", "pareto_khat": "k_pareto_fit", "psis": "k_psis_column", "hdi": "k_hdi_pick",
               "autocorr": "k_acf_pool"}                      # one launch per chunk
ENTRIES = pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
EACH_CALL = pytest.mark.parametrize("name", CALLS)


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ffi):
    """The context whose workspace limit the chunking test lowers."""
    c = ffi.Context(0)
    yield c
    c.close()


def tensor(P: int, N: int, seed: int = 7) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((P, 8, N))


@pytest.fixture(scope="module")
def x():
    return tensor(2, 64)


@pytest.fixture(scope="module")
def t(ctx, x):
    dev = ctx.upload(x)
    yield dev
    dev.free()


def outputs(ffi, name: str, P: int, nc: int, weights: int = 0):
    """The caller's arrays of a call on P parameters in nc chains, filled, and the struct that points at them."""
    n, c = max(P, 1), max(nc, 1)
    d = lambda *shape: np.full(shape, FILL)
    i = lambda *shape: np.full(shape, IFILL, dtype=np.int64)
    if name == "nested_rhat":
        arrs, struct = {k: d(n) for k in ffi.NESTED_FIELDS}, ffi.Nested
    elif name == "pareto_khat":
        arrs, struct = {"khat": d(n), "khat_left": d(n), "khat_right": d(n), "ndraws_tail": i(n)}, ffi.Pareto
    elif name == "psis":
        arrs, struct = {"khat": d(n), "ndraws_tail": i(n), "lppd": d(n), "elpd": d(n), "p_loo": d(n)}, ffi.Psis
        if weights:
            arrs["log_weights"] = d(weights)
    elif name == "hdi":
        arrs, struct = {"lo": d(n), "hi": d(n), "index": i(n)}, ffi.Hdi
    else:
        arrs, struct = {"acf": d(n, c, LAG + 1), "var": d(n, c), "tau": d(n, c), "window": i(n, c), "acf_pooled": d(n, LAG + 1),
                        "tau_pooled": d(n), "window_pooled": i(n)}, ffi.Acf
    ptr = lambda k, a: a.ctypes.data_as(C.c_void_p if k == "log_weights" else C.POINTER(C.c_int64 if a.dtype == np.int64 else C.c_double))
    return arrs, struct(**{k: ptr(k, a) for k, a in arrs.items()})


def untouched(arrs: dict) -> bool:
    return all((a == (IFILL if a.dtype == np.int64 else FILL)).all() for a in arrs.values())


def bits(arrs: dict) -> dict:
    return {k: (a if a.dtype == np.int64 else a.view(np.int64)).tolist() for k, a in arrs.items()}


def raw(c, name: str, host: bool, ptr, targs, out) -> int:
    fn = getattr(c.lib, f"mcr_{name}" if host else f"mcr_{name}_dev")
    return fn(c.handle, ptr, *targs, *EXTRA[name], None if out is None else C.byref(out))


def message(c) -> str:
    return (c.lib.mcr_last_error(c.handle) or b"").decode()


def entry_args(ffi, host: bool, x: np.ndarray, t):
    return (x.ctypes.data_as(C.c_void_p), ffi.tensor_args(x, "pcn")) if host else (t.buf.ptr, t.targs)


def good(c, ffi, name: str, host: bool, x: np.ndarray, t, weights: bool = False) -> dict:
    """The bits of every output of a call that has to succeed."""
    ptr, targs = entry_args(ffi, host, x, t)
    arrs, out = outputs(ffi, name, targs[3], targs[1], x.size if weights else 0)
    rc = raw(c, name, host, ptr, targs, out)
    assert rc == ffi.MCR_OK, (name, host, rc, message(c))
    assert not (arrs[next(iter(arrs))] == FILL).any(), (name, host)
    return bits(arrs)


# ---- the refusals every entry shares -------------------------------------------------------------------------------------

OVER = ((1, 2 ** 31 - 1), (4, 2 ** 62))                      # C * N = 2^31 - 1; a product that overflows


@EACH_CALL
@ENTRIES
def test_shared_refusals(ctx, ffi, x, t, name, host):
    first = good(ctx, ffi, name, host, x, t)
    ptr, targs = entry_args(ffi, host, x, t)
    dtype, nc, N, P, sc, sn, sp = targs
    cases = [("out is NULL", ptr, targs, False),
             ("unsupported dtype 7", ptr, (7, nc, N, P, sc, sn, sp), True),
             ("negative dimension", ptr, (dtype, nc, -1, P, sc, sn, sp), True),
             ("negative strides are not supported", ptr, (dtype, nc, N, P, sc, -sn, sp), True),
             ("draws is NULL", None, targs, True)]
    cases += [("C*N must be < 2^31 - 1", ptr, (dtype, c_, n_, P, sc, sn, sp), True) for c_, n_ in OVER]
    for text, p, bad, with_out in cases:
        arrs, out = outputs(ffi, name, P, nc)
        rc = raw(ctx, name, host, p, bad, out if with_out else None)
        print(name, "host" if host else "device", bad, "->", rc, message(ctx))
        assert rc == ffi.MCR_EINVAL, (text, bad, rc)
        assert text in message(ctx), (text, message(ctx))
        assert untouched(arrs), (text, arrs)
        assert good(ctx, ffi, name, host, x, t) == first, text


@EACH_CALL
def test_plans_answer_zero_beyond_the_limit(ctx, ffi, t, name):
    dtype, _, _, P, sc, sn, sp = t.targs
    for c_, n_ in OVER:
        v = C.c_int64(99)
        rc = getattr(ctx.lib, PLAN[name])(ctx.handle, dtype, c_, n_, P, sc, sn, sp, *PLAN_EXTRA[name], C.byref(v))
        assert rc == ffi.MCR_OK and v.value == 0, (name, c_, n_, rc, v.value, message(ctx))


# ---- empty tensors ----------------------------------------------------------------------------------------------------------

@EACH_CALL
@ENTRIES
def test_empty_tensors(ctx, ffi, t, name, host):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for shape in ((0, 8, 64), (2, 8, 0)):                # P == 0; C * N == 0
            e = np.empty(shape)
            ptr, targs = (e.ctypes.data_as(C.c_void_p) if host else t.buf.ptr), ffi.tensor_args(e, "pcn")
            arrs, out = outputs(ffi, name, shape[0], 8)
            rc = raw(ctx, name, host, ptr, targs, out)
            assert rc == ffi.MCR_OK, (shape, rc, message(ctx))
            if shape[0] == 0:
                assert untouched(arrs), arrs
                continue
            for k, a in arrs.items():                         # NaN, no tail, no index, no window
                if a.dtype == np.int64:
                    assert (a == (0 if k == "ndraws_tail" else -1)).all(), (k, a)
                else:
                    assert np.isnan(a).all(), (k, a)
        assert all(v["launches"] == 0 for v in ctx.profile_get().values()), ctx.profile_get()
    finally:
        ctx.profile(False)


# ---- a short last chunk -------------------------------------------------------------------------------------------------------

P7 = 7


def params_per_chunk(c, name: str, ts, host_weights: bool) -> int:
    if name == "nested_rhat":
        return c.nested_params_per_chunk(ts, 2)
    if name == "psis":
        return c.psis_params_per_chunk(ts, host_weights)
    if name == "hdi":
        return c.hdi_params_per_chunk(ts, 1)
    return c.autocorr_params_per_chunk(ts, LAG) if name == "autocorr" else c.pareto_params_per_chunk(ts)


def short_last_chunk(small, ffi, name: str, host_weights: bool):
    """(draws per chain, parameters per chunk) with the limit of `small` set so that the last chunk of seven is short."""
    floor = 1 << 20
    nothing = ffi.DeviceBuffer(small, 8)                      # (a plan reads no draws)
    try:
        for N in (512 << k for k in range(14)):
            shape = ffi.DeviceTensor(small, nothing, (ffi.MCR_F64, 8, N, P7, N, 1, 8 * N))
            for limit in range(floor, 64 * floor, 64 << 10):
                small._check(small.lib.mcr_set_workspace_limit(small.handle, limit))
                try:
                    per = params_per_chunk(small, name, shape, host_weights)
                except ffi.McrError:
                    continue                                  # not one parameter fits yet
                if per == P7:
                    break                                     # seven fit whole at the floor: longer chains
                if P7 % per:
                    return N, per
    finally:
        nothing.free()
    raise AssertionError(f"{name}: no limit cuts {P7} parameters into chunks with a short last one")


@EACH_CALL
@ENTRIES
def test_short_last_chunk(ctx, small, ffi, name, host):
    weights = host and name == "psis"
    N, per = short_last_chunk(small, ffi, name, weights)
    print(name, "host" if host else "device", "draws per chain", N, "parameters per chunk", per)
    x7 = tensor(P7, N, seed=11)
    whole, ts = ctx.upload(x7), small.upload(x7)
    try:
        assert params_per_chunk(ctx, name, whole, weights) == P7
        base = good(ctx, ffi, name, host, x7, whole, weights)
        assert params_per_chunk(small, name, ts, weights) == per
        small.profile(True)
        small.profile_reset()
        got = good(small, ffi, name, host, x7, ts, weights)
        launches = small.profile_get()[LAST_KERNEL[name]]["launches"]
        small.profile(False)
        assert launches == -(-P7 // per), (launches, per)
        assert got == base
    finally:
        whole.free()
        ts.free()


# ---- one context, one call after another -----------------------------------------------------------------------------------------

@ENTRIES
def test_alternation_on_one_context(ffi, x, host):
    order = ("nested_rhat", "psis", "hdi", "autocorr", "pareto_khat", "nested_rhat")
    fresh = {}
    for name in set(order):
        with ffi.Context(0) as c:
            tc = c.upload(x)
            fresh[name] = good(c, ffi, name, host, x, tc, weights=host)
            tc.free()
    with ffi.Context(0) as c:
        tc = c.upload(x)
        for name in order:
            assert good(c, ffi, name, host, x, tc, weights=host) == fresh[name], name
        tc.free()
