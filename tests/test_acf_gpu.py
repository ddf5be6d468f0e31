"""Autocorrelation functions and times on the GPU (mcr_autocorr, mcr_autocorr_dev, k_acf_mean, k_acf_products, k_acf_finish,
k_acf_pool).

* Accuracy: every output of every case against tests/test_acf_refs_cpu.py's long-double reference under the standing gate
  |got - ref| <= 1e-9 * max(1, |ref|), NaN exactly, `window` as an integer (`gate` first asserts the reference's margin
  |W - window_c tau_W| > 1e-6, so no integer hinges on rounding).  The worst error is printed.  Every case is also compared
  IN BITS with mcr_autocorr_host.
* Shapes: the smallest at which a path changes.  B = MCR_ACF_BLOCK = 512 draws per fma chain; a thread owns 4 lags, a wave
  256, a workgroup 1024 (one lag group); a workgroup takes 8, 4, 2 or 1 draw blocks as the lags need up to 32, 64, 128 or
  more quads of 4.
* One answer on every route, errors that leave the context usable, empty shapes, the Python functions, the command, and
  the kernels that run.

Worst error measured on an MI355X over all cases below: 1.9e-15, and 1.9e-11 where the draws are offset by 1e6 (x - m itself
carries 1e-10 relative there); the gate is 1e-9.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

from test_acf_refs_cpu import FLOAT_KEYS, ar1, gate, one

pytestmark = pytest.mark.gpu

B = 512                                                      # MCR_ACF_BLOCK
KEYS = FLOAT_KEYS + ("window", "window_pooled")


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    assert _ffi.MCR_ACF_BLOCK == B
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()


def bits(res: dict, p=None) -> dict:
    """The outputs (of parameter p, or of all) as integers: floats by their bit patterns."""
    out = {}
    for k in KEYS:
        a = np.asarray(res[k] if p is None else res[k][p])
        out[k] = (np.ascontiguousarray(a, dtype=np.float64).view(np.int64) if a.dtype.kind == "f" else a).tolist()
    return out


def check(ctx, ffi, x3, L, unbiased=False, wc=5.0, what=None) -> float:
    """ctx.autocorr of x3[P][C][N] against the reference and, in bits, against the host routine.  The worst float error."""
    got = ctx.autocorr(x3, "pcn", max_lag=L, unbiased=unbiased, window_c=wc)
    P, nc, N = x3.shape
    assert got["max_lag"] == L and got["acf"].shape == (P, nc, L + 1) and got["acf_pooled"].shape == (P, L + 1)
    worst_err = 0.0
    for p in range(P):
        worst_err = max(worst_err, gate(one(got, p), x3[p], L, unbiased, wc, (what, p)))
        host = ffi.autocorr_host(x3[p], max_lag=L, unbiased=unbiased, window_c=wc)
        assert bits(got, p) == bits(host, 0), (what, p)
    with np.errstate(all="ignore"):
        assert np.array_equal(got["ess_chain"], N / got["tau"], equal_nan=True)
        assert np.array_equal(got["ess_pooled"], nc * N / got["tau_pooled"], equal_nan=True)
    print(f"acf worst error {what}: {worst_err:.3e}")
    return worst_err


# ---- against the reference ---------------------------------------------------------------------------------------------------

SHAPES = [  # (C, N, L)
    (2, 1, 0), (2, 2, 0), (2, 2, 1), (3, 3, 0), (3, 3, 2),                        # N edges, L = 0, L = N - 1
    (2, B - 1, 37), (2, B, 37), (2, B + 1, 37), (2, B + 37, 37), (3, 2 * B + 1, 37),     # draw-block edges (odd N: rows off 16 bytes)
    (2, 700, 2), (2, 700, 3), (2, 700, 4),                                       # the lags of a thread: 4
    (1, 4100, 127), (1, 4100, 128),                                               # 32 | 33 quads: 8 | 4 draw blocks per workgroup
    (2, 2100, 255), (2, 2100, 256),                                               # the lags of a wave (256): 4 | 2 draw blocks
    (2, 1100, 511), (2, 1100, 512),                                               # 128 | 129 quads: 2 | 1 draw blocks
    (2, 1500, 1022), (2, 1500, 1023), (2, 1500, 1024),                           # the lags of a workgroup (1024): 1 | 2 lag groups
    (1, 1537, 1536),                                                              # L = N - 1 over three blocks and two lag groups
    (1, 4100, 4096),                                                              # MCR_ACF_MAX_LAG at a short N just above it
    (1000, 20, 19),                                                               # many short chains
]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"C{c}-N{n}-L{l}" for c, n, l in SHAPES])
def test_shapes_against_the_reference(ctx, ffi, shape):
    nc, N, L = shape
    x3 = np.stack([ar1(0.6, nc, N, seed=100 + N + L), ar1(0.2, nc, N, seed=200 + N + L, offset=-2.0)])
    check(ctx, ffi, x3, L, what=shape)


def test_decay_window_constants_and_the_unbiased_form(ctx, ffi):
    """phi in {0, 0.5, 0.9, 0.99}: found and missing windows in one call; window_c in {1, 5, 10}; both divisors."""
    x3 = np.stack([ar1(phi, 3, 2001, seed=40 + i) for i, phi in enumerate((0.0, 0.5, 0.9, 0.99))])
    seen = set()
    for wc in (1.0, 5.0, 10.0):
        for unbiased in (False, True):
            check(ctx, ffi, x3, 100, unbiased, wc, what=("decay", wc, unbiased))
        seen |= set(ctx.autocorr(x3, "pcn", max_lag=100, window_c=wc)["window"].reshape(-1).tolist())
    assert -1 in seen and any(w >= 0 for w in seen)
    r5 = ctx.autocorr(x3, "pcn", max_lag=100)
    assert (r5["window"][1] >= 0).all() and (r5["window"][3] == -1).all()           # phi = 0.5 decays, phi = 0.99 does not
    x3 = np.stack([ar1(0.5, 2, 40, seed=3), ar1(0.9, 2, 40, seed=4)])                # the unbiased form at l = N - 1: divisor 1
    check(ctx, ffi, x3, 39, True, 5.0, what="unbiased to N - 1")
    u = ctx.autocorr(x3, "pcn", max_lag=39, unbiased=True)
    d = x3 - x3.mean(axis=2, keepdims=True)
    assert np.allclose(u["acf"][:, :, 39] * u["var"], d[:, :, 0] * d[:, :, 39], rtol=1e-9)


def test_the_mean_is_taken_first(ctx, ffi):
    """Draws offset by 1e6: sums of x_i x_{i+l} minus N m^2 would lose ten digits and miss the gate."""
    x3 = np.stack([ar1(0.5, 2, 1301, seed=8, offset=1e6), ar1(0.8, 2, 1301, seed=9, offset=-1e6, scale=0.01)])
    check(ctx, ffi, x3, 64, what="offset 1e6")


def test_constant_chains(ctx, ffi):
    x3 = np.stack([ar1(0.4, 3, 600, seed=5), ar1(0.4, 3, 600, seed=6)])
    x3[0, 1] = 2.5                                                              # a constant chain among varying ones
    x3[1] = np.array([1.0, -3.0, 7.5])[:, None]                                 # every chain of a parameter constant
    check(ctx, ffi, x3, 50, what="constant")
    r = ctx.autocorr(x3, "pcn", max_lag=50)
    assert np.isnan(r["acf"][0, 1]).all() and np.isnan(r["tau"][0, 1]) and r["window"][0, 1] == -1 and r["var"][0, 1] == 0.0
    assert np.isfinite(r["acf"][0, [0, 2]]).all() and np.isfinite(r["acf_pooled"][0]).all() and r["window_pooled"][0] >= 0
    assert np.isnan(r["acf"][1]).all() and np.isnan(r["acf_pooled"][1]).all() and np.isnan(r["tau_pooled"][1])
    assert r["window_pooled"][1] == -1 and np.isnan(r["ess_pooled"][1])


# ---- one answer on every route ------------------------------------------------------------------------------------------------

def test_one_answer_on_every_route(ctx, ffi):
    P, nc, N, L = 9, 4, 4201, 1030                                              # odd N: later chains' rows are off 16 bytes
    x3 = np.stack([ar1(0.3 + 0.07 * p, nc, N, seed=60 + p, offset=float(p)) for p in range(P)])
    got = ctx.autocorr(x3, "pcn", max_lag=L)
    gate(one(got, 4), x3[4], L, False, 5.0, "routes")
    base = bits(got)
    for p in (0, 3, 8):                                                         # alone, and against the host routine
        assert bits(ctx.autocorr(x3[p:p + 1], "pcn", max_lag=L), 0) == bits(got, p), p
    assert bits(ffi.autocorr_host(x3[5], max_lag=L), 0) == bits(got, 5)
    rev = ctx.autocorr(np.ascontiguousarray(x3[::-1]), "pcn", max_lag=L)        # every other place in the batch
    assert all(bits(rev, P - 1 - p) == bits(got, p) for p in range(P))
    cnp = np.ascontiguousarray(x3.transpose(1, 2, 0))                           # the default layout: the ingest pass
    assert bits(ctx.autocorr(cnp, max_lag=L)) == base
    wide = np.zeros((P, nc, 2 * N))                                             # a strided view: every other draw of a wider array
    wide[:, :, ::2] = x3
    assert bits(ctx.autocorr(wide[:, :, ::2], "pcn", max_lag=L)) == base
    t = ctx.upload(x3)
    try:
        assert bits(ctx.autocorr(t, max_lag=L)) == base                         # device entry
        assert ctx.autocorr_params_per_chunk(t, L) == P
    finally:
        t.free()
    with ffi.Context(0) as small:                                               # 1, 2 and 3 workspace chunks
        ts = small.upload(x3)
        limits = {}
        for mib in range(1, 8):                                                 # (a parameter needs ~0.33 MiB)
            small._check(small.lib.mcr_set_workspace_limit(small.handle, mib << 20))
            limits.setdefault(-(-P // small.autocorr_params_per_chunk(ts, L)), mib)
        assert {1, 2, 3} <= set(limits), limits
        small.profile(True)
        for chunks in (1, 2, 3):
            small._check(small.lib.mcr_set_workspace_limit(small.handle, limits[chunks] << 20))
            small.profile_reset()
            assert bits(small.autocorr(ts, max_lag=L)) == base, chunks
            prof = small.profile_get()
            assert all(prof[k]["launches"] == chunks for k in ("k_acf_mean", "k_acf_products", "k_acf_finish", "k_acf_pool")), prof
        small.profile(False)
        assert bits(small.autocorr(x3, "pcn", max_lag=L)) == base               # the host entry in chunks
        assert bits(small.autocorr(cnp, max_lag=L)) == base                     # ... and through the ingest pass
        ts.free()


def test_f32_is_the_f64_call_on_the_widened_tensor(ctx):
    x32 = np.stack([ar1(0.5, 3, 1101, seed=70), ar1(0.9, 3, 1101, seed=71, offset=5.0)]).astype(np.float32)
    want = bits(ctx.autocorr(x32.astype(np.float64), "pcn", max_lag=200))
    assert bits(ctx.autocorr(x32, "pcn", max_lag=200)) == want
    assert bits(ctx.autocorr(np.ascontiguousarray(x32.transpose(1, 2, 0)), max_lag=200)) == want
    t = ctx.upload(x32)
    try:
        assert bits(ctx.autocorr(t, max_lag=200)) == want
    finally:
        t.free()


def test_only_the_new_kernels_run(ctx):
    x3 = np.stack([ar1(0.5, 4, 3000, seed=80 + p) for p in range(3)])
    ctx.profile(True)
    ctx.profile_reset()
    ctx.autocorr(x3, "pcn", max_lag=100)
    prof = ctx.profile_get()
    ctx.profile_reset()
    ctx.autocorr(np.ascontiguousarray(x3.transpose(1, 2, 0)), max_lag=100)
    prof_cnp = ctx.profile_get()
    ctx.profile(False)
    new = {"k_acf_mean", "k_acf_products", "k_acf_finish", "k_acf_pool"}
    assert {k for k, v in prof.items() if v["launches"]} == new, prof
    assert all(prof[k]["launches"] == 1 for k in new)
    assert {k for k, v in prof_cnp.items() if v["launches"]} == new | {"k_ingest"}, prof_cnp


# ---- errors and empty shapes ---------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(ctx, ffi):
    x3 = np.stack([ar1(0.5, 4, 300, seed=90), ar1(0.7, 4, 300, seed=91)])
    base = bits(ctx.autocorr(x3, "pcn", max_lag=40))

    def refused(match, code=None, draws=x3, **kw):
        kw = {"max_lag": 40, **kw}
        with pytest.raises(ffi.McrError, match=match) as e:
            ctx.autocorr(draws, "pcn", **kw)
        assert e.value.code == (ffi.MCR_EINVAL if code is None else code)
        with pytest.raises(ValueError, match=match):                            # what diagnostics / convert / the command raise
            with ffi.value_errors():
                ctx.autocorr(draws, "pcn", **kw)
        assert bits(ctx.autocorr(x3, "pcn", max_lag=40)) == base                # a good call afterwards

    bad = x3.copy()
    for v in (np.nan, np.inf, -np.inf):
        bad[1, 1, 7] = v
        refused("non-finite", ffi.MCR_ENONFINITE, draws=bad)
    refused("max_lag = -1", max_lag=-1)
    refused("exceeds N - 1", max_lag=300)
    refused("MCR_ACF_MAX_LAG", max_lag=ffi.MCR_ACF_MAX_LAG + 1)
    for wc in (0.0, -5.0, float("nan"), float("inf")):
        refused("window_c", window_c=wc)
    out_arrs, out = ffi._acf_arrays(2, 4, 40)
    ptr, targs = x3.ctypes.data_as(C.c_void_p), list(ffi.tensor_args(x3, "pcn"))
    t = ctx.upload(x3)
    try:
        for fn, p in ((ctx.lib.mcr_autocorr, ptr), (ctx.lib.mcr_autocorr_dev, t.buf.ptr)):
            with pytest.raises(ffi.McrError, match="unknown flag bits") as e:
                ctx._check(fn(ctx.handle, p, *targs, 40, 6, 5.0, C.byref(out)))
            assert e.value.code == ffi.MCR_EINVAL
            neg = list(targs)
            neg[5] = -neg[5]                                                    # a negative draw stride
            with pytest.raises(ffi.McrError, match="negative strides"):
                ctx._check(fn(ctx.handle, p, *neg, 40, 0, 5.0, C.byref(out)))
            neg = list(targs)
            neg[2] = -1                                                         # a negative dimension
            with pytest.raises(ffi.McrError, match="negative dimension"):
                ctx._check(fn(ctx.handle, p, *neg, 40, 0, 5.0, C.byref(out)))
        assert np.isnan(out_arrs["acf"]).all()                                  # (rejected before anything is written)
        ctx.enqueue(t)                                                          # a summary in flight
        with pytest.raises(ffi.McrError, match="summaries in flight") as e:
            ctx.autocorr(t, max_lag=40)
        assert e.value.code == ffi.MCR_EINVAL
        ctx.wait()
        assert bits(ctx.autocorr(t, max_lag=40)) == base
    finally:
        t.free()


def test_empty_shapes_and_the_default_lag(ctx):
    r = ctx.autocorr(np.empty((2, 3, 0)), "pcn", max_lag=4)                     # no draws: NaN and -1
    assert r["acf"].shape == (2, 3, 5) and np.isnan(r["acf"]).all() and (r["window"] == -1).all()
    assert np.isnan(r["acf_pooled"]).all() and (r["window_pooled"] == -1).all() and np.isnan(r["tau_pooled"]).all()
    r = ctx.autocorr(np.empty((2, 0, 5)), "pcn", max_lag=4)                     # no chains
    assert r["acf"].shape == (2, 0, 5) and np.isnan(r["acf_pooled"]).all() and (r["window_pooled"] == -1).all()
    r = ctx.autocorr(np.empty((0, 3, 10)), "pcn")                               # no parameters
    assert r["acf"].shape == (0, 3, 10) and r["tau_pooled"].shape == (0,) and r["max_lag"] == 9
    assert ctx.autocorr(ar1(0.5, 2, 250, seed=1)[None], "pcn")["max_lag"] == 100
    assert ctx.autocorr(ar1(0.5, 2, 50, seed=1)[None], "pcn")["max_lag"] == 49


# ---- Python and the command ------------------------------------------------------------------------------------------------------

def test_python_functions_and_the_command(ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli, diagnostics
    from mcmc_ref_hip.convert import autocorr_file
    x = np.stack([ar1(0.5, 3, 400, seed=21), ar1(0.95, 3, 400, seed=22)])       # [P][C][N]
    want = ctx.autocorr(x, "pcn", max_lag=60)
    d = diagnostics.autocorr([c.tolist() for c in x[1]], 60, context=ctx)
    for k in ("acf", "var", "tau", "window", "ess_chain", "acf_pooled", "tau_pooled", "window_pooled", "ess_pooled"):
        assert np.array_equal(d[k], want[k][1], equal_nan=True), k
    assert d["max_lag"] == 60 and d["ess_pooled"] == 3 * 400 / d["tau_pooled"]
    assert diagnostics.autocorr([c.tolist() for c in x[0]], context=ctx)["max_lag"] == 100
    with pytest.raises(ValueError, match="equal length"):
        diagnostics.autocorr([[1.0, 2.0, 3.0], [1.0, 2.0]], context=ctx)
    with pytest.raises(ValueError, match="exceeds N - 1"):
        diagnostics.autocorr([c.tolist() for c in x[0]], 400, context=ctx)
    with pytest.raises(ValueError, match="non-finite"):
        diagnostics.autocorr([[1.0, float("nan"), 3.0]], 1, context=ctx)

    def write(path, lengths):
        with open(path, "w") as f:
            f.write("chain,draw,a,b\n")
            for c, n in enumerate(lengths):
                for i in range(n):
                    f.write(f"{c},{i},{float(x[0, c, i])!r},{float(x[1, c, i])!r}\n")
    csv = tmp_path / "draws.csv"
    write(csv, [400, 400, 400])
    got = autocorr_file(csv, max_lag=60, context=ctx)
    assert list(got) == ["a", "b"]
    for p, n in enumerate(("a", "b")):
        assert got[n]["acf"] == want["acf"][p].tolist() and got[n]["tau"] == want["tau"][p].tolist()
        assert got[n]["window"] == want["window"][p].tolist() and got[n]["tau_pooled"] == want["tau_pooled"][p]
        assert got[n]["ess_pooled"] == want["ess_pooled"][p] and got[n]["max_lag"] == 60
    assert list(autocorr_file(csv, params=["b"], max_lag=10, unbiased=True, window_c=2.0, context=ctx)) == ["b"]
    ragged = tmp_path / "ragged.csv"
    write(ragged, [400, 399, 400])
    with pytest.raises(ValueError, match="equal length"):
        autocorr_file(ragged, context=ctx)
    res = CliRunner().invoke(cli.main, ["autocorr", str(csv), "--max-lag", "60", "--format", "json"])
    assert res.exit_code == 0, res.output
    assert json.loads(res.output) == json.loads(json.dumps(got))
    res = CliRunner().invoke(cli.main, ["autocorr", str(csv), "--max-lag", "60"])
    assert res.exit_code == 0, res.output
    lines = res.output.splitlines()
    assert lines[0].split() == ["param", "tau", "window", "ess_pooled", "tau_min", "chain_min", "tau_max", "chain_max"]
    row = lines[2].split()                                                      # parameter b
    taus = want["tau"][1]
    assert row[0] == "b" and row[1] == f"{want['tau_pooled'][1]:.6g}" and row[2] == str(want["window_pooled"][1])
    assert row[4] == f"{taus.min():.6g}" and row[5] == str(int(taus.argmin())) and row[6] == f"{taus.max():.6g}" and row[7] == str(int(taus.argmax()))
    res = CliRunner().invoke(cli.main, ["autocorr", str(csv), "--params", "b", "--unbiased", "--window-c", "1", "--max-lag", "5"])
    assert res.exit_code == 0 and len(res.output.splitlines()) == 2
    res = CliRunner().invoke(cli.main, ["autocorr", str(ragged)])
    assert res.exit_code != 0 and "equal length" in res.output
    res = CliRunner().invoke(cli.main, ["autocorr", str(csv), "--params", "nope"])
    assert res.exit_code != 0 and "Unknown parameter" in res.output
    res = CliRunner().invoke(cli.main, ["autocorr", str(csv), "--window-c", "0"])
    assert res.exit_code != 0 and "window_c" in res.output
