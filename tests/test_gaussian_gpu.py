"""Dense Cholesky, lower solve and the joint Gaussian check on the GPU (include/mcmcref_hip_ext.h: mcrx_cholesky, mcrx_solve_lower,
mcrx_gaussian_check and their _dev forms; k_chol_panel, k_chol_below, k_chol_update, k_chol_finish, k_solve_lower,
k_sym_scale, k_row_mean, k_row_sumsq, k_gauss_sums).

The references, the derived bounds and the cases are those of tests/test_gaussian_refs_cpu.py (Higham's entrywise residual
bounds for any summation order; long double for the statistics; the logdet rule).  Shapes: around the wave, the MFMA tile
(16) and the block size NB = 64 -- one block, the first edge block, two and three block columns with an edge --, which is
where a tile, a mask or a trailing update can go wrong.  What the header promises in bits is asked in bits: the leading
minors, host against device entry, any row stride, any 8-byte alignment, repeated calls, profiling, a column alone
against the batch.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math

import numpy as np
import pytest

from test_gaussian_refs_cpu import (CONDS, GAUSS_CASES, KEYS, NB, bits, check_factor, check_statistics, defect_matrix, gauss_case,
                                    gaussian_reference, solve_residual_ratio, spd, stat_bits)

pytestmark = pytest.mark.gpu

CHOL_SIZES = (1, 2, 15, 16, 17, NB - 1, NB, NB + 1, 2 * NB - 1, 2 * NB, 2 * NB + 1, 3 * NB + 1)
NEW_KERNELS = {"k_chol_panel", "k_chol_below", "k_chol_update", "k_chol_finish", "k_solve_lower", "k_sym_scale", "k_row_sumsq",
               "k_gauss_sums", "k_row_mean"}
COV_KERNELS = {"k_moments", "k_moments_final", "k_cov_mfma", "k_cov_final"}


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def g():
    from mcmc_ref_hip import gaussian
    return gaussian


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()


class OnDevice:
    """A float64 array in device memory, its first element `shift` bytes past a 16-byte aligned allocation."""

    def __init__(self, ctx, x, shift=0):
        from mcmc_ref_hip import _ffi
        self.ctx, self.x = ctx, np.ascontiguousarray(x, dtype=np.float64)
        self.buf = _ffi.DeviceBuffer(ctx, self.x.nbytes + 16)
        assert self.buf.ptr.value % 16 == 0 and shift in (0, 8)
        self.addr = self.buf.ptr.value + shift
        ctx._check(ctx.lib.mcr_memcpy_h2d(ctx.handle, C.c_void_p(self.addr), self.x.ctypes.data_as(C.c_void_p), self.x.nbytes))

    def get(self) -> np.ndarray:
        out = np.empty_like(self.x)
        self.ctx._check(self.ctx.lib.mcr_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.addr), out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.buf.free()


@pytest.fixture(scope="module")
def big():
    """One matrix of order 3 NB + 1 and its device factor: the leading-minor tests share it."""
    return spd(3 * NB + 1, 1e3, seed=7)


# ---- Cholesky -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cond", CONDS)
def test_cholesky_shapes(ctx, g, cond):
    for P in CHOL_SIZES:
        A = spd(P, cond, seed=P)
        A[np.triu_indices(P, 1)] = np.nan                       # the strict upper triangle is not read
        L, info, logdet = g.cholesky(A, context=ctx)
        ratio = check_factor(np.tril(A) + np.tril(A, -1).T, L, info, logdet, (P, cond))
        print(f"P = {P} cond = {cond:g}: residual / bound = {ratio:.3f}")


def test_cholesky_leading_minors_in_bits(ctx, g, big):
    L = g.cholesky(big, context=ctx)[0]
    for n in CHOL_SIZES[:-1]:
        Ln, info, _ = g.cholesky(big[:n, :n], context=ctx)     # (a view: row stride 3 NB + 1)
        assert info == 0 and bits(Ln) == bits(L[:n, :n]), n


def test_cholesky_routes_in_bits(ctx, g, big):
    P = 2 * NB + 1
    A = np.ascontiguousarray(big[:P, :P])
    L, info, logdet = g.cholesky(A, context=ctx)
    want = (bits(L), info, bits(logdet))
    assert (bits(g.cholesky(A, context=ctx)[0])) == want[0]                                    # a second call
    padded = np.full((P, P + 3), np.nan)
    padded[:, :P] = A
    for arr, lda in ((A, P), (padded, P + 3)):
        for shift in (0, 8):
            with OnDevice(ctx, arr, shift) as d:
                i2, ld2 = g.cholesky_dev(d.addr, P, lda, context=ctx)
                got = d.get()
            assert (bits(got[:, :P]), i2, bits(ld2)) == want, (lda, shift)
            assert lda == P or np.isnan(got[:, P:]).all()                                      # the padding is not touched
    ctx.profile(True)
    try:
        ctx.profile_reset()
        L3, i3, ld3 = g.cholesky(A, context=ctx)
        prof = ctx.profile_get()
    finally:
        ctx.profile(False)
    assert (bits(L3), i3, bits(ld3)) == want
    nblk = -(-P // NB)
    assert {k: v["launches"] for k, v in prof.items()} == {"k_chol_panel": nblk, "k_chol_below": nblk - 1, "k_chol_update": nblk - 1,
                                                           "k_chol_finish": 1}


@pytest.mark.parametrize("kind", ["neg", "zero", "nan", "block"])
def test_cholesky_info(ctx, g, kind):
    P = 2 * NB + 5
    good = spd(P, 1e3, seed=11)
    want_good = bits(g.cholesky(good, context=ctx)[0])
    for k in (0, 1, NB - 1, NB, NB + 1, 2 * NB, P - 1):
        if kind == "block" and k == P - 1:
            continue
        A, want = defect_matrix(P, kind, k)
        L, info, logdet = g.cholesky(A, context=ctx)
        c = want - 1
        assert info == want and math.isnan(logdet), (kind, k, info, logdet)
        if c:
            Lc, ic, _ = g.cholesky(A[:c, :c], context=ctx)
            assert ic == 0 and bits(L[:c, :c]) == bits(Lc), (kind, k)
    assert bits(g.cholesky(good, context=ctx)[0]) == want_good                                 # the next call is right


def test_cholesky_nan_below_the_diagonal(ctx, g):
    P = 2 * NB + 5
    for i, j in ((20, 7), (NB + 3, 2), (P - 1, NB + 1), (2 * NB + 1, 2 * NB)):
        A = spd(P, 1e3, seed=11)
        A[i, j] = np.nan
        info = g.cholesky(A, context=ctx)[1]
        assert 1 <= info <= i + 1, (i, j, info)


# ---- lower solve ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", CHOL_SIZES)
@pytest.mark.parametrize("cond", CONDS)
def test_solve_lower(ctx, g, cond, P):
    rng = np.random.default_rng(9)
    L = np.linalg.cholesky(spd(P, cond, seed=P))
    noisy = L + np.triu(np.full((P, P), np.nan), 1)               # the strict upper triangle is not read
    for K in (1, 2, 63, 64, 65, 130):
        B = rng.standard_normal((P, K))
        X = g.solve_lower(noisy, B, context=ctx)
        ratio = solve_residual_ratio(L, X, B)
        assert ratio <= 1.0, (P, K, ratio)
        for col in {0, K - 1, K // 2}:
            assert bits(g.solve_lower(L, B[:, col], context=ctx)) == bits(X[:, col]), (P, K, col)
        padded = np.full((P, K + 5), np.nan)
        padded[:, :K] = B
        assert bits(g.solve_lower(L, padded[:, :K], context=ctx)) == bits(X), (P, K)


def test_solve_lower_device_entry(ctx, g):
    P, K = 2 * NB + 1, 65
    L = np.linalg.cholesky(spd(P, 1e3, seed=P))
    B = np.random.default_rng(2).standard_normal((P, K))
    X = g.solve_lower(L, B, context=ctx)
    padded = np.full((P, K + 3), np.nan)
    padded[:, :K] = B
    for shift in (0, 8):
        with OnDevice(ctx, L, shift) as dl, OnDevice(ctx, padded, 8 - shift) as db:
            g.solve_lower_dev(dl.addr, P, db.addr, K, ldb=K + 3, context=ctx)
            got = db.get()
        assert bits(got[:, :K]) == bits(X) and np.isnan(got[:, K:]).all()


# ---- the Gaussian check ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", GAUSS_CASES + ((1, 50, 40),), ids=str)
def test_gaussian_check_against_long_double(ctx, g, case):
    ref, act, scale, want = gauss_case(*case)
    got = g.gaussian_check(ref, act, scale=scale, shift=True, context=ctx)
    print({k: (got[k], want[k]) for k in KEYS})
    check_statistics(got, want, case)
    assert np.abs(got["shift"] - want["shift"]).max() <= 1e-9 * max(1.0, np.abs(want["shift"]).max())
    # one answer on every route
    P, Mr, Ma = case
    assert stat_bits(g.gaussian_check(ref, act, scale=scale, context=ctx)) == stat_bits(got)
    for shift in (0, 8):
        with OnDevice(ctx, ref, shift) as dr, OnDevice(ctx, act, 8 - shift) as da:
            dev = g.gaussian_check_dev(dr.addr, Mr, da.addr, Ma, P, scale=scale, shift=True, context=ctx)
        assert stat_bits(dev) == stat_bits(got) and bits(dev["shift"]) == bits(got["shift"]), shift


def test_gaussian_check_symmetries(ctx, g):
    ref, act, scale, _ = gauss_case(65, 1000, 700)
    one, two = g.gaussian_check(ref, act, context=ctx), g.gaussian_check(act, ref, context=ctx)
    for a, b in (("d2_ref", "d2_act"), ("trace_ref", "trace_act"), ("logdet_ref", "logdet_act"), ("kl_act_ref", "kl_ref_act")):
        assert bits(one[a]) == bits(two[b]) and bits(one[b]) == bits(two[a]), (a, b)
    same = g.gaussian_check(ref, ref, context=ctx)
    assert same["d2_ref"] == 0.0 and same["d2_act"] == 0.0 and abs(same["kl_sym"]) <= 1e-9 * 65
    # a zero in the scale against the call on the remaining rows: the covariance's split depends on P, so not in bits
    s = scale.copy()
    s[[0, 17, 64]] = 0.0
    keep = s > 0
    dropped = g.gaussian_check(ref, act, scale=s, shift=True, context=ctx)
    fewer = g.gaussian_check(ref[keep], act[keep], scale=s[keep], shift=True, context=ctx)
    assert dropped["p_live"] == fewer["p_live"] == 62
    for k in KEYS:
        assert abs(dropped[k] - fewer[k]) <= 1e-9 * max(abs(fewer[k]), 62), k
    assert np.abs(dropped["shift"] - fewer["shift"]).max() <= 1e-9
    ctx.profile(True)
    try:
        ctx.profile_reset()
        again = g.gaussian_check(ref, act, context=ctx)
        names = set(ctx.profile_get())
    finally:
        ctx.profile(False)
    assert stat_bits(again) == stat_bits(one)
    assert names <= NEW_KERNELS | COV_KERNELS and NEW_KERNELS <= names and {"k_cov_mfma", "k_cov_final"} <= names, names


def test_gaussian_check_singular_is_a_finding(ctx, g):
    ref, act, scale, _ = gauss_case(17, 400, 300)
    flat = ref.copy()
    flat[5] = 1.0                                                # a constant parameter: mean 1, every centred draw +0
    s = np.ones(17)
    s[2] = 0.0                                                   # ... at live index 4
    r = g.gaussian_check(flat, act, scale=s, shift=True, context=ctx)
    assert (r["p_live"], r["info_ref"], r["info_act"]) == (16, 5, 0), r
    assert all(math.isnan(r[k]) for k in ("d2_ref", "trace_ref", "trace_act", "logdet_ref", "kl_act_ref", "kl_ref_act", "mahalanobis"))
    assert math.isfinite(r["d2_act"]) and math.isfinite(r["logdet_act"]) and np.isnan(r["shift"]).all()
    want = gaussian_reference(flat, act, s, 1e-8)
    assert np.linalg.cond(want["C_act"]) <= 2e3
    r = g.gaussian_check(flat, act, scale=s, jitter=1e-8, context=ctx)
    assert r["info_ref"] == 0 and all(math.isfinite(r[k]) for k in KEYS), r
    mirrored = g.gaussian_check(act, flat, scale=s, context=ctx)
    assert (mirrored["info_ref"], mirrored["info_act"]) == (0, 5) and math.isfinite(mirrored["d2_ref"]) and math.isnan(mirrored["d2_act"])
    flat[5] = 3.7                                                # any constant: the mean is taken around the first draw
    assert g.gaussian_check(act, flat, context=ctx)["info_act"] == 6
    none = g.gaussian_check(ref, act, scale=np.zeros(17), shift=True, context=ctx)
    assert (none["p_live"], none["info_ref"], none["info_act"]) == (0, 0, 0) and all(math.isnan(none[k]) for k in KEYS)
    assert none["shift"].size == 0
    check_statistics(g.gaussian_check(ref, act, scale=scale, context=ctx), gauss_case(17, 400, 300)[3])


# ---- limits and errors ----------------------------------------------------------------------------------------------------

def test_workspace_limit(ctx, g, ffi):
    P, Mr, Ma = 129, 2000, 1500                                  # (a limit is at least 1 MiB: this shape carves more)
    ref, act, scale, _ = gauss_case(P, Mr, Ma)
    got = g.gaussian_check(ref, act, scale=scale, context=ctx)
    need = g.gaussian_workspace(Mr, Ma, P, context=ctx)
    assert need >= 3 * 8 * P * P and need > (1 << 20)
    with ffi.Context(0) as small:
        small._check(small.lib.mcr_set_workspace_limit(small.handle, need))
        assert g.gaussian_workspace(Mr, Ma, P, context=small) == need
        assert stat_bits(g.gaussian_check(ref, act, scale=scale, context=small)) == stat_bits(got)
        small._check(small.lib.mcr_set_workspace_limit(small.handle, need - 1))
        with pytest.raises(ffi.McrError) as exc:
            g.gaussian_check(ref, act, scale=scale, context=small)
        assert exc.value.code == ffi.MCR_ENOMEM and str(need) in exc.value.message, exc.value.message
        small._check(small.lib.mcr_set_workspace_limit(small.handle, 64 * need))
        assert stat_bits(g.gaussian_check(ref, act, scale=scale, context=small)) == stat_bits(got)


def test_errors_leave_the_context_usable(ctx, g, ffi):
    from mcmc_ref_hip import _xabi
    lib = _xabi.bind(ctx.lib)
    dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))
    ref, act, scale, want = gauss_case(2, 33, 47)
    out, info = np.full(8, -7.0), np.full(3, -7, dtype=np.int64)
    good = dict(ref=ref, Mr=33, act=act, Ma=47, P=2, scale=scale, jitter=0.0, out=out, info=info)

    def call(**kw):
        a = {**good, **kw}
        rc = lib.mcrx_gaussian_check(ctx.handle, dp(a["ref"]), a["Mr"], dp(a["act"]), a["Ma"], a["P"], dp(a["scale"]), a["jitter"],
                                     dp(a["out"]), None if a["info"] is None else a["info"].ctypes.data_as(C.POINTER(C.c_int64)), None)
        return rc, (ctx.lib.mcr_last_error(ctx.handle) or b"").decode()

    def bad(v, where, value):
        w = v.copy()
        w.flat[where] = value
        return w

    einval = [(dict(ref=None), "NULL"), (dict(act=None), "NULL"), (dict(out=None), "NULL"), (dict(info=None), "NULL"), (dict(Mr=0), "draw"),
              (dict(Ma=-1), "draw"), (dict(P=-1), "negative"), (dict(P=_xabi.MCRX_LINALG_MAX_P + 1), "MCRX_LINALG_MAX_P"),
              (dict(scale=bad(scale, 1, -0.5)), "scale[1]"), (dict(scale=bad(scale, 0, np.nan)), "scale[0]"),
              (dict(scale=bad(scale, 1, np.inf)), "scale[1]"), (dict(jitter=-1e-9), "jitter"), (dict(jitter=math.inf), "jitter"),
              (dict(jitter=math.nan), "jitter")]
    for kw, cause in einval:
        rc, msg = call(**kw)
        assert rc == ffi.MCR_EINVAL and cause in msg, (list(kw), rc, msg)
        assert np.all(out == -7.0) and np.all(info == -7)          # nothing was written
        assert call()[0] == ffi.MCR_OK
        check_statistics(dict(zip(KEYS, out)) | dict(zip(_xabi.GAUSSIAN_INFO_KEYS, info), mahalanobis=math.sqrt(out[0]), kl_sym=out[6] + out[7]), want)
        out[:] = -7.0
        info[:] = -7
    assert call(P=0)[0] == ffi.MCR_OK and np.all(out == -7.0) and np.all(info == -7)               # P == 0 writes nothing
    v = C.c_size_t(7)
    assert lib.mcrx_gaussian_workspace(ctx.handle, 0, 4, 2, C.byref(v)) == ffi.MCR_EINVAL
    assert lib.mcrx_gaussian_workspace(ctx.handle, 4, 4, 2, None) == ffi.MCR_EINVAL
    assert lib.mcrx_gaussian_workspace(ctx.handle, 4, 4, 0, C.byref(v)) == ffi.MCR_OK and v.value == 0
    # the factorisation and the solve
    A = spd(5, 1e3, seed=5)
    L = np.zeros((5, 5))
    i64, f64 = C.c_int64(-7), C.c_double(-7.0)
    chol = lambda a, P, lda, l: (lib.mcrx_cholesky(ctx.handle, dp(a), P, lda, dp(l), C.byref(i64), C.byref(f64)),
                                 (ctx.lib.mcr_last_error(ctx.handle) or b"").decode())
    for args, cause in (((None, 5, 5, L), "NULL"), ((A, 5, 5, None), "NULL"), ((A, -1, 5, L), "negative"), ((A, 5, 4, L), "lda"),
                        ((A, _xabi.MCRX_LINALG_MAX_P + 1, 1 << 20, L), "MCRX_LINALG_MAX_P")):
        rc, msg = chol(*args)
        assert rc == ffi.MCR_EINVAL and cause in msg and i64.value == -7 and not L.any(), (cause, rc, msg)
    assert chol(A, 0, 0, L)[0] == ffi.MCR_OK and (i64.value, f64.value) == (0, 0.0) and not L.any()
    B, X = np.ones((5, 3)), np.zeros((5, 3))
    solve = lambda l, P, ldl, b, K, ldb, x: (lib.mcrx_solve_lower(ctx.handle, dp(l), P, ldl, dp(b), K, ldb, dp(x)),
                                             (ctx.lib.mcr_last_error(ctx.handle) or b"").decode())
    for args, cause in (((None, 5, 5, B, 3, 3, X), "NULL"), ((A, 5, 5, None, 3, 3, X), "NULL"), ((A, 5, 5, B, 3, 3, None), "NULL"),
                        ((A, -1, 5, B, 3, 3, X), "negative"), ((A, 5, 5, B, -1, 3, X), "negative"), ((A, 5, 4, B, 3, 3, X), "ldl"),
                        ((A, 5, 5, B, 3, 2, X), "ldb"), ((A, _xabi.MCRX_LINALG_MAX_P + 1, 1 << 20, B, 3, 3, X), "MCRX_LINALG_MAX_P")):
        rc, msg = solve(*args)
        assert rc == ffi.MCR_EINVAL and cause in msg and not X.any(), (cause, rc, msg)
    assert solve(A, 0, 0, B, 3, 3, X)[0] == ffi.MCR_OK and solve(A, 5, 5, B, 0, 0, X)[0] == ffi.MCR_OK and not X.any()
    # summaries in flight
    t = ctx.upload(np.random.default_rng(0).normal(size=(2, 4, 100)), "pcn")
    try:
        ctx.enqueue(t)
        for rc, msg in (call(), chol(A, 5, 5, L), solve(A, 5, 5, B, 3, 3, X)):
            assert rc == ffi.MCR_EINVAL and "in flight" in msg, msg
        ctx.wait_one()
    finally:
        t.free()
    # the Python functions refuse what the library would
    for kw in (dict(scale=bad(scale, 0, -1.0)), dict(scale=scale[:1]), dict(jitter=-1.0), dict(jitter=math.nan)):
        with pytest.raises(ValueError):
            g.gaussian_check(ref, act, context=ctx, **kw)
    with pytest.raises(ValueError):
        g.gaussian_check(ref, act[:1], context=ctx)
    with pytest.raises(ValueError):
        g.cholesky(np.ones((3, 4)), context=ctx)
    with pytest.raises(ValueError):
        g.solve_lower(np.eye(3), np.ones((4, 2)), context=ctx)
    L5, i5, _ = g.cholesky(A, context=ctx)
    assert i5 == 0 and bits(L5) == bits(g.cholesky(A, context=ctx)[0])
    check_statistics(g.gaussian_check(ref, act, scale=scale, context=ctx), want)


# ---- validate() and the commands ------------------------------------------------------------------------------------------
# separation_case: unit marginals everywhere, correlation +0.9 in the reference and the control, -0.9 in the actual sample.
# Two Gaussians with these correlation matrices have tr(C_r^-1 C_a) = 3.62 / 0.19, so each KL is (19.05 - 2) / 2 = 8.5 and
# kl_sym 17; two samples of ~2000 draws from ONE Gaussian have a kl_sym of about (5 moments) (1 / Mr + 1 / Ma) = 0.005 and a
# squared Mahalanobis shift of about 2 (1 / Mr + 1 / Ma) = 0.002.  The thresholds 0.05 and 0.2 sit a factor of 10 (and 20 in
# the square) above the control's scale and a factor of 300 below the wrong correlation's.
KL_MAX, SHIFT_MAX = 0.05, 0.2


@pytest.fixture(scope="module")
def separation_store(tmp_path_factory):
    """A temporary store holding the reference of separation_case as model `corr` (4 chains of 500 draws), and the
    wrong-correlation and control samples as dicts and as CSV files; the reference also as a CSV file."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    from test_sliced_cpu import PARAMS, separation_case
    root = tmp_path_factory.mktemp("gaussian")
    (root / "draws").mkdir()
    (root / "meta").mkdir()
    ref, actual, control = separation_case()
    Cn, N = 4, ref.shape[1] // 4
    cols = {"chain": np.repeat(np.arange(Cn), N), "draw": np.tile(np.arange(N), Cn)}
    cols.update({p: ref[i] for i, p in enumerate(PARAMS)})
    pq.write_table(pa.table(cols), root / "draws" / "corr.draws.parquet")
    (root / "meta" / "corr.meta.json").write_text(json.dumps({"diagnostics": {}}))
    samples, files = {}, {}
    for name, x in (("actual", actual), ("control", control)):
        samples[name] = {p: [float(v) for v in x[i]] for i, p in enumerate(PARAMS)}
        files[name] = root / f"{name}.csv"
        files[name].write_text(",".join(PARAMS) + "\n" + "".join(f"{float(a)!r},{float(b)!r}\n" for a, b in zip(*x)))
    files["ref"] = root / "draws" / "corr.draws.parquet"
    return DataStore(local_root=root, packaged_root=root / "none"), root, samples, files


def test_validate_separates_a_wrong_correlation(separation_store, ctx):
    from mcmc_ref_hip import validate as validate_mod
    store, _, samples, _ = separation_store
    validate = lambda *a, **kw: validate_mod.validate(*a, metrics=("std",), store=store, context=ctx, **kw)
    plain = validate("corr", samples["actual"], ks_max=0.1)
    assert plain.passed and plain.gaussian is None and plain.gaussian_shift is None         # every marginal is right
    info = validate("corr", samples["actual"], ks_max=0.1, gaussian=True)
    assert info.passed and info.failures == plain.failures                                   # information only without a threshold
    assert type(plain) is validate_mod.ValidateResult and isinstance(info, validate_mod.GaussianValidateResult)
    assert all(getattr(info, f.name) == getattr(plain, f.name) for f in dataclasses.fields(validate_mod.ValidateResult))
    res = validate("corr", samples["actual"], ks_max=0.1, gaussian_kl_max=KL_MAX, gaussian_shift_max=10.0, gaussian=True)
    print(f"wrong correlation: {res.gaussian}")
    assert not res.passed and res.failures == [f"gaussian.kl={res.gaussian['kl_sym']:.3g} > {KL_MAX}"], res.failures
    assert 17.0 / 1.5 < res.gaussian["kl_sym"] < 17.0 * 1.5 and res.gaussian_shift == res.gaussian["mahalanobis"]
    assert set(res.gaussian["shift"]) == {"a", "b"} and res.gaussian["singular_ref"] is None and res.gaussian["singular_actual"] is None
    ok = validate("corr", samples["control"], ks_max=0.1, gaussian=True, gaussian_kl_max=KL_MAX, gaussian_shift_max=SHIFT_MAX)
    print(f"control: {ok.gaussian}")
    assert ok.passed and ok.gaussian["kl_sym"] < KL_MAX and ok.gaussian_shift < SHIFT_MAX
    shifted = {p: [v + 0.5 for v in vs] for p, vs in samples["control"].items()}
    moved = validate("corr", shifted, gaussian=True, gaussian_shift_max=SHIFT_MAX, tolerance=1e9)
    assert moved.failures == [f"gaussian.shift={moved.gaussian_shift:.3g} > {SHIFT_MAX}"] and moved.gaussian_shift > 0.4        # (0.5, 0.5) at correlation 0.9: sqrt(0.5 / 1.9) = 0.51
    # a constant parameter: reported by name, a failure only under a threshold
    flat = dict(samples["control"], b=[1.0] * len(samples["control"]["b"]))
    found = validate("corr", flat, gaussian=True, tolerance=1e9)
    assert found.passed and found.gaussian["singular_actual"] == "b" and found.gaussian["singular_ref"] is None
    assert math.isnan(found.gaussian["kl_sym"]) and math.isfinite(found.gaussian_shift)
    failed = validate("corr", flat, gaussian=True, tolerance=1e9, gaussian_kl_max=KL_MAX)
    assert failed.failures == [f"gaussian.kl=nan > {KL_MAX}"]
    with pytest.raises(ValueError, match="gaussian needs joint draws"):
        validate("corr", {"a": [0.0, 1.0, 2.0], "b": [0.0, 1.0]}, gaussian=True)


def test_commands(separation_store, monkeypatch):
    from click.testing import CliRunner
    from mcmc_ref_hip import store as store_mod
    from mcmc_ref_hip.cli import main
    _, root, _, files = separation_store
    monkeypatch.setenv("MCMC_REF_LOCAL_ROOT", str(root))
    monkeypatch.setattr(store_mod, "default_packaged_root", lambda: None)
    run = lambda *args: CliRunner().invoke(main, ["validate", "corr", "--metrics", "std", *args])
    out = run("--actual", str(files["actual"]))
    assert out.exit_code == 0 and out.output.splitlines() == ["passed"], out.output           # the text is unchanged
    doc = json.loads(run("--actual", str(files["actual"]), "--format", "json").output)
    assert "gaussian" not in doc and "gaussian_shift" not in doc                               # only when asked for
    out = run("--actual", str(files["actual"]), "--gaussian-kl-max", str(KL_MAX))             # implies --gaussian
    lines = out.output.splitlines()
    assert out.exit_code == 2 and lines[0] == "failed" and lines[1].startswith("- gaussian.kl=") and lines[2].startswith("gaussian shift"), out.output
    out = run("--actual", str(files["control"]), "--gaussian", "--gaussian-kl-max", str(KL_MAX), "--gaussian-shift-max", str(SHIFT_MAX),
              "--format", "json")
    doc = json.loads(out.output)
    assert out.exit_code == 0 and doc["passed"] is True and doc["gaussian_shift"] == doc["gaussian"]["mahalanobis"] < SHIFT_MAX
    assert doc["gaussian"]["kl_sym"] < KL_MAX and set(doc["gaussian"]["shift"]) == {"a", "b"}
    out = CliRunner().invoke(main, ["gaussian-check", str(files["ref"]), str(files["actual"]), "--format", "json"])
    assert out.exit_code == 0, out.output
    doc = json.loads(out.output)
    assert doc["params"] == ["a", "b"] and 17.0 / 1.5 < doc["kl_sym"] < 17.0 * 1.5 and doc["p_live"] == 2
    out = CliRunner().invoke(main, ["gaussian-check", str(files["ref"]), str(files["control"]), "--jitter", "1e-9"])
    assert out.exit_code == 0 and out.output.splitlines()[0].startswith("gaussian shift"), out.output
