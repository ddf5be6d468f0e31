"""Sliced two-sample KS / Wasserstein-1 (mcr_sliced_two_sample, mcr_sliced_two_sample_dev, k_project) on the GPU.

* The projection against an 80-bit reference, inside the derived bound gamma_{P+2} sum_p |W[k][p]| |X[p][m] - c[p]| (one
  rounded subtraction and a length-P fma chain), at shapes on both sides of every tile constant of k_project.
* The fixed summation order: the same bits whatever K is and wherever k stands, for a draws pointer 8 bytes past a 16-byte
  boundary, through the host and the device-resident entry, and under a workspace limit that forces direction chunks.
* The statistics are mcr_two_sample's on the projected rows: equal in bits to Context.two_sample of the downloaded
  projections, KS equal in bits to the exact rational, W1 inside w1_tolerance of the exact sum.
* Every error leaves the context usable.
* Separating power through validate() and the `validate` command: a sample with every marginal right and the correlation
  wrong passes the marginal thresholds and fails the sliced one (inputs pinned on the host by tests/test_sliced_cpu.py).
"""
from __future__ import annotations

import ctypes
import dataclasses
import json

import numpy as np
import pytest

from test_ext_refs_cpu import EPS, MERGE_TILE, exact_w1, expected_ks, two_sample_blocks, w1_tolerance
from test_sliced_cpu import PARAMS, SLICED_K, SLICED_SEED, separation_case

pytestmark = pytest.mark.gpu


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
def tiles(ffi):
    return ffi.MCR_PROJ_TILE_M, ffi.MCR_PROJ_TILE_K, ffi.MCR_PROJ_CHUNK_P


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def offset_case(P, Mr, Ma, K, seed):
    """Draws with a large common offset (1e6 + N(0, 1)) and a center near it, so that the subtraction matters;
    directions of mixed sign and scale."""
    rng = np.random.default_rng(seed)
    ref = 1e6 + rng.normal(size=(P, Mr))
    act = 1e6 + 0.5 + 1.5 * rng.normal(size=(P, Ma))
    center = 1e6 + rng.normal(size=P) * 0.25
    W = rng.normal(size=(K, P)) * 10.0 ** rng.integers(-2, 3, size=(K, 1))
    return ref, act, W, center


def longdouble_projection(X, W, c):
    """(sum_p W[k][p] (X[p][m] - c[p]), sum_p |W[k][p]| |X[p][m] - c[p]|) in np.longdouble, p by p."""
    ld = np.longdouble
    z = np.zeros((W.shape[0], X.shape[1]), dtype=ld)
    mag = np.zeros_like(z)
    for p in range(X.shape[0]):
        d = X[p].astype(ld) - ld(c[p])
        z += W[:, p].astype(ld)[:, None] * d[None, :]
        mag += np.abs(W[:, p]).astype(ld)[:, None] * np.abs(d)[None, :]
    return z, mag


def check_projection(ctx, P, Mr, Ma, K, seed):
    """One sliced call; returns the worst |err| / bound over both projections."""
    ref, act, W, center = offset_case(P, Mr, Ma, K, seed)
    ks, w1, zr, za = ctx.sliced_two_sample(ref, act, W, center, projections=True)
    assert zr.shape == (K, Mr) and za.shape == (K, Ma) and ks.shape == w1.shape == (K,)
    return max(projection_error(X, W, center, z, (P, Mr, Ma, K)) for X, z in ((ref, zr), (act, za)))


def projection_error(X, W, center, z, what=()) -> float:
    """The projected rows z [K][M] of X [P][M] inside the derived bound of the 80-bit reference; the worst |err| / bound
    (tests/call_families.py shares this gate)."""
    P = X.shape[0]
    gamma = (P + 2) * EPS / (1 - (P + 2) * EPS)
    want, mag = longdouble_projection(X, W, center)
    err, bound = np.abs(z.astype(np.longdouble) - want), gamma * mag
    bad = np.argwhere(~(err <= bound))
    assert len(bad) == 0, (*what, "first (k, m):", bad[:5])
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- the projection against an 80-bit reference ------------------------------------------------------------------------

def test_projection_along_the_draw_axis(ctx, tiles):
    TM, TK, CP = tiles
    Ms = [1, 2, 3, TM - 1, TM, TM + 1, 2 * TM + 1]
    for K, P in ((2, 3), (TK + 1, CP + 1)):
        for i, Mr in enumerate(Ms):
            Ma = Ms[(i + 3) % len(Ms)]                       # Mr != Ma, every size on both sides
            worst = check_projection(ctx, P, Mr, Ma, K, seed=100 + i)
            print(f"projection P={P} K={K} Mr={Mr} Ma={Ma}: worst |err| / bound = {worst:.3g}")


def test_projection_along_the_direction_axis(ctx, tiles):
    TM, TK, CP = tiles
    for Mr, Ma, P in ((3, 5, 2), (TM + 1, 2 * TM + 1, CP + 1)):
        for K in (1, TK - 1, TK, TK + 1, 2 * TK + 1):
            worst = check_projection(ctx, P, Mr, Ma, K, seed=200 + K)
            print(f"projection P={P} K={K} Mr={Mr} Ma={Ma}: worst |err| / bound = {worst:.3g}")


def test_projection_along_the_parameter_axis(ctx, tiles):
    TM, TK, CP = tiles
    for Mr, Ma, K in ((3, 2, 1), (TM + 1, TM, TK + 1)):
        for P in (1, 2, CP - 1, CP, CP + 1, 300):
            worst = check_projection(ctx, P, Mr, Ma, K, seed=300 + P)
            print(f"projection P={P} K={K} Mr={Mr} Ma={Ma}: worst |err| / bound = {worst:.3g}")


# ---- the fixed order ---------------------------------------------------------------------------------------------------

def test_a_direction_has_the_same_bits_alone_and_in_a_batch(ctx, tiles):
    TM, TK, CP = tiles
    K = 2 * TK + 1
    ref, act, W, center = offset_case(CP + 1, TM + 1, TM + 188, K, seed=1)
    ks, w1, zr, za = ctx.sliced_two_sample(ref, act, W, center, projections=True)
    for k in range(K):
        ks1, w11, zr1, za1 = ctx.sliced_two_sample(ref, act, W[k:k + 1], center, projections=True)
        assert np.array_equal(bits(zr1[0]), bits(zr[k])) and np.array_equal(bits(za1[0]), bits(za[k])), k
        assert bits(ks1)[0] == bits(ks)[k] and bits(w11)[0] == bits(w1)[k], k


class OnDevice:
    """x [P][M] f64 in device memory, its first element `shift` bytes past a 256-byte aligned allocation."""

    def __init__(self, ctx, x, shift=0):
        from mcmc_ref_hip import _ffi
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.buf = _ffi.DeviceBuffer(ctx, self.x.nbytes + 16)
        assert self.buf.ptr.value % 16 == 0 and shift in (0, 8)
        self.addr = self.buf.ptr.value + shift
        ctx._check(ctx.lib.mcr_memcpy_h2d(ctx.handle, ctypes.c_void_p(self.addr), self.x.ctypes.data_as(ctypes.c_void_p),
                                          self.x.nbytes))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.buf.free()


@pytest.mark.parametrize("Mr,Ma", [(1026, 700), (1025, 701), (1026, 701)])
def test_alignment_and_entry_do_not_change_a_bit(ctx, tiles, Mr, Ma):
    """Even and odd M through the host entry, the device entry on 16-byte aligned buffers (the 16-byte loads when M is
    even) and on buffers 8 bytes further (the 8-byte loads): the same bits."""
    TM, TK, CP = tiles
    P, K = CP + 3, TK + 2
    ref, act, W, center = offset_case(P, Mr, Ma, K, seed=Mr)
    host = ctx.sliced_two_sample(ref, act, W, center, projections=True)
    for sr, sa in ((0, 0), (8, 8), (0, 8)):
        with OnDevice(ctx, ref, sr) as dr, OnDevice(ctx, act, sa) as da:
            dev = ctx.sliced_two_sample_dev(dr.addr, Mr, da.addr, Ma, P, W, center, projections=True)
        for name, h, d in zip(("ks", "w1", "zr", "za"), host, dev):
            assert np.array_equal(bits(h), bits(d)), (name, sr, sa)
    ks2, w12 = ctx.sliced_two_sample(ref, act, W, center)
    assert np.array_equal(bits(ks2), bits(host[0])) and np.array_equal(bits(w12), bits(host[1]))
    zero_center = ctx.sliced_two_sample(ref, act, W, np.zeros(P), projections=True)
    no_center = ctx.sliced_two_sample(ref, act, W, None, projections=True)
    for z, n in zip(zero_center, no_center):
        assert np.array_equal(bits(z), bits(n))


def test_direction_chunks_do_not_change_a_bit(ctx, ffi, tiles):
    TM, TK, CP = tiles
    K, P, Mr, Ma = 2 * TK + 1, 5, 3000, 3001
    ref, act, W, center = offset_case(P, Mr, Ma, K, seed=7)
    assert ctx.sliced_dirs_per_chunk(Mr, Ma, P, K) == K
    whole = ctx.sliced_two_sample(ref, act, W, center, projections=True)
    with ffi.Context(0) as small:
        small._check(small.lib.mcr_set_workspace_limit(small.handle, 1 << 20))
        per = small.sliced_dirs_per_chunk(Mr, Ma, P, K)
        print(f"1 MiB workspace: {per} of {K} directions per chunk")
        assert 1 <= per and -(-K // per) >= 2
        chunked = small.sliced_two_sample(ref, act, W, center, projections=True)
    for name, a, b in zip(("ks", "w1", "zr", "za"), whole, chunked):
        assert np.array_equal(bits(a), bits(b)), name


# ---- the statistics ----------------------------------------------------------------------------------------------------

def check_statistics(ctx, ref, act, W, center, what):
    ks, w1, zr, za = ctx.sliced_two_sample(ref, act, W, center, projections=True)
    ks2, w12 = ctx.two_sample(zr, za)
    assert np.array_equal(bits(ks), bits(ks2)) and np.array_equal(bits(w1), bits(w12)), what
    for k in range(len(W)):
        assert ks[k] == expected_ks(zr[k], za[k]), (what, k)
        exact = exact_w1(zr[k], za[k])
        tol = w1_tolerance(zr[k], za[k], exact)
        err = abs(float(np.longdouble(w1[k]) - exact))
        print(f"{what} direction {k}: ks = {ks[k]:.6g}, w1 = {w1[k]:.6g}, |w1 err| / bound = {err / tol if tol else 0.0:.3g}")
        assert err <= tol, (what, k, err, tol)
    return ks, w1


@pytest.mark.parametrize("total", [MERGE_TILE - 1, MERGE_TILE, MERGE_TILE + 1])
def test_statistics_are_the_two_sample_pass_on_the_projections(ctx, total):
    Mr = 2000
    Ma = total - Mr
    assert two_sample_blocks(Mr, Ma) == (1 if total <= MERGE_TILE else 2)
    ref, act, W, center = offset_case(5, Mr, Ma, 3, seed=total)
    check_statistics(ctx, ref, act, W, center, f"pooled {total}")


def test_tied_and_constant_projections(ctx):
    rng = np.random.default_rng(11)
    Mr, Ma = 3000, 2500                                        # two merge blocks, runs of equal values across their boundary
    ref = np.stack([rng.integers(0, 10, size=Mr).astype(np.float64), rng.normal(size=Mr)])
    act = np.stack([rng.integers(2, 12, size=Ma).astype(np.float64), rng.normal(size=Ma)])
    W = np.array([[0.5, 0.0], [0.0, 0.0], [0.0, 1.0]])
    ks, w1 = check_statistics(ctx, ref, act, W, np.array([3.0, 0.0]), "ties")
    assert ks[1] == 0.0 and w1[1] == 0.0                       # the zero direction: both samples constant and equal
    assert 0.0 < ks[0] < 1.0 and w1[0] > 0.0


# ---- errors ------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(ctx, ffi):
    dp = lambda v: None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    P, K, Mr, Ma = 2, 3, 4, 5
    ref, act, W, center = offset_case(P, Mr, Ma, K, seed=3)
    ks, w1 = np.full(K, -7.0), np.full(K, -7.0)
    good = dict(ref=ref, Mr=Mr, act=act, Ma=Ma, P=P, dirs=W, center=center, K=K, ks=ks, w1=w1)

    def call(entry=None, **kw):
        a = {**good, **kw}
        rc = (entry or ctx.lib.mcr_sliced_two_sample)(ctx.handle, dp(a["ref"]), a["Mr"], dp(a["act"]), a["Ma"], a["P"],
                                                      dp(a["dirs"]), dp(a["center"]), a["K"], dp(a["ks"]), dp(a["w1"]),
                                                      None, None)
        return rc, (ctx.lib.mcr_last_error(ctx.handle) or b"").decode()

    def bad(v, where, value):
        out = v.copy()
        out.flat[where] = value
        return out

    einval = [dict(ref=None), dict(act=None), dict(dirs=None), dict(ks=None), dict(w1=None), dict(K=-1), dict(P=0),
              dict(P=-1), dict(Mr=0), dict(Ma=0), dict(K=65536), dict(Mr=2 ** 32 - 1), dict(Ma=2 ** 32 - 1),
              dict(Mr=94906266, Ma=94906266), dict(dirs=bad(W, 4, np.nan)), dict(dirs=bad(W, 5, np.inf)),
              dict(center=bad(center, 1, np.nan)), dict(center=bad(center, 0, -np.inf))]
    for kw in einval:
        rc, msg = call(**kw)
        assert rc == ffi.MCR_EINVAL and msg, (list(kw), rc, msg)
    assert call(K=0, Mr=0)[0] == ffi.MCR_EINVAL               # Mr < 1 is refused whatever K is
    assert np.all(ks == -7.0) and np.all(w1 == -7.0)          # nothing was written
    # summaries in flight
    t = ctx.upload(np.random.default_rng(0).normal(size=(2, 4, 100)), "pcn")
    try:
        ctx.enqueue(t)
        rc, msg = call()
        assert rc == ffi.MCR_EINVAL and "in flight" in msg
        ctx.wait_one()
    finally:
        t.free()
    # K == 0: fine, and nothing is written (even with NULL everywhere a direction would be needed)
    assert call(K=0)[0] == ffi.MCR_OK
    assert call(K=0, dirs=None, ks=None, w1=None, ref=None, act=None, P=0)[0] == ffi.MCR_OK
    assert np.all(ks == -7.0) and np.all(w1 == -7.0)
    k0, w0 = ctx.sliced_two_sample(ref, act, np.zeros((0, P)))
    assert k0.shape == w0.shape == (0,)
    # non-finite draws and an overflowing projection: seen by the sort's own count
    for kw in (dict(ref=bad(ref, 3, np.nan)), dict(act=bad(act, 7, np.inf)), dict(dirs=bad(W, 2, 1e308), center=None)):
        rc, msg = call(**kw)
        assert rc == ffi.MCR_ENONFINITE and "non-finite" in msg, (list(kw), rc, msg)
    with OnDevice(ctx, bad(ref, 0, np.nan)) as dr, OnDevice(ctx, act) as da:
        with pytest.raises(ffi.McrError) as exc:
            ctx.sliced_two_sample_dev(dr.addr, Mr, da.addr, Ma, P, W, center)
        assert exc.value.code == ffi.MCR_ENONFINITE
    # the Python method checks what Context.two_sample checks, with the same exceptions
    with pytest.raises(ValueError):
        ctx.sliced_two_sample(bad(ref, 0, np.nan), act, W)
    with pytest.raises(ValueError):
        ctx.sliced_two_sample(ref, act[:1], W)
    with pytest.raises(ValueError):
        ctx.sliced_two_sample(ref, act, W[:, :1])
    with pytest.raises(ValueError):
        ctx.sliced_two_sample(ref, act, W, center[:1])
    with pytest.raises(ValueError):
        ctx.sliced_two_sample(ref, act, bad(W, 0, np.nan))
    # one good call at the end
    rc, msg = call()
    assert rc == ffi.MCR_OK
    want = ctx.sliced_two_sample(ref, act, W, center)
    assert np.array_equal(bits(ks), bits(want[0])) and np.array_equal(bits(w1), bits(want[1]))
    assert np.all((0.0 <= ks) & (ks <= 1.0)) and np.all(w1 >= 0.0)


# ---- separating power, through validate() and the CLI --------------------------------------------------------------------

@pytest.fixture(scope="module")
def separation_store(tmp_path_factory):
    """A temporary store holding the reference of separation_case as model `corr` (4 chains of 500 draws), and the
    wrong-correlation and control samples as dicts and as CSV files."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    root = tmp_path_factory.mktemp("sliced")
    (root / "draws").mkdir()
    (root / "meta").mkdir()
    ref, actual, control = separation_case()
    C, N = 4, ref.shape[1] // 4
    cols = {"chain": np.repeat(np.arange(C), N), "draw": np.tile(np.arange(N), C)}
    cols.update({p: ref[i] for i, p in enumerate(PARAMS)})
    pq.write_table(pa.table(cols), root / "draws" / "corr.draws.parquet")
    (root / "meta" / "corr.meta.json").write_text(json.dumps({"diagnostics": {}}))
    samples, files = {}, {}
    for name, x in (("actual", actual), ("control", control)):
        samples[name] = {p: [float(v) for v in x[i]] for i, p in enumerate(PARAMS)}
        files[name] = root / f"{name}.csv"
        files[name].write_text(",".join(PARAMS) + "\n" + "".join(f"{float(a)!r},{float(b)!r}\n" for a, b in zip(*x)))
    return DataStore(local_root=root, packaged_root=root / "none"), root, samples, files


def test_validate_separates_a_wrong_correlation(separation_store):
    from mcmc_ref_hip import validate as validate_mod
    store, _, samples, _ = separation_store
    # The reference's gate is a RELATIVE error, and the means of separation_case are zero up to sampling noise, so their
    # relative error says nothing (1.9 here, for the control too): the gate is asked about the std alone.
    validate = lambda *a, **kw: validate_mod.validate(*a, metrics=("std",), **kw)
    wrong = validate("corr", samples["actual"], ks_max=0.1, store=store)
    assert wrong.passed and max(wrong.ks.values()) < 0.1                  # every marginal is right
    assert wrong.sliced_ks is None and wrong.sliced_w1 is None and wrong.sliced is None
    res = validate("corr", samples["actual"], ks_max=0.1, sliced=SLICED_K, sliced_seed=SLICED_SEED, sliced_ks_max=0.2,
                   store=store)
    print(f"wrong correlation: marginal ks {res.ks}, sliced ks {res.sliced_ks:.4g}, sliced w1 {res.sliced_w1:.4g}")
    assert max(res.ks.values()) < 0.1 and res.sliced_ks > 0.2
    assert not res.passed and [f for f in res.failures if f.startswith("sliced.ks=")] == res.failures
    s = res.sliced
    assert len(s["ks"]) == len(s["w1"]) == SLICED_K and s["ks"][s["worst"]] == res.sliced_ks == max(s["ks"])
    assert res.sliced_w1 == max(s["w1"])
    wa, wb = (s["worst_direction"][p] for p in PARAMS)
    assert wa * wb > 0 and 1 / 3 < abs(wa / wb) < 3                       # along a + b, where the two variances differ
    assert abs(np.hypot(wa, wb) - 1.0) < 1e-12                            # a unit direction of the standardised space
    both = validate("corr", samples["actual"], sliced=SLICED_K, sliced_ks_max=0.2, sliced_w1_max=0.5, store=store)
    assert [f.split("=")[0] for f in both.failures] == ["sliced.ks", "sliced.w1"]
    # without thresholds `passed` never changes, and every existing field is what it is without `sliced`
    free = validate("corr", samples["actual"], ks_max=0.1, sliced=SLICED_K, store=store)
    assert free.passed and free.sliced_ks == res.sliced_ks
    for f in dataclasses.fields(wrong):
        if not f.name.startswith("sliced"):
            assert getattr(free, f.name) == getattr(wrong, f.name), f.name
    assert validate("corr", samples["actual"], ks_max=0.1, sliced=0, store=store) == wrong
    # the control passes both
    ok = validate("corr", samples["control"], ks_max=0.1, sliced=SLICED_K, sliced_ks_max=0.2, store=store)
    print(f"control: marginal ks {ok.ks}, sliced ks {ok.sliced_ks:.4g}, sliced w1 {ok.sliced_w1:.4g}")
    assert ok.passed and max(ok.ks.values()) < 0.1 and ok.sliced_ks < 0.1
    # no joint draws
    ragged = {"a": samples["actual"]["a"], "b": samples["actual"]["b"][:-1]}
    with pytest.raises(ValueError):
        validate("corr", ragged, sliced=SLICED_K, store=store)
    assert validate("corr", ragged, store=store).sliced is None


def test_validate_without_a_live_parameter(separation_store, tmp_path):
    """Every reference std 0: no direction exists and the three fields stay None."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    from mcmc_ref_hip.validate import validate
    (tmp_path / "draws").mkdir()
    (tmp_path / "meta").mkdir()
    pq.write_table(pa.table({"chain": np.repeat(np.arange(4), 10), "draw": np.tile(np.arange(10), 4),
                             "a": np.full(40, 2.0), "b": np.full(40, -1.0)}), tmp_path / "draws" / "flat.draws.parquet")
    (tmp_path / "meta" / "flat.meta.json").write_text(json.dumps({"diagnostics": {}}))
    res = validate("flat", {"a": [2.0] * 7, "b": [-1.0] * 7}, sliced=4, sliced_ks_max=0.2,
                   store=DataStore(local_root=tmp_path, packaged_root=tmp_path / "none"))
    assert res.passed and res.sliced_ks is None and res.sliced_w1 is None and res.sliced is None


def test_validate_command(separation_store, monkeypatch):
    from click.testing import CliRunner
    from mcmc_ref_hip import store as store_mod
    from mcmc_ref_hip.cli import main
    _, root, _, files = separation_store
    monkeypatch.setenv("MCMC_REF_LOCAL_ROOT", str(root))
    monkeypatch.setattr(store_mod, "default_packaged_root", lambda: None)
    run = lambda *args: CliRunner().invoke(main, ["validate", "corr", *args])
    # (the means of separation_case are zero up to noise: the relative-error gate is asked about the std alone)
    sliced = ["--metrics", "std", "--ks-max", "0.1", "--sliced", str(SLICED_K), "--sliced-ks-max", "0.2"]
    out = run("--actual", str(files["actual"]), "--metrics", "std", "--ks-max", "0.1")
    assert out.exit_code == 0 and out.output.splitlines() == ["passed"], out.output
    out = run("--actual", str(files["actual"]), *sliced)
    lines = out.output.splitlines()
    assert out.exit_code == 2 and lines[0] == "failed" and len(lines) == 2 and lines[1].startswith("- sliced.ks="), out.output
    out = run("--actual", str(files["control"]), *sliced)
    assert out.exit_code == 0 and out.output.splitlines() == ["passed"], out.output
    out = run("--actual", str(files["actual"]), *sliced, "--sliced-seed", str(SLICED_SEED), "--format", "json")
    assert out.exit_code == 2
    doc = json.loads(out.output)
    assert doc["passed"] is False and doc["sliced_ks"] > 0.2 and len(doc["sliced"]["ks"]) == SLICED_K
    assert set(doc["ks"]) == set(PARAMS) == set(doc["sliced"]["worst_direction"])
    assert doc["failures"][0].startswith("sliced.ks=") and doc["compare"]["passed"] is True
