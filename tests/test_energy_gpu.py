"""The energy distance (mcr_energy_distance, mcr_energy_distance_dev, k_energy_pairs, k_energy_reduce) on the GPU.

* The device against mcr_energy_distance_host (pinned on the host by tests/test_energy_refs_cpu.py) at every tile and
  chunk edge of the kernel as built: A, B, C within 1e-9 relative, E within 1e-9 * 2A.
* Inputs whose distances are all integers: A, B, C in bits, with one launch and with many, and at full size (P = 1,
  40 000 draws a side) against the sort-and-cumulative-sum identity.
* One pair: the bits of the definition.
* The same bits on both entries, at either alignment, on repeated calls, with profiling, under a tight workspace limit.
* Launch counts, every documented error, and the check through validate() and the `validate` command.
"""
from __future__ import annotations

import ctypes
import dataclasses
import json

import numpy as np
import pytest

from test_energy_refs_cpu import (LATTICE_P, PAIR_P, assert_close, general_case, lattice_case, lattice_expected, line_case,
                                  line_expected, pair_case, pair_distance)
from test_sliced_cpu import PARAMS, separation_case

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
def edges(ffi):
    TI, TJ, PC = ffi.MCR_ENERGY_TILE_I, ffi.MCR_ENERGY_TILE_J, ffi.MCR_ENERGY_CHUNK_P
    sides = lambda T: (1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1)
    return sides(TI), sides(TJ), (1, 2, PC - 1, PC, PC + 1, 2 * PC + 1)


@pytest.fixture(scope="module")
def line():
    """The full-size case and its exact answer, computed once."""
    ref, act = line_case()
    return ref, act, line_expected(ref, act)


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


def abc(d: dict):
    return d["a"], d["b"], d["c"]


# ---- against the host routine ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pi", range(6))
def test_device_against_host_at_every_edge(ctx, ffi, edges, pi):
    """Mr over the edges of TI crossed with Ma over the edges of TJ, odd and even, for one P of the chunk edges; the
    variants of the host test rotate through the cases (plain, scale, one zero scale, offset 1e6)."""
    sides_i, sides_j, chunk = edges
    P = chunk[pi]
    worst = {"a": 0.0, "b": 0.0, "c": 0.0, "e": 0.0}
    n = 0
    for Mr in sides_i:
        for Ma in sides_j:
            variant = ("plain", "scale", "zero", "offset")[n % 4]
            n += 1
            ref, act, scale = general_case(Mr, Ma, P, variant)
            got = ctx.energy_distance(ref, act, scale)
            exp = ffi.energy_distance_host(ref, act, scale)
            for k in "abc":
                if exp[k]:
                    worst[k] = max(worst[k], abs(got[k] - exp[k]) / abs(exp[k]))
            if exp["a"]:
                worst["e"] = max(worst["e"], abs(got["e"] - exp["e"]) / (2 * exp["a"]))
            assert_close(got, exp, (Mr, Ma, P, variant))
            assert got["h"] == (got["e"] / (2 * got["a"]) if got["a"] else 0.0) and got["t"] == Mr * Ma / (Mr + Ma) * got["e"]
    print(f"P = {P}: worst relative error over {n} shapes: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("Mr,Ma", [(258, 130), (257, 131), (258, 131)])
def test_alignment_and_entry_do_not_change_a_bit(ctx, ffi, Mr, Ma):
    """Even and odd M through the host entry, the device entry on 16-byte aligned samples (16-byte loads when both M are
    even) and on samples 8 bytes further (8-byte loads): the same bits, inside the gates of the host routine."""
    P = ffi.MCR_ENERGY_CHUNK_P + 3
    ref, act, scale = general_case(Mr, Ma, P, "scale")
    host = ctx.energy_distance(ref, act, scale)
    assert_close(host, ffi.energy_distance_host(ref, act, scale), (Mr, Ma))
    for sr, sa in ((0, 0), (8, 8), (0, 8)):
        with OnDevice(ctx, ref, sr) as dr, OnDevice(ctx, act, sa) as da:
            assert ctx.energy_distance_dev(dr.addr, Mr, da.addr, Ma, P, scale) == host, (sr, sa)
    assert ctx.energy_distance(ref, act, scale) == host                         # a repeated call
    assert ctx.energy_distance(ref, act, np.ones(P)) == ctx.energy_distance(ref, act, None)
    ctx.profile(True)
    try:
        assert ctx.energy_distance(ref, act, scale) == host
    finally:
        ctx.profile(False)


# ---- exact cases ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", PAIR_P)
def test_pair_bits(ctx, P):
    x, y, s = pair_case(P)
    for scale in (None, s):
        got = ctx.energy_distance(x[:, None], y[:, None], scale)
        assert got["a"] == pair_distance(x, y, scale)
        assert got["b"] == 0.0 and got["c"] == 0.0 and got["h"] == 1.0
        assert ctx.energy_distance(y[:, None], x[:, None], scale)["a"] == got["a"]


@pytest.mark.parametrize("P", LATTICE_P)
def test_lattice_bits(ctx, ffi, P):
    TI = ffi.MCR_ENERGY_TILE_I
    for Mr, Ma in ((1, 1), (5, 3), (TI + 2, 2 * TI + 1), (2 * TI, 2 * TI)):
        ref, act, sums = lattice_case(P, Mr, Ma)
        assert abc(ctx.energy_distance(ref, act)) == lattice_expected(sums, Mr, Ma), (Mr, Ma)


def test_launch_budget_changes_no_bit(ctx, ffi, monkeypatch):
    """A context whose launch budget (MCR_ENERGY_LAUNCH_WORK, read at mcr_init) holds one tile, then four: as many
    launches as the header's rule says, the exact lattice answer and the bits of the default context."""
    TI, TJ = ffi.MCR_ENERGY_TILE_I, ffi.MCR_ENERGY_TILE_J
    Mr, Ma = 2 * TI + 2, 3 * TI + 1
    ref, act, sums = lattice_case(4, Mr, Ma)
    P = ref.shape[0]
    rnd_r, rnd_a, scale = general_case(Mr, Ma, P, "scale")
    whole, whole_rnd = ctx.energy_distance(ref, act), ctx.energy_distance(rnd_r, rnd_a, scale)
    assert abc(whole) == lattice_expected(sums, Mr, Ma)
    for tiles in (1, 4):
        budget = tiles * TI * TJ * P + 5
        monkeypatch.setenv("MCR_ENERGY_LAUNCH_WORK", str(budget))
        with ffi.Context(0) as small:
            small.profile(True)
            assert small.energy_distance(ref, act) == whole
            prof = small.profile_get()
            launches = ffi.energy_launches(Mr, Ma, P, budget)
            assert launches == -(-(3 * 4 + 6 + 10) // tiles) and launches > 1
            assert prof["k_energy_pairs"]["launches"] == launches and prof["k_energy_reduce"]["launches"] == 1, prof
            small.profile(False)
            assert small.energy_distance(rnd_r, rnd_a, scale) == whole_rnd
        monkeypatch.delenv("MCR_ENERGY_LAUNCH_WORK")


def test_launch_counts(ctx, ffi):
    ref, act, scale = general_case(300, 37, 7, "plain")
    ctx.profile_reset()
    ctx.profile(True)
    try:
        ctx.energy_distance(ref, act)
        prof = ctx.profile_get()
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    assert ffi.energy_launches(300, 37, 7) == 1
    assert ffi.energy_launches(40000, 40000, 100) == 2 and ffi.energy_launches(40000, 40000, 1) == 1
    assert prof["k_energy_pairs"]["launches"] == 1 and prof["k_energy_reduce"]["launches"] == 1, prof
    assert set(prof) == {"k_energy_pairs", "k_energy_reduce"}


def test_full_size_line_and_workspace_limit(ctx, ffi, line):
    """P = 1, 40 000 integer-valued draws a side: A, B, C in bits against the sort-and-cumsum identity; the same bits
    under a workspace limit that just fits; MCR_ENOMEM, naming the need, under one that does not."""
    ref, act, exact = line
    M = ref.shape[1]
    got = ctx.energy_distance(ref, act)
    assert abc(got) == exact
    need = ctx.energy_workspace(M, M, 1)
    nt = -(-M // ffi.MCR_ENERGY_TILE_I)
    jobs = nt * nt + nt * (nt + 1)                                # the cross tiles and the two upper triangles
    assert need >= 8 * jobs > (1 << 20)
    with ffi.Context(0) as small:
        small._check(small.lib.mcr_set_workspace_limit(small.handle, need))
        assert small.energy_workspace(M, M, 1) == need
        assert small.energy_distance(ref, act) == got
        small._check(small.lib.mcr_set_workspace_limit(small.handle, need - 1))
        with pytest.raises(ffi.McrError) as exc:
            small.energy_distance(ref, act)
        assert exc.value.code == ffi.MCR_ENOMEM and str(need) in exc.value.message, exc.value.message
        assert small.energy_distance(ref[:, :300], act[:, :200]) == ctx.energy_distance(ref[:, :300], act[:, :200])


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(ctx, ffi):
    dp = lambda v: None if v is None else v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    P, Mr, Ma = 3, 5, 4
    ref, act, scale = general_case(Mr, Ma, P, "scale")
    out = np.full(6, -7.0)
    good = dict(ref=ref, Mr=Mr, act=act, Ma=Ma, P=P, scale=scale, out=out)

    def call(**kw):
        a = {**good, **kw}
        rc = ctx.lib.mcr_energy_distance(ctx.handle, dp(a["ref"]), a["Mr"], dp(a["act"]), a["Ma"], a["P"], dp(a["scale"]), dp(a["out"]))
        return rc, (ctx.lib.mcr_last_error(ctx.handle) or b"").decode()

    def bad(v, where, value):
        w = v.copy()
        w.flat[where] = value
        return w

    want = ctx.energy_distance(ref, act, scale)
    einval = [(dict(ref=None), "NULL"), (dict(act=None), "NULL"), (dict(out=None), "NULL"), (dict(Mr=0), "draw"), (dict(Ma=0), "draw"),
              (dict(Mr=-3), "draw"), (dict(P=0), "parameter"), (dict(P=-1), "parameter"), (dict(scale=bad(scale, 1, -0.5)), "scale[1]"),
              (dict(scale=bad(scale, 2, np.nan)), "scale[2]"), (dict(scale=bad(scale, 0, np.inf)), "scale[0]"),
              (dict(Mr=1 << 22, Ma=1 << 22), "work limit"), (dict(Mr=1 << 40, Ma=1 << 40, P=1 << 40), "work limit")]
    for kw, cause in einval:
        rc, msg = call(**kw)
        assert rc == ffi.MCR_EINVAL and cause in msg, (list(kw), rc, msg)
        assert np.all(out == -7.0)                                  # nothing was written
        assert call()[0] == ffi.MCR_OK and dict(zip(ffi.ENERGY_KEYS, out)) == want
        out[:] = -7.0
    v = ctypes.c_size_t(0)
    assert ctx.lib.mcr_energy_workspace(ctx.handle, 0, 4, 2, ctypes.byref(v)) == ffi.MCR_EINVAL
    assert ctx.lib.mcr_energy_workspace(ctx.handle, 4, 4, 2, None) == ffi.MCR_EINVAL
    assert ctx.lib.mcr_energy_workspace(ctx.handle, 1 << 22, 1 << 22, 1, ctypes.byref(v)) == ffi.MCR_EINVAL
    # summaries in flight
    t = ctx.upload(np.random.default_rng(0).normal(size=(2, 4, 100)), "pcn")
    try:
        ctx.enqueue(t)
        rc, msg = call()
        assert rc == ffi.MCR_EINVAL and "in flight" in msg
        ctx.wait_one()
    finally:
        t.free()
    assert call()[0] == ffi.MCR_OK
    # non-finite draws and an overflowing squared distance
    big_r, big_a = bad(ref, 1, 1e200), bad(act, 1, -1e200)
    for kw in (dict(ref=bad(ref, 3, np.nan)), dict(act=bad(act, 7, np.inf)), dict(ref=bad(ref, 14, -np.inf)),
               dict(ref=big_r, act=big_a, scale=None)):
        out[:] = -7.0
        rc, msg = call(**kw)
        assert rc == ffi.MCR_ENONFINITE and "non-finite" in msg and "overflow" in msg, (list(kw), rc, msg)
        assert np.all(out == -7.0)
        assert call()[0] == ffi.MCR_OK and dict(zip(ffi.ENERGY_KEYS, out)) == want
    with OnDevice(ctx, bad(ref, 0, np.nan)) as dr, OnDevice(ctx, act) as da:
        with pytest.raises(ffi.McrError) as exc:
            ctx.energy_distance_dev(dr.addr, Mr, da.addr, Ma, P, scale)
        assert exc.value.code == ffi.MCR_ENONFINITE
    # the Python method checks what Context.two_sample checks, with the same exceptions
    with pytest.raises(ValueError):
        ctx.energy_distance(bad(ref, 0, np.nan), act)
    with pytest.raises(ValueError):
        ctx.energy_distance(ref, act[:1])
    with pytest.raises(ValueError):
        ctx.energy_distance(ref, act, scale[:1])
    with pytest.raises(ValueError):
        ctx.energy_distance(ref, act, bad(scale, 0, -1.0))
    assert ctx.energy_distance(ref, act, scale) == want


# ---- separating power, through validate() and the CLI ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def separation_store(tmp_path_factory):
    """A temporary store holding the reference of separation_case as model `corr` (4 chains of 500 draws), and the
    wrong-correlation and control samples as dicts and as CSV files."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    root = tmp_path_factory.mktemp("energy")
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


def test_validate_separates_a_wrong_correlation(separation_store, ffi):
    from mcmc_ref_hip import validate as validate_mod
    store, _, samples, _ = separation_store
    # (the means of separation_case are zero up to noise: the relative-error gate is asked about the std alone)
    validate = lambda *a, **kw: validate_mod.validate(*a, metrics=("std",), **kw)
    plain = validate("corr", samples["actual"], ks_max=0.1, store=store)
    assert plain.passed and plain.energy is None and plain.energy_detail is None        # every marginal is right
    res = validate("corr", samples["actual"], ks_max=0.1, energy=True, energy_max=0.03, store=store)
    print(f"wrong correlation: {res.energy_detail}")
    assert not res.passed and len(res.failures) == 1 and res.failures[0].startswith("energy="), res.failures
    assert res.failures[0] == f"energy={res.energy:.3g} > 0.03"
    d = res.energy_detail
    assert res.energy == d["e"] > 0.1 and set(d) == {"a", "b", "c", "e", "h", "t", "mr", "ma"} and (d["mr"], d["ma"]) == (2000, 2037)
    ref, actual, control = separation_case()
    host = ffi.energy_distance_host(ref, actual, 1.0 / ref.std(axis=1))
    assert abs(d["e"] - host["e"]) <= 1e-8 * 2 * host["a"]       # (validate scales by the device's std: numpy's within 1e-9)
    # without energy_max `passed` and every other field are what they are without `energy`
    free = validate("corr", samples["actual"], ks_max=0.1, energy=True, store=store)
    assert free.passed and free.energy == res.energy and free.energy_detail == d
    for f in dataclasses.fields(plain):
        if not f.name.startswith("energy"):
            assert getattr(free, f.name) == getattr(plain, f.name), f.name
    assert validate("corr", samples["actual"], ks_max=0.1, energy=False, store=store) == plain
    # the control passes
    ok = validate("corr", samples["control"], ks_max=0.1, energy=True, energy_max=0.03, store=store)
    print(f"control: {ok.energy_detail}")
    assert ok.passed and 0.0 <= ok.energy < 0.01
    # thinned to at most 500 draws a side, the two are still apart
    thin_bad = validate("corr", samples["actual"], energy=True, energy_max=0.03, energy_max_draws=500, store=store)
    thin_ok = validate("corr", samples["control"], energy=True, energy_max=0.03, energy_max_draws=500, store=store)
    print(f"500 draws: wrong {thin_bad.energy:.4g}, control {thin_ok.energy:.4g}")
    assert (thin_bad.energy_detail["mr"], thin_bad.energy_detail["ma"]) == (500, 408)
    assert not thin_bad.passed and thin_bad.energy > 0.1 and thin_ok.passed and thin_ok.energy < 0.03
    # no joint draws
    ragged = {"a": samples["actual"]["a"], "b": samples["actual"]["b"][:-1]}
    with pytest.raises(ValueError):
        validate("corr", ragged, energy=True, store=store)
    assert validate("corr", ragged, store=store).energy is None


def test_validate_without_a_live_parameter(tmp_path):
    """Every reference std 0: nothing to scale by, and the two fields stay None."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip.store import DataStore
    from mcmc_ref_hip.validate import validate
    (tmp_path / "draws").mkdir()
    (tmp_path / "meta").mkdir()
    pq.write_table(pa.table({"chain": np.repeat(np.arange(4), 10), "draw": np.tile(np.arange(10), 4),
                             "a": np.full(40, 2.0), "b": np.full(40, -1.0)}), tmp_path / "draws" / "flat.draws.parquet")
    (tmp_path / "meta" / "flat.meta.json").write_text(json.dumps({"diagnostics": {}}))
    res = validate("flat", {"a": [2.0] * 7, "b": [-1.0] * 7}, energy=True, energy_max=0.03,
                   store=DataStore(local_root=tmp_path, packaged_root=tmp_path / "none"))
    assert res.passed and res.energy is None and res.energy_detail is None


def test_validate_command(separation_store, monkeypatch):
    from click.testing import CliRunner
    from mcmc_ref_hip import store as store_mod
    from mcmc_ref_hip.cli import main
    _, root, _, files = separation_store
    monkeypatch.setenv("MCMC_REF_LOCAL_ROOT", str(root))
    monkeypatch.setattr(store_mod, "default_packaged_root", lambda: None)
    run = lambda *args: CliRunner().invoke(main, ["validate", "corr", "--metrics", "std", *args])
    out = run("--actual", str(files["actual"]), "--energy")
    assert out.exit_code == 0 and out.output.splitlines() == ["passed"], out.output        # the text is unchanged
    out = run("--actual", str(files["actual"]), "--energy-max", "0.03")                       # implies --energy
    lines = out.output.splitlines()
    assert out.exit_code == 2 and lines[0] == "failed" and len(lines) == 2 and lines[1].startswith("- energy="), out.output
    out = run("--actual", str(files["control"]), "--energy", "--energy-max", "0.03")
    assert out.exit_code == 0 and out.output.splitlines() == ["passed"], out.output
    out = run("--actual", str(files["actual"]), "--energy-max", "0.03", "--energy-max-draws", "500", "--format", "json")
    assert out.exit_code == 2
    doc = json.loads(out.output)
    assert doc["passed"] is False and doc["energy"] == doc["energy_detail"]["e"] > 0.1
    assert (doc["energy_detail"]["mr"], doc["energy_detail"]["ma"]) == (500, 408)
    assert doc["failures"] == [f"energy={doc['energy']:.3g} > 0.03"] and doc["compare"]["passed"] is True
    out = run("--actual", str(files["control"]), "--energy-max", "0.03", "--energy-max-draws", "500", "--format", "json")
    assert out.exit_code == 0 and json.loads(out.output)["energy"] < 0.03
    out = run("--actual", str(files["actual"]), "--format", "json")
    doc = json.loads(out.output)
    assert out.exit_code == 0 and doc["energy"] is None and doc["energy_detail"] is None
