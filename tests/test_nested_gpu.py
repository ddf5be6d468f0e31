"""Nested R-hat on the GPU (mcr_nested_rhat, mcr_nested_rhat_dev, k_chain_moments, k_nested_combine).

* Every output against tests/test_nested_refs_cpu.py's reference in longdouble with the project's float gate
  rel_close(.., 1e-9); inf, NaN and 1.0 branches exactly.  Shapes: the smallest at which each path can go wrong (past 256
  chains, both sides of 16-bit positions, past the bucket path), and the kernel's own edges (lanes without a draw, the
  register block of MCR_NESTED_BLOCK draws, odd N, a misaligned row, heavy ties).
* One order of summation: labels are names only, and host / device entry, either layout, any workspace chunking and any
  place in the batch give the same bits.
* Errors leave the context usable; split R-hat keeps its limit of 256 chains.
* The Python functions and the `nested-rhat` command separate the pair pinned on the CPU.

Worst relative error seen on an MI355X over all gated cases: see DESIGN.md section 7 (the test prints it).
"""
from __future__ import annotations

import ctypes
import json
import types

import numpy as np
import pytest

from conftest import rel_close
from test_nested_refs_cpu import KINDS, block_ids, exact_sums, nested_all, separating, starts_remembered

pytestmark = pytest.mark.gpu

KEYS = ["nrhat"] + [f"{f}_{k}" for k in KINDS for f in ("nrhat", "between", "within")]
WORST = {"rel": 0.0, "where": ""}


@pytest.fixture(scope="module")
def ffi():
    from mcmc_ref_hip import _ffi
    return _ffi


@pytest.fixture(scope="module")
def ctx(ffi):
    c = ffi.Context(0)
    yield c
    c.close()
    print(f"\nnested R-hat: worst relative error against longdouble {WORST['rel']:.3e} ({WORST['where']})")


def bits(r: dict) -> dict:
    return {k: np.ascontiguousarray(r[k], dtype=np.float64).view(np.int64).tolist() for k in KEYS}


def centred(P, C, N, seed, K=None):
    """[P][C][N] draws around zero: a scale per parameter, and a small offset per chain so that B is not pure noise."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(P, C, N)) * (10.0 ** rng.integers(-1, 2, size=(P, 1, 1)))
    return x + 0.2 * rng.normal(size=(P, C, 1))


def gate(got: dict, x, ids, what: str):
    """Every output of every parameter against the longdouble reference."""
    for p in range(x.shape[0]):
        ref = nested_all(x[p], ids, np.longdouble)
        for k in KEYS:
            g, r = float(got[k][p]), ref[k]
            exact = r != r or r in (float("inf"), 1.0) or r == 0.0
            if exact:
                assert (g != g and r != r) or g == r, (what, p, k, g, r)
                continue
            rel = abs(g - r) / abs(r)
            if rel > WORST["rel"]:
                WORST["rel"], WORST["where"] = rel, f"{what} p={p} {k}"
            assert rel_close(g, r, 1e-9), (what, p, k, g, r, rel)
    print(f"{what}: worst relative error so far {WORST['rel']:.3e}")


SHAPES = [(4, 8, 2, 3), (6, 5, 3, 3), (8, 1, 4, 3), (8, 16, 8, 3), (300, 7, 10, 3), (511, 128, 7, 3), (512, 128, 8, 3),
          (4096, 160, 64, 2)]


@pytest.mark.parametrize("C,N,K,P", SHAPES)
def test_shapes_against_longdouble(ctx, C, N, K, P):
    x = centred(P, C, N, seed=C * 7 + N)
    ids = (np.arange(C) % K).astype(np.int32)                      # interleaved labels
    gate(ctx.nested_rhat(x, ids), x, ids, f"shape ({C}, {N}, {K})")


@pytest.mark.parametrize("N", [63, 64, 65, 511, 512, 513, 1030])
def test_chain_length_edges(ctx, ffi, N):
    """Lanes without a draw (63, 64, 65), and both sides of the register block: a chain of MCR_NESTED_BLOCK draws is kept in
    registers for the second pass, a longer one is read again.  Odd N: every other chain starts off a 16-byte boundary."""
    assert ffi.MCR_NESTED_BLOCK == 512
    C, K, P = 12, 3, 3
    x = centred(P, C, N, seed=N)
    ids = block_ids(C, K)
    gate(ctx.nested_rhat(x, ids), x, ids, f"N = {N}")


def test_exact_sums(ctx):
    """Sums with one right answer at an offset of 2^27 (a one-pass variance is off by tens of percent there)."""
    P, C, N, K = 3, 64, 16, 8
    x = np.stack([exact_sums(C, N, seed=s) for s in range(P)])
    ids = block_ids(C, K)
    got = ctx.nested_rhat(x, ids)
    gate(got, x, ids, "exact sums")
    for p in range(P):                                             # B's terms are exact: the raw between-variance has one value
        assert got["between_raw"][p] == nested_all(x[p], ids)["between_raw"]


def test_heavy_ties(ctx):
    x = np.round(centred(3, 300, 7, seed=5), 1)
    ids = (np.arange(300) % 10).astype(np.int32)
    gate(ctx.nested_rhat(x, ids), x, ids, "draws rounded to one decimal")


def test_branches(ctx):
    nan = float("nan")
    C, N, K = 8, 4, 4
    ids = block_ids(C, K)
    const = np.full((1, C, N), 2.5)
    got = ctx.nested_rhat(const, ids)
    for kind in KINDS:
        assert got[f"nrhat_{kind}"][0] == 1.0 and got[f"between_{kind}"][0] == 0.0 and got[f"within_{kind}"][0] == 0.0
    assert got["nrhat"][0] == 1.0
    levels = (np.repeat(np.arange(4.0), 2)[:, None] * np.ones((C, N)))[None]
    got = ctx.nested_rhat(levels, ids)
    assert got["nrhat_raw"][0] == float("inf") and got["within_raw"][0] == 0.0 and got["between_raw"][0] > 0.0
    gate(got, levels, ids, "constant chains, a level per superchain")
    x = centred(2, C, N, seed=3)
    one = ctx.nested_rhat(x, np.zeros(C, dtype=np.int32))          # K = 1
    assert all(np.isnan(one[k]).all() for k in ("nrhat", "nrhat_raw", "nrhat_bulk", "nrhat_tail", "between_raw"))
    gate(one, x, np.zeros(C, dtype=np.int32), "one superchain")
    empty = ctx.nested_rhat(np.empty((2, 4, 0)), block_ids(4, 2))
    assert all(np.isnan(empty[k]).all() and empty[k].shape == (2,) for k in KEYS)
    assert nan != nan


# ---- one order of summation ---------------------------------------------------------------------------------------------

def test_labels_are_names_only(ctx):
    P, C, N, K = 3, 300, 7, 10
    x = centred(P, C, N, seed=21)
    rng = np.random.default_rng(22)
    base_ids = block_ids(C, K)
    base = bits(ctx.nested_rhat(x, base_ids))
    # relabelling: 7, -2, 100, ...
    names = np.array([7, -2, 100, 5, 2 ** 31 - 1, -2 ** 31, 0, 13, 1, 99], dtype=np.int64)
    assert bits(ctx.nested_rhat(x, names[base_ids])) == base
    # interleaved and shuffled labels against the same grouping with contiguous labels: chains moved so that the
    # superchains lie in blocks, in the order of their first chain, chains in index order inside
    for ids in ((np.arange(C) % K).astype(np.int32), rng.permutation(base_ids)):
        first = {g: i for i, g in reversed(list(enumerate(ids.tolist())))}
        order = np.array(sorted(range(C), key=lambda c: (first[ids[c]], c)))
        moved = np.ascontiguousarray(x[:, order, :])
        assert bits(ctx.nested_rhat(x, ids)) == bits(ctx.nested_rhat(moved, base_ids))
    assert bits(ctx.nested_rhat(x, K)) == base                     # the int shorthand


def test_routes_give_the_same_bits(ctx, ffi):
    P, C, N, K = 3, 512, 128, 8
    x = centred(P, C, N, seed=31)
    ids = (np.arange(C) % K).astype(np.int32)
    base = bits(ctx.nested_rhat(x, ids))
    t = ctx.upload(x)
    try:
        assert bits(ctx.nested_rhat(t, ids)) == base               # device entry
        assert ctx.nested_params_per_chunk(t, K) == P
        cnp = np.ascontiguousarray(x.transpose(1, 2, 0))           # the ingest pass
        assert bits(ctx.nested_rhat(cnp, ids, "cnp")) == base
        with ffi.Context(0) as small:                              # one parameter per workspace chunk
            ts = small.upload(x)
            for mib4 in range(4, 256):
                small._check(small.lib.mcr_set_workspace_limit(small.handle, mib4 << 18))
                try:
                    per = small.nested_params_per_chunk(ts, K)
                except ffi.McrError:
                    continue
                break
            print(f"{mib4 / 4} MiB workspace: {per} of {P} parameters per chunk")
            assert per == 1
            assert bits(small.nested_rhat(ts, ids)) == base
            assert bits(small.nested_rhat(x, ids)) == base
            ts.free()
        for p in range(P):                                         # a parameter alone against its place in the batch
            alone = bits(ctx.nested_rhat(np.ascontiguousarray(x[p:p + 1]), ids))
            assert all(alone[k][0] == base[k][p] for k in KEYS), p
    finally:
        t.free()


@pytest.mark.parametrize("C,N", [(12, 64), (12, 130), (10, 7)])
def test_row_alignment_changes_no_bit(ctx, ffi, C, N):
    """The same draws 8 bytes further on: rows off the 16-byte boundary take single loads, and give the same sums."""
    P, K = 3, 2
    x = centred(P, C, N, seed=41 + N)
    ids = block_ids(C, K)
    base = bits(ctx.nested_rhat(x, ids))
    flat = np.concatenate([[0.0], x.reshape(-1)])
    buf = ffi.DeviceBuffer(ctx, flat.nbytes).upload(flat)
    try:
        shifted = types.SimpleNamespace(ptr=ctypes.c_void_p(buf.ptr.value + 8))
        t = ffi.DeviceTensor(ctx, shifted, ffi.tensor_args(x, "pcn"))
        assert bits(ctx.nested_rhat(t, ids)) == base
    finally:
        buf.free()


def test_f32_equals_f64_of_the_widened_array(ctx):
    P, C, N, K = 3, 300, 7, 10
    x32 = centred(P, C, N, seed=51).astype(np.float32)
    ids = (np.arange(C) % K).astype(np.int32)
    want = bits(ctx.nested_rhat(x32.astype(np.float64), ids))
    assert bits(ctx.nested_rhat(x32, ids)) == want
    assert bits(ctx.nested_rhat(np.ascontiguousarray(x32.transpose(1, 2, 0)), ids, "cnp")) == want
    t = ctx.upload(x32)
    try:
        assert bits(ctx.nested_rhat(t, ids)) == want
    finally:
        t.free()


# ---- errors -------------------------------------------------------------------------------------------------------------

def raw_call(ctx, ffi, x, ids):
    out = ffi.Nested()
    ip = None if ids is None else ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return ctx.lib.mcr_nested_rhat(ctx.handle, x.ctypes.data_as(ctypes.c_void_p), *ffi.tensor_args(x, "pcn"), ip, ctypes.byref(out))


def test_errors_leave_the_context_usable(ctx, ffi):
    x = centred(2, 8, 16, seed=61)
    ids = block_ids(8, 4)
    base = bits(ctx.nested_rhat(x, ids))

    def still_works():
        assert bits(ctx.nested_rhat(x, ids)) == base

    assert raw_call(ctx, ffi, x, np.array([0, 0, 0, 1, 1, 2, 2, 3], dtype=np.int32)) == ffi.MCR_EINVAL
    assert b"same number of chains" in ctx.lib.mcr_last_error(ctx.handle)
    still_works()
    assert raw_call(ctx, ffi, x, None) == ffi.MCR_EINVAL
    assert b"superchain is NULL" in ctx.lib.mcr_last_error(ctx.handle)
    still_works()
    with pytest.raises(ValueError, match="same number of chains"):
        ctx.nested_rhat(x, [0, 0, 0, 1, 1, 2, 2, 3])
    over = ffi.MCR_NESTED_MAX_CHAINS + 1
    with pytest.raises(ffi.McrError, match=f"at most {ffi.MCR_NESTED_MAX_CHAINS} chains") as e:
        ctx.nested_rhat(np.zeros((1, over, 1)), 1)
    assert e.value.code == ffi.MCR_EINVAL
    still_works()
    bad = x.copy()
    bad[1, 3, 5] = np.nan
    with pytest.raises(ffi.McrError) as e:
        ctx.nested_rhat(bad, ids)
    assert e.value.code == ffi.MCR_ENONFINITE
    still_works()
    flat = ffi.DeviceBuffer(ctx, x.nbytes).upload(x)
    try:
        ragged = ctx.ragged_tensor(flat, [10, 20, 30, 68], 2)
        with pytest.raises(ValueError, match="ragged"):
            ctx.nested_rhat(ragged, 2)
        t = ffi.DeviceTensor(ctx, flat, ffi.tensor_args(x, "pcn"))
        ctx.enqueue(t)                                             # a summary in flight
        with pytest.raises(ffi.McrError, match="summaries in flight"):
            ctx.nested_rhat(t, ids)
        ctx.wait()
        assert bits(ctx.nested_rhat(t, ids)) == base
    finally:
        flat.free()
    still_works()


def test_split_rhat_keeps_its_limit(ctx, ffi):
    with pytest.raises(ffi.McrError, match="at most 256 chains are supported"):
        ctx.summarize(centred(1, 300, 7, seed=71))


# ---- Python and the command ---------------------------------------------------------------------------------------------

def test_python_layers_separate_the_pair(ctx):
    from mcmc_ref_hip import diagnostics
    good, bad, ids = separating()
    g, b = ctx.nested_rhat(good[None], ids), ctx.nested_rhat(bad[None], ids)
    for k in ("nrhat", "nrhat_raw", "nrhat_bulk", "nrhat_tail"):
        assert g[k][0] < 1.01 and b[k][0] > 1.1, (k, g[k], b[k])
    assert diagnostics.nested_rhat(list(good), ids, context=ctx) == g["nrhat"][0]
    assert diagnostics.nested_rhat(list(bad), ids, context=ctx) > 1.1
    detail = diagnostics.nested_rhat_detail(list(bad), ids, context=ctx)
    assert detail == {k: float(v[0]) for k, v in b.items()}
    x, sid = starts_remembered()
    assert ctx.nested_rhat(x[None], sid)["nrhat_raw"][0] > 2.0
    profile_ctx_reports_the_kernels(ctx, bad, ids)


def profile_ctx_reports_the_kernels(ctx, x, ids):
    ctx.profile(True)
    ctx.profile_reset()
    ctx.nested_rhat(x[None], ids)
    prof = ctx.profile_get()
    ctx.profile(False)
    assert prof["k_chain_moments"]["launches"] == 1 and prof["k_nested_combine"]["launches"] == 1
    assert "k_acov_seg" not in prof and "k_diag" not in prof and "k_diag_combine2" not in prof


def test_nested_rhat_command(tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import cli
    good, bad, ids = separating()
    C, N = good.shape
    chain_id = (ids.astype(np.int64) * (C // 16) + np.arange(C) // 16)          # blocks in chain-id order = the builder's superchains
    path = tmp_path / "draws.csv"
    with path.open("w") as f:
        f.write("chain,draw,good,bad\n")
        for c in range(C):
            for n in range(N):
                f.write(f"{chain_id[c]},{n},{float(good[c, n])!r},{float(bad[c, n])!r}\n")
    res = CliRunner().invoke(cli.main, ["nested-rhat", str(path), "--superchains", "16", "--format", "json"])
    assert res.exit_code == 0, res.output
    out = json.loads(res.output)
    assert set(out) == {"good", "bad"} and set(out["good"]) == {"nrhat", "nrhat_bulk", "nrhat_tail", "nrhat_raw"}
    for k in out["good"]:
        assert out["good"][k] < 1.01 and out["bad"][k] > 1.1, (k, out)
    res = CliRunner().invoke(cli.main, ["nested-rhat", str(path), "--superchains", "16", "--params", "bad"])
    assert res.exit_code == 0 and "nrhat_raw" in res.output and "good" not in res.output
    res = CliRunner().invoke(cli.main, ["nested-rhat", str(path), "--superchains", "7"])
    assert res.exit_code != 0 and "do not divide" in res.output
