"""The extension entry points (mcr_covariance, mcr_covariance_dev, mcr_two_sample) at every tile and slice edge.

Every expected value comes from the CPU references of tests/test_ext_refs_cpu.py (pinned there against scipy, exact
fractions and integer arithmetic), never from a second GPU call; every geometry a case claims is asserted through
`cov_plan` / `two_sample_blocks`, so a change of the host arithmetic makes the case say it misses its edge.

Covariance is held to the per-entry bound of `cov_tolerance` (no max-norm term) and, on the exact-integer inputs of
`exact_cov_inputs`, to the bits of G / M.  KS is held to the bits of the exact rational at every size, W1 to
`w1_tolerance` (and to the project's rel = 1e-12 outside the 1e15-offset family).

Measured on an MI355X (printed per case, `-v` shows them): every exact-integer case bit-identical
to G / M on all three paths; real-valued covariance at most 6.5 eps sqrt(c_ii c_jj) (0.07 of the bound at M = 2, 1e-4 of
it at M = 40 000); W1 at most 0.072 of its bound (8 draws a side), 1e-5 .. 5e-4 of it on long samples.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np
import pytest

from test_ext_refs_cpu import (COV_TILE, EPS, MERGE_TILE, cov_plan, cov_tolerance, exact_cov_inputs, exact_cov_ref,
                               exact_ks_numerator, exact_two_sample_rows, exact_w1, expected_ks,
                               ill_conditioned_inputs, last_slice_draws, longdouble_cov, m_with_last_slice,
                               special_rows, two_sample_blocks, w1_tolerance)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture
def say(request, capsys):
    """Prints a measured figure: captured with the test (shown on failure) and straight to the terminal under -v."""
    def _say(line: str):
        print(line)
        if request.config.getoption("verbose") > 0:
            with capsys.disabled():
                print("\n    " + line, end="")
    return _say


class _At:
    """What a DeviceTensor reads of its buffer: the address of the view's first element."""

    def __init__(self, ptr: int):
        self.ptr = ctypes.c_void_p(ptr)


class OnDevice:
    """x [P][M] f64 in device memory, its first element `shift` bytes past a 256-byte aligned allocation."""

    def __init__(self, ctx, x: np.ndarray, shift: int = 0):
        from mcmc_ref_hip import _ffi
        self.ctx, self.x = ctx, np.ascontiguousarray(x, dtype=np.float64)
        self.P, self.M = self.x.shape
        self.buf = _ffi.DeviceBuffer(ctx, self.x.nbytes + 16)
        assert self.buf.ptr.value % 16 == 0 and shift in (0, 8)
        self.addr = self.buf.ptr.value + shift
        ctx._check(ctx.lib.mcr_memcpy_h2d(ctx.handle, ctypes.c_void_p(self.addr),
                                          self.x.ctypes.data_as(ctypes.c_void_p), self.x.nbytes))
        self.out = _ffi.DeviceBuffer(ctx, self.P * self.P * 8)

    def moments(self):
        from mcmc_ref_hip import _ffi
        t = _ffi.DeviceTensor(self.ctx, _At(self.addr), _ffi.tensor_args(self.x.reshape(self.P, 1, self.M), "pcn"))
        return self.ctx.moments(t)

    def covariance(self) -> np.ndarray:
        c = self.ctx
        c._check(c.lib.mcr_covariance_dev(c.handle, ctypes.c_void_p(self.addr), self.M, self.P, self.out.ptr))
        return self.out.download(np.float64, self.P * self.P).reshape(self.P, self.P)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.buf.free()
        self.out.free()


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_cov(got, ref, mean, M, what, say):
    """The per-entry bound, and the structure every result has: entries mirrored across the block diagonal are the
    same stored value; inside a diagonal block the two halves agree within the bound.  Returns max |err| / (eps u)."""
    P = len(got)
    ref64 = np.asarray(ref, dtype=np.float64)
    tol = cov_tolerance(ref, mean, M)
    err = np.abs(got - ref).astype(np.float64)
    sd = np.sqrt(ref64.diagonal())
    u = np.outer(sd, sd)
    live = u > 0
    fig = float((err[live] / (EPS * u[live])).max()) if live.any() else 0.0
    frac = float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0
    say(f"cov {what}: max |err| / (eps u) = {fig:.3g}, max |err| / bound = {frac:.3g}, bound's M + 8 = {M + 8}")
    bad = np.argwhere(~(err <= tol))
    assert len(bad) == 0, (what, len(bad), "first (i, j, got, ref, tol):",
                           [(int(i), int(j), got[i, j], float(ref64[i, j]), tol[i, j]) for i, j in bad[:5]])
    blk = np.arange(P) // COV_TILE
    unequal = bits(got) != bits(got.T)
    across = blk[:, None] != blk[None, :]
    assert not (unequal & across).any(), (what, "mirror across blocks", np.argwhere(unequal & across)[:5])
    assert np.all(np.abs(got - got.T) <= tol), (what, "symmetry inside the diagonal blocks")
    return fig


def check_exact_case(ctx, P, M, say, seed, host=True, shifted=True):
    """Exact-integer inputs through mcr_covariance_dev at a 16-byte aligned address, at one 8 bytes further (the
    non-EVEN kernel on an even M) and through the host entry point; the means first."""
    rng = np.random.default_rng(seed)
    x, off, D = exact_cov_inputs(P, M, rng)
    ref = exact_cov_ref(D)
    pl = cov_plan(M, P)
    results = {}
    for shift in (0, 8) if shifted else (0,):
        assert cov_plan(M, P, aligned16=shift == 0).even == (M % 2 == 0 and shift == 0)
        with OnDevice(ctx, x, shift) as dev:
            mean, _ = dev.moments()
            assert np.array_equal(bits(mean), bits(off)), ("moments are not exact", P, M, shift,
                                                           np.flatnonzero(mean != off)[:5])
            results[f"dev+{shift}"] = dev.covariance()
    if host:
        results["host"] = ctx.covariance(x)
    del x, D
    ndiff = {}
    for name, got in results.items():
        check_cov(got, ref, off, M, f"exact P={P} M={M} {pl} {name}", say)
        ndiff[name] = int(np.count_nonzero(bits(got) != bits(ref)))
    say(f"cov exact P={P} M={M}: entries that differ from G / M in bits: {ndiff}")
    # every centred value, product and partial sum is an integer below 2^53: observed bit-identical on every case
    assert all(n == 0 for n in ndiff.values()), (P, M, ndiff)
    return results


def check_real_case(ctx, P, M, say, seed):
    """Real-valued draws of mixed scale at the same shape, against the long-double reference: here every draw carries
    weight, the last one of an odd M included (the exact-integer inputs end an odd M on a centred value of zero, so
    they cannot see that draw counted twice or not at all)."""
    x = ill_conditioned_inputs(P, M, np.random.default_rng(seed), special=False)
    ref, mean = longdouble_cov(x)
    results = {"host": ctx.covariance(x)}
    for shift in (0, 8):
        with OnDevice(ctx, x, shift) as dev:
            results[f"dev+{shift}"] = dev.covariance()
    for name, got in results.items():
        check_cov(got, ref, mean, M, f"real P={P} M={M} {name}", say)


# =====================================================================================================================
# covariance: exact-integer inputs
# =====================================================================================================================
@pytest.mark.parametrize("P,nb", [(127, 1), (128, 1), (129, 2), (255, 2), (256, 2), (257, 3), (384, 3), (640, 5),
                                  (1000, 8)])
def test_cov_block_counts_one_to_eight(ctx, say, P, nb):
    """nb = 1 .. 8 with ragged and full last blocks: from nb = 3 on, the (bi, bj) decode loop runs more than once, a
    tile lies off the diagonal and off the first block row, and the finisher's mirror read reaches such a tile."""
    M = 4000
    pl = cov_plan(M, P)
    assert pl.nb == nb and pl.tiles == nb * (nb + 1) // 2 and pl.even and pl.S == 1 and pl.ksplit >= 2
    assert (P % COV_TILE == 0) == (P in (128, 256, 384, 640))
    check_exact_case(ctx, P, M, say, seed=P)


def test_cov_benchmarked_shape(ctx, say):
    """1 000 x 40 000: the shape of the README's TFLOP/s figure."""
    P, M = 1000, 40000
    pl = cov_plan(M, P)
    assert (pl.nb, pl.tiles, pl.ksplit, pl.kchunk, pl.even, pl.S) == (8, 36, 15, 2672, True, 8)
    check_exact_case(ctx, P, M, say, seed=1)


def test_cov_partial_tile_cap_lowers_ksplit(ctx, say):
    """nb = 15: 120 tiles ask for 5 draw slices, 128 MB of 1920 x 1920 partial tiles hold 4."""
    P, M = 1900, 2048
    pl = cov_plan(M, P)
    assert 1793 <= P <= 1920 and M >= 1280
    assert (pl.nb, pl.tiles, pl.ksplit_wanted, pl.cap, pl.ksplit, pl.kchunk) == (15, 120, 5, 4, 4, 512)
    check_exact_case(ctx, P, M, say, seed=2)


def test_cov_ksplit_equals_cap(ctx, say):
    P, M = 2048, 4096
    pl = cov_plan(M, P)
    assert (pl.nb, pl.tiles, pl.ksplit_wanted, pl.cap, pl.ksplit, pl.kchunk) == (16, 136, 4, 4, 4, 1024)
    check_exact_case(ctx, P, M, say, seed=3)


def test_cov_single_slice_of_528_tiles(ctx, say):
    """Every entry is one accumulation chain over all 4096 draws."""
    P, M = 4096, 4096
    pl = cov_plan(M, P)
    assert (pl.nb, pl.tiles, pl.cap, pl.ksplit, pl.kchunk) == (32, 528, 1, 1, 4096)
    check_exact_case(ctx, P, M, say, seed=4)


def test_cov_limit_8192_and_rejection_above(ctx, say):
    """P = 8192: 2080 tiles, 512 MB of partial tiles; the cap computes to 0 and only its clamp keeps one slice.
    P = 8193 is rejected by name, and the context answers afterwards."""
    from mcmc_ref_hip import _ffi
    P, M = 8192, 512
    pl = cov_plan(M, P)
    assert (pl.nb, pl.tiles, pl.ksplit_wanted, pl.cap, pl.ksplit, pl.kchunk) == (64, 2080, 1, 0, 1, 512)
    check_exact_case(ctx, P, M, say, seed=5)
    with pytest.raises(_ffi.McrError) as ei:
        ctx.covariance(np.zeros((8193, 16)))
    assert ei.value.code == _ffi.MCR_EINVAL and "8192" in ei.value.message
    with OnDevice(ctx, np.zeros((8193, 2))) as dev:
        with pytest.raises(_ffi.McrError) as ei:
            dev.covariance()
        assert ei.value.code == _ffi.MCR_EINVAL and "8192" in ei.value.message
    check_exact_case(ctx, 5, 100, say, seed=6)


@pytest.mark.parametrize("M", [1, 2, 15, 16, 17, 255, 256, 257, 511, 513, 16383, 16384, 16385])
def test_cov_draw_count_sweep(ctx, say, M):
    """P = 129: the one-slice limit of 256 draws, kchunk's rounding to 16 and the moments kernel's switch to 8
    slices."""
    P = 129
    pl = cov_plan(M, P)
    assert pl.nb == 2 and pl.tiles == 3
    assert pl.ksplit == {1: 1, 2: 1, 15: 1, 16: 1, 17: 1, 255: 1, 256: 1, 257: 2, 511: 2, 513: 3, 16383: 64,
                         16384: 64, 16385: 65}[M]
    assert pl.kchunk == {1: 16, 2: 16, 15: 16, 16: 16, 17: 32, 255: 256, 256: 256, 257: 144, 511: 256, 513: 176,
                         16383: 256, 16384: 256, 16385: 256}[M]
    assert pl.S == (8 if M >= 16384 else 1)
    check_exact_case(ctx, P, M, say, seed=100 + M)
    check_real_case(ctx, P, M, say, seed=300 + M)


@pytest.mark.parametrize("last", [1, 2, 14, 15, 16, 17, 18])
def test_cov_last_slice_length(ctx, say, last):
    """A last draw slice of exactly 1, 15, 16 and 17 draws.  Slices are multiples of 16 draws, so M has the parity of
    the last slice: 1, 15 and 17 are odd M (the scalar-load kernel, clamped at M - 1), 16 an even M; 2, 14 and 18 are
    the even M next to them, where the 16-byte-load kernel clamps its ragged last step at M - 2."""
    P = 129
    M = m_with_last_slice(P, last)
    pl = cov_plan(M, P)
    assert pl.ksplit >= 2 and last_slice_draws(M, P) == last == M - (pl.ksplit - 1) * pl.kchunk
    assert pl.even == (last % 2 == 0) and M % 2 == last % 2
    check_exact_case(ctx, P, M, say, seed=200 + last)
    check_real_case(ctx, P, M, say, seed=400 + last)


# =====================================================================================================================
# covariance: real-valued, ill-conditioned inputs
# =====================================================================================================================
@pytest.mark.parametrize("P", [37, 130, 260])
@pytest.mark.parametrize("M", [10001, 40000])
def test_cov_ill_conditioned(ctx, say, P, M):
    """Correlated rows of scale 1e-6 .. 1e6, offset by up to 1e6 standard deviations, against the long-double two-pass
    reference; and the special rows.  A constant row: the moments kernel returns the constant itself, so its row and
    column are exactly zero.  Two identical rows: cov_ij, cov_ii and cov_jj are the same bits, inside a block and
    across blocks (the order in which draws are accumulated does not depend on the tile; the pairs lie an even number
    of rows apart, so with M odd both start on the same 16-byte phase and their means are summed in the same order)."""
    rng = np.random.default_rng(1000 * P + M)
    x = ill_conditioned_inputs(P, M, rng)
    ref, mean = longdouble_cov(x)
    rows = special_rows(P)
    assert len(rows["identical"]) == (2 if P > COV_TILE else 1)
    if P > COV_TILE:
        for kind in ("identical", "negated", "shifted"):
            (a0, b0), (a1, b1) = rows[kind]
            assert a0 // COV_TILE == b0 // COV_TILE and a1 // COV_TILE != b1 // COV_TILE
        assert rows["constant"][1][1] // COV_TILE == cov_plan(M, P).nb - 1
    results = {"host": ctx.covariance(x)}
    with OnDevice(ctx, x, 0) as dev:
        got_mean, _ = dev.moments()
        results["dev+0"] = dev.covariance()
    if M % 2 == 0:
        assert not cov_plan(M, P, aligned16=False).even
        with OnDevice(ctx, x, 8) as dev:
            results["dev+8"] = dev.covariance()
    for name, got in results.items():
        check_cov(got, ref, mean, M, f"ill-conditioned P={P} M={M} {name}", say)
        for _, c in rows["constant"]:
            assert got_mean[c] == x[c, 0], (name, "constant row's mean", c)
            assert not got[c].any() and not got[:, c].any(), (name, "constant row", c)
        for i, j in rows["identical"]:
            assert len({got[a, b].tobytes() for a in (i, j) for b in (i, j)}) == 1, (name, "identical", i, j)
            assert np.array_equal(bits(got[i]), bits(got[j])), (name, "identical rows", i, j)
    assert np.array_equal(bits(results["host"]), bits(results["dev+0"]))


def test_cov_same_bits_on_fresh_and_grown_context(ctx):
    from mcmc_ref_hip import _ffi
    rng = np.random.default_rng(77)
    x = ill_conditioned_inputs(257, 4001, rng)
    ctx.covariance(exact_cov_inputs(640, 4000, rng)[0])        # grows this context's stage and workspace
    ctx.two_sample(rng.normal(size=(3, 20000)), rng.normal(size=(3, 9000)))
    grown = ctx.covariance(x)
    with _ffi.Context(0) as fresh:
        first = fresh.covariance(x)
    assert np.array_equal(bits(first), bits(grown))


@pytest.mark.parametrize("M", [4001, 4000])
def test_cov_non_finite_draws_stay_in_their_row(ctx, say, M):
    """numpy parity: a NaN or infinity poisons its own row and column and nothing else.  Row 0 matters because padding
    rows of a ragged block read row 0 and are masked by a select."""
    P = 130
    rng = np.random.default_rng(M)
    clean = (rng.normal(size=(P, P)) @ rng.normal(size=(P, M))) * 10.0 ** rng.integers(-3, 4, size=(P, 1)) \
        + rng.normal(size=(P, 1)) * 50.0
    ref, mean = longdouble_cov(clean)
    assert cov_plan(M, P).nb == 2 and (P - 1) // COV_TILE == 1 and P % COV_TILE
    places = [(0, 7), (P - 1, 100), (0, M - 1), (P - 1, M - 1), (5, M - 1)]
    for poison in (np.nan, np.inf, -np.inf):
        for row, col in places:
            x = clean.copy()
            x[row, col] = poison
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                exp = np.cov(x, ddof=0)
            finite = np.isfinite(exp)
            hit = np.zeros((P, P), dtype=bool)
            hit[row, :] = hit[:, row] = True
            assert np.array_equal(finite, ~hit)
            for name, got in (("host", ctx.covariance(x)),):
                what = (name, poison, row, col)
                assert not np.isfinite(got[~finite]).any(), what
                assert np.isfinite(got[finite]).all(), (what, np.argwhere(finite & ~np.isfinite(got))[:5])
                patched = np.where(finite, got, ref.astype(np.float64))
                check_cov(patched, ref, mean, M, f"non-finite {what}", lambda s: None)
            with OnDevice(ctx, x, 0) as dev:
                got = dev.covariance()
                assert np.array_equal(np.isfinite(got), finite), ("dev", poison, row, col)
    say(f"cov non-finite M={M}: {3 * len(places)} poisoned inputs, every other row finite and within the bound")


# =====================================================================================================================
# two-sample
# =====================================================================================================================
def check_two_sample(ctx, r, a, what, say, rel12=True):
    """KS in bits, W1 within w1_tolerance of exact_w1 (and exactly zero where the bound is zero); rel12: also the
    project's rel = 1e-12.  Returns the largest |err| / bound."""
    r, a = np.atleast_2d(r), np.atleast_2d(a)
    ks, w1 = ctx.two_sample(r, a)
    worst = 0.0
    for p in range(len(r)):
        assert ks[p] == expected_ks(r[p], a[p]), (what, p, "ks", ks[p], exact_ks_numerator(r[p], a[p]))
        w = exact_w1(r[p], a[p])
        tol = w1_tolerance(r[p], a[p], w)
        err = float(abs(np.longdouble(w1[p]) - w))
        if tol == 0.0:
            assert w1[p] == 0.0, (what, p, "w1 where the bound is zero", w1[p])
        else:
            worst = max(worst, err / tol)
        assert err <= tol, (what, p, "w1", w1[p], float(w), err, tol)
        if rel12:
            assert err <= 1e-12 * float(w) + 0.0, (what, p, "w1 rel 1e-12", w1[p], float(w))
    say(f"two-sample {what}: max |w1 err| / bound = {worst:.3g}")
    return ks, w1


SIZES = [1, 4095, 4096, 4097, 8192, 12288, 70001]


@pytest.mark.parametrize("Mr", SIZES)
def test_two_sample_disjoint_supports(ctx, say, Mr):
    """All reference draws below all actual draws (row 0) and the reverse (row 1): every merge block but at most one
    holds a single sample, and where the lower sample's length is a multiple of 4096 a block boundary is the end of a
    sample, so the block before it has no look-ahead draw from its own sample."""
    rng = np.random.default_rng(Mr)
    boundary = 0
    for Ma in SIZES:
        lo_r, hi_a = rng.uniform(0, 1, size=Mr), rng.uniform(2, 3, size=Ma)
        hi_r, lo_a = rng.uniform(2, 3, size=Mr), rng.uniform(0, 1, size=Ma)
        r, a = np.stack([lo_r, hi_r]), np.stack([hi_a, lo_a])
        nblk = two_sample_blocks(Mr, Ma)
        assert nblk == -(-(Mr + Ma) // MERGE_TILE)
        # blocks wholly inside one sample, for the sample that comes first in the pooled order being Mr or Ma long
        for first in (Mr, Ma):
            single = sum(1 for b in range(nblk)
                         if min((b + 1) * MERGE_TILE, Mr + Ma) <= first or b * MERGE_TILE >= first)
            assert single >= nblk - 1
            boundary += first % MERGE_TILE == 0               # a block boundary that is the end of the lower sample
        ks, w1 = check_two_sample(ctx, r, a, f"disjoint Mr={Mr} Ma={Ma} blocks={nblk}", say)
        assert ks[0] == 1.0 and ks[1] == 1.0
        for p in range(2):
            assert w1[p] == pytest.approx(abs(a[p].mean() - r[p].mean()), rel=1e-12)
    assert boundary == 3 + (len(SIZES) if Mr % MERGE_TILE == 0 else 0)   # Ma in {4096, 8192, 12288}; every Ma for such an Mr


def test_two_sample_extreme_imbalance(ctx, say):
    assert 1 in SIZES and 70001 in SIZES and two_sample_blocks(1, 70001) == 18
    rng = np.random.default_rng(9)
    one, many = np.array([[0.3]]), rng.normal(size=(1, 70001))
    check_two_sample(ctx, one, many, "1 inside 70001", say)
    check_two_sample(ctx, many, one, "70001 around 1", say)


def test_two_sample_nested_supports(ctx, say):
    """One sample wholly inside a gap of the other: whole blocks of one sample on both sides of the other's."""
    rng = np.random.default_rng(10)
    outer = np.concatenate([rng.uniform(0, 1, size=6000), rng.uniform(2, 3, size=6000)])
    inner = rng.uniform(1.4, 1.6, size=9000)
    pooled_is_outer = np.concatenate([np.ones(6000, bool), np.zeros(9000, bool), np.ones(6000, bool)])
    nblk = two_sample_blocks(len(outer), len(inner))
    kinds = [set(pooled_is_outer[b * MERGE_TILE:(b + 1) * MERGE_TILE]) for b in range(nblk)]
    assert nblk == 6 and kinds[0] == {True} and kinds[2] == {False} and kinds[4] == {True} and kinds[1] == {True, False}
    check_two_sample(ctx, outer, inner, "inner sample is the actual one", say)
    check_two_sample(ctx, inner, outer, "inner sample is the reference", say)


def _run_covers_a_block(r, a, value) -> bool:
    v = np.sort(np.concatenate([r, a]))
    lo, hi = np.searchsorted(v, value, side="left"), np.searchsorted(v, value, side="right")
    return any(lo <= b * MERGE_TILE and (b + 1) * MERGE_TILE <= hi for b in range(two_sample_blocks(len(r), len(a))))


def test_two_sample_runs_longer_than_a_block(ctx, say):
    """A value repeated 10 000 times: at least one merge block lies entirely inside the run and must contribute
    nothing (its last value's successor, the look-ahead draw, is equal to it)."""
    rng = np.random.default_rng(11)
    run = np.full(10000, 0.25)
    for where in ("reference", "actual", "both"):
        r = np.concatenate([rng.normal(size=3000), run]) if where != "actual" else rng.normal(size=5000)
        a = np.concatenate([rng.normal(size=2000), run]) if where != "reference" else rng.normal(size=5000)
        r, a = rng.permutation(r), rng.permutation(a)
        assert _run_covers_a_block(r, a, 0.25)
        check_two_sample(ctx, r, a, f"run of 10000 in {where}", say)
    c, d = np.full(5000, 1.5), np.full(7000, 1.5)
    assert _run_covers_a_block(c, d, 1.5) and two_sample_blocks(5000, 7000) == 3
    ks, w1 = check_two_sample(ctx, c, d, "both constant and equal", say)
    assert ks[0] == 0.0 and w1[0] == 0.0
    ks, w1 = check_two_sample(ctx, c, d + 2.25, "both constant and different", say)
    assert ks[0] == 1.0 and w1[0] == 2.25
    ks, w1 = check_two_sample(ctx, c + 2.25, d, "both constant and different, reversed", say)
    assert ks[0] == 1.0 and w1[0] == 2.25


@pytest.mark.parametrize("n", [4095, 4096, 4097, 4098])
def test_two_sample_run_ending_at_a_block_boundary(ctx, say, n):
    """The pooled order starts with n equal values (3000 of them reference draws): the run ends on pooled element
    n - 1, just before, on and just after the first block boundary."""
    rng = np.random.default_rng(n)
    r = np.concatenate([np.zeros(3000), 0.1 + np.abs(rng.normal(size=2500))])
    a = np.concatenate([np.zeros(n - 3000), 0.1 + np.abs(rng.normal(size=3000))])
    v = np.sort(np.concatenate([r, a]))
    assert v[n - 1] == 0.0 and v[n] > 0.0 and two_sample_blocks(len(r), len(a)) == 3
    check_two_sample(ctx, rng.permutation(r), rng.permutation(a), f"run of {n} from the start", say)


@pytest.mark.parametrize("total", [4095, 4096, 4097, 8191, 8192, 8193])
def test_two_sample_total_length(ctx, say, total):
    rng = np.random.default_rng(total)
    Mr = total // 3
    Ma = total - Mr
    assert two_sample_blocks(Mr, Ma) == {4095: 1, 4096: 1, 4097: 2, 8191: 2, 8192: 2, 8193: 3}[total]
    r, a = rng.normal(size=(2, Mr)), rng.normal(loc=0.1, scale=1.2, size=(2, Ma))
    r[1], a[1] = np.round(r[1], 1), np.round(a[1], 1)
    check_two_sample(ctx, r, a, f"total {total}", say)
    check_two_sample(ctx, a, r, f"total {total} swapped", say)


def test_two_sample_scaled_and_offset_values(ctx, say):
    rng = np.random.default_rng(12)
    r, a = rng.normal(size=(2, 10000)), rng.normal(loc=0.1, scale=1.2, size=(2, 7000))
    r[1], a[1] = np.round(r[1], 1), np.round(a[1], 1)
    assert two_sample_blocks(10000, 7000) == 5
    check_two_sample(ctx, r * 1e-300, a * 1e-300, "times 1e-300", say)
    check_two_sample(ctx, r * (1e300 / 8), a * (1e300 / 8), "times 1e300 / 8", say)
    # gaps of a few ulp: W1 is checked through the first term of the bound
    check_two_sample(ctx, r + 1e15, a + 1e15, "offset 1e15", say, rel12=False)
    near = rng.normal(size=100000)
    check_two_sample(ctx, near, near + 1e-9 * rng.normal(size=100000), "near-identical, 100000 draws", say)


def test_two_sample_65535_parameters(ctx, say):
    P = 65535
    rng = np.random.default_rng(13)
    r, a = rng.normal(size=(P, 8)), rng.normal(loc=0.1, scale=1.2, size=(P, 8))
    r[::2], a[::2] = np.round(r[::2], 1), np.round(a[::2], 1)
    num, w = exact_two_sample_rows(r, a)
    ks, w1 = ctx.two_sample(r, a)
    assert np.array_equal(ks, num.astype(np.float64) / (8.0 * 8.0))
    span = np.maximum(r.max(axis=1), a.max(axis=1)) - np.minimum(r.min(axis=1), a.min(axis=1))
    tol = (4 * 2.0 ** -53 * span + (8 + 8 + 8) * EPS * w).astype(np.float64)
    err = np.abs(w1 - w).astype(np.float64)
    say(f"two-sample P=65535: max |w1 err| / bound = {(err / tol).max():.3g}")
    assert np.all(err <= tol) and np.all(err <= 1e-12 * w.astype(np.float64))


def test_two_sample_size_rejections(ctx):
    """P > 65535, a sample of 2^32 - 1 draws and Mr Ma >= 2^53 are refused before any buffer is read."""
    from mcmc_ref_hip import _ffi
    dp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    short, ks, w1 = np.zeros(8), np.zeros(8), np.zeros(8)

    def call(Mr, Ma, P):
        rc = ctx.lib.mcr_two_sample(ctx.handle, dp(short), Mr, dp(short), Ma, P, dp(ks), dp(w1))
        return rc, (ctx.lib.mcr_last_error(ctx.handle) or b"").decode()

    rc, msg = call(1, 1, 65536)
    assert rc == _ffi.MCR_EINVAL and "65535" in msg
    for Mr, Ma in [(2 ** 32 - 1, 1), (1, 2 ** 32 - 1), (94906266, 94906266)]:
        assert Mr >= 2 ** 32 - 1 or Ma >= 2 ** 32 - 1 or float(Mr) * float(Ma) >= 2.0 ** 53
        rc, msg = call(Mr, Ma, 1)
        assert rc == _ffi.MCR_EINVAL and "2^53" in msg, (Mr, Ma, rc, msg)
    assert 94906265 * 94906265 < 2 ** 53 <= 94906266 * 94906266
    ks, w1 = ctx.two_sample(np.array([[1.0, 2.0]]), np.array([[1.5]]))      # the context still answers
    assert ks[0] == 0.5 and w1[0] == 0.5
