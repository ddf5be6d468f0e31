"""References and host-side geometry for the extension kernels (covariance, two-sample KS / Wasserstein-1), pinned on
the CPU so that a wrong reference cannot pass for a right kernel.  tests/test_ext_edges_gpu.py imports from here.

* `cov_plan`, `two_sample_blocks` restate the launch arithmetic of `mcr_covariance_dev` / `mcr_two_sample`
  (mcr_stats.hip): the GPU tests assert through them that a shape still reaches the edge it was chosen for.
* `exact_cov_inputs`: integer-valued draws whose population covariance is exact in f64 in ANY summation order.
* `longdouble_cov`, `cov_tolerance`: a two-pass extended-precision covariance for real-valued draws and the per-entry
  bound the kernel is held to (no max-norm term: every entry is judged on the scale of its own two parameters).
* `exact_ks_numerator`, `exact_w1`: the KS statistic as the exact rational the kernel forms, and Wasserstein-1 in
  extended precision with the CDF difference taken from the integer numerator.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import pytest

EPS = 2.0 ** -52
COV_TILE, COV_STEP, MERGE_TILE = 128, 16, 4096     # kCovBM, kCovBK (mcr_ext.hpp); kTile (mcr_pipe.hpp)
COV_MAX_P = 8192


# ---------------------------------------------------------------------------------------------------------------------
# host-side geometry
# ---------------------------------------------------------------------------------------------------------------------
class CovPlan(NamedTuple):
    nb: int             # block rows of 128 parameters
    tiles: int          # workgroups per draw slice: tiles on or above the block diagonal
    ksplit: int         # draw slices actually launched
    kchunk: int         # draws per slice (a multiple of 16)
    even: bool          # the EVEN instantiation (16-byte loads): M even and the pointer 16-byte aligned
    S: int              # slices of the moments kernel that supplies the means
    ksplit_wanted: int  # slices before the 128 MB cap on the partial tiles
    cap: int            # the cap as computed, before its clamp to 1 (0 above P = 4096)


def cov_plan(M: int, P: int, aligned16: bool = True) -> CovPlan:
    """mcr_covariance_dev's launch arithmetic."""
    nb = -(-P // COV_TILE)
    p64 = nb * COV_TILE
    tiles = nb * (nb + 1) // 2
    ksplit = -(-512 // tiles)
    maxsplit = -(-M // (16 * COV_STEP))
    ksplit = min(ksplit, maxsplit)
    wanted = ksplit
    cap = (128 << 20) // (p64 * p64 * 8)
    if ksplit > cap:
        ksplit = max(cap, 1)
    ksplit = max(ksplit, 1)
    kchunk = -(-M // ksplit)
    kchunk = -(-kchunk // COV_STEP) * COV_STEP
    ksplit = -(-M // kchunk)
    return CovPlan(nb, tiles, ksplit, kchunk, M % 2 == 0 and aligned16, 8 if M >= 16384 else 1, wanted, cap)


def last_slice_draws(M: int, P: int) -> int:
    pl = cov_plan(M, P)
    return M - (pl.ksplit - 1) * pl.kchunk


def m_with_last_slice(P: int, last: int, lo: int = 300, hi: int = 40000) -> int:
    """The smallest M in [lo, hi) whose covariance plan has at least two draw slices, the last one of `last` draws.
    Slices are multiples of 16 draws, so M has the parity of `last`."""
    for M in range(lo, hi):
        if cov_plan(M, P).ksplit >= 2 and last_slice_draws(M, P) == last:
            return M
    raise AssertionError((P, last))


def two_sample_blocks(Mr: int, Ma: int) -> int:
    """Merge blocks of k_two_sample: 4096 pooled draws each."""
    return -(-(Mr + Ma) // MERGE_TILE)


# ---------------------------------------------------------------------------------------------------------------------
# covariance references
# ---------------------------------------------------------------------------------------------------------------------
def exact_cov_inputs(P: int, M: int, rng):
    """(x, off, D): x[p] = off[p] + D[p] with D integers in [-1000, 1000] in adjacent negated pairs
    (D[p, 2k + 1] = -D[p, 2k], a final 0 when M is odd), off[p] distinct integer multiples of 8.  Every even-aligned,
    even-length stretch of a row sums to off[p] times its length exactly, so the exact mean is off[p], the centred
    draws are D, and G = D @ D.T is an integer matrix below 2^53 whatever the order of summation."""
    assert M * 1000 * 1000 < 2 ** 53
    D = np.zeros((P, M))
    half = rng.integers(-1000, 1001, size=(P, M // 2)).astype(np.float64)
    D[:, 0:2 * (M // 2):2] = half
    D[:, 1:2 * (M // 2):2] = -half
    off = 8.0 * (17 * np.arange(P) - 5 * P)
    assert len(np.unique(off)) == P
    x = D + off[:, None]
    assert np.array_equal(x - off[:, None], D)
    return x, off, D


def exact_cov_ref(D: np.ndarray) -> np.ndarray:
    """The exact population covariance of exact_cov_inputs, correctly rounded: one division of an exact integer."""
    return (D @ D.T) / float(D.shape[1])


def longdouble_cov(x: np.ndarray):
    """(cov, mean) of x [P][M], two-pass in np.longdouble (with the mean's residual folded back in)."""
    xl = np.asarray(x, dtype=np.longdouble)
    M = xl.shape[1]
    mean = xl.sum(axis=1) / M
    c = xl - mean[:, None]
    corr = c.sum(axis=1) / M
    mean = mean + corr
    c = c - corr[:, None]
    g = np.empty((len(c), len(c)), dtype=np.longdouble)
    for i in range(len(c)):                                    # the upper triangle, mirrored: half the products
        g[i, i:] = c[i:] @ c[i]
        g[i:, i] = g[i, i:]
    return g / M, mean


def cov_tolerance(ref, mean, M: int) -> np.ndarray:
    """Per-entry bound |got_ij - ref_ij| <= (M + 8) eps u_ij + d_i d_j with u_ij = sqrt(c_ii c_jj) and
    d_i = 2 spacing(|mean_i|) + 16 eps sqrt(c_ii).

    First term: each centred operand carries one rounding, at most M products are accumulated per entry in some
    order across the draw slices, then one division -- Higham's gamma_M sum|terms|, and Cauchy-Schwarz gives
    sum|x - mu||y - nu| / M <= u_ij.  Second term: an error delta_i of the mean enters only as delta_i delta_j (the
    first-order terms multiply sum(x - mu) = 0); d_i is the bound the moments kernel is held to
    (tests/test_strides_gpu.py, assert_moments)."""
    sd = np.sqrt(np.diag(np.asarray(ref, dtype=np.float64)))
    d = 2 * np.spacing(np.abs(np.asarray(mean, dtype=np.float64))) + 16 * EPS * sd
    return (M + 8) * EPS * np.outer(sd, sd) + np.outer(d, d)


def special_rows(P: int):
    """Placement of the special rows of ill_conditioned_inputs: {kind: [(source row, derived row), ...]}, each kind
    once inside the first 128-block and, when P has more than one block, once across the last two blocks.  Pairs lie an even
    number of rows apart, so that with an odd M both rows start on the same 16-byte phase and the moments kernel
    reads them with the same kind of load."""
    inside = {"constant": (None, 3), "identical": (5, 9), "negated": (6, 12), "shifted": (7, 15)}
    out = {k: [v] for k, v in inside.items()}
    if P > COV_TILE:
        src = (P - 1) // COV_TILE * COV_TILE          # first row of the last (ragged) block, shared by the three kinds
        near = src - COV_TILE                          # derived rows one block above it: tile (nb - 2, nb - 1)
        out["constant"].append((None, P - 1))
        out["identical"].append((src, near + 30))
        out["negated"].append((src, near + 32))
        out["shifted"].append((src, near + 34))
    return out


def ill_conditioned_inputs(P: int, M: int, rng, special: bool = True) -> np.ndarray:
    """Correlated rows (L @ z), scaled per parameter by 10^k, k in [-6, 6], offset by up to 10^6 standard deviations;
    plus the special rows of special_rows(P)."""
    L = rng.normal(size=(P, P)) / np.sqrt(P)
    x = L @ rng.normal(size=(P, M))
    scale = 10.0 ** rng.integers(-6, 7, size=P)
    scale[:13] = 10.0 ** np.arange(-6, 7)[:min(P, 13)]
    sign = np.where(rng.random(P) < 0.5, -1.0, 1.0)
    offset = sign * scale * 10.0 ** rng.uniform(0, 6, size=P)
    offset[0] = scale[0] * 1e6
    x = x * scale[:, None] + offset[:, None]
    if special:
        for kind, places in special_rows(P).items():
            for src, dst in places:
                if kind == "constant":
                    x[dst] = offset[dst]
                elif kind == "identical":
                    x[dst] = x[src]
                elif kind == "negated":
                    x[dst] = -x[src]
                else:
                    x[dst] = x[src] + 3.0 * scale[src]
    return x


# ---------------------------------------------------------------------------------------------------------------------
# two-sample references
# ---------------------------------------------------------------------------------------------------------------------
def _cdf_numerators(r, a, at):
    rs, as_ = np.sort(r), np.sort(a)
    i = np.searchsorted(rs, at, side="right").astype(np.int64)
    j = np.searchsorted(as_, at, side="right").astype(np.int64)
    assert float(len(rs)) * float(len(as_)) < 2.0 ** 53
    return np.abs(i * np.int64(len(as_)) - j * np.int64(len(rs)))


def exact_ks_numerator(r, a) -> int:
    """max |i Ma - j Mr| over the pooled distinct values v, i = #(r <= v), j = #(a <= v): the KS statistic is this
    integer over Mr Ma."""
    r, a = np.asarray(r, dtype=np.float64), np.asarray(a, dtype=np.float64)
    return int(_cdf_numerators(r, a, np.unique(np.concatenate([r, a]))).max())


def expected_ks(r, a) -> float:
    """The statistic as the kernel forms it: the exact numerator divided once by the f64 product Mr Ma."""
    return float(exact_ks_numerator(r, a)) / (float(len(r)) * float(len(a)))


def exact_w1(r, a):
    """sum |i/Mr - j/Ma| (v[t+1] - v[t]) over the pooled sorted values in np.longdouble, the CDF difference taken from
    the integer numerator."""
    r, a = np.asarray(r, dtype=np.float64), np.asarray(a, dtype=np.float64)
    v = np.sort(np.concatenate([r, a]))
    if len(v) < 2:
        return np.longdouble(0)
    num = _cdf_numerators(r, a, v[:-1]).astype(np.longdouble)
    gaps = np.diff(v.astype(np.longdouble))
    return (num * gaps).sum() / (np.longdouble(len(r)) * np.longdouble(len(a)))


def exact_two_sample_rows(r, a):
    """(KS numerators, W1) of every row of r [P][Mr], a [P][Ma] at once, for short samples: the same definitions by
    direct counting."""
    r, a = np.asarray(r, dtype=np.float64), np.asarray(a, dtype=np.float64)
    Mr, Ma = r.shape[1], a.shape[1]
    v = np.sort(np.concatenate([r, a], axis=1), axis=1)
    i = (r[:, None, :] <= v[:, :, None]).sum(axis=2).astype(np.int64)
    j = (a[:, None, :] <= v[:, :, None]).sum(axis=2).astype(np.int64)
    num = np.abs(i * Ma - j * Mr)
    gaps = np.diff(v.astype(np.longdouble), axis=1)
    w1 = (num[:, :-1].astype(np.longdouble) * gaps).sum(axis=1) / (np.longdouble(Mr) * np.longdouble(Ma))
    return num.max(axis=1), w1


def w1_tolerance(r, a, w1) -> float:
    """|got - exact_w1| <= 4 * 2^-53 (v_max - v_min) + (Mr + Ma + 8) 2^-52 exact_w1.  First term: the kernel rounds i/Mr,
    j/Ma and their difference, about three half-ulps of a number that is at most 1, on every gap.  Second term: the
    summation of non-negative terms."""
    lo, hi = min(np.min(r), np.min(a)), max(np.max(r), np.max(a))
    return float(4 * 2.0 ** -53 * (np.longdouble(hi) - np.longdouble(lo))
                 + (len(r) + len(a) + 8) * EPS * np.longdouble(w1))


# =====================================================================================================================
# the tests that pin the above
# =====================================================================================================================
def test_cov_plan_reaches_the_edges_the_gpu_tests_name():
    assert [cov_plan(4000, P).nb for P in (127, 128, 129, 255, 256, 257, 384, 640, 1000)] == [1, 1, 2, 2, 2, 3, 3, 5, 8]
    pl = cov_plan(40000, 1000)
    assert (pl.nb, pl.tiles, pl.ksplit, pl.kchunk, pl.even, pl.S) == (8, 36, 15, 2672, True, 8)
    # the 128 MB cap first bites at nb = 15: 120 tiles want 5 slices, 1920^2 doubles fit 4 times
    assert [P for P in range(1, 2049) if cov_plan(2048, P).ksplit_wanted > cov_plan(2048, P).cap][0] == 1793
    pl = cov_plan(2048, 1900)
    assert (pl.nb, pl.tiles, pl.ksplit_wanted, pl.cap, pl.ksplit, pl.kchunk) == (15, 120, 5, 4, 4, 512)
    pl = cov_plan(4096, 2048)
    assert (pl.nb, pl.ksplit_wanted, pl.cap, pl.ksplit) == (16, 4, 4, 4)
    pl = cov_plan(4096, 4096)
    assert (pl.nb, pl.tiles, pl.cap, pl.ksplit, pl.kchunk) == (32, 528, 1, 1, 4096)
    pl = cov_plan(512, 8192)
    assert (pl.nb, pl.tiles, pl.ksplit_wanted, pl.cap, pl.ksplit, pl.kchunk) == (64, 2080, 1, 0, 1, 512)
    assert cov_plan(512, 4097).cap == 0 and cov_plan(512, 4096).cap == 1
    # maxsplit: one slice up to 256 draws, two from 257
    assert [cov_plan(M, 129).ksplit for M in (1, 255, 256, 257, 511, 513)] == [1, 1, 1, 2, 2, 3]
    assert [cov_plan(M, 129).kchunk for M in (1, 15, 16, 17, 257)] == [16, 16, 16, 32, 144]
    assert [cov_plan(M, 129).S for M in (16383, 16384, 16385)] == [1, 8, 8]
    assert cov_plan(4000, 129).even and not cov_plan(4000, 129, aligned16=False).even and not cov_plan(4001, 129).even
    # every slice but the last is full, and the slices cover M
    for M in (1, 17, 256, 257, 4000, 4001, 16385, 40000):
        for P in (1, 129, 1000, 1900, 4096):
            pl = cov_plan(M, P)
            assert pl.kchunk % 16 == 0 and (pl.ksplit - 1) * pl.kchunk < M <= pl.ksplit * pl.kchunk
            assert pl.ksplit * (pl.nb * 128) ** 2 * 8 <= max(128 << 20, (pl.nb * 128) ** 2 * 8)


def test_last_slice_search():
    for P in (129, 257):
        for last in (1, 2, 14, 15, 16, 17, 18):
            M = m_with_last_slice(P, last)
            pl = cov_plan(M, P)
            assert pl.ksplit >= 2 and M - (pl.ksplit - 1) * pl.kchunk == last and M % 2 == last % 2


def test_two_sample_blocks():
    assert [two_sample_blocks(1, M) for M in (1, 4094, 4095, 4096, 8191, 8192)] == [1, 1, 1, 2, 2, 3]
    assert two_sample_blocks(70001, 70001) == 35


def test_exact_cov_inputs_are_order_independent():
    rng = np.random.default_rng(11)
    for P, M in [(7, 64), (130, 4001), (257, 4000)]:
        x, off, D = exact_cov_inputs(P, M, rng)
        assert np.all(D == np.round(D)) and np.abs(D).max() <= 1000 and np.all(off % 8 == 0)
        assert np.array_equal(D[:, 1:2 * (M // 2):2], -D[:, 0:2 * (M // 2):2]) and (M % 2 == 0 or np.all(D[:, -1] == 0))
        for b, e in [(0, 2), (0, M // 2 * 2), (2, 66), (M // 4 * 2, M // 2 * 2)]:
            assert np.all(D[:, b:e].sum(axis=1) == 0)
        G = D @ D.T
        assert np.array_equal(G, D[:, ::-1] @ D[:, ::-1].T)
        perm = rng.permutation(M)
        assert np.array_equal(G, D[:, perm] @ D[:, perm].T)
        if P <= 130:
            Di = D.astype(np.int64)
            assert np.array_equal(G.astype(np.int64), Di @ Di.T) and np.all(G == np.round(G))
        ref = exact_cov_ref(D)
        ld, mean = longdouble_cov(x)
        assert np.array_equal(mean.astype(np.float64), off)
        assert np.array_equal(ld.astype(np.float64), ref)      # the exact rational, rounded once, either way


def test_longdouble_cov_agrees_with_exact_fractions():
    from fractions import Fraction
    rng = np.random.default_rng(12)
    x = ill_conditioned_inputs(4, 9, rng, special=False)
    ld, mean = longdouble_cov(x)
    fx = [[Fraction(float(v)) for v in row] for row in x]
    frac = lambda v: Fraction(float(v)) + Fraction(float(v - np.longdouble(float(v))))     # a longdouble, exactly
    mu = [sum(row) / 9 for row in fx]
    for i in range(4):
        assert abs(frac(mean[i]) - mu[i]) <= abs(mu[i]) * Fraction(1, 2 ** 62)
        for j in range(4):
            c = sum((fx[i][t] - mu[i]) * (fx[j][t] - mu[j]) for t in range(9)) / 9
            u = float(np.sqrt(ld[i, i] * ld[j, j]))
            assert abs(float(frac(ld[i, j]) - c)) <= 1e-17 * u


@pytest.mark.parametrize("P,M", [(37, 10001), (130, 40000)])
def test_cov_tolerance_holds_numpy_and_rejects_one_dropped_term(P, M):
    """np.cov stays well inside the bound on the ill-conditioned family; the same input with ONE draw of one
    small-scale row replaced by that row's mean (the effect of one dropped product term) falls outside it -- while the
    max-norm tolerance of test_ext_gpu.py accepts it."""
    rng = np.random.default_rng(13)
    x = ill_conditioned_inputs(P, M, rng)
    ref, mean = longdouble_cov(x)
    tol = cov_tolerance(ref, mean, M)
    ref64 = ref.astype(np.float64)
    got = np.cov(x, ddof=0)
    ratio = np.abs(got - ref).astype(np.float64) / np.where(tol > 0, tol, 1.0)
    live = np.flatnonzero(ref64.diagonal() > 0)               # numpy's mean of a constant row is a few ulp off: d_i d_j
    print(f"np.cov P={P} M={M}: max |err| / bound = {ratio.max():.3g} ({ratio[np.ix_(live, live)].max():.3g} off the "
          f"constant rows)")
    assert np.all(np.abs(got - ref) <= tol)
    row = 1                                                    # scale 1e-5
    assert np.sqrt(ref64[row, row]) < 1e-4 * np.sqrt(ref64.diagonal().max())
    y = x.copy()
    y[row, M // 3] = float(mean[row])
    bad = np.cov(y, ddof=0)
    worst = (np.abs(bad - ref).astype(np.float64) / np.where(tol > 0, tol, 1.0)).max()
    print(f"one dropped term: max |err| / bound = {worst:.3g}")
    assert worst > 1e3
    assert np.allclose(bad, ref64, rtol=1e-10, atol=1e-12 * np.abs(ref64).max())     # the old assertion does not see it


def test_exact_ks_matches_scipy_exact_mode():
    from scipy.stats import ks_2samp, wasserstein_distance
    rng = np.random.default_rng(4)
    for P, Mr, Ma in [(3, 10000, 4000), (2, 5000, 5000), (4, 37, 41), (1, 1, 1), (1, 4096, 8192), (3, 100, 100),
                      (3, 10, 10)]:
        ref = rng.normal(size=(P, Mr))
        act = rng.normal(loc=0.1, scale=1.2, size=(P, Ma))
        if P > 1:
            ref[1] = np.round(ref[1], 1); act[1] = np.round(act[1], 1)
        for p in range(P):
            assert expected_ks(ref[p], act[p]) == ks_2samp(ref[p], act[p], method="exact").statistic, (Mr, Ma, p)
            w = exact_w1(ref[p], act[p])
            assert float(w) == pytest.approx(wasserstein_distance(ref[p], act[p]), rel=1e-12, abs=1e-15)
            assert abs(wasserstein_distance(ref[p], act[p]) - w) <= w1_tolerance(ref[p], act[p], w)
    # the long shape of the GPU test: scipy has no exact mode there, the rational still agrees with its asymp value
    r, a = rng.normal(size=70000), rng.normal(loc=0.1, scale=1.2, size=9000)
    assert expected_ks(r, a) == pytest.approx(ks_2samp(r, a, method="asymp").statistic, rel=1e-13)
    assert float(exact_w1(r, a)) == pytest.approx(wasserstein_distance(r, a), rel=1e-12)


def test_two_sample_references_on_cases_with_known_answers():
    lo, hi = np.arange(5.0), 10.0 + np.arange(7.0)
    assert exact_ks_numerator(lo, hi) == 35 and expected_ks(lo, hi) == 1.0 and expected_ks(hi, lo) == 1.0
    assert float(exact_w1(lo, hi)) == pytest.approx(hi.mean() - lo.mean(), rel=1e-15)
    c = np.full(9, 2.5)
    assert exact_ks_numerator(c, c[:4]) == 0 and exact_w1(c, c[:4]) == 0 and w1_tolerance(c, c[:4], 0) == 0.0
    assert expected_ks(c, c + 1) == 1.0 and exact_w1(c, c[:4] + 1) == 1
    # by hand: r = {0, 0, 1}, a = {0, 2}: at 0 |2/3 - 1/2|, at 1 |1 - 1/2|; W1 = 1/6 * 1 + 1/2 * 1
    r, a = np.array([0.0, 1.0, 0.0]), np.array([2.0, 0.0])
    assert exact_ks_numerator(r, a) == 3 and float(exact_w1(r, a)) == pytest.approx(1 / 6 + 1 / 2, rel=1e-15)
    # a brute-force CDF walk agrees on ties
    rng = np.random.default_rng(5)
    r, a = np.round(rng.normal(size=300), 1), np.round(rng.normal(size=200), 1)
    vals = np.unique(np.concatenate([r, a]))
    num = max(abs(int((r <= v).sum()) * 200 - int((a <= v).sum()) * 300) for v in vals)
    assert exact_ks_numerator(r, a) == num
    w = sum(abs((r <= v).sum() / 300 - (a <= v).sum() / 200) * (vals[t + 1] - v) for t, v in enumerate(vals[:-1]))
    assert float(exact_w1(r, a)) == pytest.approx(w, rel=1e-13)


def test_row_batched_two_sample_reference():
    rng = np.random.default_rng(6)
    r, a = rng.normal(size=(50, 8)), np.round(rng.normal(size=(50, 8)), 1)
    r[:, ::3] = np.round(r[:, ::3], 1)
    num, w1 = exact_two_sample_rows(r, a)
    for p in range(50):
        assert num[p] == exact_ks_numerator(r[p], a[p])
        assert float(abs(w1[p] - exact_w1(r[p], a[p]))) <= 1e-18 * float(w1[p])
