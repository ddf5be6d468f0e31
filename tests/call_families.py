"""The families of public calls that carve the context's buffers, one entry each, for the tests that run every entry
behind every other on one context (test_call_order_gpu.py) and for the CPU test that keeps this list complete and its
inputs honest (test_call_families_cpu.py).  A plain module: no GPU and no library is touched at import.

A family has

* `inputs(size)` for size in SIZES = ("small", "large"): built once from a seed of its own (7000 + 100 * index, + 1 for
  large) and cached, never changed afterwards;
* `run(ctx, inputs)`: ONE public call (the moments family: the device-tensor and the flat-array moments, two calls) whose
  result compares with `==`: a dict of fields, every array as (dtype, shape, bytes), so floats compare as bit patterns;
* `check(inputs, got, ctx)`: the result against the family's reference at the gate of the family's own tests, both imported
  from the sibling test modules -- nothing is restated here.  `ctx` is the context that produced `got`; only the host's
  re-reading of the draws files uses it (as test_context_buffers_gpu.Ingest.check_host does);
* `symbols`: the entries of the C ABI its run reaches, and `pooled(size)`: the length its sort works on (None: no sort).

Sizes.  small: an odd pooled length below one sort tile (4096) that no other family's small size has, P = 3; large: for
the families that sort, 4 x 16 385 = 65 540 pooled draws (32-bit positions, seventeen tiles, merge passes) with P = 2, for
the others the second size their own edge tests use.  Large draws are offset by 1000 * (index + 1) where the statistic
allows, so that a word a large call left behind is never a plausible value of the small call that follows.

The entries of the four ABI tables are placed here: `_abi.SYMBOLS` (mcr_*), `_xabi.XSYMBOLS` (mcrx_*: they carve the main
context's lane workspace), `_iabi.ISYMBOLS` (mci_*) and `_babi.BSYMBOLS` (mcb_*), the last two in companion libraries whose
handles -- one per Context, each with buffers of its own that only grow -- the families reach through
`indicator._handle(ctx)` and `batchmeans._handle(ctx)`.

REFUSED: calls that end in a documented error, most of them after device work has run, and one that stops part-way with
MCR_OK and says so in its result.
"""
from __future__ import annotations

import atexit
import ctypes as C
import shutil
import tempfile
from pathlib import Path

import numpy as np

SIZES = ("small", "large")
TILE = 4096                     # draws of a sort tile
WIDE = 65536                    # pooled lengths from here on carry 32-bit positions
BIG_LIMIT = 8 << 30             # the workspace limit the tests restore (as test_hip_parity and test_csv_write_gpu do)


# ---- results that compare with == ------------------------------------------------------------------------------------

def pack(fields: dict) -> dict:
    """Every array (or scalar) of `fields` as (dtype, shape, bytes); anything else as it is."""
    out = {}
    for k, v in fields.items():
        if isinstance(v, (np.ndarray, np.generic, float, int)) and not isinstance(v, bool):
            a = np.asarray(v)
            out[k] = (a.dtype.str, a.shape, np.ascontiguousarray(a).tobytes())      # (a scalar keeps the shape ())
        else:
            out[k] = v
    return out


def unpack(got: dict) -> dict:
    out = {}
    for k, v in got.items():
        if isinstance(v, tuple) and len(v) == 3 and isinstance(v[2], bytes):
            out[k] = np.frombuffer(v[2], dtype=np.dtype(v[0])).reshape(v[1]).copy()
        else:
            out[k] = v
    return out


def first_difference(got, want) -> str:
    """The name of the first output field in which two results of one family differ ("" if none)."""
    if isinstance(got, dict) and isinstance(want, dict):
        for k in want:
            if k not in got or got[k] != want[k]:
                return str(k)
        return next((str(k) for k in got if k not in want), "")
    if isinstance(got, (tuple, list)) and isinstance(want, (tuple, list)):
        for i, (a, b) in enumerate(zip(got, want)):
            if a != b:
                return f"[{i}]"
        return "" if len(got) == len(want) else "length"
    return "" if got == want else "value"


# ---- shared state: the oracle, the files -----------------------------------------------------------------------------

_STATE: dict = {}


def oracle():
    if "oracle" not in _STATE:
        from oracle import oracle as orc
        orc.build()
        _STATE["oracle"] = orc
    return _STATE["oracle"]


def workdir() -> Path:
    if "dir" not in _STATE:
        _STATE["dir"] = Path(tempfile.mkdtemp(prefix="call_families_"))
        atexit.register(shutil.rmtree, _STATE["dir"], ignore_errors=True)
    return _STATE["dir"]


def ingest():
    """The files and texts of test_context_buffers_gpu.Ingest, both sizes, written once.  The small JSON document and the
    small table CSV of this instance hold an all-integer column beside a real one: the decoders' per-column "not an
    integer" words are cleared per call, and only a column whose word has to stay clear shows one that was not."""
    if "ingest" not in _STATE:
        import test_csv_table_gpu as TT
        import test_json_gpu as TJ
        from test_context_buffers_gpu import Ingest
        i = _STATE["ingest"] = Ingest(workdir(), oracle())
        doc = TJ.iid_document(6, 2, 3, 1, int_column=True)
        i.f["json", "small"] = dict(text=doc, path=TJ.archive(workdir(), "small_int", doc))
        data = TT.write_table(2, 3, 2, "mixed", "both", TT.ENDS[0], 4)
        i.f["table_csv", "small"] = dict(data=data, path=TT.put(workdir(), "small_mixed_table", data))
        assert len(doc) < 1000 and len(data) < 1000
    return _STATE["ingest"]


# ---- the families ----------------------------------------------------------------------------------------------------

class Family:
    name = ""
    symbols: tuple = ()
    sorts = False               # a sort stage runs: the large size has at least WIDE + 1 pooled draws

    def __init__(self, index: int):
        self.index = index
        self._inputs: dict = {}

    def seed(self, size: str) -> int:
        return 7000 + 100 * self.index + SIZES.index(size)

    def offset(self, size: str) -> float:
        return 1000.0 * (self.index + 1) if size == "large" else 0.0

    def inputs(self, size: str):
        if size not in self._inputs:
            self._inputs[size] = self.build(size)
        return self._inputs[size]

    def pooled(self, size: str):
        return None

    def build(self, size: str):
        raise NotImplementedError

    def run(self, ctx, inputs):
        raise NotImplementedError

    def check(self, inputs, got, ctx=None):
        raise NotImplementedError

    def __repr__(self):
        return self.name


def chains_draws(size: str, small_cn) -> tuple:
    """(C, N, P) of a family whose chains have equal lengths."""
    return (*small_cn, 3) if size == "small" else (4, 16385, 2)


class Summarize(Family):
    name, symbols, sorts = "summarize", ("mcr_summarize",), True
    SMALL = (5, 201)

    def pooled(self, size):
        C_, N, _ = chains_draws(size, self.SMALL)
        return C_ * N

    def build(self, size):
        from mcmc_ref_hip import synth
        C_, N, P = chains_draws(size, self.SMALL)
        return dict(x=synth.c1_model(C_, N, P, seed=self.seed(size)) + self.offset(size), layout="pcn")

    def run(self, ctx, inputs):
        return pack(ctx.summarize(inputs["x"], inputs["layout"]))

    def check(self, inputs, got, ctx=None):
        from test_hip_parity import check_summary
        check_summary(unpack(got), oracle().summarize(inputs["x"], inputs["layout"]), what=self.name)


class Enqueue(Summarize):
    """A device tensor, f32 in the Arrow layout: the ingest pass and the 32-bit record sort."""
    name, symbols = "enqueue", ("mcr_summarize_enqueue", "mcr_summarize_wait_one")
    SMALL = (5, 203)

    def build(self, size):
        x = Summarize.build(self, size)["x"]
        return dict(x=np.ascontiguousarray(np.transpose(x, (1, 2, 0))).astype(np.float32), layout="cnp")

    def run(self, ctx, inputs):
        t = ctx.upload(inputs["x"], inputs["layout"])
        try:
            ctx.enqueue(t)
            return pack(ctx.wait_one().result())
        finally:
            t.free()


class DiagnoseChains(Family):
    name, symbols, sorts = "diagnose_chains", ("mcr_diagnose_chains",), True

    def pooled(self, size):
        return 1021 if size == "small" else 65541

    def build(self, size):
        from test_rank_refs_cpu import chains_of
        x = np.random.default_rng(self.seed(size)).normal(size=self.pooled(size)) + self.offset(size)
        return dict(x=x, chains=chains_of(x))

    def run(self, ctx, inputs):
        r = ctx.diagnose_chains(inputs["chains"], min_chains=2, debug=True)
        return pack({k: (np.concatenate(v) if isinstance(v, list) else v) for k, v in r.items()})

    def check(self, inputs, got, ctx=None):
        from test_rank_codes_gpu import check_diagnosis
        r = unpack(got)
        r = {k: ([v] if k.startswith(("z_", "rank_")) else v.item()) for k, v in r.items()}
        check_diagnosis(r, inputs["x"], inputs["chains"], oracle(), self.name)


class Moments(Family):
    """mcr_moments_dev on a device tensor and mcr_basic_stats on its first parameter."""
    name, symbols = "moments", ("mcr_moments_dev", "mcr_basic_stats")

    def pooled(self, size):
        return 5 * 207 if size == "small" else None

    def build(self, size):
        C_, N, P = (5, 207, 3) if size == "small" else (4, 1000, 65)          # test_strides_gpu's moments shape
        rng = np.random.default_rng(self.seed(size))
        return dict(x=rng.normal(size=(P, C_, N)) * 10.0 ** rng.integers(-2, 3, size=(P, 1, 1)) + self.offset(size))

    def run(self, ctx, inputs):
        t = ctx.upload(inputs["x"], "pcn")
        try:
            mean, std = ctx.moments(t)
        finally:
            t.free()
        b = ctx.basic_stats(inputs["x"][0].reshape(-1))
        return pack(dict(mean=mean, std=std, basic_mean=b["mean"], basic_std=b["std"]))

    def check(self, inputs, got, ctx=None):
        from test_hip_parity import check_basic_stats
        from test_strides_gpu import assert_moments, exact_moments
        r, x = unpack(got), inputs["x"]
        assert_moments(r["mean"], r["std"], *exact_moments(x), self.name)       # the streaming kernels' bound, against fsum
        for p, row in enumerate(x):                                             # and the oracle, at the gate of its sum
            check_basic_stats({"mean": float(r["mean"][p]), "std": float(r["std"][p])}, oracle().basic_stats(row.reshape(-1)))
        check_basic_stats({"mean": r["basic_mean"].item(), "std": r["basic_std"].item()}, oracle().basic_stats(x[0].reshape(-1)))


class Compare(Family):
    name, symbols = "compare", ("mcr_compare",)
    TOL = 1e-3

    def build(self, size):
        n = 1041 if size == "small" else 70001
        rng = np.random.default_rng(self.seed(size))
        ref = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n) + self.offset(size)
        act = ref * (1.0 + self.TOL * rng.normal(size=n))                      # about a third of them fail
        ref[::97], act[::97] = 0.0, 0.0                                        # both zero
        ref[1::97] = 0.0                                                       # a zero reference alone
        act[2::97] = ref[2::97]                                                # equal
        return dict(ref=ref, act=act)

    def run(self, ctx, inputs):
        rel, ok = ctx.compare(inputs["ref"], inputs["act"], self.TOL)
        return pack(dict(rel=rel, ok=ok))

    def check(self, inputs, got, ctx=None):
        from test_hip_parity import check_compare
        r = unpack(got)
        check_compare(r["rel"], r["ok"], *oracle().compare(inputs["ref"], inputs["act"], self.TOL))


class TwoSample(Family):
    name, symbols, sorts = "two_sample", ("mcr_two_sample",), True
    SHAPES = {"small": (523, 524, 3), "large": (WIDE + 1, 9001, 2)}        # (Mr, Ma, P)

    def pooled(self, size):
        Mr, Ma, _ = self.SHAPES[size]
        return Mr + Ma if size == "small" else Mr

    def build(self, size):
        Mr, Ma, P = self.SHAPES[size]
        rng = np.random.default_rng(self.seed(size))
        ref = rng.normal(size=(P, Mr)) + self.offset(size)
        act = rng.normal(loc=0.1, scale=1.2, size=(P, Ma)) + self.offset(size)
        ref[1], act[1] = np.round(ref[1], 1), np.round(act[1], 1)              # ties within and across the samples
        return dict(ref=ref, act=act)

    def run(self, ctx, inputs):
        ks, w1 = ctx.two_sample(inputs["ref"], inputs["act"])
        return pack(dict(ks=ks, w1=w1))

    def check(self, inputs, got, ctx=None):
        from test_ext_gpu import assert_two_sample_matches_scipy
        r = unpack(got)
        assert_two_sample_matches_scipy(r["ks"], r["w1"], inputs["ref"], inputs["act"], (self.name,))


class SlicedTwoSample(Family):
    name, symbols, sorts = "sliced_two_sample", ("mcr_sliced_two_sample",), True
    SHAPES = {"small": (500, 551, 3, 3), "large": (WIDE + 1, 4099, 2, 3)}    # (Mr, Ma, P, K)

    def pooled(self, size):
        Mr, Ma, _, _ = self.SHAPES[size]
        return Mr + Ma if size == "small" else Mr

    def build(self, size):
        Mr, Ma, P, K = self.SHAPES[size]
        rng = np.random.default_rng(self.seed(size))
        off = self.offset(size)
        return dict(ref=off + rng.normal(size=(P, Mr)), act=off + 0.5 + 1.5 * rng.normal(size=(P, Ma)),
                    W=rng.normal(size=(K, P)) * 10.0 ** rng.integers(-2, 3, size=(K, 1)), center=off + rng.normal(size=P) * 0.25)

    def run(self, ctx, inputs):
        ks, w1, zr, za = ctx.sliced_two_sample(inputs["ref"], inputs["act"], inputs["W"], inputs["center"], projections=True)
        return pack(dict(ks=ks, w1=w1, zr=zr, za=za))

    def check(self, inputs, got, ctx=None):
        from test_ext_gpu import assert_two_sample_matches_scipy
        from test_sliced_gpu import projection_error
        r = unpack(got)
        for X, z in ((inputs["ref"], r["zr"]), (inputs["act"], r["za"])):
            projection_error(X, inputs["W"], inputs["center"], z, (self.name,))
        assert_two_sample_matches_scipy(r["ks"], r["w1"], r["zr"], r["za"], (self.name,))


class EnergyDistance(Family):
    name, symbols = "energy_distance", ("mcr_energy_distance",)
    SHAPES = {"small": (130, 70, 3), "large": (300, 260, 9)}                 # (Mr, Ma, P)

    def build(self, size):
        Mr, Ma, P = self.SHAPES[size]
        rng = np.random.default_rng(self.seed(size))
        off = self.offset(size)
        return dict(ref=off + rng.normal(size=(P, Mr)), act=off + 0.2 + 1.3 * rng.normal(size=(P, Ma)),
                    scale=rng.uniform(0.2, 3.0, size=P))

    def run(self, ctx, inputs):
        return pack(ctx.energy_distance(inputs["ref"], inputs["act"], inputs["scale"]))

    def check(self, inputs, got, ctx=None):
        from mcmc_ref_hip import _ffi
        from test_energy_refs_cpu import assert_close
        r = {k: float(v) for k, v in unpack(got).items()}
        assert_close(r, _ffi.energy_distance_host(inputs["ref"], inputs["act"], inputs["scale"]), self.name)


class Covariance(Family):
    name, symbols = "covariance", ("mcr_covariance",)
    SHAPES = {"small": (1061, 3), "large": (16385, 40)}                      # (M, P)

    def pooled(self, size):
        return self.SHAPES[size][0] if size == "small" else None

    def build(self, size):
        M, P = self.SHAPES[size]
        rng = np.random.default_rng(self.seed(size))
        L = rng.normal(size=(P, P))
        return dict(x=(L @ rng.normal(size=(P, M))) * 1e-2 + rng.normal(size=(P, 1)) * 50.0 + self.offset(size))

    def run(self, ctx, inputs):
        return pack(dict(cov=ctx.covariance(inputs["x"])))

    def check(self, inputs, got, ctx=None):
        from test_ext_gpu import assert_covariance_matches_numpy
        assert_covariance_matches_numpy(unpack(got)["cov"], inputs["x"], (self.name,))


class NestedRhat(Family):
    name, symbols, sorts = "nested_rhat", ("mcr_nested_rhat",), True

    def shape(self, size):
        return (9, 119, 3, 3) if size == "small" else (4, 16385, 2, 2)       # (C, N, P, K)

    def pooled(self, size):
        C_, N, _, _ = self.shape(size)
        return C_ * N

    def build(self, size):
        from test_nested_refs_cpu import block_ids
        C_, N, P, K = self.shape(size)
        rng = np.random.default_rng(self.seed(size))
        x = rng.normal(size=(P, C_, N)) * (10.0 ** rng.integers(-1, 2, size=(P, 1, 1))) + 0.2 * rng.normal(size=(P, C_, 1))
        return dict(x=x + self.offset(size), ids=block_ids(C_, K))

    def run(self, ctx, inputs):
        return pack(ctx.nested_rhat(inputs["x"], inputs["ids"]))

    def check(self, inputs, got, ctx=None):
        from test_nested_gpu import gate
        gate(unpack(got), inputs["x"], inputs["ids"], self.name)


class Pooled(Family):
    """A family on the pooled draws of a tensor [P][C][N]: x [P][M], handed over as chains_of the sibling tests do."""
    sorts = True
    SMALL_M = 0

    def pooled(self, size):
        return self.SMALL_M if size == "small" else 4 * 16385

    def shape(self, size):
        return (self.pooled(size), 3 if size == "small" else 2)

    @staticmethod
    def chains_of(x):
        P, M = x.shape
        return x.reshape(P, 4, M // 4) if M % 4 == 0 else x.reshape(P, 1, M)


class ParetoKhat(Pooled):
    name, symbols, SMALL_M = "pareto_khat", ("mcr_pareto_khat",), 1077

    def build(self, size):
        from test_pareto_refs_cpu import DISTS, draws
        M, P = self.shape(size)
        return dict(x=np.stack([draws(DISTS[p % len(DISTS)], M, seed=self.seed(size) + p) for p in range(P)]))

    def run(self, ctx, inputs):
        r = ctx.pareto_khat(self.chains_of(inputs["x"]))
        return pack({k: r[k] for k in ("khat", "khat_left", "khat_right", "ndraws_tail")})

    def check(self, inputs, got, ctx=None):
        from mcmc_ref_hip import _ffi
        from test_pareto_gpu import gate
        from test_pareto_refs_cpu import same
        r = unpack(got)
        gate(r, inputs["x"], self.name)
        for p, row in enumerate(inputs["x"]):
            kl, kr, t = _ffi.pareto_fit_host(np.sort(row))
            assert int(r["ndraws_tail"][p]) == t and same(float(r["khat_left"][p]), kl) and same(float(r["khat_right"][p]), kr), (self.name, p)


class Psis(Pooled):
    name, symbols, SMALL_M = "psis", ("mcr_psis",), 1083

    def build(self, size):
        from test_psis_refs_cpu import values
        M, P = self.shape(size)
        return dict(x=np.stack([values(d, M, seed=self.seed(size) + p) for p, d in enumerate(("normal3", "t3", "rounded")[:P])]))

    def run(self, ctx, inputs):
        r = ctx.psis(self.chains_of(inputs["x"]), weights=True)
        return pack({k: r[k] for k in ("khat", "ndraws_tail", "log_weights")})

    def check(self, inputs, got, ctx=None):
        from mcmc_ref_hip import _ffi
        from test_psis_refs_cpu import check
        r = unpack(got)
        for p, row in enumerate(inputs["x"]):
            check({k: r[k][p] for k in ("khat", "ndraws_tail", "log_weights")}, _ffi.psis_host(row), (self.name, p))


class Hdi(Pooled):
    name, symbols, SMALL_M = "hdi", ("mcr_hdi",), 1089
    PROBS = [0.94, 0.5, 0.1]

    def build(self, size):
        from test_hdi_refs_cpu import draws
        M, P = self.shape(size)
        kinds = ("tied", "normal", "bimodal")[:P]
        return dict(x=np.stack([draws(k, M, seed=self.seed(size) + p) for p, k in enumerate(kinds)]) + self.offset(size))

    def run(self, ctx, inputs):
        r = ctx.hdi(self.chains_of(inputs["x"]), prob=self.PROBS)
        return pack({k: r[k] for k in ("lo", "hi", "index")})

    def check(self, inputs, got, ctx=None):
        from mcmc_ref_hip import _ffi
        from test_hdi_gpu import gate
        r = unpack(got)
        gate(r, inputs["x"], self.PROBS, self.name)
        for p, row in enumerate(inputs["x"]):
            lo, hi, idx = _ffi.hdi_sorted_host(np.sort(row), self.PROBS)
            assert r["index"][p].tolist() == idx.tolist() and r["lo"][p].tolist() == lo.tolist() and r["hi"][p].tolist() == hi.tolist(), (self.name, p)


class Autocorr(Family):
    name, symbols = "autocorr", ("mcr_autocorr",)
    PHI = (0.6, 0.2, 0.4)

    def shape(self, size):
        return (5, 219, 3, 37) if size == "small" else (3, 2 * 512 + 1, 2, 255)       # (C, N, P, max_lag): test_acf_gpu's edges

    def pooled(self, size):
        C_, N, _, _ = self.shape(size)
        return C_ * N if size == "small" else None

    def build(self, size):
        from test_acf_refs_cpu import ar1
        C_, N, P, L = self.shape(size)
        x = np.stack([ar1(self.PHI[p], C_, N, seed=self.seed(size) + 10 * p, offset=self.offset(size)) for p in range(P)])
        return dict(x=x, L=L)

    def run(self, ctx, inputs):
        r = ctx.autocorr(inputs["x"], "pcn", max_lag=inputs["L"])
        return pack({k: r[k] for k in ("acf", "var", "tau", "window", "acf_pooled", "tau_pooled", "window_pooled")})

    def host(self, inputs, p: int) -> dict:
        from mcmc_ref_hip import _ffi
        return _ffi.autocorr_host(inputs["x"][p], max_lag=inputs["L"])

    def check(self, inputs, got, ctx=None):
        from test_acf_refs_cpu import gate, one
        r = unpack(got)
        for p in range(inputs["x"].shape[0]):
            gate(one(r, p), inputs["x"][p], inputs["L"], False, 5.0, (self.name, p))
            host = self.host(inputs, p)
            for k in r:
                assert r[k][p].tobytes() == np.ascontiguousarray(host[k][0]).tobytes(), (self.name, p, k)


class WeightedSummary(Pooled):
    """Log weights and quantiles; the linear weights the call formed come back too."""
    name, symbols, SMALL_M = "weighted_summary", ("mcr_weighted_summary",), 1093

    def shape(self, size):
        return (self.pooled(size), 2)                         # (x0, -x0), as test_weighted_gpu.test_log_weights

    def build(self, size):
        from test_weighted_refs_cpu import QS, real_sample
        M, _ = self.shape(size)
        x0, w = real_sample(M, self.seed(size), offset=0.0)
        return dict(x=np.stack([x0, -x0]) + self.offset(size), w=w, lw=np.log(w) + 700.0, qs=QS)

    def run(self, ctx, inputs):
        r = ctx.weighted_summary(self.chains_of(inputs["x"]), log_weights=inputs["lw"], quantiles=inputs["qs"], return_weights=True)
        return pack({k: r[k] for k in ("mean", "sd", "mean_se", "quantiles", "ess", "weight_sum", "weights")})

    @staticmethod
    def host_weights(inputs):
        return np.exp(inputs["lw"] - inputs["lw"].max())      # the host's exp

    def check(self, inputs, got, ctx=None):
        from mcmc_ref_hip import _ffi
        from test_weighted_refs_cpu import check_floats, numpy_quantiles
        r, x, wh = unpack(got), inputs["x"], self.host_weights(inputs)
        assert r["weights"].shape == wh.shape and r["weights"].max() == 1.0 and np.allclose(r["weights"], wh, rtol=1e-12, atol=0)
        for p in range(2):
            assert np.array_equal(r["quantiles"][p], numpy_quantiles(x[p], wh, inputs["qs"])), (self.name, p)
            if p == 0:                                        # (exact rational arithmetic: once, as test_log_weights does)
                check_floats({**{k: float(r[k][p]) for k in ("mean", "sd", "mean_se")}, "ess": float(r["ess"]),
                              "weight_sum": float(r["weight_sum"])}, x[p], wh)
            host = _ffi.weighted_host(x[p], weights=r["weights"], quantiles=inputs["qs"])      # linear weights: the device's bits
            for k in ("mean", "sd", "mean_se"):
                assert np.float64(host[k]).tobytes() == r[k][p].tobytes(), (self.name, p, k)
            assert host["quantiles"].tobytes() == r["quantiles"][p].tobytes(), (self.name, p)


class SbcRanks(Family):
    """Layout "scnp": the simulations' ingest copy lives in the lane workspace."""
    name, symbols = "sbc_ranks", ("mcr_sbc_ranks",)
    SHAPES = {"small": (3, 2, 129), "large": (9, 7, 2049)}                   # (S, P, L)

    def build(self, size):
        from test_sbc_gpu import as_layout, chains
        from test_sbc_refs_cpu import edge_sample
        S, P, L = self.SHAPES[size]
        x, t = edge_sample(S, P, L, seed=self.seed(size))
        x, t = x + self.offset(size), t + self.offset(size)
        return dict(x=x, t=t, x4=as_layout(x.reshape(S, P, chains(L), -1), "scnp"))

    def run(self, ctx, inputs):
        return pack(ctx.sbc_ranks(inputs["x4"], inputs["t"], "scnp"))

    def check(self, inputs, got, ctx=None):
        from mcmc_ref_hip import _ffi
        from test_sbc_refs_cpu import check_against_references
        r = unpack(got)
        r["n_draws"] = int(r["n_draws"])
        check_against_references(r, inputs["x"], inputs["t"])
        host = _ffi.sbc_ranks_host(inputs["x"], inputs["t"])
        for k in ("n_less", "n_equal", "mean", "sd"):
            assert r[k].tobytes() == np.ascontiguousarray(host[k]).tobytes(), (self.name, k)


class ReadColumns(Family):
    """A Parquet image with Snappy pages and dictionary columns, read back by mcr_parquet_decode."""
    name, symbols = "read_columns", ("mcr_parquet_open", "mcr_parquet_decode", "mcr_parquet_close")

    def build(self, size):
        import pyarrow as pa
        from test_parquet_gpu import image, mixed_table
        if size == "large":
            return dict(img=image(mixed_table(6000, seed=self.seed(size)), compression="snappy", use_dictionary=True))
        rng = np.random.default_rng(self.seed(size))
        n = 8                                                 # (834 bytes: most of them the footer)
        t = pa.table({"x": rng.normal(size=n), "ties": np.round(rng.normal(size=n), 0)})
        return dict(img=image(t, compression="snappy", use_dictionary=True))

    def run(self, ctx, inputs):
        from mcmc_ref_hip.parquet import read_columns
        return pack(read_columns(ctx, inputs["img"]))

    def check(self, inputs, got, ctx=None):
        from test_parquet_gpu import assert_equals_pyarrow
        assert_equals_pyarrow(unpack(got), inputs["img"])


class IngestFamily(Family):
    """One of the paths of test_context_buffers_gpu.Ingest: its files, its call, its host check."""
    kind = ""

    def build(self, size):
        return dict(size=size, **ingest().f[self.kind, size])

    def run(self, ctx, inputs):
        return ingest().run(ctx, self.kind, inputs["size"])

    def check(self, inputs, got, ctx=None):
        if self.kind == "files":                              # the host check reads the files again: the same answer, then held
            assert ingest().run(ctx, self.kind, inputs["size"]) == got
        ingest().check_host(ctx, self.kind, inputs["size"], got)


class SummarizeFiles(IngestFamily):
    name, kind = "summarize_files", "files"
    symbols = ("mcr_summarize_files", "mcr_fileset_size", "mcr_fileset_params", "mcr_fileset_chains", "mcr_fileset_draws",
               "mcr_fileset_export", "mcr_fileset_names", "mcr_fileset_free")


class CsvDecode(IngestFamily):
    name, kind = "csv_decode", "chain_csv"
    symbols = ("mcr_csv_open_paths", "mcr_csv_num_columns", "mcr_csv_column_name", "mcr_csv_stage", "mcr_csv_decode", "mcr_csv_close")


class JsonDecode(IngestFamily):
    name, kind = "json_decode", "json"
    symbols = ("mcr_json_open", "mcr_json_num_chains", "mcr_json_num_keys", "mcr_json_key", "mcr_json_length", "mcr_json_decode",
               "mcr_json_close")


class CsvTableDecode(IngestFamily):
    name, kind = "csv_table_decode", "table_csv"
    symbols = ("mcr_csv_open_table_paths", "mcr_csv_num_columns", "mcr_csv_column_name", "mcr_csv_stage", "mcr_csv_decode_table",
               "mcr_csv_close", "mcr_chain_layout_dev")        # (convert.read_csv_dev asks for the row order of the id columns too)


class WriteParquet(IngestFamily):
    name, kind = "write_parquet", "write"
    symbols = ("mcr_parquet_write_dev", "mcr_pq_image_data", "mcr_pq_image_size", "mcr_pq_image_pages", "mcr_pq_image_free")


class WriteCsv(Family):
    name = "write_csv"
    symbols = ("mcr_csv_write_dev", "mcr_text_image_data", "mcr_text_image_size", "mcr_text_image_free")
    SHAPES = {"small": (3, 7), "large": (40, 3000)}                          # (columns, rows): test_csv_write_gpu's

    def build(self, size):
        import csvwrite_cases as W
        cols, rows = W.table_case(*self.SHAPES[size], seed=self.seed(size))
        return dict(cols=cols, rows=rows)

    def run(self, ctx, inputs):
        from test_csv_write_gpu import write_dev
        return dict(text=write_dev(ctx, inputs["cols"], inputs["rows"]))

    def check(self, inputs, got, ctx=None):
        import csvwrite_cases as W
        assert got["text"] == W.expected(inputs["cols"], inputs["rows"])       # pyarrow.csv.write_csv of the same table
        assert got["text"] == W.write_host(inputs["cols"], inputs["rows"])


class ChainLayout(Family):
    """An unordered ragged table's id columns: the radix passes over the row keys."""
    name, symbols = "chain_layout", ("mcr_chain_layout_dev",)

    def build(self, size):
        import ragged_cases
        chain, draw = ragged_cases.id_columns(1099 if size == "small" else 70001, "shuffled", seed=self.seed(size))
        return dict(chain=chain, draw=draw)

    def run(self, ctx, inputs):
        from test_chain_layout_gpu import layout
        rc, order, ids, counts, in_order = layout(ctx, inputs["chain"], inputs["draw"])
        return pack(dict(rc=rc, order=order, ids=ids, counts=counts, in_order=in_order))

    def check(self, inputs, got, ctx=None):
        from test_chain_layout_gpu import expect
        r = unpack(got)
        order, ids, counts, in_order = expect(inputs["chain"], inputs["draw"])
        assert int(r["rc"]) == 0 and not in_order and int(r["in_order"]) == 0
        assert np.array_equal(r["order"], order) and np.array_equal(r["ids"], ids) and np.array_equal(r["counts"], counts)


# ---- the extension entries and the two companion libraries ---------------------------------------------------------------
# mcrx_* carve the main context's lane workspace; mci_* and mcb_* each have a handle of their own per Context (a stream, a
# workspace and an upload buffer that only grow), and mean_shift_test crosses all three in one call.  Each of these
# families also has `host(inputs)`: the same fields from the definitions on the host, which the CPU test feeds to `check`.

def _scalars(r: dict) -> dict:
    """unpack()'s 0-d arrays as Python numbers, as the public calls return them."""
    return {k: (v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v) for k, v in r.items()}


class Linalg(Family):
    """mcrx_cholesky of an SPD matrix, then mcrx_solve_lower of the factor it returned against K right-hand sides."""
    name, symbols = "linalg", ("mcrx_cholesky", "mcrx_solve_lower")
    SHAPES = {"small": (17, 1), "large": (3 * 64 + 1, 65)}                  # (P, K): 3 NB + 1, test_gaussian_gpu's largest

    def build(self, size):
        from test_gaussian_refs_cpu import spd
        P, K = self.SHAPES[size]
        return dict(A=spd(P, 1e3, self.seed(size)), B=np.random.default_rng(self.seed(size)).standard_normal((P, K)))

    @staticmethod
    def _both(inputs, cholesky, solve_lower):
        L, info, logdet = cholesky(inputs["A"])
        return pack(dict(L=L, info=info, logdet=logdet, X=solve_lower(L, inputs["B"])))

    def run(self, ctx, inputs):
        from mcmc_ref_hip import gaussian
        return self._both(inputs, lambda a: gaussian.cholesky(a, context=ctx), lambda l, b: gaussian.solve_lower(l, b, context=ctx))

    def host(self, inputs):
        from mcmc_ref_hip import gaussian
        return self._both(inputs, gaussian.cholesky_host, gaussian.solve_lower_host)

    def check(self, inputs, got, ctx=None):
        from test_gaussian_refs_cpu import check_factor, solve_residual_ratio
        r = _scalars(unpack(got))
        check_factor(inputs["A"], r["L"], r["info"], r["logdet"], self.name)
        ratio = solve_residual_ratio(r["L"], r["X"], inputs["B"])
        assert r["X"].shape == inputs["B"].shape and ratio <= 1.0, (self.name, ratio)


class GaussianCheck(Family):
    """scale = 1 / the reference's std with the middle parameter dropped by a zero: P_live < P, so Cr, Ca and W are
    written PL x PL inside their P x P carve."""
    name, symbols = "gaussian_check", ("mcrx_gaussian_check",)
    SHAPES = {"small": (3, 131, 77), "large": (2 * 64 + 1, 2049, 1025)}      # (P, Mr, Ma): 2 NB + 1

    def __init__(self, index):
        super().__init__(index)
        self._want: dict = {}

    def build(self, size):
        from test_gaussian_refs_cpu import pair
        P, Mr, Ma = self.SHAPES[size]
        ref, act = pair(P, Mr, Ma, seed=self.seed(size))
        scale = 1.0 / ref.std(axis=1)
        scale[P // 2] = 0.0
        return dict(ref=ref, act=act, scale=scale)

    def reference(self, inputs) -> dict:
        """gaussian_reference of the inputs (long double), once per size."""
        from test_gaussian_refs_cpu import gaussian_reference
        key = id(inputs)
        if key not in self._want:
            self._want[key] = gaussian_reference(inputs["ref"], inputs["act"], inputs["scale"])
        return self._want[key]

    def run(self, ctx, inputs):
        from mcmc_ref_hip import gaussian
        return pack(gaussian.gaussian_check(inputs["ref"], inputs["act"], inputs["scale"], shift=True, context=ctx))

    def host(self, inputs):
        from mcmc_ref_hip import gaussian
        return pack(gaussian.gaussian_check_host(inputs["ref"], inputs["act"], inputs["scale"], shift=True))

    def check(self, inputs, got, ctx=None):
        from test_gaussian_refs_cpu import check_statistics
        r, want = _scalars(unpack(got)), self.reference(inputs)
        assert want["p_live"] == inputs["ref"].shape[0] - 1
        check_statistics(r, want, self.name)
        assert np.abs(r["shift"] - want["shift"]).max() <= 1e-9 * max(1.0, np.abs(want["shift"]).max()), self.name


class IndicatorEss(Family):
    """x <= the pooled quantiles at PROBS; parameter 0 is rounded to halves (ties, and draws equal to a threshold).  small:
    the ballot pack and the lag kernel on LDS; large: the smallest N whose C (ceil(N / 64) + 1) words exceed MCI_LDS_WORDS,
    parameters innermost: the tile pack and the lag kernel on global words with its prefix counts."""
    name, symbols = "indicator_ess", ("mci_indicator_ess",)
    PROBS = (0.05, 0.5, 0.95)
    LDS_WORDS = 8192                                          # MCI_LDS_WORDS (the CPU test holds it to the mirror)

    def shape(self, size):
        """(C, N, P, layout)"""
        if size == "small":
            return 2, 129, 3, "pcn"
        C_ = 3
        return C_, 64 * (self.LDS_WORDS // C_ - 1) + 1, 2, "cnp"

    def build(self, size):
        from test_indicator_gpu import draws, quantile_requests
        C_, N, P, layout = self.shape(size)
        if size == "small":
            x = draws(self.seed(size), P, C_, N)
        else:                                                 # iid: the walk ends in the first lag block
            x = np.random.default_rng(self.seed(size)).normal(size=(P, C_, N))
            x[0] = np.round(x[0] * 2) / 2
        upper = quantile_requests(x, self.PROBS)[1]
        return dict(x=np.ascontiguousarray(np.transpose(x, ["pcn".index(a) for a in layout])), layout=layout, upper=upper)

    def run(self, ctx, inputs):
        from mcmc_ref_hip import indicator
        return pack(indicator.indicator_ess(inputs["x"], -np.inf, inputs["upper"], inputs["layout"], ctx))

    def host(self, inputs):
        from mcmc_ref_hip import indicator
        return pack(indicator.indicator_ess_host(inputs["x"], -np.inf, inputs["upper"], inputs["layout"]))

    def check(self, inputs, got, ctx=None):
        from test_indicator_gpu import same
        from test_indicator_refs_cpu import close, restate
        r = unpack(got)
        assert same(r, unpack(self.host(inputs))), self.name
        x = np.transpose(inputs["x"], [inputs["layout"].index(a) for a in "pcn"])
        p, k = x.shape[0] - 1, 1                              # the last parameter's median, by the definition in integers
        exp = restate((x[p] <= inputs["upper"][p, k]).astype(np.int64))
        assert (int(r["trunc"][p, k]), int(r["ones"][p, k])) == exp[1:] and close(float(r["ess"][p, k]), exp[0]), (self.name, exp)


class BatchMeans(Family):
    """small: stride_n == 1, the time route with one register row of batches; large: parameters innermost, the tile
    route, a batch of more than one block of 1024 leaves, P off the 64-parameter tile.  (b is a multiple of 3: r = 3.)"""
    name, symbols = "batch_means", ("mcb_batch_means",)
    SHAPES = {"small": (2, 131, 3, 9, "pcn"), "large": (3, 3 * 1101 + 7, 130, 1101, "cnp")}      # (C, N, P, b, layout)

    def build(self, size):
        from test_batchmeans_gpu import draws
        C_, N, P, b, layout = self.SHAPES[size]
        x = draws(self.seed(size), P, C_, N) + self.offset(size)
        return dict(x=np.ascontiguousarray(np.transpose(x, ["pcn".index(a) for a in layout])), layout=layout, b=b)

    def run(self, ctx, inputs):
        from mcmc_ref_hip import batchmeans
        return pack(batchmeans.batch_means(inputs["x"], inputs["layout"], batch=inputs["b"], r=3, context=ctx))

    def host(self, inputs):
        from mcmc_ref_hip import batchmeans
        return pack(batchmeans.batch_means_host(inputs["x"], inputs["layout"], batch=inputs["b"], r=3))

    def check(self, inputs, got, ctx=None):
        from test_batchmeans_gpu import same
        from test_batchmeans_refs_cpu import bits, restate_batch_means
        r = _scalars(unpack(got))
        assert same(r, _scalars(unpack(self.host(inputs)))), self.name
        bm, mu = restate_batch_means(inputs["x"], inputs["layout"], inputs["b"])
        assert bits(r["bm"]) == bits(bm) and bits(r["mu"]) == bits(mu), self.name


class MeanShiftTest(Family):
    """One call, three handles: mcb_batch_means_dev -> mcb_pooled_dev -> mcr_covariance_dev -> mcb_lrv_finish_dev /
    mcb_pool_dev -> mcrx_cholesky_dev -> mcrx_solve_lower_dev.  The cases are test_batchmeans_refs_cpu.e2e_case's at the
    smallest and the largest P_live (cached there per P, with the long double answer)."""
    name = "mean_shift_test"
    symbols = ("mcb_batch_means_dev", "mcb_pooled_dev", "mcr_covariance_dev", "mcb_lrv_finish_dev", "mcb_pool_dev", "mcrx_cholesky_dev",
               "mcrx_solve_lower_dev")

    @staticmethod
    def p_live(size) -> int:
        from test_batchmeans_refs_cpu import E2E_P
        return min(E2E_P) if size == "small" else max(E2E_P)

    def build(self, size):
        from test_batchmeans_refs_cpu import e2e_case
        ref, act, scale, b_ref, b_act, _ = e2e_case(self.p_live(size))
        return dict(ref=ref, act=act, scale=scale, b_ref=b_ref, b_act=b_act, size=size)

    def run(self, ctx, inputs):
        from mcmc_ref_hip import batchmeans
        return pack(batchmeans.mean_shift_test(inputs["ref"], inputs["act"], scale=inputs["scale"], r=3, context=ctx,
                                               batch_ref=inputs["b_ref"], batch_act=inputs["b_act"]))

    def host(self, inputs):
        from mcmc_ref_hip import batchmeans
        return pack(batchmeans.mean_shift_test_host(inputs["ref"], inputs["act"], scale=inputs["scale"], r=3,
                                                    batch_ref=inputs["b_ref"], batch_act=inputs["b_act"]))

    def check(self, inputs, got, ctx=None):
        from test_batchmeans_refs_cpu import check_mean_test, e2e_case
        check_mean_test(_scalars(unpack(got)), e2e_case(self.p_live(inputs["size"]))[5], self.name)


FAMILIES = [cls(i) for i, cls in enumerate((
    Summarize, Enqueue, DiagnoseChains, Moments, Compare, TwoSample, SlicedTwoSample, EnergyDistance, Covariance, NestedRhat,
    ParetoKhat, Psis, Hdi, Autocorr, WeightedSummary, SbcRanks, ReadColumns, SummarizeFiles, CsvDecode, JsonDecode,
    CsvTableDecode, WriteParquet, WriteCsv, ChainLayout, Linalg, GaussianCheck, IndicatorEss, BatchMeans, MeanShiftTest))]
NEW_FAMILIES = FAMILIES[24:]                                  # the ones with `host`
BY_NAME = {f.name: f for f in FAMILIES}
NAMES = [f.name for f in FAMILIES]


# ---- refused calls ---------------------------------------------------------------------------------------------------

class Refusal:
    """A call that returns a documented error: call(ctx) makes it and asserts the code and the message.  With `outcome`
    (a predicate on what the call returned) the call is one that stops part-way and says so in its result, not in a code:
    then the code is MCR_OK, no message is asked for, and call(ctx) asserts the predicate."""

    def __init__(self, name: str, family: str, defect: str, code_name: str, fragment: str, build, call, outcome=None):
        self.name, self.family, self.defect, self.code_name, self.fragment = name, family, defect, code_name, fragment
        self._build, self._call, self._inputs, self.outcome = build, call, None, outcome

    def inputs(self):
        if self._inputs is None:
            self._inputs = self._build()
        return self._inputs

    def code(self) -> int:
        from mcmc_ref_hip import _ffi
        return getattr(_ffi, self.code_name)

    def call(self, ctx):
        from mcmc_ref_hip import _ffi
        if self.outcome is not None:
            result = self._call(ctx, self.inputs())
            assert self.code() == _ffi.MCR_OK and self.outcome(result), (self.name, result)
            return
        try:
            rc = self._call(ctx, self.inputs())
            message = (ctx.lib.mcr_last_error(ctx.handle) or b"").decode()
        except _ffi.McrError as e:
            rc, message = e.code, e.message
        assert rc == self.code(), (self.name, rc, message)
        assert self.fragment in message, (self.name, message)

    def __repr__(self):
        return self.name


def _poisoned(x: np.ndarray, where, value) -> np.ndarray:
    bad = x.copy()
    bad[where] = value
    return bad


def _tensor(seed: int, shape) -> np.ndarray:
    return np.random.default_rng(seed).normal(size=shape)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _two_sample_raw(ctx, i):
    P = i["ref"].shape[0]
    ks, w1 = np.full(P, np.nan), np.full(P, np.nan)
    return ctx.lib.mcr_two_sample(ctx.handle, _dp(i["ref"]), i["ref"].shape[1], _dp(i["act"]), i["act"].shape[1], P, _dp(ks), _dp(w1))


def _weighted_inputs():
    from test_weighted_gpu import chains_of, sample
    x, w = sample(4096, 2)
    return dict(x=chains_of(x), w=_poisoned(w, 77, -1.0))


def _sbc_inputs():
    from test_sbc_refs_cpu import edge_sample
    x, t = edge_sample(5, 7, 300, seed=4)
    bad = x.copy()
    bad[1, 0, 7], bad[1, 0, 8], bad[4, 6, 299] = np.nan, -np.inf, np.inf
    return dict(x=bad.reshape(5, 7, 3, -1), t=t)


def _energy_inputs():
    from test_energy_refs_cpu import general_case
    ref, act, _ = general_case(5, 4, 3, "scale")
    ref, act = ref.copy(), act.copy()
    ref.flat[1], act.flat[1] = 1e200, -1e200
    return dict(ref=ref, act=act)


def _snappy_inputs():
    import pyarrow as pa
    from mcmc_ref_hip.parquet import ParquetFile
    from test_parquet_gpu import image
    good = image(pa.table({"x": np.tile(np.arange(50.0), 200)}), use_dictionary=False)
    with ParquetFile(good) as f:
        at = f.pages()[0]["payload_offset"]
    bad = bytearray(good)
    bad[at] ^= 0x55                                           # breaks the length preamble
    return dict(good=good, img=bytes(bad), at=at)


def _read_columns(ctx, i):
    from mcmc_ref_hip.parquet import read_columns
    read_columns(ctx, i["img"])
    return 0


LOW_LIMIT = 1 << 20                                           # the smallest workspace limit the library takes


def _under_the_limit(ctx, i):
    ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, LOW_LIMIT))
    try:
        ctx.summarize(i["x"], "pcn")
    finally:
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, BIG_LIMIT))
    return 0


COMPANION_LIMIT = 1 << 30                                     # the default limit of an mci or mcb handle, which the tests restore
TINY_LIMIT = 64                                               # below the 256 bytes any one parameter's workspace is rounded up to


def _batchmeans():
    from mcmc_ref_hip import batchmeans
    return batchmeans


def _stopped_inputs():
    from test_gaussian_refs_cpu import NB, defect_matrix
    A, info = defect_matrix(2 * NB + 5, "neg", NB + 1)
    return dict(A=A, info=info)


def _cholesky_raw(ctx, i):
    """(info, logdet, the info the definition gives)"""
    from mcmc_ref_hip import gaussian
    _, info, logdet = gaussian.cholesky(i["A"], context=ctx)
    return info, logdet, i["info"]


def _gaussian_limit_inputs():
    from test_gaussian_refs_cpu import gauss_case
    ref, act, scale, _ = gauss_case(129, 2000, 1500)           # test_gaussian_gpu.test_workspace_limit's shape
    return dict(ref=ref, act=act, scale=scale)


def _gaussian_under_the_limit(ctx, i):
    from mcmc_ref_hip import gaussian
    P, Mr = i["ref"].shape
    assert gaussian.gaussian_workspace(Mr, i["act"].shape[1], P, context=ctx) > LOW_LIMIT
    ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, LOW_LIMIT))
    try:
        gaussian.gaussian_check(i["ref"], i["act"], i["scale"], context=ctx)
    finally:
        ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, BIG_LIMIT))
    return 0


def _indicator_under_the_limit(ctx, i):
    from mcmc_ref_hip import indicator
    indicator.set_workspace_limit(TINY_LIMIT, ctx)
    try:
        indicator.indicator_ess(i["x"], -np.inf, 0.0, "pcn", ctx)
    finally:
        indicator.set_workspace_limit(COMPANION_LIMIT, ctx)
    return 0


def _batch_means_under_the_limit(ctx, i):
    bm = _batchmeans()
    bm.set_workspace_limit(TINY_LIMIT, context=ctx)
    try:
        bm.batch_means(i["x"], batch=i["batch"], r=3, context=ctx)
    finally:
        bm.set_workspace_limit(COMPANION_LIMIT, context=ctx)
    return 0


REFUSED = [
    # one NaN in the last of the two sort tiles of a parameter (4 x 1100 pooled draws)
    Refusal("summarize_nan_in_last_tile", "summarize", "one_nan", "MCR_ENONFINITE", "non-finite",
            lambda: dict(x=_poisoned(_tensor(9001, (2, 4, 1100)), (1, 3, 1099), np.nan)),
            lambda ctx, i: ctx.summarize(i["x"], "pcn") and 0),
    Refusal("two_sample_infinity", "two_sample", "one_inf", "MCR_ENONFINITE", "non-finite",
            lambda: dict(ref=_tensor(9002, (3, 40000)), act=_poisoned(_tensor(9003, (3, 25000)), (1, 11), np.inf)),
            _two_sample_raw),
    Refusal("weighted_negative_weight", "weighted_summary", "one_negative_weight", "MCR_EINVAL", "weights",
            _weighted_inputs, lambda ctx, i: ctx.weighted_summary(i["x"], weights=i["w"]) and 0),
    Refusal("sbc_nonfinite_draws", "sbc_ranks", "three_nonfinite", "MCR_ENONFINITE", "3 non-finite",
            _sbc_inputs, lambda ctx, i: ctx.sbc_ranks_rc(np.ascontiguousarray(np.transpose(i["x"], (0, 2, 3, 1))), i["t"], "scnp")[0]),
    Refusal("energy_overflow", "energy_distance", "overflow", "MCR_ENONFINITE", "overflow",
            _energy_inputs, lambda ctx, i: ctx.energy_distance(i["ref"], i["act"]) and 0),
    Refusal("psis_nan", "psis", "one_nan", "MCR_ENONFINITE", "non-finite",
            lambda: dict(x=_poisoned(_tensor(9004, (2, 4, 1024)), (1, 2, 5), np.nan)), lambda ctx, i: ctx.psis(i["x"]) and 0),
    Refusal("hdi_nan", "hdi", "one_nan", "MCR_ENONFINITE", "non-finite",
            lambda: dict(x=_poisoned(_tensor(9005, (2, 4, 1024)), (1, 2, 5), np.nan)), lambda ctx, i: ctx.hdi(i["x"]) and 0),
    Refusal("nested_rhat_nan", "nested_rhat", "one_nan", "MCR_ENONFINITE", "non-finite",
            lambda: dict(x=_poisoned(_tensor(9006, (2, 4, 1024)), (1, 2, 5), np.nan)), lambda ctx, i: ctx.nested_rhat(i["x"], 2) and 0),
    Refusal("autocorr_nan", "autocorr", "one_nan", "MCR_ENONFINITE", "non-finite",
            lambda: dict(x=_poisoned(_tensor(9007, (2, 4, 300)), (1, 1, 7), np.nan)),
            lambda ctx, i: ctx.autocorr(i["x"], "pcn", max_lag=40) and 0),
    Refusal("read_columns_broken_snappy", "read_columns", "snappy_preamble", "MCR_EINVAL", "Snappy", _snappy_inputs, _read_columns),
    # a parameter's 160 000 keys alone are larger than the limit
    Refusal("summarize_under_the_limit", "summarize", "limit", "MCR_ENOMEM", "one parameter needs",
            lambda: dict(x=_tensor(9008, (2, 4, 40000))), _under_the_limit),
    # the pivot of column NB + 1 is -1: the second diagonal block stops at its second column, the panels after it skip on
    # the info word, and the factor area is left half-done.  MCR_OK: the finding is in (info, logdet).
    Refusal("cholesky_stopped_mid_block", "linalg", "negative_pivot", "MCR_OK", "", _stopped_inputs, _cholesky_raw,
            outcome=lambda r: r[0] == r[2] and r[1] != r[1]),
    # after both samples were staged
    Refusal("gaussian_check_under_the_limit", "gaussian_check", "gaussian_limit", "MCR_ENOMEM", "workspace limit too small",
            _gaussian_limit_inputs, _gaussian_under_the_limit),
    Refusal("indicator_under_the_limit", "indicator_ess", "companion_limit", "MCR_ENOMEM", "one parameter needs",
            lambda: dict(x=_tensor(9009, (2, 2, 100)), batch=None), _indicator_under_the_limit),
    Refusal("batch_means_under_the_limit", "batch_means", "companion_limit", "MCR_ENOMEM", "limit",
            lambda: dict(x=_tensor(9010, (2, 3, 3 * 99 + 5)), batch=99), _batch_means_under_the_limit),
    Refusal("batch_means_batch_over_n", "batch_means", "batch_over_n", "MCR_EINVAL", "outside [1, N",
            lambda: dict(x=_tensor(9011, (2, 3, 3 * 99 + 5)), batch=3 * 99 + 6),
            lambda ctx, i: _batchmeans().batch_means(i["x"], batch=i["batch"], r=1, context=ctx) and 0),
]


# ---- the ABI ---------------------------------------------------------------------------------------------------------

NOT_IN_THE_MATRIX = {
    "no context, or no device work": (
        "mcr_version", "mcr_device_count", "mcr_init", "mcr_free", "mcr_last_error", "mcr_pareto_tail_length", "mcr_psis_tail_length",
        "mcr_sbc_uniformity", "mcr_chi2_sf", "mcr_format_double", "mcr_parse_double", "mcr_parse_csv_number", "mcr_parse_json_number",
        "mci_version", "mci_init", "mci_free", "mci_last_error", "mcb_version", "mcb_init", "mcb_free", "mcb_last_error"),
    "a query of the planner: host arithmetic on the limit": (
        "mcr_plan_chunks", "mcr_plan_chunks_chains", "mcr_sliced_plan", "mcr_energy_workspace", "mcr_nested_plan", "mcr_pareto_plan",
        "mcr_psis_plan", "mcr_hdi_plan", "mcr_weighted_plan", "mcr_sbc_plan", "mcr_autocorr_plan", "mcrx_gaussian_workspace",
        "mci_indicator_plan", "mcb_batch_size"),
    "the profiler": ("mcr_profile_enable", "mcr_profile_reset", "mcr_profile_get", "mci_profile_enable", "mci_kernel_ms",
                     "mcb_profile_enable", "mcb_kernel_ms"),
    "the caller's own memory, and waiting": ("mcr_dev_alloc", "mcr_dev_free", "mcr_memcpy_h2d", "mcr_memcpy_d2h", "mcr_sync"),
    "a setting (REFUSED's *_under_the_limit entries set and restore it)": (
        "mcr_set_workspace_limit", "mci_set_workspace_limit", "mcb_set_workspace_limit"),
    "a counter": ("mcr_rho_guard_count", "mcr_tile_fallback_count"),
    "measurement and synthetic data: they write the caller's tensor only": ("mcr_hbm_probe", "mcr_fill_synthetic", "mcr_fill_synthetic_at"),
    "a host routine": ("mcr_energy_distance_host", "mcr_pareto_fit_host", "mcr_psis_host", "mcr_hdi_sorted_host", "mcr_weighted_host",
                       "mcr_sbc_ranks_host", "mcr_autocorr_host", "mcr_parquet_write_host", "mcr_csv_write_host",
                       "mcrx_cholesky_host", "mcrx_solve_lower_host", "mcrx_gaussian_check_host", "mci_indicator_ess_host",
                       "mcb_batch_means_host", "mcb_lrv_finish_host", "mcb_pool_host", "mcb_tree_sum_host"),
    "the communicator": ("mcr_comm_unique_id", "mcr_comm_init", "mcr_comm_free", "mcr_comm_world", "mcr_comm_rank", "mcr_comm_has_deadline",
                         "mcr_comm_all_gather", "mcr_comm_all_reduce", "mcr_comm_barrier"),
    "an accessor of a handle": (
        "mcr_parquet_num_rows", "mcr_parquet_num_columns", "mcr_parquet_column_name", "mcr_parquet_column_type", "mcr_parquet_num_pages",
        "mcr_parquet_page_info", "mcr_fileset_param_name", "mcr_fileset_field", "mcr_fileset_phases", "mcr_fileset_jobs",
        "mcr_csv_body_offset", "mcr_csv_table_flags"),
    "test_call_order_gpu.test_default_lanes calls it between the families": ("mcr_summarize_wait",),
    # Not among the reasons the matrix was planned with: the twin of an entry that IS in the matrix.  It carves the same
    # layout in the same buffers behind the caller's upload (or, for the images, behind another way to hand the bytes
    # over), and its own family's route tests hold it to the matrix entry's bits: mcrx_gaussian_check_dev in
    # test_gaussian_gpu.test_gaussian_check_against_long_double, mci_indicator_ess_dev in
    # test_indicator_gpu.test_routes_entries_and_dtypes_agree.  (mcr_covariance_dev, mcrx_cholesky_dev, mcrx_solve_lower_dev
    # and mcb_batch_means_dev are reached by the mean_shift_test family.)
    "the device-resident (or caller-image) twin of an entry in the matrix": (
        "mcr_summarize_dev", "mcr_summarize_models", "mcr_summarize_chains_enqueue", "mcr_summarize_chains_dev",
        "mcr_sliced_two_sample_dev", "mcr_energy_distance_dev", "mcr_nested_rhat_dev", "mcr_pareto_khat_dev", "mcr_psis_dev",
        "mcr_hdi_dev", "mcr_weighted_summary_dev", "mcr_sbc_ranks_dev", "mcr_autocorr_dev", "mcr_csv_open",
        "mcr_csv_open_table", "mcr_chain_layout_many_dev", "mcrx_gaussian_check_dev", "mci_indicator_ess_dev"),
    # Also outside the planned reasons: three small row utilities of the exporters, each one kernel on the caller's
    # buffers plus a counter word; test_csv_write_gpu and test_chain_layout_gpu run them behind summaries.
    "a row utility on the caller's buffers": ("mcr_select_rows_dev", "mcr_gather_rows_dev", "mcr_gather_rows_order_dev"),
}
