"""The context's buffers across calls: every buffer grows through one rule, the lanes own their workspaces, the staged
text is one piece of state, and a context can be made and freed any number of times.

Each result is compared with the oracle (the tolerances of test_hip_parity.py; for the ingest paths the host's own
reading of the same bytes) and, bit for bit, with the same call on a fresh context: a buffer that grew, shrank in use or
was borrowed by another entry point in between must not show in any result."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pqwrite_cases as W
import test_csv_gpu as TC
import test_csv_table_gpu as TT
import test_json_gpu as TJ
import test_parquet_write_gpu as TW
from test_hip_parity import TIGHT, check_summary, close

pytestmark = pytest.mark.gpu

SMALL, LARGE, MID = (4, 64, 3), (4, 8192, 33), (4, 4100, 20)      # (C, N, P)
# LARGE is 8.25 MiB of f64: past the 8 MiB threshold of the piecewise upload on the copy stream, three sort tiles per
# parameter, and larger than anything SMALL left in `stage`, the workspaces and the slots


def fresh_context():
    from mcmc_ref_hip import _ffi
    return _ffi.Context(0)


def same_bits(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a)


@pytest.fixture(scope="module")
def tensors():
    from mcmc_ref_hip import synth
    return {s: synth.c1_model(*s, seed=100 + s[1]) for s in (SMALL, LARGE, MID)}


@pytest.fixture(scope="module")
def expected(tensors, oracle):
    return {s: oracle.summarize(x, "pcn") for s, x in tensors.items()}


@pytest.fixture(scope="module")
def fresh(tensors, expected):
    """Every shape on a context of its own, held to the oracle here once."""
    out = {}
    for s, x in tensors.items():
        with fresh_context() as c:
            out[s] = c.summarize(x, "pcn")
        check_summary(out[s], expected[s], what=f"fresh{s}")
    return out


def test_two_fresh_contexts_agree_in_bits(tensors, fresh):
    """What lets the tests below ask for bit equality with a fresh context."""
    for s, x in tensors.items():
        with fresh_context() as c:
            assert same_bits(c.summarize(x, "pcn"), fresh[s]), s


# ---- 1. grow, shrink, grow ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [None, "1"])
def test_grow_shrink_grow_on_one_context(tensors, expected, fresh, monkeypatch, lanes):
    if lanes:
        monkeypatch.setenv("MCR_LANES", lanes)
    with fresh_context() as c:
        for k, s in enumerate([SMALL, LARGE, SMALL, LARGE]):
            got = c.summarize(tensors[s], "pcn")
            check_summary(got, expected[s], what=f"call {k} {s}")
            assert same_bits(got, fresh[s]), (k, s)


# ---- 2. growth with work in flight -------------------------------------------------------------------------------------

def test_buffers_grow_under_calls_in_flight(tensors, expected, fresh):
    """Eight small calls fill the window of MCR_MAX_INFLIGHT; every larger call that follows retires the oldest one only,
    so its workspace and slot grow while seven calls are still in flight."""
    from mcmc_ref_hip import _ffi
    with fresh_context() as c:
        ts = {s: c.upload(tensors[s], "pcn") for s in (SMALL, MID)}
        try:
            done = []
            for _ in range(_ffi.MCR_MAX_INFLIGHT):
                c.enqueue(ts[SMALL])
            for _ in range(8):
                done.append(c.wait_one())
                c.enqueue(ts[MID])
            assert c.inflight == _ffi.MCR_MAX_INFLIGHT
            while c.inflight:
                done.append(c.wait_one())
            assert len(done) == 16
            for k, b in enumerate(done):
                s = SMALL if k < 8 else MID
                check_summary(b.result(), expected[s], what=f"in flight {k}")
                assert same_bits(b.result(), fresh[s]), k
        finally:
            for t in ts.values():
                t.free()


# ---- 3. the ingest paths -----------------------------------------------------------------------------------------------

def hard_chain_text(seed: int, rows: int) -> str:
    """Four plain and four special fields per row: more hard fields than the hard list's first 4096 entries hold."""
    import random
    rng = random.Random(seed)
    special = ["inf", "nan", "-inf", "NaN"]
    header = ["lp__"] + [f"theta.{i + 1}" for i in range(7)]
    lines = [",".join(header)]
    for r in range(rows):
        lines.append(",".join(TC.number(rng, "%.17g") if (r + k) % 2 else special[(r + k) % 4] for k in range(8)))
    return "\n".join(lines) + "\n"


def draws_file(path, C_: int, N: int, P: int, seed: int):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(P, C_, N))
    cols = {"chain": np.repeat(np.arange(C_), N), "draw": np.tile(np.arange(N), C_)}
    cols.update({f"theta[{p + 1}]": x[p].reshape(-1) for p in range(P)})
    pq.write_table(pa.table(cols), path)
    return x


class Ingest:
    """The files of both sizes, written once; run(ctx, kind, size) makes one call and returns what it decoded in a form
    that compares with ==; want(kind, size) is the same call on a fresh context, held to the host's reading once."""
    KINDS = ["chain_csv", "json", "files", "table_csv", "write"]

    def __init__(self, d, oracle):
        self.oracle, self.f, self._want = oracle, {}, {}
        for size, big in (("small", False), ("large", True)):
            texts = [hard_chain_text(7 + c, 2000) for c in range(2)] if big else [TC.chain_text(3 + c, 2, 1, comments=False) for c in range(2)]
            self.f["chain_csv", size] = dict(texts=texts, paths=[TC.write(d, f"{size}{c}.csv", t) for c, t in enumerate(texts)])
            doc = TJ.document(5, 2, 4, 2000) if big else TJ.document(6, 2, 1, 3)
            self.f["json", size] = dict(text=doc, path=TJ.archive(d, size, doc))
            shapes = [(4, 5000, 3), (4, 5000, 2)] if big else [(4, 8, 1), (2, 10, 2)]
            paths = [d / f"{size}{k}.draws.parquet" for k in range(2)]
            self.f["files", size] = dict(paths=paths, x=[draws_file(p, *s, seed=40 + k) for k, (p, s) in enumerate(zip(paths, shapes))])
            data = TT.write_table(4, 1000, 5, "%.17g", "both", TT.ENDS[0], 9) if big else TT.write_table(2, 3, 1, "%.17g", "both", TT.ENDS[0], 4)
            self.f["table_csv", size] = dict(data=data, path=TT.put(d, f"{size}_table", data))
            rows = 2 * W.PAGE_ROWS + 3 if big else 5
            self.f["write", size] = dict(cols=TW.matrix_columns(rows, 21)[0], rows=rows)
        assert all(300 << 10 > len(t) > 100 << 10 for t in self.f["chain_csv", "large"]["texts"])
        assert len(self.f["json", "large"]["text"]) > 200 << 10 and len(self.f["table_csv", "large"]["data"]) > 200 << 10
        assert len(self.f["chain_csv", "small"]["texts"][0]) < 1000 and len(self.f["json", "small"]["text"]) < 1000

    def run(self, ctx, kind: str, size: str):
        f = self.f[kind, size]
        if kind == "chain_csv":
            names, got, hard = TC.decode(ctx, f["paths"])
            return names, got.shape, got.tobytes(), hard
        if kind == "json":
            got, ph = TJ.read_dev(ctx, f["path"])
            assert got is not None, ph
            return got[0], got[1].shape, got[1].tobytes(), list(got[2]), ph["hard"]
        if kind == "files":
            from mcmc_ref_hip import parquet
            return repr(parquet._summarize_paths(ctx, [str(p) for p in f["paths"]], 2, [0.05, 0.5, 0.95], True))
        if kind == "table_csv":
            from mcmc_ref_hip import convert
            ph: dict = {}
            got = convert.read_csv_dev(f["path"], context=ctx, phases=ph)
            assert got is not None and "fallback" not in ph, ph
            d, fbuf, ints = got
            try:
                n = len(d.params) * int(np.sum(d.counts))
                return d.params, fbuf.download(np.float64, n).tobytes(), np.ascontiguousarray(d.to_host()).tobytes(), list(ints), ph["hard"]
            finally:
                d.free()
                fbuf.free()
        return TW.write_dev(ctx, f["cols"], f["rows"])

    def want(self, kind: str, size: str):
        if (kind, size) not in self._want:
            with fresh_context() as c:
                got = self._want[kind, size] = self.run(c, kind, size)
                self.check_host(c, kind, size, got)
        return self._want[kind, size]

    def check_host(self, ctx, kind: str, size: str, got):
        f = self.f[kind, size]
        if kind == "chain_csv":
            from mcmc_ref_hip import cmdstan_generate as cs
            per = [TC.expected_from_text(t) for t in f["texts"]]
            at = [[[cs._normalize_cmdstan_param_name(h) for h in header].index(n) for header, _ in per] for n in got[0]]
            exp = np.array([[[row[at[k][c]] for row in rows] for c, (_, rows) in enumerate(per)] for k in range(len(got[0]))], dtype=np.float64)
            assert TC.same_bits(np.frombuffer(got[2]).reshape(got[1]), exp)
            assert size == "small" or got[3] > 4096          # the hard list overflowed on this fresh context
        elif kind == "json":
            params, exp, ints = TJ.expected_from_text(f["text"])
            assert got[0] == params and got[3] == ints and TJ.same_bits(np.frombuffer(got[2]).reshape(got[1]), exp)
        elif kind == "files":
            from mcmc_ref_hip import parquet
            res = parquet._summarize_paths(ctx, [str(p) for p in f["paths"]], 2, [0.05, 0.5, 0.95], True)
            for x, r in zip(f["x"], res):
                exp = self.oracle.summarize(x, "pcn", min_chains=2)
                for p in range(x.shape[0]):
                    e = r[f"theta[{p + 1}]"]
                    assert close(e["mean"], exp["mean"][p], TIGHT, scale=TIGHT * float(exp["std"][p]))
                    assert [e["q5"], e["q50"], e["q95"]] == [float(v) for v in exp["q"][p]]
                    for k in ("std", "rhat", "ess_bulk", "ess_tail"):
                        assert close(e[k], exp[k][p], TIGHT), (k, p)
        elif kind == "table_csv":
            table = TT.read_host(f["data"])
            flat = np.frombuffer(got[1]).reshape(len(got[0]), -1)
            for p, name in enumerate(got[0]):
                assert np.array_equal(flat[p].view(np.uint64), table.column(name).to_numpy().astype(np.float64).view(np.uint64)), name
        else:
            W.check_file(ctx.lib, got, f["cols"], f["rows"], 0)


@pytest.fixture(scope="module")
def ingest(tmp_path_factory, oracle):
    return Ingest(tmp_path_factory.mktemp("ingest"), oracle)


@pytest.mark.parametrize("kind", Ingest.KINDS)
def test_each_ingest_path_small_large_small(ingest, kind):
    with fresh_context() as c:
        for k, size in enumerate(["small", "large", "small"]):
            assert ingest.run(c, kind, size) == ingest.want(kind, size), (kind, k, size)


def test_ingest_paths_interleaved_on_one_context(ingest):
    """Every path borrows the file image, the parse scratch or the lane workspace from the one before it."""
    order = ["chain_csv", "json", "files", "table_csv", "write", "chain_csv"]
    with fresh_context() as c:
        for size in ("large", "small"):
            for k, kind in enumerate(order):
                assert ingest.run(c, kind, size) == ingest.want(kind, size), (size, k, kind)


# ---- 4. stale staging ---------------------------------------------------------------------------------------------------

def test_a_decode_after_another_writer_of_the_staged_tables_is_refused():
    """mcr_json_open borrows the buffer of the staged row starts: the decode that follows must say so on the host (before
    any launch or copy: it is the first thing mcr_csv_decode checks after its arguments) and staging again must work."""
    from mcmc_ref_hip import _ffi
    text = b"a,b\n1.5,2.5\n-3.25,4e3\n"
    doc = b'[{"x":[1,2,3],"y":[4.5,5.5,6.5]}]'
    with fresh_context() as c:
        L = c.lib
        image = ctypes.create_string_buffer(text, len(text))
        h = ctypes.c_void_p()
        assert L.mcr_csv_open(None, image, len(text), ctypes.byref(h)) == 0
        hs = (ctypes.c_void_p * 1)(h)
        rows = np.zeros(1, dtype=np.int64)
        cols = np.array([[0, 1]], dtype=np.intc)
        out = _ffi.DeviceBuffer(c, 4 * 8)
        hard = ctypes.c_int64(-1)

        def stage():
            c._check(L.mcr_csv_stage(c.handle, hs, 1, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            assert rows.tolist() == [2]

        def decode() -> int:
            return L.mcr_csv_decode(c.handle, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 2, 2, out.ptr, 4, 2, 1, ctypes.byref(hard))
        try:
            stage()
            j = ctypes.c_void_p()
            c._check(L.mcr_json_open(c.handle, doc, len(doc), ctypes.byref(j)))
            try:
                assert decode() == _ffi.MCR_EINVAL
                assert b"no staged files" in L.mcr_last_error(c.handle)
            finally:
                L.mcr_json_close(j)
            stage()
            assert decode() == 0 and hard.value == 0
            assert out.download(np.float64, 4).tolist() == [1.5, 2.5, -3.25, 4000.0]
        finally:
            out.free()
            L.mcr_csv_close(h)


# ---- 5. context lifetime -------------------------------------------------------------------------------------------------

def test_contexts_made_and_freed_in_one_process(tensors, expected, fresh, tmp_path):
    text = TC.chain_text(77, 5, 2)
    path = TC.write(tmp_path, "life.csv", text)
    first = None
    for k in range(3):
        with fresh_context() as c:
            got = c.summarize(tensors[SMALL], "pcn")
            check_summary(got, expected[SMALL], what=f"round {k}")
            assert same_bits(got, fresh[SMALL]), k
            TC.check_files(c, [path], [text])
            names, arr, _ = TC.decode(c, [path])
        first = first or (names, arr.tobytes())
        assert (names, arr.tobytes()) == first, k


def test_init_on_a_device_out_of_range_leaves_nothing_behind():
    from mcmc_ref_hip import _ffi
    L = _ffi.load_library()
    h = ctypes.c_void_p()
    assert L.mcr_init(L.mcr_device_count(), ctypes.byref(h)) == _ffi.MCR_ENODEVICE
    assert h.value is None and b"out of range" in L.mcr_last_error(None)
    with pytest.raises(_ffi.HipUnavailableError):
        _ffi.Context(1 << 20)
