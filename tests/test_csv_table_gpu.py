"""Table CSVs parsed on the GPU: `Context.csv_table_decode`, `convert.read_csv_dev`,
`convert_files(reader="auto")`, `summarize_csv` / `csv-summary`.

The expected table is `pyarrow.csv.read_csv` of the same bytes -- the reader the host route uses -- and every value is
compared bit for bit, every column type and every chain count exactly."""
from __future__ import annotations

import io
import json
import zipfile
from datetime import date
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 16384            # MCR_CSV_CHUNK (include/mcmcref_hip.h): bytes of text per workgroup of the line index
MID = "1.00000000000000011102230246251565404236316680908203125"      # 1 + 2^-53: halfway between 1 and its successor


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    with _ffi.Context(0) as c:
        yield c


def read_host(data: bytes):
    import pyarrow.csv as pacsv
    return pacsv.read_csv(io.BytesIO(data))


def put(tmp_path: Path, name: str, data: bytes) -> Path:
    path = tmp_path / f"{name}.csv"
    path.write_bytes(data)
    return path


def check_against_pyarrow(ctx, path: Path, data: bytes, min_hard: int = 0) -> dict:
    """The device route is taken and gives pyarrow's table: values in bits, column types, chains and counts, and the
    draws in (chain, draw) order equal `table_to_tensor` of that table."""
    import pyarrow as pa
    from mcmc_ref_hip import convert
    table = read_host(data)
    phases: dict = {}
    got = convert.read_csv_dev(path, context=ctx, phases=phases)
    assert got is not None and "fallback" not in phases, phases
    d, fbuf, ints = got
    try:
        params = [c for c in table.column_names if c not in ("chain", "draw")]
        assert d.params == params
        P, M = len(params), table.num_rows
        flat = fbuf.download(np.float64, P * M).reshape(P, M)
        for p, name in enumerate(params):
            col = table.column(name)
            assert col.type in (pa.int64(), pa.float64()), (name, col.type)
            assert ints[p] == (col.type == pa.int64()), (name, col.type, ints[p])
            want = col.to_numpy()
            if ints[p]:
                assert np.array_equal(flat[p].astype(np.int64), want), name
                assert np.array_equal(flat[p], want.astype(np.float64)), name
            else:
                assert np.array_equal(flat[p].view(np.uint64), want.view(np.uint64)), name
        full = convert._ensure_chain_draw(table)
        ids, _order, counts = convert.chain_layout(full)
        assert np.array_equal(d.chain_ids, ids) and np.array_equal(d.counts, counts), (d.chain_ids, ids, d.counts, counts)
        x, _ = convert.table_to_tensor(full, params)
        assert np.array_equal(d.to_host().view(np.uint64), np.ascontiguousarray(x, dtype=np.float64).view(np.uint64))
        assert phases["hard"] >= min_hard, phases
    finally:
        d.free()
        fbuf.free()
    return phases


# ---- writer matrix ---------------------------------------------------------------------------------------------------
FORMATS = ["%.6g", "%.17g", "repr", "mixed"]
IDS = ["both", "chain", "draw", "none"]
ENDS = [("\n", True, False), ("\r\n", True, False), ("\n", False, False), ("\r\n", False, False), ("\n", True, True),
        ("\r\n", True, True)]          # (line end, final newline, empty lines inside the body and at the end)


def write_table(C_: int, N: int, P: int, fmt: str, ids: str, end: tuple, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    M = C_ * N
    x = rng.standard_normal((M, P)) * 10.0 ** rng.integers(-3, 4, size=(1, P))
    names = [f"p{j}" for j in range(P)]
    cols = []
    for j in range(P):
        if fmt == "mixed" and j % 3 == 0:
            cols.append([str(int(v)) for v in rng.integers(-1000, 1000, size=M)])
        elif fmt in ("repr", "mixed"):
            cols.append([repr(float(v)) for v in x[:, j]])
        else:
            cols.append([fmt % v for v in x[:, j]])
    if ids in ("both", "chain"):
        at = min(seed % (P + 1), len(names))
        names.insert(at, "chain")
        cols.insert(at, [str(c) for c in np.repeat(np.arange(C_), N)])
    if ids in ("both", "draw"):
        at = min((seed // 3) % (P + 1), len(names))
        names.insert(at, "draw")
        cols.insert(at, [str(n) for n in np.tile(np.arange(N), C_)])
    nl, final, empties = end
    lines = [",".join(names)] + [",".join(r) for r in zip(*cols)]
    if empties:
        lines.insert(0, "")
        for k in range(len(lines) - 1, 1, -max(M // 3, 1)):
            lines.insert(k, "")
    text = nl.join(lines) + (nl if final else "")
    if empties:
        text += nl + nl
    return text.encode()


@pytest.mark.parametrize("P", [1, 2, 7, 300])
@pytest.mark.parametrize("C_", [1, 2, 4])
def test_writer_matrix_equals_pyarrow(ctx, tmp_path, C_, P):
    for k, N in enumerate([1, 2, 63, 64, 65, 1000]):
        case = ([1, 2, 4].index(C_) * 4 + [1, 2, 7, 300].index(P)) * 6 + k     # 0 .. 71
        fmt, ids, end = FORMATS[case % 4], IDS[(case // 4 + case // 16) % 4], ENDS[(case + case // 6) % 6]
        if P == 300 and N == 1000:
            fmt = "%.6g"                                     # the widest table: short text keeps the case quick
        data = write_table(C_, N, P, fmt, ids, end, seed=case)
        check_against_pyarrow(ctx, put(tmp_path, f"w{N}", data), data)


def test_every_writer_variant_with_rows_longer_than_a_batch_and_without_commas(ctx, tmp_path):
    """Each format x id set x line end once more on two fixed shapes, so that none depends on the walk above."""
    k = 0
    for fmt in FORMATS:
        for ids in IDS:
            end = ENDS[k % 6]
            for C_, N, P in [(2, 5, 1), (3, 7, 9)]:
                data = write_table(C_, N, P, fmt, ids, end, seed=100 + k)
                check_against_pyarrow(ctx, put(tmp_path, f"v{k}_{P}", data), data)
            k += 1
    for end in ENDS:
        data = write_table(4, 3, 2, "repr", "both", end, seed=7)
        check_against_pyarrow(ctx, put(tmp_path, "e", data), data)


# ---- edges of the index and the parser ------------------------------------------------------------------------------
def doc_with_row_at(target: int, nl: str = "\n") -> bytes:
    """A two-column document one of whose rows starts exactly at byte `target`."""
    text = "a,b" + nl
    row = "1.5,2" + nl
    while target - len(text) >= len(row) + 40:
        text += row
    fill = target - len(text)                                # one row of exactly this many bytes
    if fill:
        text += "1." + "0" * (fill - len(",2" + nl) - 2) + ",2" + nl
    assert len(text) == target
    return (text + "3.25,4" + nl + "-7e-3,8" + nl).encode()


@pytest.mark.parametrize("edge", [CHUNK, 2 * CHUNK, 192, 64 * 100])
def test_row_starts_at_chunk_and_thread_edges(ctx, tmp_path, edge):
    for delta in (-1, 0, 1):
        for nl in ("\n", "\r\n"):
            data = doc_with_row_at(edge + delta, nl)
            check_against_pyarrow(ctx, put(tmp_path, f"r{delta}", data), data)


def test_fields_at_batch_edges_and_long_fields(ctx, tmp_path):
    # a row's first batch holds the byte in front of it and its first 63 bytes: first fields of 58 .. 70 bytes end
    # before, exactly on and after that edge, and the field behind them starts in the last lane or straddles
    rows = ["1." + "5" * (n - 2) + ",2.5," + "0." + "3" * 70 for n in range(58, 71)]
    rows += ["1,2." + "7" * (n - 4) + ",3" for n in range(58, 71)]
    rows += ["-" + "1" * 15 + ",0.5,-4e-3"]
    data = ("a,b,c\n" + "\n".join(rows) + "\n").encode()
    check_against_pyarrow(ctx, put(tmp_path, "edges", data), data)
    # longer than a batch, with digits past the 19th that decide the rounding: the host finishes them
    rows = [MID + "0" * 30 + ",1", MID + "0" * 30 + "1,2", "-" + MID + ",3", "0." + "0" * 80 + MID.replace(".", "") + ",4"]
    data = ("a,b\n" + "\n".join(rows)).encode()
    phases = check_against_pyarrow(ctx, put(tmp_path, "hard", data), data, min_hard=1)
    assert phases["hard"] >= 3


def test_a_hard_list_that_overflows_is_parsed_once_more(tmp_path):
    """5 961 of the 6 000 value fields are midpoints of neighbouring doubles whose digits past the 19th decide: more
    than the first capacity of the hard list (4 096), so the parse runs again with a list that fits."""
    import random

    import pyarrow as pa
    from mcmc_ref_hip import _ffi
    from test_csv_gpu import halfway
    rng = random.Random(13)
    rows = [f"{c},{n},{halfway(rng)},{halfway(rng)}" for c in range(4) for n in range(750)]
    data = ("chain,draw,x,y\n" + "\n".join(rows) + "\n").encode()
    assert read_host(data).schema.types == [pa.int64(), pa.int64(), pa.float64(), pa.float64()]
    with _ffi.Context(0) as fresh:                           # its capacity is the initial one whatever the module's has seen
        check_against_pyarrow(fresh, put(tmp_path, "overflow", data), data, min_hard=4097)


def test_type_inference_covers_the_whole_file(ctx, tmp_path):
    import pyarrow as pa
    lines = ["a,b"] + [f"{k},{k % 7}" for k in range(6000)] + ["1.5,3"]
    data = "\n".join(lines).encode()
    assert len(data) > 2 * CHUNK
    assert read_host(data).schema.types == [pa.float64(), pa.int64()]
    check_against_pyarrow(ctx, put(tmp_path, "late", data), data)
    # and across pyarrow's own blocks of 1 MB: the only non-integer literal lies in the file's last row, past the second
    lines = ["a,b"] + [f"{k},{k % 7}" for k in range(260_000)] + ["1.5,3"]
    data = "\n".join(lines).encode()
    assert len(data) > 2 * (1 << 20)
    assert read_host(data).schema.types == [pa.float64(), pa.int64()]
    check_against_pyarrow(ctx, put(tmp_path, "late", data), data)


def test_negative_zero_and_the_largest_integers(ctx, tmp_path):
    import pyarrow as pa
    from mcmc_ref_hip import convert
    data = b"d,i,big\n-0,-0,9007199254740992\n1.5,3,-9007199254740992\n-0.0,0,0\n"
    table = read_host(data)
    assert table.schema.types == [pa.float64(), pa.int64(), pa.int64()]
    check_against_pyarrow(ctx, put(tmp_path, "zero", data), data)
    d, fbuf, ints = convert.read_csv_dev(put(tmp_path, "zero", data), context=ctx)
    flat = fbuf.download(np.float64, 9).reshape(3, 3)
    d.free()
    fbuf.free()
    assert ints == [False, True, True]
    assert np.signbit(flat[0, 0]) and np.signbit(flat[0, 2])          # the double column keeps the sign, as pyarrow does
    assert not np.signbit(flat[1, 0])                                 # an int64 column has no negative zero: +0.0 resident
    phases: dict = {}
    assert convert.read_csv_dev(put(tmp_path, "big", b"a\n1\n9007199254740993\n"), context=ctx, phases=phases) is None
    assert "above 2^53" in phases["fallback"]


# ---- rows out of order, ragged chains ---------------------------------------------------------------------------------
def long_table(counts, P: int, seed: int, shuffle: bool) -> bytes:
    rng = np.random.default_rng(seed)
    rows = []
    for c, n in enumerate(counts):
        for k in range(n):
            rows.append(",".join([str(10 + 3 * c), str(k)] + [repr(float(v)) for v in rng.standard_normal(P)]))
    if shuffle:
        rng.shuffle(rows)
    return ("chain,draw," + ",".join(f"x{j}" for j in range(P)) + "\n" + "\n".join(rows) + "\n").encode()


def test_shuffled_ragged_and_many_chain_tables(ctx, tmp_path):
    from mcmc_ref_hip import convert
    for name, counts, shuffle in [("shuffled", [50] * 4, True), ("ragged", [50, 49, 50, 1], False),
                                  ("ragged_shuffled", [50, 49, 50, 1], True)]:
        data = long_table(counts, 3, 11, shuffle)
        phases = check_against_pyarrow(ctx, put(tmp_path, name, data), data)
        assert "layout" not in phases                        # the device layout code ordered them
    data = long_table([2] * 300, 2, 12, True)                # more than 256 chains: the host's lexsort
    phases = check_against_pyarrow(ctx, put(tmp_path, "many", data), data)
    assert phases.get("layout") == "host"

    data = long_table([50] * 4, 3, 13, True)
    path = put(tmp_path, "sum", data)
    table = read_host(data)
    want = convert.summarize_table(table, ["x0", "x1", "x2"], context=ctx)
    assert same_numbers(convert.summarize_csv(path, context=ctx), want)
    data = long_table([50, 49, 50, 1], 3, 14, True)
    x, counts = convert.table_to_tensor(read_host(data), ["x0", "x1", "x2"])
    from mcmc_ref_hip import _ffi
    r = ctx.summarize_chains(x, counts)
    want = dict(zip(["x0", "x1", "x2"], _ffi.entries(r, [0.05, 0.5, 0.95], True)))
    assert same_numbers(convert.summarize_csv(put(tmp_path, "sumr", data), context=ctx), want)


# ---- fallbacks ---------------------------------------------------------------------------------------------------------
BODY = "chain,draw,a\n" + "".join(f"{c},{k},{c + k / 8}\n" for c in range(4) for k in range(6))
FALLBACKS = {      # condition of the list in include/mcmcref_hip.h -> (document, words of the reason)
    "quote_in_body": (BODY + '0,6,"1.5"\n', "'\"'"),
    "quote_in_header": ('chain,draw,"a"\n0,0,1.5\n', "'\"' in the header"),
    "empty_field": (BODY + "0,6,\n", "outside the number grammar"),
    "space": (BODY + "0,6, 1.5\n", "outside the number grammar"),
    "plus": (BODY + "0,6,+1.5\n", "outside the number grammar"),
    "leading_zero": (BODY + "0,6,01\n", "outside the number grammar"),
    "dot_five": (BODY + "0,6,.5\n", "outside the number grammar"),
    "five_dot": (BODY + "0,6,5.\n", "outside the number grammar"),
    "inf": (BODY + "0,6,inf\n", "outside the number grammar"),
    "nan": (BODY + "0,6,nan\n", "outside the number grammar"),
    "boolean": (BODY + "0,6,true\n", "outside the number grammar"),
    "date": (BODY + "0,6,2020-01-01\n", "outside the number grammar"),
    "text": (BODY + "0,6,abc\n", "outside the number grammar"),
    "big_integer": (BODY + "0,6,9007199254740993\n", "above 2^53"),
    "short_row": (BODY + "0,6\n", "field count"),
    "long_row": (BODY + "0,6,1.5,2\n", "field count"),
    "lone_cr": (BODY + "0,6,1.5\r0,7,2.5\n", "carriage return without a line feed"),
    "lone_cr_at_the_end": (BODY + "0,6,1.5\r", "carriage return without a line feed"),
    "whitespace_line": (BODY + "  \n0,6,1.5\n", "whitespace-only line"),
    "byte_order_mark": ("\ufeff" + BODY, "byte-order mark"),
    "duplicate_name": ("chain,draw,a,a\n0,0,1,2\n", "duplicated header name"),
    "empty_name": ("chain,draw,,a\n0,0,1,2\n", "empty header name"),
    "id_not_integer": (BODY + "0.5,6,1.5\n", "id column"),
    "id_exponent": (BODY + "0,1e1,1.5\n", "id column"),
    "no_rows": ("chain,draw,a\n", "no data rows"),
    "no_rows_no_newline": ("chain,draw,a", "no data rows"),
    "empty_file": ("", "no header"),
}


def outcome(result):
    """What a convert_files entry is, comparably: the exception's type and text, or the written files."""
    import pyarrow.parquet as pq
    if isinstance(result, Exception):
        return type(result), str(result)
    return pq.read_table(result.draws_path), result.meta_path.read_text(), json.dumps(result.meta, sort_keys=True)


def same_outcome(a, b) -> bool:
    if len(a) == 2 or len(b) == 2:                           # an exception: the same type and text
        return len(a) == len(b) and a == b
    return a[0].schema.equals(b[0].schema) and a[0].equals(b[0]) and a[1] == b[1] and a[2] == b[2]


def same_numbers(a: dict, b: dict) -> bool:
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)      # repr round-trips every double; NaN equals NaN


def convert_both(ctx, tmp_path: Path, jobs, force=True):
    from mcmc_ref_hip import convert
    outs = []
    for reader in ("auto", "host"):
        out = tmp_path / f"out_{reader}"
        (out / "draws").mkdir(parents=True, exist_ok=True)
        (out / "meta").mkdir(parents=True, exist_ok=True)
        outs.append(convert.convert_files(jobs, out / "draws", out / "meta", force=force, context=ctx, reader=reader))
    return outs


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_every_fallback_condition_goes_to_the_host_reader(ctx, tmp_path, name):
    from mcmc_ref_hip import convert
    text, words = FALLBACKS[name]
    path = put(tmp_path, name, text.encode())
    phases: dict = {}
    assert convert.read_csv_dev(path, context=ctx, phases=phases) is None
    assert words in phases["fallback"] and str(path) in phases["fallback"], phases
    auto, host = convert_both(ctx, tmp_path, [(path, name)])
    assert same_outcome(outcome(auto[0]), outcome(host[0])), (auto[0], host[0])


def test_the_fallback_message_names_the_first_reason_and_its_byte(ctx, tmp_path):
    from mcmc_ref_hip import convert
    text = BODY + "0,6,abc\n0,7,9007199254740993\n"
    phases: dict = {}
    assert convert.read_csv_dev(put(tmp_path, "first", text.encode()), context=ctx, phases=phases) is None
    assert "outside the number grammar" in phases["fallback"] and f"(byte {len(BODY) + 4})" in phases["fallback"], phases
    # a '"' behind another reason in the same row and the same 64 bytes does not hide it; alone it is named, with its byte
    for text, words, byte in [(BODY + '0,abc,"1"\n', "outside the number grammar", len(BODY) + 2),
                              (BODY + '0,+6,"1"\n', "outside the number grammar", len(BODY) + 2),
                              (BODY + '0,6,1"5\n0,7,abc\n', "a '\"'", len(BODY) + 5),
                              (BODY + '0,6,"1.5"\n', "a '\"'", len(BODY) + 4)]:
        phases = {}
        assert convert.read_csv_dev(put(tmp_path, "first", text.encode()), context=ctx, phases=phases) is None
        assert words in phases["fallback"] and f"(byte {byte})" in phases["fallback"], (text[len(BODY):], phases)


# ---- convert_files on a batch --------------------------------------------------------------------------------------------
def json_zip(path: Path, C_: int, N: int, seed: int) -> Path:
    rng = np.random.default_rng(seed)
    doc = [{"mu": rng.standard_normal(N).tolist(), "k": rng.integers(0, 9, N).tolist()} for _ in range(C_)]
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr(path.name[:-4], json.dumps(doc))
    return path


def test_convert_files_on_a_mixed_batch_equals_the_host_route(ctx, tmp_path):
    from click.testing import CliRunner

    from mcmc_ref_hip import cli, convert
    jobs = [
        (put(tmp_path, "a", write_table(4, 60, 3, "mixed", "both", ENDS[0], 1)), "a"),
        (json_zip(tmp_path / "j1.json.zip", 4, 40, 2), "j1"),
        (put(tmp_path, "b", write_table(4, 33, 2, "%.17g", "chain", ENDS[1], 3)), "b"),
        (put(tmp_path, "poisoned", long_table([20] * 4, 2, 4, False) + b"10,20,nan,1.5\n"), "poisoned"),
        (put(tmp_path, "c", write_table(1, 50, 2, "repr", "none", ENDS[4], 5)), "c"),
        (put(tmp_path, "ragged", long_table([30, 29, 30, 7], 2, 6, True)), "ragged"),
        (json_zip(tmp_path / "j2.json.zip", 5, 25, 7), "j2"),
        (put(tmp_path, "d", write_table(2, 10, 1, "%.6g", "draw", ENDS[3], 8)), "d"),
        (tmp_path / "missing.csv", "missing"),
    ]
    phases: dict = {}
    assert convert.read_csv_dev(jobs[3][0], context=ctx, phases=phases) is None and "number grammar" in phases["fallback"]
    for k in (0, 2, 4, 5, 7):                               # the others take the device route
        got = convert.read_csv_dev(jobs[k][0], context=ctx)
        assert got is not None
        got[0].free()
        got[1].free()
    auto, host = convert_both(ctx, tmp_path, jobs)
    assert len(auto) == len(host) == len(jobs)
    for (path, name), a, h in zip(jobs, auto, host):
        assert same_outcome(outcome(a), outcome(h)), (name, a, h)
    assert isinstance(auto[3], ValueError) and isinstance(auto[8], Exception)
    for k in (0, 2, 5):
        assert not isinstance(auto[k], Exception), auto[k]
    assert auto[0].meta["generated_date"] == date.today().isoformat()
    assert (tmp_path / "out_auto" / "meta" / "a.meta.json").read_text() == (tmp_path / "out_host" / "meta" / "a.meta.json").read_text()
    # the quality gate raises the same on both routes
    strict = convert_both(ctx, tmp_path / "strict", jobs[:3], force=False)
    for a, h in zip(*strict):
        assert same_outcome(outcome(a), outcome(h)), (a, h)

    path = jobs[0][0]
    want = convert.summarize_csv(path, context=ctx)
    r = CliRunner().invoke(cli.main, ["csv-summary", str(path), "--format", "json"])
    assert r.exit_code == 0, r.output
    assert same_numbers(json.loads(r.output), want)
    r = CliRunner().invoke(cli.main, ["csv-summary", str(path), str(jobs[2][0]), "--format", "json"])
    assert r.exit_code == 0 and set(json.loads(r.output)) == {str(path), str(jobs[2][0])}
    r = CliRunner().invoke(cli.main, ["csv-summary", str(jobs[7][0])])
    assert r.exit_code != 0 and "chain" in r.output


def recorded_decodes(monkeypatch, refuse=lambda paths: None):
    """Every Context.csv_table_decode call's paths from here on; `refuse(paths)` may give the library's message of a
    call that it ends with MCR_EINVAL."""
    from mcmc_ref_hip import _ffi
    calls = []
    real = _ffi.Context.csv_table_decode

    def decode(self, paths, phases=None):
        calls.append([Path(p).name for p in paths])
        why = refuse(paths)
        if why:
            raise _ffi.McrError(_ffi.MCR_EINVAL, why)
        return real(self, paths, phases)

    monkeypatch.setattr(_ffi.Context, "csv_table_decode", decode)
    return calls


def test_a_job_the_library_cannot_read_leaves_the_others_and_its_host_exception(ctx, tmp_path, monkeypatch):
    """What the library answers besides MCR_EFALLBACK -- a file it cannot open, text beyond its limit -- is the host
    reader's job as well: the other jobs keep the device route, and every result equals reader="host"."""
    from mcmc_ref_hip import convert
    locked = put(tmp_path, "locked", write_table(4, 12, 2, "repr", "both", ENDS[0], 31))
    locked.chmod(0)                                          # (a user who may read it anyway gets equal files instead)
    jobs = [
        (put(tmp_path, "a", write_table(4, 30, 2, "repr", "both", ENDS[0], 32)), "a"),
        (locked, "locked"),
        (json_zip(tmp_path / "j.json.zip", 4, 20, 33), "j"),
        (put(tmp_path, "huge", write_table(4, 25, 3, "%.17g", "chain", ENDS[1], 34)), "huge"),
        (put(tmp_path, "b", write_table(4, 18, 1, "mixed", "none", ENDS[2], 35)), "b"),
    ]
    limit = "csv: the files of one call hold 4398046511104 bytes; the limit is 4 GiB"
    calls = recorded_decodes(monkeypatch, lambda paths: limit if any(Path(p).name == "huge.csv" for p in paths) else None)
    try:
        auto, host = convert_both(ctx, tmp_path, jobs)
    finally:
        locked.chmod(0o600)
    for (path, name), a, h in zip(jobs, auto, host):
        assert same_outcome(outcome(a), outcome(h)), (name, a, h)
    for k in (0, 2, 3, 4):
        assert not isinstance(auto[k], Exception), auto[k]
    assert ["a.csv"] in calls and ["b.csv"] in calls and ["huge.csv"] in calls      # read one by one after the refusal
    assert calls[0] == ["a.csv", "locked.csv", "huge.csv", "b.csv"]

    # the jobs of a batch are read in groups that stay below the library's limit for one call
    calls.clear()
    monkeypatch.setattr(convert, "_CSV_BATCH_BYTES", jobs[0][0].stat().st_size + 10)
    small = [jobs[0], jobs[4], jobs[2]]
    auto, host = convert_both(ctx, tmp_path / "groups", small)
    for a, h in zip(auto, host):
        assert not isinstance(a, Exception) and same_outcome(outcome(a), outcome(h)), (a, h)
    assert calls[:2] == [["a.csv"], ["b.csv"]]


def test_a_file_that_falls_back_is_dropped_from_the_batch_and_the_rest_read_once_more(ctx, tmp_path, monkeypatch):
    jobs = [(put(tmp_path, f"g{k}", write_table(4, 10 + k, 2, "repr", "both", ENDS[k % 6], 40 + k)), f"g{k}") for k in range(4)]
    jobs.insert(2, (put(tmp_path, "bad", long_table([20] * 4, 2, 4, False) + b"10,20,nan,1.5\n"), "bad"))
    jobs.append((tmp_path / "gone.csv", "gone"))
    calls = recorded_decodes(monkeypatch)
    auto, host = convert_both(ctx, tmp_path, jobs)
    for (path, name), a, h in zip(jobs, auto, host):
        assert same_outcome(outcome(a), outcome(h)), (name, a, h)
    assert isinstance(auto[5], FileNotFoundError) and isinstance(auto[2], ValueError)
    good = ["g0.csv", "g1.csv", "g2.csv", "g3.csv"]
    assert calls == [good[:2] + ["bad.csv"] + good[2:], good]       # (the missing path never reaches the library)


# ---- several files in one call ----------------------------------------------------------------------------------------
def test_several_files_in_one_decode_call_equal_their_single_file_results(ctx, tmp_path):
    datas = [write_table(4, 65, 7, "mixed", "both", ENDS[1], 21), write_table(1, 1, 1, "repr", "none", ENDS[2], 22),
             write_table(2, 1000, 2, "%.17g", "chain", ENDS[4], 23), long_table([9, 3, 5], 4, 24, True),
             ("a,b\n" + MID + "1,2\n3,4\n").encode()]
    paths = [str(put(tmp_path, f"m{k}", d)) for k, d in enumerate(datas)]

    def snapshot(entries):
        out = []
        for names, buf, ints, ids, hard, header in entries:
            M = buf.nbytes // 8 // max(len(names), 1)
            out.append((names, buf.download(np.uint64, len(names) * M).tolist(), ints.tolist(),
                        [None if b is None else b.download(np.int64, b.nbytes // 8).tolist() for b in ids], header))
            for b in (buf, *ids):
                if b is not None:
                    b.free()
        return out

    phases: dict = {}
    together = snapshot(ctx.csv_table_decode(paths, phases))
    assert "fallback" not in phases and phases["hard"] == 1
    alone = [snapshot(ctx.csv_table_decode([p]))[0] for p in paths]
    assert together == alone
    for (names, _v, _i, ids, header), data in zip(together, datas):
        table = read_host(data)
        assert header == table.column_names and names == [c for c in header if c not in ("chain", "draw")]
        for which, b in zip(("chain", "draw"), ids):
            assert (b is None) == (which not in header)
            if b is not None:
                assert b == table.column(which).to_pylist()
