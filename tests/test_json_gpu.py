"""Chain-list JSON archives parsed on the GPU: `read_json_zip_dev` / `convert_files(reader="auto")` /
`summarize_json_zip` / `json-summary`.

The expected value of every draw is float(v) of json.loads on the same text computed here, the reference's own
conversion (src/mcmc_ref/convert.py:78-102), and every comparison is bit for bit."""
from __future__ import annotations

import json
import random
import re
import struct
import zipfile
from decimal import Decimal, localcontext
import math
from pathlib import Path

import numpy as np
import pytest

from conftest import load_json

pytestmark = pytest.mark.gpu

CASES = load_json("json_zip_cases.json")
CHUNK = 16384            # MCR_JSON_CHUNK (include/mcmcref_hip.h): bytes of text per workgroup of the structural index
PARSE_BLOCK = 256        # MCR_JSON_PARSE_BLOCK: array elements per workgroup of the element parser
# the recorded documents inside the subset the device reader certifies; every other one is for the host reader
CERTIFIED = {"float_columns", "int_column", "mixed_column", "int_in_one_chain_float_in_other", "negative_zero_literals",
             "negative_zero_int_column", "int_at_2_53", "sorted_params_document_first_length", "longer_later_chain_is_cut",
             "extra_key_in_later_chain", "structural_characters_in_keys", "nonfinite_literals", "indented_crlf",
             "twenty_five_digit_tie"}


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    with _ffi.Context(0) as c:
        yield c


def same_bits(got: np.ndarray, exp: np.ndarray) -> bool:
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    if got.shape != exp.shape:
        return False
    nan = np.isnan(exp)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], exp.view(np.uint64)[~nan]))


def archive(tmp_path: Path, name: str, text: str | bytes) -> Path:
    p = tmp_path / f"{name}.json.zip"
    with zipfile.ZipFile(p, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=1) as zf:
        zf.writestr(f"{name}.json", text if isinstance(text, bytes) else text.encode("utf-8"))
    return p


def expected_from_text(text: str):
    """(params, [P][C][N] float(v), int_columns) by the reference's rules, straight from json.loads of the text."""
    payload = json.loads(text)
    params = sorted(payload[0])
    N = len(next(iter(payload[0].values())))
    exp = np.array([[[float(v) for v in ch[p][:N]] for ch in payload] for p in params], dtype=np.float64).reshape(len(params), len(payload), N)
    ints = [bool(N) and all(isinstance(v, int) for ch in payload for v in ch[p][:N]) for p in params]
    return params, exp, ints


def read_dev(ctx, path: Path):
    """(params, [P][C][N] downloaded, int_columns, phases) or (None, phases)."""
    from mcmc_ref_hip import convert
    ph: dict = {}
    got = convert.read_json_zip_dev(path, context=ctx, phases=ph)
    if got is None:
        return None, ph
    params, t, ints = got
    try:
        _, C_, N, P = t.targs[:4]
        flat = t.buf.download(np.float64, P * C_ * N) if P * C_ * N else np.empty(0)
        return (params, flat.reshape(P, C_, N), ints), ph
    finally:
        t.free()


def check_text(ctx, tmp_path: Path, name: str, text: str):
    """The device reader's names, shape, bits and int_columns equal json.loads of the text; returns the hard count."""
    got, ph = read_dev(ctx, archive(tmp_path, name, text))
    assert got is not None, ph
    params, exp, ints = expected_from_text(text)
    assert got[0] == params and got[1].shape == exp.shape and got[2] == ints, name
    assert same_bits(got[1], exp), name
    return ph["hard"]


# ---- documents as the writers write them -----------------------------------------------------------------------------

def token(rng: random.Random, fmt: str) -> str:
    v = rng.gauss(0.0, 1.0) * 10.0 ** rng.randint(-12, 12)
    if fmt == "int":
        return str(rng.randrange(-10 ** rng.randint(1, 15), 10 ** rng.randint(1, 15)))
    if fmt == "mixed":
        fmt = rng.choice(["repr", "%.17g", "%.6g", "int", "-0", "%.3e"])
        if fmt in ("int", "-0"):
            return "-0" if fmt == "-0" else token(rng, "int")
    return repr(v) if fmt == "repr" else fmt % v


SEPARATORS = {"compact": {"separators": (",", ":")}, "default": {}, "indent": {"indent": 2}, "crlf": {"indent": 2}}


def document(seed: int, C_: int, P: int, N: int, fmt: str = "repr", sep: str = "default", names=None, lengths=None) -> str:
    """json.dumps of C chains x P keys x N numbers with the number text of `fmt` (the tokens go through dumps as marked
    strings and lose their quotes afterwards).  lengths[c][k] overrides N for one array."""
    rng = random.Random(seed)
    names = names or [f"theta[{k + 1}]" for k in range(P)]
    payload = [{nm: ["@@" + token(rng, fmt) for _ in range(lengths[c][k] if lengths else N)] for k, nm in enumerate(names)}
               for c in range(C_)]
    text = re.sub(r'"@@([^"]*)"', r"\1", json.dumps(payload, **SEPARATORS[sep]))
    return text.replace("\n", "\r\n") if sep == "crlf" else text


@pytest.mark.parametrize("fmt", ["repr", "%.17g", "%.6g", "int", "mixed"])
@pytest.mark.parametrize("sep", sorted(SEPARATORS))
def test_writer_matrix_equals_json_loads_in_bits(ctx, tmp_path, sep, fmt):
    seed = 0
    for C_ in (1, 2, 5):
        for P in (1, 3):
            for N in (0, 1, 2, 63, 64, 65, PARSE_BLOCK - 1, PARSE_BLOCK, PARSE_BLOCK + 1, 1000):
                seed += 1
                hard = check_text(ctx, tmp_path, "m", document(seed, C_, P, N, fmt, sep))
                assert hard == 0


def test_int_columns_follow_the_literals(ctx, tmp_path):
    text = '[{"i": [1, -2, 0], "f": [1.0, 2, 3], "e": [1e0, 2, 3], "z": [-0, 0, 5]}, {"i": [4, 5, 6], "f": [4, 5, 6], "e": [4, 5, 6], "z": [1, 2, -0]}]'
    got, _ = read_dev(ctx, archive(tmp_path, "ints", text))
    assert got[0] == ["e", "f", "i", "z"] and got[2] == [False, False, True, True]
    check_text(ctx, tmp_path, "ints", text)


# ---- every boundary --------------------------------------------------------------------------------------------------

BOUNDARY_DOC = document(31, 2, 2, 180, "repr", "compact", names=["alpha", "theta[1,2]"])


def _features() -> dict[str, int]:
    """Offsets, in BOUNDARY_DOC, of the features slid across the edges: all in the second chain's second member."""
    key = BOUNDARY_DOC.rindex('"theta[1,2]"')
    opening = key + len('"theta[1,2]":')
    commas = [m.start() for m in re.finditer(",", BOUNDARY_DOC[opening:BOUNDARY_DOC.index("]", opening)])]
    comma = opening + commas[len(commas) // 2]
    return {"key_open_quote": key, "key_close_quote": key + len('"theta[1,2]"') - 1, "array_open": opening,
            "comma": comma, "array_close": BOUNDARY_DOC.index("]", opening), "number_middle": comma + 5}


FEATURES = _features()


@pytest.mark.parametrize("delta", [-2, -1, 0, 1, 2])
@pytest.mark.parametrize("edge", [CHUNK, 7 * 64 + CHUNK])            # a chunk edge; a thread edge inside the second chunk
@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_every_feature_at_every_offset_around_chunk_and_thread_edges(ctx, tmp_path, feature, edge, delta):
    at = FEATURES[feature]
    assert BOUNDARY_DOC[at] in {"key_open_quote": '"', "key_close_quote": '"', "array_open": "[", "comma": ",", "array_close": "]"}.get(
        feature, "0123456789.e-")
    pad = edge + delta - at
    assert 0 <= pad and at < CHUNK - 2
    text = " " * pad + BOUNDARY_DOC
    assert text[edge + delta] == BOUNDARY_DOC[at]
    assert check_text(ctx, tmp_path, "edge", text) == 0


def test_a_string_open_across_a_whole_chunk_and_a_document_ending_on_an_edge(ctx, tmp_path):
    long_key = "k[,]{:}" * 3000                                      # 21 000 bytes of structural characters inside one key
    text = '[{"%s": [1.5, 2.5], "b": [3, 4]}, {"b": [5, 6], "%s": [7.5, 8.5]}]' % (long_key, long_key)
    check_text(ctx, tmp_path, "longkey", text)
    base = '[{"a":[1.5,2,3e5]}]'
    for total in (63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK):
        check_text(ctx, tmp_path, "end", " " * (total - len(base)) + base)      # the closing bracket is the last byte
        check_text(ctx, tmp_path, "end", base + " " * (total - len(base)))


# ---- keys and the reference's rules -----------------------------------------------------------------------------------

def test_structural_characters_inside_keys(ctx, tmp_path):
    names = ["theta[1,2]", "a:b", "{x}", "],["]
    for sep in sorted(SEPARATORS):
        text = document(77, 3, 4, 70, "mixed", sep, names=names)
        got, _ = read_dev(ctx, archive(tmp_path, "keys", text))
        assert got[0] == sorted(names)
        check_text(ctx, tmp_path, "keys", text)


def test_reference_rules(ctx, tmp_path):
    # n_draws comes from the document-first key (zeta: 3), not the sorted-first (alpha: 5); longer arrays are cut
    text = document(3, 3, 2, 0, names=["zeta", "alpha"], lengths=[[3, 5], [4, 3], [3, 9]])
    got, _ = read_dev(ctx, archive(tmp_path, "first", text))
    assert got[0] == ["alpha", "zeta"] and got[1].shape == (2, 3, 3)
    check_text(ctx, tmp_path, "first", text)
    # extra keys in later chains are ignored, wherever they stand
    text = '[{"b": [1.5, 2.5], "a": [3.5, 4.5]}, {"extra": [9, 9, 9], "a": [5.5, 6.5], "more": [], "b": [7.5, 8.5, 9.5]}]'
    got, _ = read_dev(ctx, archive(tmp_path, "extra", text))
    assert got[0] == ["a", "b"] and got[1].tolist() == [[[3.5, 4.5], [5.5, 6.5]], [[1.5, 2.5], [7.5, 8.5]]]
    # -0 inside a float column is +0.0, -0.0 stays
    text = '[{"z": [-0, -0.0, 1.5, -0e0]}]'
    got, _ = read_dev(ctx, archive(tmp_path, "zero", text))
    assert [struct.pack("<d", v) for v in got[1][0, 0]] == [struct.pack("<d", v) for v in (0.0, -0.0, 1.5, -0.0)]
    assert got[2] == [False]
    check_text(ctx, tmp_path, "zero", text)
    # what lies behind the cut is still checked: a string there is for the host reader
    assert read_dev(ctx, archive(tmp_path, "tail", '[{"a": [1.5]}, {"a": [2.5, "x"]}]'))[0] is None
    assert read_dev(ctx, archive(tmp_path, "tail", '[{"a": [1.5]}, {"a": [2.5], "extra": [true]}]'))[0] is None
    check_text(ctx, tmp_path, "tail", '[{"a": [1.5]}, {"a": [2.5, 9007199254740993], "extra": [123456789012345678901234567890]}]')


# ---- hard tokens ----------------------------------------------------------------------------------------------------

def test_hard_tokens_are_counted_and_finished_exactly(ctx, tmp_path):
    rng = random.Random(8)
    ties = []
    with localcontext() as c:
        c.prec = 200
        while len(ties) < 37:
            x = math.ldexp(float(rng.randrange(1 << 52, 1 << 53)), rng.randint(38, 44) - 52)     # 2^41 <= x < 2^42: 13 + 12 digits
            s = format((Decimal(x) + Decimal(math.nextafter(x, math.inf))) / 2, "f")
            if len(s.replace(".", "")) == 25:
                ties.append(s)
    words = ["Infinity"] * 5 + ["-Infinity"] * 3 + ["NaN"] * 2
    plain = [repr(rng.gauss(0, 1)) for _ in range(600 - len(ties) - len(words))]
    tokens = ties + words + plain
    rng.shuffle(tokens)
    text = "[" + ", ".join('{"a": [%s], "b": [%s]}' % (", ".join(tokens[c * 150:(c + 1) * 150]), ", ".join(plain[:150])) for c in range(4)) + "]"
    assert check_text(ctx, tmp_path, "hard", text) == len(ties) + len(words)
    # more hard tokens than the list holds at first: the second pass
    many = "[" + ", ".join('{"a": [%s]}' % ", ".join(ties[(c + i) % len(ties)] for i in range(1500)) for c in range(4)) + "]"
    assert check_text(ctx, tmp_path, "hard", many) == 6000


# ---- fallback ---------------------------------------------------------------------------------------------------------

def results_equal(a, b) -> bool:
    import pyarrow.parquet as pq
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b) and str(a) == str(b)
    ta, tb = pq.read_table(a.draws_path), pq.read_table(b.draws_path)
    same_meta = json.dumps(a.meta, sort_keys=True) == json.dumps(b.meta, sort_keys=True)      # as text: a NaN diagnostic equals itself
    return same_meta and ta.schema.equals(tb.schema) and ta.equals(tb) and a.meta_path.read_text() == b.meta_path.read_text()


def convert_both(ctx, tmp_path: Path, path: Path, force: bool):
    from mcmc_ref_hip import convert
    out = []
    for reader in ("auto", "host"):
        d = tmp_path / f"out_{reader}"
        d.mkdir(exist_ok=True)
        try:
            out.append(convert.convert_files([(path, "model")], d, d, force=force, context=ctx, reader=reader)[0])
        except Exception as exc:  # noqa: BLE001 - what ends the batch on one route must end it on the other
            out.append(exc)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_documents_take_the_right_route_and_both_routes_agree(ctx, tmp_path, name):
    path = archive(tmp_path, name, CASES[name]["text"])
    got, ph = read_dev(ctx, path)
    assert (got is not None) == (name in CERTIFIED), ph
    if got is None:
        assert ph["fallback"]
    else:
        rec = CASES[name]
        assert ["chain", "draw"] + got[0] == rec["columns"]
        assert [("int64" if i else "double") for i in got[2]] == rec["types"][2:]
    auto, host = convert_both(ctx, tmp_path, path, force=True)
    assert results_equal(auto, host), (auto, host)
    if "error" in CASES[name] and name not in ("member_is_nested", "int_beyond_2_53_with_floats"):   # (there the host
        # reader has an answer of its own: test_json_cpu.py)
        assert type(host).__name__ == CASES[name]["error"]["type"] and str(host) == CASES[name]["error"]["message"]


@pytest.mark.parametrize("text", [
    b'\xef\xbb\xbf[{"a": [1.5]}]',                    # a byte-order mark
    b' x[{"a": [1.5]}]', b'', b'   ', b'[', b'[{', b'[{"a"', b'[{"a":', b'[{"a":[', b'[{"a":[1.5', b'[{"a":[1.5]', b'[{"a":[1.5]}',
    b'[{"a": [1.5]}] x', b'[{"a": [1.5]}, ]', b'[{"a": [1.5],}]', b'[{"a": [1.5] "b": [2.5]}]', b'[{"a" [1.5]}]', b'[{a: [1.5]}]',
    b'[{"a": [1.5]} {"a": [2.5]}]', b'[{"a": [1.5]},, {"a": [2.5]}]', b'[{"a": [1.5,, 2.5]}]', b'[{"a": [,]}]', b'[{"a": [1.5 2.5]}]',
    b'[{"a": [1.5}]', b'[{"a": [1.5]]', b'[{"a": {"b": [1.5]}}]', b'[{"a": [{"b": 1}]}]', b'[{"a\tb": [1.5]}]', b'[{"a": [1.5], "a": [2.5]}]',
    b'[{"a": "[1.5]"}]', b'[{"a": [1.5]}, 7]', b'[{"a": [1.5]}, {"a": [2.5]]', b'[{"\xff\xfe": [1.5]}]', b'[{"a": [1.5\x00]}]',
    b'[{"a": ["x]}]', b'[{"a": [1.5], "b": ["]}, {"a": [2.5], "b": ["]}]', b'[{"a"": [1.5]}]', b'[{"a": [0x10]}]', b'[{"a": [1.5]}]\x00',
    b'[{"draw": [1.5]}]', b'[{"chain": [1.5], "a": [2.5]}]', b'{"a": [1.5]}', b'[[1.5]]', b'[]', b'[{}]', b'[{"a": []}, {}]',
])
def test_documents_outside_the_subset_go_to_the_host_reader_and_both_routes_agree(ctx, tmp_path, text):
    path = archive(tmp_path, "bad", text)
    got, ph = read_dev(ctx, path)
    assert got is None and ph["fallback"]
    auto, host = convert_both(ctx, tmp_path, path, force=True)
    assert results_equal(auto, host), (auto, host)


def test_a_file_that_is_no_archive_and_an_empty_archive(ctx, tmp_path):
    p = tmp_path / "broken.json.zip"
    p.write_bytes(b"not a zip file")
    assert read_dev(ctx, p)[0] is None
    auto, host = convert_both(ctx, tmp_path, p, force=True)
    assert isinstance(host, Exception) and results_equal(auto, host)
    with zipfile.ZipFile(tmp_path / "empty.json.zip", "w"):
        pass
    auto, host = convert_both(ctx, tmp_path, tmp_path / "empty.json.zip", force=True)
    assert isinstance(host, IndexError) and results_equal(auto, host)


# ---- through the public interface -----------------------------------------------------------------------------------

def iid_document(seed: int, C_: int, N: int, P: int, int_column: bool = False, shift: float = 0.0) -> str:
    rng = np.random.default_rng(seed)
    payload = []
    for c in range(C_):
        ch = {f"beta[{p + 1}]": (rng.standard_normal(N) + shift * c).tolist() for p in range(P)}
        if int_column:
            ch["count"] = rng.integers(0, 50, N).tolist()
        payload.append(ch)
    return json.dumps(payload)


def test_convert_files_writes_the_same_files_on_both_routes(ctx, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from mcmc_ref_hip import convert
    # well-formed, 4 x 250 x 3 (the draw-count check fails at this size: force writes the files and records the checks)
    auto, host = convert_both(ctx, tmp_path, archive(tmp_path, "ok", iid_document(1, 4, 250, 3)), force=True)
    assert isinstance(auto, convert.ConvertResult) and results_equal(auto, host)
    assert auto.meta["n_chains"] == 4 and auto.meta["n_draws_per_chain"] == 250 and auto.meta["checks"]["rhat_below_1_01"]
    # with an all-integer column: int64 in the written file on both routes
    auto, host = convert_both(ctx, tmp_path, archive(tmp_path, "ints", iid_document(2, 4, 250, 3, int_column=True)), force=True)
    assert isinstance(auto, convert.ConvertResult) and results_equal(auto, host)
    schema = pq.read_table(auto.draws_path).schema
    assert schema.field("count").type == pa.int64() and schema.field("beta[1]").type == pa.float64()
    # chains that do not mix fail the quality gate with the same ValueError
    auto, host = convert_both(ctx, tmp_path, archive(tmp_path, "gate", iid_document(3, 4, 250, 3, shift=3.0)), force=False)
    assert isinstance(host, ValueError) and "rhat_below_1_01" in str(host) and results_equal(auto, host)
    # 4 x 2500 passes the gate: no force
    auto, host = convert_both(ctx, tmp_path, archive(tmp_path, "full", iid_document(4, 4, 2500, 2)), force=False)
    assert isinstance(auto, convert.ConvertResult) and results_equal(auto, host) and all(auto.meta["checks"].values())
    # too few chains: the same message before any statistics
    auto, host = convert_both(ctx, tmp_path, archive(tmp_path, "two", iid_document(5, 2, 250, 1)), force=False)
    assert isinstance(host, ValueError) and "at least 4 chains" in str(host) and results_equal(auto, host)
    # several inputs of one call, either route per input, in order
    jobs = [(archive(tmp_path, f"j{i}", t), f"j{i}") for i, t in enumerate(
        [iid_document(6, 4, 250, 2), '[{"a": "x"}]', iid_document(7, 4, 250, 1, int_column=True),
         iid_document(8, 4, 250, 2).replace("beta[1]", "beta\\u005b1]")])]
    outs = []
    for reader in ("auto", "host"):
        d = tmp_path / f"many_{reader}"
        d.mkdir()
        outs.append(convert.convert_files(jobs, d, d, force=True, context=ctx, reader=reader))
    assert all(results_equal(a, h) for a, h in zip(*outs))
    assert [isinstance(outs[0][i], convert.ConvertResult) for i in (0, 2, 3)] == [True, True, True]
    assert outs[0][3].meta["parameters"] == ["beta[1]", "beta[2]"]
    with pytest.raises(ValueError, match="reader"):
        convert.convert_files(jobs, tmp_path, tmp_path, reader="device")


def test_convert_file_keeps_its_contract(tmp_path):
    import pyarrow.parquet as pq
    from mcmc_ref_hip import convert
    text = iid_document(9, 4, 2500, 2, int_column=True)
    res = convert.convert_file(archive(tmp_path, "m", text), "m", tmp_path, tmp_path)
    params, exp, ints = expected_from_text(text)
    table = pq.read_table(res.draws_path)
    assert table.column_names == ["chain", "draw"] + params and res.meta["parameters"] == params
    for k, p in enumerate(params):
        assert same_bits(table.column(p).to_numpy().astype(np.float64), exp[k].reshape(-1))
        assert str(table.schema.field(p).type) == ("int64" if ints[k] else "double")


def test_summarize_json_zip_equals_the_host_route_exactly_and_the_cli_prints_it(ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import _ffi, cli, convert
    path = archive(tmp_path, "s", iid_document(11, 4, 250, 3, int_column=True))
    got = convert.summarize_json_zip(path, context=ctx)
    table = convert._read_json_zip(path)
    params = [c for c in table.column_names if c not in {"chain", "draw"}]
    x, counts = convert.table_to_tensor(table, params)
    qs = (0.05, 0.5, 0.95)
    r = ctx.summarize(x.reshape(len(params), len(counts), int(counts[0])), "pcn", quantiles=qs)
    exp = dict(zip(params, _ffi.entries(r, list(qs), True)))
    assert list(got) == list(exp)
    for n in params:
        assert list(got[n]) == list(exp[n])
        for k in exp[n]:
            assert struct.pack("<d", got[n][k]) == struct.pack("<d", exp[n][k]), (n, k)
    plain = convert.summarize_json_zip(path, diagnostics=False, quantiles=(0.5,), context=ctx)
    assert list(plain[params[0]]) == ["mean", "std", "q50"] and plain[params[0]]["mean"] == exp[params[0]]["mean"]
    # a document for the host reader gives the same numbers; one it refuses raises what it raises
    escaped = archive(tmp_path, "esc", iid_document(11, 4, 250, 3, int_column=True).replace("beta[1]", "beta\\u005b1]"))
    assert convert.summarize_json_zip(escaped, context=ctx) == got
    with pytest.raises(KeyError):
        convert.summarize_json_zip(archive(tmp_path, "k", CASES["chain_missing_a_parameter"]["text"]), context=ctx)
    r = CliRunner().invoke(cli.main, ["json-summary", str(path), "--format", "json"])
    assert r.exit_code == 0, r.output
    assert json.loads(r.output) == {n: exp[n] for n in params}
    r = CliRunner().invoke(cli.main, ["json-summary", str(path)])
    assert r.exit_code == 0 and r.output.splitlines()[0].split() == ["param"] + sorted(exp[params[0]])
    assert r.output.splitlines()[1].split()[0] == params[0]
    r = CliRunner().invoke(cli.main, ["json-summary", str(path), str(escaped), "--format", "json"])
    assert r.exit_code == 0 and json.loads(r.output) == {str(path): exp, str(escaped): exp}
    r = CliRunner().invoke(cli.main, ["json-summary", str(archive(tmp_path, "one", iid_document(12, 1, 50, 1)))])
    assert r.exit_code != 0 and "chain" in r.output


# ---- one multi-megabyte document ----------------------------------------------------------------------------------

def test_a_multi_megabyte_document_equals_the_host_route_in_bits(ctx, tmp_path):
    from mcmc_ref_hip import convert
    rng = np.random.default_rng(2024)
    payload = [{f"theta[{p + 1},{p % 3}]": (rng.standard_normal(10_000) * 10.0 ** (p - 4)).tolist() for p in range(8)} for _ in range(4)]
    text = json.dumps(payload)
    assert len(text) > 200 * CHUNK
    path = archive(tmp_path, "big", text)
    got, ph = read_dev(ctx, path)
    assert got is not None and ph["hard"] == 0
    table = convert._read_json_zip(path)
    params = [c for c in table.column_names if c not in {"chain", "draw"}]
    x, counts = convert.table_to_tensor(table, params)
    assert got[0] == params and got[2] == [False] * 8 and counts.tolist() == [10_000] * 4
    assert same_bits(got[1].reshape(8, -1), x)
