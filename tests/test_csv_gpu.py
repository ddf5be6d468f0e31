"""CmdStan chain CSVs parsed on the GPU: `chains_tensor_dev` / `summarize_chains` / `cmdstan-summary`.

The expected value of every field is float(field) computed here, the reference's own conversion
(src/mcmc_ref/cmdstan_generate.py:28), and every comparison is bit for bit."""
from __future__ import annotations

import ctypes
import json
import math
import random
import struct
from decimal import Decimal, localcontext
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, load_json

pytestmark = pytest.mark.gpu

CASES = load_json("cmdstan_csv_cases.json")
CHUNK = 16384            # MCR_CSV_CHUNK (include/mcmcref_hip.h): bytes of text per workgroup of the line index
INTERNAL = ["lp__", "accept_stat__", "stepsize__", "treedepth__", "n_leapfrog__", "divergent__", "energy__"]


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


def expected_from_text(text: str):
    """(raw header, [rows][header fields] of float(field)) by the reference's rules, straight from the text."""
    lines = [ln for ln in text.replace("\r\n", "\n").split("\n") if not ln.startswith("#")]
    header = [h.strip() for h in lines[0].split(",")]
    rows = [[float(v) for v in ln.split(",")] for ln in lines[1:] if ln.strip()]
    return header, rows


def decode(ctx, paths, phases=None):
    from mcmc_ref_hip import cmdstan_generate as cs
    ph = {} if phases is None else phases
    names, t = cs.chains_tensor_dev(paths, context=ctx, phases=ph)
    try:
        _, C_, N, P = t.targs[:4]
        flat = t.buf.download(np.float64, P * C_ * N) if P * C_ * N else np.empty(0)
        return names, flat.reshape(P, C_, N), ph["hard"]
    finally:
        t.free()


def check_files(ctx, paths, texts):
    """Every selected field of every file equals float(field); returns the hard count."""
    from mcmc_ref_hip import cmdstan_generate as cs
    names, got, hard = decode(ctx, paths)
    per = [expected_from_text(t) for t in texts]
    N = min(len(rows) for _, rows in per)
    assert got.shape == (len(names), len(paths), N)
    for c, (header, rows) in enumerate(per):
        norm = [cs._normalize_cmdstan_param_name(h) for h in header]
        exp = np.array(rows[:N], dtype=np.float64).reshape(N, len(header))
        for k, name in enumerate(names):
            assert same_bits(got[k, c], exp[:, norm.index(name)]), (paths[c], name)
    return names, hard


def number(rng: random.Random, fmt: str) -> str:
    v = rng.gauss(0.0, 1.0) * 10.0 ** rng.randint(-12, 12)
    return repr(v) if fmt == "repr" else fmt % v


def chain_text(seed: int, N: int, P: int, fmt: str = "%.17g", eol: str = "\n", final_newline: bool = True,
               comments: bool = True, lead_pad: int = 0) -> str:
    rng = random.Random(seed)
    header = INTERNAL[:3] + [f"theta.{i + 1}" for i in range(P)] + INTERNAL[3:]
    lines = ["# model = demo", "#   seed = %d" % seed] if comments else []
    if lead_pad:
        lines.append("#" + "p" * (lead_pad - 1 - len(eol)))
    lines.append(",".join(header))
    if comments:
        lines += ["# Adaptation terminated", "# Step size = 0.35"]
    for r in range(N):
        lines.append(",".join(number(rng, fmt) for _ in header))
        if comments and rng.random() < 0.2:
            lines.append("# between the draws, with, commas")
    if comments:
        lines += ["# ", "#  Elapsed Time: 0.01 seconds"]
    return eol.join(lines) + (eol if final_newline else "")


def write(tmp_path: Path, name: str, text: str) -> Path:
    p = tmp_path / name
    p.write_bytes(text.encode())
    return p


# ---- golden files and recorded reference cases -----------------------------------------------------------------------

@pytest.mark.parametrize("files", [["chain_1.csv", "chain_2.csv"], ["chain_1.csv", "chain_2.csv", "chain_2.csv", "chain_1.csv"]])
def test_golden_chain_files_equal_the_host_reader_in_bits(ctx, files):
    from mcmc_ref_hip import cmdstan_generate as cs
    paths = [GOLDEN / "cmdstan" / f for f in files]
    names_h, x = cs.chains_tensor(paths)
    names_d, got, hard = decode(ctx, paths)
    assert names_d == names_h
    assert same_bits(got, x)
    assert hard == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_reference_cases(ctx, tmp_path, name):
    case = CASES[name]
    p = write(tmp_path, "chain.csv", case["text"])
    names, got, _ = decode(ctx, [p])
    assert got.shape[1:] == (1, case["rows"])
    if case["rows"]:
        assert names == case["names"]
        for k, n in enumerate(names):
            assert same_bits(got[k, 0], np.array([float.fromhex(h) for h in case["columns"][n]])), n


# ---- writer matrix ---------------------------------------------------------------------------------------------------

FORMATS = [(fmt, eol, fin) for fmt in ("%.6g", "%.17g", "%.25e") for eol in ("\n", "\r\n") for fin in (True, False)]


@pytest.mark.parametrize("fmt,eol,final_newline", FORMATS)
def test_formats_line_ends_and_comments_everywhere(ctx, tmp_path, fmt, eol, final_newline):
    texts = [chain_text(100 + c, 65, 7, fmt, eol, final_newline) for c in range(2)]
    paths = [write(tmp_path, f"c{c}.csv", t) for c, t in enumerate(texts)]
    _, hard = check_files(ctx, paths, texts)
    assert hard == 0


@pytest.mark.parametrize("P", [1, 7, 64, 65, 1000, 10000])
def test_column_counts(ctx, tmp_path, P):
    texts = [chain_text(200 + c, 5, P, "repr") for c in range(2)]
    paths = [write(tmp_path, f"c{c}.csv", t) for c, t in enumerate(texts)]
    names, hard = check_files(ctx, paths, texts)
    assert len(names) == P and hard == 0


@pytest.mark.parametrize("N", [0, 1, 2, 63, 64, 65, 10000])
def test_row_counts(ctx, tmp_path, N):
    texts = [chain_text(300 + c, N, 3, "%.17g", comments=N < 1000) for c in range(2)]
    paths = [write(tmp_path, f"c{c}.csv", t) for c, t in enumerate(texts)]
    check_files(ctx, paths, texts)


@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_file_size_at_the_index_chunk(ctx, tmp_path, delta, final_newline):
    base = chain_text(400, 60, 7, "%.17g", final_newline=final_newline, comments=False)
    pad = 2 * CHUNK + delta - len(base)
    assert pad > 8
    text = chain_text(400, 60, 7, "%.17g", final_newline=final_newline, comments=False, lead_pad=pad)
    assert len(text.encode()) == 2 * CHUNK + delta
    check_files(ctx, [write(tmp_path, "a.csv", text), write(tmp_path, "b.csv", base)], [text, base])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_row_start_at_the_index_chunk(ctx, tmp_path, delta):
    base = chain_text(500, 200, 7, "%.17g", comments=False)
    lines = base.split("\n")
    at = len("\n".join(lines[:101])) + 1          # offset of data row 100
    text = chain_text(500, 200, 7, "%.17g", comments=False, lead_pad=3 * CHUNK + delta - at)
    assert text.encode()[3 * CHUNK + delta - 1:3 * CHUNK + delta] == b"\n" and text.split("\n")[102] == lines[101]
    check_files(ctx, [write(tmp_path, "a.csv", text)], [text])


def test_chains_of_unequal_length_are_cut_to_the_shortest(ctx, tmp_path):
    texts = [chain_text(600 + c, n, 5) for c, n in enumerate((70, 33, 64, 120))]
    paths = [write(tmp_path, f"c{c}.csv", t) for c, t in enumerate(texts)]
    from mcmc_ref_hip import cmdstan_generate as cs
    names, got, _ = decode(ctx, paths)
    assert got.shape == (5, 4, 33)
    names_h, x = cs.chains_tensor(paths)
    assert names == names_h and same_bits(got, x)
    check_files(ctx, paths, texts)


def test_column_subset_in_another_order_and_headers_that_differ(ctx, tmp_path):
    rng = random.Random(7)
    cols_a, cols_b = ["a", "lp__", "b.1", "b.2", "c"], ["c", "b.2", "a", "energy__", "b.1"]
    rows = [[number(rng, "%.17g") for _ in range(5)] for _ in range(40)]
    ta = "\n".join([",".join(cols_a)] + [",".join(r) for r in rows]) + "\n"
    tb = "\n".join([",".join(cols_b)] + [",".join(r) for r in rows]) + "\n"
    pa, pb = write(tmp_path, "a.csv", ta), write(tmp_path, "b.csv", tb)
    check_files(ctx, [pa, pb], [ta, tb])          # names in the first file's order, the second file's columns permuted

    def select(_f, header):                       # two parameters, against header order
        return ["c", "a"], [header.index("c"), header.index("a")]
    names, t, hard = ctx.csv_decode([str(pa), str(pb)], select)
    try:
        got = t.buf.download(np.float64, 2 * 2 * 40).reshape(2, 2, 40)
    finally:
        t.free()
    exp = np.array([[float(v) for v in r] for r in rows])
    assert names == ["c", "a"] and hard == 0
    assert same_bits(got[0, 0], exp[:, 4]) and same_bits(got[1, 0], exp[:, 0])
    assert same_bits(got[0, 1], exp[:, 0]) and same_bits(got[1, 1], exp[:, 2])


def test_caller_images_into_a_cnp_tensor_through_the_c_abi(ctx):
    """mcr_csv_open on images the caller holds, one mcr_csv_stage + mcr_csv_decode for both, [C][N][P] strides."""
    from mcmc_ref_hip import _ffi
    L = ctx.lib
    texts = [chain_text(900 + c, 70 + c, 5, "%.17g", eol) for c, eol in enumerate(("\n", "\r\n"))]
    raws = [t.encode() for t in texts]
    bufs = [ctypes.create_string_buffer(r, len(r)) for r in raws]
    hs = (ctypes.c_void_p * 2)()
    for i, (b, r) in enumerate(zip(bufs, raws)):
        h = ctypes.c_void_p()
        assert L.mcr_csv_open(None, b, len(r), ctypes.byref(h)) == 0
        hs[i] = h
    try:
        rows = np.zeros(2, dtype=np.int64)
        ctx._check(L.mcr_csv_stage(ctx.handle, hs, 2, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        assert rows.tolist() == [70, 71]
        header = [L.mcr_csv_column_name(hs[0], c).decode() for c in range(L.mcr_csv_num_columns(hs[0]))]
        want = [header.index(n) for n in ("theta.5", "lp__", "theta.1")]
        cols = np.array([want, want], dtype=np.intc)
        N, P = 70, 3
        buf = _ffi.DeviceBuffer(ctx, 2 * N * P * 8)
        try:
            hard = ctypes.c_int64(-1)
            for _ in range(2):                     # a staged set can be decoded again
                ctx._check(L.mcr_csv_decode(ctx.handle, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), P, N, buf.ptr,
                                            N * P, P, 1, ctypes.byref(hard)))
            got = buf.download(np.float64, 2 * N * P).reshape(2, N, P)
        finally:
            buf.free()
        assert hard.value == 0
        for c, t in enumerate(texts):
            _, exp = expected_from_text(t)
            assert same_bits(got[c], np.array(exp)[:N][:, want])
    finally:
        for h in hs:
            L.mcr_csv_close(h)


# ---- hard fields ------------------------------------------------------------------------------------------------------

def halfway(rng: random.Random) -> str:
    with localcontext() as c:
        c.prec = 1200
        x = abs(struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64) & ~(1 << 63)))[0])
        while x != x or math.isinf(x) or math.isinf(math.nextafter(x, math.inf)):
            x = rng.random()
        return format((Decimal(x) + Decimal(math.nextafter(x, math.inf))) / 2, "e")


def test_hard_fields_are_finished_on_the_host(ctx, tmp_path):
    from mcmc_ref_hip import _ffi, cmdstan_generate as cs
    rng = random.Random(11)
    special = ["inf", "nan", "-inf", "NaN", "Infinity", "-Infinity", "+nan"]
    rows = []
    for r in range(300):
        row = [number(rng, "%.17g") for _ in range(6)]
        if r % 3 == 0:
            row[rng.randrange(6)] = halfway(rng)
        if r % 7 == 0:
            row[rng.randrange(6)] = rng.choice(special)
        rows.append(row)
    header = ["lp__", "a", "b", "c.1", "c.2", "d"]
    texts = ["\n".join([",".join(header)] + [",".join(r) for r in (rows if c % 2 == 0 else rows[::-1])]) + "\n" for c in range(4)]
    paths = [write(tmp_path, f"c{c}.csv", t) for c, t in enumerate(texts)]
    L, predicted = ctx.lib, 0
    for t in texts:
        for ln in t.split("\n")[1:-1]:
            for field in ln.split(",")[1:]:           # lp__ is not selected
                out = ctypes.c_double()
                rc = L.mcr_parse_double(field.encode(), len(field), ctypes.byref(out))
                assert rc in (0, 1)
                predicted += rc
    _, hard = check_files(ctx, paths, texts)
    assert hard == predicted and hard > 200
    names, t = cs.chains_tensor_dev(paths, context=ctx)
    try:
        with pytest.raises(_ffi.McrError) as ei:
            ctx.summarize(t)
        assert ei.value.code == _ffi.MCR_ENONFINITE
    finally:
        t.free()
    with pytest.raises(ValueError):
        cs.summarize_chains(paths, context=ctx)


def test_a_hard_list_that_overflows_is_parsed_again(ctx, tmp_path):
    rng = random.Random(13)
    text = "x,y\n" + "".join(f"{halfway(rng)},{halfway(rng)}\n" for _ in range(3000))
    p = write(tmp_path, "h.csv", text)
    predicted = 0                                  # (a midpoint of at most 19 digits is decided)
    for field in text.replace("\n", ",").split(",")[2:-1]:
        predicted += ctx.lib.mcr_parse_double(field.encode(), len(field), ctypes.byref(ctypes.c_double()))
    _, hard = check_files(ctx, [p], [text])
    assert hard == predicted and hard > 4096       # more than the list's first capacity


# ---- errors -----------------------------------------------------------------------------------------------------------

def _bad(kind: str) -> tuple[str, int]:
    lines = chain_text(700, 20, 4, comments=False).split("\n")
    row = 12
    f = lines[1 + row].split(",")
    if kind == "short":
        f = f[:-1]
    elif kind == "long":
        f = f + ["1.0"]
    elif kind == "text":
        f[4] = "abc"
    elif kind == "empty":
        f[4] = ""
    elif kind == "quoted":
        f[4] = '"1.5"'
    lines[1 + row] = ",".join(f)
    return "\n".join(lines), row


@pytest.mark.parametrize("kind", ["short", "long", "text", "empty", "quoted"])
def test_bad_rows_raise_value_error_naming_file_and_row(ctx, tmp_path, kind):
    from mcmc_ref_hip import cmdstan_generate as cs
    good = chain_text(701, 20, 4)
    text, row = _bad(kind)
    pg, pb = write(tmp_path, "good.csv", good), write(tmp_path, f"bad_{kind}.csv", text)
    with pytest.raises(ValueError) as ei:
        cs.chains_tensor_dev([pg, pb], context=ctx)
    msg = str(ei.value)
    assert str(pb) in msg and f"row {row}" in msg, msg
    if kind == "quoted":
        assert "quoted fields are not supported" in msg
    if kind == "text":
        assert "abc" in msg
    if kind in ("short", "long"):
        assert f"has {10 if kind == 'short' else 12} fields, header has 11" in msg
    check_files(ctx, [pg], [good])                 # the context is still good


def test_mismatched_parameter_sets_raise_like_the_host_reader(ctx, tmp_path):
    from mcmc_ref_hip import cmdstan_generate as cs
    pa = write(tmp_path, "a.csv", "lp__,a,b\n1,2,3\n")
    pb = write(tmp_path, "b.csv", "lp__,a,c\n1,2,3\n")
    for fn in (cs.chains_tensor, lambda p: cs.chains_tensor_dev(p, context=ctx)):
        with pytest.raises(ValueError, match="chain 1 parameter keys mismatch"):
            fn([pa, pb])
    with pytest.raises(ValueError, match="no chain draws provided"):
        cs.chains_tensor_dev([], context=ctx)
    pc = write(tmp_path, "c.csv", "# nothing\n")
    with pytest.raises(ValueError, match="chain draws contain no parameters"):
        cs.chains_tensor_dev([pc], context=ctx)
    pd = write(tmp_path, "d.csv", "theta.1,theta[1]\n1,2\n")
    with pytest.raises(ValueError, match="both normalise to"):
        cs.chains_tensor_dev([pd], context=ctx)
    with pytest.raises(ValueError, match="cannot open"):
        cs.chains_tensor_dev([tmp_path / "missing.csv"], context=ctx)
    good = chain_text(702, 9, 2)
    check_files(ctx, [write(tmp_path, "g.csv", good)], [good])


# ---- end to end -------------------------------------------------------------------------------------------------------

def test_summarize_chains_equals_the_host_route_exactly_and_the_cli_prints_it(ctx, tmp_path):
    from click.testing import CliRunner
    from mcmc_ref_hip import _ffi, cli, cmdstan_generate as cs
    texts = [chain_text(800 + c, 250, 6, "repr") for c in range(4)]
    paths = [write(tmp_path, f"chain_{c}.csv", t) for c, t in enumerate(texts)]
    got = cs.summarize_chains(paths, context=ctx)
    names, x = cs.chains_tensor(paths)
    qs = (0.05, 0.5, 0.95)
    exp = dict(zip(names, _ffi.entries(ctx.summarize(x, "pcn", quantiles=qs), list(qs), True)))
    assert list(got) == list(exp)
    for n in names:
        assert list(got[n]) == list(exp[n])
        for k in exp[n]:
            assert struct.pack("<d", got[n][k]) == struct.pack("<d", exp[n][k]), (n, k)
    plain = cs.summarize_chains(paths, diagnostics=False, quantiles=(0.5,), context=ctx)
    assert list(plain[names[0]]) == ["mean", "std", "q50"] and plain[names[0]]["mean"] == exp[names[0]]["mean"]
    r = CliRunner().invoke(cli.main, ["cmdstan-summary", *map(str, paths), "--format", "json"])
    assert r.exit_code == 0, r.output
    assert json.loads(r.output) == {n: exp[n] for n in names}
    r = CliRunner().invoke(cli.main, ["cmdstan-summary", *map(str, paths)])
    assert r.exit_code == 0 and r.output.splitlines()[0].split() == ["param"] + sorted(exp[names[0]])
    assert r.output.splitlines()[1].split()[0] == names[0]
    r = CliRunner().invoke(cli.main, ["cmdstan-summary", str(paths[0]), "--format", "csv"])
    assert r.exit_code != 0 and "chain" in r.output
