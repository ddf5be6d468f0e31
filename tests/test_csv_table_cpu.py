"""The table CSV reader's host side, without a GPU: the field routine the kernel runs
(`mcr_parse_csv_number` compiles the same `__host__ __device__` text) against `pyarrow.csv.read_csv` in bits and in
column type, the list of texts it hands back, and the header reader `mcr_csv_open_table`."""
from __future__ import annotations

import ctypes
import importlib.util
import io
import math
import random
import struct
from decimal import Decimal, localcontext

import numpy as np
import pytest

from conftest import ROOT

EINVAL, EFALLBACK = -1, -10
T_BOM, T_DUP, T_EMPTY, T_QUOTE, T_CR, T_NO_HEADER = 1, 2, 4, 8, 16, 32     # MCR_CSV_T_* (include/mcmcref_hip.h)


@pytest.fixture(scope="module")
def L():
    spec = importlib.util.spec_from_file_location("mcr_build", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from mcmc_ref_hip import _ffi
    return _ffi.load_library()


def parse(L, s: str):
    b = s.encode()
    out, is_int = ctypes.c_double(math.nan), ctypes.c_int(-1)
    rc = L.mcr_parse_csv_number(b, len(b), ctypes.byref(out), ctypes.byref(is_int))
    return rc, out.value, is_int.value


def _strings(n_each: int, seed: int) -> list[str]:
    """What writers print: repr, %.6g, %.17g and %.25e of finite doubles of every binade (and of ordinary magnitudes),
    and integer literals up to +-2^53."""
    rng = random.Random(seed)
    out = []
    for k in range(n_each):
        if k % 2:
            x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
            if not math.isfinite(x):
                x = rng.uniform(-1, 1)
        else:
            x = rng.gauss(0.0, 1.0) * 10.0 ** rng.randint(-6, 6)
        out += [repr(x), "%.6g" % x, "%.17g" % x, "%.25e" % x]
        out.append(str(rng.randint(-(2 ** rng.randint(1, 53)), 2 ** rng.randint(1, 53))))
    with localcontext() as lc:                               # exact midpoints of neighbouring doubles: digits past the 19th decide
        lc.prec = 1200
        for _ in range(200):
            x = abs(rng.gauss(0.0, 1.0)) * 10.0 ** rng.randint(-8, 8) or 1.0
            mid = (Decimal(x) + Decimal(math.nextafter(x, math.inf))) / 2
            out += [format(mid, "f"), format(mid, "f") + "1", "-" + format(mid, "e")]
    return out + ["0", "-0", "9007199254740992", "-9007199254740992", "0.0", "-0.0", "0e0", "-0e-5", "1e400", "-1e400",
                  "1e-400", "4.9e-324", "2.4703282292062328e-324", "1.7976931348623157e308", "1.7976931348623159e308"]


def test_the_field_routine_equals_pyarrow_in_bits_and_in_column_type(L):
    import pyarrow as pa
    import pyarrow.csv as pacsv
    strings = _strings(41_000, 20260117)
    assert len(strings) >= 200_000
    results = [parse(L, s) for s in strings]
    # %.17g prints doubles in [2^53, 10^17) as 17-digit integer literals: above 2^53, so they go back like any such literal
    big = [i for i, s in enumerate(strings) if s.lstrip("-").isdigit() and abs(int(s)) > 2 ** 53]
    assert len(big) < len(strings) // 500
    for i in big:
        assert results[i][0] == EFALLBACK and results[i][2] == 1, strings[i]
    big_set = set(big)
    keep = [i for i in range(len(strings)) if i not in big_set]
    assert all(results[i][0] in (0, 1) for i in keep), [strings[i] for i in keep if results[i][0] not in (0, 1)][:5]
    n_hard = sum(results[i][0] == 1 for i in keep)
    print(f"{len(keep)} strings, {n_hard} hard")
    assert n_hard >= 200                                     # the midpoints reach the host finisher

    # values: the column read as double
    doc = ("a\n" + "\n".join(strings[i] for i in keep) + "\n").encode()
    want = pacsv.read_csv(io.BytesIO(doc), convert_options=pacsv.ConvertOptions(column_types={"a": pa.float64()}))
    want = want.column("a").to_numpy().view(np.uint64)
    got = np.array([results[i][1] for i in keep], dtype=np.float64).view(np.uint64)
    bad = np.flatnonzero(want != got)
    assert bad.size == 0, [(strings[keep[j]], hex(want[j]), hex(got[j])) for j in bad[:5]]

    # is_int = 1: pyarrow types a column of exactly these literals int64, and the cast doubles are its integers
    ints = [i for i in keep if results[i][2] == 1]
    table = pacsv.read_csv(io.BytesIO(("a\n" + "\n".join(strings[i] for i in ints) + "\n").encode()))
    assert table.schema.field("a").type == pa.int64() and len(ints) > 40_000
    assert np.array_equal(table.column("a").to_numpy(), np.array([results[i][1] for i in ints]).astype(np.int64))
    # is_int = 0: each such literal alone makes its column double (a sample, one document per literal, and every format)
    floats = [i for i in keep if results[i][2] == 0]
    rng = random.Random(5)
    for i in rng.sample(floats, 200):
        t = pacsv.read_csv(io.BytesIO(f"a\n{strings[i]}\n".encode()))
        assert t.schema.field("a").type == pa.float64(), strings[i]
    assert len(ints) + len(floats) == len(keep)

    rc, v, is_int = parse(L, "-0")
    assert (rc, is_int) == (0, 1) and struct.pack("<d", v) == struct.pack("<d", -0.0)
    assert parse(L, "9007199254740992") == (0, 2.0 ** 53, 1) and parse(L, "-9007199254740992") == (0, -(2.0 ** 53), 1)


def test_the_csv_and_the_json_entry_point_agree_where_their_grammars_overlap(L):
    """Both run csv::strict_number.  Without whitespace around the text and without NaN / Infinity, JSON adds one thing:
    the integer literal -0 has no sign (int(-0) is 0), where pyarrow's double column keeps it."""
    strings = _strings(5_000, 20260118)

    def parse_json(s: str):
        b = s.encode()
        out, is_int = ctypes.c_double(math.nan), ctypes.c_int(-1)
        rc = L.mcr_parse_json_number(b, len(b), ctypes.byref(out), ctypes.byref(is_int))
        return rc, struct.pack("<d", out.value), is_int.value

    seen = {0: 0, 1: 0, EFALLBACK: 0}
    for s in strings:
        rc, v, is_int = parse(L, s)
        got = parse_json(s)
        if s == "-0":
            assert (rc, struct.pack("<d", v), is_int) == (0, struct.pack("<d", -0.0), 1), s
            assert got == (0, struct.pack("<d", 0.0), 1), s
            continue
        assert got == (rc, struct.pack("<d", v), is_int), s
        seen[rc] += 1
    assert strings.count("-0") >= 1 and seen[0] > 20_000 and seen[1] >= 200 and seen[EFALLBACK] >= 1, seen


REJECTED = ["", " 1", "1 ", "+1", "01", ".5", "5.", "1e", "-", "inf", "Infinity", "nan", "NaN", "true", "0x10", "1_0",
            "2020-01-01", '"1"', "9007199254740993"]


def test_texts_outside_the_subset_are_handed_back(L):
    for s in REJECTED + ["-9007199254740993", "1e+", "1.e5", "-.5", "--1", "1,", "1\r", "\t1", "00", "-01", "1.5.2", "1e5e5",
                         "١", "1" * 17, "12345678901234567890"]:
        assert parse(L, s)[0] == EFALLBACK, s
    out, is_int = ctypes.c_double(), ctypes.c_int()
    assert L.mcr_parse_csv_number(None, 3, ctypes.byref(out), ctypes.byref(is_int)) == EINVAL
    assert L.mcr_parse_csv_number(b"1", 1, None, ctypes.byref(is_int)) == EINVAL
    assert L.mcr_parse_csv_number(b"1", 1, ctypes.byref(out), None) == EINVAL


def header(L, data: bytes):
    h = ctypes.c_void_p()
    assert L.mcr_csv_open_table(None, data, len(data), ctypes.byref(h)) == 0
    try:
        names = [L.mcr_csv_column_name(h, c) for c in range(L.mcr_csv_num_columns(h))]
        return names, L.mcr_csv_table_flags(h), L.mcr_csv_body_offset(h)
    finally:
        L.mcr_csv_close(h)


def test_the_header_is_the_first_non_empty_line_with_raw_names(L):
    import pyarrow.csv as pacsv
    for data in [b"a,b\n1,2\n", b"\n\r\n\na, b ,#c\r\n1,2,3\r\n", b"# not a comment,x\n1,2\n", b"a,b", b"\r\na\r\n1"]:
        names, flags, body = header(L, data)
        table = pacsv.read_csv(io.BytesIO(data)) if b"\n1" in data else None
        if table is not None:
            assert [n.decode() for n in names] == table.column_names, data
        assert flags == 0, data
        first = data.lstrip(b"\r\n")
        end = first.find(b"\n")
        assert body == (len(data) if end < 0 else len(data) - len(first) + end + 1), data
    assert header(L, b"a, b ,#c\r\n")[0] == [b"a", b" b ", b"#c"]
    assert header(L, b"a,b")[0] == [b"a", b"b"]


def test_header_conditions_outside_the_subset_are_flagged(L):
    assert header(L, b"\xef\xbb\xbfa,b\n1,2\n")[1] & T_BOM
    assert header(L, b"a,b,a\n1,2,3\n")[1] == T_DUP
    assert header(L, b"a,,b\n1,2,3\n")[1] == T_EMPTY
    assert header(L, b"a,b,\n1,2,3\n")[1] == T_EMPTY
    assert header(L, b'a,"b"\n1,2\n')[1] == T_QUOTE
    assert header(L, b"a\rb,c\n1,2\n")[1] == T_CR
    assert header(L, b"")[1] == T_NO_HEADER and header(L, b"\n\r\n\n")[1] == T_NO_HEADER
    # a chain-file handle has no table flags, and the CmdStan header rules are not these
    h = ctypes.c_void_p()
    assert L.mcr_csv_open(None, b"# c\na,b\n", 8, ctypes.byref(h)) == 0
    assert L.mcr_csv_table_flags(h) == -1 and L.mcr_csv_num_columns(h) == 2
    L.mcr_csv_close(h)
    assert L.mcr_csv_table_flags(None) == -1
