"""The CmdStan CSV decoder's host side, without a GPU: the power-of-five table, the field parser the
kernels run (`mcr_parse_double` compiles the same `__host__ __device__` text) against Python's float() in bits, and
`mcr_csv_open` on the texts recorded from the reference."""
from __future__ import annotations

import ctypes
import importlib.util
import math
import random
import re
import struct
from decimal import Decimal, localcontext

import pytest

from conftest import GOLDEN, ROOT, load_json

CASES = load_json("cmdstan_csv_cases.json")


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
    out = ctypes.c_double(math.nan)
    rc = L.mcr_parse_double(b, len(b), ctypes.byref(out))
    return rc, out.value


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def sig_digits(s: str) -> int:
    m = re.fullmatch(r"\s*[+-]?(\d*)\.?(\d*)(?:[eE][+-]?\d+)?\s*", s)
    return len((m.group(1) + m.group(2)).strip("0"))      # zeros at either end carry no digit of the value


def test_committed_table_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("gen_pow5", ROOT / "tools" / "gen_pow5.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.OUT == ROOT / "mcmc-db_amd" / "csrc" / "mcr_pow5.h"
    assert gen.OUT.read_text() == gen.text()
    assert gen.entry(0) == 1 << 127 and gen.entry(-1) == 0xCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCD
    assert len(re.findall(r"0x[0-9a-f]{16}ull", gen.text())) == 2 * 651


def _writer_strings(n: int, seed: int):
    rng = random.Random(seed)
    for _ in range(n):
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        g = rng.gauss(0.0, 1.0) * 10.0 ** rng.randint(-30, 30)
        for v in (x, g):
            if v != v or math.isinf(v):
                continue
            yield repr(v)
            yield "%.6g" % v
            yield "%.18g" % v
            yield "%.25e" % v


def test_parser_equals_float_in_bits_and_decides_every_writer_format(L):
    n = hard = 0
    for s in _writer_strings(130_000, 4711):
        rc, got = parse(L, s)
        n += 1
        hard += rc == 1
        assert rc in (0, 1) and bits(got) == bits(float(s)), (s, rc, got)
    assert n >= 1_000_000
    assert hard == 0          # the published algorithm decides all of these


def test_parser_on_integers_and_named_edge_cases(L):
    rng = random.Random(7)
    hard = 0
    for _ in range(20_000):     # beyond 19 digits a rounding boundary may lie between the two 19-digit brackets: hard, never wrong
        s = str(rng.randrange(10 ** rng.randint(1, 30)))
        rc, got = parse(L, s)
        assert rc in (0, 1) and (rc == 0 or sig_digits(s) > 19) and bits(got) == bits(float(s)), (s, rc, got)
        hard += rc
    assert hard < 400
    strings = [".5", "5.", "+1.5", "1E5", "-0", "1e400", "1e-400", "-1e400", "5e-324", "0", "000", "0.000", "-0.0e10",
                "2.4703282292062327e-324", "2.4703282292062328e-324",      # either side of half the smallest subnormal
                "1.7976931348623157e308", "1.7976931348623159e308", "1.7976931348623158e308",
                "9007199254740993", "9007199254740992", "9007199254740995", "2.2250738585072011e-308",
                "2.2250738585072014e-308", "1e23", "8.5e22", "1e-343", "1e-342", "1e309", "1e308",
                " 1.5", "1.5 ", "\t1.5\r", "1e+5", "1e-5", "0e99999999999999999999", "1e99999999999999999999",
                "1e-99999999999999999999", "0." + "0" * 400 + "1e401", "1" + "0" * 400 + "e-400"]
    for s in strings:
        rc, got = parse(L, s)
        assert rc == 0 and bits(got) == bits(float(s)), (s, rc, got)


def test_golden_cmdstan_fields_are_all_decided(L):
    n = 0
    for chain in (1, 2):
        lines = [ln for ln in (GOLDEN / "cmdstan" / f"chain_{chain}.csv").read_text().splitlines() if not ln.startswith("#")]
        for ln in lines[1:]:
            for field in ln.split(","):
                rc, got = parse(L, field)
                assert rc == 0 and bits(got) == bits(float(field)), field
                n += 1
    assert n == 1440


def _halfway_strings(n: int, seed: int):
    """The exact midpoint of a finite double and its successor, every digit written out."""
    rng = random.Random(seed)
    with localcontext() as c:
        c.prec = 1200
        for i in range(n):
            if i % 4 == 0:      # integers of 54 .. 63 bits: midpoints of at most 19 digits
                x = float(rng.randrange(1 << 53, 1 << 62))
            else:
                x = abs(struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64) & ~(1 << 63)))[0])
            y = math.nextafter(x, math.inf)
            if x != x or math.isinf(x) or math.isinf(y):
                continue
            mid = (Decimal(x) + Decimal(y)) / 2
            yield format(mid, "f") if i % 2 else format(mid, "e")


def test_halfway_values_are_hard_or_right(L):
    n = hard = long_ones = 0
    for s in _halfway_strings(20_000, 99):
        rc, got = parse(L, s)
        n += 1
        assert rc in (0, 1) and bits(got) == bits(float(s)), (s, rc, got)     # decided or finished by the host: float()
        if sig_digits(s) > 19:
            long_ones += 1
            assert rc == 1, s          # no 19-digit prefix can settle a tie
        hard += rc == 1
    assert n > 19_000 and long_ones > 10_000 and hard >= long_ones


@pytest.mark.parametrize("text", ["inf", "nan", "-Infinity", "+INF", "NaN", "-nan", " inf ", "iNfInItY"])
def test_words_are_hard_and_finished_like_float(L, text):
    rc, got = parse(L, text)
    assert rc == 1
    exp = float(text)
    assert (got != got and exp != exp) or bits(got) == bits(exp)


@pytest.mark.parametrize("text", ["abc", "", " ", "1_0", "0x1p3", "1e", "--1", "1e+", ".", "+", "1.5.2", "1,5", "infinit", "nane",
                                  "1 2", "e5", "- 1"])
def test_text_float_refuses_is_einval(L, text):
    with pytest.raises(ValueError):
        float(text.replace("_", "x"))           # (float() itself allows 1_0: the grammar here is the one without underscores)
    rc, _ = parse(L, text)
    assert rc == -1


def _open(L, raw: bytes):
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(raw, max(len(raw), 1))
    assert L.mcr_csv_open(None, buf if raw else None, len(raw), ctypes.byref(h)) == 0
    try:
        n = L.mcr_csv_num_columns(h)
        names = [L.mcr_csv_column_name(h, c).decode() for c in range(n)]
        assert L.mcr_csv_column_name(h, n) is None and L.mcr_csv_column_name(h, -1) is None
        return names, int(L.mcr_csv_body_offset(h))
    finally:
        L.mcr_csv_close(h)


@pytest.mark.parametrize("name", sorted(CASES))
def test_csv_open_finds_header_names_and_body_of_every_recorded_text(L, name):
    case = CASES[name]
    names, body = _open(L, case["text"].encode())
    assert names == case["header"]
    assert body == case["body_offset"]
    from mcmc_ref_hip import cmdstan_generate as cs
    kept = [cs._normalize_cmdstan_param_name(h) for h in names if h and not h.endswith("__")]
    if case["rows"]:
        assert kept == case["names"]              # the reference's own keys, in its order


def test_csv_open_without_a_header(L):
    raw = b"# only\n# comments\n"
    assert _open(L, raw) == ([], len(raw))
    assert _open(L, b"") == ([], 0)
    assert _open(L, b"# no newline") == ([], 12)
    assert _open(L, b" a , b.1 ,c__\r\n1,2,3\r\n") == (["a", "b.1", "c__"], 15)
    assert _open(L, b"a,b") == (["a", "b"], 3)


def test_chunk_constant_is_documented():
    header = (ROOT / "include" / "mcmcref_hip.h").read_text()
    assert re.search(r"#define MCR_CSV_CHUNK 16384\b", header)
