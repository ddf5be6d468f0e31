"""Shared by test_csv_write_cpu.py and test_csv_write_gpu.py: the values, tables and row lists the CSV writer is tried
on, and what `pyarrow.csv.write_csv` makes of the same table -- the one oracle, compared byte for byte.

A column here is (name, physical type, numpy array of float64 / int64 -- possibly a strided view) or
(name, type, ("seq", div, mod)).  No GPU, no library: numpy and pyarrow only."""
from __future__ import annotations

import decimal
import io
import math

import numpy as np

INT32, INT64, DOUBLE = 1, 2, 5
F = 2048                               # MCR_CSVW_TILE_FIELDS (asserted against the header by the CPU test)
FIELD_MAX = 26                         # MCR_CSVW_FIELD_MAX
SELECT_BLOCK = 256                     # MCR_SELECT_BLOCK_ROWS
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
N_COLS = (1, 2, 3, F - 1, F, F + 1, 2 * F + 1)


def rows_for(n_cols: int) -> list[int]:
    """1, R - 1, R, R + 1, 2R + 3 for the R whole rows a tile holds at this width (R = 1 when a row is cut)."""
    R = max(F // n_cols, 1)
    return sorted({1, R - 1, R, R + 1, 2 * R + 3})


def py_field(v: float) -> str:
    """A plain-Python model of the float64 grammar: repr's shortest digits, placed by the rules of the header."""
    if v != v:
        return "nan"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    sign = "-" if math.copysign(1.0, v) < 0 else ""
    if v == 0:
        return sign + "0"
    _s, digits, exp = decimal.Decimal(repr(abs(float(v)))).as_tuple()
    d = "".join(map(str, digits)).rstrip("0")
    exp += len(digits) - len(d)
    n, e = len(d), exp + len(d) - 1
    if -6 <= e <= 9:
        if e < 0:
            return sign + "0." + "0" * (-e - 1) + d
        return sign + (d + "0" * exp if exp >= 0 else d[:e + 1] + "." + d[e + 1:])
    return sign + d[0] + ("." + d[1:] if n > 1 else "") + ("e-" if e < 0 else "e+") + str(abs(e))


def corpus() -> np.ndarray:
    """The value corpus: random bit patterns, normals at 22 scales, integer-valued doubles, denormals, and every power
    of two with both neighbours."""
    rng = np.random.default_rng(20261018)
    parts = [rng.integers(0, 1 << 64, size=420_000, dtype=np.uint64).view(np.float64)]
    parts += [rng.standard_normal(14_000) * 10.0 ** k for k in range(-9, 13)]
    parts.append(np.trunc(rng.uniform(-1e12, 1e12, size=60_000)))
    parts.append(rng.integers(-100_000, 100_000, size=20_000).astype(np.float64))
    parts.append(rng.integers(1, 1 << 52, size=50_000, dtype=np.uint64).view(np.float64) * rng.choice([-1.0, 1.0], size=50_000))
    p2 = np.ldexp(1.0, np.arange(-1074, 1024))
    parts += [p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf)]
    return np.concatenate(parts)


def nan_bits(sign: int, payload: int) -> float:
    return float(np.array([(sign << 63) | (0x7FF << 52) | payload], dtype=np.uint64).view(np.float64)[0])


DBL_MIN = 2.2250738585072014e-308
EDGES = (
    [10.0 ** k for k in range(-10, 25)] + [1.5 * 10.0 ** k for k in range(-10, 25)]
    + [9.999999e-7, 1e-6, 9.5e-7]
    + [9999999999.0, 1e10, 12345000000.0, 1099511627776.0]
    + [999999999999999.0, 123456789012345.6]
    + [2.0 ** 53, 2.0 ** 53 + 2]
    + [DBL_MIN, float(np.nextafter(DBL_MIN, 0.0)), float(np.nextafter(DBL_MIN, 1.0))]
    + [5e-324, 1.7976931348623157e308, 0.0, -0.0, math.inf, -math.inf]
    + [nan_bits(0, 1 << 51), nan_bits(1, 1 << 51), nan_bits(0, 1), nan_bits(1, 0xABCDE)]
    + [1 / 3, -1 / 3, 0.1, 12345.678, 1500000000.0, 0.000001]
)
INT_EDGES = [0, 1, -1, 9, 10, -10, 2147483647, -2147483648, 2147483648, INT64_MAX, INT64_MIN, INT64_MAX - 1, 10 ** 18, -(10 ** 18)]


def length_class_columns(rows: int = 40):
    """One double column per field length 1 .. 25, values of the edge list's kinds: small integers, 1.5, 10^10 and
    1.5 x 10^10 of either sign, and 0.000001 followed by 0 .. 16 more digits, of either sign."""
    rng = np.random.default_rng(7)
    short = {1: 5.0, 2: 15.0, 3: 1.5, 4: -1.5, 5: 1e10, 6: -1e10, 7: 1.5e10}
    cols = []
    for L in range(1, 26):
        if L in short:
            a = np.full(rows, short[L])
        else:
            neg = L % 2 == 1                       # 0.000001 and `extra` more digits: 8 + extra bytes, one more when negative
            extra, a = L - 8 - neg, []
            while len(a) < rows:
                if extra <= 14:                    # up to 15 significant digits always read back as themselves
                    v = float("0.000001" + "".join(str(d) for d in rng.integers(1, 10, size=extra)))
                else:                              # 16 or 17 digits: whichever doubles need that many
                    v = float(rng.uniform(1e-6, 2e-6))
                v = -v if neg else v
                if len(py_field(v)) == L:
                    a.append(v)
            a = np.array(a)
        assert all(len(py_field(v)) == L for v in a), L
        cols.append((f"len{L}", DOUBLE, a))
    return cols, rows


def mixed_values(n: int, seed: int) -> np.ndarray:
    """n doubles of every kind of text: normals at many scales, integers, edges."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-9, 13, size=n)
    k = rng.integers(0, 10, size=n)
    a[k == 0] = np.trunc(a[k == 0])
    e = np.asarray(EDGES)
    a[k == 1] = e[rng.integers(0, e.size, size=int((k == 1).sum()))]
    return a


def table_case(n_cols: int, rows: int, seed: int = 0):
    """A table of n_cols columns: generated `chain` / `draw` first when there is room, an int64 column, doubles at
    stride 1, at stride 3, and interleaved in one row-major matrix."""
    rng = np.random.default_rng(seed + 31 * n_cols + rows)
    cols = []
    if n_cols >= 3:
        per = max((rows + 3) // 4, 1)
        cols += [("chain", INT32, ("seq", per, INT64_MAX)), ("draw", INT64, ("seq", 1, per))]
    if n_cols >= 4:
        cols.append(("count", INT64, rng.integers(-10 ** 6, 10 ** 6, size=rows).astype(np.int64)))
    left = n_cols - len(cols)
    n_inter = left // 2 if left >= 4 else 0
    mat = mixed_values(rows * n_inter, seed + 1).reshape(rows, n_inter) if n_inter else None
    for j in range(left):
        if j < n_inter:
            a = mat[:, j]
        elif j % 2:
            a = np.full(rows * 3, 77.0)[::3]
            a[:] = mixed_values(rows, seed + 2 + j)
        else:
            a = mixed_values(rows, seed + 2 + j)
        cols.append((f"x[{j}]", DOUBLE, a))
    return cols, rows


def row_lists(rows: int) -> dict:
    rng = np.random.default_rng(rows)
    return {"reversed": np.arange(rows, dtype=np.int64)[::-1].copy(),
            "repeats": rng.integers(0, max(rows, 1), size=rows + 5).astype(np.int64) if rows else np.zeros(0, dtype=np.int64),
            "empty": np.zeros(0, dtype=np.int64)}


def host_values(col, rows: int) -> np.ndarray:
    _name, type_, src = col
    if isinstance(src, tuple):
        _seq, div, mod = src
        a = (np.arange(rows, dtype=np.int64) // div) % mod
    else:
        a = np.asarray(src)[:rows]
    return a if type_ == DOUBLE else a.astype(np.int32 if type_ == INT32 else np.int64)


def expected(cols, rows: int, row_index=None, header: str = "quoted") -> bytes:
    """pyarrow.csv.write_csv of the same table."""
    import pyarrow as pa
    import pyarrow.csv as pacsv
    arrays = [host_values(c, rows) for c in cols]
    if row_index is not None:
        arrays = [a[np.asarray(row_index, dtype=np.int64)] for a in arrays]
    table = pa.Table.from_arrays([pa.array(a) for a in arrays], names=[c[0] for c in cols])
    opts = {"quoted": pacsv.WriteOptions(), "plain": pacsv.WriteOptions(quoting_header="none"),
            "none": pacsv.WriteOptions(include_header=False)}[header]
    sink = io.BytesIO()
    pacsv.write_csv(table, sink, opts)
    return sink.getvalue()


def host_columns(cols):
    """The columns as _ffi.write_csv_host takes them."""
    from mcmc_ref_hip import _ffi
    return [_ffi.pq_sequence(n, t, s[1], s[2]) if isinstance(s, tuple) else _ffi.pq_column(n, t, s) for n, t, s in cols]


def write_host(cols, rows: int, row_index=None, header: str = "quoted") -> bytes:
    from mcmc_ref_hip import _ffi
    with _ffi.write_csv_host(host_columns(cols), rows, row_index, header) as image:
        return image.tobytes()
