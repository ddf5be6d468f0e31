"""The CSV writer's grammar and tiling without a GPU: mcr_format_double and mcr_csv_write_host, which runs the device's
formatter over the device's tiles.  Every comparison is bytes == bytes against pyarrow.csv.write_csv of the same table
(tests/csvwrite_cases.py); there are no tolerances."""
from __future__ import annotations

import ctypes as C
import importlib.util
import re

import numpy as np
import pytest

import csvwrite_cases as W
from conftest import ROOT
from csvwrite_cases import DOUBLE, INT32, INT64


@pytest.fixture(scope="module")
def ffi():
    spec = importlib.util.spec_from_file_location("mcr_build", ROOT / "mcmc-db_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from mcmc_ref_hip import _ffi
    _ffi.load_library()
    return _ffi


def test_constants_match_the_header(ffi):
    header = (ROOT / "include" / "mcmcref_hip.h").read_text()
    defs = dict(re.findall(r"#define (MCR_(?:CSVW|SELECT)_[A-Z_]+) (\d+)", header))
    assert int(defs["MCR_CSVW_TILE_FIELDS"]) == W.F == ffi.MCR_CSVW_TILE_FIELDS
    assert int(defs["MCR_CSVW_FIELD_MAX"]) == W.FIELD_MAX == ffi.MCR_CSVW_FIELD_MAX
    assert int(defs["MCR_SELECT_BLOCK_ROWS"]) == W.SELECT_BLOCK == ffi.MCR_SELECT_BLOCK_ROWS
    assert {k: int(defs[f"MCR_CSVW_HEADER_{k.upper()}"]) for k in ffi.CSV_HEADERS} == ffi.CSV_HEADERS


def test_value_corpus_equals_pyarrow_and_reads_back(ffi):
    x = W.corpus()
    assert x.size >= 856_293
    cols = [("v", DOUBLE, x)]
    got = W.write_host(cols, x.size, header="none")
    assert got == W.expected(cols, x.size, header="none")
    fields = got.split(b"\n")[:-1]
    assert len(fields) == x.size and max(map(len, fields)) == 25
    finite = np.isfinite(x)
    back = np.array([float(f) for f, ok in zip(fields, finite) if ok])
    assert np.array_equal(back.view(np.uint64), x[finite].view(np.uint64))          # the shortest digits still read back to the bits
    assert all(f in (b"nan", b"inf", b"-inf") for f, ok in zip(fields, finite) if not ok)


def test_edge_list(ffi):
    x = np.array(W.EDGES + [-v for v in W.EDGES])
    cols = [("v", DOUBLE, x)]
    exp = W.expected(cols, x.size, header="none")
    assert W.write_host(cols, x.size, header="none") == exp
    fields = exp.decode().split("\n")[:-1]
    for v, f in zip(x, fields):
        assert ffi.format_double(float(v)) == f == W.py_field(float(v)), repr(v)
    for v, text in ((1e-6, "0.000001"), (9.5e-7, "9.5e-7"), (1e10, "1e+10"), (9999999999.0, "9999999999"), (1500000000.0, "1500000000"),
                    (12345.678, "12345.678"), (5e-324, "5e-324"), (1.7976931348623157e308, "1.7976931348623157e+308"),
                    (2.0 ** 53, "9.007199254740992e+15"), (-0.0, "-0"), (W.nan_bits(1, 5), "nan"), (-np.inf, "-inf")):
        assert ffi.format_double(v) == text


def test_integer_columns(ffi):
    i = np.array(W.INT_EDGES, dtype=np.int64)
    small = np.array([0, 1, -1, 2147483647, -2147483648], dtype=np.int64)
    cols = [("a", INT64, i), ("b", INT32, np.resize(small, i.size)), ("c", INT64, np.resize(small, i.size).astype(np.float64)),
            ("d", INT32, i)]                                   # INT32 and INT64 print alike: the full range
    exp = W.expected([cols[0], cols[1], ("c", INT64, np.resize(small, i.size)), ("d", INT64, i)], i.size)
    assert W.write_host(cols, i.size) == exp
    bad = np.resize(small, i.size).astype(np.float64)
    bad[3] = 0.5
    with pytest.raises(ffi.McrError, match=r"column 'frac', row 3 .*not an integer") as err:
        W.write_host([("a", INT64, i), ("frac", INT64, bad)], i.size)
    assert err.value.code == ffi.MCR_EINVAL


@pytest.mark.parametrize("header", ["quoted", "plain", "none"])
def test_headers(ffi, header):
    names = ['say "hi"', "a,b", "line\nbreak", "theta[1]", "µ_σ²", "plain"] if header != "plain" else ["theta[1]", "µ_σ²", "plain", "a b"]
    for rows in (0, 3):
        cols = [(n, DOUBLE, np.arange(rows) + 0.5) for n in names]
        assert W.write_host(cols, rows, header=header) == W.expected(cols, rows, header=header)
    if header == "plain":
        for name in ('q"', "a,b", "x\ny", "x\r"):
            with pytest.raises(ffi.McrError, match="plain header"):
                W.write_host([(name, DOUBLE, np.zeros(1))], 1, header="plain")
    if header == "quoted":
        assert W.write_host([('a"b', INT64, ("seq", 1, 5))], 0) == b'"a""b"\n'


@pytest.mark.parametrize("n_cols", W.N_COLS)
def test_geometry(ffi, n_cols):
    for rows in W.rows_for(n_cols):
        cols, rows = W.table_case(n_cols, rows)
        assert len(cols) == n_cols
        assert W.write_host(cols, rows) == W.expected(cols, rows), rows
    cols, rows = W.table_case(n_cols, W.rows_for(n_cols)[-1])
    for name, index in W.row_lists(rows).items():
        assert W.write_host(cols, rows, index, "none") == W.expected(cols, rows, index, "none"), name


def test_length_classes_share_a_tile(ffi):
    cols, rows = W.length_class_columns()
    assert len(cols) * rows <= W.F
    got = W.write_host(cols, rows, header="none")
    assert got == W.expected(cols, rows, header="none")
    assert {len(f) for line in got.split(b"\n")[:-1] for f in line.split(b",")} == set(range(1, 26))


def test_bad_arguments_are_named(ffi):
    lib = ffi.load_library()
    x = np.arange(4, dtype=np.float64)

    def call(cols, rows, index=None, n_index=0, n_cols=None):
        arr, _keep = ffi._pq_columns(cols, host=True)
        h = C.c_void_p()
        rc = lib.mcr_csv_write_host(None, arr, len(cols) if n_cols is None else n_cols, rows,
                                    None if index is None else index.ctypes.data_as(C.POINTER(C.c_int64)), n_index, 0, C.byref(h))
        return rc, (lib.mcr_last_error(None) or b"").decode()

    col = ffi.pq_column("x", DOUBLE, x)
    for args, what in (((([col], -1)), "row count -1"), (([col], 1 << 31), "row count 2147483648"), (([col], 4, None, 0, 0), "n_cols = 0")):
        rc, msg = call(*args)
        assert rc == ffi.MCR_EINVAL and what in msg, msg
    arr, _keep = ffi._pq_columns([col], host=True)
    arr[0].stride = 0
    h = C.c_void_p()
    assert lib.mcr_csv_write_host(None, arr, 1, 4, None, 0, 0, C.byref(h)) == ffi.MCR_EINVAL
    assert "stride 0" in lib.mcr_last_error(None).decode()
    for index, at in ((np.array([0, 4], dtype=np.int64), 1), (np.array([-1, 0, 9], dtype=np.int64), 0)):
        rc, msg = call([col], 4, index, index.size)
        assert rc == ffi.MCR_EINVAL and f"entry {at} of the row list" in msg, msg
    with pytest.raises(ffi.McrError, match="integer source"):
        W.write_host([("i", DOUBLE, np.arange(3, dtype=np.int64))], 3)


def test_generator_reproduces_the_committed_table(ffi):
    spec = importlib.util.spec_from_file_location("gen_pow10", ROOT / "tools" / "gen_pow10.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.OUT.read_bytes() == mod.text().encode()
