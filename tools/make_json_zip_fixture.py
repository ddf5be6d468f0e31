#!/usr/bin/env python3
"""Records what the reference's JSON-zip reader does with a set of small documents: tests/golden/json_zip_cases.json.

    python tools/make_json_zip_fixture.py /path/to/reference/src

The reference package is imported from the path given on the command line and its `convert._read_json_zip` is run on
every document below.  Only data is written: per case the document's text and either the table's column names, Arrow
types and values or the exception's type and message.  Non-finite values are recorded as the strings "NaN",
"Infinity", "-Infinity".
"""
from __future__ import annotations

import importlib
import json
import math
import sys
import tempfile
import zipfile
from pathlib import Path

OUT = Path(__file__).resolve().parents[1] / "tests" / "golden" / "json_zip_cases.json"

# name -> document text.  The first block is inside the subset the device reader certifies, the second is its fallback
# list (mcmcref_hip.h, MCR_EFALLBACK) and the reference's own KeyError / IndexError cases.
DOCUMENTS = {
    "float_columns": '[{"mu": [0.5, -1.25, 3e-05], "tau": [1.0, 2.5, 1e+22]}, {"mu": [0.1, 0.2, 0.3], "tau": [4.0, 5.0, 6.0]}]',
    "int_column": '[{"k": [1, 2, 3], "x": [0.5, 1.5, 2.5]}, {"k": [4, -5, 0], "x": [3.5, 4.5, 5.5]}]',
    "mixed_column": '[{"m": [1, 2.5, 3]}, {"m": [4, 5, 6]}]',
    "int_in_one_chain_float_in_other": '[{"m": [1, 2, 3]}, {"m": [4.0, 5.0, 6.0]}]',
    "negative_zero_literals": '[{"z": [-0, 1.5, -0.0]}, {"z": [0, -0, 2.0]}]',
    "negative_zero_int_column": '[{"z": [-0, 1]}, {"z": [2, -0]}]',
    "int_at_2_53": '[{"b": [9007199254740992, 1]}, {"b": [-9007199254740992, 2]}]',
    "sorted_params_document_first_length": '[{"zeta": [1.5, 2.5], "alpha": [9.5, 8.5, 7.5]}, {"alpha": [1.0, 2.0, 3.0], "zeta": [5.0, 6.0]}]',
    "longer_later_chain_is_cut": '[{"a": [1.5, 2.5]}, {"a": [3.5, 4.5, 5.5, 6.5]}]',
    "extra_key_in_later_chain": '[{"a": [1.5]}, {"a": [2.5], "extra": [1, 2, 3]}]',
    "structural_characters_in_keys": '[{"theta[1,2]": [1.5], "a:b": [2.5], "{x}": [3.5], "],[": [4.5]}]',
    "nonfinite_literals": '[{"v": [NaN, Infinity, -Infinity, 1.0]}]',
    "indented_crlf": '[\r\n  {\r\n    "a": [\r\n      1.5,\r\n      2\r\n    ]\r\n  }\r\n]\r\n',
    "twenty_five_digit_tie": '[{"t": [9007199254740993.00000000, 0.1000000000000000055511151231257827]}]',
    "backslash_in_key": '[{"a\\\\nb": [1.5, 2.5]}]',
    "unicode_escape_in_key": '[{"\\u0061": [1.5]}]',
    "top_level_object": '{"a": [1.5, 2.5]}',
    "top_level_array_of_numbers": '[1.5, 2.5]',
    "top_level_array_of_arrays": '[[1.5, 2.5]]',
    "byte_order_mark": '\ufeff[{"a": [1.5]}]',
    "empty_top_level_array": '[]',
    "member_is_a_number": '[{"a": 1.5}]',
    "member_is_nested": '[{"a": [[1.5], [2.5]]}]',
    "member_holds_strings": '[{"a": ["x", "y"]}]',
    "member_holds_true_and_null": '[{"a": [true, null]}]',
    "duplicate_key": '[{"a": [1.5, 2.5], "a": [3.5, 4.5]}]',
    "chain_missing_a_parameter": '[{"a": [1.5], "b": [2.5]}, {"a": [3.5]}]',
    "shorter_later_chain": '[{"a": [1.5, 2.5, 3.5]}, {"a": [4.5, 5.5]}]',
    "int_beyond_2_53_with_floats": '[{"a": [9007199254740993, 1.5]}]',
    "int_beyond_int64": '[{"a": [123456789012345678901234567890, 1]}]',
    "leading_plus": '[{"a": [+1.5]}]',
    "leading_zero": '[{"a": [01.5]}]',
    "trailing_comma": '[{"a": [1.5, 2.5,]}]',
    "unclosed": '[{"a": [1.5, 2.5]}',
    "first_chain_has_no_keys": '[{}, {"a": [1.5]}]',
}


def plain(v):
    if isinstance(v, float) and not math.isfinite(v):
        return "NaN" if v != v else ("Infinity" if v > 0 else "-Infinity")
    return v


def record(convert, text: str, tmp: Path) -> dict:
    path = tmp / "case.json.zip"
    with zipfile.ZipFile(path, "w") as zf:
        zf.writestr("case.json", text.encode("utf-8"))
    try:
        table = convert._read_json_zip(path)
    except Exception as exc:  # noqa: BLE001 - the exception is the record
        return {"text": text, "error": {"type": type(exc).__name__, "message": str(exc)}}
    return {"text": text, "columns": table.column_names, "types": [str(t) for t in table.schema.types],
            "values": [[plain(v) for v in table.column(c).to_pylist()] for c in table.column_names]}


def main() -> None:
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    convert = importlib.import_module("mcmc_ref.convert")
    with tempfile.TemporaryDirectory() as d:
        cases = {name: record(convert, text, Path(d)) for name, text in DOCUMENTS.items()}
    OUT.write_text(json.dumps(cases, indent=1, sort_keys=True) + "\n")
    print(f"{OUT}: {len(cases)} cases")


if __name__ == "__main__":
    main()
