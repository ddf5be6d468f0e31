#!/usr/bin/env python3
"""Golden cases for the CmdStan CSV decoder, made by IMPORTING the reference.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_csv.py

Runs only in the build container (needs /root/reference).  Emits data only, cmdstan_csv_cases.json: small CSV texts
written by this script and what the reference's parse_cmdstan_csv() returned for each ({normalised name: draws}, values
as hex floats, names in the order the reference produced them), plus the raw header fields csv.reader sees on the same
filtered lines and the offset of the first byte after the header line.  The texts pin the row, comment and name rules:
comments before, between and after the draws, CRLF line ends, a last line without a newline, blank lines, `__`
columns in the middle of the header, dotted names, spaces around fields, the number spellings CmdStan and other writers
produce.
"""
from __future__ import annotations

import csv
import json
import sys
import tempfile
from pathlib import Path

REF = Path("/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [str(REF / "src")]
HERE = Path(__file__).resolve().parent

from mcmc_ref import cmdstan_generate as ref_cs  # noqa: E402

HEADER = "lp__,accept_stat__,mu,tau,theta.1,theta.2"
ROWS = ["-7.25,0.91,1.5,0.25,-3.0e-2,4", "-6.5,0.88,2.5,0.5,1e3,-0.0", "-8,1,3.5,0.75,2.2250738585072014e-308,17.000000000000004"]

TEXTS = {
    "plain": "\n".join([HEADER] + ROWS) + "\n",
    "comments_everywhere": "\n".join(["# model = demo", "#", HEADER, "# Adaptation terminated", "# Step size = 0.35", ROWS[0],
                                      "# a comment between the draws, with, commas", ROWS[1], "#", ROWS[2], "# ",
                                      "#  Elapsed Time: 0.01 seconds (Warm-up)"]) + "\n",
    "crlf": "\r\n".join(["# model = demo", HEADER, "# adaptation"] + ROWS + ["# done"]) + "\r\n",
    "crlf_blank_lines": "\r\n".join([HEADER, ROWS[0], "", ROWS[1], "", "", ROWS[2], ""]) + "\r\n",
    "no_final_newline": "\n".join(["# c", HEADER] + ROWS),
    "no_final_newline_comment_last": "\n".join([HEADER] + ROWS + ["# trailing comment without a newline"]),
    "blank_lines": "\n".join([HEADER, "", ROWS[0], "", "", ROWS[1], ROWS[2], "", ""]) + "\n",
    "internal_in_the_middle": "\n".join(["a,lp__,b.1,stepsize__,b.2,energy__,c", "1,2,3,4,5,6,7", "8,9,10,11,12,13,14"]) + "\n",
    "dotted_names": "\n".join(["theta.1,theta.12.3,Sigma.1.2.3,a.b,x.1a,z_9.0,_t.2,plain", "1,2,3,4,5,6,7,8", "9,10,11,12,13,14,15,16"]) + "\n",
    "spaces_around_fields": "\n".join(["mu,tau,eta", " 1.5, 2.5 ,3.5 ", "  -4e-3 ,\t5,6\t", "7 , 8 , 9"]) + "\n",
    "number_spellings": "\n".join(["a,b,c,d", "+1.5,.5,5.,1E5", "-0,0.0,-0.0e0,00012", "1e-400,1e400,-1e400,5e-324",
                                   "9007199254740993,0.1,1.7976931348623157e308,123456789012345678901234567890",
                                   "2.4703282292062327e-324,2.4703282292062328e-324,4.9406564584124654e-324,1e23"]) + "\n",
    "header_only": "# c\n" + HEADER + "\n# no draws\n",
    "header_only_no_newline": HEADER,
    "one_column": "x\n1\n2\n3\n",
    "one_row_no_newline": "x,y\n1.25,2.5",
}


def case(text: str) -> dict:
    with tempfile.TemporaryDirectory() as td:
        p = Path(td) / "chain.csv"
        p.write_bytes(text.encode())
        got = ref_cs.parse_cmdstan_csv(p)
        with p.open() as f:
            kept = [ln for ln in f if not ln.startswith("#")]
    header = next(csv.reader(kept)) if kept else []
    raw, off = text.encode(), 0
    while off < len(raw):                   # the first byte after the first line that is no comment
        end = raw.find(b"\n", off)
        end = len(raw) if end < 0 else end + 1
        comment = raw[off:off + 1] == b"#"
        off = end
        if not comment:
            break
    return {"text": text, "header": header, "body_offset": off,
            "names": list(got), "rows": len(next(iter(got.values()))) if got else 0,
            "columns": {k: [float(x).hex() for x in v] for k, v in got.items()}}


def main():
    out = {name: case(text) for name, text in TEXTS.items()}
    (HERE / "cmdstan_csv_cases.json").write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", HERE / "cmdstan_csv_cases.json", (HERE / "cmdstan_csv_cases.json").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
