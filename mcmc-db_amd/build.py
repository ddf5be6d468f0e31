#!/usr/bin/env python3
"""Builds mcmc-db_amd/lib/libmcmcref_hip.so and its companions libmcmcref_iess.so (include/mcmcref_iess.h),
libmcmcref_bm.so (include/mcmcref_bm.h), libmcmcref_std.so (include/mcmcref_std.h) and libmcmcref_recdf.so
(include/mcmcref_recdf.h) -- each with its own units and its own version script, none linked against another -- for
gfx950 with hipcc (cross-compiles without a GPU).  libmcmcref_std.so and libmcmcref_recdf.so reuse the sort stage and the
summary pipeline as code: the objects of the main units are linked into each beside its own unit, and its version
script keeps every name but mcs_* (mce_*) local.

One object per translation unit of csrc/ (lib/obj/), each with the dependency file the compiler writes for it; stale
units compile concurrently and the objects are linked into the library.  No kernel is called across units, so the link
needs no relocatable device code."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parent
UNITS = ("mcr_api", "mcr_stats", "mcr_files", "mcr_comm")
IESS_UNITS = ("mci_api",)
BM_UNITS = ("mcb_api",)
STD_UNITS = ("mcs_api",)
RECDF_UNITS = ("mce_api",)
OBJ = HERE / "lib" / "obj"
OUT = HERE / "lib" / "libmcmcref_hip.so"
IESS_OUT = HERE / "lib" / "libmcmcref_iess.so"
BM_OUT = HERE / "lib" / "libmcmcref_bm.so"
STD_OUT = HERE / "lib" / "libmcmcref_std.so"
RECDF_OUT = HERE / "lib" / "libmcmcref_recdf.so"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden",
         "-Wall", "-Wno-unused-value", "-Wno-pass-failed"]
IESS_FLAGS = FLAGS + ["-ffp-contract=off", f"-I{HERE.parent / 'include'}"]    # host and device must round alike


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or add /opt/rocm/bin to PATH)")


def dep_files(dep: Path) -> list[str]:
    """The prerequisites a make-style dependency file names ("target: file file \\<newline> file ...")."""
    words = dep.read_text().replace("\\\n", " ").split(":", 1)[1].split()
    return [w.replace("\\ ", " ") for w in words]


def stale(unit: str) -> bool:
    """The object is missing, or older than a file its dependency file names (or that file cannot be read)."""
    obj, dep = OBJ / f"{unit}.o", OBJ / f"{unit}.d"
    try:
        return any(os.stat(f).st_mtime > obj.stat().st_mtime for f in dep_files(dep))
    except (OSError, IndexError, UnicodeError):
        return True


def run(cmd: list[str], verbose: bool) -> None:
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


# (output, units, version script): libmcmcref_std.so and libmcmcref_recdf.so link the main units' objects beside their own
LIBRARIES = ((OUT, UNITS, "mcr_exports.map"), (IESS_OUT, IESS_UNITS, "mci_exports.map"), (BM_OUT, BM_UNITS, "mcb_exports.map"),
             (STD_OUT, UNITS + STD_UNITS, "mcs_exports.map"), (RECDF_OUT, UNITS + RECDF_UNITS, "mce_exports.map"))
UNIT_FLAGS = {**{u: FLAGS for u in UNITS}, **{u: IESS_FLAGS for u in IESS_UNITS + BM_UNITS + STD_UNITS + RECDF_UNITS}}


def link(out: Path, units: tuple, version_script: str, relinked: bool, verbose: bool) -> None:
    objs = [OBJ / f"{u}.o" for u in units]
    if relinked or not out.exists() or any(o.stat().st_mtime > out.stat().st_mtime for o in objs):
        run([hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", f"-Wl,--version-script={HERE / 'csrc' / version_script}",
             "-o", str(out)] + [str(o) for o in objs], verbose)


def build(force: bool = False, verbose: bool = False) -> Path:
    """All five libraries; returns the path of libmcmcref_hip.so."""
    OBJ.mkdir(parents=True, exist_ok=True)
    cc = [hipcc()] + (["-Rpass-analysis=kernel-resource-usage"] if verbose else [])
    todo = [u for u in UNIT_FLAGS if force or stale(u)]
    if todo:
        jobs = min(len(todo), int(os.environ.get("MAX_JOBS", "4")))
        with ThreadPoolExecutor(max_workers=max(jobs, 1)) as pool:
            list(pool.map(lambda u: run(cc + UNIT_FLAGS[u] + ["-c", "-MD", "-MF", str(OBJ / f"{u}.d"), "-o", str(OBJ / f"{u}.o"),
                                                         str(HERE / "csrc" / f"{u}.hip")], verbose), todo))
    for out, units, version_script in LIBRARIES:
        link(out, units, version_script, any(u in units for u in todo), verbose)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
