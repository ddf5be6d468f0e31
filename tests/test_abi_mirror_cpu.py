"""One check of the whole Python mirror of include/mcmcref_hip.h, and of the surface `_ffi` re-exports.

`mcmc_ref_hip/_abi.py` restates the header by hand: constants, structures, and (restype, argtypes) of every entry.  A wrong
argtypes entry -- c_int where the header says int64_t -- is silent undefined behaviour, so everything the header states is
compared here, once: every `#define MCR_*` the module mirrors, the fields of every structure, the parameters and the
return type of every declaration.  The header is regular enough for ONE regular expression per kind over the
comment-stripped text; a declaration that does not parse fails the test by name.

`tests/golden/ffi_surface.json` records what `_ffi` offered before it was split into units (names, signatures, docstring
hashes): the split moved code and changed nothing a caller sees.  No GPU, no device call.
"""
from __future__ import annotations

import ast
import ctypes as C
import hashlib
import inspect
import itertools
import json
import re
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SURFACE = ROOT / "tests" / "golden" / "ffi_surface.json"

# ---- the header ---------------------------------------------------------------------------------------------------------
DEFINE = re.compile(r"^[ \t]*#define[ \t]+(MCR_\w+)[ \t]+\(?(-?\d+)(?:ll)?\)?[ \t]*$", re.M)
STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
DECLARATION = re.compile(r"^[ \t]*((?:const[ \t]+)?\w+[ \t]*\**)[ \t]*(mcr_\w+)[ \t]*\(([^()]*)\)[ \t]*;", re.M)

# a C scalar and a ctypes scalar agree when kind, width and sign do (size_t and uint64_t are one ctypes type on LP64)
C_SCALARS = {"int": "i32", "int64_t": "i64", "size_t": "u64", "uint64_t": "u64", "double": "f64", "void": "void"}
PY_SCALARS = {C.c_int: "i32", C.c_int64: "i64", C.c_size_t: "u64", C.c_uint64: "u64", C.c_double: "f64", None: "void"}

# header structure -> its class in _abi (mcr_parquet_request is the one typedef without a tag)
STRUCTS = {"mcr_summary": "Summary", "mcr_kernel_time": "KernelTime", "mcr_model_desc": "ModelDesc", "mcr_nested": "Nested",
           "mcr_pareto": "Pareto", "mcr_psis_out": "Psis", "mcr_hdi_out": "Hdi", "mcr_weighted_out": "Weighted",
           "mcr_sbc_out": "Sbc", "mcr_acf_out": "Acf", "mcr_parquet_request": "ParquetRequest",
           "mcr_id_columns": "IdColumns", "mcr_pq_column": "PqColumn"}


@pytest.fixture(scope="module")
def header() -> str:
    text = (ROOT / "include" / "mcmcref_hip.h").read_text()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.fixture(scope="module")
def abi():
    from mcmc_ref_hip import _abi
    return _abi


def c_class(text: str) -> str:
    """The class of a C parameter, return type or field: "ptr" for a pointer of any kind, else the scalar's."""
    if "*" in text:
        return "ptr"
    words = [w for w in text.split() if w != "const"]
    assert words and words[0] in C_SCALARS, f"no class for the C type in {text!r}"
    return C_SCALARS[words[0]]


def py_class(t) -> str:
    if t in (C.c_void_p, C.c_char_p) or (inspect.isclass(t) and issubclass(t, C._Pointer)):
        return "ptr"
    if inspect.isclass(t) and issubclass(t, C.Array):
        return f"{t._type_.__name__}[{t._length_}]"
    assert t in PY_SCALARS, f"no class for the ctypes type {t!r}"
    return PY_SCALARS[t]


def c_fields(body: str) -> list:
    """(name, class) of every field of a structure body: `double *a, *b;`, `int64_t C, N, P;`, `char name[48];`."""
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", decl, flags=re.S).groups()
        for d in rest.split(","):
            name = d.replace("*", " ").strip()
            if "[" in name:                                   # an array of chars: c_char[48]
                name, n = re.fullmatch(r"(\w+)\[(\d+)\]", name).groups()
                out.append((name, f"c_{base}[{n}]"))
            else:
                out.append((name, c_class(f"{base} {d}")))
    return out


def test_constants(header, abi):
    defines = {k: int(v) for k, v in DEFINE.findall(header)}
    mirrored = {k: v for k, v in vars(abi).items() if k.startswith("MCR_") and isinstance(v, int)}
    assert len(mirrored) >= 13
    for name, value in sorted(mirrored.items()):
        assert name in defines, f"_abi.{name} has no #define in mcmcref_hip.h"
        assert value == defines[name], f"_abi.{name} = {value}, the header says {defines[name]}"


def test_structures(header, abi):
    found = {m.group(3): m.group(2) for m in STRUCT.finditer(header)}
    assert set(found) == set(STRUCTS), "the header's structures and the table of their classes differ"
    classes = {k for k, v in vars(abi).items() if inspect.isclass(v) and issubclass(v, C.Structure)}
    assert classes == set(STRUCTS.values()), "a ctypes.Structure of _abi mirrors no structure of the header"
    for cname, body in found.items():
        mirror = [(n, py_class(t)) for n, t in getattr(abi, STRUCTS[cname])._fields_]
        assert mirror == c_fields(body), f"{STRUCTS[cname]}._fields_ is not {cname}"


def test_functions(header, abi):
    named = set(re.findall(r"\b(mcr_[a-z0-9_]+)\s*\(", header))          # what test_abi_exports_every_declared_symbol counts
    parsed = {m.group(2): (m.group(1), m.group(3)) for m in DECLARATION.finditer(header)}
    assert not named - set(parsed), f"declarations that do not parse: {sorted(named - set(parsed))}"
    assert set(parsed) == set(abi.SYMBOLS)
    lib = abi.load_library()
    for name, (ret, params) in sorted(parsed.items()):
        assert hasattr(lib, name), name
        restype, argtypes = abi.SYMBOLS[name]
        want = [] if params.strip() in ("", "void") else [c_class(p) for p in params.split(",")]
        assert [py_class(t) for t in argtypes] == want, f"{name}: argtypes do not match ({' '.join(params.split())})"
        assert py_class(restype) == c_class(ret), f"{name}: restype does not match {ret.strip()!r}"


def test_context_bases_share_no_method():
    from mcmc_ref_hip import _ffi
    bases = _ffi.Context.__bases__
    assert len(bases) == 3 and all(b.__bases__ == (object,) for b in bases)
    implicit = {"__module__", "__doc__", "__dict__", "__weakref__"}          # what every class statement defines
    own = {b.__name__: set(vars(b)) - implicit for b in bases}              # __init__, __del__, ... count too
    for a, b in itertools.combinations(own, 2):
        assert not own[a] & own[b], f"{a} and {b} both define {sorted(own[a] & own[b])}"
    assert not set(vars(_ffi.Context)) - implicit, "Context itself defines nothing"


# ---- the surface of _ffi ------------------------------------------------------------------------------------------------
def _described(f) -> list:
    return [str(inspect.signature(f)), hashlib.sha256((f.__doc__ or "").encode()).hexdigest()]


def surface(mod) -> dict:
    """The non-dunder names of `mod`; signature and docstring hash of each of the package's functions there and of the
    public methods and properties of each of its public classes."""
    names = sorted(n for n in dir(mod) if not (n.startswith("__") and n.endswith("__")))
    ours = lambda o: getattr(o, "__module__", "").startswith("mcmc_ref_hip")
    classes, functions = {}, {}
    for n in names:
        o = getattr(mod, n)
        if inspect.isfunction(o) and ours(o):
            functions[n] = _described(o)
        elif inspect.isclass(o) and ours(o) and not n.startswith("_"):
            members = {}
            for m in ["__init__"] + [m for m in dir(o) if not m.startswith("_")]:
                v = inspect.getattr_static(o, m, None)
                if isinstance(v, (staticmethod, classmethod)):
                    v = v.__func__
                if inspect.isfunction(v):
                    members[m] = _described(v)
                elif isinstance(v, property):
                    members[m] = ["property"] + _described(v.fget)[1:]
            classes[n] = {"doc": hashlib.sha256((o.__doc__ or "").encode()).hexdigest(), "members": members}
    return {"names": names, "classes": classes, "functions": functions}


# names of the recorded surface that are gone, each with its reason (the submodules are attributes of the package,
# not of _ffi, and section 2's new helpers stay in their units: nothing is new here)
GONE = {
    "_lib": "load_library's cache moved with it to _abi; a re-export would be a stale copy of a rebound global",
    "_lib_lock": "the lock of that cache, moved with it",
    "math": "stdlib module _ffi itself no longer uses; nothing reached it through _ffi",
    "os": "stdlib module _ffi itself no longer uses; nothing reached it through _ffi",
    "time": "stdlib module _ffi itself no longer uses; nothing reached it through _ffi",
    "typing": "stdlib module _ffi itself no longer uses; nothing reached it through _ffi",
    "Path": "pathlib class _ffi itself no longer uses; nothing reached it through _ffi",
}


def test_surface_is_what_it_was():
    from mcmc_ref_hip import _ffi
    was, now = json.loads(SURFACE.read_text()), surface(_ffi)
    assert set(now["names"]) == set(was["names"]) - set(GONE)
    assert now["functions"] == {k: v for k, v in was["functions"].items() if k not in GONE}
    assert now["classes"] == was["classes"]


def test_reexports_are_the_units_objects():
    """Every name `_ffi` imports from a unit is that unit's object, and every unit imports only the units before it, at
    module level."""
    from mcmc_ref_hip import _ffi
    order = ["_abi", "_hostdefs", "_device", "_filecalls", "_statcalls", "_context", "_ffi"]
    units = {u: sys.modules[f"mcmc_ref_hip.{u}"] for u in order}
    for n in json.loads(SURFACE.read_text())["names"]:
        homes = [u for u in order[:-1] if n in vars(units[u]) and not inspect.ismodule(vars(units[u])[n])]
        if n not in GONE and homes:
            assert getattr(_ffi, n) is vars(units[homes[0]])[n], n
    for i, u in enumerate(order):
        later = {f"mcmc_ref_hip.{v}" for v in order[i + 1:]}
        used = {getattr(v, "__module__", None) for v in vars(units[u]).values()} | \
               {v.__name__ for v in vars(units[u]).values() if inspect.ismodule(v)}
        assert not used & later, f"{u} imports from {sorted(used & later)}"
        inner = [n.lineno for f in ast.walk(ast.parse(Path(units[u].__file__).read_text())) if isinstance(f, ast.FunctionDef)
                 for n in ast.walk(f) if isinstance(n, (ast.Import, ast.ImportFrom))]
        assert not inner, f"{u} imports inside a function (lines {inner})"
