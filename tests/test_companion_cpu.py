"""The plumbing the companion libraries share: one handle class, one loader and one handle owner.  `_companion` holds the
Python side (the three mirrors `_iabi`, `_babi`, `_sabi` describe their library to it and bind its loader and handle under
their own names), csrc/mcc_handle.hpp the C++ side (the stream, the events and the two allocations of a handle that stands
alone).  No GPU: the libraries are loaded, never initialised.
"""
from __future__ import annotations

import re
from pathlib import Path

import pytest

from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build)

PKG = Path(__file__).resolve().parents[1] / "mcmc-db_amd"


def companions():
    from mcmc_ref_hip import _babi, _iabi, _sabi
    return ((_iabi.IESS, _iabi.IessHandle, _iabi.load_iess_library, _iabi.ISYMBOLS),
            (_babi.BM, _babi.BmHandle, _babi.load_bm_library, _babi.BSYMBOLS),
            (_sabi.STD, _sabi.StdHandle, _sabi.load_std_library, _sabi.SSYMBOLS))


def test_the_three_handles_are_the_shared_class(built_lib):
    from mcmc_ref_hip import _babi, _companion, batchmeans, indicator, standard
    seen = set()
    for comp, handle, load, symbols in companions():
        assert issubclass(handle, _companion.Handle) and handle is comp.Handle and handle.companion is comp
        assert handle.__init__ is _companion.Handle.__init__ and handle.close is _companion.Handle.close
        assert load == comp.load and comp.symbols is symbols and all(name.startswith(comp.prefix) for name in symbols)
        assert {comp.prefix + n for n in ("init", "free", "last_error", "set_workspace_limit", "profile_enable", "kernel_ms")} <= set(symbols)
        assert load() is load() and load()._name == str(comp.default_path)
        seen.add(handle.__name__)
    assert seen == {"IessHandle", "BmHandle", "StdHandle"}
    assert [m._handle.__self__ for m in (indicator, batchmeans, standard)] == [c[0] for c in companions()]
    assert _babi.host_check == _babi.BM.host_check
    assert [c[0].main_first for c in companions()] == [False, False, True]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["mci_", "mcb_", "mcs_"])
def test_a_missing_library_is_named_with_the_way_to_build_it(built_lib, which, tmp_path, monkeypatch):
    from mcmc_ref_hip import _companion
    from mcmc_ref_hip._abi import HipUnavailableError
    comp, _, load, symbols = companions()[which]
    loaded = load()
    gone = tmp_path / "nowhere" / comp.default_path.name
    other = _companion.Companion(comp.prefix, comp.default_path.name, comp.env, symbols, "Other", "A handle.", comp.main_first)
    monkeypatch.setenv(comp.env, str(gone))
    with pytest.raises(HipUnavailableError) as err:
        other.load()
    assert str(gone) in str(err.value) and "build.py" in str(err.value)
    with pytest.raises(HipUnavailableError):
        other.Handle(0)
    assert load() is loaded and comp._lib is loaded              # the loaded library stays as it is
    monkeypatch.delenv(comp.env)
    assert other.load() is not None and other.default_path == comp.default_path


def test_ffi_knows_nothing_of_the_companions():
    from mcmc_ref_hip import _abi, _companion, _ffi
    assert not [k for k, v in vars(_ffi).items() if v is _companion or getattr(v, "__module__", None) == _companion.__name__]
    assert not re.search(r"\b_companion\b|_[ibs]abi\b", (PKG / "mcmc_ref_hip" / "_ffi.py").read_text())
    imports = re.findall(r"^from \.(\w*) import|^from \. import (\w+)", (PKG / "mcmc_ref_hip" / "_companion.py").read_text(), re.M)
    assert {a or b for a, b in imports} == {"_abi"} and _companion.load_library is _abi.load_library


def test_one_owner_of_streams_events_allocations_and_dlopen():
    src = {p.name: p.read_text() for p in (PKG / "csrc").iterdir() if p.suffix in (".hip", ".hpp")}
    for word in ("hipStreamCreateWithFlags", "hipEventCreate", "hipMalloc"):
        assert word in src["mcc_handle.hpp"], word
        assert word not in src["mci_api.hip"] and word not in src["mcb_api.hip"], word
    for unit in ("mci_api.hip", "mcb_api.hip", "mcs_api.hip"):
        assert '#include "mcc_handle.hpp"' in src[unit], unit
    assert "mcr_ctx" not in src["mcr_carve.hpp"] and "mcr_host.hpp" not in src["mcc_handle.hpp"]
    assert '#include "mcr_carve.hpp"' in src["mcr_host.hpp"] and "struct Carve" not in src["mcr_host.hpp"]
    dlopens = sorted(p.name for p in (PKG / "mcmc_ref_hip").glob("*.py") if "CDLL(" in p.read_text())
    assert dlopens == ["_abi.py", "_companion.py"]
