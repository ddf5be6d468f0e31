"""CPU-only tests of how csrc/ is cut into translation units (mcmc-db_amd/build.py: UNITS), read from what the build
leaves in lib/obj: the summary unit and the statistics unit do not see each other's kernel headers, the file and comm
units see neither group, and every kernel belongs to one unit."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_host_cpu import built_lib  # noqa: F401  (the fixture: an up-to-date build)

HOT_PATH = {"mcr_kernels.hpp", "mcr_diag.hpp", "mcr_fft.hpp", "mcr_sortnet.h"}
STATISTICS = {"mcr_ext.hpp", "mcr_energy.hpp", "mcr_nested.hpp", "mcr_acf.hpp", "mcr_pareto.hpp", "mcr_psis.hpp", "mcr_hdi.hpp",
              "mcr_weighted.hpp", "mcr_sbc.hpp"}
# what each unit's dependency file must not name
FORBIDDEN = {"mcr_api": STATISTICS, "mcr_stats": HOT_PATH, "mcr_files": HOT_PATH | STATISTICS, "mcr_comm": HOT_PATH | STATISTICS}


@pytest.fixture(scope="module")
def build_mod(built_lib):  # noqa: F811
    import importlib.util
    spec = importlib.util.spec_from_file_location("mcr_build", built_lib.parents[1] / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_units_include_only_their_side_of_the_seam(build_mod):
    assert set(build_mod.UNITS) == set(FORBIDDEN)
    csrc = build_mod.HERE / "csrc"
    for header in HOT_PATH | STATISTICS:
        assert (csrc / header).is_file(), header
    for unit, forbidden in FORBIDDEN.items():
        deps = {Path(f).name for f in build_mod.dep_files(build_mod.OBJ / f"{unit}.d")}
        assert f"{unit}.hip" in deps and "mcr_host.hpp" in deps        # the file is this unit's, and it is complete
        assert not deps & forbidden, f"{unit} includes {sorted(deps & forbidden)}"
    # the two statistics units do include their own side
    assert HOT_PATH <= {Path(f).name for f in build_mod.dep_files(build_mod.OBJ / "mcr_api.d")}
    assert STATISTICS <= {Path(f).name for f in build_mod.dep_files(build_mod.OBJ / "mcr_stats.d")}


def test_every_kernel_is_defined_in_one_unit(build_mod):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not on the path")
    owner: dict[str, str] = {}
    for unit in build_mod.UNITS:
        out = subprocess.run([nm, "--defined-only", "--demangle", str(build_mod.OBJ / f"{unit}.o")], check=True,
                             capture_output=True, text=True).stdout
        # a kernel's host-side symbols: its handle and its launch stub, k_* in mcr or a namespace inside it (template arguments dropped)
        kernels = set(re.findall(r"\b(mcr::(?:\w+::)*?)(?:__device_stub__)?(k_\w+)[<(]", out))
        for ns, name in kernels:
            assert owner.setdefault(ns + name, unit) == unit, f"{ns}{name} is defined in {owner[ns + name]} and in {unit}"
    units = set(owner.values())
    assert units == {"mcr_api", "mcr_stats", "mcr_files"}, units       # (the communicator has no kernel)
    assert owner["mcr::k_tile_sort"] == "mcr_api" and owner["mcr::fft::k_fft_twiddles"] == "mcr_api"
    assert owner["mcr::k_psis_column"] == "mcr_stats" and owner["mcr::k_moments_rows"] == "mcr_api"
