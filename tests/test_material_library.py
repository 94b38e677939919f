"""Gel material library, the parts that need no GPU: the cfg class, the C ABI's argument checks that return before any device call, and the
header / binding agreement on the new symbols (tests/test_capi_symbols.py checks every symbol; this pins the three by name)."""
import re

import numpy as np
import pytest


def test_gel_material_cfg_has_the_references_fields_and_defaults():
    from tacex_amd.uipc import GelMaterialCfg, UipcObjectCfg

    m = GelMaterialCfg()
    snh = UipcObjectCfg.StableNeoHookeanCfg()
    assert (m.youngs_modulus, m.poisson_rate, m.mass_density, m.friction_ratio) == (snh.youngs_modulus, snh.poisson_rate, UipcObjectCfg().mass_density, None)
    assert (m.youngs_modulus, m.poisson_rate, m.mass_density) == (0.01, 0.49, 1e3)
    m2 = GelMaterialCfg(youngs_modulus=0.05, friction_ratio=1.0)
    assert m2.youngs_modulus == 0.05 and m2.friction_ratio == 1.0 and GelMaterialCfg().youngs_modulus == 0.01  # (instances do not share state)


def test_material_setters_refuse_a_null_context_without_touching_a_device():
    from tacex_amd import _lib

    lib = _lib.load_library()
    one = np.array([1e4])
    assert lib.tacex_fem_set_material_library(None, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data) == 2
    assert b"tacex_fem_set_material_library" in lib.tacex_last_error()
    assert lib.tacex_fem_set_material_ids(None, None) == 2 and b"tacex_fem_set_material_ids" in lib.tacex_last_error()
    assert lib.tacex_fem_set_material_coarse_inverses(None, 1, one.ctypes.data) == 2
    assert b"tacex_fem_set_material_coarse_inverses" in lib.tacex_last_error()


def test_header_binding_and_flag_agree_on_the_material_library():
    from conftest import REPO
    from tacex_amd import _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    assert int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 19
    lib = _lib.load_library()
    for name in ("tacex_fem_set_material_library", "tacex_fem_set_material_ids", "tacex_fem_set_material_coarse_inverses"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert hasattr(lib, name) and name not in _lib.MISSING_SYMBOLS
    src = (REPO / "tacex_amd" / "csrc" / "fem_device.h").read_text()
    assert re.search(r"kFemFlagBadMaterial\s*=\s*64\b", src) and "flag 64" in hdr  # the next free bit after the mesh library's 32


def test_id_validation_is_host_side():
    """`UipcSim._check_ids` (shared by the mesh and the material library) needs no device."""
    from tacex_amd.uipc.uipc_sim import UipcSim

    class Stub:
        num_envs = 3

    chk = lambda ids, n: UipcSim._check_ids(Stub(), ids, n, "material")  # noqa: E731
    assert chk(None, 2).tolist() == [0, 0, 0] and chk([1, 0, 1], 2).dtype == np.int32
    for bad in ([0, 1], [0, 1, 2], [0, -1, 0], [0.0, 1.0, 0.0]):
        with pytest.raises(ValueError):
            chk(bad, 2)
