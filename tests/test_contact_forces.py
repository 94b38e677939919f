"""Contact forces and net wrench of the gelpad (`tacex_fem_contact_forces`, `UipcSim.contact_forces`): the parts that need no GPU - the
symbol through header, library and ctypes table, the argument check, the unchanged ABI version - and the NumPy restatement of the record
(tests/contact_forces_ref.py) pinned on a closed-form case.  The GPU tests compare the kernel with that restatement."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import contact_forces_ref as ref

REPO = Path(__file__).resolve().parents[1]
NAME = "tacex_fem_contact_forces"


def test_symbol_is_declared_exported_and_bound():
    from tacex_amd import _lib

    header = (REPO / "include" / "tacex_hip.h").read_text()
    decl = re.search(r"int\s+tacex_fem_contact_forces\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/tacex_hip.h does not declare tacex_fem_contact_forces"
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params) == 9
    assert args[4] is C.c_int and args[7] is C.c_int  # with_friction, num_envs
    lib = _lib.load_library()
    assert hasattr(lib, NAME) and NAME not in _lib.MISSING_SYMBOLS


def test_null_arguments_are_refused_with_a_message_before_any_hip_call():
    from tacex_amd import _lib

    lib = _lib.load_library()
    assert lib.tacex_fem_contact_forces(None, None, None, None, 0, None, None, 1, None) == 2
    assert NAME.encode() in lib.tacex_last_error()


def test_abi_version_is_unchanged():
    from tacex_amd import _lib

    header = (REPO / "include" / "tacex_hip.h").read_text()
    assert re.search(r"#define\s+TACEX_ABI_VERSION\s+20\b", header)
    assert _lib.ABI_VERSION == 20 and _lib.load_library().tacex_abi_version() == 20


def test_contact_forces_dataclass_views_the_record():
    import torch

    from tacex_amd.uipc.uipc_sim import ContactForces

    rec = torch.arange(32, dtype=torch.float64).reshape(2, 16)
    w = ContactForces(rec)
    for name, sl in ref.SLOTS.items():
        got = getattr(w, name)
        assert torch.equal(got, rec[:, sl]) and got.data_ptr() == rec[:, sl].data_ptr(), name  # views, not copies
    assert torch.equal(w.force, rec[:, 0:3] + rec[:, 3:6]) and w.vertex_forces is None


def _flat_face_case(g):
    """Half-space indenter (solid side above) at uniform gap g over the flat top face of a box pad; vertex weights of the TOP FACE's
    triangles alone, so that they sum to the face area exactly."""
    from oracle.fem_oracle import box_tet_mesh
    from tacex_amd.uipc import UipcObject, UipcObjectCfg

    P, T = box_tet_mesh(4, 5, 2)
    tri = UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T)).surface_triangles()
    top = P[:, 2].max()
    tri = tri[(P[tri][:, :, 2] > top - 1e-12).all(1)]
    a = 0.5 * np.linalg.norm(np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]), axis=1)
    area = np.zeros(len(P))
    np.add.at(area, tri.reshape(-1), np.repeat(a / 3.0, 3))
    ind = np.array([2.0, 0.3, -0.2, top + g, 0.0, 0.0, 0.0, -1.0])
    return P, area, ind, top


def test_record_restatement_on_the_closed_form_half_space_case():
    """Sum f_n = -kappa b'(g / d_hat) / d_hat * (face area) along the indenter's normal; the centre of pressure is the face centroid; the
    torque about it vanishes; area, count and smallest gap are those of the face."""
    from oracle.fem_oracle import barrier

    dhat, kappa, dt, g = 1e-3, 1e7, 0.01, 4e-4
    P, area, ind, top = _flat_face_case(g)
    face = 0.02075 * 0.02525
    np.testing.assert_allclose(area.sum(), face, rtol=1e-13)
    f_n, d = ref.normal_forces(area, ind, dhat, kappa, dt, P)
    centroid = np.array([0.02075 / 2, 0.02525 / 2, top])
    r = ref.wrench_record(P, f_n, np.zeros_like(f_n), area, d, dhat, centroid)
    b1 = float(barrier(g / dhat)[1])
    assert b1 < 0
    F = -kappa * b1 / dhat * face
    np.testing.assert_allclose(r[0:3], F * ind[5:8], rtol=1e-12, atol=1e-12 * F)  # ON the pad: pushed down, away from the solid above
    assert r[2] < 0 and np.all(r[3:6] == 0)
    np.testing.assert_allclose(r[9], F, rtol=1e-12)
    np.testing.assert_allclose(r[10], face, rtol=1e-13)
    assert r[11] == (area > 0).sum() == 6 * 5
    np.testing.assert_allclose(r[12:15], centroid, rtol=0, atol=1e-12 * 0.02525)
    assert np.abs(r[6:9]).max() <= 1e-12 * F * 0.02525
    np.testing.assert_allclose(r[15], g, rtol=1e-12)
    # torque about another point = (centroid - ref) x F
    r2 = ref.wrench_record(P, f_n, np.zeros_like(f_n), area, d, dhat, np.array([0.001, -0.002, 0.03]))
    np.testing.assert_allclose(r2[6:9], np.cross(centroid - np.array([0.001, -0.002, 0.03]), r[0:3]), rtol=0, atol=1e-12 * F * 0.03)
    np.testing.assert_allclose(r2[12:15], centroid, rtol=0, atol=1e-12 * 0.03)


def test_record_restatement_without_contact():
    dhat, kappa, dt = 1e-3, 1e7, 0.01
    P, area, ind, top = _flat_face_case(2e-3)  # beyond d_hat
    f_n, d = ref.normal_forces(area, ind, dhat, kappa, dt, P)
    p0 = np.array([0.1, 0.2, 0.3])
    r = ref.wrench_record(P, f_n, np.zeros_like(f_n), area, d, dhat, p0)
    assert np.all(r[0:12] == 0) and np.array_equal(r[12:15], p0)
    np.testing.assert_allclose(r[15], 2e-3, rtol=1e-12)
    none = np.zeros(8)
    f_n, d = ref.normal_forces(area, none, dhat, kappa, dt, P)
    r = ref.wrench_record(P, f_n, np.zeros_like(f_n), area, d, dhat, p0)
    assert np.all(r[0:12] == 0) and r[15] == np.inf
