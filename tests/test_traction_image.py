"""Contact traction image of the FEM pad (`tacex_traction_image_from_deformed_mesh`, `FemTractionImage`) without a GPU: the C ABI's
declaration and argument checks, and the properties of the NumPy restatement (tests/traction_image_ref.py) the kernel is compared with
bit for bit in tests/test_traction_image_gpu.py - a constant field is reproduced, a linear field is interpolated exactly, the image
integrates to the forces put in, and the winner of a pixel does not depend on the order two triangles are listed in."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from conftest import REPO
from traction_image_ref import F, camera_frame_f32, project, render, tilt_and_dent, vertex_tractions

CAM = (0.010375, 0.012625, -0.024)  # the pad centre, 24 mm behind the back face (z = 0), optical axis +z
CLIP = (0.024, 0.029)
# 80 x 40: 2 x 2 tiles of 64 x 32, the right tile 16 columns wide, the bottom tile 8 rows high; the pad covers 77.5 % of either image
SIZES = {(320, 240): (340.0, 325.0, 160.0, 125.0), (80, 40): (85.0, 54.2, 40.0, 20.8)}
NAME = "tacex_traction_image_from_deformed_mesh"


# -- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_lists_the_function():
    from tacex_amd import _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", code)
    lib = _lib.load_library()
    assert hasattr(lib, NAME) and _lib.MISSING_SYMBOLS == []
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 22
    assert int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 20 == lib.tacex_abi_version() == _lib.ABI_VERSION


def test_abi_rejects_bad_arguments_without_a_gpu():
    from tacex_amd import _lib

    lib = _lib.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    good = dict(x=p, V=8, ids=p, Vs=4, tris=p, T=2, force=p, area=p, pos=p, rot=p, fx=340.0, fy=325.0, cx=160.0, cy=125.0, near=0.024,
                far=0.029, traction=p, depth=p, B=1, H=8, W=8)

    def call(**kw):
        a = {**good, **kw}
        return getattr(lib, NAME)(a["x"], a["V"], a["ids"], a["Vs"], a["tris"], a["T"], a["force"], a["area"], a["pos"], a["rot"], a["fx"],
                                  a["fy"], a["cx"], a["cy"], a["near"], a["far"], a["traction"], a["depth"], a["B"], a["H"], a["W"], None)

    for k in ("x", "ids", "tris", "force", "area", "pos", "rot", "traction"):
        assert call(**{k: None}) == 2 and b"null" in lib.tacex_last_error() and NAME.encode() in lib.tacex_last_error()
    for k in ("V", "Vs", "T", "B", "H", "W"):
        assert call(**{k: 0}) == 2 and b"counts" in lib.tacex_last_error()
        assert call(**{k: -3}) == 2
    assert call(Vs=9) == 2 and b"counts" in lib.tacex_last_error()  # more surface vertices than the mesh has
    for near, far in ((0.029, 0.024), (0.024, 0.024), (-0.001, 0.029), (float("nan"), 0.029)):
        assert call(near=near, far=far) == 2 and b"clipping" in lib.tacex_last_error()
    # a null depth with a bad count: the count is what is refused (depth_m_dev is optional)
    assert call(depth=None, T=0) == 2 and b"counts" in lib.tacex_last_error()


def test_the_class_is_exported():
    import tacex_amd
    from tacex_amd.simulation_approaches.fem_based import ManiSkillSimulator
    from tacex_amd.simulation_approaches.fem_based.sim import VisionTactileSensorUIPC

    assert "FemTractionImage" in tacex_amd.__all__ and tacex_amd.FemTractionImage.__module__ == "tacex_amd.height_map_source"
    assert callable(VisionTactileSensorUIPC.traction_image) and callable(ManiSkillSimulator.traction_image)


# -- properties of the reference ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pad():
    """The C4 pad: points, contact-face vertex ids, face triangles over those ids, barrier vertex areas."""
    from tacex_amd.height_map_source import contact_face_triangles
    from tacex_amd.uipc.uipc_object import UipcObject, UipcObjectCfg, gelpad_box_mesh

    P, T = gelpad_box_mesh(8, 10, 4)
    tri = contact_face_triangles(P, T, [0.0, 0.0, 1.0])
    ids, local = np.unique(tri.reshape(-1), return_inverse=True)
    area = UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T)).surface_vertex_areas()
    return P, ids, local.reshape(-1, 3), area


def _render(x_face, tau, res, dtype=F):
    W, H = res
    pc = camera_frame_f32(x_face, CAM, np.eye(3))
    return pc, render(pc, _pad()[2], tau, *SIZES[res], CLIP[0], CLIP[1], H, W, dtype)


def _constant_field_ulp(res):
    P, ids, _, _ = _pad()
    c = np.array([3.0, -2.0, 7.0], F)
    _, (depth, winner, img) = _render(tilt_and_dent(P)[ids], np.tile(c, (len(ids), 1)), res)
    seen = winner >= 0
    assert 0.75 < seen.mean() < 0.80 and (img[~seen] == 0).all() and np.isinf(depth[~seen]).all()
    assert depth[seen].min() < 0.0285 - 3e-4 and depth[seen].max() > 0.0285 + 1.5e-4  # dented and tilted
    return float((np.abs(img[seen] - c) / np.spacing(np.abs(c))).max())


LIN_A = np.array([[200.0, -100.0, 50.0], [-80.0, 120.0, 30.0], [60.0, 90.0, -40.0]])
LIN_B = np.array([1.0, -2.0, 3.0])


def _linear_field_error(res):
    """max |image - field(back-projected pixel)| / max |field|, for the float32 image and for the float64 interpolation of the same
    float32 projections."""
    P, ids, _, _ = _pad()
    W, H = res
    fx, fy, cx, cy = SIZES[res]
    pc = camera_frame_f32(P[ids], CAM, np.eye(3))
    tau = (pc.astype(np.float64) @ LIN_A.T + LIN_B).astype(F)
    errs = []
    for dtype in (F, np.float64):
        _, (depth, winner, img) = _render(P[ids], tau, res, dtype)
        i, j = np.nonzero(winner >= 0)
        z = depth[i, j].astype(np.float64)
        p = np.stack([(j + 0.5 - cx) / fx * z, (i + 0.5 - cy) / fy * z, z], 1)
        errs.append(float(np.abs(img[i, j] - (p @ LIN_A.T + LIN_B)).max() / np.abs(tau).max()))
    return tuple(errs)


def _integral_error(res):
    """Relative error of sum_px t_z z^2 / (fx fy) against the sum of the vertex forces of a cos^2 pressure bump on the flat face."""
    P, ids, tris, area = _pad()
    fx, fy, _, _ = SIZES[res]
    face = P[ids]
    r = np.hypot(face[:, 0] - CAM[0], face[:, 1] - CAM[1])
    interior = (face[:, 0] > 0) & (face[:, 0] < P[:, 0].max()) & (face[:, 1] > 0) & (face[:, 1] < P[:, 1].max())
    # (the barrier's area of an interior face vertex is a third of its six face triangles: the integral of its hat function)
    f = np.zeros((len(ids), 3))
    on = interior & (r < 0.006)
    f[on, 2] = -2.0e4 * area[ids][on] * np.cos(np.pi * r[on] / 0.012) ** 2
    assert on.sum() >= 12
    _, (depth, winner, img) = _render(face, vertex_tractions(f, area[ids], np.eye(3)), res)
    seen = winner >= 0
    got = float((img[seen][:, 2].astype(np.float64) * depth[seen].astype(np.float64) ** 2).sum() / (fx * fy))
    return abs(got / f[:, 2].sum() - 1.0)


# Figures of this reference (NumPy float32, every operation rounded), measured once; the tests hold it to them.
CONSTANT_ULP = {(320, 240): 3.0, (80, 40): 2.0}           # measured: 3 and 2 ulp; bound: + 1 ulp
LINEAR_REL = {(320, 240): 1.97e-7, (80, 40): 1.49e-7}     # measured (float32 image); bound: x 4
INTEGRAL_REL = {(320, 240): 4.97e-5, (80, 40): 1.42e-3}   # measured (pixel quadrature of a piecewise linear image); bound: x 4


@pytest.mark.parametrize("res", list(SIZES))
def test_constant_field_is_reproduced(res):
    ulp = _constant_field_ulp(res)
    print(f"constant field {res}: {ulp} ulp")
    assert ulp <= CONSTANT_ULP[res] + 1.0


@pytest.mark.parametrize("res", list(SIZES))
def test_linear_field_is_interpolated_at_the_back_projected_point(res):
    e32, e64 = _linear_field_error(res)
    print(f"linear field {res}: float32 {e32:.3g}, float64 interpolation {e64:.3g} of the largest magnitude")
    assert e32 <= 4.0 * LINEAR_REL[res]
    # the float64 interpolation of the same float32 projections and vertex values is no further off: the error is the rounding of those
    # inputs (measured: 1.8e-7 and 1.5e-7), not of the interpolation's own float32 operations
    assert e64 <= 4.0 * LINEAR_REL[res]


@pytest.mark.parametrize("res", list(SIZES))
def test_image_integrates_to_the_vertex_forces(res):
    e = _integral_error(res)
    print(f"integral {res}: relative error {e:.3g}")
    assert e <= 4.0 * INTEGRAL_REL[res]


def test_shared_edge_through_pixel_centres_goes_to_the_lower_index():
    """Two coplanar triangles (z = 1) whose shared edge is the column of pixel centres x = 4.5: both give a fragment there.  Coordinates
    are binary fractions and the areas powers of two, so every operation is exact and the two fragments' z are equal bit for bit."""
    pc = np.array([[0.5 / 8, 4.5 / 8, 1.0], [4.5 / 8, 0.5 / 8, 1.0], [4.5 / 8, 8.5 / 8, 1.0], [8.5 / 8, 4.5 / 8, 1.0]], F)
    tau = np.array([[1.0, 0.0, 5.0], [2.0, -1.0, 6.0], [3.0, 4.0, 7.0], [-2.0, 8.0, 9.0]], F)
    t_left, t_right = [0, 1, 2], [1, 3, 2]
    args = (8.0, 8.0, 0.0, 0.0, 0.5, 2.0, 10, 10)
    sx, sy, _, _ = project(pc, 8.0, 8.0, 0.0, 0.0)
    np.testing.assert_array_equal(sx, [0.5, 4.5, 4.5, 8.5])
    z_left, _, _ = render(pc, [t_left], tau, *args)
    z_right, _, _ = render(pc, [t_right], tau, *args)
    tie = np.isfinite(z_left) & np.isfinite(z_right) & (z_left.view(np.uint32) == z_right.view(np.uint32))
    assert tie[:, 4].sum() == 9 and tie.sum() == 9  # the pixel centres (4.5, 0.5 ... 8.5)
    d0, w0, img0 = render(pc, [t_left, t_right], tau, *args)
    d1, w1, img1 = render(pc, [t_right, t_left], tau, *args)
    assert (w0[tie] == 0).all() and (w1[tie] == 0).all()  # the lower index, whichever triangle carries it
    only_left = np.isfinite(z_left) & ~np.isfinite(z_right)
    assert (w0[only_left] == 0).all() and (w1[only_left] == 1).all()
    np.testing.assert_array_equal(d0, d1)
    np.testing.assert_array_equal(img0, img1)
    np.testing.assert_array_equal(img0[4, 4], [2.5, 1.5, 6.5])  # the midpoint of the shared edge
