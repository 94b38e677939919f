"""Contact force field on the CPU: the ABI (symbol, refusals before any GPU call), the Python layer's argument checks, the NumPy
restatement (tests/contact_field_ref.py) against closed forms of sphere and cylinder contact, and the vetting of the GPU tests' input
frames (few pixels whose stick / slip decision is borderline)."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from conftest import REPO
from contact_field_ref import (GELS, borderline_pixels, case_batch, case_pixmm, case_slip, contact_frame, cylinder_map, frame_scalars, gel_row,
                               indentation_depth, sphere_map)

PIXMM = 0.0295
SPHERES = [(240, 320, 60, 0.5, 160.3, 120.7), (48, 64, 20, 0.25, 30.2, 22.9), (37, 53, 14, 0.2, 25.4, 17.6)]  # H, W, R px, d mm, cx, cy


def _lib_and_module():
    from tacex_amd import _lib

    return _lib.load_library(), _lib


def test_symbol_declared_exported_and_bound():
    lib, _lib = _lib_and_module()
    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"tacex_contact_field\s*\(([^)]*)\)", txt)
    assert decl, "tacex_contact_field is not declared in include/tacex_hip.h"
    assert hasattr(lib, "tacex_contact_field") and "tacex_contact_field" in _lib.SIGNATURES
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["tacex_contact_field"][1]) == 18
    assert lib.tacex_abi_version() == int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 20


def test_the_translation_unit_is_built_without_fp_contraction():
    from tacex_amd import _build

    assert "contact_field.hip" in _build.SOURCES and (REPO / "tacex_amd" / "csrc" / "contact_field.hip").exists()
    assert "-ffp-contract=off" in _build.FILE_FLAGS["contact_field.hip"]


def test_exported_from_the_package():
    import tacex_amd

    assert {"ContactField", "ContactGel", "TactileContactModel", "slip_from_fots"} <= set(tacex_amd.__all__)
    assert tacex_amd.TactileContactModel.__module__ == "tacex_amd.contact_field"
    assert hasattr(tacex_amd.GelSightSensor, "contact_field")
    for name in ("normal_force", "friction_force", "torque", "centre_of_pressure", "contact_area", "max_penetration", "volume", "num_contact",
                 "num_slipping", "slip_ratio", "patch_angle", "patch_aspect"):
        assert isinstance(getattr(tacex_amd.ContactField, name), property), name


# arguments of a valid call (the pointers are never dereferenced: every case below is refused before any GPU call)
_OK = dict(hm=0x1000, fmin=0x2000, ind=0x3000, gels=0x4000, P=1, ids=None, slip=None, pixmm=0.03, rects=None, rows=2, cols=3, rec=0x5000,
           cells=0x6000, img=None, B=1, H=4, W=8)


@pytest.mark.parametrize("change, word", [
    (dict(hm=None), b"hm_mm_dev"), (dict(fmin=None), b"frame_min_dev"), (dict(ind=None), b"indent_mm_dev"), (dict(gels=None), b"gels_dev"),
    (dict(rec=None), b"record_dev"), (dict(P=0), b"num_gels"), (dict(P=-2), b"num_gels"),
    (dict(B=0), b"num_frames"), (dict(B=-1), b"num_frames"), (dict(H=0), b"height"), (dict(W=0), b"width"), (dict(W=-5), b"width"),
    (dict(pixmm=0.0), b"pixmm"), (dict(pixmm=-0.03), b"pixmm"), (dict(pixmm=float("nan")), b"pixmm"),
    (dict(rows=0), b"grid_rows"), (dict(rows=5), b"grid_rows"), (dict(cols=0), b"grid_cols"), (dict(cols=9), b"grid_cols"),
    (dict(cols=9, cells=None), b"grid_cols"),
    (dict(H=8, W=20000, cols=1), b"LDS"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_return_2_and_name_the_argument(change, word):
    lib, _lib = _lib_and_module()
    a = dict(_OK, **change)
    rc = lib.tacex_contact_field(a["hm"], a["fmin"], a["ind"], a["gels"], a["P"], a["ids"], a["slip"], a["pixmm"], a["rects"], a["rows"], a["cols"],
                                 a["rec"], a["cells"], a["img"], a["B"], a["H"], a["W"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_contact_field" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "tacex_contact_field")


def test_contact_gel_and_model_argument_checks():
    from tacex_amd import ContactGel, TactileContactModel
    from tacex_amd._lib import TacexHipError

    row = ContactGel(3e4, 1.2e4, 0.6).row()
    assert row.dtype == np.float32 and row.shape == (4,) and row[3] == 0
    np.testing.assert_array_equal(row, gel_row(3e4, 1.2e4, 0.6))
    np.testing.assert_array_equal(ContactGel(5.0).row(), gel_row(5.0))
    for bad in (dict(k_n=-1.0), dict(k_n=1.0, k_t=-2.0), dict(k_n=1.0, mu=-0.1), dict(k_n=float("nan")), dict(k_n=1.0, k_t=float("inf")),
                dict(k_n=1e39)):
        with pytest.raises(ValueError):
            ContactGel(**bad).row()
    # the elastic-foundation moduli of a bonded layer, in Pa/mm
    E, v, h = 1.2e5, 0.45, 0.0045
    g = ContactGel.from_material(E, v, h, mu=0.7)
    assert g.k_n == pytest.approx(E * (1 - v) / ((1 + v) * (1 - 2 * v) * h) * 1e-3, rel=1e-12)
    assert g.k_t == pytest.approx(E / (2 * (1 + v) * h) * 1e-3, rel=1e-12) and g.mu == 0.7
    assert ContactGel.from_material(1e5, 0.0, 0.002).k_n == pytest.approx(1e5 / 0.002 * 1e-3)
    for nu in (0.5, 0.6):
        with pytest.raises(ValueError, match="directly"):
            ContactGel.from_material(E, nu, h)
    for bad in ((E, v, 0.0), (-1.0, v, h), (E, -1.0, h), (E, float("nan"), h)):
        with pytest.raises(ValueError):
            ContactGel.from_material(*bad)
    one = [ContactGel(1.0)]
    with pytest.raises(ValueError):
        TactileContactModel([], 2, "cuda")
    with pytest.raises(ValueError):
        TactileContactModel([np.zeros(4)], 2, "cuda")
    with pytest.raises(ValueError):
        TactileContactModel(one, 0, "cuda")
    with pytest.raises(ValueError):
        TactileContactModel(one, 2, "cuda", pixmm=0.0)
    with pytest.raises(ValueError):
        TactileContactModel(one, 2, "cuda", grid=(0, 3))
    with pytest.raises(TacexHipError):  # no CPU path
        TactileContactModel(one, 2, "cpu")


def test_slip_from_fots_reads_the_trajectory_state():
    """[len, x0, y0, th0, xl, yl, thl, n] with centroids in mm from the image centre -> [dx, dy, dtheta, cx_px, cy_px]; torch ops only."""
    from tacex_amd import slip_from_fots

    traj = torch.tensor([[3, 0.5, -0.25, 0.1, 0.75, 0.25, 0.3, 12], [0, 9, 9, 9, 9, 9, 9, 0], [1, -1.0, 2.0, -0.2, -1.0, 2.0, -0.2, 4]], dtype=torch.float32)
    sim = SimpleNamespace(_traj_state=traj, cfg=SimpleNamespace(tactile_img_res=(320, 240), mm_to_pixel=20.0))
    slip = slip_from_fots(sim)
    assert slip.dtype == torch.float32 and tuple(slip.shape) == (3, 5) and slip.is_contiguous()
    want = torch.tensor([[0.25, 0.5, 0.3 - 0.1, 0.75 * 20 + 160, 0.25 * 20 + 120], [0, 0, 0, 0, 0], [0, 0, 0, -20.0 + 160, 40.0 + 120]])
    assert torch.allclose(slip, want, rtol=0, atol=1e-6)
    assert torch.equal(slip[1], torch.zeros(5))


# ---- the restatement against closed forms ----------------------------------------------------------------------------------------
KN, KT, MU = 3.0e4, 1.2e4, 0.6


def _sphere(H, W, R, d, cx, cy, slip=None, kt=KT, grid=(1, 1)):
    hm = sphere_map(H, W, R, d, cx, cy, PIXMM, dtype=np.float32)
    fmin, ind = frame_scalars(hm)
    return contact_frame(hm, fmin, ind, gel_row(KN, kt, MU), slip, PIXMM, grid)


@pytest.mark.parametrize("H, W, R, d, cx, cy", SPHERES)
def test_sphere_volume_force_and_centre_of_pressure(H, W, R, d, cx, cy):
    rec, cells, image, _ = _sphere(H, W, R, d, cx, cy, grid=(3, 4))
    cap = np.pi * d * d * (3 * R * PIXMM - d) / 3
    print(f"volume {rec[12]:.6f} mm^3, cap {cap:.6f}, rel {rec[12] / cap - 1:+.2e}; Fn {rec[6]:.6f} N; cop ({rec[9]:.4f}, {rec[10]:.4f}); aspect {rec[15]:.4f}")
    assert abs(rec[12] / cap - 1) < 1e-3
    assert rec[6] == pytest.approx(KN * rec[12] * 1e-6, rel=1e-6)
    assert abs(rec[9] - cx) < 0.01 and abs(rec[10] - cy) < 0.01
    # the deepest pixel lies within sqrt(0.5) px of the apex: r^2 / (2 R) px below it, to first order (0.6 / R covers the next order)
    assert d - 0.6 / R * PIXMM <= rec[11] <= d * (1 + 1e-6) and rec[15] > 0.95
    assert rec[0] == rec[1] == rec[5] == rec[13] == 0  # no slip table: no shear, and nothing slips while mu p > 0
    assert rec[7] == pytest.approx(rec[8] * (PIXMM * 1e-3) ** 2, rel=1e-6)
    # the torque of a pure pressure is the lever of its centre times the normal force on the pad (0, 0, -Fn)
    m = PIXMM * 1e-3
    assert rec[3] == pytest.approx((rec[10] - (H - 1) / 2) * m * -rec[6], rel=1e-6, abs=1e-12)
    assert rec[4] == pytest.approx((rec[9] - (W - 1) / 2) * m * rec[6], rel=1e-6, abs=1e-12)
    np.testing.assert_allclose(cells.sum(axis=(0, 1)), rec[0:3], rtol=1e-12, atol=0)
    assert (image[..., 2] <= 0).all() and image[..., 2].min() == pytest.approx(-KN * rec[11], rel=1e-6)


@pytest.mark.parametrize("H, W, R, d, cx, cy", SPHERES)
def test_sphere_gross_slip_and_stick(H, W, R, d, cx, cy):
    # pure translation, stiff in shear: every contact pixel is on the cone, |F_t| = mu Fn along the motion
    rec, _, _, _ = _sphere(H, W, R, d, cx, cy, slip=[0.03, -0.04, 0.0, cx, cy], kt=1e9)
    ft = np.hypot(rec[0], rec[1])
    print(f"gross slip: {rec[13]:.0f} of {rec[8]:.0f} slip, |F_t| / (mu Fn) - 1 = {ft / (MU * rec[6]) - 1:+.2e}")
    assert rec[13] == rec[8] > 0
    assert ft == pytest.approx(MU * rec[6], rel=1e-6)
    assert rec[0] / ft == pytest.approx(0.6, rel=1e-6) and rec[1] / ft == pytest.approx(-0.8, rel=1e-6)
    # a small translation: nothing slips, the shear is the elastic one, F_t = k_t u area
    u = np.array([6e-10, -8e-10])
    rec, _, _, _ = _sphere(H, W, R, d, cx, cy, slip=[u[0], u[1], 0.0, cx, cy])
    print(f"stick: {rec[13]:.0f} slip, F_t / (k_t u A) - 1 = {rec[0] / (KT * u[0] * rec[7]) - 1:+.2e}, {rec[1] / (KT * u[1] * rec[7]) - 1:+.2e}")
    assert rec[13] == 0
    np.testing.assert_allclose(rec[0:2], KT * u * rec[7], rtol=1e-6)


@pytest.mark.parametrize("dth", [0.2, -0.2])
@pytest.mark.parametrize("H, W, R, d, cx, cy", SPHERES)
def test_sphere_twist_at_full_slip(H, W, R, d, cx, cy, dth):
    rec, _, _, _ = _sphere(H, W, R, d, cx, cy, slip=[0.0, 0.0, dth, cx, cy], kt=1e9)
    ft = np.hypot(rec[0], rec[1])
    print(f"twist {dth:+}: {rec[13]:.0f} of {rec[8]:.0f} slip, |F_t| / (mu Fn) = {ft / (MU * rec[6]):.2e}, torque z {rec[5]:+.3e} N m")
    assert rec[13] >= rec[8] - 1  # (a pixel exactly at the centre of rotation does not move)
    assert ft < 0.005 * MU * rec[6]
    assert np.sign(rec[5]) == np.sign(dth) and abs(rec[5]) > 0


@pytest.mark.parametrize("deg", [0, 30, 90])
def test_cylinder_patch_angle(deg):
    H, W = 240, 320
    hm = cylinder_map(H, W, 40, 0.3, 158.6, 121.2, np.deg2rad(deg), 70, PIXMM, dtype=np.float32)
    fmin, ind = frame_scalars(hm)
    rec, _, _, _ = contact_frame(hm, fmin, ind, gel_row(KN, KT, MU), None, PIXMM)
    diff = (rec[14] - np.deg2rad(deg) + np.pi / 2) % np.pi - np.pi / 2
    print(f"cylinder at {deg} deg: angle {np.rad2deg(rec[14]):.3f} deg, aspect {rec[15]:.4f}")
    assert abs(diff) < 0.02 and rec[15] < 0.5 and rec[8] > 1000


# ---- the GPU tests' inputs, vetted here --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(24, 32), (37, 53), (48, 64), (240, 320)])
def test_gpu_case_frames_have_few_borderline_pixels(H, W):
    """The kernel's stick / slip count may differ from the restatement's by the pixels whose k_t n and mu p agree to 1e-5 relative
    (a 1-ulp difference decides them); the inputs keep those under 0.5 % of the contact pixels, for every gel and slip row."""
    hm, kinds = case_batch(H, W, 10)
    fmin, ind = indentation_depth(hm)
    slips = case_slip(4, H, W)
    assert (ind[[k != "none" for k in kinds]] > 0).all() and ind[kinds.index("none")] == 0
    for b, kind in enumerate(kinds):
        for gel in GELS:
            for slip in slips:
                nb, nc = borderline_pixels(hm[b], fmin[b], ind[b], gel, slip, case_pixmm(H))
                assert nb <= 0.005 * nc, (kind, gel, slip, nb, nc)
                assert (nc == 0) == (kind == "none") and (nc == H * W) == (kind == "full")
