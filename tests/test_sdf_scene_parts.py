"""The owner of a hit on the CPU: the NumPy restatement of `tacex_height_map_from_sdf_scene_parts` (tests/sdf_scene_parts_ref.py)
against the plain restatement (the height maps keep their bits) and against the float64 closed form of analytic constructive solid
geometry (which solid's surface one sees); `part_slip`'s known answers; the C ABI's argument checks (no GPU call is made) and the host
layer's refusals."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import sdf_scene_parts_ref as P
import sdf_scene_ref as S
import test_sdf_scene as T  # its analytic cases, grids and interpolation error
import test_volume_source as TV
import volume_source_ref as V
from conftest import REPO

F32 = np.float32
NEAR, FAR, TOL = S.NEAR, S.FAR, S.TOL
SHAPES = [(24, 32), (30, 40), (9, 4)]
NAME = "tacex_height_map_from_sdf_scene_parts"


@functools.lru_cache(maxsize=None)
def _library():
    return S.library(S.three_volumes())


@functools.lru_cache(maxsize=None)
def restated(H, W, K, max_steps):
    """(height map, owner) of `gpu_scene` - shared with tests/test_sdf_scene_parts_gpu.py, read-only."""
    ids, ops, pose = S.gpu_scene(H, W, K)
    out = P.height_and_part_map(*_library(), ids, pose, ops, H, W, S.scene_pixmm(H, W), NEAR, FAR, max_steps, TOL)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the restatement against the plain one ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", [1, 8, 32])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_height_maps_keep_the_plain_restatements_bits(H, W, K, max_steps):
    ids, ops, pose = S.gpu_scene(H, W, K)
    want = S.height_map(*_library(), ids, pose, ops, H, W, S.scene_pixmm(H, W), NEAR, FAR, max_steps, TOL)
    hm, owner = restated(H, W, K, max_steps)
    assert np.array_equal(hm.view(np.uint32), want.view(np.uint32))
    far = hm == F32(FAR)
    assert owner.dtype == np.uint8 and np.array_equal(owner == P.NO_OWNER, far)  # 255 exactly where the map is at the far clip
    assert (owner[~far] < K).all()


def test_every_kind_of_slot_owns_pixels():
    """24 x 32, K = 8, 32 steps: hard union, blended union, subtract, blended subtract, intersect and blended intersect each own at
    least 10 pixels in some env (12, 28, 39, 64, 110 and 391 when the scene was laid out)."""
    H, W, K = 24, 32, 8
    ids, ops, pose = S.gpu_scene(H, W, K)
    counts = P.owner_kinds(restated(H, W, K, 32)[1], ops, pose)
    print(dict(zip(P.KINDS, counts.max(0).tolist())))
    assert (counts.max(0) >= 10).all(), dict(zip(P.KINDS, counts.max(0).tolist()))


# ---- the restated owner against the closed form ---------------------------------------------------------------------------------------
# The cases of tests/test_sdf_scene.py: the union of two spheres and the box minus a sphere, aligned and rotated.  Its "box and sphere"
# intersection leaves 9 % of its pixels undecided at the margin below (the crease between the box's near face and the sphere runs along
# a 3 mm circle, and the box grid's interpolation error, 0.0525 mm, is that of its corners): an intersection of two of its spheres - a
# lens - stands in for it, on the same grids and helpers.
H, W, PIX, CX, CY = T.H, T.W, T.PIX, T.CX, T.CY
LENS = "lens of two spheres"
OWNER_CASES = [c for c in range(len(T.CASES)) if T.CASES[c][0] in (0, 1)] + [(LENS, False), (LENS, True)]


def _case_parts(case):
    if isinstance(case, int):
        return T._parts(case)
    Rs = [V.quat_matrix(q) if case[1] else np.eye(3) for q in T.GRID_TURNS]
    return [("sphere", S.UNION, Rs[0], np.array([CX - 0.5, CY, 29.6]), 0.7, 0.0),
            ("sphere", S.INTERSECT, Rs[1], np.array([CX + 0.5, CY + 0.2, 29.5]), 0.6, 0.0)]


@functools.lru_cache(maxsize=None)
def _closed_form_owner(case):
    """In float64, per pixel: (the slot whose surface one sees, -1 where one sees none; undecided: the two nearest candidate depths
    differ by no more than the margin).  Along a ray two slots' exact fields differ by at least slope x (the gap of their candidate
    depths), slope the smaller |n_z| of the two surfaces, and each tapped field is within E (the grids' interpolation error, the one
    tests/test_sdf_scene.py uses) + tol of the exact one where the ray stops: the comparison inside smin is decided when
    gap > 2 (E + tol) / slope."""
    parts = _case_parts(case)
    kind = T.CASES[case][0] if isinstance(case, int) else 2
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X, Y = (x * PIX).reshape(-1), (y * PIX).reshape(-1)
    E = max(TV._interpolation_error(name, 0.0) * scale for name, _, _, _, scale, _ in parts)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind in (0, 2):  # two spheres: the nearer entry of a union, the later entry of an intersection (before the earlier exit)
            (_, _, _, ca, sa, _), (_, _, _, cb, sb, _) = parts
            ra, rb = T.SPHERE_R * sa, T.SPHERE_R * sb
            (za, xa), (zb, xb) = T._sphere_span(X, Y, ca, ra), T._sphere_span(X, Y, cb, rb)
            if kind == 0:
                seen = ~np.isnan(za) | ~np.isnan(zb)
                owner = np.where(~np.isnan(za) & (np.isnan(zb) | (za <= zb)), 0, 1)
            else:
                seen = ~np.isnan(za) & ~np.isnan(zb) & (np.fmax(za, zb) < np.fmin(xa, xb))
                owner = np.where(zb > za, 1, 0)
            z = np.where(owner == 0, za, zb)
            gap, slope = np.abs(za - zb), np.minimum((ca[2] - za) / ra, (cb[2] - zb) / rb)
        else:  # box minus sphere: the box's entry face, or the far wall of the ball where the entry lies in the ball
            (_, _, Rb, tb, sb, _), (_, _, _, cs, ss, _) = parts
            b1, b2, axis = T._box_span(X, Y, Rb, tb, 0.5 * T.BOX_SIZE * sb)
            rs = T.SPHERE_R * ss
            s1, s2 = T._sphere_span(X, Y, cs, rs)
            in_ball = ~np.isnan(s1) & (s1 <= b1) & (b1 < s2)
            z = np.where(in_ball, np.where(s2 < b2, s2, np.nan), b1)
            seen, owner = ~np.isnan(z), np.where(in_ball, 1, 0)
            gap = np.fmin(np.abs(b1 - s1), np.abs(b1 - s2))
            slope = np.minimum(np.abs(Rb[2])[axis], np.fmin(np.abs(cs[2] - s1), np.abs(s2 - cs[2])) / rs)
        seen = seen & (z < FAR)
        undecided = seen & ~np.isnan(gap) & ~(gap > 2.0 * (E + TOL) / slope)
    return np.where(seen, owner, -1).reshape(H, W), undecided.reshape(H, W)


@functools.lru_cache(maxsize=None)
def _restated_case(case):
    parts = _case_parts(case)
    names = ("sphere", "box")
    vox, vi, vf = V.library([(TV._volume(n).sdf_mm, T.PITCH, None, 1.0) for n in names])
    ids = np.array([[names.index(p[0]) for p in parts]], np.int32)
    ops = np.array([[p[1] for p in parts]], np.int32)
    pose = np.stack([S.scene_row(p[2], p[3], p[4], 0.0, p[5]) for p in parts])[None]
    hm, owner = P.height_and_part_map(vox, vi, vf, ids, pose, ops, H, W, PIX, NEAR, FAR, 32, TOL)
    return hm[0], owner[0]


@pytest.mark.parametrize("case", OWNER_CASES, ids=lambda c: f"{T.KINDS[T.CASES[c][0]]}-{T.CASES[c][1]}" if isinstance(c, int) else f"{c[0]}-{c[1]}")
def test_restated_owner_against_the_closed_form(case):
    want, undecided = _closed_form_owner(case)
    seen = want >= 0
    # from the float64 reference alone: both solids are seen, and few pixels are undecided
    assert all((want == k).sum() >= 300 for k in (0, 1)), [(want == k).sum() for k in (0, 1)]
    assert undecided.sum() <= 0.05 * seen.sum(), (int(undecided.sum()), int(seen.sum()))
    hm, owner = _restated_case(case)
    covered = seen & (hm < F32(FAR))
    assert covered.sum() >= 0.95 * seen.sum()
    compared = covered & ~undecided
    bad = compared & (owner != want)
    print("seen", int(seen.sum()), "undecided", int(undecided.sum()), "compared", int(compared.sum()), "differ", int(bad.sum()))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- part_slip ------------------------------------------------------------------------------------------------------------------------
def _pose(R, t):
    return S.scene_row(np.asarray(R, np.float64), t)


def _yaw(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _tilt(a):  # about the x axis
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def test_part_slip_known_answers():
    import torch
    from tacex_amd.sdf_scene import part_slip

    pix = 0.05
    R0 = V.quat_matrix((0.9, 0.3, -0.2, 0.25))
    ref = np.stack([_pose(np.eye(3), [4.0, 3.0, 28.0]), _pose(R0, [5.0, 2.0, 28.5]), _pose(R0, [5.0, 2.0, 28.5]), _pose(R0, [1.0, 1.0, 28.0])])[None]
    now = np.stack([_pose(np.eye(3), [4.3, 2.8, 27.9]),              # pure translation (the z motion is not slip)
                    _pose(_yaw(0.2) @ R0, [5.0, 2.0, 28.5]),          # pure yaw
                    _pose(_yaw(-0.35) @ R0, [5.5, 2.25, 28.5]),       # both
                    _pose(_tilt(0.3) @ R0, [1.0, 1.0, 28.0])])[None]  # a tilt about an in-plane axis
    got = part_slip(torch.from_numpy(now), torch.from_numpy(ref), pix).numpy()
    assert got.shape == (1, 4, 5) and got.dtype == np.float32
    want = np.array([[0.3, -0.2, 0.0, 4.3 / pix, 2.8 / pix], [0.0, 0.0, 0.2, 5.0 / pix, 2.0 / pix],
                     [0.5, 0.25, -0.35, 5.5 / pix, 2.25 / pix], [0.0, 0.0, 0.0, 1.0 / pix, 1.0 / pix]])
    # (the poses are float32: a rotation entry is off by 2^-24, a translation by 2^-22)
    np.testing.assert_allclose(got[0, :, :3], want[:, :3], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got[0, :, 3:], want[:, 3:], rtol=0, atol=2e-6 / pix)
    assert got[0, 3, 0] == 0.0 and got[0, 3, 1] == 0.0  # tilt does not leak into the translation
    with pytest.raises(ValueError, match="reference_pose"):
        part_slip(torch.zeros(2, 3, 16), torch.zeros(2, 3, 15), pix)
    with pytest.raises(ValueError, match="part_pose is"):
        part_slip(torch.zeros(2, 3, 16), torch.zeros(2, 2, 16), pix)
    with pytest.raises(ValueError, match="pixmm"):
        part_slip(torch.zeros(2, 3, 16), torch.zeros(2, 3, 16), 0.0)


# ---- ABI and host layer ---------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_exports():
    import tacex_amd
    from tacex_amd import _build, _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr).group(1)
    plain = re.search(r"\bint\s+tacex_height_map_from_sdf_scene\s*\(([^)]*)\)", hdr).group(1)
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 25 == len(decl.split(",")) == len(plain.split(",")) + 1
    for want, text in zip(args, decl.split(",")):
        assert want is (C.c_void_p if "*" in text else C.c_int if re.search(r"\bint\b", text) else C.c_float), text
    assert "uint8_t* part_map_dev" in decl and "part_map_dev" not in plain
    assert hasattr(_lib.load_library(), NAME)
    assert int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 20  # no change of the version
    text = (_build.CSRC / "sdf_scene.hip").read_text()
    assert "template <bool IDS>" in text and "sdf_scene_kernel<true>" in text and "sdf_scene_kernel<false>" in text  # one kernel source
    assert "part_slip" in tacex_amd.__all__ and "PartContactField" in tacex_amd.__all__


def test_the_entry_point_refuses_before_any_gpu_call():
    from tacex_amd import _lib

    lib = _lib.load_library()
    raw = np.full(2 * 8 * 16 + 8, -3.0, F32)
    off = (-raw.ctypes.data % 16) // 4
    hm = raw[off:off + 2 * 8 * 16]
    fmin, indent, rows = np.full(2, -1.0, F32), np.full(2, -1.0, F32), np.full((2, 4), -7, np.int32)
    parts = np.full((2, 8, 16), 77, np.uint8)
    one = 16
    good = dict(vox=one, nvox=8, vi=one, vf=one, P=1, ids=one, pose=one, ops=one, K=3, pix=0.0295, near=24.0, far=29.0, steps=32, tol=1e-4,
                hm=hm.ctypes.data, fmin=fmin.ctypes.data, parts=parts.ctypes.data, B=2, H=8, W=16)

    def call(**kw):
        a = good | kw
        return getattr(lib, NAME)(a["vox"], a["nvox"], a["vi"], a["vf"], a["P"], a["ids"], a["pose"], a["ops"], a["K"], a["pix"], a["near"],
                                  a["far"], a["steps"], a["tol"], 0.0045, 0.024, a["hm"], a["fmin"], indent.ctypes.data, rows.ctypes.data,
                                  a["parts"], a["B"], a["H"], a["W"], 0)

    cases = [(dict(parts=0), "null part_map_dev"), (dict(vox=0), "null voxels_dev"), (dict(vi=0), "null volumes_i_dev"),
             (dict(vf=0), "null volumes_f_dev"), (dict(ids=0), "null part_ids_dev"), (dict(pose=0), "null part_pose_dev"),
             (dict(ops=0), "null part_ops_dev"), (dict(hm=0), "null hm_mm_dev"), (dict(fmin=0), "null frame_min_dev"),
             (dict(nvox=0), "num_voxels = 0"), (dict(P=0), "num_volumes = 0"), (dict(B=0), "num_frames = 0"), (dict(H=0), "height = 0"),
             (dict(W=-4), "width = -4"), (dict(W=18), "width = 18"), (dict(K=0), "num_slots = 0"), (dict(K=9), "num_slots = 9"),
             (dict(H=2049), "2049 x 16"), (dict(W=2052), "8 x 2052"), (dict(steps=0), "max_steps = 0"), (dict(steps=129), "max_steps = 129"),
             (dict(tol=0.0), "tol_mm = 0"), (dict(tol=float("nan")), "tol_mm"), (dict(near=29.0), "near_clip_mm = 29"),
             (dict(pix=0.0), "pixmm = 0"), (dict(hm=hm.ctypes.data + 4), "16-byte aligned")]
    for kw, text in cases:
        assert call(**kw) == 2, kw
        msg = lib.tacex_last_error().decode()
        assert NAME + ":" in msg and text in msg, (kw, msg)
        assert (raw == -3.0).all() and (fmin == -1.0).all() and (indent == -1.0).all() and (rows == -7).all() and (parts == 77).all(), kw


def test_constructor_takes_part_map_and_still_refuses():
    import inspect

    from tacex_amd import SdfSceneSource, SdfVolume, _lib

    assert inspect.signature(SdfSceneSource.__init__).parameters["part_map"].default is False  # no default moves
    ok = SdfVolume(V.half_space(), 1.0)
    with pytest.raises(ValueError, match="num_slots = 9"):
        SdfSceneSource([ok], 2, "cpu", num_slots=9, part_map=True)
    with pytest.raises(_lib.TacexHipError, match="no CPU fallback"):
        SdfSceneSource([ok], 2, "cpu", num_slots=2, part_map=True)
