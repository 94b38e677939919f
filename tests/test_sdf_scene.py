"""SDF scenes on the CPU: the host layer's refusals, the C ABI's argument checks (no GPU call is made), and the NumPy restatement of
`tacex_height_map_from_sdf_scene` (tests/sdf_scene_ref.py) against the single-volume restatement (bit for bit, one union slot) and
against analytic constructive solid geometry - the reference there is the closed form in float64, never the code under test."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import sdf_scene_ref as S
import test_volume_source as TV  # its grids (sphere R = 3 mm, box 5 x 3 x 2 mm at 0.1 mm), _interpolation_error and EXCLUDED_CAP
import volume_source_ref as V
from conftest import REPO

F32 = np.float32
GEL_TOP, NEAR, FAR, TOL = S.GEL_TOP, S.NEAR, S.FAR, S.TOL
PITCH = TV.PITCH
H, W, PIX = 96, 128, 0.075  # 9.6 x 7.2 mm, as test_volume_source.py looks at, at finer pixels: a crease costs a smaller share
CX, CY = 64 * PIX, 48 * PIX  # the frame centre lies on a pixel


# ---- host layer ---------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    from tacex_amd import SdfSceneSource, SdfVolume, _lib

    ok = SdfVolume(V.half_space(), 1.0)
    with pytest.raises(ValueError, match="non-empty sequence"):
        SdfSceneSource([], 2, "cpu")
    poisoned = SdfVolume(V.half_space(), 0.1)
    poisoned.sdf_mm = np.full((2, 2, 2), np.nan, F32)
    with pytest.raises(ValueError, match="NaN or inf"):
        SdfSceneSource([poisoned], 2, "cpu")
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match=f"num_slots = {k}"):
            SdfSceneSource([ok], 2, "cpu", num_slots=k)
    for n in (0, -3):
        with pytest.raises(ValueError, match="num_frames"):
            SdfSceneSource([ok], n, "cpu")
    with pytest.raises(ValueError, match="max_steps = 0"):
        SdfSceneSource([ok], 2, "cpu", max_steps=0)
    with pytest.raises(ValueError, match="max_steps = 129"):
        SdfSceneSource([ok], 2, "cpu", max_steps=129)
    with pytest.raises(ValueError, match="tol_mm"):
        SdfSceneSource([ok], 2, "cpu", tol_mm=0.0)
    with pytest.raises(ValueError, match="near_clip_mm"):
        SdfSceneSource([ok], 2, "cpu", near_clip_mm=29.0, far_clip_mm=29.0)
    with pytest.raises(ValueError, match="pixmm"):
        SdfSceneSource([ok], 2, "cpu", pixmm=0.0)
    with pytest.raises(_lib.TacexHipError, match="no CPU fallback"):  # every ValueError comes before the device is looked at
        SdfSceneSource([ok], 2, "cpu", num_slots=8)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_exports():
    import tacex_amd
    from tacex_amd import _build, _lib, sdf_scene, volume_source

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    assert re.search(r"\bint\s+tacex_height_map_from_sdf_scene\s*\(", hdr)
    decl = re.search(r"\bint\s+tacex_height_map_from_sdf_scene\s*\(([^)]*)\)", hdr).group(1)
    res, args = _lib.SIGNATURES["tacex_height_map_from_sdf_scene"]
    assert res is C.c_int and len(args) == 24 == len(decl.split(","))
    for want, text in zip(args, decl.split(",")):  # pointer, int and float arguments in the header's order
        assert want is (C.c_void_p if "*" in text else C.c_int if re.search(r"\bint\b", text) else C.c_float), text
    lib = _lib.load_library()
    assert hasattr(lib, "tacex_height_map_from_sdf_scene")
    assert lib.tacex_abi_version() == int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION
    assert "sdf_scene.hip" in _build.SOURCES and "-ffp-contract=off" in _build.FILE_FLAGS["sdf_scene.hip"]
    assert (_build.CSRC / "sdf_tap.h").exists()  # one copy of the tap: both units include it, neither defines it
    for unit in ("sdf_scene.hip", "volume_source.hip"):
        text = (_build.CSRC / unit).read_text()
        assert '#include "sdf_tap.h"' in text and "float sdf_lerp" not in text, unit
    assert tacex_amd.SdfSceneSource.writes_frame_rows is True and "SdfSceneSource" in tacex_amd.__all__
    assert sdf_scene.POSE_FIELDS[:14] == volume_source.POSE_FIELDS[:14] and sdf_scene.POSE_FIELDS[14] == "blend_mm"


def test_the_entry_point_refuses_before_any_gpu_call():
    """Every refusal of the contract returns 2 and leaves the (host) output buffers, poisoned beforehand, untouched: a refused call
    dereferences nothing."""
    from tacex_amd import _lib

    lib = _lib.load_library()
    raw = np.full(2 * 8 * 16 + 8, -3.0, F32)
    off = (-raw.ctypes.data % 16) // 4
    hm = raw[off:off + 2 * 8 * 16]  # 16-byte aligned
    fmin, indent, rows = np.full(2, -1.0, F32), np.full(2, -1.0, F32), np.full((2, 4), -7, np.int32)
    one = 16  # any non-null address for the inputs
    good = dict(vox=one, nvox=8, vi=one, vf=one, P=1, ids=one, pose=one, ops=one, K=3, pix=0.0295, near=24.0, far=29.0, steps=32, tol=1e-4,
                hm=hm.ctypes.data, fmin=fmin.ctypes.data, B=2, H=8, W=16)

    def call(**kw):
        a = good | kw
        return lib.tacex_height_map_from_sdf_scene(a["vox"], a["nvox"], a["vi"], a["vf"], a["P"], a["ids"], a["pose"], a["ops"], a["K"],
                                                   a["pix"], a["near"], a["far"], a["steps"], a["tol"], 0.0045, 0.024, a["hm"], a["fmin"],
                                                   indent.ctypes.data, rows.ctypes.data, a["B"], a["H"], a["W"], 0)

    cases = [(dict(vox=0), "null voxels_dev"), (dict(vi=0), "null volumes_i_dev"), (dict(vf=0), "null volumes_f_dev"),
             (dict(ids=0), "null part_ids_dev"), (dict(pose=0), "null part_pose_dev"), (dict(ops=0), "null part_ops_dev"),
             (dict(hm=0), "null hm_mm_dev"), (dict(fmin=0), "null frame_min_dev"),
             (dict(nvox=0), "num_voxels = 0"), (dict(P=0), "num_volumes = 0"), (dict(P=-2), "num_volumes = -2"),
             (dict(B=0), "num_frames = 0"), (dict(H=0), "height = 0"), (dict(W=-4), "width = -4"), (dict(W=18), "width = 18"),
             (dict(K=0), "num_slots = 0"), (dict(K=9), "num_slots = 9"), (dict(K=-1), "num_slots = -1"),
             (dict(H=2049), "2049 x 16"), (dict(W=2052), "8 x 2052"), (dict(steps=0), "max_steps = 0"),
             (dict(steps=129), "max_steps = 129"), (dict(tol=0.0), "tol_mm = 0"), (dict(tol=-1.0), "tol_mm = -1"),
             (dict(tol=float("nan")), "tol_mm"), (dict(near=29.0), "near_clip_mm = 29"), (dict(near=30.0, far=29.0), "near_clip_mm = 30"),
             (dict(pix=0.0), "pixmm = 0"), (dict(hm=hm.ctypes.data + 4), "16-byte aligned")]
    for kw, text in cases:
        assert call(**kw) == 2, kw
        assert "tacex_height_map_from_sdf_scene" in lib.tacex_last_error().decode() and text in lib.tacex_last_error().decode(), (
            kw, lib.tacex_last_error())
        assert (raw == -3.0).all() and (fmin == -1.0).all() and (indent == -1.0).all() and (rows == -7).all(), kw


# ---- one union slot is the volume source ----------------------------------------------------------------------------------------------
def _one_slot_poses(Hh, Ww, pix):
    c = np.array([0.5 * Ww * pix, 0.5 * Hh * pix])
    R1, R2 = V.quat_matrix((0.9, 0.3, -0.2, 0.25)), V.quat_matrix((0.8, -0.25, 0.5, 0.3))
    nan = V.pose_row(R1, [c[0], c[1], 29.0])
    nan[2] = np.nan
    poses = [(2, V.pose_row(R1, [c[0], c[1], 28.6], 1.3, 0.05)), (1, V.pose_row(R2, [c[0] + 0.3, c[1], 28.3], 1.2)),
             (0, V.pose_row(np.eye(3), [c[0], c[1], 28.4], 1.0, 0.6)), (7, V.pose_row(R1, [c[0], c[1], 28.0])), (-1, V.pose_row(R1, [c[0], c[1], 28.0])),
             (1, V.pose_row(np.eye(3), [c[0], c[1], NEAR + 0.9 * 0.35 * (16.0 * pix)], scale=16.0 * pix)),  # starts inside, at the near clip
             (0, V.pose_row(R1, [c[0], c[1], 28.3], scale=1.2, level_mm=0.1)), (2, V.pose_row(R2, [c[0], c[1], FAR + 1.05])),  # no hit
             (2, V.pose_row(R1, [c[0] + Ww * pix + 2.0, c[1], 29.0])), (2, nan),  # outside the frame; a NaN
             (2, V.pose_row(np.eye(3), [c[0] - 0.2, c[1] + 0.1, 29.1], scale=0.0)), (1, V.pose_row(R2, [c[0], c[1], 28.8], scale=-1.0))]
    return np.array([p[0] for p in poses], np.int32), np.stack([p[1] for p in poses])


@pytest.mark.parametrize("max_steps", [1, 8, 32])
@pytest.mark.parametrize("Hh,Ww", [(24, 32), (30, 40), (9, 4), (60, 80)])
def test_one_union_slot_restates_the_volume_source(Hh, Ww, max_steps):
    """The required equivalence on the restatements: a scene of one union slot with blend 0 - alone, or followed by empty slots -
    gives the bits of `volume_source_ref.height_map`."""
    vox, vi, vf = V.library(V.three_volumes())
    pix = 3.0 / min(Hh, Ww)
    ids, pose = _one_slot_poses(Hh, Ww, pix)
    want = V.height_map(vox, vi, vf, ids, pose, Hh, Ww, pix, NEAR, FAR, max_steps, TOL)
    assert sum(int((want[b] < F32(FAR)).any()) for b in range(len(ids))) >= 4
    got = S.height_map(vox, vi, vf, ids[:, None], pose[:, None], np.zeros((len(ids), 1), np.int32), Hh, Ww, pix, NEAR, FAR, max_steps, TOL)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # with empty slots behind it: no such volume, no such op
    ids3 = np.stack([ids, np.full_like(ids, -1), np.full_like(ids, 2)], 1)
    ops3 = np.stack([np.zeros_like(ids), np.ones_like(ids), np.full_like(ids, 3)], 1)
    got = S.height_map(vox, vi, vf, ids3, np.repeat(pose[:, None], 3, 1), ops3, Hh, Ww, pix, NEAR, FAR, max_steps, TOL)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- restatement against analytic geometry --------------------------------------------------------------------------------------------
# Grids: the sphere of radius 3 mm and the box of 5 x 3 x 2 mm of test_volume_source.py, both at 0.1 mm, placed with a scale.
SPHERE_R, BOX_SIZE = TV.SHAPES["sphere"]["radius"], np.asarray(TV.SHAPES["box"]["size"])
ALIGNED, ROTATED = (1.0, 0.0, 0.0, 0.0), (0.985, 0.05, -0.08, 0.12)
GRID_TURNS = [(0.9, 0.3, -0.2, 0.25), (0.5, -0.6, 0.4, 0.2)]  # how the rotated cases turn the spheres' grids (the shape stays)
BLEND = 0.6
KINDS = ("union of two spheres", "box minus sphere", "box and sphere", "blended spheres")
CASES = [(kind, rotated) for kind in range(4) for rotated in (False, True)]


def _parts(case):
    """[(grid name, op, R, t [mm], scale, blend)] of the case, float64."""
    kind, rotated = CASES[case]
    Rb = V.quat_matrix(ROTATED if rotated else ALIGNED)
    Rs = [V.quat_matrix(q) if rotated else np.eye(3) for q in GRID_TURNS]
    if kind == 0:
        return [("sphere", S.UNION, Rs[0], np.array([CX - 1.2, CY - 0.2, 29.7]), 0.7, 0.0),
                ("sphere", S.UNION, Rs[1], np.array([CX + 1.2, CY + 0.4, 29.7]), 0.6, 0.0)]
    if kind in (1, 2):
        tb = np.array([CX, CY, 29.2 if not rotated else 29.4])  # the box 1.4 x: 7 x 4.2 x 2.8 mm, its near face 0.7 mm under the gel top
        if kind == 1:  # a dimple of radius 0.9 mm, its centre 0.15 mm in front of the near face
            return [("box", S.UNION, Rb, tb, 1.4, 0.0), ("sphere", S.SUBTRACT, Rs[0], tb + Rb @ np.array([0.28, 0.06, -1.55]), 0.3, 0.0)]
        return [("box", S.UNION, Rb, tb, 1.4, 0.0), ("sphere", S.INTERSECT, Rs[0], tb, 1.1, 0.0)]
    d = np.array([0.0, 1.2, 0.0]) if rotated else np.array([1.2, 0.0, 0.0])  # side by side at equal depth: the mirror plane is a pixel column / row
    c = np.array([CX, CY, 29.3])
    return [("sphere", S.UNION, Rs[0], c - d, 0.6, BLEND), ("sphere", S.UNION, Rs[1], c + d, 0.6, BLEND)]


def _sphere_span(X, Y, c, r):
    d2 = r * r - (X - c[0]) ** 2 - (Y - c[1]) ** 2
    s = np.sqrt(np.where(d2 > 0, d2, np.nan))
    return c[2] - s, c[2] + s


def _box_span(X, Y, R, t, half):
    """Entry and exit depth of the rays (X, Y, .) through the box, NaN where they miss, and the axis of the entry face."""
    o0 = np.stack([X - t[0], Y - t[1], np.full_like(X, -t[2])], -1) @ R  # R^T (P - t) at z = 0
    d = R[2]  # R^T e_z
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-half - o0) / d, (half - o0) / d
    tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
    for k in range(3):
        if abs(d[k]) < 1e-12:
            inside = np.abs(o0[:, k]) <= half[k]
            tn[:, k], tf[:, k] = np.where(inside, -np.inf, np.inf), np.where(inside, np.inf, -np.inf)
    lo, hi, axis = tn.max(1), tf.min(1), tn.argmax(1)
    miss = ~(lo < hi)
    return np.where(miss, np.nan, lo), np.where(miss, np.nan, hi), axis


@functools.lru_cache(maxsize=None)
def _analytic(case):
    """The closed form along every pixel's ray, in float64: (z* with NaN where the ray hits nothing, |n_z| of the surface hit, a label
    of the surface hit (0: none), the largest interpolation error of the scene's grids in camera mm)."""
    kind, _ = CASES[case]
    parts = _parts(case)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X, Y = (x * PIX).reshape(-1), (y * PIX).reshape(-1)
    E = max(TV._interpolation_error(name, 0.0) * scale for name, _, _, _, scale, _ in parts)
    nan = np.full(X.size, np.nan)
    if kind in (0, 3):
        (_, _, _, ca, sa, _), (_, _, _, cb, sb, _) = parts
        ra, rb = SPHERE_R * sa, SPHERE_R * sb
        if kind == 0:  # the nearer of the two first hits
            za, zb = _sphere_span(X, Y, ca, ra)[0], _sphere_span(X, Y, cb, rb)[0]
            first_a = ~np.isnan(za) & (np.isnan(zb) | (za <= zb))
            z = np.where(first_a, za, zb)
            nz = np.where(first_a, (ca[2] - z) / ra, (cb[2] - z) / rb)
            label = np.where(np.isnan(z), 0, np.where(first_a, 1, 2))
        else:  # on the mirror plane a = b and smin(a, a) = a - k/4: a sphere of radius r + k/4 about either centre
            mirror = np.abs((X - 0.5 * (ca[0] + cb[0])) * (cb[0] - ca[0]) + (Y - 0.5 * (ca[1] + cb[1])) * (cb[1] - ca[1])) < 1e-9
            rr = ra + BLEND / 4
            z = np.where(mirror, _sphere_span(X, Y, ca, rr)[0], np.nan)
            nz = (ca[2] - z) / rr
            label = np.where(np.isnan(z), 0, 1)
    else:
        (_, _, Rb, tb, sb, _), (_, _, _, cs, ss, _) = parts
        b1, b2, axis = _box_span(X, Y, Rb, tb, 0.5 * BOX_SIZE * sb)
        rs = SPHERE_R * ss
        s1, s2 = _sphere_span(X, Y, cs, rs)
        face_nz = np.abs(Rb[2])[axis]
        if kind == 1:  # the first point of the box that is not in the ball
            in_ball = ~np.isnan(s1) & (s1 <= b1) & (b1 < s2)  # the entry into the box lies in the ball: out of it at s2, if still in the box
            z = np.where(in_ball, np.where(s2 < b2, s2, np.nan), b1)
            nz = np.where(in_ball, (z - cs[2]) / rs, face_nz)
            label = np.where(np.isnan(z), 0, np.where(in_ball, 3, 10 + axis))
        else:  # the later of the two entries, if before the earlier exit
            lo, hi = np.fmax(b1, s1), np.fmin(b2, s2)
            both = ~np.isnan(b1) & ~np.isnan(s1) & (lo < hi)
            z = np.where(both, lo, np.nan)
            on_ball = both & (s1 > b1)
            nz = np.where(on_ball, (cs[2] - z) / rs, face_nz)
            label = np.where(~both, 0, np.where(on_ball, 3, 10 + axis))
    z = np.where(np.isnan(z), nan, z)
    return z.reshape(H, W), np.where(label > 0, nz, 0.0).reshape(H, W), label.reshape(H, W), E


def _neighbours_differ(label, reach=1):
    """Pixels with another label within `reach` pixels: with reach * pixmm >= scale * 0.1 mm, within one projected voxel of a
    silhouette or of a crease between two surfaces."""
    pad = np.pad(label, reach, mode="edge")
    out = np.zeros(label.shape, bool)
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            out |= pad[dy:dy + H, dx:dx + W] != label
    return out


@functools.lru_cache(maxsize=None)
def _restated(case, blend=None, max_steps=32):
    parts = _parts(case)
    names = ("sphere", "box")
    vox, vi, vf = V.library([(TV._volume(n).sdf_mm, PITCH, None, 1.0) for n in names])
    ids = np.array([[names.index(p[0]) for p in parts]], np.int32)
    ops = np.array([[p[1] for p in parts]], np.int32)
    pose = np.stack([S.scene_row(p[2], p[3], p[4], 0.0, p[5] if blend is None else blend) for p in parts])[None]
    stats = {}
    hm = S.height_map(vox, vi, vf, ids, pose, ops, H, W, PIX, NEAR, FAR, max_steps, TOL, stats)[0]
    hm.setflags(write=False)
    return hm, stats


def _masks(case):
    kind, _ = CASES[case]
    zstar, nz, label, E = _analytic(case)
    with np.errstate(invalid="ignore"):
        hit = (label > 0) & (zstar < FAR)  # (a surface beyond the far clip keeps its label - no crease there - and is not compared)
    crease = _neighbours_differ(label, 2 if kind in (1, 2) else 1)  # (a voxel is at most 0.07 mm in the sphere cases, 0.14 mm in the box cases)
    if kind == 3:  # only the mirror plane is known in closed form: its neighbours across the plane are not creases
        crease = np.zeros_like(hit)
    excluded = hit & ((nz < 0.25) | crease)
    return zstar, nz, label, E, hit, excluded


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_poses_stay_inside_the_exclusion_caps(case):
    """On the analytic side alone: the pixels left out of the depth comparison (n_z < 0.25, within a voxel of a silhouette or crease)
    are a small share of the pixels that hit."""
    kind, rotated = CASES[case]
    zstar, nz, label, E, hit, excluded = _masks(case)
    cap = TV.EXCLUDED_CAP["box" if kind in (1, 2) else "sphere"]
    print(KINDS[kind], "rotated" if rotated else "aligned", "hit", int(hit.sum()), "excluded", int(excluded.sum()), "labels", np.unique(label).tolist())
    if kind == 3:
        assert hit.sum() >= 20  # the rays of the mirror plane
    else:
        assert hit.sum() >= 400 and (~hit).sum() >= 300  # an imprint and a background
        assert len(np.unique(label)) >= 3  # a background and two surfaces
    assert excluded.sum() <= cap * hit.sum()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_restatement_against_the_closed_form(case):
    """|z - z*| <= 2 (E + tol) / n_z, with E the largest |float64 trilinear interpolant - closed form| of the scene's grids near their
    surfaces, magnified with the part (min, max and the smooth minimum move by at most what their arguments move by, so the folded
    field is off by at most E), and n_z the slope of the field along the ray at the hit."""
    kind, rotated = CASES[case]
    zstar, nz, label, E, hit, excluded = _masks(case)
    hm, stats = _restated(case)
    far = hm == F32(FAR)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound_map = 2.0 * (E + TOL) / nz
    must = hit & ~excluded
    required = must & (zstar + bound_map < FAR)
    assert not far[required].any(), (int(far[required].sum()), np.argwhere(far & required)[:4].tolist())
    compared = must & ~far
    assert compared.sum() >= (20 if kind == 3 else 300)
    err = np.abs(hm.astype(np.float64) - zstar)[compared]
    bound = bound_map[compared]
    worst = float((err / bound).max())
    print(KINDS[kind], "rotated" if rotated else "aligned", "E =", E, "compared", int(compared.sum()), "max |z - z*| =", float(err.max()),
          "worst error / bound =", worst, {k: v for k, v in stats.items() if v})
    assert (err <= bound).all(), worst
    if kind != 3:  # rays with nothing within three pixels (0.225 mm: a voxel and more) hit nothing
        clear = ~_neighbours_differ(label, 3) & (label == 0)
        assert clear.sum() >= 300 and far[clear].all(), int((~far[clear]).sum())
    want = {0: "changed_union", 1: "changed_subtract", 2: "changed_intersect", 3: "blended"}[kind]
    assert stats[want] > 100 and stats["outside"] > 0  # the operation under test shaped the field


@pytest.mark.parametrize("rotated", [False, True])
def test_a_blend_never_digs_deeper_than_the_hard_union(rotated):
    """smin <= min: the blended surface encloses the hard one.  A ray stops within tol of the field's zero or, by the grazing-ray
    rule, within a voxel of it, so the blended map is at most tol_mm + one voxel deeper anywhere."""
    case = CASES.index((3, rotated))
    soft, hard = _restated(case, max_steps=64)[0].astype(np.float64), _restated(case, blend=0.0, max_steps=64)[0].astype(np.float64)
    vox = 0.6 * PITCH
    assert (soft < hard - 0.05).sum() > 50  # the fillet is there
    assert (soft <= hard + TOL + vox).all(), float((soft - hard).max())


def test_an_env_alone_equals_the_env_in_a_batch():
    Hh, Ww = 30, 40
    vox, vi, vf = S.library(S.three_volumes())
    ids, ops, pose = S.gpu_scene(Hh, Ww)
    batch = S.height_map(vox, vi, vf, ids, pose, ops, Hh, Ww, S.scene_pixmm(Hh, Ww), NEAR, FAR, 32, TOL)
    for b in range(S.NUM_ENVS):
        alone = S.height_map(vox, vi, vf, ids[b:b + 1], pose[b:b + 1], ops[b:b + 1], Hh, Ww, S.scene_pixmm(Hh, Ww), NEAR, FAR, 32, TOL)[0]
        assert np.array_equal(alone.view(np.uint32), batch[b].view(np.uint32)), b


def test_the_scene_covers_its_cases():
    """On the restatement alone: what the scene of the GPU tests (`sdf_scene_ref.gpu_scene`) is meant to exercise is there."""
    Hh, Ww = 30, 40
    vox, vi, vf = S.library(S.three_volumes())
    P = vi.shape[0]
    ids, ops, pose = S.gpu_scene(Hh, Ww)
    far = F32(FAR)

    def run(b, K=8, steps=32, **change):
        i, o, p = (a[b:b + 1, :K].copy() for a in (ids, ops, pose))
        for k, v in change.items():
            {"ids": i, "ops": o}[k][0, v[0]] = v[1]
        st = {}
        return S.height_map(vox, vi, vf, i, p, o, Hh, Ww, S.scene_pixmm(Hh, Ww), NEAR, FAR, steps, TOL, st)[0], st

    maps, stats = zip(*(run(b) for b in range(S.NUM_ENVS)))
    # an empty slot, an id out of range, an op out of range: each presses something once it is repaired
    assert ids[0, 3] == -1 and ids[0, 4] == P and ops[0, 5] == 7 and stats[0]["empty_slots"] == 3
    for slot, fix in ((4, dict(ids=(4, S.BALL))), (5, dict(ops=(5, S.UNION)))):
        assert run(0, **fix)[1]["empty_slots"] == 2, slot
    assert ops[6, 2] == -1 and stats[6]["empty_slots"] == 6
    # an env with no union slot: far clip everywhere, every tile dead, no tap
    assert ((ops[1] != S.UNION) | (ids[1] < 0)).all() and (maps[1] == far).all() and stats[1]["dead_tiles"] == stats[1]["tiles"] and stats[1]["taps"] == 0
    assert stats[1]["empty_slots"] == 3  # (the others would cut, were there something to cut)
    # a first slot that is a subtraction: it changes nothing, the slots behind it press
    assert ops[2, 0] == S.SUBTRACT and (maps[2] < far).sum() > 100
    assert np.array_equal(maps[2], run(2, ids=(0, -1))[0])
    # blend 0 and blend > 0; all three operations shape the field
    assert all(stats[b]["blended"] > 50 for b in (0, 2, 3, 4, 6)) and (pose[0, 0, 14] == 0) and (pose[0, 2, 14] > 0)
    assert stats[0]["changed_subtract"] > 50 and stats[0]["changed_intersect"] > 50 and stats[4]["changed_intersect"] > 50
    assert stats[3]["changed_subtract"] > 50 and all(stats[b]["changed_union"] > 50 for b in (0, 2, 3, 4, 6))
    assert not np.array_equal(maps[0], run(0, ids=(1, -1))[0]) and not np.array_equal(maps[0], run(0, ids=(7, -1))[0])
    assert not np.array_equal(maps[3], run(3, ids=(2, -1))[0]) and not np.array_equal(maps[4], run(4, ids=(2, -1))[0])
    # overlapping boxes, outside-box evaluations with and without a tap, the same volume in two slots
    assert all(stats[b]["overlap_rays"] > 100 and stats[b]["outside"] > 100 for b in (0, 2, 3, 4, 6))
    assert stats[2]["outside_skipped"] > 100 and stats[3]["outside_skipped"] > 100
    assert ids[0, 0] == ids[0, 2] == S.BALL and ids[3, 3] == ids[3, 4] == S.CAPSULE and ops[3, 3] == ops[3, 4] == S.UNION
    # a slot whose box misses the frame; a tile without a live union slot; a ray that meets only a subtract slot's box
    assert stats[5]["culled_slots"] >= stats[5]["tiles"] // 2 and stats[5]["dead_tiles"] > 0 and (maps[5] == far).all()
    assert stats[0]["culled_slots"] > 0 and stats[3]["dead_tiles"] == 0
    assert stats[5]["subtract_only_rays"] > 100 and stats[0]["subtract_only_rays"] > 10
    for K in (1, 3, 8):  # (every call of the GPU test has dead tiles)
        for hh, ww in ((24, 32), (30, 40), (9, 4), (8, 2048)):
            st = {}
            S.height_map(vox, vi, vf, *(a[:, :K] for a in S.gpu_scene(hh, ww)[::2]), S.gpu_scene(hh, ww)[1][:, :K], hh, ww,
                         S.scene_pixmm(hh, ww), NEAR, FAR, 1, TOL, st)
            assert st["dead_tiles"] > 0 and st["covered"] > 0, (K, hh, ww)
    # a non-finite pose: that slot alone is empty
    assert np.isnan(pose[3, 0]).sum() == 1 and stats[3]["empty_slots"] == 4 and (maps[3] < far).sum() > 100
    # grazing rays, rays that start inside a part, hits, taps without a hit
    assert sum(s["grazing"] for s in stats) > 50 and stats[2]["entered_inside"] > 50 and all(stats[b]["hits"] > 100 for b in (0, 2, 3, 4, 6))
    assert (run(4, K=1)[0] == far).all() and run(4, K=1)[1]["taps"] > 100  # (env 4's first slot: marched, never hit)
    # the tap budget matters
    assert not np.array_equal(run(0, steps=1)[0], run(0, steps=8)[0]) and not np.array_equal(run(0, steps=8)[0], maps[0])
