"""Camera depth of the affine body from its state (`AffineBodyDepthSource`, `tacex_depth_from_affine_body`): the symbol, the argument
checks and the NumPy reference against the analytic sphere on the CPU; on the GPU the kernel against that reference bit for bit (three
meshes, six states / cameras, a frame with partial tiles in both axes), against `tacex_depth_from_deformed_mesh` on the same world points,
and through the sensor in `FemBallScene`."""
import ctypes as C
import re

import numpy as np
import pytest

import affine_body_depth_ref as ref
from conftest import REPO

LEVELS = {1: (42, 80), 3: (642, 1280), 4: (2562, 5120)}  # fewer triangles than threads | five setup rounds | above 2048 vertices: unstaged


# -- CPU ------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported():
    from tacex_amd import _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+tacex_depth_from_affine_body\s*\(([^)]*)\)\s*;", code)
    assert m, "tacex_depth_from_affine_body is not declared in include/tacex_hip.h"
    restype, argtypes = _lib.SIGNATURES["tacex_depth_from_affine_body"]
    assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")) == 18
    lib = _lib.load_library()
    assert hasattr(lib, "tacex_depth_from_affine_body")
    assert int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == lib.tacex_abi_version() == _lib.ABI_VERSION == 20
    import tacex_amd

    assert "AffineBodyDepthSource" in tacex_amd.__all__


def test_affine_body_abi_rejects_bad_arguments_without_a_gpu():
    from tacex_amd import _lib

    lib = _lib.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    good = dict(X=p, nv=4, tris=p, T=2, q=p, pos=p, rot=p, fx=340.0, fy=325.0, cx=160.0, cy=125.0, near=0.024, far=0.029, depth=p, B=1, H=8, W=8)

    def call(**kw):
        a = {**good, **kw}
        return lib.tacex_depth_from_affine_body(a["X"], a["nv"], a["tris"], a["T"], a["q"], a["pos"], a["rot"], a["fx"], a["fy"], a["cx"], a["cy"],
                                                a["near"], a["far"], a["depth"], a["B"], a["H"], a["W"], None)

    for k in ("X", "tris", "q", "pos", "rot", "depth"):
        assert call(**{k: None}) == 2 and b"null" in lib.tacex_last_error()
    for k in ("nv", "T", "B", "H", "W"):
        assert call(**{k: 0}) == 2 and b"counts" in lib.tacex_last_error()
        assert call(**{k: -3}) == 2 and b"counts" in lib.tacex_last_error()
    for near, far in ((0.029, 0.024), (0.024, 0.024), (-0.001, 0.029), (float("nan"), 0.029)):
        assert call(near=near, far=far) == 2 and b"clipping" in lib.tacex_last_error()


@pytest.mark.parametrize("level", [2, 3, 4])
def test_reference_against_the_analytic_sphere(level):
    """A = I, radius 9 mm, the top 28.0 mm in front of the camera and 0.8 / 0.5 mm off the axis.  The mesh is inscribed in the sphere: along a
    ray it lies behind the sphere by at most the sagitta of a facet, sag = R - sqrt(R^2 - rc^2) with rc the largest face circumradius,
    measured along the normal; with cos(ray, normal) > 0.5 that is at most 2 sag along the ray, and the z-depth differs by less than the
    distance along the ray."""
    from oracle.mesh_depth_oracle import icosphere

    v, t = icosphere(ref.RADIUS, level)
    X = v.astype(np.float64)
    R = ref.RADIUS
    c = ref.TOP + [0.0, 0.0, R]
    d = ref.render(X, t, ref.state(c)[None], np.zeros((1, 3)), np.eye(3)[None])[0].astype(np.float64)
    a, b, cc = (X[t[:, k]] for k in range(3))
    la, lb, lc = np.linalg.norm(b - cc, axis=1), np.linalg.norm(cc - a, axis=1), np.linalg.norm(a - b, axis=1)
    rc = (la * lb * lc / (2.0 * np.linalg.norm(np.cross(b - a, cc - a), axis=1))).max()
    sag = R - np.sqrt(R * R - rc * rc)
    W, H = ref.RES
    fx, fy, cx, cy = ref.INTR
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ray = np.stack([(jj - cx) / fx, (ii - cy) / fy, np.ones_like(jj)], -1)  # z component 1: the ray parameter is the z-depth
    A_, B_, C_ = (ray * ray).sum(-1), -2.0 * (ray @ c), c @ c - R * R
    disc = B_ * B_ - 4.0 * A_ * C_
    hit = disc > 0.0
    z = np.where(hit, (-B_ - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * A_), np.inf)
    n = (ray * np.where(hit, z, 0.0)[..., None] - c) / R
    cos = np.where(hit, -(ray * n).sum(-1) / np.sqrt(A_), 0.0)
    front = hit & (cos > 0.5)
    seen = front & np.isfinite(d)
    err = d[seen] - z[seen]
    print(f"level {level}: {int(seen.sum())} seen pixels, max error {err.max() * 1e3:.3f} mm, 2 sag {2e3 * sag:.3f} mm")
    assert seen.sum() > 500
    assert err.min() >= 0.0 and err.max() <= 2.0 * sag
    # nothing that must be seen is missing: the mesh lies within 2 sag behind the sphere wherever the sphere is inside the clipping range
    must = front & (z >= ref.CLIP[0]) & (z <= ref.CLIP[1] - 2.0 * sag)
    assert must.sum() > 400 and np.isfinite(d[must]).all()


def test_sources_refuse_the_wrong_kind_of_object():
    from types import SimpleNamespace

    from tacex_amd import AffineBodyDepthSource

    pad = SimpleNamespace(is_affine_body=False, _uipc_sim=None)
    with pytest.raises(ValueError, match="affine body"):
        AffineBodyDepthSource(pad, (0, 0, 0), (1, 0, 0, 0))
    loose = SimpleNamespace(is_affine_body=True, _uipc_sim=None)
    with pytest.raises(RuntimeError, match="set up"):
        AffineBodyDepthSource(loose, (0, 0, 0), (1, 0, 0, 0))


# -- GPU: the kernel ------------------------------------------------------------------------------------------------------------
_rendered = {}


def _mesh(level):
    from oracle.mesh_depth_oracle import icosphere

    v, t = icosphere(ref.RADIUS, level)
    assert (len(v), len(t)) == LEVELS[level]
    return v.astype(np.float64), t


def _affine_body_depth(X, tris, q, pos, rot_inv, res=ref.RES, intr=ref.INTR):
    import torch

    from tacex_amd import _lib

    lib = _lib.load_library()
    W, H = res
    dev = "cuda:0"
    Xd, td, qd, pd, rd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, tris.astype(np.int32), q, pos, rot_inv))
    depth = torch.full((len(q), H, W), -1.0, dtype=torch.float32, device=dev)
    _lib.check(lib.tacex_depth_from_affine_body(_lib.ptr(Xd), len(X), _lib.ptr(td), len(tris), _lib.ptr(qd), _lib.ptr(pd), _lib.ptr(rd), *intr,
                                                ref.CLIP[0], ref.CLIP[1], _lib.ptr(depth), len(q), H, W, _lib.current_stream_handle(depth.device)),
               "tacex_depth_from_affine_body")
    return depth.cpu().numpy()


def _gpu_image(level):
    """The six cases of mesh `level` through tacex_depth_from_affine_body, rendered once for the tests that compare it."""
    if level not in _rendered:
        X, t = _mesh(level)
        _rendered[level] = _affine_body_depth(X, t, *ref.cases())
    return _rendered[level]


def _check_seen(img):
    seen = np.isfinite(img).reshape(6, -1).sum(1)
    assert (seen[[0, 1, 2, 4, 5]] > 0).all() and seen[3] == 0, seen  # (equality must not pass on empty images)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("level", sorted(LEVELS))
def test_affine_body_depth_equals_reference_bit_for_bit(level):
    X, t = _mesh(level)
    q, pos, rot_inv = ref.cases()
    want = ref.render(X, t, q, pos, rot_inv)
    got = _gpu_image(level)
    np.testing.assert_array_equal(np.isfinite(got), np.isfinite(want))
    m = np.isfinite(want)
    np.testing.assert_array_equal(got[m], want[m])
    seen = _check_seen(got)
    print(f"level {level}: seen {seen.tolist()}, dropped in case 5: {int(ref.dropped_triangles(X, t, q, pos, rot_inv)[4])}")
    assert ref.dropped_triangles(X, t, q, pos, rot_inv)[4] > 0  # vertices behind the camera plane: their triangles dropped whole
    # the tiles the kernel leaves unstaged (its bounding-sphere test, restated): some in the off-axis case, all beyond the far plane, none
    # with the camera inside the body - and never one that holds a pixel
    skip = ref.skipped_tiles(X, q, pos, rot_inv)
    assert 0 < skip[2].sum() < skip[2].size and skip[3].all() and not skip[4].any() and not skip[0].all(), skip
    W, H = ref.RES
    for b, i, j in zip(*np.nonzero(skip)):
        assert not np.isfinite(want[b, 32 * i:32 * i + 32, 64 * j:64 * j + 64]).any(), (b, i, j)


@pytest.mark.gpu
@pytest.mark.parametrize("level", sorted(LEVELS))
def test_affine_body_depth_equals_the_deformed_mesh_entry_point(level):
    """The same world points uploaded as x with surf_ids = arange through tacex_depth_from_deformed_mesh: the shared part is shared."""
    import torch

    from tacex_amd import _lib

    X, t = _mesh(level)
    q, pos, rot_inv = ref.cases()
    lib = _lib.load_library()
    W, H = ref.RES
    dev = "cuda:0"
    x = torch.from_numpy(np.ascontiguousarray(ref.world_points(X, q))).to(dev)
    ids = torch.arange(len(X), dtype=torch.int32, device=dev)
    td, pd, rd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (t.astype(np.int32), pos, rot_inv))
    depth = torch.full((6, H, W), -1.0, dtype=torch.float32, device=dev)
    _lib.check(lib.tacex_depth_from_deformed_mesh(_lib.ptr(x), len(X), _lib.ptr(ids), len(X), _lib.ptr(td), len(t), _lib.ptr(pd), _lib.ptr(rd),
                                                  *ref.INTR, ref.CLIP[0], ref.CLIP[1], _lib.ptr(depth), 6, H, W,
                                                  _lib.current_stream_handle(depth.device)), "tacex_depth_from_deformed_mesh")
    got = _gpu_image(level)
    _check_seen(got)
    np.testing.assert_array_equal(got, depth.cpu().numpy())


# -- GPU: the source in the ball scene ------------------------------------------------------------------------------------------------
RES_C4, INTR_C4 = (320, 240), (340.0, 325.0, 160.0, 125.0)


def _scene_source(scene):
    from tacex_amd import AffineBodyDepthSource

    pos, quat = scene.camera_pose()
    return AffineBodyDepthSource(scene.ball, pos, quat, resolution=RES_C4, intrinsics=INTR_C4, clipping_range=ref.CLIP)


def _scene_reference(scene, src):
    """The reference on the scene's own mesh and state (not on the tables the source under test made of them)."""
    return ref.render(scene.ball.points, scene.ball.tris, scene.sim.q.cpu().numpy(), src.pos.cpu().numpy(), src.rot_inv.cpu().numpy(),
                      RES_C4, INTR_C4)


def _follow_the_case(scene, src, pos_z0, i):
    """The camera moves with the sensor case: the motion FemBallScene._step gives the pad's back face in step i."""
    c = float(0.5 - 0.5 * np.cos(0.3 * i))
    src.pos[:, 2] = pos_z0 - c * scene.depth


def _sensor(scene, B, src=None):
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.calibration import CALIB_GELSIGHT_MINI
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg

    cfg = GelSightSensorCfg(
        num_envs=B, sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=RES_C4, clipping_range=ref.CLIP, depth_source=src),
        data_types=["tactile_rgb", "height_map"],
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(CALIB_GELSIGHT_MINI), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                          with_shadow=False, tactile_img_res=RES_C4, device="cuda:0"),
        marker_motion_sim_cfg=None, device="cuda:0")
    s = GelSightSensor(cfg, gelpad_obj=scene.gelpad)
    s.initialize()
    return s


@pytest.mark.gpu
def test_scene_mesh_at_the_sensor_resolution_equals_reference():
    """The scene's own level-2 ball (162 vertices / 320 triangles) at 320 x 240 through `AffineBodyDepthSource`: the six states written into
    `UipcSim.q`, the cameras into `pos` / `rot_inv`, all in place."""
    import torch

    from tacex_amd.uipc.gelpad_scene import FemBallScene

    scene = FemBallScene(6, "cuda:0")
    src = _scene_source(scene)
    assert tuple(src.rest_verts.shape) == (162, 3) and tuple(src.tris.shape) == (320, 3)
    q, pos, rot_inv = ref.cases()
    q_ptr = scene.sim.q.data_ptr()
    scene.sim.q.copy_(torch.from_numpy(q))
    src.pos.copy_(torch.from_numpy(pos))
    src.rot_inv.copy_(torch.from_numpy(rot_inv))
    got = src().cpu().numpy()
    assert scene.sim.q.data_ptr() == q_ptr
    want = _scene_reference(scene, src)
    np.testing.assert_array_equal(np.isfinite(got), np.isfinite(want))
    m = np.isfinite(want)
    np.testing.assert_array_equal(got[m], want[m])
    seen = _check_seen(got)
    assert seen[0] > 5000, seen  # a 0.3 x frame sees 552 pixels of this mesh
    skip = ref.skipped_tiles(scene.ball.points, q, pos, rot_inv, RES_C4, INTR_C4)  # 5 x 8 tiles: most of them are not staged
    assert skip[0].sum() >= 20 and skip[3].all() and not skip[4].any(), skip.reshape(6, -1).sum(1)
    for b, i, j in zip(*np.nonzero(skip)):
        assert not np.isfinite(want[b, 32 * i:32 * i + 32, 64 * j:64 * j + 64]).any(), (b, i, j)
    with pytest.raises(ValueError, match="gel pad"):  # (existing behaviour: the pad's source still refuses the body)
        from tacex_amd import FemSurfaceDepthSource

        FemSurfaceDepthSource(scene.ball, *scene.camera_pose())


@pytest.mark.gpu
def test_pressed_ball_through_the_sensor():
    """FemBallScene, the ball's depth as the sensor's depth source, the camera following the case.  At rest the ball's top lies 1.02 d_hat
    beyond the gel plane (28.5 mm), beyond the far plane: nothing is seen.  At the press peak (step 10) the pad has come down over the ball:
    the height map is the reference's on the same q and camera, its minimum is the ball's nearest vertex (up to the slope of the facets
    across half a pixel, the bound tests/test_fem_surface_depth.py uses for the pad), and the envs see more the deeper they press
    (scene.depth: 0.2 ... 0.8 mm over the envs)."""
    import torch

    from oracle.taxim_oracle import TaximOracle
    from tacex_amd.uipc.gelpad_scene import FemBallScene

    B = 4
    scene = FemBallScene(B, "cuda:0")
    src = _scene_source(scene)
    pos_z0 = src.pos[:, 2].clone()
    s = _sensor(scene, B, src=src)
    far_mm = np.float32(ref.CLIP[1]) * np.float32(1000.0)
    s.update(dt=0.01, force_recompute=True)
    assert not torch.isfinite(src.depth).any()
    np.testing.assert_array_equal(s.data.output["height_map"].cpu().numpy(), np.full((B, 240, 320), far_mm))
    np.testing.assert_array_equal(s.indentation_depth.cpu().numpy(), np.zeros(B, np.float32))
    rgb0 = s.data.output["tactile_rgb"].clone()
    for i in range(11):  # c = 0.5 - 0.5 cos(0.3 i): the peak is at i = 10
        scene.step(i)
        _follow_the_case(scene, src, pos_z0, i)
        s.update(dt=0.01, force_recompute=True)
    hm = s.data.output["height_map"].cpu().numpy()
    want = _scene_reference(scene, src)
    np.testing.assert_array_equal(hm, np.where(np.isfinite(want), want, np.float32(ref.CLIP[1])) * np.float32(1000.0))
    ind = s.indentation_depth.cpu().numpy()
    np.testing.assert_array_equal(ind, TaximOracle.indentation_depth(hm))
    pc = ref.camera_frame_f32(ref.world_points(scene.ball.points, scene.sim.q.cpu().numpy()), src.pos.cpu().numpy(),
                              src.rot_inv.cpu().numpy())
    zmin = pc[:, :, 2].min(1).astype(np.float64) * 1000.0  # mm
    seen = np.isfinite(want).reshape(B, -1).sum(1)
    dmin = hm.reshape(B, -1).min(1).astype(np.float64)  # (an env that sees nothing: the far clip)
    print(f"seen {seen.tolist()} px, nearest depth {dmin.tolist()} mm, nearest vertex {zmin.tolist()} mm, indentation {ind.tolist()} mm")
    assert (dmin[seen > 0] >= zmin[seen > 0] - 1e-5).all(), (dmin, zmin)
    assert (dmin <= zmin + 0.05).all(), (dmin, zmin)
    assert (np.diff(seen) >= 0).all() and (np.diff(ind) >= 0).all(), (seen, ind)
    assert seen[-1] > 0 and ind[-1] > 0.0, (seen, ind)
    rgb = s.data.output["tactile_rgb"]
    assert torch.isfinite(rgb).all()
    assert float((rgb[-1] - rgb0[-1]).abs().max()) > 0.02


@pytest.mark.gpu
def test_fill_equals_depth_source():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemBallScene

    B = 4
    scene = FemBallScene(B, "cuda:0")
    srcs = (_scene_source(scene), _scene_source(scene))
    pos_z0 = srcs[0].pos[:, 2].clone()
    via_source = _sensor(scene, B, src=srcs[0])
    via_fill = _sensor(scene, B)
    via_fill.set_height_map_source(srcs[1])
    for i in range(9):
        scene.step(i)
        for src, s in zip(srcs, (via_source, via_fill)):
            _follow_the_case(scene, src, pos_z0, i)
            s.update(dt=0.01, force_recompute=True)
        a, b = via_source, via_fill
        assert torch.equal(a.data.output["height_map"], b.data.output["height_map"])
        assert torch.equal(a.optical_simulator._frame_min, b.optical_simulator._frame_min)
        assert torch.equal(a.indentation_depth, b.indentation_depth)
    assert bool(torch.isfinite(srcs[1].depth).any())  # (the ball has come into view)


@pytest.mark.gpu
def test_render_waits_for_a_step_on_the_side_stream():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemBallScene

    B = 8
    scene = FemBallScene(B, "cuda:0", side_stream=True)
    src = _scene_source(scene)
    pos_z0 = src.pos[:, 2].clone()
    s = _sensor(scene, B, src=src)
    for i in range(11):
        scene.step(i)
        _follow_the_case(scene, src, pos_z0, i)
        s.update(dt=0.01, force_recompute=True)  # renders on the current stream right behind the step's event
        hm = s.data.output["height_map"].clone()
        torch.cuda.synchronize()
        d = src().clone()
        want = torch.where(torch.isfinite(d), d, torch.full_like(d, ref.CLIP[1])) * 1000.0
        assert torch.equal(hm, want), i
    assert scene.sim.step_done is not None
    assert bool(torch.isfinite(d).any())
