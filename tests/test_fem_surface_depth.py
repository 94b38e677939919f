"""Camera depth of the FEM gel pad's deformed contact face (`FemSurfaceDepthSource`, `tacex_depth_from_deformed_mesh`): face selection
and argument checks on the CPU; on the GPU the rasteriser against oracle/mesh_depth_oracle.py bit for bit (camera-frame float32 vertices,
identity pose), the rest plane, the physics of a pressed pad through the sensor, the ball scene, `fill` against `depth_source` and the
side-stream ordering."""
import ctypes as C

import numpy as np
import pytest

CAM_C4 = (0.010375, 0.012625, -0.024)  # the pad centre, 24 mm behind the back face (z = 0), optical axis +z
QUAT_ID = (1.0, 0.0, 0.0, 0.0)
INTR = {(320, 240): (340.0, 325.0, 160.0, 125.0), (640, 480): (680.0, 650.0, 320.0, 250.0)}
CLIP = (0.024, 0.029)


# -- CPU ------------------------------------------------------------------------------------------------------------------------
def test_contact_face_of_the_c4_pad():
    from tacex_amd.height_map_source import contact_face_triangles
    from tacex_amd.uipc.uipc_object import UipcObject, UipcObjectCfg, gelpad_box_mesh

    P, T = gelpad_box_mesh(8, 10, 4)
    tri = contact_face_triangles(P, T, [0.0, 0.0, 1.0])
    assert tri.shape == (160, 3)  # 2 x 8 x 10
    assert np.all(P[tri][..., 2] == P[:, 2].max()) and P[:, 2].max() == pytest.approx(0.0045)
    a, b, c = (P[tri[:, k]] for k in range(3))
    assert (np.cross(b - a, c - a)[:, 2] > 0).all()  # wound along the outward normal
    # the trap: the winding of surface_triangles() looks inward on this mesh - its "+z" faces are the back face
    st = UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T)).surface_triangles()
    a, b, c = (P[st[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    wound = st[n[:, 2] / np.linalg.norm(n, axis=1) > 0.5]
    assert len(wound) == 160 and np.all(P[wound][..., 2] == 0.0)


def test_contact_face_of_the_turned_ball_scene_pad():
    from tacex_amd.height_map_source import contact_face_triangles
    from tacex_amd.simulation_approaches.fem_based.sim.tactile_sensor_uipc import quat_to_matrix
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    import torch

    P, T = gelpad_box_mesh(8, 10, 4)
    Pw = P * np.array([1.0, -1.0, -1.0]) + np.array([-0.0096, 0.0131, 0.0215])  # FemBallScene's placement: turned by pi about x
    axis = quat_to_matrix(torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64))[:, 2].numpy()  # camera_pose()'s ROS quaternion
    tri = contact_face_triangles(Pw, T, axis)
    assert tri.shape == (160, 3) and np.all(Pw[tri][..., 2] == Pw[:, 2].min())
    assert len(np.unique(tri)) == 9 * 11


def test_deformed_mesh_abi_rejects_bad_arguments_without_a_gpu():
    from tacex_amd import _lib

    lib = _lib.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    good = dict(x=p, V=8, ids=p, Vs=4, tris=p, T=2, pos=p, rot=p, fx=340.0, fy=325.0, cx=160.0, cy=125.0, near=0.024, far=0.029,
                depth=p, B=1, H=8, W=8)

    def call(**kw):
        a = {**good, **kw}
        return lib.tacex_depth_from_deformed_mesh(a["x"], a["V"], a["ids"], a["Vs"], a["tris"], a["T"], a["pos"], a["rot"], a["fx"], a["fy"],
                                                  a["cx"], a["cy"], a["near"], a["far"], a["depth"], a["B"], a["H"], a["W"], None)

    for k in ("x", "ids", "tris", "pos", "rot", "depth"):
        assert call(**{k: None}) == 2 and b"null" in lib.tacex_last_error()
    for k in ("V", "Vs", "T", "B", "H", "W"):
        assert call(**{k: 0}) == 2 and b"counts" in lib.tacex_last_error()
    assert call(Vs=9) == 2  # more surface vertices than the mesh has
    for near, far in ((0.029, 0.024), (0.024, 0.024), (-0.001, 0.029), (float("nan"), 0.029)):
        assert call(near=near, far=far) == 2 and b"clipping" in lib.tacex_last_error()


# -- GPU ------------------------------------------------------------------------------------------------------------------------
def _rot(ax, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def _source(fem, res=(320, 240), cam=CAM_C4, quat=QUAT_ID):
    from tacex_amd import FemSurfaceDepthSource

    return FemSurfaceDepthSource(fem.gelpad, cam, quat, resolution=res, intrinsics=INTR[res], clipping_range=CLIP)


def _camera_frame_f32(src, x):
    """(B, Vs, 3) float32 camera-frame surface vertices, float64 arithmetic in the kernel's order, rounded once."""
    ids = src.surf_ids.cpu().numpy()
    pos, R = src.pos.cpu().numpy(), src.rot_inv.cpu().numpy()
    out = []
    for b in range(x.shape[0]):
        d = x[b, ids] - pos[b]
        out.append(np.stack([(R[b, i, 0] * d[:, 0] + R[b, i, 1] * d[:, 1]) + R[b, i, 2] * d[:, 2] for i in range(3)], 1).astype(np.float32))
    return np.stack(out)


def _oracle(src, res):
    from oracle.mesh_depth_oracle import pose_rows, render_depth

    W, H = res
    fx, fy, cx, cy = INTR[res]
    pc = _camera_frame_f32(src, src._sim.x.cpu().numpy())
    ident = pose_rows(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0, 0.0]]))
    tris = src.tris.cpu().numpy()
    return np.stack([render_depth(pc[b], tris, ident, fx, fy, cx, cy, CLIP[0], CLIP[1], H, W)[0] for b in range(len(pc))])


def _sensor(fem, B, res=(320, 240), src=None, markers=True, cam=CAM_C4, quat=QUAT_ID):
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.calibration import CALIB_GELSIGHT_MINI
    from tacex_amd.simulation_approaches.fem_based import ManiSkillSimulatorCfg
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg

    W, H = res
    cfg = GelSightSensorCfg(
        num_envs=B, sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=CLIP, depth_source=src),
        data_types=["tactile_rgb", "height_map"] + (["marker_motion"] if markers else []),
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(CALIB_GELSIGHT_MINI), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                          with_shadow=False, tactile_img_res=(W, H), device="cuda:0"),
        marker_motion_sim_cfg=ManiSkillSimulatorCfg(tactile_img_res=(W, H), device="cuda:0", camera_pos_w=cam, camera_quat_w_ros=quat)
        if markers else None,
        device="cuda:0")
    s = GelSightSensor(cfg, gelpad_obj=fem.gelpad)
    s.initialize()
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("res,B", [((320, 240), 6), ((640, 480), 2)])
def test_deformed_pad_depth_equals_oracle_bit_for_bit(res, B):
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    fem = FemGelpad(B, "cuda:0", motion="breathing")
    for i in range(12):
        fem.step(i)
    src = _source(fem, res)
    assert src.tris.shape[0] == 160
    # a different camera pose per env (in place, as a camera following the sensor case would): shifted, tilted, rolled
    c = np.array(CAM_C4)
    poses = [(c, np.eye(3)), (c + [0.0005, -0.0003, 0.0], _rot("x", 3.0)), (c, _rot("y", -4.0) @ _rot("x", 2.0)), (c, _rot("z", 10.0)),
             (c + [0.012, 0.0, 0.0], np.eye(3)),   # half the pad out of view
             (c + [0.0, 0.0, -0.007], np.eye(3))]  # the whole pad beyond the far plane
    if B == 2:
        poses = [poses[2], poses[4]]
    for b, (p, R) in enumerate(poses):
        src.pos[b] = torch.from_numpy(p)
        src.rot_inv[b] = torch.from_numpy(R.T.copy())  # R: camera -> world
    depth = src().cpu().numpy()
    want = _oracle(src, res)
    np.testing.assert_array_equal(np.isfinite(depth), np.isfinite(want))
    m = np.isfinite(want)
    np.testing.assert_array_equal(depth[m], want[m])
    seen = m.reshape(B, -1).sum(1)
    W, H = res
    assert seen[0] > 0.5 * W * H
    if B == 6:
        assert 0.2 * seen[0] < seen[4] < 0.7 * seen[0] and seen[5] == 0
    assert depth[m].min() < 0.0285 - 2e-4  # the indenter has pressed the face towards the camera


@pytest.mark.gpu
def test_rest_state_is_the_gel_plane():
    from oracle.taxim_oracle import TaximOracle
    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 2
    fem = FemGelpad(B, "cuda:0")
    src = _source(fem)
    d = src().cpu().numpy()
    # the pad spans columns 36.2 ... 283.8 and every row; the back face (at the near plane) and the sides are not drawn
    inner = d[:, :, 38:282]
    assert np.isfinite(inner).all() and np.abs(inner - np.float32(0.0285)).max() <= 3e-8  # float32 rounding of 1/z interpolation
    assert not np.isfinite(d[:, :, :35]).any() and not np.isfinite(d[:, :, 286:]).any()
    s = _sensor(fem, B, src=src)
    s.update(dt=0.01, force_recompute=True)
    hm = s.data.output["height_map"].cpu().numpy()
    np.testing.assert_array_equal(hm, np.where(np.isfinite(d), d, np.float32(CLIP[1])) * np.float32(1000.0))
    ind = s.indentation_depth.cpu().numpy()
    # the reference's formula (TS:115-131) on the flat 28.5 mm map: zero up to the float32 rounding of (0.0045 - (min / 1000 - 0.024))
    np.testing.assert_array_equal(ind, TaximOracle.indentation_depth(hm))
    assert (np.abs(ind) <= 1e-5).all()


@pytest.mark.gpu
def test_pressed_pad_through_the_sensor():
    """ManiSkillSimulator markers + Taxim RGB, depth from the pad itself: at the press peak the indentation is the deepest optical-axis
    displacement of the contact face (up to the slope of the mesh across half a pixel), grows with the env's press depth, and the RGB
    frame sees it."""
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 4
    fem = FemGelpad(B, "cuda:0", motion="breathing")
    src = _source(fem)
    s = _sensor(fem, B, src=src)
    s.update(dt=0.01, force_recompute=True)
    rgb0 = s.data.output["tactile_rgb"].clone()
    md0 = s.data.output["marker_motion"].clone()
    for i in range(11):  # c = 0.5 - 0.5 cos(0.3 i): the peak is at i = 10
        fem.step(i)
        s.update(dt=0.01, force_recompute=True)
    ind = s.indentation_depth.cpu().numpy()
    face = np.unique(src.triangles)
    disp = (0.0045 - fem.sim.x[:, face, 2].cpu().numpy()).max(1) * 1000.0  # mm towards the camera
    assert (ind <= disp + 1e-5).all(), (ind, disp)  # (1e-5 mm: float32 rounding of the depth -> indentation pass)
    assert (ind >= disp - 0.05).all(), (ind, disp)
    assert (np.diff(ind) > 0).all() and ind[-1] > 0.3, ind  # fem.depth: 0.4 ... 1.4 mm over the envs
    rgb = s.data.output["tactile_rgb"]
    assert torch.isfinite(rgb).all()
    pressed = torch.from_numpy(ind > 0.1).to(rgb.device)  # (the first env's indenter barely reaches into the barrier zone)
    assert int(pressed.sum()) >= 2
    assert ((rgb - rgb0).abs().amax(dim=(1, 2, 3))[pressed] > 0.02).all()
    assert float((s.data.output["marker_motion"] - md0).abs().max()) > 0.05  # the markers follow the same pad


@pytest.mark.gpu
def test_ball_scene_contact_is_seen_where_the_ball_is():
    from tacex_amd.uipc.gelpad_scene import FemBallScene

    B = 4
    scene = FemBallScene(B, "cuda:0")
    pos, quat = scene.camera_pose()
    src = _source(scene, cam=pos, quat=quat)
    assert src.tris.shape[0] == 160
    s = _sensor(scene, B, src=src, markers=False)
    for i in range(11):
        scene.step(i)
        s.update(dt=0.01, force_recompute=True)
    ind = s.indentation_depth.cpu().numpy()
    assert (ind > 0).all(), ind
    hm = s.data.output["height_map"].cpu().numpy()
    x = scene.sim.x.cpu().numpy()
    ball = scene.sim.q[:, 0].cpu().numpy()  # (B,3) ball centres
    face = np.unique(src.triangles)
    fx, fy, cx, cy = INTR[(320, 240)]
    for b in range(B):
        # the pad's surface is piecewise linear over a 2.6 x 2.5 mm grid: the face vertex nearest the ball's axis is the one the ball
        # pushes furthest towards the camera (the pad looks down, the camera above it: the highest vertex), and the depth minimum
        # lies on that vertex's projection
        fv = x[b, face]
        near_ball = face[np.argmin(np.hypot(fv[:, 0] - ball[b, 0], fv[:, 1] - ball[b, 1]))]
        assert near_ball == face[np.argmax(fv[:, 2])]
        pc = _camera_frame_f32(src, x[b:b + 1])[0][np.searchsorted(src.surf_ids.cpu().numpy(), near_ball)]
        u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
        i, j = np.unravel_index(np.argmin(hm[b]), hm[b].shape)
        assert np.hypot(j + 0.5 - u, i + 0.5 - v) <= 3.0, (b, (i, j), (u, v))
        assert abs(hm[b, i, j] - pc[2] * 1000.0) <= 0.05


@pytest.mark.gpu
def test_fill_equals_depth_source():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 4
    fem = FemGelpad(B, "cuda:0", motion="rolling")
    via_source = _sensor(fem, B, src=_source(fem))
    via_fill = _sensor(fem, B)
    via_fill.set_height_map_source(_source(fem))
    for i in range(8):
        fem.step(i)
        for s in (via_source, via_fill):
            s.update(dt=0.01, force_recompute=True)
        a, b = via_source, via_fill
        assert torch.equal(a.data.output["height_map"], b.data.output["height_map"])
        assert torch.equal(a.optical_simulator._frame_min, b.optical_simulator._frame_min)
        assert torch.equal(a.indentation_depth, b.indentation_depth)
    assert float(via_fill.indentation_depth.min()) > 0.0


@pytest.mark.gpu
def test_render_waits_for_a_step_on_the_side_stream():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 8
    fem = FemGelpad(B, "cuda:0", side_stream=True)
    src = _source(fem)
    s = _sensor(fem, B, src=src)
    for i in range(6):
        fem.step(i)
        s.update(dt=0.01, force_recompute=True)  # renders on the current stream right behind the step's event
        hm = s.data.output["height_map"].clone()
        torch.cuda.synchronize()
        d = src().clone()
        want = torch.where(torch.isfinite(d), d, torch.full_like(d, CLIP[1])) * 1000.0
        assert torch.equal(hm, want), i
    assert fem.sim.step_done is not None
