"""Contact traction image of the FEM pad on the GPU (`fem_traction_image_kernel`, `tacex_traction_image_from_deformed_mesh`,
`FemTractionImage`, `VisionTactileSensorUIPC.traction_image`): the kernel against tests/traction_image_ref.py bit for bit through the C
ABI with synthetic states and forces (both staging limits, the unstaged paths), determinism, the optional depth output, and the physics
of the pressed pad, the sheared pad and the ball scene through the Python interface."""
import functools

import numpy as np
import pytest

from traction_image_ref import render_envs, tilt_and_dent

pytestmark = pytest.mark.gpu

CAM_C4 = (0.010375, 0.012625, -0.024)
QUAT_ID = (1.0, 0.0, 0.0, 0.0)
INTR = {(320, 240): (340.0, 325.0, 160.0, 125.0), (80, 40): (85.0, 54.2, 40.0, 20.8)}
CLIP = (0.024, 0.029)


def _rot(ax, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


# the three camera poses (position, camera -> world rotation): identity, tilted 3 deg about x and rolled 10 deg about z, shifted 12 mm
# (half the pad out of view)
POSES = [(np.array(CAM_C4), np.eye(3)), (np.array(CAM_C4), _rot("z", 10.0) @ _rot("x", 3.0)), (np.array(CAM_C4) + [0.012, 0.0, 0.0], np.eye(3))]


@functools.lru_cache(maxsize=None)
def _mesh(cells):
    """points, contact-face vertex ids, face triangles over those ids, barrier vertex areas of `gelpad_box_mesh(*cells)`."""
    from tacex_amd.height_map_source import contact_face_triangles
    from tacex_amd.uipc.uipc_object import UipcObject, UipcObjectCfg, gelpad_box_mesh

    P, T = gelpad_box_mesh(*cells)
    tri = contact_face_triangles(P, T, [0.0, 0.0, 1.0])
    ids, local = np.unique(tri.reshape(-1), return_inverse=True)
    area = UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T)).surface_vertex_areas()
    return P, ids.astype(np.int32), local.reshape(-1, 3).astype(np.int32), area


def _case(cells, B, seed=0):
    """Synthetic inputs of the C entry point: the tilted and dented pad in every env, normal forces on the surface vertices, one face
    vertex without area and one with a negative area (their traction is zero)."""
    P, ids, tris, area = _mesh(cells)
    rng = np.random.default_rng(seed)
    x = np.repeat(tilt_and_dent(P)[None], B, 0)
    forces = np.where(area[None, :, None] > 0, rng.normal(scale=1e-3, size=(B, len(P), 3)), 0.0)
    area = area.copy()
    area[ids[len(ids) // 2]] = 0.0
    area[ids[len(ids) // 3]] = -1e-6
    pos = np.stack([POSES[b % 3][0] for b in range(B)])
    rot_inv = np.stack([POSES[b % 3][1].T for b in range(B)])
    return dict(x=x, ids=ids, tris=tris, forces=forces, area=area, pos=pos, rot_inv=np.ascontiguousarray(rot_inv))


def _launch(c, res, with_depth=True, depth_fill=None):
    """`tacex_traction_image_from_deformed_mesh` and `tacex_depth_from_deformed_mesh` on the case: traction, depth (or the untouched
    buffer), the depth kernel's image."""
    import torch

    from tacex_amd import _lib

    lib = _lib.load_library()
    W, H = res
    B = len(c["x"])
    dev = "cuda:0"
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("x", "ids", "tris", "forces", "area", "pos", "rot_inv")}
    traction = torch.full((B, H, W, 3), float("nan"), dtype=torch.float32, device=dev)
    depth = torch.full((B, H, W), float("nan") if depth_fill is None else depth_fill, dtype=torch.float32, device=dev)
    depth_only = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    V, Vs, T = c["x"].shape[1], len(c["ids"]), len(c["tris"])
    rc = lib.tacex_traction_image_from_deformed_mesh(
        t["x"].data_ptr(), V, t["ids"].data_ptr(), Vs, t["tris"].data_ptr(), T, t["forces"].data_ptr(), t["area"].data_ptr(),
        t["pos"].data_ptr(), t["rot_inv"].data_ptr(), *INTR[res], *CLIP, traction.data_ptr(), depth.data_ptr() if with_depth else None, B, H, W, st)
    _lib.check(rc, "tacex_traction_image_from_deformed_mesh")
    rc = lib.tacex_depth_from_deformed_mesh(t["x"].data_ptr(), V, t["ids"].data_ptr(), Vs, t["tris"].data_ptr(), T, t["pos"].data_ptr(),
                                            t["rot_inv"].data_ptr(), *INTR[res], *CLIP, depth_only.data_ptr(), B, H, W, st)
    _lib.check(rc, "tacex_depth_from_deformed_mesh")
    torch.cuda.synchronize()
    return traction.cpu().numpy(), depth.cpu().numpy(), depth_only.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_reference(c, res, min_seen):
    W, H = res
    traction, depth, depth_only = _launch(c, res)
    want_depth, winner, want = render_envs(c["x"], c["ids"], c["tris"], c["forces"], c["area"], c["pos"], c["rot_inv"], INTR[res], CLIP, H, W)
    np.testing.assert_array_equal(_bits(depth), _bits(depth_only))  # the depth output is the depth kernel's, bit for bit
    np.testing.assert_array_equal(_bits(depth), _bits(want_depth))
    assert not np.isnan(traction).any()
    assert (_bits(traction[winner < 0]) == 0).all()  # no fragment: +0, 0, 0
    np.testing.assert_array_equal(_bits(traction), _bits(want))
    seen = (winner >= 0).reshape(len(winner), -1).mean(1)
    assert (seen >= min_seen).all() and np.abs(want).max() > 0, seen
    return seen


@pytest.mark.parametrize("cells,res,B", [((4, 5, 2), (80, 40), 3), ((8, 10, 4), (320, 240), 2)])
def test_traction_equals_reference_bit_for_bit(cells, res, B):
    seen = _check_against_reference(_case(cells, B), res, 0.2)
    assert seen[0] > 0.7 and (B < 3 or 0.2 < seen[2] < 0.55)  # the whole pad | half of it


# 46 x 47 = 2162 face vertices: neither projections (2048) nor tractions (1536) are staged; 32 x 48 = 1536: both staged, the most the
# traction staging takes; 29 x 53 = 1537: projections staged, tractions formed per winner
@pytest.mark.parametrize("cells,verts", [((45, 46, 1), 2162), ((31, 47, 1), 1536), ((28, 52, 1), 1537)])
def test_staging_limits_and_the_unstaged_path(cells, verts):
    c = _case(cells, 1)
    assert len(c["ids"]) == verts and len(c["tris"]) == 2 * cells[0] * cells[1]
    _check_against_reference(c, (80, 40), 0.7)


def test_two_launches_and_two_envs_with_the_same_state_are_bit_equal():
    c = _case((4, 5, 2), 4)
    for k in ("forces", "pos", "rot_inv"):  # env 3 = env 1 (the tilted and rolled camera), env 2 = env 0
        c[k][3], c[k][2] = c[k][1], c[k][0]
    a, da, _ = _launch(c, (80, 40))
    b, db, _ = _launch(c, (80, 40))
    np.testing.assert_array_equal(_bits(a), _bits(b))
    np.testing.assert_array_equal(_bits(da), _bits(db))
    np.testing.assert_array_equal(_bits(a[3]), _bits(a[1]))
    np.testing.assert_array_equal(_bits(a[2]), _bits(a[0]))
    assert np.abs(a[1]).max() > 0 and not np.array_equal(a[0], a[1])


def test_null_depth_writes_the_traction_only():
    c = _case((4, 5, 2), 3)
    with_depth, _, _ = _launch(c, (80, 40))
    without, canary, _ = _launch(c, (80, 40), with_depth=False, depth_fill=-7.0)
    np.testing.assert_array_equal(_bits(with_depth), _bits(without))
    assert (canary == np.float32(-7.0)).all()


# -- physics: the prescribed indenter ----------------------------------------------------------------------------------------------------
def _image(scene, cam=CAM_C4, quat=QUAT_ID, res=(320, 240)):
    from tacex_amd import FemTractionImage

    return FemTractionImage(scene.gelpad, cam, quat, resolution=res, intrinsics=INTR[res], clipping_range=CLIP)


def _project(src, pw, res=(320, 240)):
    """(B,3) world points -> (B,2) pixel coordinates (u, v) and (B,) depth through the source's camera."""
    pos, R = src.pos.cpu().numpy(), src.rot_inv.cpu().numpy()
    pc = np.einsum("bij,bj->bi", R, pw - pos)
    fx, fy, cx, cy = INTR[res]
    return np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1), pc[:, 2]


def _cell_diagonal_px(src, res=(320, 240)):
    """One mesh cell's diagonal on the contact face in pixels, at the rest depth of the face (the interpolant peaks at a vertex)."""
    P = src._sim.uipc_objects[0].points[np.unique(src.triangles)]
    dx = np.diff(np.unique(np.round(P[:, 0], 9))).max()
    dy = np.diff(np.unique(np.round(P[:, 1], 9))).max()
    fx, fy, _, _ = INTR[res]
    z = 0.0285
    return float(np.hypot(fx * dx / z, fy * dy / z))


def test_pressed_pad_image():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 3
    fem = FemGelpad(B, "cuda:0", motion="breathing")
    for i in range(11):  # c = 0.5 - 0.5 cos(0.3 i): the press peak is at i = 10
        fem.step(i)
    src = _image(fem)
    src.depth.fill_(-7.0)
    img = src().clone()
    assert (src.depth == -7.0).all()  # with_depth=False leaves the depth image alone
    w = fem.contact_forces(per_vertex=True)
    assert torch.equal(img, src.render(w.vertex_forces, with_depth=True))
    t, depth = img.cpu().numpy(), src.depth.cpu().numpy()
    n = w.num_contacts.cpu().numpy()
    assert (n > 0).sum() >= 2, n
    assert (t[..., 2] <= 0).all()
    assert (t[~np.isfinite(depth)] == 0).all() and (t[n == 0] == 0).all()
    uv, _ = _project(src, fem.ind[:, 1:4].cpu().numpy())
    diag = _cell_diagonal_px(src)
    assert 35.0 < diag < 50.0
    fx, fy, _, _ = INTR[(320, 240)]
    face = np.unique(src.triangles)
    vf = w.vertex_forces.cpu().numpy()
    peak = np.abs(t[..., 2]).reshape(B, -1).max(1)
    for b in np.nonzero(n > 0)[0]:
        i, j = np.unravel_index(np.argmax(np.abs(t[b, :, :, 2])), t.shape[1:3])
        assert np.hypot(j + 0.5 - uv[b, 0], i + 0.5 - uv[b, 1]) <= diag, (b, (i, j), uv[b])
        seen = np.isfinite(depth[b])
        integral = float((t[b][seen][:, 2].astype(np.float64) * depth[b][seen].astype(np.float64) ** 2).sum() / (fx * fy))
        total = float(vf[b, face, 2].sum())
        print(f"env {b}: peak |t_z| {peak[b]:.1f} Pa, image integral {integral:.5e} N, face vertex forces {total:.5e} N, ratio {integral / total:.4f}")
        assert 0.5 < integral / total < 1.5  # units and normalisation: a missing third of the lumped areas or a wrong footprint is 2x off
    assert (np.diff(peak) > 0).all(), peak  # fem.depth grows with the env


def test_shear_follows_the_friction_force():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 2
    fem = FemGelpad(B, "cuda:0", motion="rolling")
    for i in range(8):  # the sphere slides in +x until i = 10
        fem.step(i)
    src = _image(fem)
    t = src(friction=True).clone().cpu().numpy()
    fr = fem.contact_forces().friction_force.cpu().numpy()  # (world = camera axes: identity rotation)
    assert (np.abs(fr[:, 0]) > 0).all()
    for b in range(B):
        contact = t[b, :, :, 2] < 0
        mean_tx = float(t[b][contact][:, 0].mean())
        print(f"env {b}: contact-area mean t_x {mean_tx:.3f} Pa, friction force x {fr[b, 0]:.4e} N, contact pixels {int(contact.sum())}")
        assert contact.sum() > 100 and np.sign(mean_tx) == np.sign(fr[b, 0])
    normal_only = fem.contact_forces(per_vertex=True, friction=False).vertex_forces
    a = src(friction=False).clone()
    assert torch.equal(a, src.render(normal_only))
    assert not np.array_equal(a.cpu().numpy(), t)


# -- the ball scene ---------------------------------------------------------------------------------------------------------------------
def test_ball_scene_image_peaks_over_the_ball():
    from tacex_amd import FemTractionImage
    from tacex_amd.uipc.gelpad_scene import FemBallScene

    B = 2
    scene = FemBallScene(B, "cuda:0")
    pos, quat = scene.camera_pose()
    with pytest.raises(ValueError, match="FemTractionImage renders the deformable object"):
        FemTractionImage(scene.ball, pos, quat)
    with pytest.raises(ValueError, match="FemTractionImage: triangle indices outside"):
        FemTractionImage(scene.gelpad, pos, quat, triangles=[[0, 1, scene.gelpad.num_verts]])
    for i in range(11):
        scene.step(i)
    src = _image(scene, cam=pos, quat=quat)
    assert src.tris.shape[0] == 160
    t = src().clone().cpu().numpy()
    n = scene.contact_forces().num_contacts.cpu().numpy()
    assert (n > 0).any(), n
    uv, _ = _project(src, scene.sim.q[:, 0].cpu().numpy())  # the ball's centre: its lowest-gap point lies on the axis through it
    diag = _cell_diagonal_px(src)
    for b in np.nonzero(n > 0)[0]:
        assert np.abs(t[b]).max() > 0
        i, j = np.unravel_index(np.argmax(np.abs(t[b, :, :, 2])), t.shape[1:3])
        print(f"env {b}: peak t_z {t[b, i, j, 2]:.1f} Pa at {(i, j)}, ball centre at {uv[b]}, contacts {int(n[b])}")
        assert np.hypot(j + 0.5 - uv[b, 0], i + 0.5 - uv[b, 1]) <= diag
        assert t[b, i, j, 2] < 0


# -- the interface ----------------------------------------------------------------------------------------------------------------------
def _plugin(fem, B):
    from test_fem_surface_depth import _sensor

    return _sensor(fem, B).marker_motion_simulator


def test_simulator_traction_image_and_observation():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 2
    fem = FemGelpad(B, "cuda:0", motion="breathing")
    plugin = _plugin(fem, B)
    assert plugin.marker_motion_sim.clipping_range == CLIP  # the sensor cfg's clipping range
    for i in range(8):
        fem.step(i)
    img = plugin.traction_image().clone()
    src = plugin.marker_motion_sim.traction_source
    assert (src.near, src.far, src.W, src.H) == (*CLIP, 320, 240) and (src.fx, src.fy, src.cx, src.cy) == INTR[(320, 240)]
    assert img.shape == (B, 240, 320, 3) and float(img[..., 2].min()) < 0
    assert torch.equal(img, _image(fem)().clone())  # the sensor's camera = the depth source's of tests/test_fem_surface_depth.py
    img2, obs = plugin.traction_image(obs_res=(32, 32))
    assert torch.equal(img2, img) and obs.shape == (B, 32, 32, 3)
    want = torch.nn.functional.interpolate(img.cpu().movedim(3, 1), size=[32, 32], mode="bilinear", antialias=True).movedim(1, 3)
    err, scale = float((obs.cpu() - want).abs().max()), float(img.abs().max())
    print(f"observation: max error {err:.3e} Pa = {err / scale:.2e} of the largest traction")
    assert err <= 1e-5 * scale
    _, obs2 = plugin.marker_motion_sim.traction_image(obs_res=(48, 24))
    assert obs2.shape == (B, 24, 48, 3)


def test_traction_image_waits_for_a_step_on_the_side_stream():
    import torch

    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B = 4
    fem = FemGelpad(B, "cuda:0", side_stream=True)
    plugin = _plugin(fem, B)
    for i in range(5):
        fem.step(i)
        img = plugin.traction_image().clone()  # on the current stream, right behind the step's event
        torch.cuda.synchronize()
        assert torch.equal(img, plugin.traction_image()), i
    assert fem.sim.step_done is not None and float(img.abs().max()) > 0
