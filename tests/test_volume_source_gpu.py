"""SDF volume library on the GPU: `tacex_height_map_from_sdf` against its NumPy restatement (tests/volume_source_ref.py, written from
the header's contract) bit for bit, its frame minimum, indentation depth and contact ranges against `tacex_indentation_depth` of the
map, guard frames, and through the sensor."""
import functools

import numpy as np
import pytest
import torch
import depth_pass_ref as dref
import relief_source_ref as R
import volume_source_ref as V

pytestmark = pytest.mark.gpu

F32 = np.float32
GH, GD = dref.GELPAD_H, dref.GELPAD_DMIN
GEL_TOP, NEAR, FAR, TOL = 28.5, 24.0, 29.0, 1e-4
# a tile and a half each way, tiles with idle lanes (30x40), narrower than a wave's patch, many tiles (8 x 32 of 32 x 8), long rows
SHAPES = [(24, 32), (30, 40), (9, 4), (250, 320), (6, 1200), (8, 2048)]
STEPS = [1, 8, 32]
TILT, TURN = (0.9, 0.3, -0.2, 0.25), (0.8, -0.25, 0.5, 0.3)
IDS = np.array([2, -1, 3, 1, 0, 2, 2], np.int32)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pixmm(H, W):
    return 3.0 / min(H, W)  # the frame's shorter side spans 3 mm


def _poses(H, W):
    """(7, 16) float32, in mm about the frame centre; the volumes are those of `V.three_volumes` (half space 2x2x2 at 1 mm, capsule
    5x9x17 at 0.25 mm with step_scale 0.5, unit ball 24^3 at 0.1 mm):
      0 the ball turned, its surface 0.05 mm beyond the far clip, its grid reaching in front of it: taps, no hit
      1 id -1      2 id P
      3 the capsule axis-aligned at four pixels per voxel, straddling the near clip: rays that start inside it, and hits beside them
      4 the half space tilted, magnified 1.2 and inflated by 0.1 mm: cut flat where rays enter its cube below the surface
      5 the ball one frame width to the right: outside the frame
      6 the pressed ball with a NaN in its rotation"""
    pix = _pixmm(H, W)
    c = np.array([0.5 * W * pix, 0.5 * H * pix])
    at = lambda z, dx=0.0: [c[0] + dx, c[1], z]  # noqa: E731
    ball = V.pose_row(V.quat_matrix(TILT), at(GEL_TOP - 0.4 + 1.0))
    nan = ball.copy()
    nan[4] = np.nan
    return np.stack([V.pose_row(V.quat_matrix(TURN), at(FAR + 0.05 + 1.0)), ball, ball,
                     V.pose_row(np.eye(3), at(NEAR + 0.9 * 0.35 * (16.0 * pix)), scale=16.0 * pix),  # (its radius is 0.35 * scale)
                     V.pose_row(V.quat_matrix(TILT), at(28.3), scale=1.2, level_mm=0.1),
                     V.pose_row(V.quat_matrix(TILT), at(GEL_TOP - 0.4 + 1.0, dx=W * pix + 2.0)), nan])


@functools.lru_cache(maxsize=None)
def _library():
    lib = V.library(V.three_volumes())
    for a in lib:
        a.setflags(write=False)
    return lib


@functools.lru_cache(maxsize=None)
def _reference(H, W, max_steps):
    vox, vi, vf = _library()
    hm = V.height_map(vox, vi, vf, IDS, _poses(H, W), H, W, _pixmm(H, W), NEAR, FAR, max_steps, TOL)
    hm.setflags(write=False)
    return hm


def _source(B, H, W, max_steps=32, volumes=None, pixmm=None):
    from tacex_amd import SdfVolume, SdfVolumeSource

    vols = [SdfVolume(*v) for v in V.three_volumes()] if volumes is None else volumes
    return SdfVolumeSource(vols, B, "cuda", pixmm=_pixmm(H, W) if pixmm is None else pixmm, gel_top_mm=GEL_TOP, near_clip_mm=NEAR,
                           far_clip_mm=FAR, max_steps=max_steps, tol_mm=TOL)


def _depth_pass(hm):
    from tacex_amd import _lib

    B, H, W = hm.shape
    fmin, ind = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    rows = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load_library().tacex_indentation_depth(_lib.ptr(hm), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W,
                                                           _lib.current_stream_handle(hm.device)), "tacex_indentation_depth")
    return fmin, ind, rows


def test_the_scene_covers_its_cases():
    """On the restatement alone: what the envs of the 250x320 call are meant to exercise is there."""
    H, W = 250, 320
    vox, vi, vf = _library()
    pose, pix = _poses(H, W), _pixmm(H, W)
    hm = _reference(H, W, 32)
    far, near = F32(FAR), F32(NEAR)

    def alone(e, p=None, ids=None, steps=32):
        stats = {}
        m = V.height_map(vox, vi, vf, IDS[e:e + 1] if ids is None else ids, pose[e:e + 1] if p is None else p, H, W, pix, NEAR, FAR,
                         steps, TOL, stats)[0]
        return m, stats

    assert vi.shape[0] == 3 and IDS[1] == -1 and IDS[2] == 3 and (hm[1] == far).all() and (hm[2] == far).all()
    assert (alone(1, ids=np.array([2], np.int32))[0] < far).sum() > 1000  # (the pose of envs 1 and 2 would press the ball)
    m, st = alone(0)  # beyond the far clip: marched, never hit
    assert (m == far).all() and st["taps"] > 1000 and st["hits"] == 0 and st["grazing"] == 0
    m, st = alone(5)  # outside the frame: no ray meets the grid
    assert (m == far).all() and st["covered"] == 0
    back = pose[5:6].copy()
    back[0, 9] = pose[0, 9]
    assert (alone(5, back)[0] < F32(GEL_TOP)).sum() > 1000
    m, st = alone(3)  # the near clip cuts the interval: depth = near clip where the ray starts inside, hits beside
    assert (m == near).sum() >= 100 and ((m > near) & (m < far)).sum() >= 100 and st["entered_inside"] >= (m == near).sum()
    assert np.array_equal(pose[3, :9].reshape(3, 3), np.eye(3, dtype=F32)) and vf[1, 4] == F32(0.5)
    qx = pose[3, 0] * F32(pix) / (pose[3, 12] * vf[1, 0])
    assert abs(qx - 0.25) < 1e-6  # four pixels per voxel: every fourth column runs through voxel centres
    m, st = alone(4)  # the 2x2x2 volume: marched hits, and rays that enter the cube below the inflated surface
    assert IDS[4] == 0 and vi[0, 1:].tolist() == [2, 2, 2] and pose[4, 12] != 1 and pose[4, 13] != 0
    assert st["entered_inside"] >= 100 and st["hits"] - st["entered_inside"] >= 100 and (m == far).sum() > 1000
    assert np.isnan(pose[6]).sum() == 1 and (hm[6] == far).all()  # the NaN: far clip in that frame only
    clean = pose[6:7].copy()
    clean[0, 4] = pose[1, 4]
    assert (alone(6, clean)[0] < far).sum() > 1000
    one = _reference(H, W, 1)
    assert not np.array_equal(one, _reference(H, W, 8)) and not np.array_equal(_reference(H, W, 8), hm)


@pytest.mark.parametrize("max_steps", STEPS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_restatement(H, W, max_steps):
    want = _reference(H, W, max_steps)
    B = len(IDS)
    src = _source(B, H, W, max_steps)
    vox, vi, vf = _library()
    assert _same(src.voxels, vox) and _same(src.volumes_i, vi) and _same(src.volumes_f, vf)
    src.volume_ids.copy_(torch.from_numpy(IDS))
    src.pose.copy_(torch.from_numpy(_poses(H, W)))
    hm = torch.full((B + 1, H, W), -3.0, device="cuda")  # a guard frame and guard entries behind the call's B
    fmin, ind = torch.full((B + 1,), -1.0, device="cuda"), torch.full((B + 1,), -1.0, device="cuda")
    rows = torch.full((B + 1, 4), -7, dtype=torch.int32, device="cuda")
    src.fill(hm[:B], fmin[:B], ind[:B], GH, GD, rows=rows[:B])
    got = hm[:B].cpu().numpy()
    for b in range(B):
        bad = np.flatnonzero(got[b].view(np.uint32) != want[b].view(np.uint32))
        assert bad.size == 0, (b, bad.size, [(int(q) // W, int(q) % W, got[b].flat[q], want[b].flat[q]) for q in bad[:4]])
    assert (hm[B] == -3.0).all().item() and fmin[B].item() == -1.0 and ind[B].item() == -1.0 and (rows[B] == -7).all().item()
    # frame minimum, indentation depth and ranges: the restated ones, and the depth pass's own for the restatement's map
    rmin, rind, rrows = R.frame_outputs(want, GH, GD)
    assert _same(fmin[:B], rmin) and _same(ind[:B], rind)
    assert np.array_equal(rows[:B].cpu().numpy(), rrows), (rows[:B].cpu().numpy().tolist(), rrows.tolist())
    dmin, dind, drows = _depth_pass(torch.from_numpy(want.copy()).cuda())
    assert _same(fmin[:B], dmin) and _same(ind[:B], dind) and torch.equal(rows[:B], drows)
    # without indent and rows: the same map and minimum
    hm2, fmin2 = torch.full((B, H, W), -3.0, device="cuda"), torch.full((B,), -1.0, device="cuda")
    src.fill(hm2, fmin2, None, GH, GD)
    assert _same(hm2, want) and _same(fmin2, rmin)


def test_fill_checks_its_tensors():
    from tacex_amd import _lib

    B, H, W = 2, 24, 32
    src = _source(B, H, W)
    hm, fmin, ind = torch.zeros((B, H, W), device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    with pytest.raises(ValueError, match="hm must be"):
        src.fill(torch.zeros((B, H, W + 4), device="cuda")[:, :, :W], fmin, ind, GH, GD)  # not contiguous
    with pytest.raises(ValueError, match="rows must be"):
        src.fill(hm, fmin, ind, GH, GD, rows=torch.zeros((B, 4), device="cuda"))
    with pytest.raises(_lib.TacexHipError, match="no CPU fallback"):
        src.fill(torch.zeros((B, H, W)), fmin, ind, GH, GD)
    with pytest.raises(ValueError, match="width = 30"):
        src.fill(torch.zeros((B, H, 30), device="cuda"), fmin, ind, GH, GD)
    with pytest.raises(ValueError, match="exactly one"):
        src.set_pose(16, 12, (1, 0, 0, 0))


# ---- through the sensor -----------------------------------------------------------------------------------------------------------
PIX = 0.0295
SH, SW = 240, 320


def _sensor(calib_dir, B):
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg

    cfg = GelSightSensorCfg(
        num_envs=B, data_types=["tactile_rgb", "height_map"],
        sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(320, 240), clipping_range=(0.020, 0.029)),
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib_dir), gelpad_height=GH, gelpad_to_camera_min_distance=GD,
                                          tactile_img_res=(320, 240), device="cuda"),
        device="cuda")
    return GelSightSensor(cfg)


def _snapshot(s):
    out = s.data.output
    return {k: out[k].clone() for k in ("height_map", "tactile_rgb")} | {"indentation_depth": s.indentation_depth.clone()}


@functools.lru_cache(maxsize=None)
def _parts():
    from tacex_amd.utils import sdf_volumes as S

    return (S.sphere(2.0, 0.1), S.torus(1.6, 0.5, 0.1), S.hex_nut(3.0, 1.6, 1.2, 0.1), S.gear(10, 1.5, 0.5, 1.0, 0.1))


SENSOR_IDS = [0, 1, 2, 3, 4]  # (the last: no such volume)
SENSOR_QUAT = [(1.0, 0.0, 0.0, 0.0), (0.92, 0.3, 0.2, 0.1), (0.9, 0.35, 0.2, -0.15), (0.85, -0.2, 0.4, 0.3), (1.0, 0.0, 0.0, 0.0)]


def _sensor_source(B=5, ids=SENSOR_IDS, quat=SENSOR_QUAT):
    src = _source(B, SH, SW, volumes=list(_parts()), pixmm=PIX)
    src.volume_ids.copy_(torch.tensor(ids, dtype=torch.int32))
    src.set_pose(cx_px=torch.tensor([150.0, 170.0, 120.0, 200.0, 160.0][:B]), cy_px=torch.tensor([110.0, 130.0, 100.0, 140.0, 120.0][:B]),
                 quat_wxyz=torch.tensor(quat), press_mm=torch.tensor([0.8, 0.6, 0.5, 0.7, 0.5][:B]),
                 scale=torch.tensor([1.0, 1.2, 1.0, 1.1, 1.0][:B]), level_mm=torch.tensor([0.0, 0.0, 0.05, 0.0, 0.0][:B]))
    return src


def _ref_map(src):
    return V.height_map(src.voxels.cpu().numpy(), src.volumes_i.cpu().numpy(), src.volumes_f.cpu().numpy(), src.volume_ids.cpu().numpy(),
                        src.pose.cpu().numpy(), SH, SW, PIX, NEAR, FAR, src.max_steps, TOL)


def test_sensor_takes_its_height_map_from_the_volumes(calib_dir):
    B = 5
    src = _sensor_source()
    s, plain = _sensor(calib_dir, B), _sensor(calib_dir, B)
    plain.initialize()
    s.set_height_map_source(src)

    def step():
        s.update(0.01, force_recompute=True)
        a = _snapshot(s)
        want = _ref_map(src)
        assert _same(a["height_map"], want)
        plain.set_height_map(torch.from_numpy(want.copy()).cuda())
        plain.update(0.01, force_recompute=True)
        b = _snapshot(plain)
        assert all(_same(a[k], b[k]) for k in a), [k for k in a if not _same(a[k], b[k])]
        sim = s.optical_simulator
        assert sim._frame_rows_version == s._height_map_version == sim._frame_min_version  # the band-lean path: ranges from the fill
        assert torch.equal(sim._frame_rows, plain.optical_simulator._frame_rows)
        return a, want

    a, want = step()
    touching = (want < F32(GEL_TOP)).reshape(B, -1).sum(1)
    assert (touching[:4] >= 500).all() and touching[4] == 0, touching
    assert (a["indentation_depth"][:4] > 0.3).all().item() and a["indentation_depth"][4].item() == 0
    assert all((a["tactile_rgb"][b] != a["tactile_rgb"][4]).any().item() for b in range(4))  # (env 4 presses nothing: the no-contact frame)
    # the pose written in place between two updates turns the imprint
    src.set_pose(200.0, 140.0, (0.6, 0.1, 0.7, 0.3), press_mm=0.7, scale=1.1, env_ids=[3])
    src.pose[1, 11] -= 0.2  # (and a bare write: the torus 0.2 mm deeper)
    b, want2 = step()
    assert not _same(b["height_map"][3], a["height_map"][3]) and not _same(b["tactile_rgb"][3], a["tactile_rgb"][3])
    assert _same(b["height_map"][0], a["height_map"][0]) and _same(b["tactile_rgb"][0], a["tactile_rgb"][0])
    assert abs((b["indentation_depth"][1] - a["indentation_depth"][1]).item() - 0.2) < 1e-3
    # ids re-drawn on the device
    g = torch.Generator(device="cuda").manual_seed(5)
    ids = src.randomize(generator=g).clone()
    assert ids.device.type == "cuda" and ids.dtype == torch.int32 and ((ids >= 0) & (ids < src.num_volumes)).all().item()
    c, _ = step()
    assert torch.equal(src.volume_ids, ids)
    src.randomize(env_ids=[0], generator=g)
    assert torch.equal(src.volume_ids[1:], ids[1:])
    many = _source(4096, SH, SW, volumes=list(_parts()), pixmm=PIX).randomize(generator=g)
    assert set(many.cpu().tolist()) == {0, 1, 2, 3}


def test_an_env_alone_equals_the_env_in_a_batch(calib_dir):
    batch, alone = _sensor_source(), _sensor_source(1, [SENSOR_IDS[3]], [SENSOR_QUAT[3]])
    alone.pose.copy_(batch.pose[3:4])
    out = []
    for src, B in ((batch, 5), (alone, 1)):
        s = _sensor(calib_dir, B)
        s.set_height_map_source(src)
        s.update(0.01, force_recompute=True)
        out.append(_snapshot(s))
    assert all(_same(out[0][k][3], out[1][k][0]) for k in out[0]), [k for k in out[0] if not _same(out[0][k][3], out[1][k][0])]
    assert (out[1]["height_map"] < GEL_TOP).sum().item() >= 500


def test_set_pose_presses_the_sphere_as_deep_as_asked():
    """`set_pose(press_mm=)` is good to about one voxel pitch (its docstring); what `indent` reports is the exact depth."""
    press = torch.tensor([0.3, 0.8, 1.3, 0.6])
    src = _source(4, SH, SW, volumes=list(_parts()), pixmm=PIX)
    src.set_pose(160.3, 120.7, torch.tensor([[1.0, 0, 0, 0], [0.9, 0.3, -0.2, 0.25], [0.5, -0.6, 0.4, 0.2], [0.8, -0.25, 0.5, 0.3]]),
                 press_mm=press, scale=torch.tensor([1.0, 1.0, 1.0, 1.5]), level_mm=torch.tensor([0.0, 0.0, 0.1, 0.0]))
    hm, fmin, ind = torch.zeros((4, SH, SW), device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    src.fill(hm, fmin, ind, GH, GD)
    got = ind.cpu()
    print("asked", press.tolist(), "indent", got.tolist())
    pitch = torch.tensor([0.1, 0.1, 0.1, 0.15])  # one voxel in camera mm
    assert ((got - press).abs() <= pitch).all(), (got - press).tolist()
    src.set_pose(160.0, 120.0, (1.0, 0, 0, 0), z_mm=30.0, env_ids=[2])  # the anchor's depth given directly
    assert src.pose[2, 11].item() == 30.0 and src.pose[2, 9].item() == pytest.approx(160 * PIX)
