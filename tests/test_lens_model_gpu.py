"""Sensor lens model on the GPU: `tacex_lens_model`, `tacex_lens_camera_model` and `tacex_lens_points` against the NumPy restatement
(tests/lens_model_ref.py, written from the header's contract) - the image bit for bit on the vector and the scalar path, partial last
groups, frames of one and of several workgroups, a misaligned output, ids outside the table and NULL ids; the identity; batch
independence; the fused launch against the two launches; points; through the sensor; the Python layer's refusals."""
import numpy as np
import pytest
import torch
from camera_model_ref import profile_row as camera_row
from lens_model_ref import lens_batch, lens_camera_batch, lens_points, profile_row, profile_set

pytestmark = pytest.mark.gpu

SEED = 2 ** 35 + 991
MIX = [[0.92, 0.06, 0.02], [0.03, 0.90, 0.05], [-0.02, 0.08, 1.05]]
OFFSET = [0.015, -0.01, 0.005]
CAMERA_ROWS = np.stack([camera_row(MIX, OFFSET, 0.02, 2e-3), camera_row(MIX, OFFSET, 0.02, 2e-3, 0.03)])  # without / with a fixed pattern


def _rows(W):
    return np.stack([profile_row(**kw) for kw in profile_set(W)])


def _lens(B, W, ids=None):
    from tacex_amd import LensProfile, TactileLensModel

    m = TactileLensModel([LensProfile(**kw) for kw in profile_set(W)], B, "cuda")
    assert np.array_equal(m.profiles.cpu().numpy(), _rows(W))
    if ids is not None:
        m.profile_ids.copy_(torch.tensor(ids, dtype=torch.int32))
    return m


def _camera(B, dtype, ids, frame_offset=0):
    from tacex_amd import CameraProfile, TactileCameraModel

    m = TactileCameraModel([CameraProfile(MIX, OFFSET, 0.02, 2e-3), CameraProfile(MIX, OFFSET, 0.02, 2e-3, 0.03)], B, "cuda", seed=SEED,
                           dtype=dtype, frame_offset=frame_offset)
    m.profile_ids.copy_(torch.tensor(ids, dtype=torch.int32))
    return m


def _input(B, H, W, seed):
    return np.random.default_rng(seed).random((B, H, W, 3), dtype=np.float32)


def _same_bits(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape
    if g.dtype == np.float32:
        g, want = g.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g.ravel() != want.ravel())
    assert bad.size == 0, f"{bad.size} of {g.size} values differ, first at flat index {bad[:5]}"


# 1x1: one pixel, every tap on it; 5x7: 35 pixels, the scalar path with a partial last group; 24x32: the vector path in one workgroup;
# 37x53: 1961 pixels, odd, two workgroups per frame with a ragged tail, scalar; 40x64: the vector path in three workgroups per frame
@pytest.mark.parametrize("H, W", [(1, 1), (5, 7), (24, 32), (37, 53), (40, 64)])
def test_kernel_equals_the_restatement_bit_for_bit(H, W):
    B = 3
    x = _input(B, H, W, 1)
    xd = torch.from_numpy(x).cuda()
    rows = _rows(W)
    for ids in ([0, 1, 2], [3, 4, 5], [2, -1, 99]):  # every profile of the test set; ids outside the table are the identity
        got = _lens(B, W, ids)(xd)
        assert got.dtype == torch.float32
        _same_bits(got, lens_batch(x, rows, ids))
    assert torch.equal(got[1], xd[1]) and torch.equal(got[2], xd[2])
    assert np.array_equal(xd.cpu().numpy(), x)  # the input is read only


def test_null_ids_are_profile_zero():
    from tacex_amd import _lib

    lib = _lib.load_library()
    B, H, W = 2, 24, 32
    x = torch.from_numpy(_input(B, H, W, 2)).cuda()
    rows = _rows(W)[[4, 2]]  # row 0: softness with distortion
    prof = torch.from_numpy(rows).cuda()
    outs = []
    for ids in (None, torch.zeros(B, dtype=torch.int32, device="cuda")):
        out = torch.empty_like(x)
        rc = lib.tacex_lens_model(_lib.ptr(x), _lib.ptr(prof), 2, _lib.ptr(ids), _lib.ptr(out), B, H, W, _lib.current_stream_handle(x.device))
        _lib.check(rc, "tacex_lens_model")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    _same_bits(outs[0], lens_batch(x.cpu().numpy(), rows, None))


def test_misaligned_output_takes_the_scalar_path_and_writes_nothing_else():
    """32 x 33 = 1056 pixels (a multiple of 4), the output base 4 bytes into its storage: not 16-byte aligned."""
    B, H, W, guard, ids = 2, 32, 33, 64, [2, 4]
    n = B * H * W * 3
    x = _input(B, H, W, 3)
    store = torch.full((guard + 1 + n + guard,), -7.0, device="cuda")
    out = store[guard + 1:guard + 1 + n].view(B, H, W, 3)
    assert store.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    m = _lens(B, W, ids)
    res = m(torch.from_numpy(x).cuda(), out=out)
    assert res.data_ptr() == out.data_ptr()
    want = lens_batch(x, _rows(W), ids)
    _same_bits(out, want)
    assert (store[:guard + 1] == -7.0).all().item() and (store[guard + 1 + n:] == -7.0).all().item()
    _same_bits(m(torch.from_numpy(x).cuda()), want)  # the aligned (vector) path: the same bits


def test_the_tuned_size_240x320():
    B, H, W, ids = 2, 240, 320, [2, 4]
    x = _input(B, H, W, 4)
    _same_bits(_lens(B, W, ids)(torch.from_numpy(x).cuda()), lens_batch(x, _rows(W), ids))


@pytest.mark.parametrize("H, W", [(5, 7), (24, 32), (37, 53)])
def test_identity_profile_returns_the_input(H, W):
    from tacex_amd import LensProfile, TactileLensModel

    x = torch.from_numpy(_input(2, H, W, 5)).cuda()
    assert torch.equal(TactileLensModel(LensProfile.identity(), 2, "cuda")(x), x)
    assert torch.equal(_lens(2, W, [0, 0])(x), x)


def test_an_image_does_not_depend_on_its_batch():
    B, H, W, ids = 5, 12, 16, [2, 4, 3, 1, 5]
    x = torch.from_numpy(_input(B, H, W, 6)).cuda()
    whole = _lens(B, W, ids)(x)
    for b in range(B):
        assert torch.equal(whole[b:b + 1], _lens(1, W, ids[b:b + 1])(x[b:b + 1].contiguous()))
    assert not torch.equal(whole[0], whole[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
# (40x64: the fused vector path in three workgroups per frame - it keeps one group per lane, the lens alone does not)
@pytest.mark.parametrize("H, W", [(5, 7), (24, 32), (37, 53), (40, 64)])
def test_fused_launch_equals_the_two_launches_bit_for_bit(H, W, dtype):
    B, lens_ids, off = 3, [2, 4, 3], 1000
    x = _input(B, H, W, 7)
    xd = torch.from_numpy(x).cuda()
    lens = _lens(B, W, lens_ids)
    mid = lens(xd)
    for cam_ids in ([0, 0, 0], [1, 1, 0]):  # without a fixed pattern; with one (and one frame without)
        for call in (0, 7):
            cam = _camera(B, dtype, cam_ids, frame_offset=off)
            two = cam(mid, call=call)
            fused = lens(xd, camera=cam, call=call)
            assert fused.dtype == dtype and cam.call == 0  # an explicit call leaves the counter alone
            assert torch.equal(fused, two)
            _same_bits(fused, lens_camera_batch(x, _rows(W), lens_ids, CAMERA_ROWS, cam_ids, SEED, call, u8=dtype == torch.uint8, frame_offset=off))
    # the running counter: used and advanced by one, as the camera's own __call__ does
    cam, cam2 = _camera(B, dtype, [1, 1, 0], off), _camera(B, dtype, [1, 1, 0], off)
    cam.call = cam2.call = 7
    out = torch.empty((B, H, W, 3), dtype=dtype, device="cuda")
    assert lens(xd, out=out, camera=cam).data_ptr() == out.data_ptr()
    assert cam.call == 8 and torch.equal(out, cam2(mid)) and cam2.call == 8
    assert not torch.equal(lens(xd, camera=cam), out) and cam.call == 9  # call 8: other noise


def _marker_points(B, N, H, W, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(0, W - 1, (B, N)), g.uniform(0, H - 1, (B, N))], -1)


def test_points_equal_the_restatement_and_work_in_place():
    B, N, H, W, ids = 6, 300, 240, 320, [0, 1, 2, 3, 4, 5]  # 300 points: two workgroups per frame, the second partly idle
    p = _marker_points(B, N, H, W, 8)
    p[:, :4] = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]  # the corners
    rows = _rows(W)
    want = np.stack([lens_points(p[b], rows[ids[b]], H, W) for b in range(B)])
    lens = _lens(B, W, ids)
    pd = torch.from_numpy(p).cuda()
    got = lens.distort_points(pd, height=H, width=W)
    assert got.dtype == torch.float64 and got.shape == pd.shape and got.data_ptr() != pd.data_ptr()
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"points: max |kernel - restatement| = {err:.3e} px")
    assert err <= 1e-9
    assert np.array_equal(pd.cpu().numpy(), p)
    assert np.array_equal(got[0].cpu().numpy(), p[0])  # identity
    assert lens.distort_points(pd, out=pd, height=H, width=W).data_ptr() == pd.data_ptr() and torch.equal(pd, got)  # in place
    # ids outside the table: identity
    lens.profile_ids.copy_(torch.tensor([-1, 6, 2, 2, 2, 2], dtype=torch.int32))
    q = torch.from_numpy(p).cuda()
    assert torch.equal(lens.distort_points(q, height=H, width=W)[:2], q[:2])


def test_marker_motion_layout_keeps_its_shape_and_dtype():
    B, M, H, W, ids = 2, 63, 240, 320, [2, 3]
    p = _marker_points(B, 2 * M, H, W, 9).reshape(B, 2, M, 2)
    lens = _lens(B, W, ids)
    with pytest.raises(ValueError):
        lens.distort_points(torch.from_numpy(p).cuda())  # no frame size yet
    lens(torch.zeros((B, H, W, 3), device="cuda"))  # an image sets the size distort_points assumes
    assert lens.image_size == (H, W)
    mm = torch.from_numpy(p.astype(np.float32)).cuda()
    got = lens.distort_points(mm)
    assert got.shape == mm.shape and got.dtype == torch.float32 and got.data_ptr() != mm.data_ptr()
    rows = _rows(W)
    want = np.stack([lens_points(p[b].astype(np.float32).astype(np.float64), rows[ids[b]], H, W) for b in range(B)])
    # (the float64 results agree to 1e-9 px; rounded to float32 they can fall on either side of a tie: one ulp at 320 px is 3e-5)
    np.testing.assert_allclose(got.cpu().numpy(), want.astype(np.float32), rtol=0, atol=3.1e-5)
    out = torch.empty_like(mm)
    assert lens.distort_points(mm, out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)
    got64 = lens.distort_points(torch.from_numpy(p).cuda())  # (B,2,M,2) float64
    assert got64.dtype == torch.float64 and got64.shape == (B, 2, M, 2)
    assert np.abs(got64.cpu().numpy() - np.stack([lens_points(p[b], rows[ids[b]], H, W) for b in range(B)])).max() <= 1e-9


def test_points_move_with_the_image():
    """A 3 x 3 bright blob drawn at marker position p on a dark 48 x 64 frame: after the lens (profile 3) its intensity centroid lies
    within 0.25 px of distort_points(p) - at the centre and near two corners, 6 px inside the frame."""
    H, W = 48, 64
    marks = [(32, 24), (6, 6), (W - 7, H - 7)]  # (x, y)
    B = len(marks)
    img = np.zeros((B, H, W, 3), dtype=np.float32)
    for b, (x, y) in enumerate(marks):
        img[b, y - 1:y + 2, x - 1:x + 2] = 1.0
    lens = _lens(B, W, [2] * B)
    out = lens(torch.from_numpy(img).cuda()).cpu().numpy().astype(np.float64)[..., 0]
    q = lens.distort_points(torch.tensor(marks, dtype=torch.float64, device="cuda").view(B, 1, 2)).cpu().numpy()[:, 0]
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    for b in range(B):
        assert out[b].sum() > 4
        cx, cy = (out[b] * jj).sum() / out[b].sum(), (out[b] * ii).sum() / out[b].sum()
        d = float(np.hypot(cx - q[b, 0], cy - q[b, 1]))
        print(f"blob at {marks[b]}: centroid ({cx:.3f}, {cy:.3f}), distort_points ({q[b, 0]:.3f}, {q[b, 1]:.3f}), distance {d:.3f} px")
        assert d <= 0.25
    assert np.hypot(*(q[1] - np.array(marks[1], dtype=np.float64))) > 0.5  # the lens really moves the corner marker


def test_sensor_lens_image(calib_dir):
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
    from tacex_amd.utils.synthetic import synthetic_depth_maps

    B, H, W = 3, 24, 32

    def sensor(data_types):
        cfg = GelSightSensorCfg(
            num_envs=B, data_types=data_types,
            sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
            optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib_dir), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                              with_shadow=False, tactile_img_res=(W, H), device="cuda"),
            device="cuda")
        return GelSightSensor(cfg)

    s = sensor(["tactile_rgb", "height_map"])
    depth_mm, _ = synthetic_depth_maps(B, H, W, seed=5, flat_fraction=0.0)
    s.set_camera_depth((depth_mm / 1000.0).cuda())
    s.update(0.01, force_recompute=True)
    before = s.data.output["tactile_rgb"].clone()
    assert tuple(before.shape) == (B, H, W, 3) and before.dtype == torch.float32 and float(before.std()) > 0
    lens_ids, cam_ids = [2, 4, 3], [1, 0, 1]
    lens = _lens(B, W, lens_ids)
    img = s.lens_image(lens)
    assert img.dtype == torch.float32 and torch.equal(img, lens(before)) and not torch.equal(img, before)
    _same_bits(img, lens_batch(before.cpu().numpy(), _rows(W), lens_ids))
    cam, cam2 = _camera(B, torch.uint8, cam_ids), _camera(B, torch.uint8, cam_ids)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    fused = s.lens_image(lens, cam, out=out)
    assert fused.data_ptr() == out.data_ptr() and cam.call == 1
    assert torch.equal(fused, lens(before, camera=cam2)) and cam2.call == 1
    assert torch.equal(fused, _camera(B, torch.uint8, cam_ids)(img, call=0))
    assert torch.equal(s.data.output["tactile_rgb"], before)
    with pytest.raises(RuntimeError, match="tactile_rgb"):
        sensor(["height_map"]).lens_image(lens)


def test_python_layer_refuses_bad_tensors():
    from tacex_amd._lib import TacexHipError

    B, W = 2, 8
    lens = _lens(B, W)
    ok = torch.zeros((B, 8, W, 3), device="cuda")
    with pytest.raises(ValueError, match="in place"):
        lens(ok, out=ok)
    for bad in (ok[:1], ok[..., :2], ok.double(), ok.permute(0, 2, 1, 3)[:, ::2], torch.zeros((B, 8, W, 4), device="cuda")[..., :3]):
        with pytest.raises(ValueError):
            lens(bad)
    with pytest.raises(TacexHipError):
        lens(ok.cpu())
    for bad_out in (torch.empty((B, 8, W, 3), dtype=torch.uint8, device="cuda"), torch.empty((B, 4, W, 3), device="cuda")):
        with pytest.raises(ValueError):
            lens(ok, out=bad_out)
    cam = _camera(B, torch.uint8, [0, 1])
    with pytest.raises(ValueError):
        lens(ok, out=torch.empty_like(ok), camera=cam)  # float32 out for a uint8 camera
    with pytest.raises(ValueError, match="frames"):
        lens(ok, camera=_camera(3, torch.uint8, [0, 1, 0]))  # a camera of another num_frames
    with pytest.raises(ValueError):
        lens(ok, camera="camera")
    with pytest.raises(ValueError):
        lens(ok, camera=cam, call=-1)
    with pytest.raises(ValueError):
        lens(ok, call=3)  # a call number without a camera
    assert cam.call == 0
    with pytest.raises(ValueError):
        lens(ok, camera=_camera(B, torch.float32, [0, 1]), out=ok)  # in place is refused for the fused launch too
    pts = torch.zeros((B, 5, 2), dtype=torch.float64, device="cuda")
    for bad in (pts.float(), pts[:1], torch.zeros((B, 5, 3), dtype=torch.float64, device="cuda"), torch.zeros((B, 3, 5, 2), device="cuda"),
                torch.zeros((B, 5, 2), dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            lens.distort_points(bad, height=8, width=W)
    with pytest.raises(TacexHipError):
        lens.distort_points(pts.cpu(), height=8, width=W)
    with pytest.raises(ValueError):
        lens.distort_points(pts, out=torch.empty((B, 5, 2), device="cuda"), height=8, width=W)
    g = torch.Generator(device="cuda").manual_seed(3)
    ids = lens.randomize(generator=g).clone()
    assert ids.dtype == torch.int32 and ((ids >= 0) & (ids < 6)).all().item()
    lens.randomize(env_ids=[1], generator=g)
    assert lens.profile_ids[0] == ids[0] and 0 <= int(lens.profile_ids[1]) < 6
