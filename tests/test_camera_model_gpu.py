"""Sensor camera model on the GPU: `tacex_camera_model` against its NumPy restatement (tests/camera_model_ref.py, written from the
header's contract), bit for bit - float32 and uint8 output, the 16-byte path and the scalar path, partial last groups, frames of one
and of several workgroups, batch independence, time behaviour, in place, identity ids, NULL ids, and through the sensor."""
import numpy as np
import pytest
import torch
from camera_model_ref import camera_batch, profile_row

pytestmark = pytest.mark.gpu

MIX = [[0.92, 0.06, 0.02], [0.03, 0.90, 0.05], [-0.02, 0.08, 1.05]]
OFFSET = [0.015, -0.01, 0.005]
# identity; colour mixing + offset + read and shot noise; the same with a fixed pattern
ROWS = np.stack([profile_row(), profile_row(MIX, OFFSET, 0.02, 2e-3), profile_row(MIX, OFFSET, 0.02, 2e-3, 0.03)])
SEED = 2 ** 35 + 991


def _profiles():
    from tacex_amd import CameraProfile

    return [CameraProfile.identity(), CameraProfile(MIX, OFFSET, 0.02, 2e-3), CameraProfile(MIX, OFFSET, 0.02, 2e-3, 0.03)]


def _model(B, dtype, ids=None, frame_offset=0, profiles=None):
    from tacex_amd import TactileCameraModel

    m = TactileCameraModel(_profiles() if profiles is None else profiles, B, "cuda", seed=SEED, dtype=dtype, frame_offset=frame_offset)
    if profiles is None:
        assert np.array_equal(m.profiles.cpu().numpy(), ROWS)
    if ids is not None:
        m.profile_ids.copy_(torch.tensor(ids, dtype=torch.int32))
    return m


def _input(B, H, W, seed):
    """uniform in [-0.1, 1.1]: both clamps act"""
    return (np.random.default_rng(seed).random((B, H, W, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)


def _same_bits(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape
    if g.dtype == np.float32:
        g, want = g.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g.ravel() != want.ravel())
    assert bad.size == 0, f"{bad.size} of {g.size} values differ, first at flat index {bad[:5]}"


DTYPES = [torch.float32, torch.uint8]


# 24x32: the vector path (H W a multiple of 4, aligned pointers), one workgroup per frame; 40x64: the same in 3 workgroups per frame (the
# last one partly idle); 33x33 (1089 pixels, a partial last group): the scalar path in 2 workgroups per frame; 6x6: 36 pixels, a
# multiple of 4 but not of 16 - frames of a uint8 output start 4-byte aligned only
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
@pytest.mark.parametrize("H, W", [(24, 32), (40, 64), (33, 33), (6, 6)])
def test_batch_of_three_profiles(H, W, dtype):
    B, ids, call = 3, [2, 0, 1], 5
    x = _input(B, H, W, 1)
    assert x.min() < 0 and x.max() > 1
    want = camera_batch(x, ROWS, ids, SEED, call, u8=dtype == torch.uint8)
    if dtype == torch.uint8:
        assert want.min() == 0 and want.max() == 255
    else:
        assert want.min() == 0.0 and want.max() == 1.0
    m = _model(B, dtype, ids)
    _same_bits(m(torch.from_numpy(x).cuda(), call=call), want)
    assert m.call == 0  # an explicit call leaves the counter alone


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
@pytest.mark.parametrize("misaligned", [True, False], ids=["misaligned", "aligned"])
@pytest.mark.parametrize("H, W", [(7, 9), (5, 5)])
def test_odd_sizes_unaligned_views_and_guards(H, W, misaligned, dtype):
    """63 and 25 pixels: the last group of a frame is partial.  The input view starts one float into its storage and the output one
    element (uint8: one byte) into its storage: neither is 16-byte aligned.  Nothing outside the output is written."""
    B, ids, call, guard = 2, [2, 1], 1, 64
    n = B * H * W * 3
    x = _input(B, H, W, 2)
    shift = 1 if misaligned else 0
    store_in = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    rgb = store_in[shift:shift + n].view(B, H, W, 3)
    rgb.copy_(torch.from_numpy(x))
    fill = 0xA5 if dtype == torch.uint8 else -7.0
    store_out = torch.full((guard + shift + n + guard,), fill, dtype=dtype, device="cuda")
    out = store_out[guard + shift:guard + shift + n].view(B, H, W, 3)
    assert store_in.data_ptr() % 16 == 0 and store_out.data_ptr() % 16 == 0 and (out.data_ptr() % 16 != 0) == misaligned
    assert (rgb.data_ptr() % 16 != 0) == misaligned
    m = _model(B, dtype, ids)
    res = m(rgb, out=out, call=call)
    assert res.data_ptr() == out.data_ptr()
    _same_bits(out, camera_batch(x, ROWS, ids, SEED, call, u8=dtype == torch.uint8))
    assert (store_out[:guard + shift] == fill).all().item() and (store_out[guard + shift + n:] == fill).all().item()
    assert np.array_equal(rgb.cpu().numpy(), x)  # the input is read only


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
def test_an_image_does_not_depend_on_its_batch(dtype):
    B, H, W, ids = 5, 12, 16, [1, 2, 2, 1, 0]
    x = torch.from_numpy(_input(B, H, W, 3)).cuda()
    whole = _model(B, dtype, ids)(x, call=9)
    part = _model(2, dtype, ids[2:4], frame_offset=2)(x[2:4].contiguous(), call=9)
    assert torch.equal(whole[2:4], part)
    other = _model(2, dtype, ids[2:4], frame_offset=0)(x[2:4].contiguous(), call=9)
    assert not torch.equal(whole[2:4], other)


def test_time_behaviour():
    from tacex_amd import CameraProfile

    B, H, W = 2, 24, 32
    x = torch.full((B, H, W, 3), 0.5, device="cuda")
    m = _model(B, torch.float32, [2, 2])
    a, b = m(x), m(x)  # the counter: call 0, call 1
    assert m.call == 2 and not torch.equal(a, b)
    assert torch.equal(a, m(x, call=0)) and torch.equal(b, m(x, call=1))
    _same_bits(b, camera_batch(x.cpu().numpy(), ROWS, [2, 2], SEED, 1, u8=False))
    # a fixed pattern alone: the same in every call, another one in every frame
    fp = _model(B, torch.float32, [0, 0], profiles=[CameraProfile(fixed_pattern=0.05)])
    c, d = fp(x, call=7), fp(x, call=8)
    assert torch.equal(c, d)
    assert not torch.equal(c[0], c[1]) and not torch.equal(c, x)
    _same_bits(c, camera_batch(x.cpu().numpy(), profile_row(fixed_pattern=0.05)[None], [0, 0], SEED, 7, u8=False))


@pytest.mark.parametrize("H, W", [(24, 32), (7, 9)])
def test_in_place_float32_equals_out_of_place(H, W):
    B, ids = 3, [1, 2, 0]
    x = torch.from_numpy(_input(B, H, W, 4)).cuda()
    m = _model(B, torch.float32, ids)
    want = m(x, call=2)
    y = x.clone()
    res = m(y, out=y, call=2)
    assert res.data_ptr() == y.data_ptr() and torch.equal(y, want) and not torch.equal(y, x)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
def test_ids_outside_the_table_are_the_identity_profile(dtype):
    B, H, W = 3, 24, 32
    x = _input(B, H, W, 5)
    got = _model(B, dtype, [-1, 3, 1])(torch.from_numpy(x).cuda(), call=4)
    clamped = np.clip(x[:2], 0, 1)
    _same_bits(got[:2], np.floor(np.float32(255) * clamped + np.float32(0.5)).astype(np.uint8) if dtype == torch.uint8 else clamped)
    _same_bits(got, camera_batch(x, ROWS, [-1, 3, 1], SEED, 4, u8=dtype == torch.uint8))


def test_null_ids_are_profile_zero():
    from tacex_amd import _lib

    lib = _lib.load_library()
    B, H, W = 2, 24, 32
    x = torch.from_numpy(_input(B, H, W, 6)).cuda()
    prof = torch.from_numpy(ROWS[1:]).cuda()  # row 0: mixing + noise
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
    outs = []
    for ids in (None, zeros):
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
        rc = lib.tacex_camera_model(_lib.ptr(x), _lib.ptr(prof), 2, _lib.ptr(ids), SEED, 0, 3, _lib.ptr(out), 1, B, H, W,
                                    _lib.current_stream_handle(x.device))
        _lib.check(rc, "tacex_camera_model")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    _same_bits(outs[0], camera_batch(x.cpu().numpy(), ROWS[1:], None, SEED, 3, u8=True))


def test_the_tuned_size_240x320_uint8():
    B, H, W, ids = 2, 240, 320, [2, 1]
    x = _input(B, H, W, 7)
    got = _model(B, torch.uint8, ids)(torch.from_numpy(x).cuda(), call=11)
    _same_bits(got, camera_batch(x, ROWS, ids, SEED, 11, u8=True))


def test_offsets_past_2_to_the_31_values():
    """9400 frames of 240 x 320 x 3 = 2.17e9 values (8.7 GB of float32): value indices pass 2^31 and byte offsets 2^32 inside the batch.
    The first and the last frame against the restatement (which addresses a frame by its index alone), uint8 and float32 in place."""
    B, H, W = 9400, 240, 320
    assert B * H * W * 3 > 2 ** 31
    ids = np.ones(B, dtype=np.int32)
    ids[-1] = 2
    x = torch.rand((B, H, W, 3), device="cuda")
    ends = x[[0, B - 1]].cpu().numpy()
    m = _model(B, torch.uint8, ids)
    got = m(x, call=3)
    for k, b in enumerate((0, B - 1)):
        _same_bits(got[b:b + 1], camera_batch(ends[k:k + 1], ROWS, ids[b:b + 1], SEED, 3, u8=True, frame_offset=b))
    del got
    mf = _model(B, torch.float32, ids)
    mf(x, out=x, call=3)
    _same_bits(x[B - 1:], camera_batch(ends[1:], ROWS, ids[B - 1:], SEED, 3, u8=False, frame_offset=B - 1))


def test_python_layer_refuses_bad_tensors():
    from tacex_amd._lib import TacexHipError

    m = _model(2, torch.uint8)
    ok = torch.zeros((2, 8, 8, 3), device="cuda")
    for bad in (ok[:1], ok[..., :2], ok.double(), ok.permute(0, 2, 1, 3)[:, ::2], torch.zeros((2, 8, 8, 4), device="cuda")[..., :3]):
        with pytest.raises(ValueError):
            m(bad)
    with pytest.raises(TacexHipError):
        m(ok.cpu())
    with pytest.raises(ValueError):
        m(ok, out=torch.empty((2, 8, 8, 3), device="cuda"))  # float32 out for a uint8 model
    with pytest.raises(ValueError):
        m(ok, call=-1)
    assert m.call == 0
    g = torch.Generator(device="cuda").manual_seed(3)
    ids = m.randomize(generator=g).clone()
    assert ids.dtype == torch.int32 and ((ids >= 0) & (ids < 3)).all().item()
    m.randomize(env_ids=[1], generator=g)
    assert m.profile_ids[0] == ids[0] and 0 <= int(m.profile_ids[1]) < 3


def test_sensor_camera_image(calib_dir):
    from tacex_amd import GelSightSensor, GelSightSensorCfg, IndenterHeightMapSource
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
    from tacex_amd.utils.synthetic import PIXMM

    B, H, W, ids = 2, 240, 320, [1, 2]
    cfg = GelSightSensorCfg(
        num_envs=B, data_types=["tactile_rgb", "height_map"],
        sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib_dir), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                          tactile_img_res=(W, H), device="cuda"),
        device="cuda")
    s = GelSightSensor(cfg)
    src = IndenterHeightMapSource(B, "cuda", pixmm=PIXMM)
    src.set("sphere", cx=torch.tensor([150.0, 190.0]), cy=torch.tensor([110.0, 130.0]), r=torch.tensor([60.0, 45.0]), press_mm=torch.tensor([0.8, 1.2]))
    s.set_height_map_source(src)
    s.update(0.01, force_recompute=True)
    before = s.data.output["tactile_rgb"].clone()
    assert tuple(before.shape) == (B, H, W, 3) and before.dtype == torch.float32 and float(before.std()) > 0
    m = _model(B, torch.uint8, ids)
    img = s.camera_image(m)
    assert img.dtype == torch.uint8 and m.call == 1
    _same_bits(img, camera_batch(before.cpu().numpy(), ROWS, ids, SEED, 0, u8=True))
    assert torch.equal(s.data.output["tactile_rgb"], before)
    out = torch.empty_like(img)
    assert s.camera_image(m, out=out).data_ptr() == out.data_ptr() and not torch.equal(out, img)  # call 1: other noise
