"""Relief tile library on the GPU: `tacex_height_map_from_relief` against its NumPy restatement (tests/relief_source_ref.py, written
from the header's contract) bit for bit on every route of the launch, its frame minimum, indentation depth and contact ranges against
`tacex_indentation_depth` of the map it wrote, guard frames, refusals, and through the sensor with and without gel memory."""
import functools

import numpy as np
import pytest
import torch
import depth_pass_ref as dref
import relief_source_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GH, GD = dref.GELPAD_H, dref.GELPAD_DMIN
PIX, GEL_TOP, FAR = 0.0295, 28.5, 29.0
# less than one pass of the block (24x32 exact columns, 30x40 not), one float4 per row, 960 threads and several passes, 3 float4s per
# row, w4 = 300 (1024 threads, whole-frame columns), the widest frame the LDS minima take
SHAPES = [(24, 32), (30, 40), (9, 4), (250, 320), (1100, 12), (6, 1200), (8, 2048)]


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _tiles():
    """[(height, pitch_mm, wrap, anchor)]: 1x1, 5x7, 48x64 (rows != cols), a holed tile, a small stamp with an anchor off centre."""
    j, i = np.meshgrid(np.arange(5), np.arange(7), indexing="ij")
    small = (0.2 * (((3 * i + 5 * j) % 11) / 10.0)).astype(F32)
    j, i = np.meshgrid(np.arange(48, dtype=np.float64), np.arange(64, dtype=np.float64), indexing="ij")
    big = (0.08 * (1 + np.sin(0.55 * i) * np.cos(0.37 * j)) + 0.001 * i).astype(F32)  # no symmetry between rows and columns
    j, i = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    holed = (0.05 + 0.1 * (((i * 7 + j * 3) % 13) / 12.0)).astype(F32)
    holed[5:9, 9:12] = -np.inf
    j, i = np.meshgrid(np.arange(9, dtype=np.float64), np.arange(12, dtype=np.float64), indexing="ij")
    stamp = (0.15 * np.exp(-((i - 4) ** 2 + (j - 3) ** 2) / 20.0)).astype(F32)
    return [(np.full((1, 1), 0.05, F32), 0.05, True, None), (small, 0.04, True, None), (big, 0.02, False, None),
            (holed, 0.03, True, None), (stamp, 0.06, False, (3.0, 2.5))]


# One call's envs.  size: the footprint of a finite env (stamp extent or carrier radius) as a share of the frame; chosen per shape below.
#          tile carrier  yaw   press  gain  shift           tilt   kind
ENVS = [(1, 0, 0.4, 0.6, 1.0, (9.3, -12.6), False, "touch"),    # 5x7 wrapping, rotated and scaled, shifted beyond one period
        (2, 0, -0.7, 0.5, 1.0, (0.0, 0.0), True, "finite"),      # 48x64 stamp, rotated, tilted
        (0, 1, 0.0, 0.8, 1.0, (0.0, 0.0), False, "finite"),      # 1x1 tile on a sphere
        (3, 2, 0.3, 0.7, 1.5, (-3.75, 2.5), False, "finite"),    # holed wrapping tile on a cylinder, negative texel coordinates
        (1, 0, 0.0, 5.0, 1.0, (0.5, 0.25), False, "touch"),      # pressed past the case
        (-1, 0, 0.0, 0.5, 1.0, (0.0, 0.0), False, "none"),
        (5, 0, 0.0, 0.5, 1.0, (0.0, 0.0), False, "none"),        # id == P
        (2, 1, 1.1, 0.9, 0.5, (1.5, -0.5), True, "finite"),      # stamp on a sphere, tilted
        (3, 0, 0.0, 0.4, 1.0, (0.3, 0.6), False, "touch"),       # holed tile, plane: holes at far clip inside the contact
        (4, 2, -0.2, 0.6, 2.0, (0.0, 0.0), False, "finite")]     # small stamp on a cylinder
SIZES = (0.8, 0.6, 1.0, 0.45, 1.4, 0.3, 2.0, 0.2)


def _pose(tf, e, H, W, size):
    tile, carrier, yaw, press, gain, shift, tilt, kind = ENVS[e]
    k = min(max(tile, 0), len(tf) - 1)
    cx, cy = 0.5 * W - 0.3, 0.5 * H + 0.2
    scale, radius = 1.7, 0.0
    if not _tiles()[k][2]:  # a stamp: its longer side spans `size` of the frame's shorter side (at least three pixels)
        Th, Tw = _tiles()[k][0].shape
        scale = max(size * min(H, W), 3.0) * PIX / ((max(Th, Tw) - 1) * float(tf[k, 0]))
    if carrier:
        radius = max(0.5 * size * min(H, W), 1.9) * PIX / scale  # (object millimetres: `scale` magnifies carrier and relief alike)
    t = (0.3 / W, -0.2 / H) if tilt else (0.0, 0.0)
    return R.pose_rows(tf, [k], cx, cy, yaw, press, pixmm=PIX, scale=scale, tilt=t, carrier=carrier, radius_mm=radius, gain=gain,
                       shift=shift)[0]


def _conditions(hm, kind):
    touching, empty = int((hm < F32(GEL_TOP)).sum()), int((hm == F32(FAR)).sum())
    return {"touch": touching >= 8, "finite": touching >= 8 and empty >= 1, "none": touching == 0}[kind]


@functools.lru_cache(maxsize=None)
def _scene(H, W):
    """(library, ids, pose, {samples: reference map}): the poses chosen on the CPU so that no env degenerates at this shape - every
    env meant to touch has at least 8 pixels below the gel top, every finite footprint also a pixel at far clip, with 1 and 4 samples."""
    tex, ti, tf = R.library(_tiles())
    ids = np.array([e[0] for e in ENVS], np.int32)
    pose = np.zeros((len(ENVS), 16), F32)
    for e, env in enumerate(ENVS):
        for size in SIZES:
            pose[e] = _pose(tf, e, H, W, size)
            if all(_conditions(R.height_map(tex, ti, tf, ids[e:e + 1], pose[e:e + 1], H, W, GEL_TOP, FAR, s)[0], env[-1]) for s in (1, 4)):
                break
        else:
            raise AssertionError(f"no size in {SIZES} keeps env {e} {env} in its case at {H} x {W}")
    ref = {s: R.height_map(tex, ti, tf, ids, pose, H, W, GEL_TOP, FAR, s) for s in (1, 4)}
    for m in ref.values():
        m.setflags(write=False)
    return (tex, ti, tf), ids, pose, ref


def _source(samples, B=len(ENVS)):
    from tacex_amd import ReliefHeightMapSource, ReliefTile

    src = ReliefHeightMapSource([ReliefTile(*t) for t in _tiles()], B, "cuda", pixmm=PIX, gel_top_mm=GEL_TOP, far_clip_mm=FAR, samples=samples)
    tex, ti, tf = R.library(_tiles())
    assert _same(src.texels, tex) and _same(src.tiles_i, ti) and _same(src.tiles_f, tf)
    return src


def _depth_pass(hm):
    from tacex_amd import _lib

    B, H, W = hm.shape
    fmin, ind = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    rows = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load_library().tacex_indentation_depth(_lib.ptr(hm), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W,
                                                           _lib.current_stream_handle(hm.device)), "tacex_indentation_depth")
    return fmin, ind, rows


def test_the_scene_covers_its_cases():
    """On the reference alone: what the envs of the 250x320 call are meant to exercise is there."""
    (tex, ti, tf), ids, pose, ref = _scene(250, 320)
    hm = ref[1]
    y, x = np.meshgrid(np.arange(250, dtype=F32), np.arange(320, dtype=F32), indexing="ij")
    u3 = pose[3, 0] * x + pose[3, 1] * y + pose[3, 2]
    assert (u3 < -1).any() and (u3 > 1).any()  # negative texel coordinates on a wrapping tile
    assert abs(pose[0, 13]) > 7 and abs(pose[0, 14]) > 5 and pose[0, 13] % 1 and pose[0, 14] % 1  # beyond a period, fractional
    assert abs(np.hypot(pose[0, 0], pose[0, 1]) - 1) > 0.2 and abs(pose[0, 1]) > 0.1  # rotation with scale != 1
    fmin, indent, _ = R.frame_outputs(hm, GH, GD)
    assert fmin[4] < 24.0 and indent[4] == F32(4.5)
    assert (hm[5] == F32(FAR)).all() and (hm[6] == F32(FAR)).all()
    inside = hm[8] < F32(GEL_TOP)
    assert (hm[8] == F32(FAR)).any() and inside.any()  # holes inside a frame that is otherwise in contact
    assert {int(p[10]) for p in pose} == {0, 1, 2} and pose[1, 8] != 0 and pose[7, 9] != 0
    assert not np.array_equal(ref[1], ref[4])


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_reference(H, W, samples):
    _, ids, pose, ref = _scene(H, W)
    want = ref[samples]
    B = len(ENVS)
    src = _source(samples)
    src.relief_ids.copy_(torch.from_numpy(ids))
    src.pose.copy_(torch.from_numpy(pose))
    hm = torch.full((B + 1, H, W), -3.0, device="cuda")  # a guard frame and guard entries behind the call's B
    fmin, ind = torch.full((B + 1,), -1.0, device="cuda"), torch.full((B + 1,), -1.0, device="cuda")
    rows = torch.full((B + 1, 4), -7, dtype=torch.int32, device="cuda")
    src.fill(hm[:B], fmin[:B], ind[:B], GH, GD, rows=rows[:B])
    got = hm[:B].cpu().numpy()
    for b in range(B):
        bad = np.flatnonzero(got[b].view(np.uint32) != want[b].view(np.uint32))
        assert bad.size == 0, (b, ENVS[b], bad.size, [(int(q) // W, int(q) % W, got[b].flat[q], want[b].flat[q]) for q in bad[:4]])
    assert (hm[B] == -3.0).all().item() and fmin[B].item() == -1.0 and ind[B].item() == -1.0 and (rows[B] == -7).all().item()
    # frame minimum, indentation depth and ranges: the reference's, and the depth pass's own for the map the kernel wrote
    rmin, rind, rrows = R.frame_outputs(want, GH, GD)
    assert _same(fmin[:B], rmin) and _same(ind[:B], rind)
    assert np.array_equal(rows[:B].cpu().numpy(), rrows), (rows[:B].cpu().numpy().tolist(), rrows.tolist())
    dmin, dind, drows = _depth_pass(hm[:B].contiguous())
    assert _same(fmin[:B], dmin) and _same(ind[:B], dind) and torch.equal(rows[:B], drows)
    if dref.columns_route(H, W) == "conservative":
        assert (rows[:B, 2] == 0).all().item() and (rows[:B, 3] == W - 1).all().item()
    assert ind[4].item() == 4.5 and fmin[4].item() < 24.0
    # without indent and rows: the same map and minimum
    hm2, fmin2 = torch.full((B, H, W), -3.0, device="cuda"), torch.full((B,), -1.0, device="cuda")
    src.fill(hm2, fmin2, None, GH, GD)
    assert _same(hm2, want) and _same(fmin2, rmin)


def test_refusals_leave_the_buffers_untouched():
    from tacex_amd import _lib

    H, W = 24, 32
    _, ids, pose, _ = _scene(H, W)
    B = len(ENVS)
    src = _source(1)
    src.pose.copy_(torch.from_numpy(pose))
    lib = _lib.load_library()
    hm = torch.full((B, 4096, W + 4), -3.0, device="cuda")  # room for every refused geometry
    fmin, ind = torch.full((B,), -1.0, device="cuda"), torch.full((B,), -1.0, device="cuda")
    rows = torch.full((B, 4), -7, dtype=torch.int32, device="cuda")

    def call(h=H, w=W, samples=1, pose_ptr=None):
        return lib.tacex_height_map_from_relief(
            _lib.ptr(src.texels), _lib.ptr(src.tiles_i), _lib.ptr(src.tiles_f), src.num_tiles, _lib.ptr(src.relief_ids),
            _lib.ptr(src.pose) if pose_ptr is None else pose_ptr, GEL_TOP, FAR, GH, GD, _lib.ptr(hm), _lib.ptr(fmin), _lib.ptr(ind),
            _lib.ptr(rows), B, h, w, samples, _lib.current_stream_handle(hm.device))

    for kw, text in ((dict(w=W + 1), "width = 33"), (dict(samples=2), "samples = 2"), (dict(pose_ptr=0), "null pose_dev"),
                     (dict(h=4096), "4096 x 32")):
        assert call(**kw) == 2, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert (hm == -3.0).all().item() and (fmin == -1.0).all().item() and (ind == -1.0).all().item() and (rows == -7).all().item()
    with pytest.raises(ValueError, match="hm must be"):
        src.fill(hm[:, :H, :W], fmin, ind, GH, GD)  # not contiguous
    with pytest.raises(ValueError, match="rows must be"):
        src.fill(torch.zeros((B, H, W), device="cuda"), fmin, ind, GH, GD, rows=torch.zeros((B, 4), device="cuda"))
    with pytest.raises(_lib.TacexHipError, match="no CPU fallback"):
        src.fill(torch.zeros((B, H, W)), fmin, ind, GH, GD)


# ---- through the sensor -----------------------------------------------------------------------------------------------------------
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


SENSOR_IDS = [1, 2, 0, 3, 4, 5]  # (the last: no such tile)


def _sensor_source(B, H, W):
    src = _source(1, B)
    src.relief_ids.copy_(torch.tensor(SENSOR_IDS, dtype=torch.int32))
    src.set_pose(cx_px=torch.tensor([150.0, 170.0, 120.0, 200.0, 160.0, 160.0]), cy_px=torch.tensor([110.0, 130.0, 100.0, 140.0, 120.0, 120.0]),
                 yaw=torch.tensor([0.4, -0.7, 0.0, 0.3, 0.9, 0.0]), press_mm=torch.tensor([0.6, 0.5, 0.8, 0.7, 0.6, 0.5]),
                 scale=torch.tensor([1.7, 3.0, 1.0, 1.2, 4.0, 1.0]), tilt=(0.0005, -0.0003),
                 carrier=torch.tensor([0.0, 0.0, 1.0, 2.0, 0.0, 0.0]), radius_mm=torch.tensor([0.0, 0.0, 2.0, 1.5, 0.0, 0.0]),
                 gain=1.0, shift_texels=(0.25, -1.5))
    return src


def _ref_map(src, H, W):
    return R.height_map(src.texels.cpu().numpy(), src.tiles_i.cpu().numpy(), src.tiles_f.cpu().numpy(), src.relief_ids.cpu().numpy(),
                        src.pose.cpu().numpy(), H, W, GEL_TOP, FAR, src.samples)


def test_set_pose_follows_its_formulas():
    B, H, W = 6, 240, 320
    src = _sensor_source(B, H, W)
    tf = src.tiles_f.cpu().numpy()
    want = R.pose_rows(tf, SENSOR_IDS, [150.0, 170.0, 120.0, 200.0, 160.0, 160.0], [110.0, 130.0, 100.0, 140.0, 120.0, 120.0],
                       [0.4, -0.7, 0.0, 0.3, 0.9, 0.0], [0.6, 0.5, 0.8, 0.7, 0.6, 0.5], pixmm=PIX, scale=[1.7, 3.0, 1.0, 1.2, 4.0, 1.0],
                       tilt=(0.0005, -0.0003), carrier=[0, 0, 1, 2, 0, 0], radius_mm=[0.0, 0.0, 2.0, 1.5, 0.0, 0.0], shift=(0.25, -1.5))
    # float64 on both sides, one rounding: equal up to the last bit of the device's cos / sin
    np.testing.assert_allclose(src.pose.cpu().numpy(), want, rtol=1e-6, atol=1e-6)
    before = src.pose.clone()
    src.set_pose(100.0, 90.0, 0.0, 1.0, carrier="sphere", radius_mm=3.0, env_ids=[1, 4])
    after = src.pose.cpu().numpy()
    assert np.array_equal(after[[0, 2, 3, 5]], before.cpu().numpy()[[0, 2, 3, 5]])
    assert after[1, 10] == 1.0 and after[4, 11] == 3.0 and after[1, 6] == 1.0


def test_sensor_takes_its_height_map_from_the_reliefs(calib_dir):
    B, H, W = 6, 240, 320
    src = _sensor_source(B, H, W)
    s, plain = _sensor(calib_dir, B), _sensor(calib_dir, B)
    plain.initialize()
    s.set_height_map_source(src)

    def step():
        s.update(0.01, force_recompute=True)
        a = _snapshot(s)
        plain.set_height_map(a["height_map"])
        plain.update(0.01, force_recompute=True)
        b = _snapshot(plain)
        assert all(_same(a[k], b[k]) for k in a), [k for k in a if not _same(a[k], b[k])]
        sim = s.optical_simulator
        assert sim._frame_rows_version == s._height_map_version == sim._frame_min_version  # the band-lean path: ranges from the fill
        assert torch.equal(sim._frame_rows, plain.optical_simulator._frame_rows)
        return a

    a = step()
    want = _ref_map(src, H, W)
    assert _same(a["height_map"], want)
    touching = (want < F32(GEL_TOP)).reshape(B, -1).sum(1)
    assert (touching[:5] >= 8).all() and touching[5] == 0, touching
    assert (a["indentation_depth"][:5] > 0).all().item() and a["indentation_depth"][5].item() == 0
    assert all((a["tactile_rgb"][b] != a["tactile_rgb"][5]).any().item() for b in range(5))  # (env 5 presses nothing)
    # ids written in place, then re-drawn: the next update presses other tiles
    src.relief_ids.copy_(torch.tensor([3, 3, 5, 1, 1, 0], dtype=torch.int32))
    b = step()
    assert _same(b["height_map"], _ref_map(src, H, W)) and not _same(b["height_map"][0], a["height_map"][0])
    assert (b["height_map"][2] == FAR).all().item() and (b["height_map"][5] < GEL_TOP).any().item()
    g = torch.Generator(device="cuda").manual_seed(5)
    ids = src.randomize(generator=g).clone()
    assert ((ids >= 0) & (ids < src.num_tiles)).all().item()
    c = step()
    assert torch.equal(src.relief_ids, ids) and _same(c["height_map"], _ref_map(src, H, W))
    src.randomize(env_ids=[0], generator=g)
    assert torch.equal(src.relief_ids[1:], ids[1:])


def test_pose_written_in_place_moves_the_texture(calib_dir):
    """Identity M on the wrapping 5x7 tile: m02 += 2 and m12 -= 1 shift the map by two columns to the left and one row down."""
    B, H, W = 6, 240, 320
    src = _source(1, B)
    src.relief_ids.fill_(1)
    src.pose[:, 6] = 0.5
    s = _sensor(calib_dir, B)
    s.set_height_map_source(src)
    s.update(0.01, force_recompute=True)
    a = s.data.output["height_map"].clone()
    assert _same(a, _ref_map(src, H, W)) and len(torch.unique(a)) > 5
    src.pose[:, 2] += 2.0
    src.pose[:, 5] -= 1.0
    s.update(0.01, force_recompute=True)
    b = s.data.output["height_map"]
    assert torch.equal(b[:, 1:, :-2], a[:, :-1, 2:]) and not torch.equal(b, a)


def test_sensor_with_gel_memory_keeps_the_imprint(calib_dir):
    from gel_memory_ref import DT, GelMemoryRef, table
    from tacex_amd import GelMemoryProfile, TactileGelMemory

    B, H, W = 6, 240, 320
    profile = [((0.05, 0.0), (0.6, 0.0), 1e-4)]
    src = _sensor_source(B, H, W)
    s, plain = _sensor(calib_dir, B), _sensor(calib_dir, B)
    plain.initialize()
    s.set_height_map_source(src)
    s.set_gel_memory(TactileGelMemory(B, (W, H), [GelMemoryProfile(*profile[0])], terms=1, dt=DT, device="cuda"))
    ref = GelMemoryRef(B, H, W, 1, table(DT, profile), [0] * B)
    for t in range(2):  # pressed, then lifted off
        if t == 1:
            src.relief_ids.fill_(-1)
        raw = _ref_map(src, H, W)
        s.update(0.01, force_recompute=True)
        a = _snapshot(s)
        assert _same(a["height_map"], ref.step(raw)), t
        plain.set_height_map(a["height_map"])
        plain.update(0.01, force_recompute=True)
        b = _snapshot(plain)
        assert all(_same(a[k], b[k]) for k in a), (t, [k for k in a if not _same(a[k], b[k])])
        if t == 0:
            pressed = torch.from_numpy(raw < F32(GEL_TOP)).cuda()
        else:  # the relief is gone, its imprint is not
            assert (raw == F32(FAR)).all()
            dented = a["height_map"] < GEL_TOP
            assert all((dented[e] & pressed[e]).sum().item() >= 8 for e in range(5)) and not (dented & ~pressed).any().item()
            assert (a["indentation_depth"][:5] > 0).all().item()
