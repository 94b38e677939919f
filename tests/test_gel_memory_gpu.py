"""Gel memory on the GPU: `tacex_gel_memory` against its NumPy restatement (tests/gel_memory_ref.py, written from the header's
contract) over a press / slide / release sequence on every route of the rows pass, its frame minimum, indentation depth and contact
ranges against `tacex_indentation_depth` of the rewritten map, dead frames, batch independence, reset, and through the sensor on the
height-map-source and the camera-depth route."""
import numpy as np
import pytest
import torch
import depth_pass_ref as dref
from gel_memory_ref import DT, IDS, PROFILES, GelMemoryRef, rest_plane, sequence, table

pytestmark = pytest.mark.gpu

GH, GD = dref.GELPAD_H, dref.GELPAD_DMIN
# every route of the rows pass: exact columns (first loop), conservative columns (second loop), W % 4 != 0, npix % 4 == 3, H past the LDS limit
SHAPES = [(250, 320), (37, 640), (50, 16), (30, 40), (50, 70), (7, 9), (2049, 4)]


def _profiles(profiles=PROFILES):
    from tacex_amd import GelMemoryProfile

    return [GelMemoryProfile(t, w, f) for t, w, f in profiles]


def _model(B, H, W, K, ids=None, profiles=PROFILES):
    from tacex_amd import TactileGelMemory

    m = TactileGelMemory(B, (W, H), _profiles(profiles), terms=K, dt=DT, device="cuda")
    assert np.array_equal(m.coefficients.cpu().numpy().view(np.uint32), table(DT, profiles).view(np.uint32))
    if ids is not None:
        m.profile_ids.copy_(torch.tensor(ids, dtype=torch.int32))
    return m


def _depth_pass(hm):
    from tacex_amd import _lib

    B, H, W = hm.shape
    fmin, ind = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    rows = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load_library().tacex_indentation_depth(_lib.ptr(hm), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W,
                                                           _lib.current_stream_handle(hm.device)), "tacex_indentation_depth")
    return fmin, ind, rows


def _apply(model, hm_n, rows=True):
    """One call on a copy of hm_n -> (hm', frame_min, indent, rows) as device tensors."""
    B = hm_n.shape[0]
    hm = torch.from_numpy(np.ascontiguousarray(hm_n)).cuda()
    fmin, ind = torch.full((B,), -1.0, device="cuda"), torch.full((B,), -1.0, device="cuda")
    r = torch.full((B, 4), -7, dtype=torch.int32, device="cuda") if rows else None
    out = model.apply(hm, fmin, ind, r, gelpad_height=GH, gelpad_to_camera_min_distance=GD)
    assert out.data_ptr() == hm.data_ptr()
    return hm, fmin, ind, r


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("H, W", SHAPES)
def test_sequence_against_the_restatement(H, W, K):
    seq = sequence(H, W)
    model, ref = _model(3, H, W, K, IDS), GelMemoryRef(3, H, W, K, table(), IDS)
    lives = []
    for t, hm_n in enumerate(seq):
        hm, fmin, ind, rows = _apply(model, hm_n)
        want = ref.step(hm_n)
        assert _same(hm, want), f"step {t}: the map differs in {np.count_nonzero(_bits(hm) != _bits(want))} pixels"
        assert _same(model.state, ref.state), f"step {t}: the state differs"
        assert _same(model.live, ref.live), (t, model.live.tolist(), ref.live.tolist())
        assert _same(model.imprint(), ref.imprint())
        wmin, wind, wrows = _depth_pass(hm)
        assert _same(fmin, wmin) and _same(ind, wind) and _same(rows, wrows), (t, rows.tolist(), wrows.tolist())
        rmin, rind, rrows = dref.reference_mm(want)  # the restatement's own: exact minimum, ranges inside the reported ones
        assert _same(fmin, rmin) and np.allclose(ind.cpu().numpy(), rind, rtol=0, atol=1e-4)
        got = rows.cpu().numpy()
        hit = rrows[:, 1] >= 0
        assert (got[hit, 0] <= rrows[hit, 0]).all() and (got[hit, 1] >= rrows[hit, 1]).all()
        assert (got[hit, 2] <= rrows[hit, 2]).all() and (got[hit, 3] >= rrows[hit, 3]).all()
        lives.append(ref.live.copy())
    lives = np.stack(lives)
    # the sequence does what it is meant to: an imprint outlives the release, the fast gel is flushed inside it, the unknown id never lives
    assert lives[3, 0] == 1 and lives[5, 0] == 1 and lives[3, 1] == 1 and lives[5, 1] == 0 and not lives[:, 2].any()
    # without the rows buffer: the same map, minimum and depth
    m2 = _model(3, H, W, K, IDS)
    for hm_n in seq[:3]:
        hm2, fmin2, ind2, _ = _apply(m2, hm_n, rows=False)
    r2 = GelMemoryRef(3, H, W, K, table(), IDS)
    for hm_n in seq[:3]:
        want = r2.step(hm_n)
    assert _same(hm2, want) and _same(fmin2, dref.reference_mm(want)[0]) and _same(m2.state, r2.state)


@pytest.mark.parametrize("H, W", [(250, 320), (50, 70), (2049, 4)])
def test_dead_frames_move_no_state(H, W):
    K = 2
    n, s = dref.no_contact(H, W), dref.sphere_dent(H, W)
    hm_n = np.stack([n, s, n])
    model = _model(3, H, W, K, [0, 0, 1])
    model.state.zero_()
    model.live.zero_()
    hm, fmin, ind, rows = _apply(model, hm_n)
    assert _same(hm[0], n) and _same(hm[2], n)
    assert not model.state[0].any().item() and not model.state[2].any().item() and model.live.tolist() == [0, 1, 0]
    ref = GelMemoryRef(3, H, W, K, table(), [0, 0, 1])
    want = ref.step(hm_n)
    assert _same(hm, want) and _same(model.state, ref.state) and model.state[1].any().item()
    wmin, wind, wrows = _depth_pass(hm)
    assert _same(fmin, wmin) and _same(ind, wind) and _same(rows, wrows)
    # "no state byte moves": what stands in a dead frame's state buffer is not even read (the header's rule that live is 1 for a
    # frame with state is broken on purpose here)
    model.state[0].fill_(7.0)
    before = model.state.clone()
    hm, fmin, ind, rows = _apply(model, np.stack([n, n, n]))
    assert _same(model.state[0], before[0]) and _same(hm[0], n) and model.live.tolist() == [0, 1, 0]
    assert not _same(model.state[1], before[1]) and not _same(hm[1], n)  # the live neighbour decays, its map shows the imprint


@pytest.mark.parametrize("H, W", [(250, 320), (30, 40), (7, 9)])
def test_batch_independence_and_repetition(H, W):
    K = 2
    seq = sequence(H, W)
    model = _model(3, H, W, K, IDS)
    batch = []
    for hm_n in seq:
        hm, fmin, ind, rows = _apply(model, hm_n)
        batch.append((hm.clone(), model.state.clone(), model.live.clone(), fmin, ind, rows))
    for b in range(3):
        one = _model(1, H, W, K, [IDS[b]])
        for t, hm_n in enumerate(seq):
            hm, fmin, ind, rows = _apply(one, hm_n[b:b + 1])
            g = batch[t]
            assert _same(hm[0], g[0][b]) and _same(one.state[0], g[1][b]) and one.live[0].item() == g[2][b].item(), (b, t)
            assert _same(fmin[0], g[3][b]) and _same(ind[0], g[4][b]) and _same(rows[0], g[5][b]), (b, t)
    model.reset()
    assert not model.state.any().item() and not model.live.any().item()
    for t, hm_n in enumerate(seq):
        hm, fmin, ind, rows = _apply(model, hm_n)
        g = batch[t]
        assert _same(hm, g[0]) and _same(model.state, g[1]) and _same(model.live, g[2]) and _same(fmin, g[3]) and _same(rows, g[5]), t


def test_reset_clears_only_the_named_envs():
    H, W, K = 30, 40, 2
    s = dref.sphere_dent(H, W)
    model = _model(3, H, W, K, [0, 0, 1])
    _apply(model, np.stack([s, s, s]))
    before = model.state.clone()
    assert model.live.tolist() == [1, 1, 1]
    model.reset([1])
    assert model.live.tolist() == [1, 0, 1] and not model.state[1].any().item()
    assert _same(model.state[0], before[0]) and _same(model.state[2], before[2])
    ids = model.profile_ids.clone()
    g = torch.Generator(device="cuda").manual_seed(3)
    drawn = model.randomize(generator=g)
    assert drawn.data_ptr() == model.profile_ids.data_ptr() and ((drawn >= 0) & (drawn < 2)).all().item() and ids.shape == drawn.shape
    model.reset()
    assert not model.state.any().item() and not model.live.any().item()
    model.dt = DT / 2
    assert np.array_equal(model.coefficients.cpu().numpy(), table(DT / 2))


# ---- through the sensor -----------------------------------------------------------------------------------------------------------
FAST = [((DT / 3.0, 0.0), (0.6, 0.0), 1e-4)]  # flushed three steps after a release
ZERO = [((0.0, 0.0), (0.0, 0.0), 0.0)]
KEYS = ("height_map", "tactile_rgb")


def _sensor(calib_dir, B, camera_bytes=False):
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg

    cfg = GelSightSensorCfg(
        num_envs=B, data_types=["tactile_rgb", "height_map"] + (["camera_depth"] if camera_bytes else []),
        sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(320, 240), clipping_range=(0.020, 0.029)),
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib_dir), gelpad_height=GH, gelpad_to_camera_min_distance=GD,
                                          tactile_img_res=(320, 240), device="cuda"),
        device="cuda")
    return GelSightSensor(cfg)


def _snapshot(s):
    out = s.data.output
    return {k: out[k].clone() for k in KEYS} | {"indentation_depth": s.indentation_depth.clone()}


def _equal(a, b):
    return all(_same(a[k], b[k]) for k in a)


def test_sensor_with_a_height_map_source(calib_dir):
    from tacex_amd import IndenterHeightMapSource, TactileContactModel, ContactGel
    from tacex_amd.height_map_source import KINDS
    from tacex_amd.utils.synthetic import PIXMM

    B, H, W = 2, 240, 320
    mem = _model(B, H, W, 1, [0, 0], FAST)
    sensors = {name: _sensor(calib_dir, B) for name in ("memory", "plain", "zero", "detached")}
    sources = {name: IndenterHeightMapSource(B, "cuda", pixmm=PIXMM) for name in sensors}
    for name, s in sensors.items():
        s.set_height_map_source(sources[name])
    sensors["memory"].set_gel_memory(mem)
    sensors["zero"].set_gel_memory(_model(B, H, W, 2, [0, 0], ZERO))
    sensors["detached"].set_gel_memory(_model(B, H, W, 1, [0, 0], FAST))
    sensors["detached"].set_gel_memory(None)
    ref = GelMemoryRef(B, H, W, 1, table(DT, FAST), [0, 0])
    contact = TactileContactModel([ContactGel(3e4, 1.2e4, 0.6)], B, "cuda", pixmm=PIXMM, grid=(3, 3))
    pressed = None
    lives = []
    for t in range(7):  # press, press elsewhere, then the indenter is gone
        for src in sources.values():
            if t < 2:
                src.set("sphere", cx=torch.tensor([150.0 + 12 * t, 60.0]), cy=torch.tensor([110.0, 130.0 + 9 * t]), r=torch.tensor([60.0, 45.0]),
                        press_mm=torch.tensor([0.8, 1.2]))
            else:
                src.params[:, 0] = KINDS["none"]
        snaps = {}
        for name, s in sensors.items():
            s.update(0.01, force_recompute=True)
            snaps[name] = _snapshot(s)
        assert _equal(snaps["zero"], snaps["plain"]) and _equal(snaps["detached"], snaps["plain"]), t
        raw = snaps["plain"]["height_map"].cpu().numpy()
        want = ref.step(raw)
        assert _same(snaps["memory"]["height_map"], want), t
        assert _same(mem.live, ref.live) and _same(mem.state, ref.state)
        lives.append(ref.live.copy())
        if t == 1:
            pressed = torch.from_numpy(raw < rest_plane()).cuda()
            assert pressed[0].any().item() and pressed[1].any().item()
        if t == 2:  # the first release frame: the imprint shows where the indenter was, and the observables see it
            assert ref.live.all()
            for b in range(B):
                diff = (snaps["memory"]["tactile_rgb"][b] != snaps["plain"]["tactile_rgb"][b]).any(dim=-1)
                assert (diff & pressed[b]).any().item(), b
            assert (snaps["memory"]["indentation_depth"] > 0).all().item() and not snaps["plain"]["indentation_depth"].any().item()
            f = sensors["memory"].contact_field(contact)
            assert (f.contact_area > 0).all().item() and (f.normal_force > 0).all().item()
            assert not sensors["plain"].contact_field(contact).contact_area.any().item()
        if t >= 2 and not ref.live.any():
            assert _equal(snaps["memory"], snaps["plain"]), t
    lives = np.stack(lives)
    assert lives[:3].all() and not lives[6].any(), lives.tolist()  # (the last frame is the no-contact frame again)
    # reset(env_ids) resets the model's state of those envs
    for src in sources.values():
        src.set("sphere", cx=150.0, cy=110.0, r=60.0, press_mm=0.8)
    sensors["memory"].update(0.01, force_recompute=True)
    assert mem.live.tolist() == [1, 1]
    sensors["memory"].reset([1])
    assert mem.live.tolist() == [1, 0] and not mem.state[1].any().item() and mem.state[0].any().item()


def test_sensor_with_a_camera_depth(calib_dir):
    from tacex_amd import GelSightSensorGroup

    B, H, W = 2, 240, 320
    press = np.stack([dref.sphere_dent(H, W), dref.last_row_and_column(H, W)])
    free = np.stack([dref.no_contact(H, W)] * 2)
    steps = [press, np.roll(press, 5, axis=2), free, free, free, free]
    mem = _model(B, H, W, 2, [0, 0], FAST)
    sensors = {name: _sensor(calib_dir, B, camera_bytes=True) for name in ("memory", "plain", "zero", "detached")}
    for s in sensors.values():
        s.initialize()
    assert sensors["plain"]._can_defer_depth_pass()
    sensors["memory"].set_gel_memory(mem)
    sensors["zero"].set_gel_memory(_model(B, H, W, 1, [0, 0], ZERO))
    sensors["detached"].set_gel_memory(mem)
    assert not sensors["detached"]._can_defer_depth_pass() and not sensors["memory"]._can_defer_depth_pass()
    sensors["detached"].set_gel_memory(None)
    assert sensors["detached"]._can_defer_depth_pass()
    ref = GelMemoryRef(B, H, W, 2, table(DT, FAST), [0, 0])
    for t, hm_n in enumerate(steps):
        depth = torch.from_numpy((hm_n / np.float32(1000.0)).astype(np.float32)).cuda()
        snaps = {}
        for name, s in sensors.items():
            s.set_camera_depth(depth)
            s.update(0.01, force_recompute=True)
            snaps[name] = _snapshot(s)
        for name, s in sensors.items():  # the bytes stay those of the raw camera image
            assert _same(s.data.output["camera_depth"], sensors["plain"].data.output["camera_depth"]), (t, name)
        assert sensors["plain"].data.output["camera_depth"].any().item()
        assert _equal(snaps["zero"], snaps["plain"]) and _equal(snaps["detached"], snaps["plain"]), t
        want = ref.step(snaps["plain"]["height_map"].cpu().numpy())
        assert _same(snaps["memory"]["height_map"], want) and _same(mem.live, ref.live), t
        sim = sensors["memory"].optical_simulator
        wmin, wind, wrows = _depth_pass(sensors["memory"].data.output["height_map"])
        assert _same(sim._frame_min, wmin) and _same(sim._indentation_depth, wind) and _same(sim._frame_rows, wrows), t
        if t == 2:
            assert ref.live.all() and not _same(snaps["memory"]["tactile_rgb"], snaps["plain"]["tactile_rgb"])
        if t == 5:
            assert not ref.live.any() and _equal(snaps["memory"], snaps["plain"])
    # set_height_map applies the model too
    s = _sensor(calib_dir, B)
    s.initialize()
    m2 = _model(B, H, W, 1, [0, 0], FAST)
    s.set_gel_memory(m2)
    r2 = GelMemoryRef(B, H, W, 1, table(DT, FAST), [0, 0])
    for hm_n in (press, free):
        s.set_height_map(torch.from_numpy(hm_n).cuda())
        s.update(0.01, force_recompute=True)
        assert _same(s.data.output["height_map"], r2.step(hm_n)) and _same(m2.live, r2.live)
    # a model of another size, and a grouped sensor, are refused
    with pytest.raises(ValueError):
        s.set_gel_memory(_model(B, 30, 40, 1))
    members = [_sensor(calib_dir, B), _sensor(calib_dir, B)]
    GelSightSensorGroup(members)
    with pytest.raises(RuntimeError):
        members[0].set_gel_memory(m2)
