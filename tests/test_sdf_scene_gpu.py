"""SDF scenes on the GPU: `tacex_height_map_from_sdf_scene` against its NumPy restatement (tests/sdf_scene_ref.py, written from the
header's contract) bit for bit - height map, frame minimum, indentation depth and contact ranges -, a one-slot scene against
`SdfVolumeSource`, an env alone against the env in a batch, the host layer's checks and placement, and through the sensor."""
import functools

import numpy as np
import pytest
import torch
import depth_pass_ref as dref
import relief_source_ref as R
import sdf_scene_ref as S
import volume_source_ref as V

pytestmark = pytest.mark.gpu

F32 = np.float32
GH, GD = dref.GELPAD_H, dref.GELPAD_DMIN
GEL_TOP, NEAR, FAR, TOL = S.GEL_TOP, S.NEAR, S.FAR, S.TOL
# one tile column; ragged tiles both ways; smaller than a tile; the widest frame
SHAPES = [(24, 32), (30, 40), (9, 4), (8, 2048)]
SLOTS = [1, 3, 8]
STEPS = [1, 8, 32]
B = S.NUM_ENVS


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _library():
    lib = S.library(S.three_volumes())
    for a in lib:
        a.setflags(write=False)
    return lib


@functools.lru_cache(maxsize=None)
def _reference(H, W, K, max_steps):
    vox, vi, vf = _library()
    ids, ops, pose = S.gpu_scene(H, W, K)
    hm = S.height_map(vox, vi, vf, ids, pose, ops, H, W, S.scene_pixmm(H, W), NEAR, FAR, max_steps, TOL)
    hm.setflags(write=False)
    return hm


def _source(n, H, W, K, max_steps=32, volumes=None, pixmm=None):
    from tacex_amd import SdfSceneSource, SdfVolume

    vols = [SdfVolume(*v) for v in S.three_volumes()] if volumes is None else volumes
    return SdfSceneSource(vols, n, "cuda", num_slots=K, pixmm=S.scene_pixmm(H, W) if pixmm is None else pixmm, gel_top_mm=GEL_TOP,
                          near_clip_mm=NEAR, far_clip_mm=FAR, max_steps=max_steps, tol_mm=TOL)


def _load(src, ids, ops, pose):
    src.part_ids.copy_(torch.from_numpy(ids))
    src.part_ops.copy_(torch.from_numpy(ops))
    src.part_pose.copy_(torch.from_numpy(pose))


def _outputs(n, H, W, guard=0):
    hm = torch.full((n + guard, H, W), -3.0, device="cuda")
    fmin, ind = torch.full((n + guard,), -1.0, device="cuda"), torch.full((n + guard,), -1.0, device="cuda")
    rows = torch.full((n + guard, 4), -7, dtype=torch.int32, device="cuda")
    return hm, fmin, ind, rows


@pytest.mark.parametrize("max_steps", STEPS)
@pytest.mark.parametrize("K", SLOTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_restatement(H, W, K, max_steps):
    want = _reference(H, W, K, max_steps)
    src = _source(B, H, W, K, max_steps)
    vox, vi, vf = _library()
    assert _same(src.voxels, vox) and _same(src.volumes_i, vi) and _same(src.volumes_f, vf)
    assert (src.part_ids == -1).all().item() and (src.part_ops == 0).all().item() and src.part_pose.shape == (B, K, 16)
    _load(src, *S.gpu_scene(H, W, K))
    hm, fmin, ind, rows = _outputs(B, H, W, guard=1)  # a guard frame and guard entries behind the call's B
    src.fill(hm[:B], fmin[:B], ind[:B], GH, GD, rows=rows[:B])
    got = hm[:B].cpu().numpy()
    for b in range(B):
        bad = np.flatnonzero(got[b].view(np.uint32) != want[b].view(np.uint32))
        assert bad.size == 0, (b, bad.size, [(int(q) // W, int(q) % W, got[b].flat[q], want[b].flat[q]) for q in bad[:4]])
    assert (hm[B] == -3.0).all().item() and fmin[B].item() == -1.0 and ind[B].item() == -1.0 and (rows[B] == -7).all().item()
    rmin, rind, rrows = R.frame_outputs(want, GH, GD)
    assert _same(fmin[:B], rmin) and _same(ind[:B], rind)
    assert np.array_equal(rows[:B].cpu().numpy(), rrows), (rows[:B].cpu().numpy().tolist(), rrows.tolist())
    # without indent and rows: the same map and minimum
    hm2, fmin2 = torch.full((B, H, W), -3.0, device="cuda"), torch.full((B,), -1.0, device="cuda")
    src.fill(hm2, fmin2, None, GH, GD)
    assert _same(hm2, want) and _same(fmin2, rmin)


@pytest.mark.parametrize("max_steps", STEPS)
@pytest.mark.parametrize("H,W", SHAPES + [(250, 320)])
def test_a_one_slot_scene_is_the_volume_source(H, W, max_steps):
    """The required equivalence on the GPU: one union slot with blend 0 - here followed by two empty slots - gives the bits of
    `SdfVolumeSource` on the same volumes, poses and ids, in all four outputs (the scene of tests/test_volume_source_gpu.py)."""
    import test_volume_source_gpu as G
    from tacex_amd import SdfVolume, SdfVolumeSource

    ids, pose = G.IDS, G._poses(H, W)
    n = len(ids)
    vols = [SdfVolume(*v) for v in V.three_volumes()]
    one = SdfVolumeSource(vols, n, "cuda", pixmm=G._pixmm(H, W), gel_top_mm=GEL_TOP, near_clip_mm=NEAR, far_clip_mm=FAR, max_steps=max_steps,
                          tol_mm=TOL)
    one.volume_ids.copy_(torch.from_numpy(ids))
    one.pose.copy_(torch.from_numpy(pose))
    want = _outputs(n, H, W)
    one.fill(want[0], want[1], want[2], GH, GD, rows=want[3])
    assert (want[0] < GEL_TOP).any().item() or max_steps == 1
    for K in (1, 3):
        src = _source(n, H, W, K, max_steps, pixmm=G._pixmm(H, W))
        src.part_ids[:, 0] = torch.from_numpy(ids)
        src.part_pose[:, 0] = torch.from_numpy(pose)
        if K == 3:  # behind it: no volume, and an op that is none
            src.part_pose[:, 1:] = torch.from_numpy(pose)[:, None]
            src.part_ids[:, 2] = 2
            src.part_ops[:, 2] = 3
        got = _outputs(n, H, W)
        src.fill(got[0], got[1], got[2], GH, GD, rows=got[3])
        assert all(_same(g, w) for g, w in zip(got, want)), (K, [i for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)])


def test_an_env_alone_equals_the_env_in_a_batch():
    H, W, K = 30, 40, 8
    ids, ops, pose = S.gpu_scene(H, W, K)
    batch = _source(B, H, W, K)
    _load(batch, ids, ops, pose)
    want = _outputs(B, H, W)
    batch.fill(want[0], want[1], want[2], GH, GD, rows=want[3])
    assert _same(want[0], _reference(H, W, K, 32))
    alone = _source(1, H, W, K)
    for b in range(B):
        _load(alone, ids[b:b + 1], ops[b:b + 1], pose[b:b + 1])
        got = _outputs(1, H, W)
        alone.fill(got[0], got[1], got[2], GH, GD, rows=got[3])
        assert all(_same(g[0], w[b]) for g, w in zip(got, want)), b


def test_fill_checks_its_tensors():
    from tacex_amd import _lib

    n, H, W, K = 2, 24, 32, 3
    src = _source(n, H, W, K)
    hm, fmin, ind = torch.zeros((n, H, W), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    src.fill(hm, fmin, ind, GH, GD)
    assert (hm == FAR).all().item()  # (nothing placed yet: every slot is empty)
    with pytest.raises(ValueError, match="hm must be"):
        src.fill(torch.zeros((n, H, W + 4), device="cuda")[:, :, :W], fmin, ind, GH, GD)  # not contiguous
    with pytest.raises(ValueError, match="hm must be"):
        src.fill(torch.zeros((n + 1, H, W), device="cuda"), fmin, ind, GH, GD)
    with pytest.raises(ValueError, match="frame_min must be"):
        src.fill(hm, fmin.double(), ind, GH, GD)
    with pytest.raises(ValueError, match="rows must be"):
        src.fill(hm, fmin, ind, GH, GD, rows=torch.zeros((n, 4), device="cuda"))
    with pytest.raises(_lib.TacexHipError, match="no CPU fallback"):
        src.fill(torch.zeros((n, H, W)), fmin, ind, GH, GD)
    with pytest.raises(ValueError, match="width = 30"):
        src.fill(torch.zeros((n, H, 30), device="cuda"), fmin, ind, GH, GD)
    # the three tensors the caller writes in place, replaced by something a launch cannot take
    keep = src.part_pose
    for bad in (torch.zeros((n, K + 1, 16), device="cuda")[:, :K], torch.zeros((n, K, 16), dtype=torch.float64, device="cuda"),
                torch.zeros((n, 16), device="cuda"), torch.zeros((n, K, 16))):
        src.part_pose = bad
        with pytest.raises((ValueError, _lib.TacexHipError), match="part_pose"):
            src.fill(hm, fmin, ind, GH, GD)
    src.part_pose = keep
    keep = src.part_ids
    for bad in (torch.zeros((n, K), dtype=torch.int64, device="cuda"), torch.zeros((n, K + 1), dtype=torch.int32, device="cuda"),
                torch.zeros((K, n), dtype=torch.int32, device="cuda").t()):
        src.part_ids = bad
        with pytest.raises(ValueError, match="part_ids must stay"):
            src.fill(hm, fmin, ind, GH, GD)
    src.part_ids = keep
    src.part_ops = torch.zeros((n, K), device="cuda")
    with pytest.raises(ValueError, match="part_ops must stay"):
        src.fill(hm, fmin, ind, GH, GD)
    src.part_ops = torch.zeros((n, K), dtype=torch.int32, device="cuda")
    src.fill(hm, fmin, ind, GH, GD)
    with pytest.raises(ValueError, match="exactly one"):
        src.set_pose(0, 16, 12, (1, 0, 0, 0))
    with pytest.raises(ValueError, match="slot = 3"):
        src.set_pose(3, 16, 12, (1, 0, 0, 0), z_mm=28.0)
    with pytest.raises(ValueError, match="op = 'xor'"):
        src.set_part(0, op="xor")


def test_set_group_pose_composes_the_local_poses():
    """Moving an assembly by T equals writing the composed poses by hand: R = R_T R_local, t = R_T t_local + t_T in float64, sums
    left to right, bit for bit in `part_pose`.  No kernel runs."""
    n, K = 5, 3
    src = _source(n, 240, 320, K, pixmm=0.0295)
    src.set_part(0, volume_id=2, op="union")
    src.set_part(1, volume_id=1, op="subtract")
    src.set_part(2, volume_id=torch.tensor([0, 1, 2, 0, 1]), op=2, env_ids=slice(None))
    assert src.part_ids.cpu().tolist() == [[2, 1, v] for v in (0, 1, 2, 0, 1)] and src.part_ops.cpu().tolist() == [[0, 1, 2]] * n
    quats = torch.tensor([[1.0, 0, 0, 0], [0.9, 0.3, -0.2, 0.25], [0.5, -0.6, 0.4, 0.2], [0.8, -0.25, 0.5, 0.3], [0.3, 0.1, 0.9, -0.2]])
    src.set_pose(0, 150.0, 110.0, quats, press_mm=0.6, scale=1.1)
    src.set_pose(1, torch.tensor([140.0, 150, 160, 170, 180]), 120.0, (0.92, 0.3, 0.2, 0.1), z_mm=28.2, level_mm=0.05, blend_mm=0.3)
    src.set_pose(2, 160.0, 100.0, quats.flip(0), z_mm=torch.tensor([28.0, 28.1, 28.2, 28.3, 28.4]), blend_mm=torch.tensor([0.0, 0.1, 0.2, 0.3, 0.4]))
    local = src.local_pose.cpu().numpy()
    assert _same(src.part_pose, local) and local[0, 1, 14] == F32(0.3) and local[3, 2, 14] == F32(0.3) and local[2, 1, 13] == F32(0.05)
    assert local[1, 0, 9] == F32(150 * 0.0295) and local[4, 1, 11] == F32(28.2)
    # the placement is the volume source's own (one copy of the math)
    from tacex_amd import SdfVolume, SdfVolumeSource
    one = SdfVolumeSource([SdfVolume(*v) for v in V.three_volumes()], n, "cuda", pixmm=0.0295, gel_top_mm=GEL_TOP, near_clip_mm=NEAR,
                          far_clip_mm=FAR)
    one.volume_ids.fill_(2)
    one.set_pose(150.0, 110.0, quats, press_mm=0.6, scale=1.1)
    assert _same(one.pose, local[:, 0])
    group_q = np.array([[0.95, 0.1, -0.2, 0.15], [1.0, 0, 0, 0], [0.7, 0.7, 0, 0], [0.6, -0.3, 0.5, 0.4], [0.2, 0.9, 0.1, -0.3]])
    group_t = np.array([[0.3, -0.2, 0.1], [0, 0, 0], [1.0, 2.0, -0.5], [-0.4, 0.0, 0.25], [0.05, 0.06, 0.07]])
    src.set_group_pose(torch.from_numpy(group_q), torch.from_numpy(group_t))
    want = local.astype(np.float64)
    for e in range(n):
        w, x, y, z = group_q[e]
        w, x, y, z = group_q[e] / np.sqrt(w * w + x * x + y * y + z * z)  # (the norm as the source takes it: squares summed left to right)
        T = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        for k in range(K):
            r = local[e, k].astype(np.float64)
            for i in range(3):
                for j in range(3):
                    want[e, k, 3 * i + j] = T[i][0] * r[j] + T[i][1] * r[3 + j] + T[i][2] * r[6 + j]
                want[e, k, 9 + i] = T[i][0] * r[9] + T[i][1] * r[10] + T[i][2] * r[11] + group_t[e, i]
    got = src.part_pose.cpu().numpy()
    worst = np.abs(got.astype(np.float64) - want).max()
    assert worst <= 2.0 ** -23 * 32 and _same(got[1], local[1])  # (the identity moves nothing)
    assert np.array_equal(got.view(np.uint32), want.astype(F32).view(np.uint32)), worst
    assert _same(src.local_pose, local)  # the local poses stay
    # a subset, with one transform for all of it
    src.set_group_pose((1.0, 0, 0, 0), (0.0, 0.0, 0.5), env_ids=[0, 3])
    after = src.part_pose.cpu().numpy()
    assert _same(after[[1, 2, 4]], got[[1, 2, 4]]) and _same(after[[0, 3], :, :9], local[[0, 3], :, :9])
    assert np.array_equal(after[[0, 3], :, 11], (local[[0, 3], :, 11].astype(np.float64) + 0.5).astype(F32))
    # ids re-drawn on the device: one slot, then all
    g = torch.Generator(device="cuda").manual_seed(5)
    before = src.part_ids.clone()
    ids = src.randomize(slot=1, generator=g)
    assert ids is src.part_ids and torch.equal(ids[:, [0, 2]], before[:, [0, 2]]) and ((ids >= 0) & (ids < 3)).all().item()
    src.randomize(env_ids=[0, 2], generator=g)
    assert torch.equal(src.part_ids[[1, 3, 4]], ids[[1, 3, 4]])
    many = _source(4096, 240, 320, 2, pixmm=0.0295).randomize(generator=g)
    assert many.shape == (4096, 2) and set(many.cpu().reshape(-1).tolist()) == {0, 1, 2}


# ---- through the sensor -----------------------------------------------------------------------------------------------------------
PIX = 0.0295
SH, SW = 240, 320


@functools.lru_cache(maxsize=None)
def _parts():
    from tacex_amd.utils import sdf_volumes as Vol

    return (Vol.box((6.0, 4.0, 1.0), 0.1), Vol.sphere(1.0, 0.05), Vol.hex_nut(3.0, 1.6, 1.2, 0.1), Vol.capsule(0.5, 2.0, 0.1))


def _sensor_scene(with_hole=True):
    """Five envs of three slots: 0 a plate with a round hole; 1 the bare plate (the hole's slot empty); 2 a nut and a peg through its
    bore, moved as an assembly; 3 a capsule blended onto a ball; 4 nothing."""
    src = _source(5, SH, SW, 3, volumes=list(_parts()), pixmm=PIX)
    flat = (1.0, 0.0, 0.0, 0.0)
    src.set_part(0, volume_id=torch.tensor([0, 0, 2, 1, -1]), op="union")
    src.set_part(1, volume_id=torch.tensor([1, -1, 3, 3, -1]), op=torch.tensor([1, 1, 0, 0, 0]))
    src.set_pose(0, torch.tensor([160.0, 160.0, 150.0, 170.0, 160.0]), 120.0, torch.tensor([flat, flat, (0.96, 0.2, 0.15, 0.1), flat, flat]),
                 press_mm=torch.tensor([0.5, 0.5, 0.6, 0.7, 0.5]), scale=torch.tensor([1.0, 1.0, 1.0, 1.5, 1.0]))
    # the hole: a ball of radius 1 mm centred on the plate's near face; the peg: the capsule turned upright, with the nut's rotation
    near_face = src.part_pose[0, 0, 11].item() - 0.5
    src.set_pose(1, 175.0, 125.0, flat, z_mm=near_face, env_ids=[0, 1])
    src.set_pose(1, 150.0, 120.0, (0.7, 0.15, 0.68, 0.1), z_mm=src.part_pose[2, 0, 11].item() - 0.3, env_ids=[2])
    src.set_pose(1, 190.0, 130.0, (0.9, 0.1, 0.3, 0.3), z_mm=src.part_pose[3, 0, 11].item() - 0.6, blend_mm=0.5, env_ids=[3])
    src.part_pose[3, 0, 14] = 0.5
    src.local_pose[3, 0, 14] = 0.5
    return src


def _ref_map(src):
    return S.height_map(src.voxels.cpu().numpy(), src.volumes_i.cpu().numpy(), src.volumes_f.cpu().numpy(), src.part_ids.cpu().numpy(),
                        src.part_pose.cpu().numpy(), src.part_ops.cpu().numpy(), SH, SW, PIX, NEAR, FAR, src.max_steps, TOL)


def test_sensor_takes_its_height_map_from_the_scene(calib_dir):
    import test_volume_source_gpu as G

    n = 5
    src = _sensor_scene()
    s, plain = G._sensor(calib_dir, n), G._sensor(calib_dir, n)
    plain.initialize()
    s.set_height_map_source(src)

    def step():
        s.update(0.01, force_recompute=True)
        a = G._snapshot(s)
        want = _ref_map(src)
        assert _same(a["height_map"], want)
        plain.set_height_map(torch.from_numpy(want.copy()).cuda())
        plain.update(0.01, force_recompute=True)
        b = G._snapshot(plain)
        assert all(_same(a[k], b[k]) for k in a), [k for k in a if not _same(a[k], b[k])]
        sim = s.optical_simulator
        assert sim._frame_rows_version == s._height_map_version == sim._frame_min_version  # the band-lean path: ranges from the fill
        assert torch.equal(sim._frame_rows, plain.optical_simulator._frame_rows)
        return a, want

    a, want = step()
    touching = (want < F32(GEL_TOP)).reshape(n, -1).sum(1)
    assert (touching[:4] >= 500).all() and touching[4] == 0, touching
    assert (a["indentation_depth"][:4] > 0.3).all().item() and a["indentation_depth"][4].item() == 0
    # the plate with the hole against the bare plate: they differ inside the hole, and agree further from it than the blur reaches
    # (the levels k = 61, 33, 17, 9, 5, 3, 5 of a 320 x 240 frame in a row: 63 pixels; 80 here)
    yy, xx = np.meshgrid(np.arange(SH), np.arange(SW), indexing="ij")
    rho = np.hypot(xx - 175.0, yy - 125.0) * PIX
    inside, away = torch.from_numpy(rho < 0.7).cuda(), torch.from_numpy(rho > 1.0 + 80 * PIX).cuda()
    hole, bare = a["height_map"][0], a["height_map"][1]
    assert (hole[inside] > bare[inside] + 0.2).all().item() and _same(hole[away], bare[away]) and away.sum().item() > 10000
    rgb0, rgb1 = a["tactile_rgb"][0], a["tactile_rgb"][1]
    assert (rgb0[inside] != rgb1[inside]).any().item() and _same(rgb0[away], rgb1[away])
    assert all((a["tactile_rgb"][b] != a["tactile_rgb"][4]).any().item() for b in range(4))  # (env 4 presses nothing: the no-contact frame)
    # the assembly of env 2 moved as one body between two updates
    src.set_group_pose((0.98, 0.0, 0.0, 0.2), (0.3, -0.2, -0.1), env_ids=[2])
    b, _ = step()
    assert not _same(b["height_map"][2], a["height_map"][2]) and not _same(b["tactile_rgb"][2], a["tactile_rgb"][2])
    assert _same(b["height_map"][0], a["height_map"][0]) and _same(b["tactile_rgb"][0], a["tactile_rgb"][0])
