"""Marker pattern library on the GPU (`tacex_fem_marker_flow_library`): every env on a marker pattern and a random stream of
its own, in one launch.  The NumPy restatement of the contract lives in tests/marker_pattern_ref.py; projections are checked against
oracle.fem_oracle.marker_uv.

Scene: the pad of test_fem_gpu.py's marker tests (270 surface vertices), its smooth per-env deformation, camera at (0, 0, -0.024), B <= 8.
Randomised ranges: the first eight patterns of seed 0 have 56, 69, 64, 64, 56, 64, 56, 71 in-image markers (test_marker_patterns.py pins
that on the CPU), so with K = 60 one launch takes both the padding and the subset branch."""
import numpy as np
import pytest
import torch

from marker_pattern_ref import flow_batch, flow_one_env

pytestmark = pytest.mark.gpu

CAM = np.array([0.0, 0.0, -0.024])
RANGES = dict(marker_interval_range=(1.95, 2.15), marker_rotation_range=0.1, marker_translation_range=(1.0, 1.0),
              marker_pos_shift_range=(0.1, 0.1))
IN_IMAGE = [56, 69, 64, 64, 56, 64, 56, 71]
H, W = 240, 320


class Scene:
    """The pad in `B` envs, at rest while sensors are constructed (reference surface = rest shape) and deformed afterwards."""

    def __init__(self, B):
        from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
        from tacex_amd.uipc.uipc_object import gelpad_box_mesh

        P, Tt = gelpad_box_mesh(10, 8, 3, size=(0.030, 0.018, 0.0045))
        self.P = P - np.array([0.011, 0.009, 0.0])
        self.B = B
        self.sim = UipcSim(UipcSimCfg(device="cuda:0"), num_envs=B)
        self.gel = UipcObject(UipcObjectCfg(mesh_points=self.P, mesh_tets=Tt), self.sim)
        self.sim.setup_sim()
        self.rest = self.sim.x.clone()
        x = self.rest.clone()
        for b in range(B):
            x[b, :, 0] += 0.0004 * (b + 1) * torch.sin(300 * x[b, :, 1])
            x[b, :, 2] += 0.0003 * (b + 1) * torch.cos(200 * x[b, :, 0])
        self.x = x
        self.sim.x = x

    def sensor(self, **kw):
        from tacex_amd.simulation_approaches.fem_based.sim.tactile_sensor_uipc import VisionTactileSensorUIPC

        self.sim.x = self.rest
        s = VisionTactileSensorUIPC(self.gel, self.sim, torch.tensor(CAM, dtype=torch.float64), torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64), **kw)
        self.sim.x = self.x
        return s


@pytest.fixture(scope="module")
def scene8():
    return Scene(8)


@pytest.fixture(scope="module")
def lib8(scene8):
    """P = 8 randomised patterns of seed 0 on the 8-env scene; tests set probability / sigma / K / ids / counters themselves."""
    return scene8.sensor(num_markers=60, seed=0, marker_patterns=8, **RANGES)


def _np(t):
    return t.detach().cpu().numpy()


def _projections(ms, ids):
    """The device's noise-free projections of every env on its own pattern through the EXISTING kernel (`tacex_fem_marker_uv`), padded to
    Mmax: initial (reference surface) and current (surface in the camera frame, transformed by torch).  The library launch's initial
    projection has that kernel's arithmetic, so the restatement's mask and initial values come from here bit for bit; its current
    projection has `tacex_fem_marker_flow`'s arithmetic (camera transform inside the kernel): the restatement takes those from the
    launch's own noise-free `curr_marker_uv` output, which `_check_curr` holds against this one."""
    lib = ms.patterns
    B = len(ids)
    init = np.zeros((B, lib.max_markers, 2))
    curr = np.zeros((B, lib.max_markers, 2))
    surf = ms.get_surface_vertices_camera()
    for k in sorted(set(int(i) for i in ids)):
        n = int(lib.count[k])
        iu = _np(ms._project(ms.reference_surface_vertices_camera, lib.tri[k, :n].contiguous(), lib.wgt[k, :n].contiguous()))
        cu = _np(ms._project(surf, lib.tri[k, :n].contiguous(), lib.wgt[k, :n].contiguous()))
        for e in np.where(np.asarray(ids) == k)[0]:
            init[e, :n], curr[e, :n] = iu[e], cu[e]
    return init, curr


def _check_curr(ms, ids, curr_d):
    """`curr_marker_uv` of the last launch: rows >= count zero, the rest equal to the existing kernel's projections to round-off."""
    cuv = _np(ms.curr_marker_uv)
    cnt = _np(ms.patterns.count)
    assert cuv.shape == curr_d.shape
    for e, k in enumerate(ids):
        assert not cuv[e, cnt[k]:].any()
        np.testing.assert_allclose(cuv[e, :cnt[k]], curr_d[e, :cnt[k]], rtol=1e-13)
    return cuv


def _oracle_projections(scene, ms, ids, x=None):
    from oracle.fem_oracle import marker_uv

    lib, surf = ms.patterns, ms.surf_vertex_ids
    tri, wgt, cnt = _np(lib.tri), _np(lib.wgt), _np(lib.count)
    x = _np(scene.x if x is None else x)
    init = np.zeros((len(ids), lib.max_markers, 2))
    curr = np.zeros_like(init)
    for e, k in enumerate(ids):
        n = cnt[k]
        init[e, :n] = marker_uv((scene.P[surf] - CAM)[None], tri[k, :n], wgt[k, :n])[0]
        curr[e, :n] = marker_uv((x[e, surf] - CAM)[None], tri[k, :n], wgt[k, :n])[0]
    return init, curr


def _configure(ms, ids=None, prob=0.0, sigma=0.0, K=60, normalize=False, draws=None):
    if ids is not None:
        ms.set_pattern_ids(ids)
    ms.marker_lose_tracking_probability, ms.marker_random_noise, ms.num_markers, ms.normalize = prob, sigma, K, normalize
    if draws is not None:
        ms.marker_draws.copy_(torch.as_tensor(np.asarray(draws, dtype=np.int64).astype(np.int32)))


def test_library_of_one_equals_the_static_path_bit_for_bit():
    """P = 1 from degenerate ranges, sigma 0, probability 0.  K = 128 (56 in image: padding): flow float64 / float32, pixels / normalised,
    and curr_marker_uv bit-equal to an instance without library.  K = 40 (subset): 40 distinct in-image markers per env, values bit-equal
    to that instance's initial and current projections at those markers, in the restatement's order."""
    sc = Scene(3)
    for norm in (False, True):
        plain = sc.sensor(num_markers=128, normalize=norm)
        libs = sc.sensor(num_markers=128, normalize=norm, marker_patterns=1, seed=5)
        assert libs.patterns.num_patterns == 1 and plain.patterns is None
        a, b = plain.gen_marker_flow_fused(), libs.gen_marker_flow_fused()
        assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape == (3, 2, 128, 2)
        assert torch.equal(a, b)
        assert torch.equal(plain.curr_marker_uv, libs.curr_marker_uv)
        assert _np(libs.num_tracked).tolist() == [56, 56, 56]
        o1, o2 = (torch.zeros((3, 2, 128, 2), dtype=torch.float32, device="cuda:0") for _ in range(2))
        assert plain.gen_marker_flow_fused(out_f32=o1) is o1 and libs.gen_marker_flow_fused(out_f32=o2) is o2
        assert torch.equal(o1, o2) and torch.equal(libs.gen_marker_flow(), a)
        assert float((a[:, 1] - a[:, 0]).abs().max()) > (1.0 if not norm else 1.0 / 160)  # the markers moved
        # subset
        _configure(libs, K=40, normalize=norm, draws=[0, 0, 0])
        f = _np(libs.gen_marker_flow())
        tri, wgt = plain._setup()
        init_uv, idx_dev, idx_host = plain._static_tables(tri, wgt)
        init_uv, curr_uv = _np(init_uv), _np(plain.curr_marker_uv)
        for e in range(3):
            ref, n, chosen = flow_one_env(init_uv[e], curr_uv[e], 5, e, 0, 0.0, 0.0, H, W, 40)
            assert n == 56 and len(set(chosen.tolist())) == 40 and set(chosen.tolist()) <= set(idx_host.tolist())
            want = np.stack([init_uv[e, chosen], curr_uv[e, chosen]])
            if norm:
                want = want / 160.0 - 1.0
            assert np.array_equal(f[e], want)
        assert not np.array_equal(f[0, 0], f[1, 0])  # every env draws a subset of its own (the initial projections are the same)


def test_every_env_follows_its_own_pattern(scene8, lib8):
    """P = 8, B = 8, ids 0..7 and a permuted list with repeats; probability 0.02, sigma 0.5, K = 60, three consecutive calls each."""
    ms, K, seed = lib8, 60, 0
    cnt = _np(ms.patterns.count)
    assert ms.patterns.num_patterns == 8 and 91 <= cnt.min() and cnt.max() <= 120
    worst = 0.0
    branches = set()
    for ids in (list(range(8)), [5, 1, 1, 7, 0, 3, 5, 2]):
        _configure(ms, ids=ids, draws=np.zeros(8))
        init_d, curr_d = _projections(ms, ids)
        init_o, curr_o = _oracle_projections(scene8, ms, ids)
        for e, k in enumerate(ids):  # the device's projections against the float64 oracle (the bound of the existing marker test)
            np.testing.assert_allclose(init_d[e, :cnt[k]], init_o[e, :cnt[k]], rtol=1e-11)
            np.testing.assert_allclose(curr_d[e, :cnt[k]], curr_o[e, :cnt[k]], rtol=1e-11)
        curr_o_all = curr_o
        inimg = ((init_d[..., 0] > 5) & (init_d[..., 0] < H) & (init_d[..., 1] > 5) & (init_d[..., 1] < W)).sum(1)
        assert inimg.tolist() == [IN_IMAGE[k] for k in ids]
        for call in range(3):
            t = _np(ms.marker_draws).astype(np.int64)
            assert t.tolist() == [call] * 8
            # the noisy call
            _configure(ms, prob=0.02, sigma=0.5, K=K)
            flow = _np(ms.gen_marker_flow())
            n_dev = _np(ms.num_tracked).copy()
            cuv = _check_curr(ms, ids, curr_d)  # all current projections: noise-free, rows >= count zero
            assert _np(ms.marker_draws).tolist() == [call + 1] * 8
            ref, n_ref, chosen = flow_batch(init_d, cuv, cnt, ids, seed, t, 0.02, 0.5, H, W, K)
            assert n_dev.tolist() == n_ref.tolist()
            branches |= {bool(v) for v in (n_ref >= K)}
            err = np.abs(flow - ref).max()
            worst = max(worst, err)
            assert err <= 1e-9, err
            # the same draw with sigma 0: which marker sits in which slot, exactly
            _configure(ms, prob=0.02, sigma=0.0, K=K, draws=t)
            f0 = _np(ms.gen_marker_flow())
            ref0, n0, chosen0 = flow_batch(init_d, cuv, cnt, ids, seed, t, 0.02, 0.0, H, W, K)
            assert np.array_equal(chosen0, chosen) and _np(ms.num_tracked).tolist() == n_ref.tolist()
            assert np.array_equal(f0, ref0)
            for e, k in enumerate(ids):
                np.testing.assert_allclose(cuv[e, :cnt[k]], curr_o_all[e, :cnt[k]], rtol=1e-11)
            for e in range(8):
                assert (chosen[e] >= 0).all()
                np.testing.assert_allclose(f0[e, 0], init_o[e, chosen[e]], rtol=1e-11)
                np.testing.assert_allclose(f0[e, 1], curr_o[e, chosen[e]], rtol=1e-11)
            # float32 output, pixels and normalised, on the same draw with noise
            for norm, bound in ((False, 3e-5), (True, 2e-7)):
                _configure(ms, prob=0.02, sigma=0.5, K=K, normalize=norm, draws=t)
                o32 = torch.zeros((8, 2, K, 2), dtype=torch.float32, device="cuda:0")
                assert ms.gen_marker_flow_fused(out_f32=o32) is o32
                want = ref / 160.0 - 1.0 if norm else ref
                assert np.abs(_np(o32).astype(np.float64) - want).max() <= bound
            _configure(ms, K=K)
    print(f"\nmax |float64 flow - restatement| with noise: {worst:.3e} px (bound 1e-9)")
    assert branches == {True, False}, "one launch must take both the padding and the subset branch"


def test_envs_are_independent_of_the_batch_and_of_each_other(scene8, lib8):
    ms = lib8
    ids = [3, 1, 7, 0, 2, 1, 6, 5]
    t0 = [4, 9, 2, 0, 0, 7, 1, 3]
    _configure(ms, ids=ids, prob=0.02, sigma=0.5, K=60, draws=t0)
    f8 = ms.gen_marker_flow().clone()
    n8, c8 = ms.num_tracked.clone(), ms.curr_marker_uv.clone()
    # the first three envs alone: same ids, state, counters
    sc3 = Scene(3)
    assert torch.equal(sc3.x, scene8.x[:3])
    ms3 = sc3.sensor(num_markers=60, seed=0, marker_patterns=8, **RANGES)
    _configure(ms3, ids=ids[:3], prob=0.02, sigma=0.5, K=60, draws=t0[:3])
    f3 = ms3.gen_marker_flow()
    assert torch.equal(f3, f8[:3]) and torch.equal(ms3.num_tracked, n8[:3]) and torch.equal(ms3.curr_marker_uv, c8[:3])
    # one id written in place on the device: that env's output changes, no other
    _configure(ms, draws=t0, prob=0.02, sigma=0.5)
    ms.pattern_ids[5] = 4
    g8 = ms.gen_marker_flow()
    others = [e for e in range(8) if e != 5]
    assert torch.equal(g8[others], f8[others]) and not torch.equal(g8[5], f8[5])
    assert int(ms.num_tracked[5]) <= IN_IMAGE[4] and torch.equal(ms.num_tracked[others], n8[others])
    # two envs with the same id and the same state: the same noise-free projections, different lost markers / noise
    x = scene8.x.clone()
    x[2] = x[1]
    scene8.sim.x = x
    try:
        _configure(ms, ids=[0, 6, 6, 0, 0, 0, 0, 0], prob=0.02, sigma=0.5, draws=np.zeros(8))
        h8 = ms.gen_marker_flow()
        assert torch.equal(ms.curr_marker_uv[1], ms.curr_marker_uv[2])
        assert not torch.equal(h8[1], h8[2])
        _configure(ms, sigma=0.0, prob=0.0, draws=np.zeros(8))  # without loss and noise only the padding order is left: identical
        h0 = ms.gen_marker_flow()
        assert torch.equal(h0[1], h0[2]) and int(ms.num_tracked[1]) == IN_IMAGE[6] < 60
    finally:
        scene8.sim.x = scene8.x


def test_draw_counter(lib8):
    ms = lib8
    _configure(ms, ids=list(range(8)), prob=0.02, sigma=0.5, K=60, draws=[0, 1, 2, 3, 4, 5, 6, 0xffffffff])
    start = _np(ms.marker_draws).copy()
    a = ms.gen_marker_flow().clone()
    b = ms.gen_marker_flow().clone()
    got = _np(ms.marker_draws).astype(np.int64) & 0xffffffff
    assert got.tolist() == [2, 3, 4, 5, 6, 7, 8, 1]  # one per call, as a uint32 (the last env wrapped)
    for e in range(8):
        assert not torch.equal(a[e], b[e])
    ms.marker_draws.copy_(torch.from_numpy(start))
    assert torch.equal(ms.gen_marker_flow(), a) and torch.equal(ms.gen_marker_flow(), b)


def test_edges(scene8, lib8):
    ms = lib8
    # nothing survives
    _configure(ms, ids=list(range(8)), prob=1.0, sigma=0.5, K=60, draws=np.zeros(8))
    assert not ms.gen_marker_flow().any() and not ms.num_tracked.any()
    _configure(ms, prob=1.0, sigma=0.5, normalize=True)
    o32 = torch.zeros((8, 2, 60, 2), dtype=torch.float32, device="cuda:0")
    ms.gen_marker_flow_fused(out_f32=o32)
    assert (o32 == -1.0).all() and not ms.num_tracked.any()
    assert ms.curr_marker_uv.abs().max() > 1.0  # the projections themselves are still reported
    # far more slots than markers: padding
    _configure(ms, K=4096, draws=np.zeros(8))
    f = _np(ms.gen_marker_flow())
    init_d, curr_d = _projections(ms, list(range(8)))
    cuv = _check_curr(ms, list(range(8)), curr_d)
    ref, n, _ = flow_batch(init_d, cuv, _np(ms.patterns.count), list(range(8)), 0, np.zeros(8), 0.0, 0.0, H, W, 4096)
    assert f.shape == (8, 2, 4096, 2) and np.array_equal(f, ref) and n.tolist() == IN_IMAGE
    for e in range(8):
        assert (f[e, :, n[e]:] == f[e, :, n[e] - 1:n[e]]).all()
    # an id outside the library, written on the device: pattern 0
    _configure(ms, ids=[0] * 8, prob=0.02, sigma=0.5, K=60, draws=np.zeros(8))
    want = ms.gen_marker_flow().clone()
    want_uv = ms.curr_marker_uv.clone()
    _configure(ms, draws=np.zeros(8), prob=0.02, sigma=0.5)
    ms.pattern_ids.copy_(torch.tensor([0, 8, -1, 99, 2 ** 31 - 1, -2 ** 31, 0, 0], dtype=torch.int32))
    assert torch.equal(ms.gen_marker_flow(), want) and torch.equal(ms.curr_marker_uv, want_uv)
    with pytest.raises(ValueError):
        ms.set_pattern_ids([0, 8, 0, 0, 0, 0, 0, 0])
    ms.set_pattern_ids(list(range(8)))


def test_distribution_of_lost_markers_and_noise(lib8):
    """50 calls, B = 8, probability 0.05, sigma 0.5: the lost fraction, and mean and standard deviation of flow(sigma) - flow(0) taken with
    the counters written back, within five standard errors of their nominal values (bounds from the sample counts)."""
    ms, K, p, sigma = lib8, 60, 0.05, 0.5
    ids = list(range(8))
    _configure(ms, ids=ids, K=K, draws=np.zeros(8))
    ms.gen_marker_flow()
    n_img = _np(ms.num_tracked).astype(np.int64)
    assert n_img.tolist() == IN_IMAGE
    _configure(ms, draws=np.zeros(8))
    lost = trials = 0
    diffs = []
    for call in range(50):
        t = ms.marker_draws.clone()
        _configure(ms, prob=p, sigma=sigma, K=K)
        fs = ms.gen_marker_flow()
        n = _np(ms.num_tracked).astype(np.int64)
        ms.marker_draws.copy_(t)
        _configure(ms, prob=p, sigma=0.0, K=K)
        d = _np(fs - ms.gen_marker_flow())
        lost += int((n_img - n).sum())
        trials += int(n_img.sum())
        for e in range(8):  # distinct markers only: padding slots repeat the last survivor
            diffs.append(d[e, :, :min(n[e], K)].reshape(-1))
    frac = lost / trials
    se = np.sqrt(p * (1 - p) / trials)
    print(f"\nlost fraction {frac:.5f} of {trials} (nominal {p}, standard error {se:.5f})")
    assert abs(frac - p) <= 5 * se
    d = np.concatenate(diffs)
    S = d.size
    mean, std = d.mean(), d.std()
    print(f"noise: mean {mean:+.5f}, std {std:.5f} over {S} samples (nominal 0, {sigma}; standard errors {sigma / np.sqrt(S):.5f}, {sigma / np.sqrt(2 * S):.5f})")
    assert S > 40000
    assert abs(mean) <= 5 * sigma / np.sqrt(S)
    assert abs(std - sigma) <= 5 * sigma / np.sqrt(2 * S)  # standard error of a normal sample's standard deviation: sigma / sqrt(2 S)
    # the four values of a slot are four independent normals: no correlation between init and current, or between u and v
    q = np.concatenate([x.reshape(2, -1, 2) for x in diffs], 1)  # (2, slots, 2)
    for a, b in ((q[0, :, 0], q[1, :, 0]), (q[0, :, 0], q[0, :, 1]), (q[1, :, 0], q[1, :, 1])):
        assert abs(np.corrcoef(a, b)[0, 1]) <= 5 / np.sqrt(a.size)


def test_through_the_sensor():
    """GelSightSensor + ManiSkillSimulatorCfg(marker_patterns=4) on FemGelpad(4) (the C4 pad, 495 vertices): marker_motion against the
    restatement; after writing pattern_ids[2] and sensor.reset([2]) env 2 follows the new pattern and the others what the restatement predicts."""
    from oracle.fem_oracle import marker_uv
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.fem_based import ManiSkillSimulatorCfg
    from tacex_amd.uipc.gelpad_scene import FemGelpad

    B, K, seed, prob, sigma = 4, 54, 0, 0.02, 0.5
    cam = np.array([0.008, 0.012625, -0.024])
    fem = FemGelpad(B, "cuda:0")
    assert fem.num_verts == 495
    mcfg = ManiSkillSimulatorCfg(tactile_img_res=(W, H), device="cuda:0", camera_pos_w=tuple(cam), marker_patterns=4, marker_seed=seed,
                                 marker_lose_tracking_probability=prob, marker_random_noise=sigma,
                                 marker_params=ManiSkillSimulatorCfg.MarkerParams(num_markers=K), **RANGES)
    cfg = GelSightSensorCfg(num_envs=B, data_types=["marker_motion"], optical_sim_cfg=None, marker_motion_sim_cfg=mcfg,
                            sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H)), device="cuda:0")
    cfg.compute_indentation_depth_class = "marker_motion_sim"
    s = GelSightSensor(cfg, gelpad_obj=fem.gelpad)
    s.compute_indentation_depth_func = None
    s.initialize()
    s.compute_indentation_depth_func = None
    ms = s.marker_motion_simulator.marker_motion_sim
    cnt = _np(ms.patterns.count)
    assert ms.patterns.num_patterns == 4 and _np(ms.pattern_ids).tolist() == [0, 1, 2, 3]
    assert s.marker_motion_simulator.marker_data.dtype == torch.float32

    def step_and_check(i, ids):
        fem.step(i)
        t = _np(ms.marker_draws).astype(np.int64)
        s.update(dt=0.01, force_recompute=True)
        md = _np(s.data.output["marker_motion"]).astype(np.float64)
        assert md.shape == (B, 2, K, 2) and (_np(ms.marker_draws) == t + 1).all()
        init_d, curr_d = _projections(ms, ids)
        cuv = _check_curr(ms, ids, curr_d)
        ref, n, chosen = flow_batch(init_d, cuv, cnt, ids, seed, t, prob, sigma, H, W, K)
        assert _np(ms.num_tracked).tolist() == n.tolist()
        assert np.abs(md - ref).max() <= 3e-5
        return md, n, cuv

    ids = [0, 1, 2, 3]
    seen = set()
    for i in range(4):
        md, n, _ = step_and_check(i, ids)
        seen |= {bool(v) for v in (n >= K)}
    assert seen == {True, False}  # patterns with 52 to 61 in-image markers around K = 54: both branches
    assert np.abs(md[:, 1] - md[:, 0]).max() > 0.05
    # env 2 gets a new pattern at its reset
    ms.pattern_ids[2] = 1
    s.reset([2])
    ids = [0, 1, 1, 3]
    for i in range(4, 7):
        md, n, curr_d = step_and_check(i, ids)
    x = _np(fem.sim.x)
    surf = ms.surf_vertex_ids
    tri, wgt = _np(ms.patterns.tri), _np(ms.patterns.wgt)
    np.testing.assert_allclose(curr_d[2, :cnt[1]], marker_uv((x[2, surf] - cam)[None], tri[1, :cnt[1]], wgt[1, :cnt[1]])[0], rtol=1e-11)
    assert not np.array_equal(md[1], md[2])  # the same pattern, streams of their own
