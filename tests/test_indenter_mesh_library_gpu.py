"""Indenter mesh LIBRARY: one rigid mesh per env, in the FEM contact path (UipcSim.set_indenter_meshes, tacex_fem_set_indenter_mesh_library
/ _ids) and in the camera depth raster (MeshLibraryDepthSource, tacex_depth_from_mesh_library).  Every env must see exactly - bit for bit -
what a scene holding its mesh alone shows it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INTR = (340.0, 325.0, 160.0, 125.0)

# One scene script per Newton kernel (the TACEX_FEM_NEWTON_LDS switch is read once per process).  The deterministic switch makes every
# run reproducible bit for bit, so an env of a mixed batch can be compared with the same env of a single-mesh scene with ==.
_FEM_SCRIPT = r'''
import sys, numpy as np, torch
sys.path.insert(0, REPO)
from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
from tacex_amd.uipc.indenter_meshes import box, icosphere
from tacex_amd.uipc.uipc_object import gelpad_box_mesh

P, T = gelpad_box_mesh(8, 10, 4)
B = 6
MESHES = [icosphere(0.004, 1), box((0.003, 0.002, 0.0015)), icosphere(0.0035, 2)]
IDS = [0, 1, 2, 2, 1, 0]
STEPS = 5
top, size = P[:, 2].max(), P.max(0)


def scene():
    cfg = UipcSimCfg(device="cuda:0")
    cfg.linear_system.deterministic = True
    sim = UipcSim(cfg, num_envs=B)
    UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T), sim)
    sim.setup_sim()
    back = np.where(P[:, 2] < 1e-12)[0]
    sim.set_constraints(back, torch.from_numpy(P[back]).cuda()[None].repeat(B, 1, 1))
    assert sim.cfg.contact.enable_friction
    return sim


def rows(ids, only=None):
    """kind-4 rows placing mesh ids[b] 0.9 mm over the pad (turned about z); envs whose mesh is not `only` get no indenter"""
    ind = np.zeros((B, 8))
    for b, k in enumerate(ids):
        ind[b] = [4.0, size[0] / 2 + 3e-4 * b, size[1] / 2, top + 0.0009 - MESHES[k][0][:, 2].min(), 0.0, 0.0, 0.0, 0.3 * b]
        if only is not None and k != only:
            ind[b, 0] = 0.0
    return torch.from_numpy(ind)


def run(sim, ind, before_step=None):
    """press (by 40 % of the env's gap) and slide (+0.1 mm in x) for STEPS steps with friction"""
    sim.set_contact_indenters(ind)
    flags = []
    for k in range(STEPS):
        if before_step:
            before_step(sim, k)
        g = sim.contact_gaps().amin(1)
        i2 = sim.contact_indenters
        i2[:, 3] -= 0.4 * torch.where(torch.isfinite(g), g, torch.zeros_like(g))
        i2[:, 1] += 1e-4
        sim.step(max_newton_iter=30)
        flags.append(sim.step_info[:, 2].cpu().numpy().astype(np.int64))
    out = dict(x=sim.x.cpu().numpy(), flags=np.stack(flags), resident=bool(sim.newton_kernel_resident))
    return out


res = {}
# the mixed batch, and its gaps against the torch restatement
sim = scene()
sim.set_indenter_meshes(MESHES, IDS)
sim.set_contact_indenters(rows(IDS))
res["gaps_mixed"] = sim.contact_gaps().cpu().numpy()
res["gaps_mixed_torch"] = sim.contact_gaps_torch().cpu().numpy()
r = run(sim, rows(IDS))
res["mixed_x"], res["mixed_flags"], res["resident"] = r["x"], r["flags"], r["resident"]
# every mesh alone (the old API), envs of other meshes without an indenter
for k in range(len(MESHES)):
    sim = scene()
    sim.set_indenter_mesh(*MESHES[k])
    sim.set_contact_indenters(rows(IDS, only=k))
    res[f"gaps_single{k}"] = sim.contact_gaps().cpu().numpy()
    res[f"single{k}_x"] = run(sim, rows(IDS, only=k))["x"]
# a library of one against the old API, all envs on mesh 2
for lib in (0, 1):
    sim = scene()
    if lib:
        sim.set_indenter_meshes([MESHES[2]])
    else:
        sim.set_indenter_mesh(*MESHES[2])
    res[f"one_lib{lib}_x"] = run(sim, rows([2] * B))["x"]


# env 0 switches from mesh 0 to mesh 2 before step 2 (the id tensor mutated in place) ...
def switch(sim, k):
    if k == 2:
        sim.indenter_mesh_ids[0] = 2


sim = scene()
sim.set_indenter_meshes(MESHES, IDS)
res["switch_x"] = run(sim, rows(IDS), switch)["x"]


# ... against the old API with mesh 0 for two steps, then mesh 2
def swap(sim, k):
    if k == 2:
        sim.set_indenter_mesh(*MESHES[2])


sim = scene()
sim.set_indenter_mesh(*MESHES[0])
res["swap_x"] = run(sim, rows(IDS, only=0), swap)["x"]
# an id outside the library, written on the device behind the host check: env 3 runs without an indenter and is flagged
sim = scene()
sim.set_indenter_meshes(MESHES, IDS)
sim.indenter_mesh_ids[3] = 7
r = run(sim, rows(IDS))
res["bad_x"], res["bad_flags"] = r["x"], r["flags"]
res["bad_check"] = sim.check_step(raise_on_penetration=False)["bad_mesh_id_envs"]
res["bad_gaps"] = sim.contact_gaps().cpu().numpy()
np.savez(sys.argv[1], **res)
'''


def _fem_runs(tmp_path, flag):
    from conftest import REPO

    script = tmp_path / "mesh_library_run.py"
    script.write_text(_FEM_SCRIPT.replace("sys.path.insert(0, REPO)", f"sys.path.insert(0, {str(REPO)!r})"))
    out = tmp_path / f"lib{flag}.npz"
    r = subprocess.run([sys.executable, str(script), str(out)], env=dict(os.environ, TACEX_FEM_NEWTON_LDS=flag),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("flag", ["1", "0"], ids=["resident", "streaming"])
def test_fem_mesh_library_is_bit_equal_to_single_mesh_scenes(tmp_path, flag):
    """Three meshes of different size, 6 envs with ids [0,1,2,2,1,0], pressed and slid for 5 steps with friction: every env ends
    bit-equal to the same env in a scene that holds its mesh alone (set_indenter_mesh); a library of one equals the old API; an env
    switched between steps matches a run that swapped the mesh then; an id outside the library leaves its env contact-free and
    flagged (32) and changes no other env."""
    r = _fem_runs(tmp_path, flag)
    assert bool(r["resident"]) == (flag == "1")
    ids = [0, 1, 2, 2, 1, 0]
    x = r["mixed_x"]
    for b, k in enumerate(ids):
        np.testing.assert_array_equal(x[b], r[f"single{k}_x"][b], err_msg=f"env {b} (mesh {k})")
        np.testing.assert_array_equal(r["gaps_mixed"][b], r[f"gaps_single{k}"][b])
    np.testing.assert_allclose(r["gaps_mixed_torch"], r["gaps_mixed"], rtol=1e-12, atol=1e-15)
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, _ = gelpad_box_mesh(8, 10, 4)
    dent = [float((P[:, 2] - x[b][:, 2]).max()) for b in range(6)]
    assert min(dent) > 1e-6 and not (r["mixed_flags"] & 1).any(), dent  # pressed without penetration
    assert np.abs(x[0] - x[5]).max() > 0 and np.abs(x[2] - x[1]).max() > 0  # (same mesh, other pose / other mesh: other states)
    assert not (r["mixed_flags"] & 32).any()
    # a library of one = the old API
    np.testing.assert_array_equal(r["one_lib1_x"], r["one_lib0_x"])
    # ids changed between steps
    np.testing.assert_array_equal(r["switch_x"][0], r["swap_x"][0])
    np.testing.assert_array_equal(r["switch_x"][1:], x[1:])
    # an id outside the library
    bad = r["bad_x"]
    others = [0, 1, 2, 4, 5]
    np.testing.assert_array_equal(bad[others], x[others])
    np.testing.assert_array_equal(bad[3], r["single0_x"][3])  # (mesh 0's scene leaves env 3 without an indenter)
    assert (r["bad_flags"][:, 3] & 32).all() and not (r["bad_flags"][:, others] & 32).any()
    assert list(r["bad_check"]) == [3]
    assert np.isinf(r["bad_gaps"][3]).all() and np.isfinite(r["bad_gaps"][others]).any()


def test_mesh_library_setters_validate_on_the_host():
    from tacex_amd.uipc import UipcObject, UipcObjectCfg, UipcSim, UipcSimCfg
    from tacex_amd.uipc.indenter_meshes import box, icosphere
    from tacex_amd.uipc.uipc_object import gelpad_box_mesh

    P, T = gelpad_box_mesh(3, 3, 2)
    sim = UipcSim(UipcSimCfg(device="cuda:0"), num_envs=3)
    UipcObject(UipcObjectCfg(mesh_points=P, mesh_tets=T), sim)
    sim.setup_sim()
    meshes = [icosphere(0.004, 1), box((0.001, 0.001, 0.001))]
    with pytest.raises(ValueError):
        sim.set_indenter_meshes(meshes, [0, 1, 2])  # id out of range
    with pytest.raises(ValueError):
        sim.set_indenter_meshes(meshes, [0, 1])  # one id per env
    with pytest.raises(ValueError):
        sim.set_indenter_meshes([(meshes[1][0], meshes[1][1] + 8)])  # triangle index out of range
    sim.set_indenter_meshes(meshes, [1, 0, 1])
    assert sim.indenter_mesh_ids.dtype == torch.int32 and sim.indenter_mesh_ids.tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        sim.set_indenter_mesh_ids([0, 0, 5])
    sim.set_indenter_mesh_ids([0, 0, 1])
    assert sim.indenter_mesh_ids.tolist() == [0, 0, 1]
    lib, h = sim._lib, sim._handle
    vc = np.array([3], np.int32); tc = np.array([1], np.int32)
    v = np.zeros((3, 3)); t = np.array([[0, 1, 3]], np.int32)
    assert lib.tacex_fem_set_indenter_mesh_library(h, 1, vc.ctypes.data, v.ctypes.data, tc.ctypes.data, t.ctypes.data) != 0
    assert b"out of range" in lib.tacex_last_error()
    assert lib.tacex_fem_set_indenter_mesh_library(h, -1, 0, 0, 0, 0) != 0
    assert lib.tacex_fem_set_indenter_mesh_library(h, 0, 0, 0, 0, 0) == 0
    sim.set_indenter_mesh(None, None)
    assert sim.indenter_meshes is None and sim.indenter_mesh_ids is None


def _library():
    from oracle.mesh_depth_oracle import icosphere

    big, bt = icosphere(0.004, 3)                                      # 1280 triangles: two chunks of the library kernel
    lobe = np.concatenate([big, big * 0.6 + np.array([0.003, 0.001, -0.0015], dtype=np.float32)])
    lt = np.concatenate([bt, bt + len(big)])                           # 2560, non-convex: three chunks
    small, st = icosphere(0.0035, 1)                                   # 80
    from tacex_amd.uipc.indenter_meshes import box

    bv, btr = box((0.003, 0.002, 0.0015))                              # 12
    return [(big, bt), (lobe, lt), (small, st), (bv.astype(np.float32), btr)]


def _poses(B, seed):
    rng = np.random.RandomState(seed)
    pos = np.stack([rng.uniform(-0.004, 0.004, B), rng.uniform(-0.003, 0.003, B), rng.uniform(0.0290, 0.0315, B)], 1)
    pos[B - 2] = [0.013, 0.0, 0.030]  # half out of view on the right
    pos[B - 1] = [0.0, 0.0, 0.040]    # beyond the far plane
    quat = rng.normal(size=(B, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    return torch.from_numpy(pos).float(), torch.from_numpy(quat).float()


@pytest.mark.parametrize("res", [(320, 240), (640, 480)])
def test_depth_library_is_bit_equal_to_single_mesh_sources_and_the_oracle(res):
    from oracle.mesh_depth_oracle import pose_rows, render_depth
    from tacex_amd import MeshDepthSource, MeshLibraryDepthSource

    W, H = res
    meshes = _library()
    B = 10
    ids = torch.tensor([0, 1, 2, 3, 1, 0, 2, 3, 1, 0], dtype=torch.int32)
    pos, quat = _poses(B, 7)
    src = MeshLibraryDepthSource(meshes, B, "cuda:0", resolution=(W, H), intrinsics=INTR, clipping_range=(0.024, 0.029))
    src.pos.copy_(pos); src.quat.copy_(quat); src.mesh_ids.copy_(ids)
    depth = src().clone().cpu().numpy()
    seen = 0
    for k, (v, t) in enumerate(meshes):
        one = MeshDepthSource(v, t, B, "cuda:0", resolution=(W, H), intrinsics=INTR, clipping_range=(0.024, 0.029))
        one.pos.copy_(pos); one.quat.copy_(quat)
        want = one().cpu().numpy()
        sel = np.nonzero(ids.numpy() == k)[0]
        np.testing.assert_array_equal(depth[sel].view(np.uint32), want[sel].view(np.uint32), err_msg=f"mesh {k}")
        seen += int(np.isfinite(depth[sel]).sum())
        if W == 320 or k >= 2:  # (the NumPy oracle on the large meshes at 640 x 480 would take minutes)
            o = render_depth(v, t, pose_rows(pos[sel].numpy(), quat[sel].numpy()), *INTR, near=0.024, far=0.029, H=H, W=W)
            np.testing.assert_array_equal(depth[sel], o)
    assert seen > 1000 and np.isinf(depth[B - 1]).all()
    # ids changed in place between two renders, and an id outside the library renders nothing
    src.mesh_ids.copy_(torch.tensor([3, 2, 1, 0, 0, 1, 2, 3, 9, -1], dtype=torch.int32))
    d2 = src().cpu().numpy()
    one = MeshDepthSource(*meshes[0], B, "cuda:0", resolution=(W, H), intrinsics=INTR, clipping_range=(0.024, 0.029))
    one.pos.copy_(pos); one.quat.copy_(quat)
    np.testing.assert_array_equal(d2[[3, 4]].view(np.uint32), one().cpu().numpy()[[3, 4]].view(np.uint32))
    assert np.isinf(d2[8]).all() and np.isinf(d2[9]).all()


def test_depth_library_drives_the_sensor_like_per_shape_sources(calib_dir):
    """GelSightSensor.update() with the library source gives the RGB and height map that per-shape sources scattered by env give."""
    from tacex_amd import GelSightSensor, GelSightSensorCfg, MeshDepthSource, MeshLibraryDepthSource
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg

    B, H, W = 6, 240, 320
    meshes = _library()
    ids = torch.tensor([1, 0, 3, 2, 1, 0], dtype=torch.int32)
    pos, quat = _poses(B, 11)

    def sensor(src):
        cfg = GelSightSensorCfg(
            num_envs=B, sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029), depth_source=src),
            data_types=["tactile_rgb", "height_map"],
            optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib_dir), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                              tactile_img_res=(W, H), device="cuda:0"),
            marker_motion_sim_cfg=None, device="cuda:0")
        s = GelSightSensor(cfg); s.initialize()
        s.update(0.01, force_recompute=True)
        return s.data.output["height_map"].clone(), s.data.output["tactile_rgb"].clone(), s.indentation_depth.clone()

    lib = MeshLibraryDepthSource(meshes, B, "cuda:0", resolution=(W, H), intrinsics=INTR, clipping_range=(0.024, 0.029))
    lib.pos.copy_(pos); lib.quat.copy_(quat); lib.mesh_ids.copy_(ids)
    hm, rgb, ind = sensor(lib)
    singles = [MeshDepthSource(v, t, B, "cuda:0", resolution=(W, H), intrinsics=INTR, clipping_range=(0.024, 0.029)) for v, t in meshes]
    for s in singles:
        s.pos.copy_(pos); s.quat.copy_(quat)
    dev_ids = ids.cuda().long()

    def scattered():  # the per-shape route: K renders and a gather by env
        d = torch.stack([s() for s in singles])  # (K,B,H,W)
        return d[dev_ids, torch.arange(B, device="cuda")].contiguous()

    hm2, rgb2, ind2 = sensor(scattered)
    assert torch.equal(hm, hm2) and torch.equal(rgb, rgb2) and torch.equal(ind, ind2)
    assert (ind[:B - 2] > 0.05).sum() >= 3 and ind[B - 1] == 0.0
