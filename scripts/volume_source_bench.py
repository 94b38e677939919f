"""Time of the SDF volume height-map source (`SdfVolumeSource.fill`: the marching launch of tacex_height_map_from_sdf and the
indentation-depth launch behind it) on 2048 frames of 320 x 240 - a C3 step's height maps - warm, inputs resident, hipEvents around
`--calls` calls in a row, the variants alternating over `--reps` rounds:
  (a) a sphere (R = 3 mm) on a 64^3 grid, random rotations;
  (b) a gear on a 64^3 grid at random tilted poses, max_steps 16 / 32 / 64;
  (c) a library of 64 gears on 128^3 grids (512 MiB of voxels, beyond L2 and the Infinity Cache), one per env;
and the yardsticks measured in the same run (nothing is measured against the code under test):
  (y1) tacex_height_map_from_indenters, then tacex_indentation_depth with ranges (a sphere);
  (y2) `ReliefHeightMapSource.fill`, sphere carrier over a 64 x 64 tile;
  (y3) `MeshLibraryDepthSource.fill` on a sphere of about 5 k and of about 40 k triangles that covers as many pixels;
  (y4) one sensor `update()` with the indenter, the relief, the mesh and the volume source.
The mean number of taps per pixel is a debug count of the NumPy restatement (tests/volume_source_ref.py) on the first `--ref-frames`
frames of each case.

  --out FILE   also write the table as markdown."""
import math
import sys
from pathlib import Path

import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, rounds, sensor_update_yardstick, table

a = parse_args(calls=50, torch_calls=0, extra=[("--sensor-steps", dict(type=int, default=20)), ("--no-sensor", dict(action="store_true")),
                                               ("--ref-frames", dict(type=int, default=8)), ("--library", dict(type=int, default=64))])
sys.path.insert(0, str(Path(a.repo) / "tests"))

import volume_source_ref as V  # noqa: E402
from tacex_amd import (GelSightSensor, GelSightSensorCfg, IndenterHeightMapSource, MeshLibraryDepthSource, ReliefHeightMapSource,  # noqa: E402
                       SdfVolumeSource, _lib)
from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg  # noqa: E402
from tacex_amd.utils import relief_tiles, sdf_volumes  # noqa: E402

GH, GD, PIX = 0.0045, 0.024, 0.0295


def uv_sphere(radius, n_lon, n_lat):
    """(verts, tris) of a latitude / longitude sphere: 2 n_lon (n_lat - 1) triangles."""
    lat = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)), np.outer(np.cos(lat), np.ones(n_lon))], -1)
    verts = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius
    idx = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    quads = np.stack([idx[:-1], idx[1:], nxt[1:], nxt[:-1]], -1).reshape(-1, 4)
    caps = [[0, idx[0, j], nxt[0, j]] for j in range(n_lon)] + [[len(verts) - 1, nxt[-1, j], idx[-1, j]] for j in range(n_lon)]
    tris = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]], np.asarray(caps)])
    return verts.astype(np.float32), tris.astype(np.int32)


def main():
    B, H, W = a.frames, a.height, a.width
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    st = _lib.current_stream_handle(dev)
    g = torch.Generator().manual_seed(0)
    rnd = torch.rand((B, 6), generator=g)
    quat = torch.randn((B, 4), generator=g)
    cx, cy = (0.3 + 0.4 * rnd[:, 0]) * W, (0.3 + 0.4 * rnd[:, 1]) * H
    press = 0.2 + 1.3 * rnd[:, 3]
    fmin, ind = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    hm = torch.empty((B, H, W), device=dev)
    variants, srcs, notes = {}, {}, []

    def volume(tag, vols, max_steps=32, by_depth=None):
        src = SdfVolumeSource(vols, B, dev, pixmm=PIX, max_steps=max_steps)
        src.volume_ids.copy_(torch.arange(B, dtype=torch.int32) % len(vols))
        if by_depth is None:
            src.set_pose(cx, cy, quat, press_mm=press)
        else:  # (a large library: the anchor's depth directly, no surface-point table)
            src.set_pose(cx, cy, quat, z_mm=by_depth)
        variants[tag] = lambda: src.fill(hm, fmin, ind, GH, GD, rows=rows)
        srcs[tag] = src
        return src

    ball = sdf_volumes.from_function(lambda x, y, z: sdf_volumes.sphere_distance(x, y, z, 3.0), (64, 64, 64), 6.6 / 63)
    gear_fn = lambda t: (lambda x, y, z: sdf_volumes.gear_field(x, y, z, t, 2.2, 0.7, 1.6))  # noqa: E731
    gear = sdf_volumes.from_function(gear_fn(12), (64, 64, 64), 6.6 / 63, sdf_volumes.gear_step_scale(12, 2.2, 0.7))
    volume("(a) volume, sphere R = 3 mm on 64^3, max_steps 32", [ball])
    for steps in (16, 32, 64):
        volume(f"(b) volume, gear on 64^3 (step_scale {gear.step_scale:.2f}), tilted, max_steps {steps}", [gear], steps)
    big = [sdf_volumes.from_function(gear_fn(8 + k % 9), (128, 128, 128), 6.6 / 127, sdf_volumes.gear_step_scale(8 + k % 9, 2.2, 0.7))
           for k in range(a.library)]
    volume(f"(c) volume, {a.library} gears on 128^3 ({a.library * 8} MiB), one per env, max_steps 32", big, by_depth=28.5 - press + 2.0)
    del big
    # (y1) the primitive's two launches
    prim = IndenterHeightMapSource(B, dev, pixmm=PIX)
    prim.set("sphere", cx=cx, cy=cy, r=(0.15 + 0.2 * rnd[:, 5]) * H, press_mm=press)

    def two_launches():
        prim.fill(hm, fmin, ind, GH, GD)
        lib.tacex_indentation_depth(_lib.ptr(hm), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W, st)

    variants["(y1) tacex_height_map_from_indenters + tacex_indentation_depth with ranges (sphere)"] = two_launches
    # (y2) the relief source
    relief = ReliefHeightMapSource([relief_tiles.weave(64)], B, dev, pixmm=PIX)
    relief.set_pose(cx, cy, 2 * math.pi * rnd[:, 2], press, scale=1.0 + rnd[:, 4], carrier="sphere", radius_mm=1.5 + 1.5 * rnd[:, 5])
    variants["(y2) ReliefHeightMapSource.fill, sphere carrier, 64 x 64 tile"] = lambda: relief.fill(hm, fmin, ind, GH, GD, rows=rows)
    # (y3) a sphere through the rasteriser; 340 px focal length at 28 mm is 12.1 px per mm against 33.9 here: magnified to cover as much
    meshes, hm_mesh = {}, torch.empty_like(hm)
    for n_lon, n_lat in ((64, 41), (160, 126)):
        verts, tris = uv_sphere(3.0e-3 * (1 / PIX) / (340.0 / 28.0), n_lon, n_lat)
        m = MeshLibraryDepthSource([(verts, tris)], B, dev, resolution=(W, H))
        m.pos[:, 0], m.pos[:, 1] = (cx.to(dev) - W / 2) * (0.0282 / 340.0), (cy.to(dev) - H / 2) * (0.0282 / 325.0)
        m.pos[:, 2] = (28.5 - press.to(dev)) * 1e-3 + float(np.abs(verts).max())
        m.quat.copy_(torch.nn.functional.normalize(quat, dim=1))
        tag = f"(y3) MeshLibraryDepthSource.fill, a sphere of {tris.shape[0]} triangles"
        variants[tag] = (lambda m=m: m.fill(hm_mesh, fmin, ind, GH, GD))
        meshes[tag] = m
    ms = rounds(variants, a.calls, a.reps, 5)
    # what each case covers, and the restatement's tap counts on its first frames (outside the timing)
    cells = {}
    for tag, fn in variants.items():
        fn()
        seen = float(((hm_mesh if tag in meshes else hm) < 29.0).float().mean().item())
        taps = ""
        if tag in srcs and a.ref_frames > 0:
            s, n, stats = srcs[tag], min(a.ref_frames, B), {}
            V.height_map(s.voxels.cpu().numpy(), s.volumes_i.cpu().numpy(), s.volumes_f.cpu().numpy(), s.volume_ids[:n].cpu().numpy(),
                         s.pose[:n].cpu().numpy(), H, W, PIX, s.near_clip_mm, s.far_clip_mm, s.max_steps, s.tol_mm, stats)
            taps = f"{stats['taps'] / (n * H * W):.2f} / {stats['taps'] / max(stats['covered'], 1):.2f} / {stats['unconverged'] / (n * H * W):.4f}"
        cells[tag] = (f"{seen:.2f}", taps)
    lines = table(["share of pixels in contact", "taps per pixel / per marched pixel / share that used every tap"],
                  [(k, v, *cells[k]) for k, v in ms.items()])
    if not a.no_sensor:
        calib = Path(a.repo) / "tacex_amd" / "assets" / "calib" / "gsmini_640x480"
        cfg = GelSightSensorCfg(
            num_envs=B, data_types=["tactile_rgb", "height_map"],
            sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
            optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib), gelpad_height=GH, gelpad_to_camera_min_distance=GD,
                                              tactile_img_res=(W, H), device="cuda"),
            device="cuda")
        tags = list(srcs)
        with_source = {"(y4) sensor update, relief source (y2)": relief, "(y4) sensor update, mesh source, 5 k triangles": list(meshes.values())[0],
                       "(y4) sensor update, volume source (a)": srcs[tags[0]], "(y4) sensor update, volume source (b), max_steps 32": srcs[tags[2]]}
        sens = {}
        for tag, src in with_source.items():
            s = GelSightSensor(cfg)
            s.set_height_map_source(src)
            sens[tag] = (lambda s=s: s.update(0.01, force_recompute=True))
        sm = rounds(sens, a.sensor_steps, a.reps, 3)
        sm = {"(y4) sensor update, indenter source (spheres)": sensor_update_yardstick(a.repo, B, H, W, a.reps)} | sm
        lines += [""] + table([], list(sm.items()), first="sensor update (one GelSightSensor, tactile_rgb)")
    notes.append(f"tap counts: the NumPy restatement on the first {min(a.ref_frames, B)} frames of the case; a marched pixel is one "
                 "whose ray meets the grid's box inside the clip range")
    head = (f"# SDF volume height-map source: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, {a.reps} "
            f"alternating rounds (median, min, max of the rounds), one MI355X; the sensor {a.sensor_steps} updates per timing.  The height "
            f"maps are {B * H * W * 4 / 1e9:.3f} GB: one write at the {COPY_TBS} TB/s float4-copy rate takes {copy_ms(B * H * W * 4):.3f} ms.\n\n")
    emit(lines, a.out, head, notes)


if __name__ == "__main__":
    main()
