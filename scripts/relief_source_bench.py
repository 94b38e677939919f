"""Time of the relief height-map source (`ReliefHeightMapSource.fill`, one launch of tacex_height_map_from_relief) on 2048 frames of
320 x 240 - a C3 step's height maps - warm, inputs resident, hipEvents around `--calls` calls in a row, the variants alternating over
`--reps` rounds:
  (a) plane carrier, one wrapping 64 x 64 tile: the whole frame in contact, every pixel takes its four taps;
  (b) sphere carrier over the same tile: the pixels outside the footprint skip their taps;
  (c) samples = 4 on (a);
  (d) a library of 64 tiles of 512 x 512 (64 MiB, beyond the 4 MiB L2 of an XCD: the taps come from the Infinity Cache), a tile per env;
and the yardsticks measured in the same run (nothing is measured against the code under test):
  (y1) the two launches that deliver the same set of outputs for a primitive: tacex_height_map_from_indenters, then
       tacex_indentation_depth with ranges;
  (y2) `copy_` of the height maps (a read and a write) beside the float4-copy rate COPY_TBS;
  (y3) `MeshLibraryDepthSource.fill` on a 5 120-triangle tessellation of the same tile (texture through the rasteriser);
  (y4) a torch restatement with `grid_sample` (plane carrier, wrapping by tiling the coordinates);
  (y5) one sensor `update()` with the indenter source and with the relief source.

  --out FILE   also write the table as markdown."""
import math

import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, repeated, rounds, stats, table

a = parse_args(calls=50, torch_calls=5, extra=[("--sensor-steps", dict(type=int, default=20)), ("--no-sensor", dict(action="store_true"))])

from tacex_amd import IndenterHeightMapSource, MeshLibraryDepthSource, ReliefHeightMapSource, _lib  # noqa: E402
from tacex_amd.utils import relief_tiles  # noqa: E402

GH, GD, PIX = 0.0045, 0.024, 0.0295


def tile_mesh(tile, nu=64, nv=40, z_m=0.0282):
    """The tile as 2 nu nv triangles in the camera frame [m]: a regular grid over the tile's extent, heights sampled at the vertices."""
    h = tile.height_mm
    Th, Tw = h.shape
    u, v = np.meshgrid(np.linspace(0, Tw - 1, nu + 1), np.linspace(0, Th - 1, nv + 1), indexing="xy")
    z = h[np.rint(v).astype(int), np.rint(u).astype(int)]
    scale = 22.0  # (magnified so that the mesh covers the frame, like the tile in (a): 340 px focal length at 28 mm is 12 px per mm)
    verts = np.stack([(u - (Tw - 1) / 2) * tile.pitch_mm * scale * 1e-3, (v - (Th - 1) / 2) * tile.pitch_mm * scale * 1e-3,
                      z_m - z * 1e-3], axis=-1).reshape(-1, 3)
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nv + 1, nu + 1)
    q = np.stack([idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:], idx[1:, :-1]], axis=-1).reshape(-1, 4)
    tris = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    return verts.astype(np.float32), tris.astype(np.int32)


def torch_relief(tex, grid_xy, base, top):
    """Plane carrier, wrapping tile: bilinear taps by grid_sample on a tile padded by one texel per side (so that the wrap is exact)."""
    h = torch.nn.functional.grid_sample(tex, grid_xy, mode="bilinear", padding_mode="border", align_corners=True)[:, 0]
    hm = (base + (top - h)).clamp_(max=29.0)
    fmin = hm.amin(dim=(1, 2))
    return hm, fmin


def main():
    B, H, W = a.frames, a.height, a.width
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    st = _lib.current_stream_handle(dev)
    g = torch.Generator().manual_seed(0)
    rnd = torch.rand((B, 6), generator=g)
    cx, cy, yaw = (0.3 + 0.4 * rnd[:, 0]) * W, (0.3 + 0.4 * rnd[:, 1]) * H, 2 * math.pi * rnd[:, 2]
    press, scale = 0.2 + 1.3 * rnd[:, 3], 1.0 + rnd[:, 4]
    fmin, ind = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    hm = torch.empty((B, H, W), device=dev)
    weave = relief_tiles.weave(64)
    variants, taps = {}, {}

    def relief(tag, tiles, samples, carrier, radius):
        src = ReliefHeightMapSource(tiles, B, dev, pixmm=PIX, samples=samples)
        src.randomize(generator=torch.Generator(device=dev).manual_seed(2))
        src.set_pose(cx, cy, yaw, press, scale=scale, carrier=carrier, radius_mm=radius)
        variants[tag] = lambda: src.fill(hm, fmin, ind, GH, GD, rows=rows)
        return src

    srcs = {
        "a": relief("(a) relief, plane carrier, one wrapping 64 x 64 tile", [weave], 1, "plane", 0.0),
        "b": relief("(b) relief, sphere carrier (R = 1.5 ... 3 mm), the same tile", [weave], 1, "sphere", 1.5 + 1.5 * rnd[:, 5]),
        "c": relief("(c) relief, plane carrier, samples = 4", [weave], 4, "plane", 0.0),
    }
    big = [relief_tiles.from_array(np.tile(relief_tiles.weave(64, threads=4 + 2 * (k % 5)).height_mm, (8, 8)) + np.float32(0.001 * k), 0.02)
           for k in range(64)]
    srcs["d"] = relief("(d) relief, plane carrier, 64 tiles of 512 x 512 (64 MiB), a tile per env", big, 1, "plane", 0.0)
    del big
    for k, s in srcs.items():  # how many pixels take their taps (read back once, outside the timing)
        s.fill(hm, fmin, ind, GH, GD, rows=rows)
        taps[k] = float((hm < 29.0).float().mean().item())
    # (y1) the primitive's two launches
    prim = IndenterHeightMapSource(B, dev, pixmm=PIX)
    prim.set("sphere", cx=cx, cy=cy, r=(0.15 + 0.2 * rnd[:, 5]) * H, press_mm=press)

    def two_launches():
        prim.fill(hm, fmin, ind, GH, GD)
        lib.tacex_indentation_depth(_lib.ptr(hm), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W, st)

    variants["(y1) tacex_height_map_from_indenters + tacex_indentation_depth with ranges (sphere)"] = two_launches
    variants["(y1) tacex_height_map_from_indenters alone"] = lambda: prim.fill(hm, fmin, ind, GH, GD)
    dst = torch.empty_like(hm)
    variants["(y2) copy of the height maps (copy_, read + write)"] = lambda: dst.copy_(hm)
    # (y3) the same tile through the rasteriser
    verts, tris = tile_mesh(weave)
    mesh = MeshLibraryDepthSource([(verts, tris)], B, dev, resolution=(W, H))
    mesh.pos[:, 0], mesh.pos[:, 1], mesh.pos[:, 2] = (cx.to(dev) - W / 2) * (0.0282 / 340.0), (cy.to(dev) - H / 2) * (0.0282 / 325.0), 0.0
    hm_mesh = torch.empty_like(hm)
    variants[f"(y3) MeshLibraryDepthSource.fill, the tile as {tris.shape[0]} triangles"] = lambda: mesh.fill(hm_mesh, fmin, ind, GH, GD)
    bytes_px = {k: 4 for k in variants}
    bytes_px["(y1) tacex_height_map_from_indenters + tacex_indentation_depth with ranges (sphere)"] = 8
    bytes_px["(y2) copy of the height maps (copy_, read + write)"] = 8
    out = [(k, v, bytes_px[k]) for k, v in rounds(variants, a.calls, a.reps, 5).items()]
    mesh.fill(hm_mesh, fmin, ind, GH, GD)
    mesh_seen = float((hm_mesh < 29.0).float().mean().item())
    # (y4) torch ops
    pose = srcs["a"].pose
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    u = pose[:, 0, None, None] * xx + pose[:, 1, None, None] * yy + pose[:, 2, None, None]
    v = pose[:, 3, None, None] * xx + pose[:, 4, None, None] * yy + pose[:, 5, None, None]
    t = torch.from_numpy(np.pad(weave.height_mm, ((0, 1), (0, 1)), mode="wrap")).to(dev)  # 65 x 65: texel 64 = texel 0
    tex = t[None, None].expand(B, 1, 65, 65).contiguous()
    base = (28.5 - pose[:, 6])[:, None, None]

    def torch_call():
        grid = torch.stack([torch.remainder(u, 64.0) / 32.0 - 1.0, torch.remainder(v, 64.0) / 32.0 - 1.0], dim=-1)
        return torch_relief(tex, grid, base, weave.top_mm)

    out.append(("(y4) torch ops with grid_sample (plane carrier, wrapping tile, minimum only)", repeated(torch_call, a.torch_calls, a.reps, 2), 4))

    def rate(v, px):
        return B * H * W * px / (stats(v)[0] * 1e-3) / 1e12

    lines = table(["B/px streamed", "TB/s over them", "share of the float4-copy rate"],
                  [(k, v, f"{px:g}", f"{rate(v, px):.2f}", f"{rate(v, px) / COPY_TBS:.2f}") for k, v, px in out])
    notes = [f"share of the pixels that take their taps: (a) {taps['a']:.2f}, (b) {taps['b']:.2f}, (c) {taps['c']:.2f}, (d) {taps['d']:.2f}; "
             f"the mesh of (y3) covers {mesh_seen:.2f} of the pixels",
             "B/px streamed counts the height map alone (4 B/px written; 8 where a second launch reads it back or copy_ reads and writes); "
             "the texel taps are served by L2 / the Infinity Cache and are not in it"]
    if not a.no_sensor:
        from _bench_util import sensor_update_yardstick
        from tacex_amd import GelSightSensor, GelSightSensorCfg
        from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
        from pathlib import Path

        calib = Path(a.repo) / "tacex_amd" / "assets" / "calib" / "gsmini_640x480"
        cfg = GelSightSensorCfg(
            num_envs=B, data_types=["tactile_rgb", "height_map"],
            sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
            optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib), gelpad_height=GH, gelpad_to_camera_min_distance=GD,
                                              tactile_img_res=(W, H), device="cuda"),
            device="cuda")
        sens = {}
        for tag, key in (("(y5) sensor update, relief source (b): sphere carrier", "b"), ("(y5) sensor update, relief source (a): whole frame in contact", "a")):
            s = GelSightSensor(cfg)
            s.set_height_map_source(srcs[key])
            sens[tag] = (lambda s=s: s.update(0.01, force_recompute=True))
        sm = rounds(sens, a.sensor_steps, a.reps, 3)
        sm = {"(y5) sensor update, indenter source (spheres)": sensor_update_yardstick(a.repo, B, H, W, a.reps)} | sm
        lines += [""] + table([], list(sm.items()), first="sensor update (one GelSightSensor, tactile_rgb)")
    head = (f"# Relief height-map source: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, {a.reps} "
            f"alternating rounds (median, min, max of the rounds), one MI355X; torch ops {a.torch_calls} calls, the sensor {a.sensor_steps} "
            f"updates per timing.  The height maps are {B * H * W * 4 / 1e9:.3f} GB: one write at the {COPY_TBS} TB/s float4-copy rate takes "
            f"{copy_ms(B * H * W * 4):.3f} ms.  The rate columns are derived: streamed bytes over the median.\n\n")
    emit(lines, a.out, head, notes)


if __name__ == "__main__":
    main()
