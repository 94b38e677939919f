"""Time of the SDF scene height-map source (`SdfSceneSource.fill`: the marching launch of tacex_height_map_from_sdf_scene and the
indentation-depth launch behind it) on 2048 frames of 320 x 240, warm, inputs resident, hipEvents around `--calls` calls in a row, the
variants alternating over `--reps` rounds:
  (i)   a scene of ONE union slot against `SdfVolumeSource.fill` on the same volume and poses (a sphere, a gear; 64^3 grids);
  (ii)  union scenes of K = 2, 4, 8 small spheres, spread over the frame and overlapping in its middle, each against the composite the
        single-volume source allows: K `SdfVolumeSource.fill` calls, K - 1 `torch.minimum`, one tacex_indentation_depth;
  (iii) what only the scene can do: a plate minus a hole, and a blended pair.
Taps per marched pixel and live slots per tile are debug counts of the NumPy restatement (tests/sdf_scene_ref.py) on the first
`--ref-frames` frames of each scene.

  --out FILE   also write the table as markdown."""
import sys
from pathlib import Path

import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, rounds, table

a = parse_args(calls=20, torch_calls=0, extra=[("--ref-frames", dict(type=int, default=4))])
sys.path.insert(0, str(Path(a.repo) / "tests"))

import sdf_scene_ref as S  # noqa: E402
from tacex_amd import SdfSceneSource, SdfVolumeSource, _lib  # noqa: E402
from tacex_amd.utils import sdf_volumes  # noqa: E402

GH, GD, PIX, GEL_TOP = 0.0045, 0.024, 0.0295, 28.5


def main():
    B, H, W = a.frames, a.height, a.width
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    st = _lib.current_stream_handle(dev)
    g = torch.Generator().manual_seed(0)
    rnd = torch.rand((B, 8, 4), generator=g)
    quat = torch.randn((B, 8, 4), generator=g)
    fmin, ind = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    hm = torch.empty((B, H, W), device=dev)
    variants, scenes = {}, {}

    ball = sdf_volumes.from_function(lambda x, y, z: sdf_volumes.sphere_distance(x, y, z, 3.0), (64, 64, 64), 6.6 / 63)
    gear = sdf_volumes.from_function(lambda x, y, z: sdf_volumes.gear_field(x, y, z, 12, 2.2, 0.7, 1.6), (64, 64, 64), 6.6 / 63,
                                     sdf_volumes.gear_step_scale(12, 2.2, 0.7))
    plate = sdf_volumes.box((8.0, 6.0, 1.0), 0.1)
    vols = [ball, gear, plate]

    def scene(tag, K):
        src = SdfSceneSource(vols, B, dev, num_slots=K, pixmm=PIX)
        variants[tag] = lambda: src.fill(hm, fmin, ind, GH, GD, rows=rows)
        scenes[tag] = src
        return src

    def composite(tag, src):
        """What the single-volume source allows for the union scene `src`: one source per slot, the minimum of their maps."""
        K = src.num_slots
        singles, maps = [], [hm] + [torch.empty_like(hm) for _ in range(K - 1)]
        for k in range(K):
            one = SdfVolumeSource(vols, B, dev, pixmm=PIX)
            one.volume_ids.copy_(src.part_ids[:, k])
            one.pose.copy_(src.part_pose[:, k])
            singles.append(one)

        def run():
            for one, m in zip(singles, maps):
                one.fill(m, fmin, None, GH, GD)
            for m in maps[1:]:
                torch.minimum(hm, m, out=hm)
            lib.tacex_indentation_depth(_lib.ptr(hm), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W, st)

        variants[tag] = run

    # (i) one slot against the volume source
    cx, cy, press = (0.3 + 0.4 * rnd[:, 0, 0]) * W, (0.3 + 0.4 * rnd[:, 0, 1]) * H, 0.2 + 1.3 * rnd[:, 0, 2]
    for name, vid in (("sphere R = 3 mm", 0), ("gear", 1)):
        one = SdfVolumeSource(vols, B, dev, pixmm=PIX)
        one.volume_ids.fill_(vid)
        one.set_pose(cx, cy, quat[:, 0], press_mm=press)
        variants[f"(i) SdfVolumeSource, {name} on 64^3"] = (lambda one=one: one.fill(hm, fmin, ind, GH, GD, rows=rows))
        src = scene(f"(i) scene of one union slot, {name} on 64^3", 1)
        src.set_part(0, volume_id=vid, op="union")
        src.part_pose[:, 0] = one.pose
    # (ii) K small spheres (the ball at 0.3 x: R = 0.9 mm), spread on a grid over the frame / overlapping in its middle
    for K in (2, 4, 8):
        nx, ny = {2: (2, 1), 4: (2, 2), 8: (4, 2)}[K]
        for layout in ("spread", "overlapping"):
            src = scene(f"(ii) scene, union of {K} spheres, {layout}", K)
            for k in range(K):
                if layout == "spread":
                    px, py = (k % nx + 0.5) / nx * W, (k // nx + 0.5) / ny * H
                else:
                    px, py = 0.5 * W, 0.5 * H
                jit = 20.0 if layout == "spread" else 40.0
                src.set_part(k, volume_id=0, op="union")
                src.set_pose(k, px + jit * (rnd[:, k, 0] - 0.5), py + jit * (rnd[:, k, 1] - 0.5), quat[:, k],
                             z_mm=GEL_TOP - (0.2 + 0.8 * rnd[:, k, 2]) + 0.9, scale=0.3)
            composite(f"(ii) composite, {K} x SdfVolumeSource.fill + minimum + indentation depth, {layout}", src)
    # (iii) a plate minus a hole; a blended pair
    src = scene("(iii) scene, plate 8 x 6 x 1 mm minus a ball (R = 1.2 mm)", 2)
    src.set_part(0, volume_id=2, op="union")
    src.set_part(1, volume_id=0, op="subtract")
    flat = (1.0, 0.0, 0.0, 0.0)
    src.set_pose(0, 0.5 * W, 0.5 * H, flat, z_mm=GEL_TOP - press + 0.5)
    src.set_pose(1, cx, cy, quat[:, 1], z_mm=GEL_TOP - press, scale=0.4)
    src = scene("(iii) scene, two spheres (R = 1.5 mm) blended over 0.6 mm", 2)
    for k in range(2):
        src.set_part(k, volume_id=0, op="union")
        src.set_pose(k, cx + (60.0 * k - 30.0), cy, quat[:, k], z_mm=GEL_TOP - press + 1.5, scale=0.5, blend_mm=0.6)

    ms = rounds(variants, a.calls, a.reps, 3)
    cells = {}
    for tag, fn in variants.items():
        fn()
        seen = float((hm < 29.0).float().mean().item())
        counts = ""
        if tag in scenes and a.ref_frames > 0:
            s, n, stats = scenes[tag], min(a.ref_frames, B), {}
            S.height_map(s.voxels.cpu().numpy(), s.volumes_i.cpu().numpy(), s.volumes_f.cpu().numpy(), s.part_ids[:n].cpu().numpy(),
                         s.part_pose[:n].cpu().numpy(), s.part_ops[:n].cpu().numpy(), H, W, PIX, s.near_clip_mm, s.far_clip_mm, s.max_steps,
                         s.tol_mm, stats)
            live = s.num_slots - (stats["culled_slots"] + stats["empty_slots"] * stats["tiles"] / n) / stats["tiles"]
            counts = (f"{stats['taps'] / max(stats['covered'], 1):.2f} / {stats['outside_skipped'] / max(stats['covered'], 1):.2f} / "
                      f"{live:.2f} / {stats['dead_tiles'] / stats['tiles']:.2f}")
        cells[tag] = (f"{seen:.2f}", counts)
    lines = table(["share of pixels in contact", "taps per marched pixel / slot evaluations skipped per marched pixel / live slots per tile / share of tiles without a live union slot"],
                  [(k, v, *cells[k]) for k, v in ms.items()])
    notes = [f"the counts: the NumPy restatement on the first {min(a.ref_frames, B)} frames of the scene; a marched pixel is one whose ray meets a "
             "live union slot's box inside the clip range"]
    head = (f"# SDF scene height-map source: one call on {B} frames of {W} x {H}\n\n`python scripts/sdf_scene_bench.py --out profiles/sdf_scene_bench.md`: "
            f"{a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds (median, min, max of the rounds), one MI355X.  The height "
            f"maps are {B * H * W * 4 / 1e9:.3f} GB: one write at the {COPY_TBS} TB/s float4-copy rate takes {copy_ms(B * H * W * 4):.3f} ms.\n\n")
    emit(lines, a.out, head, notes)


if __name__ == "__main__":
    main()
