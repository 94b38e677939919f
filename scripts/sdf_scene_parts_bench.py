"""Time of the part map and of the per-part contact records on 2048 frames of 320 x 240, warm, inputs resident, hipEvents around
`--calls` calls in a row, the variants alternating over `--reps` rounds:
  (a) `SdfSceneSource.fill` on the scenes of scripts/sdf_scene_bench.py - one union slot (sphere, gear), unions of 2, 4, 8 spheres spread
      and overlapping, a plate minus a hole, a blended pair - without and with `part_map=True` (tacex_height_map_from_sdf_scene against
      tacex_height_map_from_sdf_scene_parts: the same kernel source, the owner compiled in), one beside the other in every round;
  (b) `tacex_contact_field_parts` (records only, contact rectangles) at L = 1, 2, 4, 8 labels against `tacex_contact_field` record-only
      on the same height maps: those of the spread 8-sphere scene, labelled by its part map modulo L.

  --out FILE   also write the tables as markdown."""
import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, rounds, stats, table

a = parse_args(calls=20, torch_calls=0)

from tacex_amd import ContactGel, SdfSceneSource, TactileContactModel, _lib  # noqa: E402
from tacex_amd.utils import sdf_volumes  # noqa: E402

GH, GD, PIX, GEL_TOP = 0.0045, 0.024, 0.0295, 28.5


def main():
    B, H, W = a.frames, a.height, a.width
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rnd = torch.rand((B, 8, 4), generator=g)
    quat = torch.randn((B, 8, 4), generator=g)
    fmin, ind = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    hm = torch.empty((B, H, W), device=dev)
    ball = sdf_volumes.from_function(lambda x, y, z: sdf_volumes.sphere_distance(x, y, z, 3.0), (64, 64, 64), 6.6 / 63)
    gear = sdf_volumes.from_function(lambda x, y, z: sdf_volumes.gear_field(x, y, z, 12, 2.2, 0.7, 1.6), (64, 64, 64), 6.6 / 63,
                                     sdf_volumes.gear_step_scale(12, 2.2, 0.7))
    vols = [ball, gear, sdf_volumes.box((8.0, 6.0, 1.0), 0.1)]
    variants, pairs = {}, {}

    def scene(tag, K, place):
        """The same scene twice: without and with the part map."""
        for with_map in (False, True):
            src = SdfSceneSource(vols, B, dev, num_slots=K, pixmm=PIX, part_map=with_map)
            place(src)
            variants[f"{tag}{', part map' if with_map else ''}"] = lambda src=src: src.fill(hm, fmin, ind, GH, GD, rows=rows)
            pairs.setdefault(tag, []).append(src)

    cx, cy, press = (0.3 + 0.4 * rnd[:, 0, 0]) * W, (0.3 + 0.4 * rnd[:, 0, 1]) * H, 0.2 + 1.3 * rnd[:, 0, 2]
    flat = (1.0, 0.0, 0.0, 0.0)
    for name, vid in (("sphere R = 3 mm", 0), ("gear", 1)):
        def one(src, vid=vid):
            src.set_part(0, volume_id=vid, op="union")
            src.set_pose(0, cx, cy, quat[:, 0], press_mm=press)
        scene(f"one union slot, {name} on 64^3", 1, one)
    for K in (2, 4, 8):
        nx, ny = {2: (2, 1), 4: (2, 2), 8: (4, 2)}[K]
        for layout in ("spread", "overlapping"):
            def spheres(src, K=K, nx=nx, ny=ny, layout=layout):
                for k in range(K):
                    px, py = ((k % nx + 0.5) / nx * W, (k // nx + 0.5) / ny * H) if layout == "spread" else (0.5 * W, 0.5 * H)
                    jit = 20.0 if layout == "spread" else 40.0
                    src.set_part(k, volume_id=0, op="union")
                    src.set_pose(k, px + jit * (rnd[:, k, 0] - 0.5), py + jit * (rnd[:, k, 1] - 0.5), quat[:, k],
                                 z_mm=GEL_TOP - (0.2 + 0.8 * rnd[:, k, 2]) + 0.9, scale=0.3)
            scene(f"union of {K} spheres, {layout}", K, spheres)

    def plate(src):
        src.set_part(0, volume_id=2, op="union")
        src.set_part(1, volume_id=0, op="subtract")
        src.set_pose(0, 0.5 * W, 0.5 * H, flat, z_mm=GEL_TOP - press + 0.5)
        src.set_pose(1, cx, cy, quat[:, 1], z_mm=GEL_TOP - press, scale=0.4)
    scene("plate 8 x 6 x 1 mm minus a ball (R = 1.2 mm)", 2, plate)

    def pair(src):
        for k in range(2):
            src.set_part(k, volume_id=0, op="union")
            src.set_pose(k, cx + (60.0 * k - 30.0), cy, quat[:, k], z_mm=GEL_TOP - press + 1.5, scale=0.5, blend_mm=0.6)
    scene("two spheres (R = 1.5 mm) blended over 0.6 mm", 2, pair)

    ms = rounds(variants, a.calls, a.reps, 3)
    rows_a = []
    for tag, (plain, parts) in pairs.items():
        base = float(np.median(ms[tag]))
        for name in (tag, tag + ", part map"):
            variants[name]()
            seen = float((hm < 29.0).float().mean().item())
            rows_a.append((name, ms[name], f"{seen:.2f}", f"{float(np.median(ms[name])) / base:.3f}"))
        far = hm >= 29.0
        assert torch.equal(parts.part_map == 255, far) and (parts.part_map[~far] < parts.num_slots).all().item(), tag
    lines = table(["share of pixels in contact", "median / median without the part map"], rows_a)

    # (b) the per-part records on the spread 8-sphere scene's maps
    src = pairs["union of 8 spheres, spread"][1]
    src.fill(hm, fmin, ind, GH, GD, rows=rows)
    model = TactileContactModel([ContactGel(3.0e4, 1.2e4, 0.6), ContactGel(8.0e4, 5.0e4, 0.35)], B, dev, pixmm=PIX, grid=(1, 1))
    model.randomize(generator=torch.Generator(device=dev).manual_seed(2))
    u = torch.rand((B, 8, 5), generator=g)
    slip = torch.stack((0.06 * (u[..., 0] - 0.5), 0.06 * (u[..., 1] - 0.5), 0.2 * (u[..., 2] - 0.5), (0.3 + 0.4 * u[..., 3]) * W,
                        (0.3 + 0.4 * u[..., 4]) * H), dim=-1).to(dev)
    lib, st = _lib.load_library(), _lib.current_stream_handle(dev)
    rec1 = torch.empty((B, 16), dtype=torch.float64, device=dev)
    contact = {"tacex_contact_field, record only, contact rectangles": lambda s=slip[:, 0].contiguous(): lib.tacex_contact_field(
        _lib.ptr(hm), _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(model.gels), model.num_gels, _lib.ptr(model.gel_ids), _lib.ptr(s), PIX, _lib.ptr(rows),
        1, 1, _lib.ptr(rec1), 0, 0, B, H, W, st)}
    for L in (1, 2, 4, 8):
        labels = torch.where(src.part_map == 255, src.part_map, src.part_map % L).contiguous()
        rec = torch.empty((B, L, 16), dtype=torch.float64, device=dev)
        contact[f"tacex_contact_field_parts, L = {L}, records only, contact rectangles"] = (
            lambda labels=labels, rec=rec, L=L, s=slip[:, :L].contiguous(): lib.tacex_contact_field_parts(
                _lib.ptr(hm), _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(model.gels), model.num_gels, _lib.ptr(model.gel_ids), _lib.ptr(labels), L,
                _lib.ptr(s), PIX, _lib.ptr(rows), _lib.ptr(rec), 0, B, H, W, st))
    ms_b = rounds(contact, 5 * a.calls, a.reps, 5)
    base = stats(next(iter(ms_b.values())))[0]
    r = rows.cpu().numpy().astype(np.int64)
    rect = np.clip(r[:, 1] - r[:, 0] + 1, 0, None) * np.clip(r[:, 3] - r[:, 2] + 1, 0, None)
    lines += ["", f"Per-part contact records on the maps of the spread 8-sphere scene (the contact rectangles cover {rect.sum() / (B * H * W):.1%} of the "
              f"pixels), labels = part map modulo L, {5 * a.calls} calls per timing:", ""]
    lines += table(["median / tacex_contact_field"], [(k, v, f"{stats(v)[0] / base:.2f}") for k, v in ms_b.items()])
    head = (f"# Part map and per-part contact records: one call on {B} frames of {W} x {H}\n\n`python scripts/sdf_scene_parts_bench.py --out "
            f"profiles/sdf_scene_parts_bench.md`: {a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds (median, min, max of "
            f"the rounds), one MI355X.  The height maps are {B * H * W * 4 / 1e9:.3f} GB, the part map {B * H * W / 1e9:.3f} GB: one write of it at the "
            f"{COPY_TBS} TB/s float4-copy rate takes {copy_ms(B * H * W):.3f} ms.\n\n")
    emit(lines, a.out, head)


if __name__ == "__main__":
    main()
