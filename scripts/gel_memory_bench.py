"""Time of the gel memory (`TactileGelMemory.apply`, one launch of tacex_gel_memory) on 2048 frames of 320 x 240 - a C3 step's height
maps - warm, inputs resident, hipEvents around `--calls` calls in a row, the variants alternating over `--reps` rounds:
  (a) every frame dead (no contact, zero state), beside one read of the height maps measured in the same run: `tacex_indentation_depth`
      with and without the contact ranges (the passes the call stands in for), and `copy_` (a read and a write);
  (b) sparse contact, K = 1: a quarter of the frames in contact (a random quarter, and every fourth frame), the others dead;
  (c) every frame live, K = 1 and K = 2, against the float4-copy rate over the algorithmic bytes 4 + 4 + 8 K + 4 B/px;
  (d) the same model in torch ops (K = 1, every frame live);
  (e) a whole `GelSightSensor.update()` of one 2048-env sensor (tactile_rgb + FOTS markers from a camera depth image) without the model
      (depth pass deferred into the render, and not deferred) and with it (sparse contact, K = 1 and K = 2).
The map is rewritten in place, so a timed call works on the previous call's output: a pressed frame stays pressed (its imprint is a
penetration) and a dead frame stays dead - the traffic per call does not change.

  --out FILE   also write the table as markdown."""
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, repeated, rounds, stats, table

a = parse_args(calls=50, torch_calls=5, extra=[("--sensor-steps", dict(type=int, default=20)), ("--no-sensor", dict(action="store_true"))])

from tacex_amd import GelMemoryProfile, TactileGelMemory, _lib  # noqa: E402
from tacex_amd.gel_memory import rest_plane_mm  # noqa: E402
from tacex_amd.utils.synthetic import synthetic_depth_maps  # noqa: E402

GH, GD, DT = 0.0045, 0.024, 1.0 / 60.0
GELS = [GelMemoryProfile((0.05, 0.4), (0.5, 0.3)), GelMemoryProfile((0.12, 0.8), (0.6, 0.2))]


def torch_model(hm, state, a1, c1, floor, z0):
    """K = 1 of the contract in torch ops, the way a user would write it (temporaries allocated by torch)."""
    d = (z0 - hm).clamp_(min=0)
    m = a1 * state + c1 * d
    m = torch.where((d == 0) & (m < floor), torch.zeros_like(m), m)
    state.copy_(m)
    r = z0 - m
    hm.copy_(torch.where((m > 0) & (r < hm), r, hm))
    fmin = hm.amin(dim=(1, 2))
    live = (m != 0).flatten(1).any(dim=1)
    return fmin, live


def main():
    B, H, W = a.frames, a.height, a.width
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    st = _lib.current_stream_handle(dev)
    contact = synthetic_depth_maps(B, H, W, seed=3, device=dev, flat_fraction=0.0)[0].contiguous()
    flat = torch.full((B, H, W), 29.0, device=dev)
    # a quarter of the frames in contact: drawn at random (seeded), and every fourth frame - workgroups go to the 8 XCDs round robin, so
    # the strided batch puts all its live frames on two of them
    pick = torch.randperm(B, generator=torch.Generator().manual_seed(5))[:B // 4].to(dev)
    sparse, strided = flat.clone(), flat.clone()
    sparse[pick] = contact[pick]
    strided[::4] = contact[::4]
    z0 = rest_plane_mm(GH, GD)
    pressed = (contact < z0).flatten(1).any(dim=1)
    fmin, ind = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    rows = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    variants, bytes_px = {}, {}

    def memory(tag, src, K, px):
        model = TactileGelMemory(B, (W, H), GELS, terms=K, dt=DT, device=dev)
        model.randomize(generator=torch.Generator(device=dev).manual_seed(2))
        hm = src.clone()
        variants[tag] = lambda: model.apply(hm, fmin, ind, rows, gelpad_height=GH, gelpad_to_camera_min_distance=GD)
        bytes_px[tag] = px
        return model

    models = {
        "a": memory("(a) gel memory, every frame dead, K = 1", flat, 1, 4),
        "b": memory("(b) gel memory, a random quarter of the frames in contact, K = 1", sparse, 1, 4 + (4 + 8 + 4) / 4),
        "bs": memory("(b) gel memory, every fourth frame in contact, K = 1", strided, 1, 4 + (4 + 8 + 4) / 4),
        "c1": memory("(c) gel memory, every frame live, K = 1", contact, 1, 4 + 4 + 8 + 4),
        "c2": memory("(c) gel memory, every frame live, K = 2", contact, 2, 4 + 4 + 16 + 4),
    }
    rd = flat.clone()
    variants["one read: tacex_indentation_depth with contact ranges (frame_rows_kernel)"] = lambda: lib.tacex_indentation_depth(
        _lib.ptr(rd), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W, st)
    variants["one read: tacex_indentation_depth without ranges (frame_min_kernel)"] = lambda: lib.tacex_indentation_depth(
        _lib.ptr(rd), GH, GD, _lib.ptr(fmin), _lib.ptr(ind), 0, B, H, W, st)
    dst = torch.empty_like(rd)
    variants["copy of the height maps (copy_, read + write)"] = lambda: dst.copy_(rd)
    bytes_px.update({k: 4 for k in variants if k.startswith("one read")})
    bytes_px["copy of the height maps (copy_, read + write)"] = 8
    out = [(k, v, bytes_px[k]) for k, v in rounds(variants, a.calls, a.reps, 5).items()]
    live = {k: int(m.live.sum().item()) for k, m in models.items()}
    # (d) torch ops, K = 1, every frame live
    hm_t, state_t = contact.clone(), torch.zeros((B, H, W), device=dev)
    row = GELS[0].row(DT)
    fn = lambda: torch_model(hm_t, state_t, float(row[0]), float(row[1]), float(row[4]), z0)  # noqa: E731
    out.append(("(d) the model in torch ops, every frame live, K = 1", repeated(fn, a.torch_calls, a.reps, 2), 4 + 4 + 8 + 4))

    def rate(v, px):  # TB/s of the algorithmic bytes over the median
        return B * H * W * px / (stats(v)[0] * 1e-3) / 1e12

    lines = table(["algorithmic B/px", "TB/s over them", "share of the float4-copy rate"],
                  [(k, v, f"{px:g}", f"{rate(v, px):.2f}", f"{rate(v, px) / COPY_TBS:.2f}") for k, v, px in out])
    notes = [f"{int(pressed.sum().item())} of {B} frames of the contact batch hold a pressed pixel; live frames after the timed calls: "
             f"(a) {live['a']}, (b) {live['b']} and {live['bs']}, (c) K = 1 {live['c1']}, K = 2 {live['c2']}"]
    # (e) a whole sensor update
    if not a.no_sensor:
        import bench
        from tacex_amd import gelsight_sensor

        depth = {"sparse": (sparse / 1000.0).contiguous(), "dense": (contact / 1000.0).contiguous()}
        sens = []

        def sensor(tag, K, defer, data):
            s = bench.build_sensor(B, H, W, True, "cuda:0")
            if K:
                m = TactileGelMemory(B, (W, H), GELS, terms=K, dt=DT, device=dev)
                m.randomize(generator=torch.Generator(device=dev).manual_seed(2))
                s.set_gel_memory(m)

            def step():
                gelsight_sensor._DEFER_DEPTH = defer
                s.set_camera_depth(depth[data])
                s.update(DT, force_recompute=True)
            sens.append((tag, step))

        for data in ("sparse", "dense"):
            sensor(f"(e) sensor update, {data} contact, no model (depth pass deferred into the render)", 0, True, data)
            sensor(f"(e) sensor update, {data} contact, no model, depth pass not deferred", 0, False, data)
            sensor(f"(e) sensor update, {data} contact, gel memory K = 1", 1, True, data)
            sensor(f"(e) sensor update, {data} contact, gel memory K = 2", 2, True, data)
        sm = rounds(dict(sens), a.sensor_steps, a.reps, 3)
        gelsight_sensor._DEFER_DEPTH = True
        lines += [""] + table([], list(sm.items()), first="sensor update (one GelSightSensor, tactile_rgb + FOTS markers)")
    head = (f"# Gel memory: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds "
            f"(median, min, max of the rounds), one MI355X; torch ops {a.torch_calls} calls, the sensor {a.sensor_steps} updates per timing.  "
            f"The height maps are {B * H * W * 4 / 1e9:.3f} GB: one read at the {COPY_TBS} TB/s float4-copy rate takes "
            f"{copy_ms(B * H * W * 4):.3f} ms.  The rate columns are derived: algorithmic bytes over the median.\n\n")
    emit(lines, a.out, head, notes)


if __name__ == "__main__":
    main()
