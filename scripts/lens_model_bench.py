"""Time of the sensor lens model (`TactileLensModel`) on 2048 frames of 320 x 240 - a C3 step's `tactile_rgb`: the gather alone with
one tap and with four taps per pixel, the fused lens + camera launch (`tacex_lens_camera_model`) to uint8 and to float32, and the two
separate launches (`tacex_lens_model`, then `tacex_camera_model`) it replaces.  hipEvents around `--calls` calls in a row, the
variants alternating over `--reps` rounds after a warm-up.  Beside them, three yardsticks:
  - the bytes a call must move over the 6.29 TB/s float4-copy rate of one MI355X (derived, not measured);
  - the torch restatement a user would write without the kernel (an explicit sampling grid, grid_sample, the vignette multiply):
    not bit-equal, a cost comparison;
  - one sensor `update()` that renders those 2048 frames (height map from analytic indenters, tactile_rgb), for scale.

  --out FILE   also write the table as markdown."""
import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, repeated, rounds, sensor_update_yardstick, table

a = parse_args(calls=200, torch_calls=10, torch_help="calls per timing of the torch restatement (it is many times slower)",
               extra=[("--no-update", dict(action="store_true", help="skip the sensor update() yardstick"))])

from tacex_amd import CameraProfile, LensProfile, TactileCameraModel, TactileLensModel  # noqa: E402

MIX = [[0.92, 0.06, 0.02], [0.03, 0.90, 0.05], [-0.02, 0.08, 1.05]]
ONE_TAP = [LensProfile(k1=-0.15, k2=0.03, rotation_deg=1.5, scale=1.02, shift_px=(2.5, -1.0), vignette=(-0.25, -0.05)),
           LensProfile(k1=-0.10, k2=0.01, p1=0.004, p2=-0.003, rotation_deg=-0.8, scale=0.99, centre_px=(4.5, -3.25), vignette=(-0.2, -0.1))]
FOUR_TAPS = [LensProfile(k1=-0.15, k2=0.03, rotation_deg=1.5, scale=1.02, shift_px=(2.5, -1.0), vignette=(-0.25, -0.05), softness=(0.3, 1.2)),
             LensProfile(k1=-0.10, k2=0.01, p1=0.004, p2=-0.003, rotation_deg=-0.8, scale=0.99, centre_px=(4.5, -3.25), vignette=(-0.2, -0.1),
                         softness=(0.5, 0.8))]


def torch_restatement(x_nchw, rows, H, W):
    """One tap per pixel: the source grid of every env from its row, grid_sample (bilinear, border), the vignette gain."""
    r = rows.view(-1, 16, 1, 1)
    k1, k2, p1, p2, e00, e01, e10, e11, tx, ty, cx, cy, v1, v2 = (r[:, k] for k in range(14))
    j = torch.arange(W, device=x_nchw.device, dtype=torch.float32).view(1, 1, W)
    i = torch.arange(H, device=x_nchw.device, dtype=torch.float32).view(1, H, 1)
    px, py = j + 0.5 - W / 2 - cx, i + 0.5 - H / 2 - cy
    xn, yn = px * (2 / W), py * (2 / W)
    r2 = xn * xn + yn * yn
    rad = (k1 + k2 * r2) * r2
    dx = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    dy = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    u = j + e00 * px + e01 * py + (W / 2) * dx + tx
    v = i + e10 * px + e11 * py + (W / 2) * dy + ty
    grid = torch.stack([(2 * u + 1) / W - 1, (2 * v + 1) / H - 1], -1)  # align_corners=False
    g = (1 + (v1 + v2 * r2) * r2).clamp_(0, 1)
    return torch.nn.functional.grid_sample(x_nchw, grid, mode="bilinear", padding_mode="border", align_corners=False) * g.unsqueeze(1)


def main():
    B, H, W = a.frames, a.height, a.width
    dev = "cuda:0"
    x = torch.rand((B, H, W, 3), device=dev)
    mid = torch.empty_like(x)
    out_f32 = torch.empty_like(x)
    out_u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    px = B * H * W
    gen = lambda: torch.Generator(device=dev).manual_seed(2)  # noqa: E731
    lens1, lens4 = TactileLensModel(ONE_TAP, B, dev), TactileLensModel(FOUR_TAPS, B, dev)
    prof = [CameraProfile(MIX, [0.01, 0.0, -0.01], 0.01, 2e-4, 0.02), CameraProfile(np.eye(3), 0.0, 0.02, 1e-4, 0.02)]
    cam_u8 = TactileCameraModel(prof, B, dev, seed=1, dtype=torch.uint8)
    cam_f32 = TactileCameraModel(prof, B, dev, seed=1, dtype=torch.float32)
    for m in (lens1, lens4, cam_u8, cam_f32):
        m.randomize(generator=gen())

    def two(cam, out):
        lens1(x, out=mid)
        cam(mid, out=out)

    # name -> (call, bytes per pixel a call must move)
    variants = {
        "lens alone, one tap": (lambda: lens1(x, out=out_f32), 24),
        "lens alone, four taps": (lambda: lens4(x, out=out_f32), 24),
        "fused lens + camera -> uint8 (one tap, fixed pattern)": (lambda: lens1(x, out=out_u8, camera=cam_u8), 15),
        "two launches, lens then camera -> uint8": (lambda: two(cam_u8, out_u8), 39),
        "fused lens + camera -> float32 (one tap, fixed pattern)": (lambda: lens1(x, out=out_f32, camera=cam_f32), 24),
        "two launches, lens then camera -> float32": (lambda: two(cam_f32, out_f32), 48),
    }

    def row(k, v, bytes_px):  # (the bytes of a call over the copy rate, ms)
        floor = copy_ms(bytes_px * px)
        return (k, v, f"{floor:.3f}", f"{floor / float(np.median(v)):.2f}")

    ms = rounds({k: fn for k, (fn, _) in variants.items()}, a.calls, a.reps, 10)
    rows = [row(k, v, variants[k][1]) for k, v in ms.items()]
    # the torch restatement (allocates its temporaries, like the code a user would write); channels-last view of the NHWC batch
    x_nchw = x.permute(0, 3, 1, 2)
    lens_rows = lens1.profiles[lens1.profile_ids.long()]
    tfn = lambda: torch_restatement(x_nchw, lens_rows, H, W)  # noqa: E731
    rows.append(row("torch restatement, one tap (explicit grid, grid_sample, vignette)", repeated(tfn, a.torch_calls, a.reps, 2), 24))
    del mid, out_f32, out_u8
    torch.cuda.empty_cache()
    if not a.no_update:
        rows.append(row(f"sensor update() rendering the {B} frames (for scale)", sensor_update_yardstick(a.repo, B, H, W, a.reps), float("nan")))
    head = (f"# Sensor lens model: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds "
            f"(median, min, max of the rounds), one MI355X; the torch restatement {a.torch_calls} calls per timing, the sensor update 20.  "
            f"The copy-rate column is derived: the bytes a call must move (12 B / pixel in; 12 out for float32, 3 for uint8; the two launches "
            f"also write and read the 12 B / pixel between them) over the {COPY_TBS} TB/s float4-copy rate; the fraction is that time over "
            f"the measured median.\n\n")
    emit(table(["bytes / 6.29 TB/s, ms", "fraction of the copy rate"], rows), a.out, head)


if __name__ == "__main__":
    main()
