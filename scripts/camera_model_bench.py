"""Time of the sensor camera model (`TactileCameraModel`, one launch of tacex_camera_model) on 2048 frames of 320 x 240 - a C3 step's
`tactile_rgb` - for float32 -> uint8, float32 -> float32 and in place, each with and without a fixed pattern.  hipEvents around
`--calls` calls in a row, the variants alternating over `--reps` rounds after a warm-up.  Beside them, three yardsticks:
  - the bytes a call must move over the 6.29 TB/s float4-copy rate of one MI355X (derived, not measured);
  - the torch restatement a user would write without the kernel (randn_like, einsum, clamps, cast): not bit-equal, a cost comparison;
  - one sensor `update()` that renders those 2048 frames (height map from analytic indenters, tactile_rgb), for scale.

  --out FILE   also write the table as markdown."""
import numpy as np
import torch
from _bench_util import COPY_TBS, copy_ms, emit, parse_args, repeated, rounds, sensor_update_yardstick, table

a = parse_args(calls=200, torch_calls=10, torch_help="calls per timing of the torch restatement (it is tens of times slower)",
               extra=[("--no-update", dict(action="store_true", help="skip the sensor update() yardstick"))])

from tacex_amd import CameraProfile, TactileCameraModel  # noqa: E402

MIX = [[0.92, 0.06, 0.02], [0.03, 0.90, 0.05], [-0.02, 0.08, 1.05]]


def torch_restatement(x, M, o, read, shot, fixed_gain, u8):
    a = torch.einsum("bhwc,dc->bhwd", x, M) + o
    if fixed_gain is not None:
        a = a * fixed_gain
    a = a.clamp_(0, 1)
    v = (a + torch.sqrt(read * read + shot * a) * torch.randn_like(a)).clamp_(0, 1)
    return (v * 255 + 0.5).to(torch.uint8) if u8 else v


def main():
    B, H, W = a.frames, a.height, a.width
    dev = "cuda:0"
    x = torch.rand((B, H, W, 3), device=dev)
    out_u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    out_f32 = torch.empty_like(x)
    inplace = x.clone()
    nbytes = {"u8": B * H * W * 3 * (4 + 1), "f32": B * H * W * 3 * (4 + 4)}
    variants, kind = {}, {}
    for fp in (0.0, 0.02):
        prof = [CameraProfile(MIX, [0.01, 0.0, -0.01], 0.01, 2e-4, fp), CameraProfile(np.eye(3), 0.0, 0.02, 1e-4, fp)]
        tag = "fixed pattern" if fp else "no fixed pattern"
        mu = TactileCameraModel(prof, B, dev, seed=1, dtype=torch.uint8)
        mf = TactileCameraModel(prof, B, dev, seed=1, dtype=torch.float32)
        for m in (mu, mf):
            m.randomize(generator=torch.Generator(device=dev).manual_seed(2))
        variants[f"float32 -> uint8, {tag}"] = lambda m=mu: m(x, out=out_u8)
        variants[f"float32 -> float32, {tag}"] = lambda m=mf: m(x, out=out_f32)
        variants[f"float32 in place, {tag}"] = lambda m=mf: m(inplace, out=inplace)
        kind.update({f"float32 -> uint8, {tag}": "u8", f"float32 -> float32, {tag}": "f32", f"float32 in place, {tag}": "f32"})

    def row(k, v, floor):  # (floor: the bytes of a call over the copy rate, ms)
        return (k, v, f"{floor:.3f}", f"{floor / float(np.median(v)):.2f}")

    rows = [row(k, v, copy_ms(nbytes[kind[k]])) for k, v in rounds(variants, a.calls, a.reps, 10).items()]
    # the torch restatement (allocates its temporaries, like the code a user would write)
    M = torch.tensor(MIX, device=dev)
    o = torch.tensor([0.01, 0.0, -0.01], device=dev)
    gain = 1 + 0.02 * torch.randn((B, H, W, 3), device=dev)
    tv = {"torch restatement, float32 -> uint8, no fixed pattern": lambda: torch_restatement(x, M, o, 0.01, 2e-4, None, True),
          "torch restatement, float32 -> uint8, fixed pattern (gain tensor kept)": lambda: torch_restatement(x, M, o, 0.01, 2e-4, gain, True),
          "torch restatement, float32 -> float32, no fixed pattern": lambda: torch_restatement(x, M, o, 0.01, 2e-4, None, False)}
    for k, fn in tv.items():
        rows.append(row(k, repeated(fn, a.torch_calls, a.reps, 2), copy_ms(nbytes["u8" if "uint8" in k else "f32"])))
    del gain, inplace, out_f32
    torch.cuda.empty_cache()
    if not a.no_update:
        rows.append(row(f"sensor update() rendering the {B} frames (for scale)", sensor_update_yardstick(a.repo, B, H, W, a.reps), float("nan")))
    head = (f"# Sensor camera model: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds "
            f"(median, min, max of the rounds), one MI355X; the torch restatement {a.torch_calls} calls per timing, the sensor update 20.  "
            f"The copy-rate column is derived: the bytes a call must move ({nbytes['u8'] / 1e9:.2f} GB for uint8 output, {nbytes['f32'] / 1e9:.2f} GB "
            f"for float32) over the {COPY_TBS} TB/s float4-copy rate; the fraction is that time over the measured median.\n\n")
    emit(table(["bytes / 6.29 TB/s, ms", "fraction of the copy rate"], rows), a.out, head)


if __name__ == "__main__":
    main()
