"""Time of the sensor camera model (`TactileCameraModel`, one launch of tacex_camera_model) on 2048 frames of 320 x 240 - a C3 step's
`tactile_rgb` - for float32 -> uint8, float32 -> float32 and in place, each with and without a fixed pattern.  hipEvents around
`--calls` calls in a row, the variants alternating over `--reps` rounds after a warm-up.  Beside them, three yardsticks:
  - the bytes a call must move over the 6.29 TB/s float4-copy rate of one MI355X (derived, not measured);
  - the torch restatement a user would write without the kernel (randn_like, einsum, clamps, cast): not bit-equal, a cost comparison;
  - one sensor `update()` that renders those 2048 frames (height map from analytic indenters, tactile_rgb), for scale.

  --out FILE   also write the table as markdown."""
import argparse
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--frames", type=int, default=2048)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-calls", type=int, default=10, help="calls per timing of the torch restatement (it is tens of times slower)")
ap.add_argument("--no-update", action="store_true", help="skip the sensor update() yardstick")
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, a.repo)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacex_amd import CameraProfile, TactileCameraModel  # noqa: E402

COPY_TBS = 6.29  # measured float4-copy rate of one MI355X (HBM3E, 79 % of the 8.0 TB/s datasheet peak)
MIX = [[0.92, 0.06, 0.02], [0.03, 0.90, 0.05], [-0.02, 0.08, 1.05]]


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls  # ms per call


def torch_restatement(x, M, o, read, shot, fixed_gain, u8):
    a = torch.einsum("bhwc,dc->bhwd", x, M) + o
    if fixed_gain is not None:
        a = a * fixed_gain
    a = a.clamp_(0, 1)
    v = (a + torch.sqrt(read * read + shot * a) * torch.randn_like(a)).clamp_(0, 1)
    return (v * 255 + 0.5).to(torch.uint8) if u8 else v


def update_yardstick(B, H, W):
    from tacex_amd import GelSightSensor, GelSightSensorCfg, IndenterHeightMapSource
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
    from tacex_amd.utils.synthetic import PIXMM

    calib = Path(a.repo) / "tacex_amd" / "assets" / "calib" / "gsmini_640x480"
    cfg = GelSightSensorCfg(
        num_envs=B, data_types=["tactile_rgb", "height_map"],
        sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                          tactile_img_res=(W, H), device="cuda"),
        device="cuda")
    s = GelSightSensor(cfg)
    src = IndenterHeightMapSource(B, "cuda", pixmm=PIXMM)
    g = torch.Generator().manual_seed(0)
    u = torch.rand((B, 4), generator=g)
    src.set("sphere", cx=(0.3 + 0.4 * u[:, 0]) * W, cy=(0.3 + 0.4 * u[:, 1]) * H, r=(0.15 + 0.2 * u[:, 2]) * H, press_mm=0.2 + 1.3 * u[:, 3])
    s.set_height_map_source(src)
    fn = lambda: s.update(0.01, force_recompute=True)  # noqa: E731
    timed(fn, 5)
    return [timed(fn, 20) for _ in range(a.reps)], s


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
    for fn in variants.values():
        timed(fn, 10)
    ms = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn, a.calls))
    rows = []
    for k, v in ms.items():
        floor = nbytes[kind[k]] / (COPY_TBS * 1e12) * 1e3
        med = float(np.median(v))
        rows.append((k, med, float(min(v)), float(max(v)), floor, floor / med))
    # the torch restatement (allocates its temporaries, like the code a user would write)
    M = torch.tensor(MIX, device=dev)
    o = torch.tensor([0.01, 0.0, -0.01], device=dev)
    gain = 1 + 0.02 * torch.randn((B, H, W, 3), device=dev)
    tv = {"torch restatement, float32 -> uint8, no fixed pattern": lambda: torch_restatement(x, M, o, 0.01, 2e-4, None, True),
          "torch restatement, float32 -> uint8, fixed pattern (gain tensor kept)": lambda: torch_restatement(x, M, o, 0.01, 2e-4, gain, True),
          "torch restatement, float32 -> float32, no fixed pattern": lambda: torch_restatement(x, M, o, 0.01, 2e-4, None, False)}
    for k, fn in tv.items():
        timed(fn, 2)
        v = [timed(fn, a.torch_calls) for _ in range(a.reps)]
        floor = nbytes["u8" if "uint8" in k else "f32"] / (COPY_TBS * 1e12) * 1e3
        rows.append((k, float(np.median(v)), float(min(v)), float(max(v)), floor, floor / float(np.median(v))))
    del gain, inplace, out_f32
    torch.cuda.empty_cache()
    if not a.no_update:
        v, _s = update_yardstick(B, H, W)
        rows.append((f"sensor update() rendering the {B} frames (for scale)", float(np.median(v)), float(min(v)), float(max(v)), float("nan"), float("nan")))
    lines = ["| case | median ms | min | max | bytes / 6.29 TB/s, ms | fraction of the copy rate |", "|---|---|---|---|---|---|"]
    lines += [f"| {k} | {m:.3f} | {lo:.3f} | {hi:.3f} | {fl:.3f} | {fr:.2f} |" for k, m, lo, hi, fl, fr in rows]
    print("\n".join(lines), flush=True)
    if a.out:
        head = (f"# Sensor camera model: one call on {B} frames of {W} x {H}\n\n{a.calls} calls per timing between two hipEvents, {a.reps} alternating rounds "
                f"(median, min, max of the rounds), one MI355X; the torch restatement {a.torch_calls} calls per timing, the sensor update 20.  "
                f"The copy-rate column is derived: the bytes a call must move ({nbytes['u8'] / 1e9:.2f} GB for uint8 output, {nbytes['f32'] / 1e9:.2f} GB "
                f"for float32) over the {COPY_TBS} TB/s float4-copy rate; the fraction is that time over the measured median.\n\n")
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
