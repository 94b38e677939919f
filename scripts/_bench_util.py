"""What the stage benches share (camera_model_bench, lens_model_bench, contact_field_bench, gel_memory_bench): the command line, the
hipEvent timer, the warm-up and alternating-rounds loop, the copy-rate yardstick and the table / `--out` writer.  The tables under
profiles/ were recorded with these steps; a bench keeps its own variants, columns and header text."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

COPY_TBS = 6.29  # measured float4-copy rate of one MI355X (HBM3E, 79 % of the 8.0 TB/s datasheet peak; profiles/contact_field_bench.md)


def parse_args(calls, torch_calls, torch_help=None, extra=()):
    """--repo --frames --height --width --calls --reps --torch-calls [extra: (flag, add_argument keywords)] --out; puts --repo
    first on sys.path (import tacex_amd after this call)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--calls", type=int, default=calls)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-calls", type=int, default=torch_calls, help=torch_help)
    for flag, kw in extra:
        ap.add_argument(flag, **kw)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.repo)
    return a


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls  # ms per call


def rounds(variants, calls, reps, warmup):
    """name -> [ms per call, one per round]: every variant warmed up, then the variants alternating over `reps` rounds."""
    for fn in variants.values():
        timed(fn, warmup)
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            ms[k].append(timed(fn, calls))
    return ms


def repeated(fn, calls, reps, warmup):
    """[ms per call, one per round] of a yardstick timed on its own."""
    timed(fn, warmup)
    return [timed(fn, calls) for _ in range(reps)]


def stats(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def copy_ms(nbytes):
    """ms that `nbytes` take at the float4-copy rate (derived, not measured)."""
    return nbytes / (COPY_TBS * 1e12) * 1e3


def table(columns, rows, first="case"):
    """Markdown lines: `first` | median ms | min | max | columns...; a row is (name, [ms of the rounds], *formatted cells)."""
    lines = ["| " + " | ".join([first, "median ms", "min", "max", *columns]) + " |", "|---" * (4 + len(columns)) + "|"]
    for name, v, *cells in rows:
        lines.append("| " + " | ".join([name, *(f"{x:.3f}" for x in stats(v)), *cells]) + " |")
    return lines


def emit(lines, out, head, notes=()):
    """Print the table (and the notes); --out FILE: head, table and the notes as a list."""
    print("\n".join(list(lines) + ([""] + list(notes) if notes else [])), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(head + "\n".join(lines) + "\n" + ("\n" + "\n".join(f"- {n}" for n in notes) + "\n" if notes else ""))


def sensor_update_yardstick(repo, B, H, W, reps):
    """[ms] of one sensor `update()` that renders B frames (height map from analytic indenters, tactile_rgb), 20 updates per timing."""
    from tacex_amd import GelSightSensor, GelSightSensorCfg, IndenterHeightMapSource
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
    from tacex_amd.utils.synthetic import PIXMM

    calib = Path(repo) / "tacex_amd" / "assets" / "calib" / "gsmini_640x480"
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
    return repeated(lambda: s.update(0.01, force_recompute=True), 20, reps, 5)
