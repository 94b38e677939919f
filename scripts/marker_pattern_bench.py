"""Marker-flow timing on the C4 pad (FemGelpad's breathing scene, 512 envs): the static grid's one launch, the marker pattern library's one
launch, and the host path with randomised ranges that the library replaces.  hipEvents; warm-up first; every figure is per CALL of
`gen_marker_flow_fused(out_f32=marker_data)` (the plugin's per-step call) unless it says otherwise.

  --static         `tacex_fem_marker_flow` on the static grid.  Uses only what existed before the library, so `--repo DIR` can point it at
                   a checkout of an older commit (with its own built libtacex_hip.so): run it alternately on both trees for an A/B.
  --host           the host path with the randomised ranges and NO library (`gen_marker_flow()`: grid + weights rebuilt on the host per
                   call), a handful of calls with a host clock around a device synchronise.  Old API only as well (`--repo`).
  --trace P        nothing but `--iters` library launches at P patterns with loss and noise on: the program for
                   `rocprofv3 --kernel-trace --stats -- python scripts/marker_pattern_bench.py --trace 64`.
  (default)        the static grid, then the library at every P of `--p` with loss and noise off and with probability 0.01, sigma 0.5.

Two figures per configuration: "gpu" is the median time between two events around ONE call (kernel + its launch gap), "stream" is the time
of `--iters` back-to-back calls between two events divided by their number (what a step loop pays; the larger of host enqueue and device)."""
import argparse
import sys
import time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--envs", type=int, default=512)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--markers", type=int, default=128)
ap.add_argument("--static", action="store_true")
ap.add_argument("--host", action="store_true")
ap.add_argument("--host-calls", type=int, default=5)
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--p", default="1,64,512")
a = ap.parse_args()
sys.path.insert(0, a.repo)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tacex_amd.simulation_approaches.fem_based.sim.tactile_sensor_uipc import VisionTactileSensorUIPC  # noqa: E402
from tacex_amd.uipc import gelpad_scene  # noqa: E402

CAM = (0.008, 0.012625, -0.024)  # the C4 entry's camera (bench.py)
RANGES = dict(marker_interval_range=(1.95, 2.15), marker_rotation_range=0.1, marker_translation_range=(1.0, 1.0),
              marker_pos_shift_range=(0.1, 0.1))


def scene(B):
    """The C4 pad at rest (sensors take their reference surface at construction); `press` dents it."""
    fem = gelpad_scene.FemGelpad(B, "cuda:0")

    def press():
        for i in range(8):
            fem.step(i)
        torch.cuda.synchronize()

    return fem, press


def sensor(fem, **kw):
    return VisionTactileSensorUIPC(fem.gelpad, fem.sim, torch.tensor(CAM, dtype=torch.float64), torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64),
                                   num_markers=a.markers, **kw)


def time_calls(ms, out):
    call = lambda: ms.gen_marker_flow_fused(out_f32=out)  # noqa: E731
    for _ in range(a.warmup):
        assert call() is out
    torch.cuda.synchronize()
    res = []
    for _ in range(a.reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        single = float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        res.append((single, s.elapsed_time(e) * 1e3 / a.iters))
    return "; ".join(f"gpu {g:6.1f} us, stream {t:6.1f} us" for g, t in res)


def main():
    B = a.envs
    print(f"tree {a.repo}, {B} envs, {a.markers} markers, {a.iters} timed calls after {a.warmup}, {a.reps} repetitions", flush=True)
    fem, press = scene(B)
    out = torch.zeros((B, 2, a.markers, 2), dtype=torch.float32, device="cuda:0")
    if a.host:
        ms = sensor(fem, marker_random_noise=0.5, marker_lose_tracking_probability=0.01, **RANGES)
        press()
        ms.gen_marker_flow()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.host_calls):
            t0 = time.perf_counter()
            ms.gen_marker_flow()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        print(f"  host path, randomised ranges: {np.median(t):.2f} ms per call (median of {a.host_calls}; min {min(t):.2f}, max {max(t):.2f})", flush=True)
        return
    if a.trace:
        ms = sensor(fem, marker_patterns=a.trace, marker_random_noise=0.5, marker_lose_tracking_probability=0.01, **RANGES)
        press()
        for _ in range(a.iters):
            ms.gen_marker_flow_fused(out_f32=out)
        torch.cuda.synchronize()
        print(f"  {a.iters} library launches at P = {a.trace}", flush=True)
        return
    static = sensor(fem)
    libs = []
    if not a.static:
        for p in (int(s) for s in a.p.split(",")):
            t0 = time.perf_counter()
            libs.append((p, sensor(fem, marker_patterns=p, **RANGES)))
            print(f"  library of {p:3d} built on the host in {time.perf_counter() - t0:.2f} s (once, at construction); "
                  f"Mmax {libs[-1][1].patterns.max_markers}", flush=True)
    press()
    print(f"  static grid (tacex_fem_marker_flow):   {time_calls(static, out)}", flush=True)
    for p, ms in libs:
        ms.marker_lose_tracking_probability, ms.marker_random_noise = 0.0, 0.0
        print(f"  library of {p:3d}, loss and noise off:    {time_calls(ms, out)}", flush=True)
        ms.marker_lose_tracking_probability, ms.marker_random_noise = 0.01, 0.5
        print(f"  library of {p:3d}, p = 0.01, sigma = 0.5: {time_calls(ms, out)}; tracked per env {ms.num_tracked.float().mean().item():.1f}", flush=True)
    if libs:
        print(f"  static grid again:                     {time_calls(static, out)}", flush=True)


if __name__ == "__main__":
    main()
