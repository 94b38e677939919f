"""Timing of the FEM surface depth source (FemSurfaceDepthSource): the C4 pad (495 vertices, 160 contact-face triangles) after a few
FemGelpad steps, 512 and 1024 envs at 320x240 and 640x480; hipEvents around the render alone and around render + height-map pass
(`fill`).  One JSON line per configuration.  The floor is the depth written: B * H * W * 4 bytes (render), plus the height map the
pass writes and the depth it reads again."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from tacex_amd import FemSurfaceDepthSource
from tacex_amd.uipc.gelpad_scene import FemGelpad

CAM = (0.010375, 0.012625, -0.024)  # pad centre, 24 mm behind the back face
INTR = {(320, 240): (340.0, 325.0, 160.0, 125.0), (640, 480): (680.0, 650.0, 320.0, 250.0)}
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def timed(fn, reps):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


for B in (512, 1024):
    fem = FemGelpad(B, "cuda:0", motion="breathing")
    for i in range(8):  # pressed, deformed pads (i = 7: about three quarters of the press)
        fem.step(i)
    torch.cuda.synchronize()
    for res in ((320, 240), (640, 480)):
        W, H = res
        src = FemSurfaceDepthSource(fem.gelpad, CAM, (1.0, 0.0, 0.0, 0.0), resolution=res, intrinsics=INTR[res])
        hm = torch.empty((B, H, W), device="cuda:0")
        fmin = torch.empty((B,), device="cuda:0")
        ind = torch.empty((B,), device="cuda:0")
        ms_render = timed(src, REPS)
        ms_fill = timed(lambda: src.fill(hm, fmin, ind, 0.0045, 0.024), REPS)
        hit = torch.isfinite(src.depth).float().mean().item()
        depth_bytes = B * H * W * 4
        print(json.dumps({"envs": B, "res": f"{W}x{H}", "triangles": int(src.tris.shape[0]), "render_ms": round(ms_render, 4),
                          "render_plus_height_map_ms": round(ms_fill, 4), "render_GBps_written": round(depth_bytes / ms_render / 1e6, 1),
                          "hit_fraction": round(hit, 4), "indent_mm_max": round(float(ind.max()), 4)}), flush=True)
    del fem
    torch.cuda.synchronize()
