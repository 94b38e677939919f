"""Timing of the traction image (FemTractionImage, `tacex_traction_image_from_deformed_mesh`): the C4 pad (495 vertices, 160 contact-face
triangles) after 8 FemGelpad steps, 512 and 1024 envs at 320x240 and 512 envs at 640x480.  hipEvents, median of 5 rounds of 200 calls:
 (a) the traction launch alone, the per-vertex forces computed beforehand;
 (b) `contact_forces(per_vertex=True)` + the launch (`FemTractionImage.__call__`);
 (c) `tacex_depth_from_deformed_mesh` on the same state (FemSurfaceDepthSource) - the kernel (a) extends; (a) writes 12 bytes per pixel
     more than it.
Writes the table to profiles/traction_image_bench.md (or the path given as the first argument)."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from tacex_amd import FemSurfaceDepthSource, FemTractionImage
from tacex_amd.uipc.gelpad_scene import FemGelpad

CAM = (0.010375, 0.012625, -0.024)  # pad centre, 24 mm behind the back face
INTR = {(320, 240): (340.0, 325.0, 160.0, 125.0), (640, 480): (680.0, 650.0, 320.0, 250.0)}
OUT = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "traction_image_bench.md"
ROUNDS, CALLS = 5, 200


def timed(fn):
    for _ in range(10):
        fn()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    return statistics.median(ms)


rows = []
for B, res in ((512, (320, 240)), (1024, (320, 240)), (512, (640, 480))):
    fem = FemGelpad(B, "cuda:0", motion="breathing")
    for i in range(8):  # pressed, deformed pads (i = 7: about three quarters of the press)
        fem.step(i)
    torch.cuda.synchronize()
    W, H = res
    img = FemTractionImage(fem.gelpad, CAM, (1.0, 0.0, 0.0, 0.0), resolution=res, intrinsics=INTR[res])
    dep = FemSurfaceDepthSource(fem.gelpad, CAM, (1.0, 0.0, 0.0, 0.0), resolution=res, intrinsics=INTR[res])
    vf = fem.contact_forces(per_vertex=True).vertex_forces
    a = timed(lambda: img.render(vf))
    a_depth = timed(lambda: img.render(vf, with_depth=True))
    b = timed(img)
    c = timed(dep)
    hit = float((img.traction[..., 2] != 0).float().mean())
    px = B * H * W
    row = dict(envs=B, res=f"{W}x{H}", a=a, a_depth=a_depth, b=b, c=c, ratio=a / c, gbps_a=12 * px / a / 1e6, gbps_c=4 * px / c / 1e6, hit=hit)
    print(row, flush=True)
    rows.append(row)
    del fem, img, dep
    torch.cuda.synchronize()

lines = ["# Traction image against the depth render it extends", "",
         "`scripts/traction_image_bench.py`: C4 pad (495 vertices, 160 contact-face triangles), the state after 8 `FemGelpad` steps, hipEvents,",
         f"median of {ROUNDS} rounds of {CALLS} calls, milliseconds per call.  (a) `tacex_traction_image_from_deformed_mesh` alone with the",
         "per-vertex forces computed beforehand (a+: with the depth output), (b) `contact_forces(per_vertex=True)` + the launch,",
         "(c) `tacex_depth_from_deformed_mesh` on the same state.  GB/s: bytes of the image written per second (12 and 4 bytes per pixel).", "",
         "| envs | image | (a) traction | (a+) with depth | (b) forces + traction | (c) depth | (a)/(c) | (a) GB/s | (c) GB/s | pixels in contact |",
         "|---|---|---|---|---|---|---|---|---|---|"]
for r in rows:
    lines.append(f"| {r['envs']} | {r['res']} | {r['a']:.4f} | {r['a_depth']:.4f} | {r['b']:.4f} | {r['c']:.4f} | {r['ratio']:.2f} | {r['gbps_a']:.0f} | "
                 f"{r['gbps_c']:.0f} | {100 * r['hit']:.1f} % |")
lo, hi = min(r["ratio"] for r in rows), max(r["ratio"] for r in rows)
lines += ["",
          f"Reading: (a)/(c) is {lo:.2f}-{hi:.2f}.  Neither kernel is bound by the bytes it writes (the chip stores about 6 TB/s); both are bound",
          "by the work of a workgroup on its tile.  Beyond the depth kernel's, the traction kernel does per pixel: the (z, triangle) key instead",
          "of a minimum in the list walk; for the winner three index loads, six LDS reads (projections and tractions of its vertices), the edge",
          "functions and two IEEE divisions again, 18 multiply-adds; three 4-byte stores 12 bytes apart per lane instead of one store of 64",
          "consecutive floats per wave; and per workgroup the vertex tractions (three float64 divisions and a 3x3 float64 product per vertex).",
          "It holds 106 VGPRs against 68, so 4 waves per SIMD against 7.  How the extra time splits between these was not measured."]
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text("\n".join(lines) + "\n")
print(f"wrote {OUT}")
