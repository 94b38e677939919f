"""Timing of the affine-body depth source (AffineBodyDepthSource, `tacex_depth_from_affine_body`) against the route that renders the same
image without it: `UipcSim.body_points()` (a torch einsum that writes the (B, nv, 3) float64 world points) followed by
`tacex_depth_from_deformed_mesh` on the result.  FemBallScene with 512 envs, its level-2 ball (162 vertices / 320 triangles) and a level-3
ball (642 / 1280), at 320x240 and 640x480, the ball pressed into view in every env and the camera following the case.  Both routes are
timed in the same run, alternated round by round, with device events after warm-up; per route the median over the rounds and the spread
(max - min over the rounds) are reported, and the images are compared (equal up to the rounding order of the einsum's world points: the
count of differing pixels is printed, not asserted).  One JSON line per configuration."""
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from tacex_amd import AffineBodyDepthSource, _lib
from tacex_amd.uipc.gelpad_scene import FemBallScene

INTR = {(320, 240): (340.0, 325.0, 160.0, 125.0), (640, 480): (680.0, 650.0, 320.0, 250.0)}
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B = int(sys.argv[3]) if len(sys.argv) > 3 else 512
STEPS = 9  # c = 0.5 - 0.5 cos(0.3 * 8) = 0.87 of the press


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


for level in (2, 3):
    scene = FemBallScene(B, "cuda:0", level=level)
    scene.depth = torch.linspace(0.0004, 0.0008, B, device="cuda:0", dtype=torch.float64)  # every env brings the ball inside the far plane
    for i in range(STEPS):
        scene.step(i)
    torch.cuda.synchronize()
    sim = scene.sim
    pos, quat = scene.camera_pose()
    for res in ((320, 240), (640, 480)):
        W, H = res
        src = AffineBodyDepthSource(scene.ball, pos, quat, resolution=res, intrinsics=INTR[res])
        src.pos[:, 2] -= (0.5 - 0.5 * math.cos(0.3 * (STEPS - 1))) * scene.depth
        lib = src._lib
        ids = torch.arange(src.rest_verts.shape[0], dtype=torch.int32, device="cuda:0")
        depth2 = torch.empty_like(src.depth)
        nv, nt = int(src.rest_verts.shape[0]), int(src.tris.shape[0])

        def via_points():
            x = sim.body_points().contiguous()  # (the einsum may hand back a permuted view; the rasteriser reads (B, nv, 3) rows)
            rc = lib.tacex_depth_from_deformed_mesh(_lib.ptr(x), nv, _lib.ptr(ids), nv, _lib.ptr(src.tris), nt, _lib.ptr(src.pos),
                                                    _lib.ptr(src.rot_inv), src.fx, src.fy, src.cx, src.cy, src.near, src.far, _lib.ptr(depth2), B,
                                                    H, W, _lib.current_stream_handle(depth2.device))
            _lib.check(rc, "tacex_depth_from_deformed_mesh")

        for _ in range(5):
            src()
            via_points()
        t_new, t_old = [], []
        for r in range(ROUNDS):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (t_new if which == 0 else t_old).append(timed(src if which == 0 else via_points, REPS))
        torch.cuda.synchronize()
        seen = torch.isfinite(src.depth)
        differ = int(((src.depth != depth2) & (seen | torch.isfinite(depth2))).sum())
        stride = tuple(sim.body_points().stride())
        print(json.dumps({"envs": B, "res": f"{W}x{H}", "level": level, "verts": nv, "triangles": nt, "rounds": ROUNDS, "reps": REPS,
                          "affine_body_ms": round(statistics.median(t_new), 4), "affine_body_spread_ms": round(max(t_new) - min(t_new), 4),
                          "body_points_plus_deformed_mesh_ms": round(statistics.median(t_old), 4),
                          "body_points_plus_deformed_mesh_spread_ms": round(max(t_old) - min(t_old), 4),
                          "envs_seeing_the_ball": int(seen.flatten(1).any(1).sum()), "hit_fraction": round(seen.float().mean().item(), 4),
                          "pixels_differing_between_routes": differ,
                          "body_points_stride": stride}), flush=True)
    del scene, sim
    torch.cuda.synchronize()
