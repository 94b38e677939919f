"""Mesh-library timing: the C4 pad at 512 envs with K = 1, 4 and 8 indenter meshes of mixed size (one per env, ids = env % K), against a
single mesh of the K meshes' average triangle count.  Per setting: ms per FEM step (FemGelpad's breathing scene, indenter kind 4) and ms
per 1024 depth frames at 320x240 (MeshLibraryDepthSource; MeshDepthSource for the single mesh as well)."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from tacex_amd import MeshDepthSource, MeshLibraryDepthSource
from tacex_amd.uipc.gelpad_scene import FemGelpad
from tacex_amd.uipc.indenter_meshes import icosphere


def uv_sphere(radius, n_lat, n_lon):
    """(vertices, triangles) of a latitude / longitude sphere: 2 n_lon (n_lat - 1) triangles, vertices on the sphere."""
    v = [[0.0, 0.0, radius], [0.0, 0.0, -radius]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    ring = lambda i, j: 2 + (i - 1) * n_lon + j % n_lon  # noqa: E731
    t = []
    for j in range(n_lon):
        t.append([0, ring(1, j), ring(1, j + 1)])
        t.append([1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            t += [[a, c, b], [b, c, d]]
    return np.asarray(v), np.asarray(t, np.int32)


def sphere_with(radius, ntri):
    """a UV sphere of about `ntri` triangles"""
    n = max(3, int(round(np.sqrt(ntri / 4.0))))
    return uv_sphere(radius, n + 1, 2 * n)


def library(radius, k):
    """k sphere-like meshes of mixed size: icospheres of 0-3 subdivisions (20 - 1280 triangles), then UV spheres"""
    meshes = [icosphere(radius, s) for s in (0, 1, 2, 3)]
    meshes += [uv_sphere(radius, 6, 12), uv_sphere(radius, 10, 20), uv_sphere(radius, 16, 32), uv_sphere(radius, 24, 48)]
    return [meshes[2]] if k == 1 else meshes[:k]


def fem_ms(B, meshes, ids, steps):
    fem = FemGelpad(B, "cuda:0")
    fem.sim.set_indenter_meshes(meshes, ids)
    fem.ind[:, 0] = 4.0
    fem.ind[:, 4] = 0.0
    for i in range(6):
        fem.step(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(6, 6 + steps):
        fem.step(i)
        ms.append(fem.fem_ms_last())
    info = fem.sim.check_step(raise_on_penetration=False)
    return float(np.mean(ms)), float(np.median(ms)), len(info["penetrating_envs"]), len(info["bad_mesh_id_envs"])


def place(src, B):
    g = torch.Generator(device="cuda").manual_seed(0)
    src.pos[:, 0] = (torch.rand(B, device="cuda", generator=g) - 0.5) * 0.008
    src.pos[:, 1] = (torch.rand(B, device="cuda", generator=g) - 0.5) * 0.006
    src.pos[:, 2] = 0.029 + torch.rand(B, device="cuda", generator=g) * 0.003


def depth_ms(src, reps):
    for _ in range(3):
        src()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        src()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", default="1,4,8")
    ap.add_argument("--per-mesh", action="store_true", help="also time every mesh of the library alone")
    a = ap.parse_args()
    B, F = a.envs, a.frames
    for k in (int(s) for s in a.k.split(",")):
        # FEM: meshes of the scene's sphere radius (FemGelpad.R, 4 mm)
        r_fem = 0.004
        meshes = library(r_fem, k)
        counts = [len(t) for _, t in meshes]
        avg = float(np.mean([counts[e % k] for e in range(B)]))
        ids = np.arange(B) % k
        mixed = fem_ms(B, meshes, ids, a.steps)
        one = sphere_with(r_fem, avg) if k > 1 else meshes[0]
        single = fem_ms(B, [one], None, a.steps)
        # depth: 320 x 240, radius 4 mm
        dm = library(0.004, k)
        lib = MeshLibraryDepthSource(dm, F, "cuda:0", resolution=(320, 240))
        place(lib, F)
        lib.mesh_ids.copy_(torch.arange(F, device="cuda", dtype=torch.int32) % k)
        ov, ot = sphere_with(0.004, avg) if k > 1 else dm[0]
        lib1 = MeshLibraryDepthSource([(ov, ot)], F, "cuda:0", resolution=(320, 240))
        place(lib1, F)
        src1 = MeshDepthSource(ov, ot, F, "cuda:0", resolution=(320, 240))
        place(src1, F)
        d_mixed, d_one, d_old = depth_ms(lib, a.reps), depth_ms(lib1, a.reps), depth_ms(src1, a.reps)
        print(f"K={k}: triangles {counts} (mean over envs {avg:.0f}; single mesh {len(one[1])} / {len(ot)})")
        print(f"  FEM step, {B} envs: mixed {mixed[0]:.3f} ms (median {mixed[1]:.3f}), single {single[0]:.3f} ms (median {single[1]:.3f}), "
              f"ratio {mixed[0] / single[0]:.3f}; flagged envs: penetration {mixed[2]} / {single[2]}, bad id {mixed[3]}")
        print(f"  depth, {F} frames 320x240: mixed library {d_mixed:.3f} ms, single-mesh library {d_one:.3f} ms, MeshDepthSource {d_old:.3f} ms, "
              f"ratio {d_mixed / d_one:.3f}")
        if k > 1 and a.per_mesh:
            # every mesh of the library alone (ids all the same): what the mixed batch would cost if only the mean of these counted (depth:
            # the workgroups of all envs share the GPU) or only the slowest (FEM: one env per workgroup on its CU for the whole launch)
            f1 = [fem_ms(B, [m], None, a.steps)[0] for m in meshes]
            d1 = []
            for v, t in dm:
                s1 = MeshDepthSource(v, t, F, "cuda:0", resolution=(320, 240))
                place(s1, F)
                d1.append(depth_ms(s1, a.reps))
            print(f"  each mesh alone: FEM {['%.3f' % x for x in f1]} ms (mean {np.mean(f1):.3f}, max {np.max(f1):.3f}); "
                  f"depth {['%.3f' % x for x in d1]} ms (mean {np.mean(d1):.3f})")
        del lib, lib1, src1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
