"""TEST INFRASTRUCTURE ONLY (never imported by the product): NumPy restatement of `fem_traction_image_kernel`
(tacex_amd/csrc/depth_raster.hip, `tacex_traction_image_from_deformed_mesh`).  It is `oracle/mesh_depth_oracle.render_depth`'s loop -
same float32 operations in the same order, so the same fragments and depths - extended with the winner rule (triangles in ascending
index, a fragment replaces the pixel's only when its z is strictly smaller: the smallest (z, t) wins) and the perspective-correct
interpolation of a per-vertex quantity at the winner, every float32 operation rounded on its own."""
from __future__ import annotations

import numpy as np

F = np.float32


def camera_frame_f32(xw, pos, rot_inv):
    """(N,3) float64 world points -> (N,3) float32 camera-frame points: float64 arithmetic in the kernel's order, rounded once."""
    d = np.asarray(xw, np.float64) - np.asarray(pos, np.float64)
    R = np.asarray(rot_inv, np.float64)
    return np.stack([(R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2] for i in range(3)], 1).astype(F)


def vertex_tractions(force, area, rot_inv):
    """(N,3) float64 forces [N, world] and (N,) areas [m^2] of the rendered vertices -> (N,3) float32 tractions [Pa, camera frame]:
    a float64 division per component, the rotation in float64, rounded once; zero where the area is not positive."""
    f, a, R = np.asarray(force, np.float64), np.asarray(area, np.float64), np.asarray(rot_inv, np.float64)
    ok = a > 0.0
    tw = np.zeros_like(f)
    tw[ok] = f[ok] / a[ok, None]
    tc = np.stack([(R[i, 0] * tw[:, 0] + R[i, 1] * tw[:, 1]) + R[i, 2] * tw[:, 2] for i in range(3)], 1).astype(F)
    tc[~ok] = 0
    return tc


def project(pc, fx, fy, cx, cy):
    """float32 camera-frame points -> (sx, sy, iz, front), `project_deformed`'s operations."""
    pc = np.asarray(pc, F)
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    with np.errstate(divide="ignore", invalid="ignore"):
        iz = (F(1.0) / pc[:, 2]).astype(F)
        sx = ((fx * pc[:, 0]) * iz + cx).astype(F)
        sy = ((fy * pc[:, 1]) * iz + cy).astype(F)
    return sx, sy, iz, pc[:, 2] > F(1e-6)


def _weights(sx, sy, iz, tri, i, j, dtype):
    """l_k, z of the pixels (i, j) in their triangles `tri` (n,3), the walk's expressions in `dtype`."""
    T = dtype
    x, y, q = (sx[tri].astype(T), sy[tri].astype(T), iz[tri].astype(T))
    px, py = (j.astype(T) + T(0.5)), (i.astype(T) + T(0.5))
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    inv_area = T(1.0) / area
    e0 = (x[:, 2] - x[:, 1]) * (py - y[:, 1]) - (y[:, 2] - y[:, 1]) * (px - x[:, 1])
    e1 = (x[:, 0] - x[:, 2]) * (py - y[:, 2]) - (y[:, 0] - y[:, 2]) * (px - x[:, 2])
    e2 = (x[:, 1] - x[:, 0]) * (py - y[:, 0]) - (y[:, 1] - y[:, 0]) * (px - x[:, 0])
    l = [e0 * inv_area, e1 * inv_area, e2 * inv_area]
    z = T(1.0) / ((l[0] * q[:, 0] + l[1] * q[:, 1]) + l[2] * q[:, 2])
    return l, q, z


def interpolate(sx, sy, iz, tris, winner, tau, dtype=F):
    """(H,W,3) `dtype`: the per-vertex quantity `tau` (N,3) at every pixel with a winner, w_k = (l_k * iz[k]) * z,
    t[i] = (w0 tau0[i] + w1 tau1[i]) + w2 tau2[i]; 0 elsewhere.  dtype=np.float64: the same interpolant of the same float32 projections
    without the rounding of the float32 operations (property tests)."""
    out = np.zeros(winner.shape + (3,), dtype)
    i, j = np.nonzero(winner >= 0)
    if len(i) == 0:
        return out
    tri = np.asarray(tris, np.int64)[winner[i, j]]
    l, q, z = _weights(sx, sy, iz, tri, i, j, dtype)
    w = [(l[k] * q[:, k]) * z for k in range(3)]
    tv = np.asarray(tau).astype(dtype)[tri]  # (n,3 vertices,3 components)
    out[i, j] = (w[0][:, None] * tv[:, 0] + w[1][:, None] * tv[:, 1]) + w[2][:, None] * tv[:, 2]
    return out


def render(pc, tris, tau, fx, fy, cx, cy, near, far, H, W, dtype=F):
    """One env: float32 camera-frame vertices `pc` (N,3), triangles (T,3), per-vertex float32 quantity `tau` (N,3) ->
    depth (H,W) float32 (inf: no fragment), winner (H,W) int64 triangle index (-1: none), image (H,W,3) `dtype`."""
    tris = np.asarray(tris, np.int64)
    sx, sy, iz, front = project(pc, fx, fy, cx, cy)
    near, far, half = F(near), F(far), F(0.5)
    depth = np.full((H, W), np.inf, dtype=F)
    winner = np.full((H, W), -1, dtype=np.int64)
    for t, tri in enumerate(tris):  # ascending t, strict <: the smallest (z, t)
        if not front[tri].all():
            continue
        x, y, z = sx[tri], sy[tri], iz[tri]
        j0 = max(0, int(np.ceil(x.min() - half))); j1 = min(W - 1, int(np.floor(x.max() - half)))
        i0 = max(0, int(np.ceil(y.min() - half))); i1 = min(H - 1, int(np.floor(y.max() - half)))
        if j0 > j1 or i0 > i1:
            continue
        area = F((x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]))
        if area == 0:
            continue
        inv_area = F(1.0) / area
        qy = (np.arange(i0, i1 + 1, dtype=F) + half)[:, None]
        qx = (np.arange(j0, j1 + 1, dtype=F) + half)[None, :]
        e0 = ((x[2] - x[1]) * (qy - y[1]) - (y[2] - y[1]) * (qx - x[1])).astype(F)
        e1 = ((x[0] - x[2]) * (qy - y[2]) - (y[0] - y[2]) * (qx - x[2])).astype(F)
        e2 = ((x[1] - x[0]) * (qy - y[0]) - (y[1] - y[0]) * (qx - x[0])).astype(F)
        inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) if area > 0 else ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        if not inside.any():
            continue
        l0, l1, l2 = (e0 * inv_area).astype(F), (e1 * inv_area).astype(F), (e2 * inv_area).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            zz = (F(1.0) / ((l0 * z[0] + l1 * z[1]) + l2 * z[2]).astype(F)).astype(F)
        ok = inside & (zz >= near) & (zz <= far)
        blk, wblk = depth[i0:i1 + 1, j0:j1 + 1], winner[i0:i1 + 1, j0:j1 + 1]
        better = ok & (zz < blk)
        blk[better] = zz[better]
        wblk[better] = t
    return depth, winner, interpolate(sx, sy, iz, tris, winner, tau, dtype)


def render_envs(x, surf_ids, tris, forces, areas, pos, rot_inv, intr, clip, H, W):
    """The C entry point's arguments as NumPy arrays -> depth (B,H,W), winner (B,H,W), traction (B,H,W,3) float32."""
    ids = np.asarray(surf_ids, np.int64)
    out = []
    for b in range(len(x)):
        pc = camera_frame_f32(x[b][ids], pos[b], rot_inv[b])
        tau = vertex_tractions(forces[b][ids], np.asarray(areas)[ids], rot_inv[b])
        out.append(render(pc, tris, tau, *intr, clip[0], clip[1], H, W))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def tilt_and_dent(P):
    """The test state of the pad: the rest mesh tilted about y (z += 0.02 (x - 10 mm)) with a 0.4 mm Gaussian dent (sigma 3 mm) towards
    the camera at the face's centre.  (V,3) float64."""
    x = np.array(P, dtype=np.float64)
    x[:, 2] += 0.02 * (x[:, 0] - 0.01)
    r2 = (x[:, 0] - 0.010375) ** 2 + (x[:, 1] - 0.012625) ** 2
    x[:, 2] -= 0.0004 * np.exp(-r2 / (2.0 * 0.003 ** 2))
    return x
