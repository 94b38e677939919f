"""NumPy restatement of `tacex_depth_from_affine_body` (csrc/depth_raster.hip, AffineBodyVerts): world points of the affine body from its
state q = (p, c1, c2, c3) in the kernel's operation order, the float64 camera frame rounded once to float32 (what
tests/test_fem_surface_depth.py::_camera_frame_f32 does for the pad), then oracle/mesh_depth_oracle.py at the identity pose.  Also the
six states / cameras the GPU tests render (`cases`)."""
import numpy as np

from oracle.mesh_depth_oracle import pose_rows, render_depth

# the small frame of the tests: 0.3 x the sensor's 320 x 240 and its intrinsics - a partial tile in both axes (64 + 32 columns, 2 x 32 + 8 rows)
RES = (96, 72)
INTR = (102.0, 97.5, 48.0, 37.5)
CLIP = (0.024, 0.029)
RADIUS = 0.009
TOP = np.array([0.0008, 0.0005, 0.028])  # the ball's nearest point in front of a camera at the origin that looks along +z


def world_points(X, q):
    """(B,nv,3) float64: per component w = ((p + X0 c1) + X1 c2) + X2 c3, separate multiplies and adds."""
    X = np.asarray(X, np.float64)
    q = np.asarray(q, np.float64)
    X0, X1, X2 = (X[None, :, k, None] for k in range(3))
    return ((q[:, None, 0] + X0 * q[:, None, 1]) + X1 * q[:, None, 2]) + X2 * q[:, None, 3]


def camera_frame_f32(w, pos, rot_inv):
    """(B,nv,3) float32 camera-frame points: float64 arithmetic in the kernel's order, rounded once."""
    out = []
    for b in range(w.shape[0]):
        d = w[b] - pos[b]
        R = rot_inv[b]
        out.append(np.stack([(R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2] for i in range(3)], 1).astype(np.float32))
    return np.stack(out)


def render(X, tris, q, pos, rot_inv, res=RES, intr=INTR, clip=CLIP):
    """(B,H,W) float32 depth [m] of the body in state q (B,4,3) through the cameras pos (B,3) / rot_inv (B,3,3), inf where nothing is seen."""
    W, H = res
    pc = camera_frame_f32(world_points(X, q), np.asarray(pos, np.float64), np.asarray(rot_inv, np.float64))
    ident = pose_rows(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0, 0.0]]))
    return np.stack([render_depth(pc[b], tris, ident, *intr, clip[0], clip[1], H, W)[0] for b in range(len(pc))])


def dropped_triangles(X, tris, q, pos, rot_inv):
    """(B,) triangles with a vertex at or behind the camera plane (pz <= 1e-6): dropped whole."""
    pc = camera_frame_f32(world_points(X, q), np.asarray(pos, np.float64), np.asarray(rot_inv, np.float64))
    return (~(pc[:, :, 2] > np.float32(1e-6))[:, np.asarray(tris)].all(-1)).sum(1)


def skipped_tiles(X, q, pos, rot_inv, res=RES, intr=INTR, clip=CLIP, tile=(64, 32)):
    """(B, tiles_y, tiles_x) bool: the tiles the kernel does not stage (AffineBodyVerts::Env::out_of_tile): the body lies in the sphere of
    radius |A|_2 max|X| about R (p - cam_pos), |A|_2^2 bounded by the largest absolute row sum of A^T A; a fragment lies in the slab of that sphere
    between the clipping planes, whose screen bounds are tested against the tile, in float32."""
    F = np.float32
    W, H = res
    fx, fy, cx, cy = (F(v) for v in intr)
    near, far = F(clip[0]), F(clip[1])
    Xf = np.asarray(X, np.float64).astype(F)
    r2 = ((Xf[:, 0] * Xf[:, 0] + Xf[:, 1] * Xf[:, 1]) + Xf[:, 2] * Xf[:, 2]).max()
    ty, tx = (H + tile[1] - 1) // tile[1], (W + tile[0] - 1) // tile[0]
    out = np.zeros((len(q), ty, tx), bool)
    for b in range(len(q)):
        c = np.asarray(q[b, 1:], np.float64).astype(F)  # rows: the columns of A
        g = np.abs(np.array([[(c[j, 0] * c[k, 0] + c[j, 1] * c[k, 1]) + c[j, 2] * c[k, 2] for k in range(3)] for j in range(3)], F))
        a2 = max((g[j, 0] + g[j, 1]) + g[j, 2] for j in range(3))
        d = np.asarray(q[b, 0], np.float64) - pos[b]
        R = np.asarray(rot_inv[b], np.float64)
        bx, by, bz = (((R[i, 0] * d[0] + R[i, 1] * d[1]) + R[i, 2] * d[2]).astype(F) for i in range(3))
        m = F(1.001)
        r = F(F(np.sqrt(r2)) * F(np.sqrt(a2))) * m
        if bz + r < near or bz - r > far:
            out[b] = True
            continue
        zlo, zhi = max(bz - r, near), min(bz + r, far)  # the slab of the sphere a fragment can lie in
        if not zlo > F(1e-4):
            continue
        dist = bz - zhi if bz > zhi else (zlo - bz if bz < zlo else F(0))
        rho = F(np.sqrt(max(r * r - dist * dist, F(0)))) * m
        ulo = min(fx * (bx - rho) / zlo, fx * (bx - rho) / zhi) + cx - F(1)
        uhi = max(fx * (bx + rho) / zlo, fx * (bx + rho) / zhi) + cx + F(1)
        vlo = min(fy * (by - rho) / zlo, fy * (by - rho) / zhi) + cy - F(1)
        vhi = max(fy * (by + rho) / zlo, fy * (by + rho) / zhi) + cy + F(1)
        for i in range(ty):
            for j in range(tx):
                x0, y0 = j * tile[0], i * tile[1]
                x1, y1 = min(x0 + tile[0], W), min(y0 + tile[1], H)
                out[b, i, j] = uhi < x0 or ulo > x1 or vhi < y0 or vlo > y1
    return out


def state(p, A=np.eye(3)):
    """(4,3) q of a body at p with deformation gradient A: rows p, then the COLUMNS of A."""
    return np.concatenate([np.asarray(p, np.float64)[None], np.asarray(A, np.float64).T], 0)


def cases():
    """q (6,4,3), camera pos (6,3), rot_inv (6,3,3) of the six envs of the GPU tests:
    0 identity A on the axis; 1 a sheared, stretched A; 2 16 mm off axis, partly in view; 3 wholly beyond the far plane; 4 the camera
    inside a body stretched 3 x along the axis (vertices behind the camera plane); 5 case 0 through a camera shifted 0.5 mm and tilted 4 degrees
    about y."""
    c = TOP + [0.0, 0.0, RADIUS]
    shear = np.array([[1.05, 0.03, 0.0], [0.0, 0.97, 0.02], [0.01, 0.0, 0.98]])
    q = np.stack([state(c), state(c, shear), state([0.016, 0.0, c[2]]), state(c + [0.0, 0.0, 0.002]),
                  state([0.0, 0.0, 0.020], np.diag([1.0, 1.0, 3.0])), state(c)])
    pos = np.zeros((6, 3))
    rot_inv = np.tile(np.eye(3), (6, 1, 1))
    pos[5] = [0.0005, 0.0, 0.0]
    a = np.radians(4.0)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])  # camera -> world
    rot_inv[5] = R.T
    return q, pos, rot_inv
