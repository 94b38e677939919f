"""Signed-distance grids for `SdfVolumeSource` (NumPy, float64 cast once to float32, no random numbers): objects a GelSight is pressed
on at an arbitrary pose.  Distances are in object mm, negative inside; the object frame's origin is the grid centre unless a
generator says otherwise; every generator returns an `SdfVolume`.  `sphere`, `box`, `torus` and `capsule` are exact distances;
`hex_nut` is an intersection of exact distances (a lower bound with the right zero level); `gear` is a field with the right zero
level that is no distance: it comes with the `step_scale` < 1 that makes the march conservative (one over a bound of its gradient)."""
from __future__ import annotations

import math

import numpy as np

from ..volume_source import SdfVolume


def grid_points(shape, pitch_mm: float):
    """(x, y, z) float64 coordinates [mm, origin at the grid centre] of a (D, Hv, Wv) grid, each broadcastable to that shape."""
    D, Hv, Wv = (int(n) for n in shape)
    z = (np.arange(D, dtype=np.float64) - (D - 1) / 2.0) * pitch_mm
    y = (np.arange(Hv, dtype=np.float64) - (Hv - 1) / 2.0) * pitch_mm
    x = (np.arange(Wv, dtype=np.float64) - (Wv - 1) / 2.0) * pitch_mm
    return x[None, None, :], y[None, :, None], z[:, None, None]


def _shape_for(half_extents_mm, pitch_mm: float, pad_voxels: int):
    """(D, Hv, Wv) that holds half extents (x, y, z) with `pad_voxels` around them."""
    n = [2 * (int(math.ceil(h / pitch_mm)) + int(pad_voxels)) + 1 for h in half_extents_mm]
    return (n[2], n[1], n[0])


def from_function(fn, shape, pitch_mm: float, step_scale: float = 1.0) -> SdfVolume:
    """`fn(x, y, z)` -> signed distance [mm] on broadcastable float64 coordinate arrays (origin at the grid centre), sampled on a
    (D, Hv, Wv) grid."""
    x, y, z = grid_points(shape, pitch_mm)
    s = np.broadcast_to(np.asarray(fn(x, y, z), dtype=np.float64), tuple(int(n) for n in shape))
    return SdfVolume(s.astype(np.float32), pitch_mm, None, step_scale)


def sphere_distance(x, y, z, radius_mm):
    return np.sqrt(x * x + y * y + z * z) - radius_mm


def box_distance(x, y, z, size_mm):
    """Exact signed distance of an axis-aligned box of full extents (sx, sy, sz)."""
    qx, qy, qz = np.abs(x) - size_mm[0] / 2.0, np.abs(y) - size_mm[1] / 2.0, np.abs(z) - size_mm[2] / 2.0
    outside = np.sqrt(np.maximum(qx, 0) ** 2 + np.maximum(qy, 0) ** 2 + np.maximum(qz, 0) ** 2)
    return outside + np.minimum(np.maximum(qx, np.maximum(qy, qz)), 0)


def torus_distance(x, y, z, major_mm, minor_mm):
    """A torus around the z axis."""
    return np.sqrt((np.sqrt(x * x + y * y) - major_mm) ** 2 + z * z) - minor_mm


def capsule_distance(x, y, z, radius_mm, length_mm):
    """A capsule along x: a segment of `length_mm` swept by a sphere."""
    return np.sqrt((x - np.clip(x, -length_mm / 2.0, length_mm / 2.0)) ** 2 + y * y + z * z) - radius_mm


def sphere(radius_mm: float = 3.0, pitch_mm: float = 0.1, pad_voxels: int = 3) -> SdfVolume:
    return from_function(lambda x, y, z: sphere_distance(x, y, z, radius_mm), _shape_for([radius_mm] * 3, pitch_mm, pad_voxels), pitch_mm)


def box(size_mm=(5.0, 3.0, 2.0), pitch_mm: float = 0.1, pad_voxels: int = 3) -> SdfVolume:
    return from_function(lambda x, y, z: box_distance(x, y, z, size_mm), _shape_for([s / 2.0 for s in size_mm], pitch_mm, pad_voxels), pitch_mm)


def torus(major_mm: float = 2.5, minor_mm: float = 0.8, pitch_mm: float = 0.1, pad_voxels: int = 3) -> SdfVolume:
    r = major_mm + minor_mm
    return from_function(lambda x, y, z: torus_distance(x, y, z, major_mm, minor_mm), _shape_for([r, r, minor_mm], pitch_mm, pad_voxels), pitch_mm)


def capsule(radius_mm: float = 1.0, length_mm: float = 4.0, pitch_mm: float = 0.1, pad_voxels: int = 3) -> SdfVolume:
    half = [length_mm / 2.0 + radius_mm, radius_mm, radius_mm]
    return from_function(lambda x, y, z: capsule_distance(x, y, z, radius_mm, length_mm), _shape_for(half, pitch_mm, pad_voxels), pitch_mm)


def _prism(d2, z, height_mm):
    """A 2-D signed distance extruded to |z| <= height / 2 (exact when d2 is)."""
    dz = np.abs(z) - height_mm / 2.0
    return np.minimum(np.maximum(d2, dz), 0) + np.sqrt(np.maximum(d2, 0) ** 2 + np.maximum(dz, 0) ** 2)


def hex_nut(across_flats_mm: float = 5.0, bore_mm: float = 3.0, height_mm: float = 2.4, pitch_mm: float = 0.1, pad_voxels: int = 3) -> SdfVolume:
    """A hexagonal prism around z with a bore of diameter `bore_mm`.  Prism and bore are exact distances; their intersection has
    the right zero level and never exceeds the distance, so the march stays conservative with step_scale = 1."""
    a = across_flats_mm / 2.0
    rb = bore_mm / 2.0
    if not 0 < rb < a:
        raise ValueError(f"hex_nut: a bore of {bore_mm} does not fit across flats of {across_flats_mm}")

    def fn(x, y, z):
        # exact hexagon: fold into one sector, distance to the flat, clamped along it
        k = np.array([-math.sqrt(3) / 2.0, 0.5, 1.0 / math.sqrt(3)])
        px, py = np.abs(x) + 0 * y, np.abs(y) + 0 * x
        t = 2.0 * np.minimum(k[0] * px + k[1] * py, 0.0)
        px, py = px - t * k[0], py - t * k[1]
        px = px - np.clip(px, -k[2] * a, k[2] * a)
        py = py - a
        hexd = np.sqrt(px * px + py * py) * np.sign(py)
        return np.maximum(_prism(hexd, z, height_mm), rb - np.sqrt(x * x + y * y))

    r = a * 2.0 / math.sqrt(3)
    return from_function(fn, _shape_for([r, r, height_mm / 2.0], pitch_mm, pad_voxels), pitch_mm)


def gear_field(x, y, z, teeth, root_radius_mm, tooth_height_mm, height_mm):
    """rho - outline(angle), extruded: zero on the gear's surface, no distance (see `gear`)."""
    rho, ang = np.sqrt(x * x + y * y), np.arctan2(y, x)
    outline = root_radius_mm + tooth_height_mm * (0.5 + 0.5 * np.clip(1.5 * np.cos(teeth * ang), -1.0, 1.0))
    return _prism(rho - outline, z, height_mm)


def gear_step_scale(teeth, root_radius_mm, tooth_height_mm) -> float:
    """One over the bound sqrt(1 + (0.75 h teeth / root)^2) of the gradient of `gear_field` outside the root circle."""
    return 1.0 / math.sqrt(1.0 + (0.75 * tooth_height_mm * teeth / root_radius_mm) ** 2)


def gear(teeth: int = 12, root_radius_mm: float = 2.5, tooth_height_mm: float = 0.8, height_mm: float = 1.6, pitch_mm: float = 0.1,
         pad_voxels: int = 3) -> SdfVolume:
    """A spur gear around z: the outline rho = root + h * (0.5 + 0.5 clip(1.5 cos(teeth * angle), -1, 1)) - flat lands, flat roots,
    straight flanks - extruded to `height_mm`.  rho - outline(angle) is no distance: a segment from a point outside to the nearest
    surface point stays outside the root circle, where the field's gradient is at most sqrt(1 + (0.75 h teeth / root)^2); step_scale
    is one over that, which keeps every step below the distance."""
    r = root_radius_mm + tooth_height_mm
    return from_function(lambda x, y, z: gear_field(x, y, z, teeth, root_radius_mm, tooth_height_mm, height_mm),
                         _shape_for([r, r, height_mm / 2.0], pitch_mm, pad_voxels), pitch_mm, gear_step_scale(teeth, root_radius_mm, tooth_height_mm))


# ---- closed triangle meshes ----------------------------------------------------------------------------------------------------------
def _point_triangle_distance2(p, a, b, c):
    """Squared distance of points p (N, 1, 3) to triangles a, b, c (1, T, 3): closest point by the Voronoi regions of the triangle
    (vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, face - the first that applies)."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    dot = lambda u, v: (u * v).sum(-1)  # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        e_ab, e_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        e_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = va + vb + vc
        fv, fw = vb / den, vc / den
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    v = np.select(conds, [zero, one, e_ab, zero, zero, 1.0 - e_bc], fv)
    w = np.select(conds, [zero, zero, zero, one, e_ac, e_bc], fw)
    diff = ap - v[..., None] * ab - w[..., None] * ac
    return dot(diff, diff)


def _winding_number(p, a, b, c):
    """Generalised winding number of points p (N, 1, 3) about the oriented triangles a, b, c (1, T, 3): the sum of their signed solid
    angles (Van Oosterom - Strackee) over 4 pi; 1 inside a closed, outward oriented mesh, 0 outside."""
    u, v, w = a - p, b - p, c - p
    lu, lv, lw = (np.linalg.norm(t, axis=-1) for t in (u, v, w))
    num = (u * np.cross(v, w)).sum(-1)
    den = lu * lv * lw + (u * v).sum(-1) * lw + (v * w).sum(-1) * lu + (w * u).sum(-1) * lv
    return (2.0 * np.arctan2(num, den)).sum(-1) / (4.0 * np.pi)


def from_mesh(verts, tris, pitch_mm: float, pad_voxels: int = 2, chunk_points: int = 2048) -> SdfVolume:
    """The signed distance of a CLOSED triangle mesh (vertices in object mm, triangles oriented outwards or all inwards) on a grid of
    `pitch_mm` that holds its bounding box with `pad_voxels` around it; the anchor is the mesh frame's origin.  Unsigned distance:
    brute-force point-triangle distance, `chunk_points` grid points against every triangle at a time; sign: the generalised winding
    number (|w| > 0.5 is inside).  Plain NumPy, construction-time work of O(voxels * triangles): seconds for 24^3 x a few hundred
    triangles, up to a minute for 64^3 x a thousand."""
    verts, tris = np.asarray(verts, np.float64), np.asarray(tris, np.int64)
    if verts.ndim != 2 or verts.shape[1] != 3 or tris.ndim != 2 or tris.shape[1] != 3 or len(tris) == 0:
        raise ValueError(f"from_mesh: verts (Nv, 3) and tris (Nt, 3) expected, got {verts.shape} and {tris.shape}")
    lo, hi = verts.min(0), verts.max(0)
    first = np.floor(lo / pitch_mm).astype(np.int64) - int(pad_voxels)  # grid points sit on multiples of the pitch
    last = np.ceil(hi / pitch_mm).astype(np.int64) + int(pad_voxels)
    nx, ny, nz = (int(n) for n in last - first + 1)
    gz, gy, gx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = (np.stack([gx, gy, gz], -1).reshape(-1, 3) + first) * pitch_mm
    a, b, c = (verts[tris[:, k]][None] for k in range(3))
    out = np.empty(len(pts), np.float64)
    for s in range(0, len(pts), int(chunk_points)):
        p = pts[s:s + int(chunk_points), None, :]
        dist = np.sqrt(_point_triangle_distance2(p, a, b, c).min(-1))
        out[s:s + int(chunk_points)] = np.where(np.abs(_winding_number(p, a, b, c)) > 0.5, -dist, dist)
    return SdfVolume(out.reshape(nz, ny, nx).astype(np.float32), pitch_mm, tuple(float(-f) for f in first), 1.0)
