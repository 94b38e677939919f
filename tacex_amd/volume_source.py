"""Volumetric indenters: a library of signed-distance grids as a height-map source (`tacex_height_map_from_sdf`,
tacex_amd/csrc/volume_source.hip; the contract is the comment of that call in include/tacex_hip.h).

Real parts - pegs, gears, nuts, bolts - meet the pad at an arbitrary 3-D pose.  A relief tile cannot be rolled or turned over, and a
mesh costs time per triangle.  A signed-distance volume takes a full rigid pose, uniform scale and inflation (iso level), and its
cost per pixel does not depend on how detailed the object is: every pixel's ray is sphere-traced through the few millimetres between
the clip planes, one trilinear tap per step.

    from tacex_amd.utils import sdf_volumes
    vols = [sdf_volumes.hex_nut(), sdf_volumes.gear(), sdf_volumes.torus()]
    src = SdfVolumeSource(vols, num_envs, "cuda:0")
    src.randomize()                                      # at reset: a volume per env, drawn on the device
    src.set_pose(cx_px=160, cy_px=120, quat_wxyz=(0.92, 0.38, 0.0, 0.0), press_mm=0.8)
    sensor.set_height_map_source(src)                    # every update now marches the volumes

The projection is orthographic, as in `IndenterHeightMapSource`: X = column * pixmm, Y = row * pixmm, Z = depth [mm]."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _stage

POSE_FIELDS = ("r00", "r01", "r02", "r10", "r11", "r12", "r20", "r21", "r22", "tx", "ty", "tz", "scale", "level_mm", "reserved0", "reserved1")
MAX_SURFACE_POINTS = 4096


@dataclass
class SdfVolume:
    """One volume: `sdf_mm` (D, Hv, Wv) float32 - signed distances in object mm, negative inside, index order z, y, x, every axis
    >= 2, all finite, at least one value <= 0 and one > 0 -, the voxel pitch `pitch_mm`, `anchor` = (i0, j0, k0), the voxel
    coordinates (x, y, z) of the object frame's origin (default: the grid centre), and `step_scale` in (0, 1], which shortens every
    step of the march (for fields that bound the distance from below without being one)."""

    sdf_mm: object
    pitch_mm: float
    anchor: object = None
    step_scale: float = 1.0

    def __post_init__(self):
        self.validate()

    def validate(self):
        s = np.ascontiguousarray(np.asarray(self.sdf_mm, dtype=np.float32))
        if s.ndim != 3 or min(s.shape) < 2:
            raise ValueError(f"SdfVolume: sdf_mm must be a (D, Hv, Wv) array with every axis >= 2, got shape {s.shape}")
        if not np.isfinite(s).all():
            raise ValueError("SdfVolume: sdf_mm holds NaN or inf")
        if not ((s <= 0).any() and (s > 0).any()):
            raise ValueError("SdfVolume: sdf_mm needs a value <= 0 (inside) and a value > 0 (outside)")
        pitch = float(self.pitch_mm)
        if not (math.isfinite(pitch) and pitch > 0):
            raise ValueError(f"SdfVolume: pitch_mm must be > 0, got {self.pitch_mm}")
        step = float(self.step_scale)
        if not (0 < step <= 1):
            raise ValueError(f"SdfVolume: step_scale must lie in (0, 1], got {self.step_scale}")
        if self.anchor is not None:
            a = np.asarray(self.anchor, dtype=np.float64)
            if a.shape != (3,) or not np.isfinite(a).all():
                raise ValueError(f"SdfVolume: anchor must be three finite voxel coordinates (i0, j0, k0), got {self.anchor}")
        self.sdf_mm, self.pitch_mm, self.step_scale = s, pitch, step
        return s

    @property
    def anchor_ijk(self):
        D, Hv, Wv = self.sdf_mm.shape
        if self.anchor is None:
            return ((Wv - 1) / 2.0, (Hv - 1) / 2.0, (D - 1) / 2.0)
        return tuple(float(v) for v in self.anchor)

    def row(self) -> np.ndarray:
        """The (8,) float32 row [pitch_mm, i0, j0, k0, step_scale, 0, 0, 0] of the library's float table."""
        return np.asarray([self.pitch_mm, *self.anchor_ijk, self.step_scale, 0, 0, 0], dtype=np.float32)

    def surface_points(self, count: int = MAX_SURFACE_POINTS) -> np.ndarray:
        """(count, 3) float32 points [object mm, x y z] on the zero level: the voxels within one pitch of it, moved onto it along the
        grid's gradient; the extreme ones in 1024 directions first, the rest evenly thinned (repeated when there are fewer)."""
        s = self.sdf_mm.astype(np.float64)
        k, j, i = np.nonzero(np.abs(s) <= self.pitch_mm)
        if k.size == 0:  # (a grid coarser than its object: the voxels beside a change of sign)
            k, j, i = np.nonzero(np.abs(s) <= np.abs(s).min() + self.pitch_mm)
        gz, gy, gx = (g[k, j, i] for g in np.gradient(s, self.pitch_mm))
        n = np.stack([gx, gy, gz], 1)
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)
        p = (np.stack([i, j, k], 1) - np.asarray(self.anchor_ijk)) * self.pitch_mm - s[k, j, i][:, None] * n
        m = np.arange(1024) + 0.5
        polar, turn = np.arccos(1 - 2 * m / 1024), np.pi * (1 + 5 ** 0.5) * m
        dirs = np.stack([np.cos(turn) * np.sin(polar), np.sin(turn) * np.sin(polar), np.cos(polar)], 1)
        extreme = np.unique(np.concatenate([(p @ dirs[c:c + 64].T).argmax(0) for c in range(0, 1024, 64)]))[:count]
        rest = np.setdiff1d(np.arange(len(p)), extreme)
        room = count - len(extreme)
        if room and len(rest):
            rest = rest[np.linspace(0, len(rest) - 1, min(room, len(rest))).round().astype(np.int64)]
        picked = p[np.concatenate([extreme, rest[:room]])]
        return np.resize(picked, (count, 3)).astype(np.float32)


def placement_rows(src, ids, cx_px, cy_px, quat_wxyz, press_mm, z_mm, scale, level_mm, blend_mm=0.0) -> torch.Tensor:
    """(n, 16) float32 pose rows (`POSE_FIELDS`) for the volumes `ids` (n,) long of `src` (its `surface_points`, `gel_top_mm`, `pixmm`,
    `device`): the placement of `SdfVolumeSource.set_pose`, shared with `SdfSceneSource.set_pose` (whose rows carry `blend_mm`)."""
    dev = src.device
    n = ids.shape[0]
    per_env = functools.partial(_stage.per_env, n=n, device=dev)
    q = quat_wxyz.to(device=dev, dtype=torch.float64) if isinstance(quat_wxyz, torch.Tensor) else torch.tensor(
        [float(c) for c in quat_wxyz], dtype=torch.float64, device=dev)
    q = (q.expand(n, 4) if q.dim() == 1 else q)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1)
    scale, level = per_env(scale), per_env(level_mm)
    if z_mm is not None:
        tz = per_env(z_mm)
    else:
        low = (src.surface_points[ids].double() * R[:, None, 6:9]).sum(-1).min(dim=1).values
        tz = (src.gel_top_mm - per_env(press_mm)) - scale * (low - level)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    cols = [per_env(cx_px) * src.pixmm, per_env(cy_px) * src.pixmm, tz, scale, level, per_env(blend_mm) + zero, zero]
    return torch.cat([R, torch.stack(cols, dim=1)], dim=1).float()


class SdfVolumeSource(_stage.LibrarySource):
    """A signed-distance volume per env as the sensor's height-map source (`GelSightSensor.set_height_map_source`).  It owns the
    library - `voxels` (all grids back to back), `volumes_i` (P, 4) int32 [first voxel, D, Hv, Wv], `volumes_f` (P, 8) float32
    [pitch_mm, i0, j0, k0, step_scale, 0, 0, 0], `surface_points` (P, K, 3) for `set_pose(press_mm=)` - and two tensors the caller
    writes in place between steps: `pose` (num_envs, 16) float32 (`POSE_FIELDS`: R row-major object -> camera, t [mm], scale,
    level_mm; `set_pose` fills it from a placement in pixels) and `volume_ids` (num_envs,) int32 (`randomize()` re-draws them; an id
    outside [0, P) presses nothing).  The surface is {sdf = level_mm}: a positive level inflates the object.  Rays are marched
    between `near_clip_mm` and `far_clip_mm` for at most `max_steps` taps and stop within `tol_mm` of the surface."""

    _owner, _unit, _names = "SdfVolumeSource", "voxel", ("voxels", "volumes_i", "volumes_f", "volume_ids")
    volumes_f, volume_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

    def __init__(self, volumes, num_envs: int, device, pixmm: float = 0.0295, gel_top_mm: float = 28.5, near_clip_mm: float = 24.0,
                 far_clip_mm: float = 29.0, max_steps: int = 32, tol_mm: float = 1e-4):
        volumes = _stage.profile_list("SdfVolumeSource", "volumes", volumes, SdfVolume)
        grids = [v.validate() for v in volumes]
        if not 1 <= int(max_steps) <= 128:
            raise ValueError(f"SdfVolumeSource: max_steps = {max_steps} (must be 1..128)")
        if not float(tol_mm) > 0:
            raise ValueError(f"SdfVolumeSource: tol_mm must be > 0, got {tol_mm}")
        if not float(near_clip_mm) < float(far_clip_mm):
            raise ValueError(f"SdfVolumeSource: near_clip_mm = {near_clip_mm} must lie below far_clip_mm = {far_clip_mm}")
        self._open(volumes, SdfVolume, grids, [g.shape for g in grids], num_envs, device, pixmm)
        self.volumes, self.max_steps = tuple(volumes), int(max_steps)
        self.gel_top_mm, self.tol_mm = float(gel_top_mm), float(tol_mm)
        self.near_clip_mm, self.far_clip_mm = float(near_clip_mm), float(far_clip_mm)
        self._surface_points = None
        self.pose[:, 0] = self.pose[:, 4] = self.pose[:, 8] = self.pose[:, 12] = 1.0  # (identity R, scale 1)
        self.pose[:, 11] = 2.0 * self.far_clip_mm  # (until set_pose: beyond far clip)

    @property
    def num_volumes(self) -> int:
        return len(self.volumes)

    @property
    def surface_points(self) -> torch.Tensor:
        """(P, K, 3) float32 points on each volume's zero level [object mm]: built on the host at the first use, then kept."""
        if self._surface_points is None:
            self._surface_points = torch.from_numpy(np.stack([v.surface_points() for v in self.volumes])).to(self.device)
        return self._surface_points

    def set_pose(self, cx_px, cy_px, quat_wxyz, press_mm=None, z_mm=None, scale=1.0, level_mm=0.0, env_ids=slice(None)):
        """Place the volume of `env_ids` (default: all): its anchor at pixel (cx_px, cy_px), turned by `quat_wxyz` (object -> camera;
        normalised here; a tuple or an (n, 4) tensor), magnified by `scale`, inflated by `level_mm`.  Depth: `z_mm` is the anchor's
        depth [mm]; or `press_mm` puts the object's lowest point under this rotation `press_mm` below the gel top,
            tz = (gel_top - press) - scale * (min over the surface points of R[2] . p  -  level),
        with the library's `surface_points` (P, K, 3), K = 4096 points on the zero level built once on the host, at the first such
        call.  Their spacing and the projection onto the trilinear surface make this good to about ONE VOXEL PITCH (times scale);
        the exact press depth is whatever `indent` then reports.  Arguments are scalars or per-env tensors; torch ops on the device,
        no host sync."""
        if (press_mm is None) == (z_mm is None):
            raise ValueError("SdfVolumeSource.set_pose: give exactly one of press_mm and z_mm")
        ids = self.volume_ids[env_ids].long().clamp(0, self.num_volumes - 1)
        self.pose[env_ids] = placement_rows(self, ids, cx_px, cy_px, quat_wxyz, press_mm, z_mm, scale, level_mm)

    def _launch(self, voxels, volumes_i, volumes_f, ids, hm, frame_min, indent, rows, gelpad_height, gelpad_to_camera_min_distance):
        dev = self.device
        with torch.cuda.device(dev):  # (two launches: the march, then the frame outputs of the map)
            rc = self._lib.tacex_height_map_from_sdf(
                _lib.ptr(voxels), int(voxels.shape[0]), _lib.ptr(volumes_i), _lib.ptr(volumes_f), self.num_volumes, _lib.ptr(ids),
                _lib.ptr(self.pose), self.pixmm, self.near_clip_mm, self.far_clip_mm, self.max_steps, self.tol_mm, gelpad_height,
                gelpad_to_camera_min_distance, _lib.ptr(hm), _lib.ptr(frame_min), _lib.ptr(indent), _lib.ptr(rows), self.num_envs,
                int(hm.shape[1]), int(hm.shape[2]), _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_height_map_from_sdf")
