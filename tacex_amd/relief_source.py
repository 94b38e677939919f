"""Textured indenters: a library of relief tiles as a height-map source (`tacex_height_map_from_relief`,
tacex_amd/csrc/relief_source.hip; the contract is the comment of that call in include/tacex_hip.h).

A GelSight exists to see texture at pixel scale - fabric weave, knurling, threads, braille dots, coin relief.  A relief tile is a small
height field in mm; every env presses its own tile of the library, on a flat, spherical or cylindrical carrier, under a pose it updates
in place.  One HIP launch writes the height map, its frame minimum, the indentation depth and the contact ranges.

    from tacex_amd.utils import relief_tiles
    tiles = [relief_tiles.weave(), relief_tiles.knurl(), relief_tiles.disc_stamp()]
    src = ReliefHeightMapSource(tiles, num_envs, "cuda:0")
    src.randomize()                                      # at reset: a tile per env, drawn on the device
    src.set_pose(cx_px=160, cy_px=120, yaw=0.3, press_mm=0.8, carrier="sphere", radius_mm=6.0)
    sensor.set_height_map_source(src)                    # every update now rasterises the reliefs

The projection is orthographic, as in `IndenterHeightMapSource`, and the relief is displaced along the optical axis: a height field
without undercuts."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _stage

CARRIERS = {"plane": 0.0, "sphere": 1.0, "cylinder": 2.0}
POSE_FIELDS = ("m00", "m01", "m02", "m10", "m11", "m12", "press_mm", "t0", "tx", "ty", "carrier", "radius_mm", "gain", "du", "dv", "reserved")


@dataclass
class ReliefTile:
    """One relief: `height_mm` (rows, cols) - how far each texel stands proud of the carrier [mm], -inf where there is no material
    (NaN and +inf are refused) -, the texel pitch `pitch_mm`, `wrap` (the tile repeats in both directions; otherwise nothing lies
    outside it) and `anchor` = (u0, v0), the texel coordinates of the carrier's origin (default: the tile centre)."""

    height_mm: object
    pitch_mm: float
    wrap: bool = True
    anchor: object = None

    def __post_init__(self):
        self.validate()

    def validate(self):
        h = np.ascontiguousarray(np.asarray(self.height_mm, dtype=np.float32))
        if h.ndim != 2 or h.size == 0:
            raise ValueError(f"ReliefTile: height_mm must be a non-empty (rows, cols) array, got shape {h.shape}")
        if np.isnan(h).any() or np.isposinf(h).any():
            raise ValueError("ReliefTile: height_mm holds NaN or +inf (-inf marks 'no material')")
        if not np.isfinite(h).any():
            raise ValueError("ReliefTile: height_mm has no finite texel")
        pitch = float(self.pitch_mm)
        if not (math.isfinite(pitch) and pitch > 0):
            raise ValueError(f"ReliefTile: pitch_mm must be > 0, got {self.pitch_mm}")
        if self.anchor is not None:
            a = np.asarray(self.anchor, dtype=np.float64)
            if a.shape != (2,) or not np.isfinite(a).all():
                raise ValueError(f"ReliefTile: anchor must be two finite texel coordinates (u0, v0), got {self.anchor}")
        self.height_mm, self.pitch_mm, self.wrap = h, pitch, bool(self.wrap)
        return h

    @property
    def top_mm(self) -> float:
        """The largest finite texel."""
        h = self.height_mm
        return float(h[np.isfinite(h)].max())

    @property
    def anchor_uv(self):
        Th, Tw = self.height_mm.shape
        return ((Tw - 1) / 2.0, (Th - 1) / 2.0) if self.anchor is None else (float(self.anchor[0]), float(self.anchor[1]))

    def row(self) -> np.ndarray:
        """The (4,) float32 row [pitch_mm, top_mm, u0, v0] of the library's float table."""
        u0, v0 = self.anchor_uv
        return np.asarray([self.pitch_mm, self.top_mm, u0, v0], dtype=np.float32)


class ReliefHeightMapSource(_stage.LibrarySource):
    """A relief tile per env as the sensor's height-map source (`GelSightSensor.set_height_map_source`).  It owns the library - `texels`
    (all tiles back to back), `tiles_i` (P, 4) int32 [first texel, rows, cols, wrap], `tiles_f` (P, 4) float32 [pitch_mm, top_mm, u0,
    v0] - and two tensors the caller writes in place between steps: `pose` (num_envs, 16) float32 (`POSE_FIELDS`; `set_pose` fills it
    from a placement in pixels) and `relief_ids` (num_envs,) int32 (`randomize()` re-draws them; an id outside [0, P) presses
    nothing).  `samples` = 4 averages four sub-pixel samples: the anti-aliasing for stamp edges and tiles finer than the pixel.
    The projection is orthographic and the relief is displaced along the optical axis: a height field without undercuts."""

    _owner, _unit, _names = "ReliefHeightMapSource", "texel", ("texels", "tiles_i", "tiles_f", "relief_ids")
    tiles_f, relief_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

    def __init__(self, tiles, num_envs: int, device, pixmm: float = 0.0295, gel_top_mm: float = 28.5, far_clip_mm: float = 29.0,
                 samples: int = 1):
        tiles = _stage.profile_list("ReliefHeightMapSource", "tiles", tiles, ReliefTile)
        heights = [t.validate() for t in tiles]
        if samples not in (1, 4):
            raise ValueError(f"ReliefHeightMapSource: samples = {samples} (must be 1 or 4)")
        self._open(tiles, ReliefTile, heights, [(h.shape[0], h.shape[1], int(t.wrap)) for h, t in zip(heights, tiles)], num_envs, device, pixmm)
        self.tiles, self.samples = tuple(tiles), int(samples)
        self.gel_top_mm, self.far_clip_mm = float(gel_top_mm), float(far_clip_mm)
        self.pose[:, 0] = self.pose[:, 4] = 1.0  # (identity M, plane carrier; gain 1)
        self.pose[:, 12] = 1.0

    @property
    def num_tiles(self) -> int:
        return len(self.tiles)

    def set_pose(self, cx_px, cy_px, yaw, press_mm, scale=1.0, tilt=(0, 0), carrier="plane", radius_mm=0.0, gain=1.0,
                 shift_texels=(0, 0), env_ids=slice(None)):
        """Place the relief of `env_ids` (default: all): its anchor at pixel (cx_px, cy_px), turned by `yaw` [rad], magnified by
        `scale`, its highest point `press_mm` below the gel top (where the carrier is 0), the whole object tilted by `tilt` = (tx, ty)
        [mm/px] about that pixel, on `carrier` ("plane", "sphere", "cylinder" - axis along the tile's u - or a tensor of codes) of
        `radius_mm`, the relief scaled by `gain`, the texture scrolled by `shift_texels` = (du, dv) against the carrier (rolling).
        Arguments are scalars or per-env tensors.  Built with torch ops on the device from each env's tile row (gathered by
        `relief_ids` as they are now), without a host sync:
            k = pixmm / (pitch * scale);   m00 = k cos, m01 = k sin, m02 = u0 - (m00 cx + m01 cy);
            m10 = -k sin, m11 = k cos, m12 = v0 - (m10 cx + m11 cy);   t0 = -(tx cx + ty cy)"""
        dev = self.device
        ids = self.relief_ids[env_ids].long().clamp(0, self.num_tiles - 1)
        row = self.tiles_f[ids].double()
        n = ids.shape[0]
        per_env = functools.partial(_stage.per_env, n=n, device=dev)
        cx, cy, yaw, scale = per_env(cx_px), per_env(cy_px), per_env(yaw), per_env(scale)
        tx, ty = per_env(tilt[0]), per_env(tilt[1])
        k = self.pixmm / (row[:, 0] * scale)
        cs, sn = torch.cos(yaw), torch.sin(yaw)
        m00, m01, m10, m11 = k * cs, k * sn, -k * sn, k * cs
        code = CARRIERS[carrier] if isinstance(carrier, str) else carrier
        cols = [m00, m01, row[:, 2] - (m00 * cx + m01 * cy), m10, m11, row[:, 3] - (m10 * cx + m11 * cy), per_env(press_mm),
                -(tx * cx + ty * cy), tx, ty, per_env(code), per_env(radius_mm), per_env(gain), per_env(shift_texels[0]),
                per_env(shift_texels[1]), torch.zeros(n, dtype=torch.float64, device=dev)]
        self.pose[env_ids] = torch.stack(cols, dim=1).float()

    def _launch(self, texels, tiles_i, tiles_f, ids, hm, frame_min, indent, rows, gelpad_height, gelpad_to_camera_min_distance):
        dev = self.device
        with torch.cuda.device(dev):  # (one launch)
            rc = self._lib.tacex_height_map_from_relief(
                _lib.ptr(texels), _lib.ptr(tiles_i), _lib.ptr(tiles_f), self.num_tiles, _lib.ptr(ids), _lib.ptr(self.pose),
                self.gel_top_mm, self.far_clip_mm, gelpad_height, gelpad_to_camera_min_distance, _lib.ptr(hm), _lib.ptr(frame_min),
                _lib.ptr(indent), _lib.ptr(rows), self.num_envs, int(hm.shape[1]), int(hm.shape[2]), self.samples,
                _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_height_map_from_relief")
