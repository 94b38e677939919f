"""Sensor lens model: per-env distortion, mounting misalignment, vignetting and defocus for `tactile_rgb` - the stage between the
rendered frame and the camera model (`tacex_lens_model`, `tacex_lens_camera_model`, `tacex_lens_points`,
tacex_amd/csrc/lens_model.hip; the contract is the comment of `tacex_lens_model` in include/tacex_hip.h).

    units = [LensProfile.identity(), LensProfile(k1=-0.15, k2=0.03, rotation_deg=1.5, scale=1.02, shift_px=(2.5, -1.0),
                                                 vignette=(-0.25, -0.05), softness=(0.0, 1.0))]
    lens = TactileLensModel(units, num_frames=num_envs, device="cuda:0")
    lens.randomize()                                  # at reset: a unit per env, drawn on the device
    frame = sensor.lens_image(lens)                   # (num_envs, H, W, 3) float32 through the lens: one launch
    frame_u8 = sensor.lens_image(lens, camera)        # lens and `TactileCameraModel` in one launch: what the chip delivers
    markers = lens.distort_points(marker_motion)      # marker coordinates moved the way the image is

An env's image depends on its own input and profile alone, and a run is reproducible bit for bit."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _stage
from .camera_model import _OUT_DTYPES, TactileCameraModel


@dataclass
class LensProfile:
    """One sensor unit's lens and mounting.  Output pixel (i, j) shows the source position (u, v) = (j, i) + E p + (W/2) d(p s) + t
    with p = (j + 0.5 - W/2 - cx, i + 0.5 - H/2 - cy), s = 2 / W, d the Brown-Conrady displacement (`k1`, `k2` radial - a negative
    k1 pulls the source of a corner pixel towards the centre, a positive one pushes it outwards -, `p1`, `p2` tangential) and
    E = A - I for A = scale R(rotation_deg) [[1, shear], [0, 1]] (or `matrix` = A).
    `shift_px` = t = (tx, ty), `centre_px` = (cx, cy): the optical centre's offset from the frame centre.
    `vignette` = (v1, v2): gain clamp(1 + v1 r^2 + v2 r^4, 0, 1); `softness` = (b0, b2): the side clamp(b0 + b2 r^2, 0, 4) [px] of
    the box the four bilinear taps of a pixel span (both 0: one tap).  r^2 is in normalised units (1 at half the frame's width)."""

    k1: float = 0.0
    k2: float = 0.0
    p1: float = 0.0
    p2: float = 0.0
    rotation_deg: float = 0.0
    scale: float = 1.0
    shear: float = 0.0
    matrix: object = None
    shift_px: object = (0.0, 0.0)
    centre_px: object = (0.0, 0.0)
    vignette: object = (0.0, 0.0)
    softness: object = (0.0, 0.0)

    @classmethod
    def identity(cls) -> "LensProfile":
        return cls()

    def row(self) -> np.ndarray:
        """The (16,) float32 row of `tacex_lens_model`'s profile table (the trigonometry of `rotation_deg` is done here, in float64)."""
        pairs = {}
        for name in ("shift_px", "centre_px", "vignette", "softness"):
            v = np.asarray(getattr(self, name), dtype=np.float64)
            if v.shape != (2,):
                raise ValueError(f"LensProfile: {name} must be 2 values, got shape {v.shape}")
            pairs[name] = v
        scal = np.array([self.k1, self.k2, self.p1, self.p2, self.rotation_deg, self.scale, self.shear], dtype=np.float64)
        if not (np.isfinite(scal).all() and all(np.isfinite(v).all() for v in pairs.values())):
            raise ValueError("LensProfile: values must be finite")
        if self.matrix is None:
            if not self.scale > 0:
                raise ValueError(f"LensProfile: scale must be > 0, got {self.scale}")
            t = math.radians(float(self.rotation_deg))
            A = float(self.scale) * (np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
                                     @ np.array([[1.0, float(self.shear)], [0.0, 1.0]]))
        else:
            A = np.asarray(self.matrix, dtype=np.float64)
            if A.shape != (2, 2):
                raise ValueError(f"LensProfile: matrix must be 2 x 2, got shape {A.shape}")
            if not np.isfinite(A).all():
                raise ValueError("LensProfile: values must be finite")
        if (pairs["softness"] < 0).any():
            raise ValueError("LensProfile: softness must be >= 0")
        E = A - np.eye(2)
        row = np.concatenate([scal[:4], E.reshape(4), pairs["shift_px"], pairs["centre_px"], pairs["vignette"], pairs["softness"]])
        with np.errstate(over="ignore"):
            row = row.astype(np.float32)
        if not np.isfinite(row).all():
            raise ValueError("LensProfile: values must be finite in float32")
        return row


class TactileLensModel:
    """The lens model of `num_frames` envs.  `profiles` (P,16) float32 and `profile_ids` (num_frames,) int32 are device tensors the
    caller may write in place (ids at reset, like `TactileCameraModel.profile_ids`; an id outside [0, P) is the identity profile).
    `image_size` (H, W): the frame size `distort_points` assumes; every `__call__` sets it to the size of its image."""

    profiles, profile_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

    def __init__(self, profiles, num_frames: int, device, image_size=None):
        self._lib, self._table = _stage.open_stage("TactileLensModel", "profiles", "profile_ids", profiles, LensProfile, num_frames, device)
        self.device = torch.device(device)
        self.num_frames = int(num_frames)
        self.image_size = None if image_size is None else (int(image_size[0]), int(image_size[1]))

    @property
    def num_profiles(self) -> int:
        return int(self.profiles.shape[0])

    def randomize(self, env_ids=None, generator=None):
        """Re-draw the profile ids of `env_ids` (default: all) uniformly from [0, P) on the device."""
        return self._table.randomize(env_ids, generator)

    def __call__(self, rgb: torch.Tensor, out: torch.Tensor | None = None, camera: TactileCameraModel | None = None,
                 call: int | None = None) -> torch.Tensor:
        """One launch on the current stream.  `rgb` (num_frames,H,W,3) float32, contiguous, on the model's device.  `camera` None:
        the gather alone -> float32.  `camera` a `TactileCameraModel` of the same num_frames: the gather and the camera model in the
        same launch -> the camera's dtype, bit-equal to `camera(lens(rgb))`; the camera's `call` counter is used and advanced as its
        own `__call__` would (`call` overrides it).  `out`: same shape, the result's dtype, never `rgb` itself; allocated when None."""
        B, dev = self.num_frames, self._table.device
        _stage.check_tensor("TactileLensModel", "rgb", rgb, (B, "H", "W", 3), torch.float32, dev)
        if camera is not None:
            if not isinstance(camera, TactileCameraModel):
                raise ValueError(f"TactileLensModel: camera must be a TactileCameraModel, got {type(camera).__name__}")
            if camera.num_frames != B:
                raise ValueError(f"TactileLensModel: the camera model has {camera.num_frames} frames, the lens model {B}")
            if camera.profiles.device != dev:
                raise ValueError(f"TactileLensModel: the camera model is on {camera.profiles.device}, rgb on {dev}")
        elif call is not None:
            raise ValueError("TactileLensModel: call numbers the camera model's noise draws; it needs camera=")
        dtype = torch.float32 if camera is None else camera.dtype
        if out is None:
            out = torch.empty(rgb.shape, dtype=dtype, device=dev)
        else:
            _stage.check_tensor("TactileLensModel", "out", out, tuple(rgb.shape), dtype, dev)
        if out.data_ptr() == rgb.data_ptr():
            raise ValueError("TactileLensModel: out must not be rgb (a gather cannot run in place)")
        ids, prof = self._table.check()
        H, W = int(rgb.shape[1]), int(rgb.shape[2])
        self.image_size = (H, W)
        stream = _lib.current_stream_handle(dev)
        if camera is None:
            with torch.cuda.device(dev):
                rc = self._lib.tacex_lens_model(_lib.ptr(rgb), _lib.ptr(prof), int(prof.shape[0]), _lib.ptr(ids), _lib.ptr(out), B, H, W, stream)
            _lib.check(rc, "tacex_lens_model")
            return out
        cids, cprof, call = camera._tables_and_call(call)
        with torch.cuda.device(dev):
            rc = self._lib.tacex_lens_camera_model(_lib.ptr(rgb), _lib.ptr(prof), int(prof.shape[0]), _lib.ptr(ids), _lib.ptr(cprof),
                                                   int(cprof.shape[0]), _lib.ptr(cids), camera.seed, camera.frame_offset, call,
                                                   _lib.ptr(out), _OUT_DTYPES[camera.dtype], B, H, W, stream)
        _lib.check(rc, "tacex_lens_camera_model")
        return out

    def distort_points(self, xy: torch.Tensor, out: torch.Tensor | None = None, height: int | None = None,
                       width: int | None = None) -> torch.Tensor:
        """Point coordinates moved the way the lens moves a `height` x `width` image (default: `image_size`, the size of the last
        image this model was called on): `xy` (num_frames,N,2) float64 in ideal image pixels (x = column, y = row), or
        `marker_motion`'s (num_frames,2,M,2) of any float dtype (converted at the boundary; the result has the input's shape and
        dtype).  `out` may be `xy`."""
        if height is None or width is None:
            if self.image_size is None:
                raise ValueError("TactileLensModel: distort_points needs height= and width= (or image_size=) before the first image")
            height = self.image_size[0] if height is None else height
            width = self.image_size[1] if width is None else width
        dev = self._table.device
        # (xy is the one argument that need not be contiguous, and a 4-d one may have any float dtype: it is converted below)
        if not isinstance(xy, torch.Tensor) or xy.dim() not in (3, 4) or xy.shape[0] != self.num_frames or xy.shape[-1] != 2 \
                or (xy.dim() == 4 and xy.shape[1] != 2) or xy.numel() == 0 or not xy.dtype.is_floating_point:
            raise ValueError(f"TactileLensModel: xy must be a ({self.num_frames}, N, 2) float64 or ({self.num_frames}, 2, M, 2) float tensor, got "
                             f"{tuple(xy.shape) if isinstance(xy, torch.Tensor) else type(xy).__name__}")
        if xy.dim() == 3 and xy.dtype != torch.float64:
            raise ValueError(f"TactileLensModel: a ({self.num_frames}, N, 2) xy must be float64, got {xy.dtype}")
        if int(height) < 1 or int(width) < 1:
            raise ValueError(f"TactileLensModel: height x width = {height} x {width}")
        if xy.device != dev:
            raise _lib.TacexHipError(f"TactileLensModel: xy is on {xy.device}, the model on {dev} (no CPU fallback)")
        if out is not None:
            _stage.check_tensor("TactileLensModel", "out", out, tuple(xy.shape), xy.dtype, dev)
        ids, prof = self._table.check()
        direct = xy.dtype == torch.float64 and xy.is_contiguous()
        src = xy if direct else xy.to(torch.float64).contiguous()
        dst = (out if out is not None else torch.empty_like(src)) if direct else src  # a converted copy is moved in place
        n = src.numel() // (2 * self.num_frames)
        with torch.cuda.device(dev):
            rc = self._lib.tacex_lens_points(_lib.ptr(src), _lib.ptr(prof), int(prof.shape[0]), _lib.ptr(ids), _lib.ptr(dst), self.num_frames,
                                             n, int(height), int(width), _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_lens_points")
        if direct:
            return dst
        if out is None:
            return dst.to(xy.dtype)
        out.copy_(dst)
        return out
