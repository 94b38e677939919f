"""Sensor camera model: per-env colour response, fixed-pattern gain, read + shot noise and 8-bit frames for `tactile_rgb`
(`tacex_camera_model`, tacex_amd/csrc/camera_model.hip; the contract is that function's comment in include/tacex_hip.h).

    profiles = [CameraProfile.identity(), CameraProfile(color_matrix=M, offset=o, read_noise=0.01, shot_noise=2e-4, fixed_pattern=0.01)]
    model = TactileCameraModel(profiles, num_frames=num_envs, device="cuda:0", seed=7)
    model.randomize()                       # at reset: a profile per env, drawn on the device
    frame_u8 = sensor.camera_image(model)   # (num_envs, H, W, 3) uint8, one launch, no host synchronisation

Draws come from Philox4x32-10 addressed by (seed, frame_offset + env, call, pixel group): an env's image does not depend on the batch
it is rendered in, and a run is reproducible bit for bit."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, _stage

_OUT_DTYPES = {torch.float32: 0, torch.uint8: 1}


@dataclass
class CameraProfile:
    """One camera unit: out = clamp(noise(clamp(fixed_pattern(color_matrix @ rgb + offset)))).  `read_noise` is the standard deviation
    of the signal-independent noise in units of full scale, `shot_noise` the coefficient s of the signal-dependent part (variance
    s * signal), `fixed_pattern` the standard deviation of the per-pixel gain around 1 (the same pattern in every call)."""

    color_matrix: object = field(default_factory=lambda: np.eye(3, dtype=np.float32))
    offset: object = 0.0
    read_noise: float = 0.0
    shot_noise: float = 0.0
    fixed_pattern: float = 0.0

    @classmethod
    def identity(cls) -> "CameraProfile":
        return cls()

    def row(self) -> np.ndarray:
        """The (16,) float32 row of `tacex_camera_model`'s profile table."""
        m = np.asarray(self.color_matrix, dtype=np.float32)
        if m.shape != (3, 3):
            raise ValueError(f"CameraProfile: color_matrix must be 3 x 3, got shape {m.shape}")
        o = np.broadcast_to(np.asarray(self.offset, dtype=np.float32), (3,)) if np.ndim(self.offset) == 0 else np.asarray(self.offset, dtype=np.float32)
        if o.shape != (3,):
            raise ValueError(f"CameraProfile: offset must be a scalar or 3 values, got shape {o.shape}")
        scal = np.array([self.read_noise, self.shot_noise, self.fixed_pattern], dtype=np.float32)
        if not (np.isfinite(m).all() and np.isfinite(o).all() and np.isfinite(scal).all()):
            raise ValueError("CameraProfile: values must be finite")
        if (scal < 0).any():
            raise ValueError("CameraProfile: read_noise, shot_noise and fixed_pattern must be >= 0")
        return np.concatenate([m.reshape(9), o, scal, np.zeros(1, dtype=np.float32)]).astype(np.float32)


class TactileCameraModel:
    """The camera model of `num_frames` envs.  `profiles` (P,16) float32 and `profile_ids` (num_frames,) int32 are device tensors the
    caller may write in place (ids at reset, like `pattern_ids`; an id outside [0, P) is the identity profile).  `call` numbers the
    launches: it is the time coordinate of the noise draws and is incremented by every `__call__` that does not pass its own.
    `frame_offset`: the global index of this model's first env (an env shard renders the frames the whole batch would)."""

    profiles, profile_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

    def __init__(self, profiles, num_frames: int, device, seed: int = 0, dtype: torch.dtype = torch.uint8, frame_offset: int = 0):
        if dtype not in _OUT_DTYPES:
            raise ValueError(f"TactileCameraModel: dtype must be torch.uint8 or torch.float32, got {dtype}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("TactileCameraModel: seed must fit 64 bits")
        if not 0 <= int(frame_offset) <= 2 ** 32 - int(num_frames):
            raise ValueError("TactileCameraModel: frame_offset + num_frames must fit 32 bits")
        self._lib, self._table = _stage.open_stage("TactileCameraModel", "profiles", "profile_ids", profiles, CameraProfile, num_frames, device)
        self.device = torch.device(device)
        self.num_frames = int(num_frames)
        self.seed = int(seed)
        self.dtype = dtype
        self.frame_offset = int(frame_offset)
        self.call = 0

    @property
    def num_profiles(self) -> int:
        return int(self.profiles.shape[0])

    def randomize(self, env_ids=None, generator=None):
        """Re-draw the profile ids of `env_ids` (default: all) uniformly from [0, P) on the device."""
        return self._table.randomize(env_ids, generator)

    def _tables_and_call(self, call):
        """(ids, profiles, call) of one launch, this model's or a fused one: the tables as the kernels expect them, `call` or the
        running counter, which is then advanced."""
        ids, prof = self._table.check()
        if call is None:
            call = self.call
            self.call = (self.call + 1) & 0xFFFFFFFF
        elif not 0 <= int(call) < 2 ** 32:
            raise ValueError("TactileCameraModel: call must fit 32 bits")
        return ids, prof, int(call)

    def __call__(self, rgb: torch.Tensor, out: torch.Tensor | None = None, call: int | None = None) -> torch.Tensor:
        """One launch on the current stream.  `rgb` (num_frames,H,W,3) float32, contiguous, on the model's device; `out` of the same
        shape and the model's dtype (float32 may be `rgb` itself), allocated when None.  `call` overrides the running counter."""
        dev = self._table.device
        _stage.check_tensor("TactileCameraModel", "rgb", rgb, (self.num_frames, "H", "W", 3), torch.float32, dev)
        if out is None:
            out = torch.empty(rgb.shape, dtype=self.dtype, device=dev)
        else:
            _stage.check_tensor("TactileCameraModel", "out", out, tuple(rgb.shape), self.dtype, dev)
        ids, prof, call = self._tables_and_call(call)
        with torch.cuda.device(dev):
            rc = self._lib.tacex_camera_model(_lib.ptr(rgb), _lib.ptr(prof), int(prof.shape[0]), _lib.ptr(ids), self.seed, self.frame_offset,
                                              call, _lib.ptr(out), _OUT_DTYPES[self.dtype], self.num_frames, int(rgb.shape[1]),
                                              int(rgb.shape[2]), _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_camera_model")
        return out
