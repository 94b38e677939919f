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

from . import _lib

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

    def __init__(self, profiles, num_frames: int, device, seed: int = 0, dtype: torch.dtype = torch.uint8, frame_offset: int = 0):
        if isinstance(profiles, CameraProfile):
            profiles = [profiles]
        rows = [p.row() if isinstance(p, CameraProfile) else None for p in profiles]
        if not rows or any(r is None for r in rows):
            raise ValueError("TactileCameraModel: profiles must be a non-empty sequence of CameraProfile")
        if dtype not in _OUT_DTYPES:
            raise ValueError(f"TactileCameraModel: dtype must be torch.uint8 or torch.float32, got {dtype}")
        if int(num_frames) <= 0:
            raise ValueError(f"TactileCameraModel: num_frames = {num_frames}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("TactileCameraModel: seed must fit 64 bits")
        if not 0 <= int(frame_offset) <= 2 ** 32 - int(num_frames):
            raise ValueError("TactileCameraModel: frame_offset + num_frames must fit 32 bits")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.TacexHipError(f"TactileCameraModel runs on the GPU only (device {self.device}): there is no CPU fallback")
        self._lib = _lib.load_library()
        self.num_frames = int(num_frames)
        self.seed = int(seed)
        self.dtype = dtype
        self.frame_offset = int(frame_offset)
        self.call = 0
        self.profiles = torch.from_numpy(np.stack(rows)).to(self.device)
        self.profile_ids = torch.zeros(self.num_frames, dtype=torch.int32, device=self.device)

    @property
    def num_profiles(self) -> int:
        return int(self.profiles.shape[0])

    def randomize(self, env_ids=None, generator=None):
        """Re-draw the profile ids of `env_ids` (default: all) uniformly from [0, P) on the device."""
        n = self.num_frames if env_ids is None else len(env_ids)
        ids = torch.randint(0, self.num_profiles, (n,), dtype=torch.int32, device=self.device, generator=generator)
        if env_ids is None:
            self.profile_ids.copy_(ids)
        else:
            self.profile_ids[torch.as_tensor(env_ids, dtype=torch.long, device=self.device)] = ids
        return self.profile_ids

    def __call__(self, rgb: torch.Tensor, out: torch.Tensor | None = None, call: int | None = None) -> torch.Tensor:
        """One launch on the current stream.  `rgb` (num_frames,H,W,3) float32, contiguous, on the model's device; `out` of the same
        shape and the model's dtype (float32 may be `rgb` itself), allocated when None.  `call` overrides the running counter."""
        if not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.shape[0] != self.num_frames or rgb.shape[3] != 3:
            raise ValueError(f"TactileCameraModel: rgb must be a ({self.num_frames}, H, W, 3) tensor, got "
                             f"{tuple(rgb.shape) if isinstance(rgb, torch.Tensor) else type(rgb).__name__}")
        if rgb.dtype != torch.float32 or not rgb.is_contiguous() or rgb.shape[1] < 1 or rgb.shape[2] < 1:
            raise ValueError("TactileCameraModel: rgb must be float32, contiguous and non-empty")
        if rgb.device != self.profiles.device:
            raise _lib.TacexHipError(f"TactileCameraModel: rgb is on {rgb.device}, the model on {self.profiles.device} (no CPU fallback)")
        if out is None:
            out = torch.empty(rgb.shape, dtype=self.dtype, device=rgb.device)
        elif (not isinstance(out, torch.Tensor) or out.shape != rgb.shape or out.dtype != self.dtype or not out.is_contiguous()
              or out.device != rgb.device):
            raise ValueError(f"TactileCameraModel: out must be a contiguous {tuple(rgb.shape)} {self.dtype} tensor on {rgb.device}")
        ids, prof = self.profile_ids, self.profiles
        if ids.dtype != torch.int32 or tuple(ids.shape) != (self.num_frames,) or not ids.is_contiguous() or ids.device != rgb.device:
            raise ValueError(f"TactileCameraModel: profile_ids must stay a ({self.num_frames},) int32 tensor on {rgb.device}")
        if prof.dtype != torch.float32 or prof.dim() != 2 or prof.shape[1] != 16 or not prof.is_contiguous() or prof.device != rgb.device:
            raise ValueError(f"TactileCameraModel: profiles must stay a (P, 16) float32 tensor on {rgb.device}")
        if call is None:
            call = self.call
            self.call = (self.call + 1) & 0xFFFFFFFF
        elif not 0 <= int(call) < 2 ** 32:
            raise ValueError("TactileCameraModel: call must fit 32 bits")
        with torch.cuda.device(rgb.device):
            rc = self._lib.tacex_camera_model(_lib.ptr(rgb), _lib.ptr(prof), int(prof.shape[0]), _lib.ptr(ids), self.seed, self.frame_offset,
                                              int(call), _lib.ptr(out), _OUT_DTYPES[self.dtype], self.num_frames, int(rgb.shape[1]),
                                              int(rgb.shape[2]), _lib.current_stream_handle(rgb.device))
        _lib.check(rc, "tacex_camera_model")
        return out
