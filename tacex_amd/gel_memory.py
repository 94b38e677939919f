"""Gel memory: the viscoelastic residual imprint of the elastomer on the optical path, per env (`tacex_gel_memory`,
tacex_amd/csrc/gel_memory.hip; the contract is the comment of that call in include/tacex_hip.h).

A GelSight pad takes tens to hundreds of milliseconds to come back after an indenter lifts off or rolls away; the camera sees a fading
imprint meanwhile.  The model keeps K Prony branches of per-pixel state and rewrites the height map of every step in place, upstream of
everything that reads it (`tactile_rgb`, `indentation_depth`, `contact_field()`, `lens_image()`, `camera_image()`).

    gels = [GelMemoryProfile(tau_s=(0.05, 0.4), weight=(0.5, 0.2)), GelMemoryProfile(tau_s=(0.12, 0.0), weight=(0.6, 0.0))]
    memory = TactileGelMemory(num_envs, (320, 240), gels, terms=2, dt=1 / 60, device="cuda:0")
    memory.randomize()                       # at reset: a gel per env, drawn on the device
    sensor.set_gel_memory(memory)            # every update now leaves the imprint in data.output["height_map"]

An env's map depends on its own history and profile alone, and a run is reproducible bit for bit."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _stage


def rest_plane_mm(gelpad_height: float, gelpad_to_camera_min_distance: float) -> float:
    """z0 of the contract: float32((gelpad_to_camera_min_distance + gelpad_height) * 1000), sum and product in double."""
    return float(np.float32((float(gelpad_to_camera_min_distance) + float(gelpad_height)) * 1000.0))


@dataclass
class GelMemoryProfile:
    """One elastomer: time constants `tau_s` = (t1, t2) [s] and weights `weight` = (w1, w2) of the two Prony branches (the second
    pair is ignored by a model with terms=1), and `floor_mm`: a released pixel's branch below it is set to exactly zero.
    A branch follows the penetration d with m' = a m + (1 - a) w d, a = exp(-dt / tau) (tau == 0: a = 0, the branch shows w d at once
    and forgets at once).  w1 + w2 <= 1: the imprint is never deeper than the deepest past press."""

    tau_s: object = (0.05, 0.0)
    weight: object = (0.5, 0.0)
    floor_mm: float = 1e-4

    @classmethod
    def zero(cls) -> "GelMemoryProfile":
        """No memory at all: the height map passes unchanged."""
        return cls(tau_s=(0.0, 0.0), weight=(0.0, 0.0), floor_mm=0.0)

    def validate(self):
        tau, w = np.asarray(self.tau_s, dtype=np.float64), np.asarray(self.weight, dtype=np.float64)
        if tau.shape != (2,) or w.shape != (2,):
            raise ValueError(f"GelMemoryProfile: tau_s and weight must be 2 values each, got shapes {tau.shape}, {w.shape}")
        if not (np.isfinite(tau).all() and np.isfinite(w).all() and math.isfinite(float(self.floor_mm))):
            raise ValueError("GelMemoryProfile: values must be finite")
        if (tau < 0).any():
            raise ValueError(f"GelMemoryProfile: tau_s must be >= 0, got {tuple(tau)}")
        if (w < 0).any():
            raise ValueError(f"GelMemoryProfile: weight must be >= 0, got {tuple(w)}")
        if w.sum() > 1.0:
            raise ValueError(f"GelMemoryProfile: w1 + w2 must be <= 1, got {w.sum()}")
        if float(self.floor_mm) < 0:
            raise ValueError(f"GelMemoryProfile: floor_mm must be >= 0, got {self.floor_mm}")
        return tau, w

    def row(self, dt: float) -> np.ndarray:
        """The (8,) float32 row [a1, c1, a2, c2, floor_mm, 0, 0, 0] of `tacex_gel_memory`'s coefficient table for a step of `dt`
        seconds: a_k = exp(-dt / tau_k) (0 when tau_k == 0), c_k = (1 - a_k) w_k, in float64, then rounded."""
        tau, w = self.validate()
        dt = float(dt)
        if not (math.isfinite(dt) and dt > 0):
            raise ValueError(f"GelMemoryProfile: dt must be > 0, got {dt}")
        row = np.zeros(8, dtype=np.float64)
        for k in range(2):
            a = math.exp(-dt / tau[k]) if tau[k] > 0 else 0.0
            row[2 * k], row[2 * k + 1] = a, (1.0 - a) * w[k]
        row[4] = float(self.floor_mm)
        return row.astype(np.float32)


class TactileGelMemory:
    """The gel memory of `num_envs` frames of `resolution` = (width, height) pixels (the sensor's camera resolution).  It owns the
    state (num_envs, terms, H, W) float32, the live flags (num_envs,) int32, the coefficient table (P, 8) float32 and `profile_ids`
    (num_envs,) int32 - device tensors; the ids may be written in place (at reset) or re-drawn with `randomize()`; an id outside
    [0, P) is the all-zero profile.  The table is rebuilt only when `dt` or `profiles` is assigned."""

    coefficients, profile_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

    def __init__(self, num_envs: int, resolution, profiles, terms: int = 1, dt: float = 1.0 / 60.0, device="cuda:0"):
        if int(num_envs) <= 0:
            raise ValueError(f"TactileGelMemory: num_envs = {num_envs}")
        if int(terms) not in (1, 2):
            raise ValueError(f"TactileGelMemory: terms = {terms} (must be 1 or 2)")
        W, H = int(resolution[0]), int(resolution[1])
        if W <= 0 or H <= 0:
            raise ValueError(f"TactileGelMemory: resolution = {tuple(resolution)}")
        self._profiles = self._checked(profiles)
        self._lib, self._table = _stage.open_stage("TactileGelMemory", "coefficients", "profile_ids", self._profiles, GelMemoryProfile,
                                                   num_envs, device, row=lambda p: p.row(dt))
        self.device = torch.device(device)
        self.num_envs, self.terms, self.height, self.width = int(num_envs), int(terms), H, W
        self._dt = float(dt)
        self.state = torch.zeros((self.num_envs, self.terms, H, W), dtype=torch.float32, device=self.device)
        self.live = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)

    @staticmethod
    def _checked(profiles):
        profiles = _stage.profile_list("TactileGelMemory", "profiles", profiles, GelMemoryProfile)
        for p in profiles:
            p.validate()
        return profiles

    @staticmethod
    def coefficient_table(profiles, dt: float) -> np.ndarray:
        """(P, 8) float32: `GelMemoryProfile.row(dt)` of every profile."""
        return np.stack([p.row(dt) for p in profiles])

    def _rebuild(self):
        self._table.assign(self.coefficient_table(self._profiles, self._dt))  # (same storage when P stays: see ProfileTable.assign)

    @property
    def dt(self) -> float:
        return self._dt

    @dt.setter
    def dt(self, value: float):
        value = float(value)
        if not (math.isfinite(value) and value > 0):
            raise ValueError(f"TactileGelMemory: dt must be > 0, got {value}")
        if value != self._dt:
            self._dt = value
            self._rebuild()

    @property
    def profiles(self):
        return tuple(self._profiles)

    @profiles.setter
    def profiles(self, profiles):
        self._profiles = self._checked(profiles)
        self._rebuild()

    @property
    def num_profiles(self) -> int:
        return len(self._profiles)

    def randomize(self, env_ids=None, generator=None):
        """Re-draw the profile ids of `env_ids` (default: all) uniformly from [0, P) on the device."""
        return self._table.randomize(env_ids, generator)

    def reset(self, env_ids=None):
        """Zero the state and the live flag of `env_ids` (default: all); the other envs keep their imprint."""
        if env_ids is None or isinstance(env_ids, slice):
            sel = slice(None) if env_ids is None else env_ids
        else:
            sel = torch.as_tensor(env_ids, dtype=torch.long, device=self.device)
        self.state[sel] = 0
        self.live[sel] = 0

    def imprint(self) -> torch.Tensor:
        """M = sum of the branch states [mm], (num_envs, H, W): how far below its rest plane the gel still stands (a read-out)."""
        return self.state[:, 0].clone() if self.terms == 1 else self.state[:, 0] + self.state[:, 1]

    def apply(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor, rows: torch.Tensor | None = None,
              gelpad_height: float = 0.0, gelpad_to_camera_min_distance: float = 0.0) -> torch.Tensor:
        """One launch on the current stream: `hm` (num_envs, H, W) float32 [mm] is rewritten in place and the state advances one
        step; `frame_min`, `indent` (num_envs,) float32 and `rows` (num_envs, 4) int32 (optional) receive what
        `tacex_indentation_depth` gives for the rewritten map."""
        B, K, H, W = self.state.shape
        dev = self._table.device

        def arg(name, t, shape, dtype=torch.float32):
            return _stage.check_tensor("TactileGelMemory", name, t, shape, dtype, dev)

        arg("hm", hm, (B, H, W))
        arg("frame_min", frame_min, (B,))
        arg("indent", indent, (B,))
        if rows is not None:
            arg("rows", rows, (B, 4), torch.int32)
        ids, coef = self._table.check()
        with torch.cuda.device(dev):
            rc = self._lib.tacex_gel_memory(_lib.ptr(hm), _lib.ptr(self.state), _lib.ptr(self.live), _lib.ptr(coef), int(coef.shape[0]),
                                            _lib.ptr(ids), rest_plane_mm(gelpad_height, gelpad_to_camera_min_distance),
                                            float(gelpad_height), float(gelpad_to_camera_min_distance), _lib.ptr(frame_min),
                                            _lib.ptr(indent), _lib.ptr(rows), B, H, W, K, _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_gel_memory")
        return hm
