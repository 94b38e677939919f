"""What the per-env stages of the optical path share (camera_model, lens_model, contact_field, gel_memory): the profile table with
its ids, the check of a tensor argument, and the constructor preamble.  A stage keeps its own profile class, its own arguments and
its one launch; DESIGN.md 4.0.12a.4 says how a new stage uses these pieces.  `LibrarySource` is the base of the height-map sources
that press one entry of a library per env (relief_source, volume_source) or several (sdf_scene)."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib


def check_tensor(owner: str, name: str, t, shape, dtype, device, must: str = "must be", on_device=_lib.TacexHipError):
    """`t` as a launch needs it, or an exception naming `owner` and `name`.  A str in `shape` is a free dimension >= 1.  Not a
    tensor, another shape or dtype, not contiguous: ValueError; then a tensor on another device than `device`: `on_device`."""
    ok = isinstance(t, torch.Tensor) and t.dim() == len(shape) and all(
        n >= 1 if isinstance(want, str) else n == want for n, want in zip(t.shape, shape))
    if not ok or t.dtype != dtype or not t.is_contiguous():
        want = "(" + ", ".join(str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{owner}: {name} {must} a contiguous {want} {dtype} tensor, got {got}")
    if t.device != device:
        raise on_device(f"{owner}: {name} is on {t.device}, the model on {device} (no CPU fallback)")
    return t


class ProfileTable:
    """`rows` (P, C) float32 and `ids` (num_frames,) int32 on one device: the library of a stage and which row each env uses.  Both
    are plain tensors the caller may write in place; `check()` before a launch refuses what the kernels cannot take."""

    def __init__(self, owner: str, rows_name: str, ids_name: str, rows, num_frames: int, device):
        self.owner, self.rows_name, self.ids_name = owner, rows_name, ids_name
        self.num_frames = int(num_frames)
        self.ids = torch.zeros(self.num_frames, dtype=torch.int32, device=device)
        self.device = self.ids.device  # (with its index: what a tensor's .device compares equal to)
        self.rows = None
        self.assign(rows)
        self.width = int(self.rows.shape[1])

    def assign(self, rows):
        """New rows: copied into the storage there is when the shape stays (a captured graph keeps pointing at it)."""
        rows = torch.as_tensor(rows, dtype=torch.float32)
        if self.rows is not None and self.rows.shape == rows.shape:
            self.rows.copy_(rows)
        else:
            self.rows = rows.to(self.device, copy=True)  # (its own storage on a CPU device too)

    def randomize(self, env_ids=None, generator=None) -> torch.Tensor:
        """Re-draw the ids of `env_ids` (default: all) uniformly from [0, P) on the device; returns the id tensor."""
        n = self.num_frames if env_ids is None else len(env_ids)
        ids = torch.randint(0, int(self.rows.shape[0]), (n,), dtype=torch.int32, device=self.device, generator=generator)
        if env_ids is None:
            self.ids.copy_(ids)
        else:
            self.ids[torch.as_tensor(env_ids, dtype=torch.long, device=self.device)] = ids
        return self.ids

    def check(self):
        """(ids, rows) for a launch."""
        check_tensor(self.owner, self.ids_name, self.ids, (self.num_frames,), torch.int32, self.device, must="must stay")
        check_tensor(self.owner, self.rows_name, self.rows, ("P", self.width), torch.float32, self.device, must="must stay")
        return self.ids, self.rows


class table_attr:
    """A model's public name for `rows` or `ids` of its `_table` (read and assigned like the plain attribute it was)."""

    def __init__(self, field: str):
        self.field = field

    def __get__(self, obj, objtype=None):
        return self if obj is None else getattr(obj._table, self.field)

    def __set__(self, obj, value):
        setattr(obj._table, self.field, value)


def profile_list(owner: str, name: str, profiles, cls) -> list:
    """One `cls` or a sequence of them -> a non-empty list."""
    profiles = [profiles] if isinstance(profiles, cls) else list(profiles)
    if not profiles or not all(isinstance(p, cls) for p in profiles):
        raise ValueError(f"{owner}: {name} must be a non-empty sequence of {cls.__name__}")
    return profiles


def open_stage(owner: str, rows_name: str, ids_name: str, profiles, cls, num_frames: int, device, row=lambda p: p.row()):
    """The end of a stage's constructor, after its own arguments: profiles -> rows, num_frames, the device (a stage runs on the
    GPU only), the library.  Returns (library, ProfileTable); every ValueError comes before the device is looked at."""
    rows = np.stack([row(p) for p in profile_list(owner, rows_name, profiles, cls)])
    if int(num_frames) <= 0:
        raise ValueError(f"{owner}: num_frames = {num_frames}")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.TacexHipError(f"{owner} runs on the GPU only (device {device}): there is no CPU fallback")
    return _lib.load_library(), ProfileTable(owner, rows_name, ids_name, rows, num_frames, device)


def per_env(v, n: int, device) -> torch.Tensor:
    """A scalar or per-env tensor argument of a `set_pose` as (n,) float64 on `device`."""
    v = v.to(device=device, dtype=torch.float64) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64, device=device)
    return v.expand(n) if v.dim() == 0 else v


class LibrarySource:
    """A height-map source (`GelSightSensor.set_height_map_source`) that presses one entry of a library per env under a pose the caller
    writes in place: a payload tensor (all entries back to back), an int32 table (P, 4) whose first column is an entry's first payload
    element, a float32 table (P, C) and ids (num_envs,) in a `ProfileTable`, and `pose` (num_envs, 16) float32.  A subclass keeps its
    profile class, its public names for the four tensors (`_names`; the float table and the ids as `table_attr`), its own constructor
    checks, `set_pose` and `_launch`, the one call into the library."""

    writes_frame_rows = True  # fill(..., rows=) leaves the contact ranges of tacex_indentation_depth behind
    _owner = None  # the class name in messages
    _names = None  # attribute names (payload, int table, float table, ids)
    _unit = None   # what the payload counts ("texel", "voxel")

    def _open(self, profiles, cls, arrays, int_rows, num_envs: int, device, pixmm: float):
        """The end of the constructor, after the subclass's own checks: `arrays` are the entries' payloads, `int_rows` what follows
        the first payload element in each row of the int table.  Every ValueError comes before the device is looked at."""
        payload, table_i, rows_name, ids_name = self._names
        if not (math.isfinite(float(pixmm)) and float(pixmm) > 0):
            raise ValueError(f"{self._owner}: pixmm must be > 0, got {pixmm}")
        if sum(a.size for a in arrays) >= 2 ** 31:
            raise ValueError(f"{self._owner}: the library holds 2^31 {self._unit}s or more ({self._unit} indices are 32-bit)")
        self._lib, self._table = open_stage(self._owner, rows_name, ids_name, profiles, cls, num_envs, device)
        self.device = self._table.device
        self.num_envs, self.pixmm = int(num_envs), float(pixmm)
        self._num_profiles = len(profiles)
        first = np.concatenate([[0], np.cumsum([a.size for a in arrays])[:-1]])
        setattr(self, table_i, torch.tensor([[int(f), *r] for f, r in zip(first, int_rows)], dtype=torch.int32, device=self.device))
        setattr(self, payload, torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(self.device))
        self.pose = torch.zeros((self.num_envs, 16), dtype=torch.float32, device=self.device)

    def randomize(self, env_ids=None, generator=None):
        """Re-draw the library ids of `env_ids` (default: all) uniformly from [0, P) on the device."""
        return self._table.randomize(env_ids, generator)

    def fill(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor | None, gelpad_height: float,
             gelpad_to_camera_min_distance: float, rows: torch.Tensor | None = None):
        """hm (B, H, W) mm, frame_min (B,), indent (B,) or None, rows (B, 4) int32 or None - all written on the current stream;
        frame_min, indent and rows are what `tacex_indentation_depth` gives for the map."""
        B, P, dev = self.num_envs, self._num_profiles, self.device
        payload, table_i, rows_name, _ = self._names

        def arg(name, t, shape, dtype=torch.float32, must="must be"):
            return check_tensor(self._owner, name, t, shape, dtype, dev, must=must)

        arg("hm", hm, (B, "H", "W"))
        arg("frame_min", frame_min, (B,))
        if indent is not None:
            arg("indent", indent, (B,))
        if rows is not None:
            arg("rows", rows, (B, 4), torch.int32)
        self._check_pose(arg)
        ints = arg(table_i, getattr(self, table_i), (P, 4), torch.int32, must="must stay")
        data = arg(payload, getattr(self, payload), ("N",), must="must stay")
        ids, floats = self._table.check()
        arg(rows_name, floats, (P, self._table.width), must="must stay")
        self._launch(data, ints, floats, ids, hm, frame_min, indent, rows, float(gelpad_height), float(gelpad_to_camera_min_distance))
        return hm

    def _check_pose(self, arg):
        """The tensors the caller writes in place besides the ids, as `fill` needs them (a source with several poses per env has its own)."""
        arg("pose", self.pose, (self.num_envs, 16), must="must stay")

    def _launch(self, data, ints, floats, ids, hm, frame_min, indent, rows, gelpad_height, gelpad_to_camera_min_distance):
        raise NotImplementedError
