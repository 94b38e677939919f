"""Contact point cloud of the optical path: a fixed-size set of surface points per env, sampled from the contact pixels of the height
map (`tacex_contact_points`, tacex_amd/csrc/contact_points.hip; the contract is that function's comment in include/tacex_hip.h).

    model = TactileContactPoints(num_frames=num_envs, device="cuda:0", max_points=1024, pixmm=0.0295, unit=1e-3, seed=7)
    model.pose[:, [3, 7, 11]] = sensor_position_in_world      # optional: [R | t] per env, written in place
    cloud = sensor.contact_points(model)                       # one launch after the sensor's update, no host synchronisation
    cloud.points, cloud.normals, cloud.depth, cloud.valid      # (B,K,3), (B,K,3), (B,K), (B,K)

The contact pixels of a frame are ranked in row-major order and K of them taken at evenly spaced ranks (all of them, padded, when
there are at most K): the patch as 3-D points in the camera frame of `ContactField`, with the indenter surface's normal, the
penetration, the pixel and its label."""
from __future__ import annotations

import math

import torch

from . import _lib, _stage

MAX_POINTS = 16384  # TACEX_CONTACT_POINTS_MAX
_PADS = {"zero": 0, "repeat": 1}


class ContactPoints:
    """What one call of a `TactileContactPoints` returns: `points` (B,K,3) float32, `normals` (B,K,3) float32 or None, `depth` (B,K)
    float32 [mm], `pixels` (B,K,2) int32 [row, col], `labels` (B,K) uint8 and `count` (B,2) int32 [contact pixels, valid slots].
    Invalid slots hold zeros, pixel -1 and label 255.  The tensors are the MODEL's buffers: the next call overwrites them."""

    def __init__(self, points, normals, depth, pixels, labels, count):
        self.points, self.normals, self.depth, self.pixels, self.labels, self.count = points, normals, depth, pixels, labels, count

    @property
    def num_contact(self) -> torch.Tensor:
        """(B,) int32: contact pixels of the frame (N)."""
        return self.count[:, 0]

    @property
    def num_valid(self) -> torch.Tensor:
        """(B,) int32: valid slots (V); they are the first V."""
        return self.count[:, 1]

    @property
    def valid(self) -> torch.Tensor:
        """(B,K) bool: slot k holds a point.  A torch op on `count` (no synchronisation)."""
        return torch.arange(self.points.shape[1], device=self.count.device, dtype=torch.int32)[None, :] < self.count[:, 1:2]


class TactileContactPoints:
    """The point-cloud stage of `num_frames` envs.  `max_points` K slots per env; `pixmm`: pixel pitch of the height map [mm];
    `min_depth_mm`: a pixel counts when it is pressed deeper than this; `pad`: what the slots beyond the contact pixels hold when
    there are fewer than K - "zero" (invalid slots) or "repeat" (the points again, in order); `unit`: factor from mm to the unit of the
    points (1e-3: metres); `normals` False leaves them out; `seed` None: the subsample starts at rank 0, otherwise at a rank drawn per
    env and call (Philox, addressed by `seed`, `frame_offset` + env and the running `call` counter, as in `TactileCameraModel`).
    `pose` (num_frames,12) float32 on the device, a row-major [R | t] per env initialised to identity, maps the points (after `unit`)
    and rotates the normals; the caller writes it in place, `model.pose = None` leaves the points in the camera frame."""

    def __init__(self, num_frames: int, device, max_points: int = 1024, pixmm: float = 0.0295, min_depth_mm: float = 0.0, pad: str = "zero",
                 unit: float = 1.0, normals: bool = True, seed: int | None = None, frame_offset: int = 0):
        own = "TactileContactPoints"
        if int(num_frames) <= 0:
            raise ValueError(f"{own}: num_frames = {num_frames}")
        if not 1 <= int(max_points) <= MAX_POINTS:
            raise ValueError(f"{own}: max_points = {max_points} (must be 1..{MAX_POINTS})")
        if not (math.isfinite(float(pixmm)) and float(pixmm) > 0):
            raise ValueError(f"{own}: pixmm = {pixmm}")
        if not (math.isfinite(float(min_depth_mm)) and float(min_depth_mm) >= 0):
            raise ValueError(f"{own}: min_depth_mm = {min_depth_mm} (must be >= 0)")
        if pad not in _PADS:
            raise ValueError(f"{own}: pad = {pad!r} (must be 'zero' or 'repeat')")
        if not (math.isfinite(float(unit)) and float(unit) > 0):
            raise ValueError(f"{own}: unit = {unit}")
        if seed is not None and not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"{own}: seed must fit 64 bits")
        if not -2 ** 63 <= int(frame_offset) <= 2 ** 63 - int(num_frames):
            raise ValueError(f"{own}: frame_offset + num_frames must fit 64 bits (signed)")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.TacexHipError(f"{own} runs on the GPU only (device {device}): there is no CPU fallback")
        self._lib = _lib.load_library()
        B, K = int(num_frames), int(max_points)
        self.num_frames, self.max_points = B, K
        self.pixmm, self.min_depth_mm, self.pad, self.unit = float(pixmm), float(min_depth_mm), pad, float(unit)
        self.seed = None if seed is None else int(seed)
        self.frame_offset = int(frame_offset)
        self.call = 0
        self.pose = torch.eye(3, 4, dtype=torch.float32, device=device).reshape(1, 12).repeat(B, 1)
        self.device = self.pose.device  # (with its index: what a tensor's .device compares equal to)
        self._points = torch.zeros((B, K, 3), dtype=torch.float32, device=device)
        self._normals = torch.zeros((B, K, 3), dtype=torch.float32, device=device) if normals else None
        self._depth = torch.zeros((B, K), dtype=torch.float32, device=device)
        self._pixels = torch.full((B, K, 2), -1, dtype=torch.int32, device=device)
        self._labels = torch.full((B, K), 255, dtype=torch.uint8, device=device)
        self._count = torch.zeros((B, 2), dtype=torch.int32, device=device)

    def __call__(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor, frame_rows: torch.Tensor | None = None,
                 labels: torch.Tensor | None = None, label: int = -1) -> ContactPoints:
        """One launch on the current stream.  `hm` (num_frames,H,W) float32 [mm], contiguous, on the model's device; `frame_min`,
        `indent` (num_frames,) float32 as the sensor's depth pass leaves them; `frame_rows` (num_frames,4) int32 contact rectangles of
        THESE height maps or None; `labels` (num_frames,H,W) uint8 or None; `label` -1: every pixel, 0..254: the pixels of that label.
        The output buffers are allocated once, in the constructor, and every call writes the same ones: a captured graph keeps
        pointing at them, and a result that must outlive the next call has to be cloned."""
        own, B, dev = "TactileContactPoints", self.num_frames, self.device

        def arg(name, t, shape, dtype=torch.float32, must="must be"):
            return _stage.check_tensor(own, name, t, shape, dtype, dev, must=must)

        arg("hm", hm, (B, "H", "W"))
        H, W = int(hm.shape[1]), int(hm.shape[2])
        arg("frame_min", frame_min, (B,))
        arg("indent", indent, (B,))
        if frame_rows is not None:
            arg("frame_rows", frame_rows, (B, 4), torch.int32)
        if labels is not None:
            arg("labels", labels, (B, H, W), torch.uint8)
        if not -1 <= int(label) <= 254:
            raise ValueError(f"{own}: label = {label} (must be -1 or 0..254)")
        if int(label) >= 0 and labels is None:
            raise ValueError(f"{own}: label = {label} needs labels")
        if self.pose is not None:
            arg("pose", self.pose, (B, 12), must="must stay")
        call = 0
        if self.seed is not None:
            call = self.call
            self.call = (self.call + 1) & 0xFFFFFFFF
        with torch.cuda.device(dev):
            rc = self._lib.tacex_contact_points(_lib.ptr(hm), _lib.ptr(frame_min), _lib.ptr(indent), _lib.ptr(frame_rows), _lib.ptr(labels),
                                                int(label), self.pixmm, self.min_depth_mm, self.max_points, _PADS[self.pad],
                                                _lib.ptr(self.pose), self.unit, int(self.seed is not None), self.seed or 0,
                                                self.frame_offset, call, _lib.ptr(self._points), _lib.ptr(self._normals),
                                                _lib.ptr(self._depth), _lib.ptr(self._pixels), _lib.ptr(self._labels), _lib.ptr(self._count),
                                                B, H, W, _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_contact_points")
        return ContactPoints(self._points, self._normals, self._depth, self._pixels, self._labels, self._count)
