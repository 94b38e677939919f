"""Scenes of volumetric parts: several posed signed-distance volumes per env, folded by union, subtraction and intersection during
the march, as a height-map source (`tacex_height_map_from_sdf_scene`, tacex_amd/csrc/sdf_scene.hip; the contract is the comment of
that call in include/tacex_hip.h).

`SdfVolumeSource` presses one object per env.  A finger on a peg AND the rim of its hole, a plate WITH a slot, a bolt turning in a
nut, two parts filleted together need several parts that move against each other every step, and subtraction, intersection and smooth
blends cannot be made from finished depth maps: the distance fields are combined at every step of every ray.

    from tacex_amd.utils import sdf_volumes
    src = SdfSceneSource([sdf_volumes.box((8, 6, 1)), sdf_volumes.sphere(1.5)], num_envs, "cuda:0", num_slots=2)
    src.set_part(0, volume_id=0, op="union")
    src.set_part(1, volume_id=1, op="subtract")           # a plate with a round hole
    src.set_pose(0, 160, 120, (1, 0, 0, 0), press_mm=0.6)
    src.set_pose(1, 160, 120, (1, 0, 0, 0), z_mm=28.2)
    sensor.set_height_map_source(src)
    src.set_group_pose(quat, t_mm)                         # each step: the assembly as one rigid body

The library (`voxels`, `volumes_i`, `volumes_f`) and `SdfVolume` are those of `volume_source`."""
from __future__ import annotations

import torch

from . import _lib, _stage
from .volume_source import SdfVolume, SdfVolumeSource, placement_rows

MAX_SLOTS = 8
OPS = {"union": 0, "subtract": 1, "intersect": 2}
POSE_FIELDS = ("r00", "r01", "r02", "r10", "r11", "r12", "r20", "r21", "r22", "tx", "ty", "tz", "scale", "level_mm", "blend_mm", "reserved1")


class SdfSceneSource(_stage.LibrarySource):
    """`num_slots` (1..8) posed volumes per env as the sensor's height-map source (`GelSightSensor.set_height_map_source`).  Besides
    the library of `SdfVolumeSource` it owns three tensors the caller writes in place between steps: `part_ids` (num_envs, K) int32
    (the slot's volume; an id outside [0, P) leaves the slot empty; initially -1), `part_ops` (num_envs, K) int32 (0 union,
    1 subtract, 2 intersect; anything else leaves the slot empty) and `part_pose` (num_envs, K, 16) float32 (`POSE_FIELDS`: R row-major
    object -> camera, t [mm], scale, level_mm, blend_mm; initially identity beyond the far clip).  The scene's field is a left fold
    over the slots: a union adds a part, a subtraction cuts it out of what the earlier slots built, an intersection keeps what both
    hold; `blend_mm` > 0 rounds the seam with a polynomial smooth minimum of that width.  `local_pose` keeps what `set_pose` wrote,
    for `set_group_pose`.  With `part_map=True` a fill also says which slot every pixel shows
    (`tacex_height_map_from_sdf_scene_parts`): `part_map`, a (num_envs, H, W) uint8 tensor of slot indices, 255 where nothing was
    hit - None before the first fill, allocated there and written in place afterwards; the height map and the other outputs keep
    their bits."""

    _owner, _unit, _names = "SdfSceneSource", "voxel", ("voxels", "volumes_i", "volumes_f", "_row_ids")
    volumes_f = _stage.table_attr("rows")
    surface_points = SdfVolumeSource.surface_points
    num_volumes = SdfVolumeSource.num_volumes

    def __init__(self, volumes, num_envs: int, device, num_slots: int = 2, pixmm: float = 0.0295, gel_top_mm: float = 28.5,
                 near_clip_mm: float = 24.0, far_clip_mm: float = 29.0, max_steps: int = 32, tol_mm: float = 1e-4, part_map: bool = False):
        volumes = _stage.profile_list("SdfSceneSource", "volumes", volumes, SdfVolume)
        grids = [v.validate() for v in volumes]
        if not 1 <= int(num_slots) <= MAX_SLOTS:
            raise ValueError(f"SdfSceneSource: num_slots = {num_slots} (must be 1..{MAX_SLOTS})")
        if not 1 <= int(max_steps) <= 128:
            raise ValueError(f"SdfSceneSource: max_steps = {max_steps} (must be 1..128)")
        if not float(tol_mm) > 0:
            raise ValueError(f"SdfSceneSource: tol_mm must be > 0, got {tol_mm}")
        if not float(near_clip_mm) < float(far_clip_mm):
            raise ValueError(f"SdfSceneSource: near_clip_mm = {near_clip_mm} must lie below far_clip_mm = {far_clip_mm}")
        self._open(volumes, SdfVolume, grids, [g.shape for g in grids], num_envs, device, pixmm)
        del self.pose  # (one pose per slot here: part_pose)
        self.volumes, self.max_steps, self.num_slots = tuple(volumes), int(max_steps), int(num_slots)
        self.gel_top_mm, self.tol_mm = float(gel_top_mm), float(tol_mm)
        self.near_clip_mm, self.far_clip_mm = float(near_clip_mm), float(far_clip_mm)
        self._surface_points = None
        self.with_part_map, self.part_map = bool(part_map), None
        B, K, dev = self.num_envs, self.num_slots, self.device
        self.part_ids = torch.full((B, K), -1, dtype=torch.int32, device=dev)
        self.part_ops = torch.zeros((B, K), dtype=torch.int32, device=dev)
        self.part_pose = torch.zeros((B, K, 16), dtype=torch.float32, device=dev)
        self.part_pose[:, :, 0] = self.part_pose[:, :, 4] = self.part_pose[:, :, 8] = self.part_pose[:, :, 12] = 1.0  # (identity R, scale 1)
        self.part_pose[:, :, 11] = 2.0 * self.far_clip_mm  # (until set_pose: beyond far clip)
        self.local_pose = self.part_pose.clone()

    def _slot(self, slot) -> int:
        if not 0 <= int(slot) < self.num_slots:
            raise ValueError(f"SdfSceneSource: slot = {slot} (the scene has slots 0..{self.num_slots - 1})")
        return int(slot)

    def set_part(self, slot: int, volume_id=None, op=None, env_ids=slice(None)):
        """The volume (an int or a per-env tensor; None: as it is) and the operation ("union", "subtract", "intersect" or 0, 1, 2;
        None: as it is) of `slot` in `env_ids` (default: all)."""
        slot = self._slot(slot)
        if volume_id is not None:
            self.part_ids[env_ids, slot] = torch.as_tensor(volume_id, dtype=torch.int32, device=self.device)
        if op is not None:
            if isinstance(op, str) and op not in OPS:
                raise ValueError(f"SdfSceneSource.set_part: op = {op!r} (one of {', '.join(OPS)})")
            self.part_ops[env_ids, slot] = torch.as_tensor(OPS[op] if isinstance(op, str) else op, dtype=torch.int32, device=self.device)

    def set_pose(self, slot: int, cx_px, cy_px, quat_wxyz, press_mm=None, z_mm=None, scale=1.0, level_mm=0.0, blend_mm=0.0,
                 env_ids=slice(None)):
        """Place the part in `slot` of `env_ids` (default: all) as `SdfVolumeSource.set_pose` places its volume (one copy of the
        math: `volume_source.placement_rows`), with the seam's blend width `blend_mm`.  The rows go to `part_pose` and to `local_pose`,
        from which `set_group_pose` moves the assembly.  Torch ops on the device, no host sync."""
        slot = self._slot(slot)
        if (press_mm is None) == (z_mm is None):
            raise ValueError("SdfSceneSource.set_pose: give exactly one of press_mm and z_mm")
        ids = self.part_ids[env_ids, slot].long().clamp(0, self.num_volumes - 1)
        rows = placement_rows(self, ids, cx_px, cy_px, quat_wxyz, press_mm, z_mm, scale, level_mm, blend_mm)
        self.part_pose[env_ids, slot] = rows
        self.local_pose[env_ids, slot] = rows

    def set_group_pose(self, quat_wxyz, t_mm, env_ids=slice(None)):
        """Move the assembly of `env_ids` (default: all) as one rigid body: `part_pose` = T o `local_pose` for every slot, with T the
        rotation `quat_wxyz` (camera frame; normalised here; a tuple or an (n, 4) tensor) followed by the translation `t_mm` [mm] (a
        triple or (n, 3)): R = R_T R_local, t = R_T t_local + t_T in float64, every sum left to right; scale, level and blend stay.
        Torch ops on the device, no host sync."""
        dev = self.device
        local = self.local_pose[env_ids].double()  # (n, K, 16)
        n = local.shape[0]
        as64 = lambda v: v.to(device=dev, dtype=torch.float64) if isinstance(v, torch.Tensor) else torch.tensor(  # noqa: E731
            [float(c) for c in v], dtype=torch.float64, device=dev)
        q, t = as64(quat_wxyz), as64(t_mm)
        q = q.expand(n, 4) if q.dim() == 1 else q
        t = t.expand(n, 3) if t.dim() == 1 else t
        w, x, y, z = q.unbind(1)
        q = q / torch.sqrt(w * w + x * x + y * y + z * z)[:, None]
        w, x, y, z = (c[:, None] for c in q.unbind(1))
        T = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        out = local.clone()
        for i in range(3):
            for j in range(3):
                out[:, :, 3 * i + j] = T[i][0] * local[:, :, j] + T[i][1] * local[:, :, 3 + j] + T[i][2] * local[:, :, 6 + j]
            out[:, :, 9 + i] = T[i][0] * local[:, :, 9] + T[i][1] * local[:, :, 10] + T[i][2] * local[:, :, 11] + t[:, i, None]
        self.part_pose[env_ids] = out.float()

    def randomize(self, slot=None, env_ids=None, generator=None):
        """Re-draw the volume ids of `slot` (default: every slot) in `env_ids` (default: all) uniformly from [0, P) on the device;
        returns `part_ids`."""
        slots = slice(None) if slot is None else slice(self._slot(slot), self._slot(slot) + 1)
        width = self.num_slots if slot is None else 1
        n = self.num_envs if env_ids is None else len(env_ids)
        ids = torch.randint(0, self.num_volumes, (n, width), dtype=torch.int32, device=self.device, generator=generator)
        if env_ids is None:
            self.part_ids[:, slots] = ids
        else:
            self.part_ids[torch.as_tensor(env_ids, dtype=torch.long, device=self.device), slots] = ids
        return self.part_ids

    def _check_pose(self, arg):
        B, K = self.num_envs, self.num_slots
        arg("part_pose", self.part_pose, (B, K, 16), must="must stay")
        arg("part_ids", self.part_ids, (B, K), torch.int32, must="must stay")
        arg("part_ops", self.part_ops, (B, K), torch.int32, must="must stay")

    def _launch(self, voxels, volumes_i, volumes_f, ids, hm, frame_min, indent, rows, gelpad_height, gelpad_to_camera_min_distance):
        dev = self.device
        head = (_lib.ptr(voxels), int(voxels.shape[0]), _lib.ptr(volumes_i), _lib.ptr(volumes_f), self.num_volumes, _lib.ptr(self.part_ids),
                _lib.ptr(self.part_pose), _lib.ptr(self.part_ops), self.num_slots, self.pixmm, self.near_clip_mm, self.far_clip_mm,
                self.max_steps, self.tol_mm, gelpad_height, gelpad_to_camera_min_distance, _lib.ptr(hm), _lib.ptr(frame_min),
                _lib.ptr(indent), _lib.ptr(rows))
        tail = (self.num_envs, int(hm.shape[1]), int(hm.shape[2]), _lib.current_stream_handle(dev))
        name = "tacex_height_map_from_sdf_scene"
        if self.with_part_map:
            name += "_parts"
            if self.part_map is None or self.part_map.shape != hm.shape:  # (the first fill; a fill at another resolution)
                self.part_map = torch.empty(tuple(hm.shape), dtype=torch.uint8, device=dev)
            _stage.check_tensor(self._owner, "part_map", self.part_map, tuple(hm.shape), torch.uint8, dev, must="must stay")
            head += (_lib.ptr(self.part_map),)
        with torch.cuda.device(dev):  # (two launches: the march, then the frame outputs of the map)
            rc = getattr(self._lib, name)(*head, *tail)
        _lib.check(rc, name)


def part_slip(part_pose: torch.Tensor, reference_pose: torch.Tensor, pixmm: float) -> torch.Tensor:
    """The (B, K, 5) slip table [dx_mm, dy_mm, dtheta_rad, cx_px, cy_px] of `TactileContactModel.parts` from two (B, K, 16) pose tensors
    (`POSE_FIELDS`): per slot the in-plane translation of the part's origin since `reference_pose` [mm], the yaw of R R_ref^T about
    the optical axis, atan2(M[1][0] - M[0][1], M[0][0] + M[1][1]) - the in-plane rotation nearest to M; a tilt alone turns nothing -,
    and the origin's current pixel as the twist centre.  A task snapshots `SdfSceneSource.part_pose` at first contact
    (`reference_pose = src.part_pose.clone()`) and calls this every step.  Torch ops on the poses' device, no host sync."""
    for name, t in (("part_pose", part_pose), ("reference_pose", reference_pose)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 16:
            raise ValueError(f"part_slip: {name} must be a (B, K, 16) tensor")
    if part_pose.shape != reference_pose.shape:
        raise ValueError(f"part_slip: part_pose is {tuple(part_pose.shape)}, reference_pose {tuple(reference_pose.shape)}")
    if not float(pixmm) > 0:
        raise ValueError(f"part_slip: pixmm must be > 0, got {pixmm}")
    p, q = part_pose.double(), reference_pose.to(part_pose.device).double()
    # M = R R_ref^T: M[i][j] = sum_k R[i][k] R_ref[j][k] (rows 0 and 1 suffice)
    m = lambda i, j: p[..., 3 * i] * q[..., 3 * j] + p[..., 3 * i + 1] * q[..., 3 * j + 1] + p[..., 3 * i + 2] * q[..., 3 * j + 2]  # noqa: E731
    yaw = torch.atan2(m(1, 0) - m(0, 1), m(0, 0) + m(1, 1))
    out = torch.stack((p[..., 9] - q[..., 9], p[..., 10] - q[..., 10], yaw, p[..., 9] / float(pixmm), p[..., 10] / float(pixmm)), dim=-1)
    return out.float().contiguous()
