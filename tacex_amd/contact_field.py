"""Contact force field of the optical path: penalty contact from the height map (`tacex_contact_field`,
tacex_amd/csrc/contact_field.hip; the contract is that function's comment in include/tacex_hip.h).

    gels = [ContactGel.from_material(youngs=1.2e5, poisson=0.45, thickness_m=0.0045, mu=0.6), ContactGel(k_n=4e4, k_t=1.5e4, mu=0.9)]
    model = TactileContactModel(gels, num_frames=num_envs, device="cuda:0", pixmm=0.0295, grid=(9, 11))
    model.randomize()                      # at reset: a gel per env, drawn on the device
    field = sensor.contact_field(model)    # one launch after the sensor's update, no host synchronisation
    field.normal_force, field.friction_force, field.centre_of_pressure, field.slip_ratio, field.cells

Every pixel's penetration into the elastomer gives a normal pressure through a stiffness (an elastic foundation), the object's
tangential motion since first contact a shear traction capped by Coulomb's cone; the launch reduces them per env and per cell of
a coarse tactile grid."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _stage


@dataclass
class ContactGel:
    """One elastomer: normal and tangential foundation stiffness `k_n`, `k_t` [Pa/mm] (pressure per mm of penetration / of tangential
    displacement) and the friction coefficient `mu` of Coulomb's cone."""

    k_n: float
    k_t: float = 0.0
    mu: float = 0.0

    @classmethod
    def from_material(cls, youngs: float, poisson: float, thickness_m: float, mu: float = 0.0) -> "ContactGel":
        """The elastic-foundation moduli of a layer of thickness h bonded to a rigid backing: k_n = E (1 - v) / ((1 + v) (1 - 2 v) h)
        (the constrained modulus over h) and k_t = E / (2 (1 + v) h) (the shear modulus over h), in Pa/mm."""
        E, v, h = float(youngs), float(poisson), float(thickness_m)
        if not (math.isfinite(E) and E >= 0 and math.isfinite(h) and h > 0):
            raise ValueError("ContactGel.from_material: youngs must be finite and >= 0, thickness_m finite and > 0")
        if not (math.isfinite(v) and v > -1.0):
            raise ValueError("ContactGel.from_material: poisson must be finite and > -1")
        if v >= 0.5:
            raise ValueError(f"ContactGel.from_material: poisson = {v} >= 0.5 - the constrained modulus of an incompressible layer is "
                             "unbounded; pass the stiffnesses k_n, k_t directly (ContactGel(k_n, k_t, mu)), e.g. from an indentation test")
        k_n = E * (1 - v) / ((1 + v) * (1 - 2 * v) * h)  # Pa/m
        k_t = E / (2 * (1 + v) * h)
        return cls(k_n=k_n * 1e-3, k_t=k_t * 1e-3, mu=mu)

    def row(self) -> np.ndarray:
        """The (4,) float32 row [k_n, k_t, mu, 0] of `tacex_contact_field`'s gel table."""
        with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
            r = np.array([self.k_n, self.k_t, self.mu, 0.0], dtype=np.float32)
        if not np.isfinite(r).all():
            raise ValueError("ContactGel: k_n, k_t and mu must be finite (in float32)")
        if (r < 0).any():
            raise ValueError("ContactGel: k_n, k_t and mu must be >= 0")
        return r


class ContactField:
    """What one call of a `TactileContactModel` returns.  `record` (B,16) float64 (the slots of `tacex_contact_field`), `cells`
    (B,rows,cols,3) float32 force per tactile cell [N], `image` (B,H,W,3) float32 traction [Pa] or None.  Forces and tractions are
    those ON THE PAD in the camera frame (x = columns, y = rows, z = optical axis): the normal component is negative under an
    indenter, as in `FemTractionImage`.  Every property is a view of `record` or a torch op on it (no synchronisation)."""

    def __init__(self, record: torch.Tensor, cells: torch.Tensor, image: torch.Tensor | None):
        self.record, self.cells, self.image = record, cells, image

    @property
    def force(self) -> torch.Tensor:
        """(B,3) net force on the pad [N]."""
        return self.record[:, 0:3]

    @property
    def normal_force(self) -> torch.Tensor:
        """(B,) Fn >= 0 [N]."""
        return self.record[:, 6]

    @property
    def friction_force(self) -> torch.Tensor:
        """(B,2) net shear force (x, y) on the pad [N]."""
        return self.record[:, 0:2]

    @property
    def torque(self) -> torch.Tensor:
        """(B,3) torque on the pad about the image centre on the pad face [N m]."""
        return self.record[:, 3:6]

    @property
    def contact_area(self) -> torch.Tensor:
        """(B,) [m^2]."""
        return self.record[:, 7]

    @property
    def num_contact(self) -> torch.Tensor:
        return self.record[:, 8]

    @property
    def centre_of_pressure(self) -> torch.Tensor:
        """(B,2) (x, y) in pixels; the image centre without contact."""
        return self.record[:, 9:11]

    @property
    def max_penetration(self) -> torch.Tensor:
        """(B,) [mm]."""
        return self.record[:, 11]

    @property
    def volume(self) -> torch.Tensor:
        """(B,) penetrated volume [mm^3]."""
        return self.record[:, 12]

    @property
    def num_slipping(self) -> torch.Tensor:
        return self.record[:, 13]

    @property
    def slip_ratio(self) -> torch.Tensor:
        """(B,) slipping pixels / contact pixels: 0 sticking, 1 gross slip; 0 without contact."""
        return self.record[:, 13] / self.record[:, 8].clamp(min=1.0)

    @property
    def patch_angle(self) -> torch.Tensor:
        """(B,) angle of the pressure patch's long axis against the x axis [rad], in (-pi/2, pi/2]."""
        return self.record[:, 14]

    @property
    def patch_aspect(self) -> torch.Tensor:
        """(B,) short / long axis of the pressure patch: 1 round, -> 0 elongated."""
        return self.record[:, 15]


class PartContactField(ContactField):
    """What `TactileContactModel.parts` returns: `record` (B,L,16) float64, one record of `tacex_contact_field`'s slots per env and
    label (over the pixels of that label alone), and `image` (B,H,W,3) float32 traction [Pa] or None; `cells` is None (the call has
    none).  The accessors are `ContactField`'s, shaped (B, L, ...)."""

    def __init__(self, record: torch.Tensor, image: torch.Tensor | None):
        super().__init__(record, None, image)

    force = property(lambda self: self.record[..., 0:3], doc="(B,L,3) net force on the pad through each part [N].")
    normal_force = property(lambda self: self.record[..., 6], doc="(B,L) Fn >= 0 [N].")
    friction_force = property(lambda self: self.record[..., 0:2], doc="(B,L,2) net shear force (x, y) [N].")
    torque = property(lambda self: self.record[..., 3:6], doc="(B,L,3) torque about the image centre on the pad face [N m].")
    contact_area = property(lambda self: self.record[..., 7], doc="(B,L) [m^2].")
    num_contact = property(lambda self: self.record[..., 8])
    centre_of_pressure = property(lambda self: self.record[..., 9:11], doc="(B,L,2) (x, y) in pixels; the image centre without contact.")
    max_penetration = property(lambda self: self.record[..., 11], doc="(B,L) [mm].")
    volume = property(lambda self: self.record[..., 12], doc="(B,L) penetrated volume [mm^3].")
    num_slipping = property(lambda self: self.record[..., 13])
    slip_ratio = property(lambda self: self.record[..., 13] / self.record[..., 8].clamp(min=1.0), doc="(B,L) slipping / contact pixels.")
    patch_angle = property(lambda self: self.record[..., 14], doc="(B,L) [rad].")
    patch_aspect = property(lambda self: self.record[..., 15], doc="(B,L) short / long axis of the pressure patch.")


MAX_LABELS = 8


def slip_from_fots(marker_sim) -> torch.Tensor:
    """The (B,5) slip table [dx_mm, dy_mm, dtheta_rad, cx_px, cy_px] from a `FOTSMarkerSimulator`'s trajectory state
    [len, x0, y0, th0, xl, yl, thl, n] (contact centroids in mm from the image centre, indenter yaw): the shear and twist since first
    contact, about the last contact centroid in pixels.  Rows of envs out of contact (len < 1) are zero.  torch ops on the device."""
    t = marker_sim._traj_state
    W, H = marker_sim.cfg.tactile_img_res
    mm2pix = float(marker_sim.cfg.mm_to_pixel)
    slip = torch.stack((t[:, 4] - t[:, 1], t[:, 5] - t[:, 2], t[:, 6] - t[:, 3], t[:, 4] * mm2pix + W / 2.0, t[:, 5] * mm2pix + H / 2.0), dim=1)
    return torch.where((t[:, 0] >= 1.0)[:, None], slip, torch.zeros_like(slip)).contiguous()


class TactileContactModel:
    """The contact model of `num_frames` envs.  `gels` (P,4) float32 and `gel_ids` (num_frames,) int32 are device tensors the caller
    may write in place (ids at reset, like `TactileCameraModel.profile_ids`; an env whose id is outside [0, P) reports zeros).
    `pixmm`: pixel pitch of the height map [mm]; `grid` = (rows, cols) of the tactile cells laid over the image."""

    gels, gel_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

    def __init__(self, gels, num_frames: int, device, pixmm: float = 0.0295, grid=(9, 11)):
        if not (math.isfinite(float(pixmm)) and float(pixmm) > 0):
            raise ValueError(f"TactileContactModel: pixmm = {pixmm}")
        if len(grid) != 2 or int(grid[0]) < 1 or int(grid[1]) < 1:
            raise ValueError(f"TactileContactModel: grid = {grid} must be (rows >= 1, cols >= 1)")
        self._lib, self._table = _stage.open_stage("TactileContactModel", "gels", "gel_ids", gels, ContactGel, num_frames, device)
        self.device = torch.device(device)
        self.num_frames = int(num_frames)
        self.pixmm = float(pixmm)
        self.grid = (int(grid[0]), int(grid[1]))

    @property
    def num_gels(self) -> int:
        return int(self.gels.shape[0])

    def randomize(self, env_ids=None, generator=None):
        """Re-draw the gel ids of `env_ids` (default: all) uniformly from [0, P) on the device."""
        return self._table.randomize(env_ids, generator)

    def __call__(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor, slip: torch.Tensor | None = None,
                 frame_rows: torch.Tensor | None = None, image: bool | torch.Tensor = False) -> ContactField:
        """One launch on the current stream.  `hm` (num_frames,H,W) float32 [mm], contiguous, on the model's device; `frame_min`,
        `indent` (num_frames,) float32 as the sensor's depth pass leaves them; `slip` (num_frames,5) float32 or None (no shear);
        `frame_rows` (num_frames,4) int32 contact rectangles of THESE height maps or None; `image`: True allocates the traction
        image, a (num_frames,H,W,3) float32 tensor is written in place, False writes none."""
        B, dev = self.num_frames, self._table.device

        def arg(name, t, shape, dtype=torch.float32):
            return _stage.check_tensor("TactileContactModel", name, t, shape, dtype, dev)

        arg("hm", hm, (B, "H", "W"))
        H, W = int(hm.shape[1]), int(hm.shape[2])
        arg("frame_min", frame_min, (B,))
        arg("indent", indent, (B,))
        if slip is not None:
            arg("slip", slip, (B, 5))
        if frame_rows is not None:
            arg("frame_rows", frame_rows, (B, 4), torch.int32)
        gel_ids, gels = self._table.check()
        rows, cols = self.grid
        if rows > H or cols > W:
            raise ValueError(f"TactileContactModel: grid {self.grid} is larger than the {H} x {W} image")
        img = None
        if isinstance(image, torch.Tensor):
            img = arg("image", image, (B, H, W, 3))
        elif image:
            img = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        record = torch.empty((B, 16), dtype=torch.float64, device=dev)
        cells = torch.empty((B, rows, cols, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = self._lib.tacex_contact_field(_lib.ptr(hm), _lib.ptr(frame_min), _lib.ptr(indent), _lib.ptr(gels), int(gels.shape[0]),
                                               _lib.ptr(gel_ids), _lib.ptr(slip), self.pixmm, _lib.ptr(frame_rows), rows, cols,
                                               _lib.ptr(record), _lib.ptr(cells), _lib.ptr(img), B, H, W,
                                               _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_contact_field")
        return ContactField(record, cells, img)

    def parts(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor, labels: torch.Tensor, num_labels: int,
              slip: torch.Tensor | None = None, frame_rows: torch.Tensor | None = None,
              image: bool | torch.Tensor = False) -> PartContactField:
        """One launch of `tacex_contact_field_parts` on the current stream: a record per env and label.  `hm`, `frame_min`, `indent`,
        `frame_rows` and `image` as in `__call__`; `labels` (num_frames,H,W) uint8, the label of every pixel (e.g.
        `SdfSceneSource.part_map`); `num_labels` L in 1..8 - a pixel whose label is >= L has no shear and enters no record; `slip`
        (num_frames,L,5) float32, a slip row per label, or None (no shear).  The grid has no part in this call."""
        B, dev = self.num_frames, self._table.device

        def arg(name, t, shape, dtype=torch.float32):
            return _stage.check_tensor("TactileContactModel.parts", name, t, shape, dtype, dev)

        if not 1 <= int(num_labels) <= MAX_LABELS:
            raise ValueError(f"TactileContactModel.parts: num_labels = {num_labels} (must be 1..{MAX_LABELS})")
        L = int(num_labels)
        arg("hm", hm, (B, "H", "W"))
        H, W = int(hm.shape[1]), int(hm.shape[2])
        arg("frame_min", frame_min, (B,))
        arg("indent", indent, (B,))
        arg("labels", labels, (B, H, W), torch.uint8)
        if slip is not None:
            arg("slip", slip, (B, L, 5))
        if frame_rows is not None:
            arg("frame_rows", frame_rows, (B, 4), torch.int32)
        gel_ids, gels = self._table.check()
        img = None
        if isinstance(image, torch.Tensor):
            img = arg("image", image, (B, H, W, 3))
        elif image:
            img = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        record = torch.empty((B, L, 16), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = self._lib.tacex_contact_field_parts(_lib.ptr(hm), _lib.ptr(frame_min), _lib.ptr(indent), _lib.ptr(gels), int(gels.shape[0]),
                                                     _lib.ptr(gel_ids), _lib.ptr(labels), L, _lib.ptr(slip), self.pixmm, _lib.ptr(frame_rows),
                                                     _lib.ptr(record), _lib.ptr(img), B, H, W, _lib.current_stream_handle(dev))
        _lib.check(rc, "tacex_contact_field_parts")
        return PartContactField(record, img)
