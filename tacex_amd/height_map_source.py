"""Height-map sources: what fills `output["height_map"]` when no camera depth is injected.

The reference renders the gel pad with an IsaacLab `TiledCamera` and converts the depth image
(gelsight_sensor.py:229-263, 581-593).  `IndenterHeightMapSource` replaces that round trip for primitive indenters: one
HIP launch rasterises the contact geometry of every env straight into the height map and leaves the per-frame minimum
and the indentation depth (taxim_sim.py:115-131) behind, exactly what `tacex_height_map_from_depth` would have produced
from the rendered depth.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

KINDS = {"none": -1.0, "sphere": 0.0, "cylinder": 1.0, "edge": 2.0, "two_spheres": 3.0}


class IndenterHeightMapSource:
    """Per-env analytic indenter: `params` is a (num_envs, 8) float32 device tensor
    [kind, cx_px, cy_px, r_px, angle_rad, press_mm, cx2_px, cy2_px] that the caller updates in place between steps."""

    def __init__(self, num_envs: int, device, pixmm: float = 0.0295, gel_top_mm: float = 28.5, far_clip_mm: float = 29.0):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.TacexHipError("IndenterHeightMapSource needs an AMD GPU device (no CPU fallback)")
        self.params = torch.zeros((num_envs, 8), dtype=torch.float32, device=dev)
        self.params[:, 0] = KINDS["none"]
        self.pixmm, self.gel_top_mm, self.far_clip_mm = float(pixmm), float(gel_top_mm), float(far_clip_mm)
        self._lib = _lib.load_library()

    def set(self, kind, cx, cy, r, angle=0.0, press_mm=0.0, cx2=0.0, cy2=0.0, env_ids=slice(None)):
        """Convenience setter; arguments are scalars or per-env tensors, `kind` a name from KINDS or a tensor of codes."""
        k = KINDS[kind] if isinstance(kind, str) else kind
        for col, v in enumerate((k, cx, cy, r, angle, press_mm, cx2, cy2)):
            self.params[env_ids, col] = v if not isinstance(v, torch.Tensor) else v.to(self.params)

    def fill(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor | None, gelpad_height: float,
             gelpad_to_camera_min_distance: float):
        """hm (B, H, W) mm, frame_min (B,), indent (B,) or None - all written in one launch on the current stream."""
        B, H, W = hm.shape
        with torch.cuda.device(hm.device):
            rc = self._lib.tacex_height_map_from_indenters(
                _lib.ptr(self.params), self.pixmm, self.gel_top_mm, self.far_clip_mm, float(gelpad_height),
                float(gelpad_to_camera_min_distance), _lib.ptr(hm), _lib.ptr(frame_min), _lib.ptr(indent), B, H, W,
                _lib.current_stream_handle(hm.device))
        _lib.check(rc, "tacex_height_map_from_indenters")


def _bounding_sphere(verts: torch.Tensor) -> list:
    """[cx, cy, cz, r] of a (V, 3) mesh: the centre of its bounding box and the farthest vertex from it, a hair wider."""
    v = verts.double().cpu()
    c = 0.5 * (v.min(0).values + v.max(0).values)
    return [float(c[0]), float(c[1]), float(c[2]), float((v - c).norm(dim=1).max()) * 1.0001]


def _init_pinhole(self, num_envs: int, dev, resolution, intrinsics, clipping_range):
    """The pinhole camera of the rigid-mesh sources and the tensors the caller updates in place: image size, intrinsics, clipping
    range, `pos` (num_envs, 3), `quat` (num_envs, 4, wxyz), `depth` (num_envs, H, W)."""
    self.W, self.H = int(resolution[0]), int(resolution[1])
    self.fx, self.fy, self.cx, self.cy = (float(v) for v in intrinsics)
    self.near, self.far = float(clipping_range[0]), float(clipping_range[1])
    self.pos = torch.zeros((num_envs, 3), dtype=torch.float32, device=dev)
    self.pos[:, 2] = 1.0  # out of range until the caller places the object
    self.quat = torch.zeros((num_envs, 4), dtype=torch.float32, device=dev)
    self.quat[:, 0] = 1.0
    self.depth = torch.empty((num_envs, self.H, self.W), dtype=torch.float32, device=dev)


class _DepthFill:
    """`fill` of every source that renders a depth image (`self()` -> `self.depth`, clipping range `near` / `far`)."""

    def fill(self, hm: torch.Tensor, frame_min: torch.Tensor, indent: torch.Tensor | None, gelpad_height: float,
             gelpad_to_camera_min_distance: float):
        """hm (B, H, W) mm, frame_min (B,), indent (B,) or None: the render above, then the depth -> height-map pass
        (`tacex_height_map_from_depth` with this source's clipping range), both on the current stream."""
        if tuple(hm.shape) != tuple(self.depth.shape):
            raise RuntimeError(f"height map has shape {tuple(hm.shape)}, the source renders {tuple(self.depth.shape)}")
        depth = self()
        B, H, W = hm.shape
        with torch.cuda.device(hm.device):
            rc = self._lib.tacex_height_map_from_depth(
                _lib.ptr(depth), self.near, self.far, float(gelpad_height), float(gelpad_to_camera_min_distance), _lib.ptr(hm),
                _lib.ptr(frame_min), _lib.ptr(indent), 0, 0, B, H, W, _lib.current_stream_handle(hm.device))
        _lib.check(rc, "tacex_height_map_from_depth")


class MeshDepthSource:
    """Camera depth of a rigid triangle mesh per env (arbitrary indenters): a callable for
    `cfg.sensor_camera_cfg.depth_source` that stands in for the IsaacLab TiledCamera read-out of the reference
    (gelsight_sensor.py:229-263): `source()` -> (num_envs, H, W) float32 "distance_to_image_plane" depth in metres, inf where
    nothing lies inside the clipping range.  The caller updates `pos` (num_envs, 3) and `quat` (num_envs, 4, wxyz) in place -
    the pose of the object in the CAMERA frame (x right, y down, z along the optical axis)."""

    def __init__(self, verts, tris, num_envs: int, device, resolution=(320, 240), intrinsics=(340.0, 325.0, 160.0, 125.0),
                 clipping_range=(0.024, 0.029)):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.TacexHipError("MeshDepthSource needs an AMD GPU device (no CPU fallback)")
        self.verts = torch.as_tensor(verts, dtype=torch.float32).reshape(-1, 3).contiguous().to(dev)
        self.tris = torch.as_tensor(tris, dtype=torch.int32).reshape(-1, 3).contiguous().to(dev)
        if self.tris.numel() == 0 or int(self.tris.min()) < 0 or int(self.tris.max()) >= self.verts.shape[0]:
            raise ValueError("MeshDepthSource: triangle indices out of range")
        _init_pinhole(self, num_envs, dev, resolution, intrinsics, clipping_range)
        self._bsphere = (C.c_float * 4)(*_bounding_sphere(self.verts))
        self._lib = _lib.load_library()

    def __call__(self) -> torch.Tensor:
        with torch.cuda.device(self.depth.device):
            rc = self._lib.tacex_depth_from_mesh(
                _lib.ptr(self.verts), _lib.ptr(self.tris), int(self.verts.shape[0]), int(self.tris.shape[0]),
                _lib.ptr(self.pos), _lib.ptr(self.quat),
                self.fx, self.fy, self.cx, self.cy, self.near, self.far, C.cast(self._bsphere, C.c_void_p), _lib.ptr(self.depth),
                int(self.depth.shape[0]),
                self.H, self.W, _lib.current_stream_handle(self.depth.device))
        _lib.check(rc, "tacex_depth_from_mesh")
        return self.depth


class MeshLibraryDepthSource(_DepthFill):
    """Camera depth of a rigid triangle mesh per env, each env rendering ITS OWN mesh of a library (`tacex_depth_from_mesh_library`,
    one HIP launch plus one for meshes of more than 1024 triangles): the TiledCamera read-out of a scene whose envs hold different
    objects (a multi-asset spawner).  Same calling contract as `MeshDepthSource`: `source()` -> (num_envs, H, W) float32 depth in metres,
    inf where nothing is seen; the caller updates `pos` (num_envs, 3), `quat` (num_envs, 4, wxyz) - the object's pose in the CAMERA
    frame - and `mesh_ids` (num_envs,) int32 in place.  Each env's image is bit-equal to `MeshDepthSource(*meshes[id])` with the same
    pose; an id outside [0, len(meshes)) renders nothing.  `fill(...)` is the `set_height_map_source` interface (render +
    `tacex_height_map_from_depth` with this source's clipping range)."""

    def __init__(self, meshes, num_envs: int, device, resolution=(320, 240), intrinsics=(340.0, 325.0, 160.0, 125.0),
                 clipping_range=(0.024, 0.029)):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.TacexHipError("MeshLibraryDepthSource needs an AMD GPU device (no CPU fallback)")
        if len(meshes) == 0:
            raise ValueError("MeshLibraryDepthSource: empty mesh library")
        verts, tris, table, spheres, base = [], [], [], [], 0
        for k, (v, t) in enumerate(meshes):
            v = torch.as_tensor(v, dtype=torch.float32).reshape(-1, 3).cpu()
            t = torch.as_tensor(t, dtype=torch.int32).reshape(-1, 3).cpu()
            if t.numel() == 0 or int(t.min()) < 0 or int(t.max()) >= v.shape[0]:
                raise ValueError(f"MeshLibraryDepthSource: mesh {k}: triangle indices out of range")
            spheres.append(_bounding_sphere(v))
            table.append([sum(len(x) for x in tris), t.shape[0]])
            verts.append(v)
            tris.append(t + base)
            base += v.shape[0]
        self.num_meshes = len(meshes)
        self.verts = torch.cat(verts).contiguous().to(dev)
        self.tris = torch.cat(tris).contiguous().to(dev)
        self.mesh_tris = torch.tensor(table, dtype=torch.int32, device=dev)
        self.mesh_spheres = torch.tensor(spheres, dtype=torch.float32, device=dev)
        self._max_tris = max(n for _, n in table)
        _init_pinhole(self, num_envs, dev, resolution, intrinsics, clipping_range)
        self.mesh_ids = torch.zeros((num_envs,), dtype=torch.int32, device=dev)
        self._lib = _lib.load_library()

    def __call__(self) -> torch.Tensor:
        if self.mesh_ids.dtype != torch.int32 or self.mesh_ids.shape != (self.depth.shape[0],) or not self.mesh_ids.is_contiguous():
            raise ValueError(f"MeshLibraryDepthSource.mesh_ids must stay a contiguous ({self.depth.shape[0]},) int32 tensor")
        with torch.cuda.device(self.depth.device):
            rc = self._lib.tacex_depth_from_mesh_library(
                _lib.ptr(self.verts), _lib.ptr(self.tris), _lib.ptr(self.mesh_tris), _lib.ptr(self.mesh_spheres), self.num_meshes,
                self._max_tris, _lib.ptr(self.mesh_ids), _lib.ptr(self.pos), _lib.ptr(self.quat), self.fx, self.fy, self.cx, self.cy,
                self.near, self.far, _lib.ptr(self.depth), int(self.depth.shape[0]), self.H, self.W,
                _lib.current_stream_handle(self.depth.device))
        _lib.check(rc, "tacex_depth_from_mesh_library")
        return self.depth


def contact_face_triangles(points, tets, optical_axis_w, min_cos: float = 0.5) -> np.ndarray:
    """(F,3) int32 boundary triangles of a tet mesh whose REST outward unit normal n has n . optical_axis_w > min_cos, wound along n.
    The outward side of a boundary face is the side away from the fourth vertex of its tet - not the winding of
    `UipcObject.surface_triangles()`, which looks inward on negatively oriented tets (the gelpad box's)."""
    P = np.asarray(points, dtype=np.float64)
    T = np.asarray(tets, dtype=np.int64)
    faces = T[:, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]].reshape(-1, 3)
    opposite = T.reshape(-1)  # face k of a tet leaves out its vertex k
    _, inv, cnt = np.unique(np.sort(faces, axis=1), axis=0, return_inverse=True, return_counts=True)
    boundary = cnt[inv.reshape(-1)] == 1
    faces, opposite = faces[boundary], opposite[boundary]
    a, b, c = (P[faces[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    inward = np.einsum("ij,ij->i", n, P[opposite] - a) > 0.0
    n[inward] *= -1.0
    faces[inward] = faces[inward][:, [0, 2, 1]]
    axis = np.asarray(optical_axis_w, dtype=np.float64)
    cosang = (n @ axis) / (np.linalg.norm(n, axis=1) * np.linalg.norm(axis))
    return np.ascontiguousarray(faces[cosang > min_cos], dtype=np.int32)


class _SimCamera:
    """The sensor camera over a `UipcSim`: pose, intrinsics, clipping range and the (num_envs, H, W) depth image - what the depth sources
    and `FemTractionImage` share."""

    def _init_camera(self, sim, camera_pos_w, camera_quat_w_ros, resolution, intrinsics, clipping_range):
        """Sets `pos` / `rot_inv` / image size / intrinsics / clipping range / `depth`; returns the camera -> world rotation (3,3)."""
        from .simulation_approaches.fem_based.sim.tactile_sensor_uipc import quat_to_matrix

        name = type(self).__name__
        self._sim, dev, B = sim, sim.device, sim.num_envs
        q = torch.as_tensor(camera_quat_w_ros, dtype=torch.float64).reshape(-1, 4)
        q = q / q.norm(dim=1, keepdim=True)
        rot = quat_to_matrix(q)  # camera -> world
        self.pos = torch.as_tensor(camera_pos_w, dtype=torch.float64).reshape(-1, 3).expand(B, 3).contiguous().to(dev)
        self.rot_inv = rot.transpose(-1, -2).expand(B, 3, 3).contiguous().to(dev)
        self.W, self.H = int(resolution[0]), int(resolution[1])
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in intrinsics)
        self.near, self.far = float(clipping_range[0]), float(clipping_range[1])
        if not (0.0 <= self.near < self.far):
            raise ValueError(f"{name}: clipping range {clipping_range}")
        self.depth = torch.empty((B, self.H, self.W), dtype=torch.float32, device=dev)
        self._lib = _lib.load_library()
        return rot[0]


class _SimCameraDepthSource(_SimCamera, _DepthFill):
    """What `FemSurfaceDepthSource` and `AffineBodyDepthSource` share: the sensor camera over a `UipcSim` (`_SimCamera`), the ordering behind
    a step on a side stream, and `fill` (`_DepthFill`).  A subclass supplies `_render(sim)`, the one launch that writes `self.depth` from
    the simulation state."""

    def __call__(self) -> torch.Tensor:
        sim = self._sim
        sim.wait_for_step()  # a step enqueued on a side stream (UipcSim.step_done) is ordered before the render
        self._render(sim)
        return self.depth


class _FemContactFace:
    """The pad's rendered face, shared by `FemSurfaceDepthSource` and `FemTractionImage`: the object's checks, the face selection and the
    index tables the kernels read (`surf_ids`, `tris`), validated here on the host - the device does not check them."""

    def _init_face(self, uipc_object, camera_pos_w, camera_quat_w_ros, resolution, intrinsics, clipping_range, triangles):
        name = type(self).__name__
        sim = getattr(uipc_object, "_uipc_sim", None)
        if sim is None or getattr(sim, "x", None) is None:
            raise RuntimeError(f"{name} needs a UipcObject attached to a UipcSim that was set up (setup_sim)")
        if getattr(uipc_object, "is_affine_body", False):
            raise ValueError(f"{name} renders the deformable object (the gel pad), not an affine body")
        rot = self._init_camera(sim, camera_pos_w, camera_quat_w_ros, resolution, intrinsics, clipping_range)
        dev = sim.device
        if triangles is None:
            tri = contact_face_triangles(uipc_object.points, uipc_object.tets, rot[:, 2].numpy())
        else:
            tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
            if len(tri) and (tri.min() < 0 or tri.max() >= uipc_object.num_verts):
                raise ValueError(f"{name}: triangle indices outside [0, {uipc_object.num_verts})")
        if len(tri) == 0:
            raise ValueError(f"{name}: no triangles to render")
        ids, local = np.unique(tri.reshape(-1), return_inverse=True)
        self.triangles = np.ascontiguousarray(tri, dtype=np.int32)  # (F,3) object vertex ids
        self.surf_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
        self.tris = torch.from_numpy(local.reshape(-1, 3).astype(np.int32)).to(dev)
        return sim


class FemSurfaceDepthSource(_FemContactFace, _SimCameraDepthSource):
    """Camera depth of the FEM gel pad's deformed contact face, per env, straight from the FEM state (`UipcSim.x`) in one HIP launch
    (`tacex_depth_from_deformed_mesh`): the image the reference's sensor camera takes of the UIPC surface meshes after every step
    (tacex_uipc uipc_sim.py:268-284, read by GelSightSensor._get_height_map).  `source()` -> (num_envs, H, W) float32 depth in metres,
    inf where nothing is seen: a drop-in `cfg.sensor_camera_cfg.depth_source`; `fill(...)` is the `set_height_map_source` interface
    (same render + `tacex_height_map_from_depth`, bit-equal results).  Sensors of a `GelSightSensorGroup` take their depth slices from
    the group, not from a source.

    Camera: `camera_pos_w` (3,) or (num_envs, 3) and `camera_quat_w_ros` (wxyz, (4,) or (num_envs, 4)) in the convention of
    `ManiSkillSimulatorCfg.camera_pos_w` / `camera_quat_w_ros` (x right, y down, z along the optical axis).  `pos` (num_envs, 3) and
    `rot_inv` (num_envs, 3, 3) float64 are device tensors the caller may update in place (a camera that follows the sensor case).
    Rendered faces: by default the boundary triangles whose rest outward normal looks away from the camera (`n . axis > 0.5`) - the
    contact face; the back face, which sits at the near plane, and the side walls are left out.  `triangles` (F,3) vertex ids of the
    object's mesh overrides that choice."""

    def __init__(self, uipc_object, camera_pos_w, camera_quat_w_ros, resolution=(320, 240), intrinsics=(340.0, 325.0, 160.0, 125.0),
                 clipping_range=(0.024, 0.029), triangles=None):
        self._init_face(uipc_object, camera_pos_w, camera_quat_w_ros, resolution, intrinsics, clipping_range, triangles)

    def _render(self, sim):
        x = sim.x
        with torch.cuda.device(self.depth.device):
            rc = self._lib.tacex_depth_from_deformed_mesh(
                _lib.ptr(x), int(x.shape[1]), _lib.ptr(self.surf_ids), int(self.surf_ids.shape[0]), _lib.ptr(self.tris),
                int(self.tris.shape[0]), _lib.ptr(self.pos), _lib.ptr(self.rot_inv), self.fx, self.fy, self.cx, self.cy, self.near,
                self.far, _lib.ptr(self.depth), int(self.depth.shape[0]), self.H, self.W, _lib.current_stream_handle(self.depth.device))
        _lib.check(rc, "tacex_depth_from_deformed_mesh")


class AffineBodyDepthSource(_SimCameraDepthSource):
    """Camera depth of the scene's affine body (the ball of `FemBallScene`), per env, straight from its 12-unknown state (`UipcSim.q`,
    read in place) in one HIP launch (`tacex_depth_from_affine_body`): what the sensor camera sees of the object that presses into the
    pad with the gel hidden - the height map Taxim is built for (its pyramid simulates the gel), and the depth ManiSkill-ViTac's
    `gen_rgb_image` shades (tactile_sensor_sapienipc.py:424-457).  A kinematic body, whose `q` the caller moves, renders the same way.
    Same interface as `FemSurfaceDepthSource`: `source()` -> (num_envs, H, W) float32 metres, inf where nothing is seen, a drop-in
    `cfg.sensor_camera_cfg.depth_source`; `fill(...)`; `pos` / `rot_inv` updated in place by the caller.  Every triangle of the body's
    surface is rendered (the nearest fragment wins, no culling)."""

    def __init__(self, uipc_object, camera_pos_w, camera_quat_w_ros, resolution=(320, 240), intrinsics=(340.0, 325.0, 160.0, 125.0),
                 clipping_range=(0.024, 0.029)):
        sim = getattr(uipc_object, "_uipc_sim", None)
        if not getattr(uipc_object, "is_affine_body", False):
            raise ValueError("AffineBodyDepthSource renders an affine body (FemSurfaceDepthSource renders the gel pad)")
        if sim is None or getattr(sim, "x", None) is None or getattr(sim, "_body", None) is not uipc_object:
            raise RuntimeError("AffineBodyDepthSource needs the affine-body UipcObject of a UipcSim that was set up (setup_sim)")
        self._init_camera(sim, camera_pos_w, camera_quat_w_ros, resolution, intrinsics, clipping_range)
        tri = np.ascontiguousarray(uipc_object.tris, dtype=np.int32).reshape(-1, 3)
        if len(tri) == 0 or tri.min() < 0 or tri.max() >= uipc_object.num_verts:
            raise ValueError(f"AffineBodyDepthSource: no triangles, or triangle indices outside [0, {uipc_object.num_verts})")
        self.rest_verts = torch.from_numpy(np.ascontiguousarray(uipc_object.points, dtype=np.float64)).to(sim.device)  # (nv,3) body frame
        self.tris = torch.from_numpy(tri).to(sim.device)

    def _render(self, sim):
        q = sim.q
        if q.dtype != torch.float64 or tuple(q.shape) != (self.depth.shape[0], 4, 3) or not q.is_contiguous():
            raise ValueError(f"AffineBodyDepthSource: UipcSim.q must stay a contiguous ({self.depth.shape[0]}, 4, 3) float64 tensor")
        with torch.cuda.device(self.depth.device):
            rc = self._lib.tacex_depth_from_affine_body(
                _lib.ptr(self.rest_verts), int(self.rest_verts.shape[0]), _lib.ptr(self.tris), int(self.tris.shape[0]), _lib.ptr(q),
                _lib.ptr(self.pos), _lib.ptr(self.rot_inv), self.fx, self.fy, self.cx, self.cy, self.near, self.far, _lib.ptr(self.depth),
                int(self.depth.shape[0]), self.H, self.W, _lib.current_stream_handle(self.depth.device))
        _lib.check(rc, "tacex_depth_from_affine_body")


class FemTractionImage(_FemContactFace, _SimCamera):
    """Contact traction of the FEM gel pad as an image in the camera frame, per env, in one HIP launch
    (`tacex_traction_image_from_deformed_mesh`): the per-vertex contact forces of `UipcSim.contact_forces(per_vertex=True)` divided by
    the barrier's vertex areas (`UipcObject.surface_vertex_areas()`) and interpolated over the deformed contact face by the rasteriser
    of `FemSurfaceDepthSource`.  `image()` -> (num_envs, H, W, 3) float32 in Pa, pixel-aligned with that source's depth (so with
    `height_map` and `tactile_rgb` when it feeds the sensor), zero where nothing is seen.  Forces act ON the pad, in the camera frame
    (x right, y down, z along the optical axis): `[..., 2]` is the normal pressure, negative where an indenter pushes the face towards the
    camera, `[..., 0:2]` the shear.  Works on the prescribed-indenter scene and on a scene with an affine body (the pad of `FemBallScene`).

    Constructor arguments, face selection, `pos` / `rot_inv` (updated in place by the caller) as in `FemSurfaceDepthSource`.  `traction`
    and `depth` are persistent tensors, overwritten by every call."""

    def __init__(self, uipc_object, camera_pos_w, camera_quat_w_ros, resolution=(320, 240), intrinsics=(340.0, 325.0, 160.0, 125.0),
                 clipping_range=(0.024, 0.029), triangles=None):
        sim = self._init_face(uipc_object, camera_pos_w, camera_quat_w_ros, resolution, intrinsics, clipping_range, triangles)
        self.num_verts = int(uipc_object.num_verts)
        self.vertex_areas = torch.from_numpy(np.ascontiguousarray(uipc_object.surface_vertex_areas(), dtype=np.float64)).to(sim.device)
        self.traction = torch.zeros((sim.num_envs, self.H, self.W, 3), dtype=torch.float32, device=sim.device)

    def __call__(self, friction: bool | None = None, with_depth: bool = False) -> torch.Tensor:
        """The traction image of the current state: `contact_forces(per_vertex=True, friction=friction)` and the render, both on the
        current stream behind the last step, no host synchronisation.  `with_depth`: also write `self.depth` (bit-equal to
        `FemSurfaceDepthSource`'s)."""
        sim = self._sim
        sim.wait_for_step()  # a step enqueued on a side stream (UipcSim.step_done) is ordered before both launches
        forces = sim.contact_forces(per_vertex=True, friction=friction)
        return self.render(forces.vertex_forces, with_depth=with_depth)

    def render(self, vertex_forces: torch.Tensor, with_depth: bool = False) -> torch.Tensor:
        """The image of explicit per-vertex forces (num_envs, V, 3) float64 [N, world frame] on the current FEM state."""
        x = self._sim.x
        B = int(self.traction.shape[0])
        f = vertex_forces
        if not isinstance(f, torch.Tensor) or f.dtype != torch.float64 or tuple(f.shape) != (B, self.num_verts, 3) or f.device != x.device:
            raise ValueError(f"FemTractionImage.render: vertex_forces must be a ({B}, {self.num_verts}, 3) float64 tensor on {x.device}")
        f = f if f.is_contiguous() else f.contiguous()
        with torch.cuda.device(self.traction.device):
            rc = self._lib.tacex_traction_image_from_deformed_mesh(
                _lib.ptr(x), int(x.shape[1]), _lib.ptr(self.surf_ids), int(self.surf_ids.shape[0]), _lib.ptr(self.tris),
                int(self.tris.shape[0]), _lib.ptr(f), _lib.ptr(self.vertex_areas), _lib.ptr(self.pos), _lib.ptr(self.rot_inv), self.fx,
                self.fy, self.cx, self.cy, self.near, self.far, _lib.ptr(self.traction), _lib.ptr(self.depth) if with_depth else None, B,
                self.H, self.W, _lib.current_stream_handle(self.traction.device))
        _lib.check(rc, "tacex_traction_image_from_deformed_mesh")
        return self.traction
