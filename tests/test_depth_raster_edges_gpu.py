"""The three mesh rasterisers of csrc/depth_raster.hip (`tacex_depth_from_mesh`, `tacex_depth_from_mesh_library`,
`tacex_depth_from_deformed_mesh`) at the edges the 320x240 / 640x480 tests step around, each image compared with
oracle/mesh_depth_oracle.py bit for bit - the finite mask first, then the values:
  images whose width and height are no multiple of the 64 x 32 tile (77x100, 40x72) and a single partial tile (24x48);
  a triangle with a vertex behind the camera plane, zero-area triangles, both windings; a mesh so close that the bounding-sphere cull is off;
  a library mesh of exactly 1024 / 1025 triangles (one launch / two), null `mesh_ids` and `mesh_spheres`;
  the deformed kernel with five triangle-list rounds, exactly 2048 staged surface vertices and 2049 unstaged ones, a camera looking away.
The scenes are plain arrays handed to the C ABI; the CPU tests at the top check on the oracle alone that every scene has the property it
is there for."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.mesh_depth_oracle import icosphere, pose_rows, render_depth

CLIP = (0.024, 0.029)
TILE_W, TILE_H = 64, 32


def _intr(H, W):
    """The 320x240 intrinsics of tests/test_mesh_depth.py scaled to the image."""
    return dict(fx=340.0 * W / 320, fy=325.0 * H / 240, cx=160.0 * W / 320, cy=125.0 * H / 240)


def _quats(seed, n, spread):
    """n unit quaternions within `spread` of the identity (float32, as the device reads them)."""
    q = np.random.RandomState(seed).normal(size=(n, 4)) * spread
    q[:, 0] = 1.0
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _at_pixel(H, W, x, y, z):
    """Camera-frame point that projects to pixel coordinates (x, y) at depth z."""
    k = _intr(H, W)
    return [(x - k["cx"]) / k["fx"] * z, (y - k["cy"]) / k["fy"] * z, z]


def _heightfield(ny, nx, x0, x1, y0, y1, z0=0.027, amp=0.0008):
    """(ny * nx, 3) float32 grid over [x0, x1] x [y0, y1] with a smooth bump pattern in z, 2 (ny - 1)(nx - 1) triangles."""
    v, u = np.meshgrid(np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    P = np.stack([x0 + (x1 - x0) * u, y0 + (y1 - y0) * v, z0 + amp * np.sin(7.0 * u + 0.3) * np.cos(5.0 * v)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    a = (i * nx + j).reshape(-1)
    T = np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)])
    return P.astype(np.float32), T.astype(np.int32)


def _sphere_of(V):
    c = 0.5 * (V.min(0).astype(np.float64) + V.max(0))
    return np.array([*c, np.linalg.norm(V - c, axis=1).max() * 1.0001], np.float32)


# -- rigid-mesh scenes ----------------------------------------------------------------------------------------------------------------
def scene_a():
    """Two-lobe icosphere across the tile corner at pixel (64, 32) and off the right / bottom / both image edges."""
    H, W = 77, 100
    Vs, Ts = icosphere(0.004, 2)
    V = np.concatenate([Vs, Vs * 0.6 + np.array([0.003, 0.001, -0.0015], dtype=np.float32)])
    T = np.concatenate([Ts, Ts + len(Vs)])
    pos = np.array([_at_pixel(H, W, 64, 32, 0.030), _at_pixel(H, W, 98, 40, 0.0305), _at_pixel(H, W, 45, 75, 0.030),
                    _at_pixel(H, W, 97, 74, 0.0295)], np.float32)
    quat = np.random.RandomState(11).normal(size=(4, 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)
    return dict(V=V, T=T, pos=pos, quat=quat, H=H, W=W, clip=CLIP)


B_BEHIND = 3  # scene (b): index of the triangle with a vertex behind the camera plane


def scene_b(behind_z=-0.001, with_behind=True):
    """A large triangle in both windings, a nearer one on top of it, two zero-area triangles (a repeated vertex; three collinear
    vertices) and one triangle with a vertex behind the camera plane, which is dropped whole."""
    H, W = 40, 72
    V = np.array([[-0.004, -0.004, 0.027], [0.012, 0.0, 0.026], [0.0, 0.009, 0.028],      # 0-2 large
                  [0.002, 0.001, 0.0255], [0.008, 0.002, 0.0255], [0.005, 0.007, 0.0255],  # 3-5 nearer
                  [-0.006, 0.002, 0.027], [-0.004, 0.004, 0.027], [-0.002, 0.006, 0.027],  # 6-8 collinear
                  [-0.008, -0.003, 0.027], [-0.001, -0.007, 0.027], [-0.004, 0.0, behind_z]], np.float32)  # 9-11, the last one behind
    T = np.array([[0, 1, 2], [2, 1, 0], [3, 4, 5], [9, 10, 11], [6, 6, 7], [6, 7, 8]], np.int32)
    assert (T[B_BEHIND] == [9, 10, 11]).all()
    if not with_behind:
        T = np.delete(T, B_BEHIND, axis=0)
    pos = np.array([[0.0, 0.0, 0.0], [0.0005, -0.0005, 0.0003]], np.float32)
    quat = np.concatenate([np.array([[1.0, 0, 0, 0]], np.float32), _quats(5, 1, 0.02)])
    return dict(V=V, T=T, pos=pos, quat=quat, H=H, W=W, clip=CLIP)


def scene_c():
    """A 4 mm sphere centred 4 mm in front of the camera, seen from the inside: the near bound of its bounding sphere is not in front of
    the camera plane, so the tile cull switches itself off.  The second env has vertices behind the camera."""
    H, W = 24, 48
    V, T = icosphere(0.004, 2)
    pos = np.array([[0.0, 0.0, 0.004], [0.0003, -0.0002, 0.0038]], np.float32)
    quat = np.concatenate([np.array([[1.0, 0, 0, 0]], np.float32), _quats(6, 1, 0.5)])
    return dict(V=V, T=T, pos=pos, quat=quat, H=H, W=W, clip=(0.001, 0.05))


RIGID = {"a": scene_a, "b": scene_b, "c": scene_c}


def _render(s, V=None, T=None, envs=None):
    pos, quat = (s["pos"], s["quat"]) if envs is None else (s["pos"][envs], s["quat"][envs])
    return render_depth(s["V"] if V is None else V, s["T"] if T is None else T, pose_rows(pos, quat), near=s["clip"][0], far=s["clip"][1],
                        H=s["H"], W=s["W"], **_intr(s["H"], s["W"]))


@functools.lru_cache(maxsize=None)
def rigid_oracle(name):
    return _render(RIGID[name]())


# -- library scenes -------------------------------------------------------------------------------------------------------------------
def library():
    """Meshes in library order: (e) the 1024-triangle grid plus one nearer triangle = 1025, (d) the 17 x 33 grid = 1024, (f) an icosphere
    and a quad.  Every mesh sits in front of the camera by itself, so that poses near the identity keep all of them in view."""
    H, W = 77, 100
    Vd, Td = _heightfield(17, 33, -0.011, 0.011, -0.008, 0.008)
    assert len(Td) == 1024
    Ve = np.concatenate([Vd, np.array([[0.002, 0.003, 0.025], [0.009, 0.004, 0.025], [0.005, 0.009, 0.025]], np.float32)])
    Te = np.concatenate([Td, np.array([[len(Vd), len(Vd) + 1, len(Vd) + 2]], np.int32)])  # triangle 1024: the second launch's only one
    Vf, Tf = icosphere(0.003, 1)
    Vf = Vf + np.array([0.006, 0.004, 0.0285], np.float32)
    Vq = np.array([[-0.010, 0.002, 0.026], [-0.002, 0.003, 0.0265], [-0.003, 0.009, 0.027], [-0.011, 0.008, 0.0275]], np.float32)
    Tq = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    meshes = [(Ve, Te), (Vd, Td), (Vf, Tf), (Vq, Tq)]
    pos = np.array([[0.0, 0.0, 0.0], [0.0006, -0.0004, 0.0004], [-0.0008, 0.0005, -0.0003], [0.001, 0.0012, 0.0002]], np.float32)
    quat = np.concatenate([np.array([[1.0, 0, 0, 0]], np.float32), _quats(7, 3, 0.015)])
    return dict(meshes=meshes, pos=pos, quat=quat, H=H, W=W, clip=CLIP, V=None, T=None)


@functools.lru_cache(maxsize=None)
def library_oracle(ids):
    """(B, H, W): env b renders mesh ids[b] of the library alone."""
    s = library()
    return np.concatenate([_render(s, *s["meshes"][m], envs=[b]) for b, m in enumerate(ids)])


# -- deformed scenes ------------------------------------------------------------------------------------------------------------------
def _rot(ax, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def _state(surface, extra, seed):
    """FEM-like state around per-env surface positions (B, Vs, 3): x (B, Vs + extra, 3) float64 in which the surface vertices sit at the
    shuffled places `surf_ids` and every other vertex holds a value no image could survive."""
    B, Vs, _ = surface.shape
    rng = np.random.RandomState(seed)
    ids = rng.permutation(Vs + extra)[:Vs].astype(np.int32)
    x = np.full((B, Vs + extra, 3), 1.0e3)
    x[:, ids] = surface
    return x, ids


def _cameras(poses):
    pos = np.array([p for p, _ in poses], np.float64)
    rot_inv = np.stack([R.T for _, R in poses]).astype(np.float64)  # R: camera -> world
    return pos, np.ascontiguousarray(rot_inv)


def scene_g():
    """Level-3 icosphere as the deformed surface: 642 surface vertices among 700, 1280 triangles = five list rounds of 256."""
    H, W = 77, 100
    V, T = icosphere(0.004, 3)
    assert V.shape == (642, 3) and T.shape == (1280, 3)
    centre = np.array([0.0005, 0.0003, 0.030])
    surface = np.stack([V.astype(np.float64) * [1.0, 0.9, 1.05] + centre, V.astype(np.float64) * [1.1, 1.0, 0.95] + centre])
    x, ids = _state(surface, 58, 1)
    # env 1: the camera is moved so that the sphere hangs off the bottom right corner of the image
    shift = np.array(_at_pixel(H, W, 95, 73, 0.030)) - np.array(_at_pixel(H, W, W / 2, H / 2, 0.030))
    pos, rot_inv = _cameras([(np.array([0.0002, -0.0001, 0.0002]), _rot("z", 12.0) @ _rot("x", 2.0)), (-shift, _rot("y", 1.5))])
    return dict(x=x, ids=ids, T=T, pos=pos, rot_inv=rot_inv, H=H, W=W, clip=CLIP)


def scene_h(extra_surface_vertex=False):
    """Heightfield of exactly 2048 surface vertices (the staged route); with `extra_surface_vertex` one more that no triangle uses,
    placed behind the camera: 2049 surface vertices (the unstaged route), the same image."""
    H, W = 40, 72
    V, T = _heightfield(32, 64, -0.011, 0.012, -0.008, 0.0095)
    assert len(V) == 2048
    surface = np.stack([V.astype(np.float64), V.astype(np.float64) * [1.0, 1.0, 1.01] + [0.0003, 0.0, 0.0]])
    if extra_surface_vertex:
        surface = np.concatenate([surface, np.tile(np.array([[[0.05, -0.04, -0.01]]]), (2, 1, 1))], 1)
    # the same shuffle for both variants: the extra vertex takes one more place of the same permutation
    B, Vs, _ = surface.shape
    perm = np.random.RandomState(2).permutation(2048 + 52)
    ids = perm[:Vs].astype(np.int32)
    x = np.full((B, 2048 + 52, 3), 1.0e3)
    x[:, ids] = surface
    pos, rot_inv = _cameras([(np.zeros(3), np.eye(3)), (np.array([0.0004, 0.0003, -0.0002]), _rot("z", -6.0) @ _rot("y", 1.0))])
    return dict(x=x, ids=ids, T=T, pos=pos, rot_inv=rot_inv, H=H, W=W, clip=CLIP)


def scene_i():
    return scene_h(extra_surface_vertex=True)


def scene_j():
    """Scene (g)'s sphere on a single partial tile; the second env's camera is turned away by half a turn: its image is all inf."""
    s = scene_g()
    H, W = 24, 48
    pos, rot_inv = _cameras([(np.zeros(3), _rot("z", 30.0)), (np.zeros(3), _rot("y", 180.0))])
    return dict(s, pos=pos, rot_inv=rot_inv, H=H, W=W)


DEFORMED = {"g": scene_g, "h": scene_h, "i": scene_i, "j": scene_j}


def _camera_frame_f32(s):
    """(B, Vs, 3) float32 camera-frame surface vertices: float64 arithmetic in the kernel's order, rounded once
    (the statement of tests/test_fem_surface_depth.py)."""
    out = []
    for b in range(len(s["x"])):
        d, R = s["x"][b, s["ids"]] - s["pos"][b], s["rot_inv"][b]
        out.append(np.stack([(R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2] for i in range(3)], 1).astype(np.float32))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def deformed_oracle(name):
    s = DEFORMED[name]()
    pc = _camera_frame_f32(s)
    ident = pose_rows(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0, 0.0]]))
    return np.stack([render_depth(pc[b], s["T"], ident, near=s["clip"][0], far=s["clip"][1], H=s["H"], W=s["W"], **_intr(s["H"], s["W"]))[0]
                     for b in range(len(pc))])


# -- CPU: the scenes have the properties they are there for ----------------------------------------------------------------------------
def _has_edge_pixels(img):
    """Finite pixels in the last (partial) tile column and the last (partial) tile row of a (B, H, W) image."""
    _, H, W = img.shape
    f = np.isfinite(img)
    return f.sum() > 100 and f[:, :, (W - 1) // TILE_W * TILE_W:].any() and f[:, (H - 1) // TILE_H * TILE_H:, :].any()


def test_image_sizes_leave_partial_tiles():
    for H, W in ((77, 100), (40, 72)):
        assert W % TILE_W and H % TILE_H and W > TILE_W and H > TILE_H
    assert 24 < TILE_H and 48 < TILE_W


def test_rigid_scenes_have_teeth():
    for name in RIGID:
        assert _has_edge_pixels(rigid_oracle(name)), name
    a = np.isfinite(rigid_oracle("a"))
    assert a[0, 31, 63] and a[0, 32, 64] and a[0, 31, 64] and a[0, 32, 63]  # all four tiles around the corner at (64, 32)
    assert a[1, :, -1].any() and a[2, -1, :].any() and a[3, -1, -1]           # off the right edge, the bottom edge, the corner
    # (b): the behind-camera triangle exists, is dropped whole, and would show if its third vertex were in front
    s = scene_b()
    pose = pose_rows(s["pos"], s["quat"]).astype(np.float32)
    pz = (pose[:, None, 6:9] * s["V"][None]).sum(-1) + pose[:, None, 11]
    tri = s["T"][B_BEHIND]
    assert (pz[:, tri[2]] < 0).all() and (pz[:, tri[:2]] > 0.02).all()
    np.testing.assert_array_equal(rigid_oracle("b"), _render(scene_b(with_behind=False)))
    front = scene_b(behind_z=0.027)
    assert (np.isfinite(_render(front)) & ~np.isfinite(rigid_oracle("b"))).sum() > 20
    # ... both windings of the large triangle render the same pixels, the zero-area triangles none
    only = lambda rows: np.isfinite(_render(s, T=s["T"][rows]))
    np.testing.assert_array_equal(only([0]), only([1]))
    assert only([0]).sum() > 200 and not only([4, 5]).any()
    # (c): the near bound of the bounding sphere is at or behind the camera plane (cull off), env 1 has vertices behind the camera
    c = scene_c()
    pose = pose_rows(c["pos"], c["quat"]).astype(np.float32)
    pz = (pose[:, None, 6:9] * c["V"][None]).sum(-1) + pose[:, None, 11]
    assert (pose[:, 11] - np.float32(0.004 * 1.0001) <= 1e-4).all() and (pz[1] < 0).any() and (pz[0] <= 1e-6).any()
    assert np.isfinite(rigid_oracle("c")).reshape(2, -1).sum(1).min() > 100


def test_library_scenes_have_teeth():
    s = library()
    counts = [len(T) for _, T in s["meshes"]]
    assert counts[:2] == [1025, 1024] and max(counts[2:]) < 1024
    e, d = library_oracle((0, 0, 0, 0)), library_oracle((1, 1, 1, 1))
    for b in range(4):
        assert ((e[b] != d[b]) & np.isfinite(e[b])).sum() >= 20, b  # the extra, nearer triangle changes a block of pixels
    assert _has_edge_pixels(e) and _has_edge_pixels(d)
    mixed = library_oracle((1, 0, 2, 3))
    assert _has_edge_pixels(mixed) and np.isfinite(mixed).reshape(4, -1).sum(1).min() > 100


def test_deformed_scenes_have_teeth():
    for name in ("g", "h", "i"):
        img = deformed_oracle(name)
        assert _has_edge_pixels(img) and np.isfinite(img).reshape(2, -1).sum(1).min() > 100, name
    g, h, i = scene_g(), scene_h(), scene_i()
    assert len(g["ids"]) == 642 and g["x"].shape[1] > 642 and len(g["T"]) == 5 * 256 and (np.diff(g["ids"]) < 0).any()
    assert len(h["ids"]) == 2048 and len(i["ids"]) == 2049 and len(h["T"]) > 256
    assert i["T"].max() == 2047 and (_camera_frame_f32(i)[:, 2048, 2] < 0).all()  # the extra vertex: unreferenced, behind the camera
    np.testing.assert_array_equal(deformed_oracle("i"), deformed_oracle("h"))
    assert np.isfinite(deformed_oracle("g"))[1, -1, -1]  # env 1 hangs off the bottom right corner
    j = deformed_oracle("j")
    assert np.isfinite(j[0]).sum() > 40 and not np.isfinite(j[1]).any()


# -- GPU ------------------------------------------------------------------------------------------------------------------------------
def _equal_bit_for_bit(got, want, where):
    np.testing.assert_array_equal(np.isfinite(got), np.isfinite(want), err_msg=where)
    m = np.isfinite(want)
    np.testing.assert_array_equal(got[m], want[m], err_msg=where)
    assert np.isposinf(got[~m]).all(), where


def _dev(a, dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _guarded_image(B, H, W):
    import torch

    return torch.full(((B + 1) * H * W,), -7.0, dtype=torch.float32, device="cuda")


def _image(buf, B, H, W, where):
    a = buf.cpu().numpy()
    assert (a[B * H * W:] == np.float32(-7.0)).all(), f"{where}: wrote behind the image"
    return a[:B * H * W].reshape(B, H, W)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _run_rigid(s, V, T, sphere):
    from tacex_amd import _lib

    lib = _lib.load_library()
    B, H, W, k = len(s["pos"]), s["H"], s["W"], _intr(s["H"], s["W"])
    v, t, pos, quat = _dev(V, np.float32), _dev(T, np.int32), _dev(s["pos"], np.float32), _dev(s["quat"], np.float32)
    out = _guarded_image(B, H, W)
    bs = None if sphere is None else (C.c_float * 4)(*[float(e) for e in sphere])
    _lib.check(lib.tacex_depth_from_mesh(_lib.ptr(v), _lib.ptr(t), len(V), len(T), _lib.ptr(pos), _lib.ptr(quat), k["fx"], k["fy"], k["cx"], k["cy"],
                                         s["clip"][0], s["clip"][1], None if bs is None else C.cast(bs, C.c_void_p), _lib.ptr(out), B, H, W,
                                         _stream()), "tacex_depth_from_mesh")
    return _image(out, B, H, W, "tacex_depth_from_mesh")


@pytest.mark.gpu
@pytest.mark.parametrize("with_sphere", [False, True], ids=["no_sphere", "sphere"])
@pytest.mark.parametrize("name", list(RIGID))
def test_rigid_mesh_equals_oracle(name, with_sphere):
    s = RIGID[name]()
    got = _run_rigid(s, s["V"], s["T"], _sphere_of(s["V"]) if with_sphere else None)
    _equal_bit_for_bit(got, rigid_oracle(name), f"scene {name} sphere={with_sphere}")


@pytest.mark.gpu
@pytest.mark.parametrize("with_spheres", [False, True], ids=["no_spheres", "spheres"])
@pytest.mark.parametrize("ids", [None, (0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 2, 3), (3, 2, 1, 1)], ids=lambda i: "null_ids" if i is None else "ids" + "".join(map(str, i)))
def test_mesh_library_equals_single_mesh_and_oracle(ids, with_spheres):
    from tacex_amd import _lib

    lib = _lib.load_library()
    s = library()
    B, H, W, k = len(s["pos"]), s["H"], s["W"], _intr(s["H"], s["W"])
    first_v = np.cumsum([0] + [len(V) for V, _ in s["meshes"]])
    first_t = np.cumsum([0] + [len(T) for _, T in s["meshes"]])
    verts = np.concatenate([V for V, _ in s["meshes"]])
    tris = np.concatenate([T + first_v[m] for m, (_, T) in enumerate(s["meshes"])])
    mesh_tris = np.stack([first_t[:-1], np.diff(first_t)], 1)
    spheres = np.stack([_sphere_of(V) for V, _ in s["meshes"]])
    v, t, mt, sp = _dev(verts, np.float32), _dev(tris, np.int32), _dev(mesh_tris, np.int32), _dev(spheres, np.float32)
    pos, quat = _dev(s["pos"], np.float32), _dev(s["quat"], np.float32)
    mi = None if ids is None else _dev(np.array(ids), np.int32)
    out = _guarded_image(B, H, W)
    where = f"library ids={ids} spheres={with_spheres}"
    _lib.check(lib.tacex_depth_from_mesh_library(
        _lib.ptr(v), _lib.ptr(t), _lib.ptr(mt), _lib.ptr(sp) if with_spheres else 0, len(s["meshes"]), int(mesh_tris[:, 1].max()), _lib.ptr(mi),
        _lib.ptr(pos), _lib.ptr(quat), k["fx"], k["fy"], k["cx"], k["cy"], s["clip"][0], s["clip"][1], _lib.ptr(out), B, H, W, _stream()), where)
    got = _image(out, B, H, W, where)
    eff = (0,) * B if ids is None else ids
    _equal_bit_for_bit(got, library_oracle(eff), where)
    for m in sorted(set(eff)):  # ... and the single-mesh kernel on each mesh alone, all poses
        V, T = s["meshes"][m]
        single = _run_rigid(s, V, T, spheres[m] if with_spheres else None)
        for b in (b for b in range(B) if eff[b] == m):
            _equal_bit_for_bit(got[b], single[b], f"{where} env {b} vs the single-mesh kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DEFORMED))
def test_deformed_mesh_equals_oracle(name):
    from tacex_amd import _lib

    lib = _lib.load_library()
    s = DEFORMED[name]()
    B, H, W, k = len(s["x"]), s["H"], s["W"], _intr(s["H"], s["W"])
    x, ids, t = _dev(s["x"], np.float64), _dev(s["ids"], np.int32), _dev(s["T"], np.int32)
    pos, rot = _dev(s["pos"], np.float64), _dev(s["rot_inv"], np.float64)
    out = _guarded_image(B, H, W)
    where = f"deformed scene {name}"
    _lib.check(lib.tacex_depth_from_deformed_mesh(_lib.ptr(x), s["x"].shape[1], _lib.ptr(ids), len(s["ids"]), _lib.ptr(t), len(s["T"]), _lib.ptr(pos),
                                                  _lib.ptr(rot), k["fx"], k["fy"], k["cx"], k["cy"], s["clip"][0], s["clip"][1], _lib.ptr(out), B, H, W,
                                                  _stream()), where)
    _equal_bit_for_bit(_image(out, B, H, W, where), deformed_oracle(name), where)
