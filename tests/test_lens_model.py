"""Sensor lens model on the CPU: the ABI (symbols, refusals before any GPU call), `LensProfile.row()`, and known answers of the
NumPy restatement (tests/lens_model_ref.py, written from the header's contract; the GPU tests compare the kernels with it bit for
bit): identity, whole-pixel shifts, a half turn, vignetting, softness, the direction of the radial term, and the point inverse."""
import re

import numpy as np
import pytest
from conftest import REPO
from lens_model_ref import POINT_ITERATIONS, displacement, lens_frame, lens_points, profile_row, profile_set, source_positions


def _lib_and_module():
    from tacex_amd import _lib

    return _lib.load_library(), _lib


NARGS = {"tacex_lens_model": 9, "tacex_lens_camera_model": 16, "tacex_lens_points": 10}


def test_symbols_declared_exported_and_bound():
    lib, _lib = _lib_and_module()
    raw = (REPO / "include" / "tacex_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NARGS.items():
        decl = re.search(name + r"\s*\(([^)]*)\)", txt)
        assert decl, f"{name} is not declared in include/tacex_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs
    hdr = int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", raw).group(1))
    assert lib.tacex_abi_version() == hdr == _lib.ABI_VERSION == 20
    assert int(re.search(r"#define\s+TACEX_LENS_POINT_ITERATIONS\s+(\d+)", raw).group(1)) == POINT_ITERATIONS


def test_the_translation_unit_is_built_without_fp_contraction():
    from tacex_amd import _build

    assert "lens_model.hip" in _build.SOURCES and (REPO / "tacex_amd" / "csrc" / "lens_model.hip").exists()
    assert "-ffp-contract=off" in _build.FILE_FLAGS["lens_model.hip"]
    # one copy of the camera arithmetic: both units include the shared device header and neither defines camera_group itself
    for unit in ("camera_model.hip", "lens_model.hip"):
        src = (REPO / "tacex_amd" / "csrc" / unit).read_text()
        assert '#include "camera_group.h"' in src and "void camera_group(" not in src
    assert "void camera_group(" in (REPO / "tacex_amd" / "csrc" / "camera_group.h").read_text()


def test_exported_from_the_package():
    import tacex_amd

    assert {"LensProfile", "TactileLensModel"} <= set(tacex_amd.__all__)
    assert tacex_amd.TactileLensModel.__module__ == "tacex_amd.lens_model"
    assert hasattr(tacex_amd.GelSightSensor, "lens_image") and hasattr(tacex_amd.GelSightSensor, "camera_image")


# arguments of valid calls (the pointers are never dereferenced: every case below is refused before any GPU call)
_OK = dict(rgb=0x1000, lprof=0x2000, LP=1, lids=None, prof=0x4000, P=1, ids=None, seed=1, off=0, call=0, out=0x3000, dt=0, B=1, H=4, W=4)
_COMMON = [(dict(rgb=None), b"rgb_dev"), (dict(out=None), b"out_dev"), (dict(B=0), b"num_frames"), (dict(B=-1), b"num_frames"),
           (dict(H=0), b"height"), (dict(H=-2), b"height"), (dict(W=0), b"width"), (dict(W=-5), b"width"),
           (dict(out=0x1000), b"out_dev == rgb_dev")]
_ID = lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None  # noqa: E731


@pytest.mark.parametrize("change, word", _COMMON + [(dict(lprof=None), b"profiles_dev"), (dict(LP=0), b"num_profiles"),
                                                    (dict(LP=-3), b"num_profiles")], ids=_ID)
def test_lens_model_refusals_return_2_and_name_the_argument(change, word):
    lib, _lib = _lib_and_module()
    a = dict(_OK, **change)
    rc = lib.tacex_lens_model(a["rgb"], a["lprof"], a["LP"], a["lids"], a["out"], a["B"], a["H"], a["W"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_lens_model" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "tacex_lens_model")


@pytest.mark.parametrize("change, word", _COMMON + [
    (dict(lprof=None), b"lens_profiles_dev"), (dict(LP=0), b"num_lens_profiles"), (dict(prof=None), b"null profiles_dev"),
    (dict(P=0), b": num_profiles"), (dict(dt=2), b"out_dtype"), (dict(dt=-1), b"out_dtype"), (dict(dt=1, out=0x1000), b"out_dev == rgb_dev"),
], ids=_ID)
def test_lens_camera_model_refusals_return_2_and_name_the_argument(change, word):
    lib, _ = _lib_and_module()
    a = dict(_OK, **change)
    rc = lib.tacex_lens_camera_model(a["rgb"], a["lprof"], a["LP"], a["lids"], a["prof"], a["P"], a["ids"], a["seed"], a["off"], a["call"],
                                     a["out"], a["dt"], a["B"], a["H"], a["W"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_lens_camera_model" in msg and word in msg, msg


_PT_OK = dict(xy=0x1000, prof=0x2000, P=1, ids=None, out=0x1000, B=1, N=5, H=4, W=4)  # (out == xy is allowed)


@pytest.mark.parametrize("change, word", [
    (dict(xy=None), b"xy_dev"), (dict(prof=None), b"profiles_dev"), (dict(out=None), b"out_dev"), (dict(P=0), b"num_profiles"),
    (dict(B=0), b"num_frames"), (dict(N=0), b"num_points"), (dict(N=-1), b"num_points"), (dict(H=0), b"height"), (dict(W=0), b"width"),
], ids=_ID)
def test_lens_points_refusals_return_2_and_name_the_argument(change, word):
    lib, _ = _lib_and_module()
    a = dict(_PT_OK, **change)
    rc = lib.tacex_lens_points(a["xy"], a["prof"], a["P"], a["ids"], a["out"], a["B"], a["N"], a["H"], a["W"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_lens_points" in msg and word in msg, msg


def test_lens_profile_row_layout_and_errors():
    from tacex_amd import LensProfile, TactileLensModel
    from tacex_amd._lib import TacexHipError

    kw = dict(k1=-0.15, k2=0.03, p1=0.01, p2=-0.02, rotation_deg=1.5, scale=1.02, shear=0.01, shift_px=(2.5, -1.0), centre_px=(4.0, -3.0),
              vignette=(-0.25, -0.05), softness=(0.5, 1.5))
    row = LensProfile(**kw).row()
    assert row.dtype == np.float32 and row.shape == (16,)
    np.testing.assert_array_equal(row, profile_row(**kw))
    np.testing.assert_array_equal(row[[0, 1, 2, 3]], np.float32([-0.15, 0.03, 0.01, -0.02]))
    np.testing.assert_array_equal(row[8:16], np.float32([2.5, -1.0, 4.0, -3.0, -0.25, -0.05, 0.5, 1.5]))
    c, s = np.cos(np.deg2rad(1.5)), np.sin(np.deg2rad(1.5))
    A = 1.02 * np.array([[c, -s], [s, c]]) @ np.array([[1, 0.01], [0, 1]])
    np.testing.assert_allclose(row[4:8].reshape(2, 2), A - np.eye(2), rtol=0, atol=1e-7)
    np.testing.assert_array_equal(LensProfile.identity().row(), np.zeros(16, dtype=np.float32))
    np.testing.assert_array_equal(LensProfile(matrix=[[-1, 0], [0, -1]]).row()[4:8], np.float32([-2, 0, 0, -2]))
    np.testing.assert_array_equal(LensProfile(matrix=[[1.5, 0.25], [-0.5, 2]], scale=-1).row()[4:8], np.float32([0.5, 0.25, -0.5, 1]))  # scale unused
    for k in profile_set(64):
        np.testing.assert_array_equal(LensProfile(**k).row(), profile_row(**k))
    for bad in (dict(k1=float("nan")), dict(p2=float("inf")), dict(scale=0.0), dict(scale=-1.0), dict(softness=(-0.1, 0)), dict(softness=(0, -1)),
                dict(shift_px=(1, 2, 3)), dict(vignette=0.5), dict(centre_px=(0, float("nan"))), dict(matrix=np.eye(3)),
                dict(matrix=[[1, float("inf")], [0, 1]]), dict(rotation_deg=float("nan")), dict(k2=1e39)):
        with pytest.raises(ValueError):
            LensProfile(**bad).row()
    ident = [LensProfile.identity()]
    with pytest.raises(ValueError):
        TactileLensModel([], 2, "cuda")
    with pytest.raises(ValueError):
        TactileLensModel([np.zeros(16)], 2, "cuda")
    with pytest.raises(ValueError):
        TactileLensModel(ident, 0, "cuda")
    with pytest.raises(TacexHipError):  # no CPU path
        TactileLensModel(ident, 2, "cpu")


# ---- known answers on the restatement ---------------------------------------------------------------------------------------------
SIZES = [(6, 8), (7, 9), (1, 1), (5, 12)]  # even, odd, one pixel, mixed


def _rgb(H, W, seed=0):
    return np.random.default_rng(seed).random((H, W, 3), dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("H, W", SIZES)
def test_identity_row_returns_the_input_bit_for_bit(H, W):
    x = _rgb(H, W)
    x[0, 0, 0] = 0.0
    np.testing.assert_array_equal(_bits(lens_frame(x, profile_row())), _bits(x))
    u, v, _ = source_positions(profile_row(), H, W)
    np.testing.assert_array_equal(u, np.broadcast_to(np.arange(W, dtype=np.float32), (H, W)))
    np.testing.assert_array_equal(v, np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W)))


@pytest.mark.parametrize("H, W", SIZES)
def test_whole_pixel_shift_is_exact_with_edge_replicate(H, W):
    x = _rgb(H, W, 1)
    got = lens_frame(x, profile_row(shift_px=(3, -2)))
    ii = np.clip(np.arange(H) - 2, 0, H - 1)
    jj = np.clip(np.arange(W) + 3, 0, W - 1)
    np.testing.assert_array_equal(_bits(got), _bits(x[ii][:, jj]))


@pytest.mark.parametrize("H, W", SIZES)
def test_minus_identity_is_a_half_turn_about_the_frame_centre(H, W):
    """A = -I, E = -2 I: u = j - 2 (j + 0.5 - W/2) = W - 1 - j and v = H - 1 - i, exactly (half-integers are exact in float32): a half
    turn about ((W-1)/2, (H-1)/2) - the centre pixel's centre for odd sizes, the corner shared by the four middle pixels for even."""
    x = _rgb(H, W, 2)
    row = profile_row(matrix=[[-1, 0], [0, -1]])
    u, v, _ = source_positions(row, H, W)
    np.testing.assert_array_equal(u[0], np.float32(W - 1) - np.arange(W, dtype=np.float32))
    np.testing.assert_array_equal(v[:, 0], np.float32(H - 1) - np.arange(H, dtype=np.float32))
    got = lens_frame(x, row)
    np.testing.assert_array_equal(_bits(got), _bits(x[::-1, ::-1]))
    if H % 2 and W % 2:
        np.testing.assert_array_equal(got[H // 2, W // 2], x[H // 2, W // 2])  # the centre pixel stays
    np.testing.assert_array_equal(_bits(lens_frame(got, row)), _bits(x))  # two half turns


def test_pure_vignetting_gives_the_gain():
    H, W, v1, v2 = 24, 32, -0.25, -0.05
    ones = np.ones((H, W, 3), dtype=np.float32)
    got = lens_frame(ones, profile_row(vignette=(v1, v2)))
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    r2 = ((j + 0.5 - W / 2) * 2 / W) ** 2 + ((i + 0.5 - H / 2) * 2 / W) ** 2
    g = np.clip(1 + v1 * r2 + v2 * r2 * r2, 0, 1)
    np.testing.assert_allclose(got, np.repeat(g[..., None], 3, -1), rtol=0, atol=2e-7)  # a handful of float32 roundings near 1
    assert got.max() < 1 and got[H // 2, W // 2, 0] == got.max() and got[0, 0, 0] == got.min() == got[-1, -1, 0] == got[0, -1, 0]
    x = _rgb(H, W, 3)
    np.testing.assert_array_equal(_bits(lens_frame(x, profile_row(vignette=(v1, v2)))), _bits(got * x))  # out = g * colour
    # the clamps: a strong fall-off reaches 0, a positive coefficient cannot brighten
    assert lens_frame(ones, profile_row(vignette=(-2.0, 0.0)))[0, 0, 0] == 0.0
    np.testing.assert_array_equal(lens_frame(ones, profile_row(vignette=(0.5, 0.0))), ones)


def test_softness_keeps_a_constant_and_spreads_an_impulse_with_unit_sum():
    H, W = 15, 17
    for soft in ((1.0, 0.0), (0.5, 1.5), (0.3, 0.0), (9.0, 0.0)):
        flat = lens_frame(np.full((H, W, 3), 0.625, dtype=np.float32), profile_row(softness=soft))
        np.testing.assert_allclose(flat, 0.625, rtol=0, atol=1e-6)
    x = np.zeros((H, W, 3), dtype=np.float32)
    x[7, 8] = 1.0
    for side in (1.0, 0.3, 2.5, 4.0, 9.0):  # a box of the same side everywhere (b2 = 0); 9 is clamped to 4
        got = lens_frame(x, profile_row(softness=(side, 0.0)))
        assert abs(float(got[..., 0].sum(dtype=np.float64)) - 1) <= 1e-6
        assert got.max() < 1 and np.count_nonzero(got[..., 0]) >= 4
        r = int(np.ceil(min(side, 4.0) / 2)) + 1
        outside = got.copy()
        outside[7 - r:7 + r + 1, 8 - r:8 + r + 1] = 0
        assert not outside.any()
    np.testing.assert_array_equal(lens_frame(x, profile_row(softness=(9.0, 0.0))), lens_frame(x, profile_row(softness=(4.0, 0.0))))
    # softness (0, 0) is the one-tap branch: the impulse stays where it is
    np.testing.assert_array_equal(lens_frame(x, profile_row()), x)


def test_the_sign_of_k1_moves_a_corner_pixels_source_along_the_radius():
    """By the formulas of the header the source of output pixel p lies at p + (W/2) xn (k1 r2): k1 < 0 pulls a corner pixel's source
    TOWARDS the optical centre (the frame shows its middle stretched outwards), k1 > 0 pushes it outwards, past the frame's edge."""
    H, W = 24, 32
    cx, cy = (W - 1) / 2, (H - 1) / 2
    for k1, sign in ((-0.15, -1), (0.15, +1)):
        u, v, _ = source_positions(profile_row(k1=k1), H, W)
        for (i, j) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            r_out = np.hypot(j - cx, i - cy)
            r_src = np.hypot(float(u[i, j]) - cx, float(v[i, j]) - cy)
            assert sign * (r_src - r_out) > 1.0, (k1, i, j, r_src, r_out)
            # along the radius: source, pixel and centre are collinear
            assert abs((float(u[i, j]) - cx) * (i - cy) - (float(v[i, j]) - cy) * (j - cx)) < 1e-3
        assert abs(float(u[H // 2, W // 2]) - W // 2) < 1e-3  # the middle hardly moves
    assert source_positions(profile_row(k1=0.15), H, W)[0][0, 0] < 0  # outside the frame: edge replicate serves it


@pytest.mark.parametrize("H, W", [(240, 320), (48, 64), (37, 53)])
def test_points_followed_by_the_forward_displacement_return_to_the_start(H, W):
    """q = lens_points(p) solves q + displacement(q) = p: within 1e-6 px for every profile of the test set, over the whole frame, its
    corners included (where the radial term contracts slowest)."""
    xs, ys = np.meshgrid(np.linspace(0, W - 1, 23), np.linspace(0, H - 1, 19))
    p = np.stack([xs, ys], -1)
    for n, kw in enumerate(profile_set(W), 1):
        row = profile_row(**kw)
        q = lens_points(p, row, H, W)
        assert q.dtype == np.float64 and q.shape == p.shape
        ou, ov = displacement(row, q[..., 0], q[..., 1], H, W)
        err = np.hypot(q[..., 0] + ou - xs, q[..., 1] + ov - ys).max()
        print(f"profile {n} at {H} x {W}: max |q + d(q) - p| = {err:.3e} px, largest move {np.abs(q - p).max():.2f} px")
        assert err <= 1e-6
    np.testing.assert_array_equal(lens_points(p, profile_row(), H, W), p)
    np.testing.assert_array_equal(lens_points(p, profile_row(shift_px=(3, -2)), H, W), p - np.array([3.0, -2.0]))


def test_the_float64_displacement_is_the_float32_one_of_the_image():
    """the points use the image's formulas: at pixel centres the two agree to float32 rounding"""
    H, W = 37, 53
    for kw in profile_set(W)[:5]:
        row = profile_row(**kw)
        u, v, _ = source_positions(row, H, W)
        j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        ou, ov = displacement(row, j, i, H, W)
        assert np.abs(u - (j + ou)).max() < 5e-5 and np.abs(v - (i + ov)).max() < 5e-5
