"""Relief tile library on the CPU: the NumPy restatement of `tacex_height_map_from_relief` (tests/relief_source_ref.py) against the
analytic-indenter oracle and against the properties the contract promises, the tile generators, the constructor's refusals and the
C ABI's argument checks (no GPU call is made)."""
import ctypes as C
import re

import numpy as np
import pytest
import relief_source_ref as R
from conftest import REPO

F32 = np.float32
PIX = 0.0295


def _identity_pose(B=1, press=0.5, gain=1.0):
    p = np.zeros((B, 16), F32)
    p[:, 0] = p[:, 4] = 1.0
    p[:, 6], p[:, 12] = press, gain
    return p


def _tile(Th=5, Tw=7, amp=0.2):
    j, i = np.meshgrid(np.arange(Th), np.arange(Tw), indexing="ij")
    return (amp * (((3 * i + 5 * j) % 11) / 10.0)).astype(F32)


def test_zero_tile_on_a_sphere_is_the_sphere_indenter():
    """The one cross-check against an independent model: within the 2e-5 mm the indenter test allows for float32 sqrt round-off."""
    from oracle.indenter_oracle import indenter_height_map

    H, W, r = 240, 320, 60.0
    tex, ti, tf = R.library([(np.zeros((1, 1), F32), PIX, True, None)])
    pose = R.pose_rows(tf, [0], 150.0, 110.0, 0.0, 1.0, pixmm=PIX, carrier=1, radius_mm=r * PIX)
    hm = R.height_map(tex, ti, tf, None, pose, H, W)
    want = indenter_height_map(np.array([[0, 150, 110, r, 0, 1.0, 0, 0]], F32), H, W, PIX)
    err = float(np.abs(hm - want).max())
    print("sphere carrier against the indenter oracle: max |diff| =", err, "mm")
    assert (hm < 28.5).sum() > 1000 and (hm == 29.0).sum() > 1000
    assert err <= 2e-5


def test_plane_carrier_with_a_constant_tile_is_flat():
    tex, ti, tf = R.library([(np.full((4, 6), 0.3, F32), 0.02, True, None)])
    pose = R.pose_rows(tf, [0], 17.3, 9.1, 0.37, 0.625, pixmm=PIX, scale=1.3, shift=(2.25, -7.5))
    for samples in (1, 4):
        hm = R.height_map(tex, ti, tf, None, pose, 24, 32, samples=samples)
        assert np.array_equal(hm, np.full((1, 24, 32), F32(28.5) - F32(0.625), F32))


def test_identity_pose_returns_the_texels_at_integer_pixels():
    t = _tile()
    tex, ti, tf = R.library([(t, 0.02, True, None)])
    pose = _identity_pose(press=0.5, gain=1.5)
    hm = R.height_map(tex, ti, tf, None, pose, 12, 16)[0]
    j, i = np.meshgrid(np.arange(12), np.arange(16), indexing="ij")
    want = (F32(28.5) - F32(0.5)) + F32(1.5) * (t.max() - t[j % 5, i % 7])
    assert np.array_equal(hm, want.astype(F32))


def test_a_shift_by_one_period_changes_nothing():
    tex, ti, tf = R.library([(_tile(), 0.02, True, None)])
    pose = R.pose_rows(tf, [0], 8.0, 6.0, 0.0, 0.5, pixmm=0.02 * 0.25, shift=(0.5, 0.25))  # k = 1/4: u, v and the sums are exact
    base = R.height_map(tex, ti, tf, None, pose, 12, 16)
    moved = pose.copy()
    moved[:, 13] += 7
    moved[:, 14] += 5
    assert np.array_equal(R.height_map(tex, ti, tf, None, moved, 12, 16), base)
    assert len(np.unique(base)) > 10


def test_four_samples_on_a_constant_tile_equal_one():
    tex, ti, tf = R.library([(np.full((3, 3), 0.1, F32), 0.02, True, None)])
    pose = R.pose_rows(tf, [0], 10.0, 10.0, 0.2, 0.5, pixmm=PIX)
    a, b = (R.height_map(tex, ti, tf, None, pose, 20, 24, samples=s) for s in (1, 4))
    assert np.array_equal(a, b)


def test_a_hole_empties_exactly_the_pixels_whose_taps_touch_it():
    t = _tile(8, 8)
    t[3, 5] = -np.inf
    tex, ti, tf = R.library([(t, 0.02, False, None)])
    pose = _identity_pose()
    pose[:, 2] = pose[:, 5] = 0.5  # u = x + 0.5: every in-range sample has four distinct taps
    hm = R.height_map(tex, ti, tf, None, pose, 8, 8)[0]
    empty = hm == F32(29.0)
    want = np.zeros((8, 8), bool)
    want[2:4, 4:6] = True  # taps (j0, j0+1) x (i0, i0+1) with j0 = y, i0 = x touch texel (3, 5)
    want[7, :] = want[:, 7] = True  # u = 7.5 lies outside a tile that does not wrap
    assert np.array_equal(empty, want)
    pose[:, 2] = pose[:, 5] = 0.0  # integer positions: the taps (x+1, y+1) carry weight 0 but are still touched
    hm = R.height_map(tex, ti, tf, None, pose, 8, 8)[0]
    want = np.zeros((8, 8), bool)
    want[2:4, 4:6] = True
    assert np.array_equal(hm == F32(29.0), want)


def test_frame_outputs_follow_the_depth_pass_reference():
    import depth_pass_ref as dref

    tex, ti, tf = R.library([(np.zeros((1, 1), F32), PIX, True, None)])
    pose = R.pose_rows(tf, [0, 0], [20.0, 5.0], [12.0, 20.0], 0.0, [0.8, 5.0], pixmm=PIX, carrier=1, radius_mm=[6 * PIX, 4 * PIX])
    hm = R.height_map(tex, ti, tf, None, pose, 24, 32)
    fmin, indent, rows = R.frame_outputs(hm, dref.GELPAD_H, dref.GELPAD_DMIN)
    assert dref.columns_route(24, 32) == "exact"
    want = dref.reference_mm(hm)
    assert np.array_equal(fmin, want[0]) and np.array_equal(indent, want[1]) and np.array_equal(rows, want[2])
    assert fmin[1] < 24.0 and indent[1] == F32(4.5)


def test_generators():
    from tacex_amd import ReliefTile
    from tacex_amd.utils import relief_tiles as T

    made = {"weave": T.weave(), "knurl": T.knurl(), "grooves": T.grooves(), "dots": T.dots(), "disc_stamp": T.disc_stamp(),
            "from_array": T.from_array([[0.0, 0.1], [0.2, -np.inf]], 0.05, wrap=False, anchor=(0.0, 1.0))}
    again = {"weave": T.weave(), "knurl": T.knurl(), "grooves": T.grooves(), "dots": T.dots(), "disc_stamp": T.disc_stamp()}
    for name, t in made.items():
        assert isinstance(t, ReliefTile) and t.height_mm.dtype == np.float32 and t.height_mm.ndim == 2, name
        h = t.height_mm
        assert not np.isnan(h).any() and not np.isposinf(h).any(), name
        assert t.top_mm == float(h[np.isfinite(h)].max()) and t.row()[1] == F32(t.top_mm), name
        if name in again:
            assert np.array_equal(h, again[name].height_mm), name
        if name in ("disc_stamp", "from_array"):
            assert np.isneginf(h).any() and not t.wrap, name
        else:
            assert np.isfinite(h).all() and t.wrap and h.min() >= 0 and np.ptp(h) > 0.01, name
    d = made["disc_stamp"].height_mm
    c = (d.shape[0] - 1) / 2
    assert np.isfinite(d[int(c), int(c)]) and np.isneginf(d[0, 0]) and np.isneginf(d[-1, -1])
    assert made["from_array"].row().tolist() == [F32(0.05), F32(0.2), 0.0, 1.0]
    assert T.weave().row().tolist()[2:] == [31.5, 31.5]  # the anchor defaults to the tile centre


def test_constructor_refusals():
    from tacex_amd import ReliefHeightMapSource, ReliefTile, _lib

    ok = ReliefTile(np.zeros((2, 2), F32), 0.02)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="NaN or \\+inf"):
            ReliefTile(np.array([[0.0, bad]], F32), 0.02)
    poisoned = ReliefTile(np.zeros((2, 2), F32), 0.02)
    poisoned.height_mm = np.array([[np.nan]], F32)  # (written after the tile was made: the source looks again)
    with pytest.raises(ValueError, match="NaN or \\+inf"):
        ReliefHeightMapSource([poisoned], 2, "cpu")
    with pytest.raises(ValueError, match="no finite texel"):
        ReliefTile(np.full((2, 2), -np.inf, F32), 0.02)
    with pytest.raises(ValueError, match="rows, cols"):
        ReliefTile(np.zeros((4,), F32), 0.02)
    for pitch in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="pitch_mm"):
            ReliefTile(np.zeros((2, 2), F32), pitch)
    with pytest.raises(ValueError, match="anchor"):
        ReliefTile(np.zeros((2, 2), F32), 0.02, anchor=(1.0,))
    with pytest.raises(ValueError, match="non-empty sequence"):
        ReliefHeightMapSource([], 2, "cpu")
    with pytest.raises(ValueError, match="samples = 3"):
        ReliefHeightMapSource([ok], 2, "cpu", samples=3)
    with pytest.raises(ValueError, match="num_frames"):
        ReliefHeightMapSource([ok], 0, "cpu")
    with pytest.raises(_lib.TacexHipError, match="no CPU fallback"):  # every ValueError comes before the device is looked at
        ReliefHeightMapSource([ok], 2, "cpu")


def test_symbol_header_and_exports():
    import tacex_amd
    from tacex_amd import _build, _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    assert re.search(r"\bint\s+tacex_height_map_from_relief\s*\(", hdr)
    res, args = _lib.SIGNATURES["tacex_height_map_from_relief"]
    assert res is C.c_int and len(args) == 19 and args[-2] is C.c_int and args[-1] is C.c_void_p
    assert hasattr(_lib.load_library(), "tacex_height_map_from_relief")
    assert "relief_source.hip" in _build.SOURCES and "-ffp-contract=off" in _build.FILE_FLAGS["relief_source.hip"]
    assert tacex_amd.ReliefHeightMapSource.writes_frame_rows is True and "ReliefTile" in tacex_amd.__all__


def test_the_entry_point_refuses_before_any_gpu_call():
    from tacex_amd import _lib

    lib = _lib.load_library()
    one = 16  # any non-null, 16-byte aligned address: a refused call dereferences nothing
    good = dict(texels=one, ti=one, tf=one, P=1, ids=0, pose=one, hm=one, fmin=one, indent=0, rows=0, B=2, H=8, W=16, samples=1)

    def call(**kw):
        a = good | kw
        return lib.tacex_height_map_from_relief(a["texels"], a["ti"], a["tf"], a["P"], a["ids"], a["pose"], 28.5, 29.0, 0.0045, 0.024,
                                                a["hm"], a["fmin"], a["indent"], a["rows"], a["B"], a["H"], a["W"], a["samples"], 0)

    cases = [(dict(texels=0), "null texels_dev"), (dict(ti=0), "null tiles_i_dev"), (dict(tf=0), "null tiles_f_dev"),
             (dict(pose=0), "null pose_dev"), (dict(hm=0), "null hm_mm_dev"), (dict(fmin=0), "null frame_min_dev"),
             (dict(P=0), "num_tiles = 0"), (dict(B=0), "num_frames = 0"), (dict(H=0), "height = 0"), (dict(W=-4), "width = -4"),
             (dict(W=17), "width = 17"), (dict(H=2049), "2049 x 16"), (dict(W=2052), "8 x 2052"), (dict(H=4096), "4096 x 16"),
             (dict(samples=2), "samples = 2"), (dict(samples=0), "samples = 0"), (dict(hm=20), "16-byte aligned")]
    for kw, text in cases:
        assert call(**kw) == 2, kw
        assert text in lib.tacex_last_error().decode(), (kw, lib.tacex_last_error())
