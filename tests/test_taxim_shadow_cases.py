"""CPU: every case of tests/taxim_shadow_cases.py is what it claims to be, from the float64 oracle alone - dilation window, ray steps
(and that exchanging them matters), shadow blur size, the threads beyond the frame, a ring and shadow samples on every contact frame
(none without contact / without a ring), rays that leave the frame on each side and samples on its border, a curved gel map that
moves the height bins, and the conditioning of the GPU test's protocol: share of the same-bin field and the RGB bound per case."""
import subprocess

import numpy as np
import pytest

import taxim_route_cases as rc
import taxim_shadow_cases as sc
from conftest import REPO

RING_MIN = 20


@pytest.fixture(scope="module")
def calib_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("shadow_calib")


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_case_table(case, calib_dir, calib_tmp):
    ref = sc.reference(case, calib_dir, calib_tmp)
    o, sh, t, s = ref["oracle"], ref["shadow"], ref["tables"], ref["samples"]
    H, W = case.shape
    # ---- the table's entries, from the calibration folder the library reads ----
    assert tuple(sh["win"]) == case.win
    assert (sh["blur_kw"], sh["blur_kh"]) == case.sblur_k
    assert t.ksize_w[-1] == t.ksize_h[-1] == case.final_k
    assert H * W % 256 == case.rem
    if case.step is not None:
        np.testing.assert_allclose((sh["step_x"], sh["step_y"]), case.step_xy, rtol=1e-12)
        np.testing.assert_allclose(o.p.rel("shadow_step", case.shape), case.step, rtol=1e-12)
    if case.attach is None:
        assert ref["folder"] == calib_dir
    assert (case.win == (0, 0, 0, 0)) == (not case.ring)
    # ---- frames ----
    assert ref["hm"].shape == (len(case.frames), H, W) and case.frames[-1] != "none"
    rc.check_frame_properties(case, ref["M"])  # (corner and seam contacts keep their shrunken mask, on the dome too)
    ring, hit = ref["ring"], np.isfinite(ref["shadow_map"]).any(-1)
    for b, kind in enumerate(case.frames):
        if kind == "none":
            assert ref["indent"][b] == 0 and not ref["M"][b].any()
        else:
            assert ref["M"][b].sum() >= 10, (case.name, kind)
        if kind == "none" or not case.ring:
            assert not ring[b].any() and not hit[b].any(), (case.name, kind)
        else:
            assert ring[b].sum() >= RING_MIN and hit[b].sum() >= RING_MIN, (case.name, kind, int(ring[b].sum()), int(hit[b].sum()))
    if not case.ring:
        assert len(s["bi"]) == 0
        return
    # ---- rays leave the frame on every side, and samples land on its border ----
    sx, sy = s["sx"], s["sy"]
    off = {"left": int((sx < 0).sum()), "right": int((sx >= W).sum()), "top": int((sy < 0).sum()), "bottom": int((sy >= H).sum())}
    on_border = int((s["valid"] & ((sx == 0) | (sx == W - 1) | (sy == 0) | (sy == H - 1))).sum())
    print(f"{case.name}: ring {ring.sum((1, 2)).tolist()} shadowed px {hit.sum((1, 2)).tolist()} samples off the frame {off} on its border {on_border}")
    assert min(off.values()) >= 1 and on_border >= 1, (off, on_border)
    np.testing.assert_array_equal(s["inside"], (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H))
    # ---- unequal steps: exchanging them changes which pixels are shadowed ----
    if case.unequal_steps:
        swapped, _ = o.shadow_map(ref["Z32"], ref["M"], steps_wh=(case.step[1], case.step[0]))
        assert not np.array_equal(np.isfinite(swapped), np.isfinite(ref["shadow_map"]))
    # ---- curved gel: the map is in the height bin ----
    if case.gel == "curved":
        assert np.abs(o.gel).max() > 0.1
        inside = (s["hraw"] >= 0) & (s["hraw"] < s["max_h"])
        assert len(np.unique(s["hraw"][inside])) >= 3
        flat = o.shadow_samples(ref["Z32"], ref["M"], ref["gdir"], gel=np.zeros_like(o.gel))
        assert (flat["hidx"] != s["hidx"]).any()
    else:
        assert not o.gel.any()


def test_table_covers_what_it_is_for():
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)
    assert not any(c.shape in ((240, 320), (480, 640)) for c in sc.CASES)
    ring = [c for c in sc.CASES if c.ring]
    assert any(c.rem for c in ring) and any(c.W % 4 for c in ring) and any(c.H % 2 for c in ring)
    wins = {c.win for c in sc.CASES}
    assert {(1, 2, 1, 2), (0, 0, 1, 2), (1, 2, 0, 0), (4, 4, 4, 4), (0, 0, 0, 0)} <= wins
    assert {c.sblur_k for c in sc.CASES} >= {(3, 3), (5, 3), (3, 5), (5, 5)}
    uneq = [c for c in sc.CASES if c.unequal_steps]
    assert any(c.step[0] < c.step[1] for c in uneq) and any(c.step[0] > c.step[1] for c in uneq)
    assert any(c.gel == "curved" and c.unequal_steps for c in sc.CASES) and any(c.gel == "curved" and not c.unequal_steps for c in sc.CASES)
    assert any(c.H * c.W * 4 % 256 for c in sc.CASES), "a frame whose image is no multiple of 256 bytes"
    assert any(51 * max(c.step) > max(c.shape) for c in ring if c.step), "a ray longer than the frame"
    many = sc.BY_NAME[sc.MANY_FRAMES_CASE]
    assert sc.MANY_FRAMES_B * many.H * many.W * 3 > 65536 * 256 and sc.MANY_FRAMES_B % 3 == 0
    assert set(sc.BOUNDS) == set(sc.BY_NAME)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_protocol_conditioning_and_bounds(case, calib_dir, calib_tmp):
    """The GPU test compares RGB where the whole footprint of the two image blurs was shaded from the same polynomial record on both
    sides.  With a NumPy float32 restatement of the kernel's normals (exact atan / atan2 in place of the fast ones) that field must
    cover >= 95 % of all pixels and >= 90 % of the shadowed ones: conditions on the case, not figures to relax.  The RGB bound
    max(1e-6, 4 x max|f32 - f64|) of the oracle's own shadow branch on that field is what sc.BOUNDS stores."""
    ref = sc.reference(case, calib_dir, calib_tmp)
    bound, share_all, share_hit = sc.measure_bound(case, ref)
    print(f"{case.name}: RGB bound {bound:.3e} (stored {sc.bound(case):.3e}); field covers {share_all:.2%} of all, {share_hit:.2%} of the shadowed pixels")
    assert share_all >= 0.95
    if case.ring:
        assert share_hit >= 0.90
    assert sc.bound(case) == pytest.approx(bound, rel=0.05)
    assert 1e-6 <= sc.bound(case) <= 1e-5


def test_shadow_layout_of_the_small_frames(tmp_path):
    """The workspace invariants of test_taxim_workspace_layout.py (same program, same checks) for 9x12 and 33x70 frames with B = 1 and 5:
    images of 432, 2160, 9240 and 46 200 bytes, none a multiple of 256."""
    from test_taxim_workspace_layout import _compiler

    exe = tmp_path / "taxim_layout_check"
    cmd = _compiler() + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{REPO / 'tacex_amd' / 'csrc'}",
                         str(REPO / "tests" / "taxim_layout_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    args = [str(v) for H, W in ((9, 12), (33, 70)) for B in (1, 5) for v in (H, W, B)]
    assert all(H * W * B * 4 % 256 for H, W in ((9, 12), (33, 70)) for B in (1, 5))
    r = subprocess.run([str(exe)] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "20 layouts checked, 0 failures" in r.stdout, r.stdout
