"""CPU halves of the FOTS kernel tests: the oracle's deformation-level entry against its own step() on the golden sequence,
and the input builders / self-checks of tests/fots_cases.py that tests/test_fots_kernels_gpu.py relies on."""
import math

import numpy as np
import pytest

import fots_cases as fc
from oracle.fots_oracle import FOTSOracle

F32 = np.float32


@pytest.mark.parametrize("res", ["240x320", "480x640"])
def test_step_from_deformation_matches_step_on_golden_sequence(calib_dir, golden_dir, res):
    """step() is step_from_deformation() behind the Taxim oracle: fed the same (Z, M) the two give the same markers, and the
    trajectory state is what the trajectory lists say."""
    from oracle.taxim_oracle import TaximOracle

    H, W = map(int, res.split("x"))
    g = np.load(golden_dir / f"fots_{res}.npz")
    o = TaximOracle(calib_dir, (H, W), "direct")
    steps, B = g["hm"].shape[:2]
    a, b = FOTSOracle(o, B), FOTSOracle(o, B)
    for k in range(steps):
        ma = a.step(g["hm"][k], g["indent"][k], g["theta"][k]).copy()
        Z, M = o.gel_pad_deformation(o.shifted_height_map(g["hm"][k], g["indent"][k]))
        mb = b.step_from_deformation(Z, M, g["indent"][k], g["theta"][k])
        np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(b.marker_data64.astype(F32), mb[:, 1])
        np.testing.assert_array_equal(a.traj_state, b.traj_state)
        if res == "240x320":  # the sequence tests/test_oracle_golden.py pins to the reference
            np.testing.assert_array_equal(b.traj_state[:, 7].astype(np.int64), g["n_contacts"][k])
            np.testing.assert_allclose(mb, g["marker_data"][k], atol=1e-4, rtol=0)
        for e in range(B):
            tr = b.traj[e]
            assert b.traj_state[e, 0] == len(tr)
            if tr:
                np.testing.assert_array_equal(b.traj_state[e, 1:4], np.array(tr[0], F32))
                np.testing.assert_array_equal(b.traj_state[e, 4:7], np.array(tr[-1], F32))


def test_flipping_centroids_are_the_documented_ones():
    """Integer centroids whose shear / twist centre a fused multiply-add truncates to the pixel before (float32 emulation)."""
    cols, rows = fc.flipping_centroids(320), fc.flipping_centroids(240)
    assert cols == [2, 4, 5, 10, 11, 12, 16, 17, 18, 23, 24, 29, 30, 31, 36, 42, 43, 49, 55, 56, 62]
    assert len(rows) == 15 and rows[-6:] == [28, 29, 34, 35, 41, 48]
    assert len(fc.flipping_centroids(640)) == 40 and len(fc.flipping_centroids(480)) == 28
    assert 160 not in cols and 120 not in rows


@pytest.mark.parametrize("shape", [(240, 320), (480, 640)])
def test_integer_centroid_case_has_teeth(shape):
    """With the twist centre one pixel off (what the single-rounding centre gives) the oracle's own markers move by far more
    than the 1e-4 px the kernel is held to: the case can tell the two centres apart."""
    H, W = shape
    case = fc.case_integer_centroids(H, W)
    ref = fc.run_oracle(case)
    fo = fc.make_oracle(case)
    mm = fo.mm
    worst = 0.0
    for k, (Z, M, indent, theta) in enumerate(case.steps):
        fo.step_from_deformation(Z, M, indent, theta)
    for e, (first, last) in enumerate(case.info["seq"]):
        t0, tl = fo.traj[e][0], fo.traj[e][-1]
        two = [fc.centre_two_roundings(t0[0], W / 2), fc.centre_two_roundings(t0[1], H / 2),
               fc.centre_two_roundings(tl[0], W / 2), fc.centre_two_roundings(tl[1], H / 2)]
        one = [fc.centre_single_rounding(t0[0], W / 2), fc.centre_single_rounding(t0[1], H / 2),
               fc.centre_single_rounding(tl[0], W / 2), fc.centre_single_rounding(tl[1], H / 2)]
        assert two == [first[1], first[0], last[1], last[0]]
        flips = [a != b for a, b in zip(two, one)]
        assert flips[0] == flips[1] == (first in case.info["flip"]) and flips[2] == flips[3] == (last in case.info["flip"])
        if flips[2]:  # twist about (tcx - 1, tcy - 1) instead of (tcx, tcy), MM:193-205
            th = np.clip(tl[2] - t0[2], -fc.THETA_MAX, fc.THETA_MAX)
            d = []
            for cx, cy in ((two[2], two[3]), (one[2], one[3])):
                ox, oy = mm.init_x - cx, mm.init_y - cy
                gg = np.exp(-mm.lamb[2] * (ox ** 2 + oy ** 2))
                d.append(((ox * np.cos(th - 1) - oy * np.sin(th)) * gg, (ox * np.sin(th) + oy * np.cos(th - 1)) * gg))
            worst = max(worst, np.abs(d[0][0] - d[1][0]).max(), np.abs(d[0][1] - d[1][1]).max())
    assert worst > 0.5, worst  # ~1 px
    assert mm.mm2pix == fc.MM2PIX and ref[1][2][:, 0].min() == 2 and ref[1][2][:, 7].min() > 0


def test_block100_centroid_is_exact():
    H, W = 240, 320
    for dy, dx in [(-25, 25), (-10.4, 9.99), (-3.7, -0.6), (0.6, 0), (10, -10)]:
        m = fc.block100_at(H, W, 60, 100, dy, dx)
        r, c = np.nonzero(m)
        assert m.sum() == 100
        assert r.sum() == round((60 + 4.5 + dy) * 100) and c.sum() == round((100 + 4.5 + dx) * 100), (dy, dx)


def test_rect_mask_centroid_is_the_pixel():
    m = fc.rect_mask(240, 320, 48, 62, 20, 30)
    r, c = np.nonzero(m)
    assert (r.mean(), c.mean()) == (48.0, 62.0) and m.sum() == 41 * 61


@pytest.mark.parametrize("per_env", [1, 7, 64, 200])
def test_split_partials_recombine(per_env):
    case = fc.case_statistics(30, 40)
    Z, M, _, _ = case.steps[0]
    st = fc.true_stats(Z, M)
    p = fc.split_partials(st, per_env, seed=per_env)
    assert p.shape == (case.B, per_env) and p.dtype.itemsize == 16
    back = fc.combine_partials(p)
    assert back.tobytes() == st.tobytes()
    assert (p["count"] >= 0).all() and (p["sum_row"] >= 0).all() and (p["sum_col"] >= 0).all()
    if per_env > 1:
        idle = (p["count"] == 0) & np.isneginf(p["zmax"])
        assert idle.any() and (~idle).sum() > case.B  # identity records and really split envs both occur


def test_compact_inputs_gather_marker_pixels():
    case = fc.case_grid("edges", 240, 320, 6, 6, *fc.mesh_grid([-1, 0, 57, 161, 319, 320], [-1, 0, 77, 150, 239, 240]), full_mask=True)
    Z, M, _, _ = case.steps[1]
    zp, mp = fc.compact_inputs(Z, M, case.mx, case.my)
    for m in range(36):
        x, y = case.mx[m], case.my[m]
        if 0 <= x < 320 and 0 <= y < 240:
            assert zp[1, m] == Z[1, y, x] and mp[1, m] == M[1, y, x]
        else:
            assert zp[1, m] == 0 and mp[1, m] == 0


def test_case_builders_cover_their_domains():
    """The constructed sequences contain what their names promise, judged on the oracle's own trajectory state."""
    # shear: raw float32 shear in px on both sides of the +-10 clamp, on it, and negative fractions that truncate toward zero
    case = fc.case_shear_domain()
    ref = fc.run_oracle(case)
    ts = ref[1][2]
    raw = np.stack(((ts[:, 4] - ts[:, 1]) * F32(fc.MM2PIX), (ts[:, 5] - ts[:, 2]) * F32(fc.MM2PIX)), 1)
    for ax in (0, 1):
        r = raw[:, ax]
        assert (r < -10.5).any() and (r > 10.5).any() and ((r > -1) & (r < 0)).any() and ((r > 0) & (r < 1)).any()
        assert ((r > -4) & (r < -3)).any() and (np.abs(np.abs(r) - 10) < 1e-3).any() and ((r > 9.9) & (r < 10)).any() and (r == 0).any()
    assert (ts[:, 7] > 0).all() and (ref[2][2][:, 0] == 3).all()
    # twist: raw float32 angle beyond, on and inside the +-60 degree clamp
    case = fc.case_twist_domain()
    ts = fc.run_oracle(case)[1][2]
    d = ts[:, 6] - ts[:, 3]
    tm = F32(fc.THETA_MAX)
    assert (d < -tm).any() and (d > tm).any() and (d == tm).any() and (d == -tm).any() and (np.abs(d) < tm).any() and (d == 0).any()
    assert ((d > tm) & (d < tm + F32(2e-3))).any() and ((d < -tm) & (d > -tm - F32(2e-3))).any()
    # bookkeeping: the five life stories
    case = fc.case_bookkeeping()
    lens = np.stack([r[2][:, 0] for r in fc.run_oracle(case)])
    ncs = np.stack([r[2][:, 7] for r in fc.run_oracle(case)])
    np.testing.assert_array_equal(lens[:, 0], [1, 2, 3, 4, 5, 6])
    np.testing.assert_array_equal(lens[:, 1], [0, 0, 1, 2, 3, 4])
    np.testing.assert_array_equal(lens[:, 2], [1, 2, 0, 1, 2, 3])
    np.testing.assert_array_equal(lens[:, 3], [0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(lens[:, 4], [1, 2, 3, 4, 5, 6])
    assert (ncs[:, 4] == 0).all() and (ncs[:, 0] > 0).all() and (ncs[2:, 1] > 0).all()
    # batch: every kind of env occurs, the last env owns the batch maximum
    case = fc.case_batch(130)
    assert set(case.info["kind"]) == {0, 1, 2, 3, 4}
    for Z, _, _, _ in case.steps:
        assert Z.reshape(130, -1).max(1).argmax() == 129
    assert math.isclose(fc.THETA_MAX, math.pi / 3)
