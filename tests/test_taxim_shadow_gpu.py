"""GPU: the shadow branch (taxim_shadow.hip: shade_raw_kernel, fill_kernel, shadow_ray_kernel, blur_nhwc3_kernel) away from 320x240 /
640x480, against the float64 oracle built from the same calibration folder.

The cases, their calibration folders, frames and the oracle's results come from tests/taxim_shadow_cases.py; the CPU test
tests/test_taxim_shadow_cases.py shows that each case holds what it is there for (threads beyond the frame, a dilation window that
differs along x and y, unequal ray steps, a non-zero gel map in the height bin, rays leaving the frame on every side, ...).
Outputs are rendered into buffers with sentinels in front and behind (test_taxim_routes_gpu.Guarded)."""
import json
import shutil

import numpy as np
import pytest
import torch

import taxim_shadow_cases as sc
from test_taxim_routes_gpu import Guarded

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def calib_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("shadow_calib")


_TAXIM: dict = {}


def _taxim(ref, case):
    """One simulator per case and process (its context holds the case's tables)."""
    from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

    tx = _TAXIM.get(case.name)
    if tx is None:
        tx = _TAXIM[case.name] = Taxim(calib_folder=ref["folder"], backend="hip", device="cuda:0")
        sh = tx.context(case.shape).tables  # the library reads the folder the oracle read
        assert (sh.height, sh.width) == case.shape
    return tx


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # (the shared arrays are read-only: a copy)
    return (t if dtype is None else t.to(dtype)).cuda()


def _shadow_rays(tx, Z, M, g):
    """shadow_rays into a guarded buffer (every element is written: +inf where no sample lands)."""
    out = Guarded(tuple(Z.shape) + (3,))
    tx.shadow_rays(Z, M, g, out=out.t)
    torch.cuda.synchronize()
    return out.check(f"shadow_rays B={Z.shape[0]}")


def _render_shadow(tx, hm, ind, obs_dtype=None):
    """render_direct(with_shadow=True) into guarded buffers: (rgb NHWC, z, mask, obs | None)."""
    B, H, W = hm.shape
    rgb, z, m = Guarded((B, H, W, 3)), Guarded((B, H, W)), Guarded((B, H, W), torch.uint8)
    obs = Guarded((B, 32, 32, 3), obs_dtype) if obs_dtype is not None else None
    tx.render_direct(hm, True, ind, out=rgb.t, z_out=z.t, mask_out=m.t, obs_out=obs.t if obs is not None else None)
    torch.cuda.synchronize()
    tag = f"render with shadow B={B}"
    return (rgb.check(tag + " rgb"), z.check(tag + " z_out"), m.check(tag + " mask_out"),
            obs.check(tag + " obs_out", interior=obs_dtype != torch.uint8) if obs is not None else None)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_ray_march_exact(case, calib_dir, calib_tmp):
    """shadow_ray_kernel on the oracle's own deformed gel, mask and gradient direction: ring pixels, direction and height bins and
    truncated sample pixels are integer work, so the per-pixel / channel minimum map equals the oracle's in every pixel and channel -
    with threads beyond the frame, a window that differs along x and y (or is empty), steps that differ along x and y, a non-zero gel
    map in the height bin and rays that leave the frame on every side."""
    ref = sc.reference(case, calib_dir, calib_tmp)
    tx = _taxim(ref, case)
    Z, M, g = _cuda(ref["Z32"]), _cuda(ref["M"], torch.uint8), _cuda(ref["gdir"])
    got = _shadow_rays(tx, Z, M, g)
    want = ref["shadow_map"]
    np.testing.assert_array_equal(np.isfinite(got.cpu().numpy()), np.isfinite(want))  # the sample index set
    np.testing.assert_array_equal(got.cpu().numpy(), want)                            # ... and the table values that landed there
    assert np.isfinite(want).any() == case.ring
    one = _shadow_rays(tx, Z[-1:], M[-1:], g[-1:])
    assert torch.equal(one[0], got[-1]), "B = 1"


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_shadow_branch_vs_oracle(case, calib_dir, calib_tmp):
    """render_direct(with_shadow=True) from the library's own deformed gel: mask equal to the oracle's, gel within 1e-5 mm and bit-equal to
    deform(); then the RGB against the float64 oracle's shadow branch OF THAT GEL on the same-bin field (every pixel whose footprint of the
    two image blurs was shaded from the same polynomial record on both sides), within the case's bound sc.BOUNDS - computed on the CPU
    from the oracle's float32-vs-float64 difference, never from the kernels.  Frames without contact and the case without a ring cast
    no sample: there the result is the two blurs of shade and background alone."""
    ref = sc.reference(case, calib_dir, calib_tmp)
    o, tx = ref["oracle"], _taxim(ref, case)
    hm, ind = _cuda(ref["hm"]), _cuda(ref["indent"])
    rgb, z, m, _ = _render_shadow(tx, hm, ind)
    z_np, m_np, rgb_np = z.cpu().numpy(), m.cpu().numpy().astype(bool), rgb.cpu().numpy()
    np.testing.assert_array_equal(m_np, ref["M"])
    z_err = float(np.abs(z_np.astype(np.float64) - ref["Z"]).max())
    zd, md = Guarded(tuple(hm.shape)), Guarded(tuple(hm.shape), torch.uint8)
    tx.deform(hm, ind, z_out=zd.t, mask_out=md.t)
    torch.cuda.synchronize()
    assert torch.equal(zd.check("deform z_out"), z) and torch.equal(md.check("deform mask_out"), m)

    want = o.shade_with_shadow(z_np, m_np).astype(np.float64)
    idx = tx.shade(z, return_bins=True)[1].cpu().numpy().astype(np.int64)
    field = sc.same_bin_field(case, idx[..., 0], idx[..., 1], *sc.oracle_bins(o, z_np))
    smap, _ = o.shadow_map(z_np, m_np)
    hit = np.isfinite(smap).any(-1)
    share_all, share_hit = float(field.mean()), float(field[hit].mean()) if hit.any() else float("nan")
    d = np.abs(rgb_np.astype(np.float64) - want)
    err = float(d[field].max())
    cast = float(np.abs(want - o.shade(z_np).astype(np.float64))[field].max())
    print(f"{case.name}: max|Z-Zo| {z_err:.3e} mm; field covers {share_all:.2%} of all, {share_hit:.2%} of the {int(hit.sum())} shadowed pixels; "
          f"max|rgb-oracle| on the field {err:.3e} (bound {sc.bound(case):.1e}), off it {float(d[~field].max()) if (~field).any() else 0.0:.3e}; "
          f"deepest shadow {cast:.3f}")
    assert z_err <= 1e-5
    assert share_all >= 0.95
    if case.ring:
        assert share_hit >= 0.90
    assert err <= sc.bound(case)
    assert rgb_np.min() >= 0.0 and rgb_np.max() <= 1.0
    if case.ring:
        assert cast > 0.05, "shadows are really cast on the compared pixels"
    # frames that cast no sample: two blurs of shade + background
    for b, kind in enumerate(case.frames):
        if kind == "none" or not case.ring:
            assert not hit[b].any()
            if case.gel == "flat" and kind == "none":  # an untouched flat gel has no gradient anywhere: nothing to flip, every pixel counts
                assert field[b].all()
                assert float(d[b].max()) <= sc.bound(case)
    # the last frame alone reproduces the batch's last frame
    rgb1, z1, m1, _ = _render_shadow(tx, hm[-1:], ind[-1:])
    assert torch.equal(rgb1[0], rgb[-1]) and torch.equal(z1[0], z[-1]) and torch.equal(m1[0], m[-1]), "B = 1"


def test_many_frames_take_the_grid_stride_trip(calib_dir, calib_tmp):
    """72 frames of 243x324: B*H*W*3 exceeds the 65 536 blocks x 256 threads fill_kernel's grid is capped at, so its grid-stride loop runs
    a second time.  Three distinct frames, tiled: every frame equals its first copy bit for bit (the minimum is exact and order-free),
    through the ray march alone (the first three also equal the oracle exactly) and through one whole render."""
    case = sc.BY_NAME[sc.MANY_FRAMES_CASE]
    ref = sc.reference(case, calib_dir, calib_tmp)
    tx = _taxim(ref, case)
    pick = [i for i, k in enumerate(case.frames) if k != "none"][:3]
    rep, B = sc.MANY_FRAMES_B // 3, sc.MANY_FRAMES_B
    assert len(pick) == 3 and B * case.H * case.W * 3 > 65536 * 256

    def tile(a, dtype=None):
        return _cuda(a[pick], dtype).repeat((rep,) + (1,) * (a.ndim - 1))

    got = _shadow_rays(tx, tile(ref["Z32"]), tile(ref["M"], torch.uint8), tile(ref["gdir"]))
    want = ref["shadow_map"][pick]
    assert np.isfinite(want).any(axis=(1, 2, 3)).all()
    np.testing.assert_array_equal(got[:3].cpu().numpy(), want)
    assert torch.equal(got.view(rep, 3, *got.shape[1:]), got[:3].unsqueeze(0).expand(rep, -1, -1, -1, -1)), "frames b and b % 3"
    del got
    rgb, z, m, _ = _render_shadow(tx, tile(ref["hm"]), tile(ref["indent"]))
    for t in (rgb, z, m):
        assert torch.equal(t.view(rep, 3, *t.shape[1:]), t[:3].unsqueeze(0).expand(rep, *([-1] * t.dim()))), "frames b and b % 3"
    assert float(rgb.std()) > 0


def test_observation_with_shadow_off_the_tuned_sizes(calib_dir, calib_tmp):
    """`obs_out` with with_shadow=True at 243x324 (the two-pass resize, float4 vertical kernel): the bounds of
    test_policy_observation_with_shadow, against the float64 antialiased resize of the returned RGB instead of torch's float32 one."""
    from oracle.taxim_oracle import resize_bilinear_aa

    case = sc.BY_NAME[sc.MANY_FRAMES_CASE]
    ref = sc.reference(case, calib_dir, calib_tmp)
    tx = _taxim(ref, case)
    hm, ind = _cuda(ref["hm"]), _cuda(ref["indent"])
    plain = _render_shadow(tx, hm, ind)[0]
    for dt in (torch.float32, torch.uint8):
        rgb, _, _, obs = _render_shadow(tx, hm, ind, obs_dtype=dt)
        assert torch.equal(rgb, plain), "the observation must not change the RGB"
        want = np.moveaxis(resize_bilinear_aa(np.moveaxis(rgb.cpu().numpy(), 3, 1), (32, 32)), 1, 3)
        got = obs.cpu().numpy().astype(np.float64)
        if dt == torch.uint8:
            q = np.floor(255.0 * want + 0.5)
            assert np.abs(got - q).max() <= 1.0 and (got == q).mean() > 0.99
        else:
            print(f"observation with shadow 243x324: max|obs - float64 resize| {np.abs(got - want).max():.3e}")
            assert np.abs(got - want).max() < 1e-5
        assert got.std() > 0


def test_shadow_blur_wider_than_the_frame_is_refused(calib_dir, tmp_path):
    """blur_nhwc3_kernel mirrors an index once, which is only valid for a blur radius below the frame size (torch's reflect padding
    refuses anything larger).  tacex_taxim_create checks that for the pyramid and final blur; tacex_taxim_set_shadow took any odd shadow
    blur size, so a 9x12 frame with an 8 px shadow sigma along y (k = 33, radius 16) would have read in front of the image.  It is refused now, before
    anything is launched: error code and message only."""
    from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

    case = sc.BY_NAME["9x12-curved"]
    folder = tmp_path / "calib_wide_shadow_blur"
    shutil.copytree(sc.calib_folder(case, calib_dir, tmp_path), folder)
    params = json.loads((folder / "params.json").read_text())
    params["simulator"]["shadow_blur_sigma_rel"] = [0.55 / case.W, 8.0 / case.H]
    (folder / "params.json").write_text(json.dumps(params))
    tx = Taxim(calib_folder=folder, backend="hip", device="cuda:0")
    ctx = tx.context(case.shape)
    with pytest.raises(ValueError, match=r"tacex_taxim_set_shadow: shadow blur reflect padding \(1, \d+\) must be smaller than the image \(12, 9\)"):
        tx._ensure_shadow(ctx)
    assert not getattr(ctx, "shadow_ready", False)
    with pytest.raises(ValueError, match="shadow blur reflect padding"):  # ... and a render with shadow stops there as well
        tx.render_direct(torch.full((1, 9, 12), 29.0, device="cuda"), True, torch.zeros(1, device="cuda"))
