"""GPU: every Taxim blur route (matrix-core, unrolled band, looped band <384> / <640>, generic) and both fused tails (LDS-tiled,
streaming) away from 320x240 / 640x480, against the float64 oracle built from the same calibration folder.

The cases, their frames and the oracle's results come from tests/taxim_route_cases.py (checked on the CPU by
tests/test_taxim_route_cases.py).  A case first reads the routes back from the library (`Taxim.level_routes`), so that it cannot
pass on another kernel than the one it is there for.  The oracle ("direct") evaluates the blur sequence in float64: the project's
bound |Z - Zo| <= 1e-5 mm holds for every case as it stands, none carries a bound of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import taxim_route_cases as rc
from parity import rgb_rel_err

pytestmark = pytest.mark.gpu

GUARD = 4096            # sentinel elements in front of and behind every output
SENT_F, SENT_U8 = 12345.0, 0xAB  # neither is a value a kernel can produce (RGB in [0,1], gel in mm, mask 0 / 1)


class Guarded:
    """An output tensor between two guard regions of a sentinel value."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.fill = SENT_U8 if dtype == torch.uint8 else SENT_F
        self.buf = torch.full((2 * GUARD + self.n,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def check(self, what, interior=True):
        assert bool((self.buf[:GUARD] == self.fill).all()), f"{what}: stores in front of the buffer"
        assert bool((self.buf[GUARD + self.n:] == self.fill).all()), f"{what}: stores behind the buffer"
        if interior:
            assert not bool((self.t == self.fill).any()), f"{what}: elements never written"
        return self.t


@pytest.fixture(scope="module")
def calib_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("route_calib")


def _render(tx, hm, ind, mode, frames=False, obs_dtype=None):
    """render_direct into guarded buffers: (rgb NHWC, z | None, mask | None, obs | None)."""
    B, H, W = hm.shape
    tx.set_fused_tail((H, W), mode)
    rgb = Guarded((B, H, W, 3))
    z = Guarded((B, H, W)) if frames else None
    m = Guarded((B, H, W), torch.uint8) if frames else None
    obs = Guarded((B, 32, 32, 3), obs_dtype) if obs_dtype is not None else None
    tx.render_direct(hm, False, ind, out=rgb.t, z_out=z.t if frames else None, mask_out=m.t if frames else None,
                     obs_out=obs.t if obs is not None else None)
    torch.cuda.synchronize()
    tag = f"render mode {mode} B={B}"
    return (rgb.check(tag + " rgb"), z.check(tag + " z_out") if frames else None, m.check(tag + " mask_out") if frames else None,
            obs.check(tag + " obs_out", interior=obs_dtype != torch.uint8) if obs is not None else None)


def _deform(tx, hm, ind):
    """deform() at the default tail mode (the renders before it may have left another one set) into guarded buffers."""
    tx.set_fused_tail(tuple(hm.shape[-2:]), 1)
    z, m = Guarded(tuple(hm.shape)), Guarded(tuple(hm.shape), torch.uint8)
    tx.deform(hm, ind, z_out=z.t, mask_out=m.t)
    torch.cuda.synchronize()
    return z.check(f"deform B={hm.shape[0]} z_out"), m.check(f"deform B={hm.shape[0]} mask_out")


def _bins(tx, z):
    return tx.shade(z, return_bins=True)[1]


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_route_case(case, calib_dir, calib_tmp):
    from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

    ref = rc.reference(case, calib_dir, calib_tmp)
    shape, n = case.shape, len(case.frames)
    tx = Taxim(calib_folder=ref["folder"], backend="hip", device="cuda:0")

    # ---- routes: read back from the library's own launch decisions ----
    routes = tx.level_routes(shape)
    assert routes == {"ksize": list(case.ksize), "levels": case.level_routes, "tail": case.tail, "tail_frames": case.tail_frames}, routes
    assert (tx.fots_partials_per_env(shape) == 0) == (case.n_fused == 0)
    for mode, tail in ((2, "tiled" if case.n_fused else "shade"), (0, "shade"), (1, case.tail)):  # (leaves the default mode set)
        tx.set_fused_tail(shape, mode)
        assert tx.level_routes(shape)["tail"] == tail
    assert tx.level_routes(shape) == routes

    hm, ind = torch.from_numpy(ref["hm"].copy()).cuda(), torch.from_numpy(ref["indent"].copy()).cuda()  # (the shared arrays are read-only)

    # ---- deformation against the oracle (z_out / mask_out: the LDS-tiled tail where there is one) ----
    Z, M = _deform(tx, hm, ind)
    np.testing.assert_array_equal(M.cpu().numpy().astype(bool), ref["M"])
    z_err = float(np.abs(Z.cpu().numpy().astype(np.float64) - ref["Z"]).max())
    idx = _bins(tx, Z).cpu().numpy().astype(np.int64)
    same = (idx[..., 0] == ref["im"]) & (idx[..., 1] == ref["idd"])
    strong = ref["strong"]
    share = float(same[strong].mean()) if strong.any() else float("nan")

    # ---- render_direct on the three endings ----
    plain = {mode: _render(tx, hm, ind, mode)[0] for mode in (1, 2, 0)}
    rgbf2, z2, m2, _ = _render(tx, hm, ind, 2, frames=True)
    rgbf0, z0, m0, _ = _render(tx, hm, ind, 0, frames=True)
    # same-bin protocol: an RGB is compared where the bins of the deformed gel IT was shaded from equal the oracle's - the tails' gel
    # is Z (asserted below; the streaming RGB is bit-equal to the tiled one), the unfused levels' gel is z0
    idx0 = _bins(tx, z0).cpu().numpy().astype(np.int64)
    same_of = {1: same, 2: same, 0: (idx0[..., 0] == ref["im"]) & (idx0[..., 1] == ref["idd"])}
    rgb_err = {mode: float(rgb_rel_err(plain[mode].cpu().numpy(), ref["rgb"])[same_of[mode]].max()) for mode in (1, 2, 0)}
    obs_note = "tiled tail fuses the observation" if rc.tiled_obs_fusable(case.H, case.W, case.n_fused) else "observation by two-pass resize (tiled)"
    print(f"{case.name}: routes {'/'.join(routes['levels'])} tail {routes['tail']}|{routes['tail_frames']}; max|Z-Zo| {z_err:.3e} mm; "
          f"same-bin share strong {share:.4%} ({int(strong.sum())} px) all {same.mean():.4%}; rgb rel err same-bin stream/tiled/unfused "
          f"{rgb_err[1]:.2e}/{rgb_err[2]:.2e}/{rgb_err[0]:.2e}; {obs_note if min(shape) >= 64 else 'no observation (frame < 64)'}")
    assert z_err <= 1e-5
    if case.strong:
        assert share >= 0.99
    assert torch.equal(plain[1], plain[2]), "streaming and tiled RGB must be bit-equal"
    assert max(rgb_err.values()) <= 1e-4, rgb_err
    # (the unfused levels are held to the tails directly below - mask, gel, RGB on equal bins; their own share is a figure only)
    print(f"{case.name}: same-bin share strong of the unfused levels {float(same_of[0][strong].mean()) if strong.any() else float('nan'):.4%}")
    assert torch.equal(rgbf2, plain[2]) and torch.equal(rgbf0, plain[0]), "storing the frames must not change the RGB"
    assert torch.equal(z2, Z) and torch.equal(m2, M), "deform and render(z_out) run the same kernels"
    assert torch.equal(m2, m0)
    assert float((z2 - z0).abs().max()) <= 2e-6
    same_b = (_bins(tx, z2) == _bins(tx, z0)).all(-1)
    for mode in (1, 2):
        assert float((plain[mode] - plain[0]).abs()[same_b].max()) <= 2e-6

    # ---- the last frame alone (other strip segmentation, one frame per launch) must reproduce the batch's last frame ----
    if n > 1:
        for mode in (1, 2, 0):
            assert torch.equal(_render(tx, hm[-1:], ind[-1:], mode)[0][0], plain[mode][-1]), f"B = 1, mode {mode}"
        z1, m1 = _deform(tx, hm[-1:], ind[-1:])
        assert torch.equal(z1[0], Z[-1]) and torch.equal(m1[0], M[-1])

    # ---- policy observation (bounds of test_policy_observation_with_shadow) ----
    if min(shape) >= 64:
        for mode in (1, 2, 0):
            for dt in (torch.float32, torch.uint8):
                rgb, _, _, obs = _render(tx, hm, ind, mode, obs_dtype=dt)
                assert torch.equal(rgb, plain[mode]), "the observation must not change the RGB"
                want = torch.nn.functional.interpolate(rgb.movedim(3, 1), size=[32, 32], mode="bilinear", antialias=True).movedim(1, 3)
                if dt == torch.uint8:
                    q = torch.floor(255.0 * want + 0.5)
                    assert float((obs.float() - q).abs().max()) <= 1.0 and float((obs.float() == q).float().mean()) > 0.99, (mode, dt)
                else:
                    assert float((obs - want).abs().max()) < 1e-5, (mode, dt)
                assert float(obs.float().std()) > 0
    tx.set_fused_tail(shape, 1)


_BAND_SKIP_SCRIPT = r'''
import sys
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, REPO); sys.path.insert(0, REPO + "/tests")
import taxim_route_cases as rc
from tacex_amd import _lib
from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

lib, res = _lib.load_library(), {}
for name in rc.BAND_SKIP_CASES:
    case = rc.BY_NAME[name]
    H, W = case.shape
    t = Taxim(calib_folder=rc.calib_folder(case, Path(CALIB), Path(sys.argv[2])), backend="hip", device="cuda:0")
    assert t.level_routes((H, W))["levels"] == case.level_routes
    hm = torch.from_numpy(rc.band_skip_frames(H, W)).cuda()
    n = hm.shape[0]
    fmin, ind = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    rows = torch.full((n, 4), 77, dtype=torch.int32, device="cuda")
    _lib.check(lib.tacex_indentation_depth(hm.data_ptr(), 0.0045, 0.024, fmin.data_ptr(), ind.data_ptr(), rows.data_ptr(), n, H, W,
                                           torch.cuda.current_stream().cuda_stream), "tacex_indentation_depth")
    Z, M = t.deform(hm, ind)                                                     # contact rows from the library's own minimum pass
    rgb = t.render_direct(hm, False, ind).clone()                                # ... and into the streaming tail
    rgb_rows = t.render_direct(hm, False, ind, frame_min=fmin, frame_rows=rows)  # contact rows from the caller
    torch.cuda.synchronize()
    for k, v in (("Z", Z), ("M", M), ("rgb", rgb), ("rgb_rows", rgb_rows), ("rows", rows)):
        res[name + "__" + k] = v.cpu().numpy()
np.savez(sys.argv[1], **res)
'''


def test_zero_band_skipping_is_exact_off_the_tuned_sizes(calib_dir, tmp_path):
    """test_zero_band_skipping_is_exact at (80,128) / (64,128) / 432x576: five, four and 27 bands, one, two and nine waves per band
    row.  TACEX_BAND_SKIP is read once per process: two children; deformed gel, mask and RGB must agree bit for bit."""
    from conftest import REPO

    script = tmp_path / "skip_routes.py"
    script.write_text(f"REPO = {str(REPO)!r}\nCALIB = {str(calib_dir)!r}\n" + _BAND_SKIP_SCRIPT)
    outs = {}
    for skip in ("1", "0"):
        out = tmp_path / f"s{skip}.npz"
        r = subprocess.run([sys.executable, str(script), str(out), str(tmp_path)], env=dict(os.environ, TACEX_BAND_SKIP=skip),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[skip] = np.load(out)
    a, b = outs["1"], outs["0"]
    for name in rc.BAND_SKIP_CASES:
        H = rc.BY_NAME[name].H
        for k in ("Z", "M", "rgb", "rgb_rows"):
            np.testing.assert_array_equal(a[f"{name}__{k}"], b[f"{name}__{k}"], err_msg=f"{name} {k}")
        np.testing.assert_array_equal(a[f"{name}__rgb"], a[f"{name}__rgb_rows"], err_msg=f"{name}: rows from the caller")
        rows = a[f"{name}__rows"]
        assert (rows[:, 1] < 0).any(), "a frame without contact"
        assert ((rows[:, 1] >= 0) & (rows[:, 1] - rows[:, 0] < min(40, max(16, H // 4)))).any(), "a small contact (most bands skipped)"
        assert (rows[:, 0] == 0).any() and (rows[:, 1] == H - 1).any(), "contacts on the top and bottom border"
        assert np.abs(a[f"{name}__Z"]).max() > 0.1
