"""GPU: the lean matrix-core band levels (TACEX_BAND_LEAN, BlurArgs::lean / zero_bands_unread in taxim_mfma.hip) against the full
ones, bit for bit.

A lean level loads the height map and its input only inside the frame's (grown) contact rectangle and leaves the bands it knows to
be zero unwritten; the level buffers of the workspace then hold stale data that no reader may ever load.  TACEX_BAND_LEAN is read
once per process, so the two settings run in two child processes (module fixture, shared by the tests):
  =0  plain renders of frame set A and of frame set B (= A with the frames moved to other slots);
  =1  a plain render of A, then A and B in a row with the whole workspace overwritten by NaN before every launch.
Shapes: rc.BAND_SKIP_CASES - (80,128) and (64,128) are the smallest frames whose levels all run on the matrix cores (waves straddle
the rectangle's edges, reflected window rows reach it), 432x576 has a matrix-core level behind a generic one - plus 240x320 with
contacts on column 0, on column W - 1, narrower than four columns and across the full width."""
import os
import subprocess
import sys

import numpy as np
import pytest

import taxim_route_cases as rc

pytestmark = pytest.mark.gpu

EDGE = "240x320-edges"
NAMES = tuple(rc.BAND_SKIP_CASES) + (EDGE,)
OUTPUTS = ("Z", "M", "rgb", "rgb_rows", "rgb_t", "z_t", "m_t", "srgb")  # deform | streaming tail, rows from the library / the caller | tiled tail | sensor
VISIBLE = ("Z", "M", "rgb_t", "z_t", "m_t")                             # caller-visible frames: deform() and the tiled tail

_SCRIPT = r'''
import sys
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, REPO); sys.path.insert(0, REPO + "/tests")
import taxim_route_cases as rc
from tacex_amd import GelSightSensor, GelSightSensorCfg, _lib
from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

out_path, tmp, lean = sys.argv[1], Path(sys.argv[2]), sys.argv[3] == "1"
lib, res = _lib.load_library(), {}


def edge_frames(H, W):
    """Contacts on column 0, on column W - 1, two columns wide (across a 4-column lane group) and across the full width."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for cy, cx in ((H // 2, 3), (H // 3, W - 4)):
        d = np.hypot(yy - cy, xx - cx)
        out.append(np.where(d < 10.0, 28.0 + 0.02 * d, rc.FAR_MM))
    bar = np.full((H, W), rc.FAR_MM)
    bar[100:141, 151:153] = 28.0
    out.append(bar)
    out.append(np.where(np.abs(yy - 150) < 9.0, 28.0 + 0.02 * np.abs(yy - 150), rc.FAR_MM))
    return np.stack(out).astype(np.float32)


def poison(tx, shape, n, on):
    """NaN over the whole workspace the wrapper hands the library as `ws` (0xFF bytes: every float a NaN)."""
    if on:
        tx._workspace(tx.context(shape), shape, n).fill_(255)


def run(tag, tx, sensor, hm, nan):
    H, W = hm.shape[-2:]
    n, shape = hm.shape[0], (H, W)
    fmin, ind = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    rows = torch.full((n, 4), 77, dtype=torch.int32, device="cuda")
    _lib.check(lib.tacex_indentation_depth(hm.data_ptr(), 0.0045, 0.024, fmin.data_ptr(), ind.data_ptr(), rows.data_ptr(), n, H, W,
                                           torch.cuda.current_stream().cuda_stream), "tacex_indentation_depth")
    fill = float("nan")
    new = lambda *s, dt=torch.float32: torch.full(s, fill if dt == torch.float32 else 0xAB, dtype=dt, device="cuda")
    tx.set_fused_tail(shape, 1)
    poison(tx, shape, n, nan)
    Z, M = tx.deform(hm, ind, z_out=new(n, H, W), mask_out=new(n, H, W, dt=torch.uint8))
    poison(tx, shape, n, nan)
    rgb = tx.render_direct(hm, False, ind, out=new(n, H, W, 3)).clone()
    if nan:  # the level buffers: Z ping | Z pong at the head of the workspace
        zz = tx._workspace(tx.context(shape), shape, n)[:2 * n * H * W * 4].view(torch.float32)
        res[tag + "__stale"] = np.array(bool(torch.isnan(zz).any()))
    poison(tx, shape, n, nan)
    rgb_rows = tx.render_direct(hm, False, ind, out=new(n, H, W, 3), frame_min=fmin, frame_rows=rows).clone()
    tx.set_fused_tail(shape, 2)
    poison(tx, shape, n, nan)
    z_t, m_t = new(n, H, W), new(n, H, W, dt=torch.uint8)
    rgb_t = tx.render_direct(hm, False, ind, out=new(n, H, W, 3), z_out=z_t, mask_out=m_t).clone()
    tx.set_fused_tail(shape, 1)
    sensor.set_camera_depth(hm / 1000.0)
    stx = sensor.optical_simulator._taxim
    poison(stx, shape, n, nan)
    sensor.update(0.01, force_recompute=True)
    srgb = sensor.data.output["tactile_rgb"].clone()
    torch.cuda.synchronize()
    for k, v in (("Z", Z), ("M", M), ("rgb", rgb), ("rgb_rows", rgb_rows), ("rgb_t", rgb_t), ("z_t", z_t), ("m_t", m_t), ("srgb", srgb),
                 ("rows", rows)):
        res[tag + "__" + k] = v.cpu().numpy()


for name in rc.BAND_SKIP_CASES + (EDGE,):
    if name == EDGE:
        H, W, folder, frames = 240, 320, Path(CALIB), edge_frames(240, 320)
    else:
        case = rc.BY_NAME[name]
        H, W = case.shape
        folder, frames = rc.calib_folder(case, Path(CALIB), tmp), rc.band_skip_frames(H, W)
    tx = Taxim(calib_folder=folder, backend="hip", device="cuda:0")
    if name != EDGE:
        assert tx.level_routes((H, W))["levels"] == case.level_routes
    n = frames.shape[0]
    cfg = GelSightSensorCfg(num_envs=n, sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
                            data_types=["tactile_rgb", "height_map"],
                            optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(folder), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                                              tactile_img_res=(W, H), device="cuda:0"),
                            marker_motion_sim_cfg=None, device="cuda:0")
    sensor = GelSightSensor(cfg)
    sensor.initialize()
    A = torch.from_numpy(frames).cuda()
    B = torch.from_numpy(np.ascontiguousarray(np.roll(frames, 1, axis=0))).cuda()  # other frames in the same slots
    run(name + "__A", tx, sensor, A, False)
    if lean:
        run(name + "__nanA", tx, sensor, A, True)
        run(name + "__nanB", tx, sensor, B, True)
    else:
        run(name + "__B", tx, sensor, B, False)
np.savez(out_path, **res)
'''


@pytest.fixture(scope="module")
def runs(calib_dir, tmp_path_factory):
    """{"1": results of the TACEX_BAND_LEAN=1 child, "0": of the =0 child} (read-only)."""
    from conftest import REPO

    tmp = tmp_path_factory.mktemp("band_lean")
    script = tmp / "band_lean_run.py"
    script.write_text(f"REPO = {str(REPO)!r}\nCALIB = {str(calib_dir)!r}\nEDGE = {EDGE!r}\n" + _SCRIPT)
    outs = {}
    for lean in ("1", "0"):
        out = tmp / f"lean{lean}.npz"
        r = subprocess.run([sys.executable, str(script), str(out), str(tmp), lean], env=dict(os.environ, TACEX_BAND_LEAN=lean),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[lean] = np.load(out)
    return outs


def test_frames_are_what_the_cases_need(runs):
    """The contact rectangles frame_rows_kernel found: a frame without contact, small contacts, contacts on the top and bottom border
    (BAND_SKIP_CASES); on column 0, on column W - 1, narrower than four columns, across the full width (240x320)."""
    for name in rc.BAND_SKIP_CASES:
        H, rows = rc.BY_NAME[name].H, runs["0"][f"{name}__A__rows"]
        assert (rows[:, 1] < 0).any() and (rows[:, 0] == 0).any() and (rows[:, 1] == H - 1).any(), rows
        assert ((rows[:, 1] >= 0) & (rows[:, 1] - rows[:, 0] < min(40, max(16, H // 4)))).any(), rows
    rows = runs["0"][f"{EDGE}__A__rows"]
    has = rows[:, 1] >= 0
    assert has.all() and len(rows) == 4, rows
    assert (rows[:, 2] == 0).any() and (rows[:, 3] == 319).any(), rows
    assert (rows[:, 3] - rows[:, 2] < 3).any(), rows
    assert ((rows[:, 2] == 0) & (rows[:, 3] == 319)).any(), rows
    assert ((rows[:, 2] == 0) & (rows[:, 3] < 160)).any() and ((rows[:, 2] > 160) & (rows[:, 3] == 319)).any(), rows


@pytest.mark.parametrize("name", NAMES)
def test_lean_levels_are_bit_identical(runs, name):
    """TACEX_BAND_LEAN=1 against =0: deformed gel, mask and RGB of deform(), of render_direct with the library's rows and with the
    caller's, of the tiled tail and of the sensor, array for array."""
    a, b = runs["1"], runs["0"]
    for k in OUTPUTS + ("rows",):
        np.testing.assert_array_equal(a[f"{name}__A__{k}"], b[f"{name}__A__{k}"], err_msg=f"{name} {k}")
    assert np.abs(b[f"{name}__A__Z"]).max() > 0.1 and b[f"{name}__A__M"].any()
    assert not np.array_equal(b[f"{name}__A__rgb"], b[f"{name}__B__rgb"])


def _skips_a_band(name, rows) -> bool:
    """Does the LAST band level skip a 16-row band of one of these frames (the kernel's own inequality), with matrix-core levels
    alone in front of the tail?  Then neither level buffer is complete after a lean render: what the last level skips, the level
    two ahead of it (same buffer, smaller input range + radius) skipped as well.  (64x128 with k = 117 skips nothing: every window
    spans the frame.)"""
    H, ks, levels = (240, rc.K320[:3], "M M M") if name == EDGE else (rc.BY_NAME[name].H, rc.BY_NAME[name].ksize, rc.BY_NAME[name].levels)
    if set(levels.split()) != {"M"}:
        return False
    R = [(k - 1) // 2 for k in ks[:len(levels.split())]]
    g, r, by = sum(R[:-1]), R[-1], np.arange(0, H, 16)
    return any(bool(((by - r > hi + g) | (by + 15 + r < lo - g)).any()) for lo, hi in rows[:, :2])


@pytest.mark.parametrize("name", NAMES)
def test_stale_level_buffers_are_never_read(runs, name):
    """NaN over the whole workspace before every launch, two frame sets in a row through the same slots: every output equals the
    un-poisoned =0 run and holds no NaN.  Where the band levels skip a band (_skips_a_band) the level buffers must still hold NaN after
    the render - the skipped bands were really left unwritten, so the comparison means something."""
    a, b = runs["1"], runs["0"]
    for p in ("A", "B"):
        for k in OUTPUTS:
            got = a[f"{name}__nan{p}__{k}"]
            if got.dtype.kind == "f":
                assert not np.isnan(got).any(), f"{name} {p} {k}: NaN"
            np.testing.assert_array_equal(got, b[f"{name}__{p}__{k}"], err_msg=f"{name} {p} {k}")
        skips = _skips_a_band(name, a[f"{name}__nan{p}__rows"])
        assert skips or name not in ("80x128-S320", EDGE), f"{name} {p}: frames that skip no band"
        if skips:
            assert bool(a[f"{name}__nan{p}__stale"]), f"{name} {p}: no band was left unwritten"


@pytest.mark.parametrize("name", NAMES)
def test_caller_visible_frames_stay_complete(runs, name):
    """Z / M of deform() and Z / M / RGB of a render through the tiled tail, into buffers filled with NaN / 0xAB and with a poisoned
    workspace: equal to the =0 run everywhere, skipped bands included (their zeros are stored), nothing left unwritten."""
    a, b = runs["1"], runs["0"]
    for p in ("A", "B"):
        for k in VISIBLE:
            got = a[f"{name}__nan{p}__{k}"]
            assert not (np.isnan(got).any() if got.dtype.kind == "f" else (got == 0xAB).any()), f"{name} {p} {k}: elements never written"
            np.testing.assert_array_equal(got, b[f"{name}__{p}__{k}"], err_msg=f"{name} {p} {k}")
        none = a[f"{name}__nan{p}__rows"][:, 1] < 0  # frames without contact: every band skipped
        assert not a[f"{name}__nan{p}__Z"][none].any() and not a[f"{name}__nan{p}__M"][none].any()
