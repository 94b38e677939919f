"""GPU: the pipelined schedule of the band levels (TACEX_BAND_PIPE: level l of chunk s - l for every l in ONE launch,
blur_mfma_pipe_kernel in taxim_mfma.hip, run_band_pipeline in tacex_capi.hip) against the per-level launches, bit for bit.

Nothing in the arithmetic changes, so every output must be equal array for array.  TACEX_BAND_PIPE, TACEX_BAND_LEAN and
TACEX_LEVEL_CHUNK_FRAMES are read once per process: every setting runs in a child process of its own, eight side by side (module
fixture, shared by the tests): TACEX_BAND_PIPE 1 / 0 x TACEX_LEVEL_CHUNK_FRAMES 1 / 2 / 3 / 4, with TACEX_BAND_LEAN 1 and then 0.
Seven frames per pass: 7 / 4 / 3 chunks (the last of one frame; three is the least that takes the schedule) and 2 chunks, which
keep the per-level launches.  The frames hold a contact on row 0, one on the last row, one in the middle and none at all, so that
skipped bands, the padding workgroups of a role and unwritten bands (zero_bands_unread) occur inside a fused grid.  Every render
runs twice in a row on one context with different frames and no synchronisation between them: the second pass's side-stream work
meets the first pass's tail.  TACEX_DEPTH_INTERLEAVE_MIN_FRAMES=1 (in every child) lets the sensor's deferred depth pass run chunk
by chunk at these sizes, in line with the launch steps of the two pipelines.
Shapes: (80,128) with k = 61 / 33 / 17 (two waves) and 240x320 with the edge frames of the band-weights test: the level set the
fused kernel is built for; (64,128) and 64x640 with k = 117 / 61 / 33 / 15: a level set without one, which must keep its schedule.

test_fused_kernel_keeps_the_resident_workgroups asks the runtime, in this process, for the workgroups per CU of the fused kernel
against the per-level instantiations, with the dynamic LDS sizes restated from pipe_plan / launch_mfma_tiles."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import taxim_route_cases as rc

pytestmark = pytest.mark.gpu

EDGE, WIDE = "240x320-edges", "64x640-S640"
NAMES = ("80x128-S320", "64x128-S640", EDGE, WIDE)
CHUNKS = ("1", "2", "3", "4")
OUTPUTS = ("Z", "M", "rgb", "rgb2", "rgb_t", "z_t", "m_t", "srgb", "srgb2", "sind", "rows")

_SCRIPT = r'''
import sys
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, REPO); sys.path.insert(0, REPO + "/tests")
import taxim_route_cases as rc
from tacex_amd import GelSightSensor, GelSightSensorCfg, _lib
from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

out_path, tmp = sys.argv[1], Path(sys.argv[2])
lib, res = _lib.load_library(), {}
WIDE_CASE = rc.Case(64, 640, "S640", rc.K640, "M M M M", 3, "stream", True)


def edge_frames(H, W):
    """Contacts on column 0, on column W - 1 and across the full width, and a frame without contact."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for cy, cx in ((H // 2, 3), (H // 3, W - 4)):
        d = np.hypot(yy - cy, xx - cx)
        out.append(np.where(d < 10.0, 28.0 + 0.02 * d, rc.FAR_MM))
    out.append(np.where(np.abs(yy - 150) < 9.0, 28.0 + 0.02 * np.abs(yy - 150), rc.FAR_MM))
    out.append(np.full((H, W), rc.FAR_MM))
    return np.stack(out).astype(np.float32)


def seven_frames(name, H, W):
    """Contacts on row 0, on the last row and in the middle, none, and three more: the edge frames (240x320) or the first three moved along x."""
    skip = rc.band_skip_frames(H, W)
    more = edge_frames(H, W)[:3] if name == EDGE else np.roll(skip[:3], W // 4, axis=2)
    return np.concatenate([skip, more])


def run(tag, tx, sensor, hm):
    H, W = hm.shape[-2:]
    n, shape = hm.shape[0], (H, W)
    hm2 = hm.flip(0).contiguous()
    fmin, ind, ind2 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    rows = torch.full((n, 4), 77, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tacex_indentation_depth(hm2.data_ptr(), 0.0045, 0.024, fmin.data_ptr(), ind2.data_ptr(), rows.data_ptr(), n, H, W, st), "tacex_indentation_depth")
    _lib.check(lib.tacex_indentation_depth(hm.data_ptr(), 0.0045, 0.024, fmin.data_ptr(), ind.data_ptr(), rows.data_ptr(), n, H, W, st), "tacex_indentation_depth")
    tx.set_fused_tail(shape, 1)
    Z, M = tx.deform(hm, ind)
    out1, out2 = torch.empty(n, H, W, 3, device="cuda"), torch.empty(n, H, W, 3, device="cuda")
    tx.render_direct(hm, False, ind, out=out1)  # two passes in a row on one context, nothing between them
    tx.render_direct(hm2, False, ind2, out=out2)
    tx.set_fused_tail(shape, 2)
    z_t, m_t = torch.empty(n, H, W, device="cuda"), torch.empty(n, H, W, dtype=torch.uint8, device="cuda")
    rgb_t = tx.render_direct(hm, False, ind, z_out=z_t, mask_out=m_t).clone()
    tx.set_fused_tail(shape, 1)
    sensor.set_camera_depth(hm / 1000.0)
    sensor.update(0.01, force_recompute=True)
    srgb = sensor.data.output["tactile_rgb"].clone()
    sensor.set_camera_depth(hm2 / 1000.0)
    sensor.update(0.01, force_recompute=True)
    srgb2 = sensor.data.output["tactile_rgb"].clone()
    sind = sensor.indentation_depth.clone()
    torch.cuda.synchronize()
    for k, v in (("Z", Z), ("M", M), ("rgb", out1), ("rgb2", out2), ("rgb_t", rgb_t), ("z_t", z_t), ("m_t", m_t), ("srgb", srgb), ("srgb2", srgb2),
                 ("sind", sind), ("rows", rows)):
        res[tag + "__" + k] = v.cpu().numpy()


for name in NAMES:
    if name == EDGE:
        H, W, base, n_band = 240, 320, Path(CALIB), 3
    else:
        case = WIDE_CASE if name == WIDE else rc.BY_NAME[name]
        H, W = case.shape
        base, n_band = rc.calib_folder(case, Path(CALIB), tmp), len(case.levels.split())
    frames = seven_frames(name, H, W)
    tx = Taxim(calib_folder=base, backend="hip", device="cuda:0")
    routes = tx.level_routes((H, W))
    assert routes["levels"][:n_band] == ["mfma"] * n_band, routes
    res[f"{name}__ksize"] = np.array(routes["ksize"][:n_band])
    n = frames.shape[0]
    cfg = GelSightSensorCfg(num_envs=n, sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
                            data_types=["tactile_rgb", "height_map"],
                            optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(base), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                                              tactile_img_res=(W, H), device="cuda:0"),
                            marker_motion_sim_cfg=None, device="cuda:0")
    sensor = GelSightSensor(cfg)
    sensor.initialize()
    run(name, tx, sensor, torch.from_numpy(frames).cuda())
np.savez(out_path, **res)
'''


@pytest.fixture(scope="module")
def runs(calib_dir, tmp_path_factory):
    """{(pipe, lean, chunk): results of the child with TACEX_BAND_PIPE=pipe TACEX_BAND_LEAN=lean TACEX_LEVEL_CHUNK_FRAMES=chunk} (read-only);
    the eight children of one TACEX_BAND_LEAN run at once."""
    from conftest import REPO

    tmp = tmp_path_factory.mktemp("band_pipeline")
    script = tmp / "band_pipeline_run.py"
    script.write_text(f"REPO = {str(REPO)!r}\nCALIB = {str(calib_dir)!r}\nEDGE = {EDGE!r}\nWIDE = {WIDE!r}\nNAMES = {NAMES!r}\n" + _SCRIPT)
    outs = {}
    for lean in ("1", "0"):
        procs = {}
        for pipe in ("1", "0"):
            for chunk in CHUNKS:
                work = tmp / f"p{pipe}l{lean}c{chunk}"
                work.mkdir()
                env = dict(os.environ, TACEX_BAND_PIPE=pipe, TACEX_BAND_LEAN=lean, TACEX_LEVEL_CHUNK_FRAMES=chunk, TACEX_DEPTH_INTERLEAVE_MIN_FRAMES="1")
                procs[pipe, lean, chunk] = (work / "out.npz", subprocess.Popen([sys.executable, str(script), str(work / "out.npz"), str(work)], env=env,
                                                                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
        for key, (out, p) in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, f"TACEX_BAND_PIPE={key[0]} TACEX_BAND_LEAN={key[1]} TACEX_LEVEL_CHUNK_FRAMES={key[2]}: {err[-3000:]}"
            outs[key] = np.load(out)
    return outs


def test_cases_reach_the_levels_they_name(runs):
    """Kernel sizes of the matrix-core levels per shape; the seven frames hold a contact on row 0, one on the last row, and one frame none."""
    b = runs["0", "1", "1"]
    want = {"80x128-S320": [61, 33, 17], "64x128-S640": [117, 61, 33, 15], EDGE: [61, 33, 17], WIDE: [117, 61, 33, 15]}
    for name in NAMES:
        assert b[f"{name}__ksize"].tolist() == want[name], name
        M, rows = b[f"{name}__M"], b[f"{name}__rows"]
        H = M.shape[1]
        assert M.shape[0] == 7 and not M[3].any() and rows[3, 1] < 0, name
        assert M[[0, 1, 2, 4, 5, 6]].reshape(6, -1).any(axis=1).all(), name
        assert rows[0, 0] == 0 and rows[1, 1] == H - 1, (name, rows)
        assert np.abs(b[f"{name}__Z"]).max() > 0.1
        # the second pass of two in a row renders the same frames in the opposite order
        np.testing.assert_array_equal(b[f"{name}__rgb"], b[f"{name}__rgb2"][::-1], err_msg=f"{name}: the second pass in a row")


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("lean", ("1", "0"))
@pytest.mark.parametrize("name", NAMES)
def test_pipelined_levels_are_bit_identical(runs, name, lean, chunk):
    """TACEX_BAND_PIPE=1 against =0 at the same TACEX_BAND_LEAN and launch size: deformed gel and mask of deform(), RGB of two streaming
    passes in a row, RGB of the tiled tail with its gel and mask frames, two sensor updates in a row with the deferred depth pass, the
    indentation depths and the contact rectangles."""
    a, b = runs["1", lean, chunk], runs["0", lean, chunk]
    for k in OUTPUTS:
        np.testing.assert_array_equal(a[f"{name}__{k}"], b[f"{name}__{k}"], err_msg=f"{name} lean={lean} chunk={chunk} {k}")


@pytest.mark.parametrize("lean", ("1", "0"))
def test_launch_size_changes_no_bit(runs, lean):
    """The pipelined schedule at 7, 4 and 3 chunks and the per-level fallback at 2 give the same frames."""
    ref = runs["1", lean, "4"]
    for chunk in CHUNKS[:3]:
        for name in NAMES:
            for k in ("rgb", "rgb2", "srgb", "srgb2"):
                np.testing.assert_array_equal(runs["1", lean, chunk][f"{name}__{k}"], ref[f"{name}__{k}"], err_msg=f"{name} lean={lean} chunk={chunk} {k}")


# ---- resident workgroups per CU ------------------------------------------------------------------------------------------------
def _level_kernel(K, first, lean, wlds):
    b = lambda v: f"Lb{int(v)}E"
    return f"_ZN5tacex16blur_mfma_kernelILi{K}E{b(first)}Li1ELb1E{b(lean)}{b(wlds)}EEvNS_8BlurArgsE"


def _pipe_kernel(lean, wlds):
    """Itanium name of blur_mfma_pipe_kernel<true, LEAN, WLDS, 61, 33, 17>(PipeArgs)."""
    b = lambda v: f"Lb{int(v)}E"
    return f"_ZN5tacex21blur_mfma_pipe_kernelILb1E{b(lean)}{b(wlds)}Li61EJLi33ELi17EEEEvNS_8PipeArgsE"


def _lds_bytes(K, W):
    """(dynamic LDS without the filter copy, bytes of one copy) as launch_mfma_tiles and pipe_plan compute them."""
    R = (K - 1) // 2
    RA = (R + 7) & ~7
    pitch = W + 2 * RA + 4
    if ((pitch >> 2) & 1) == 0:
        pitch += 4
    return 16 * pitch * 4, ((2 * RA + 31 + 15) & ~15) * 4


def test_fused_kernel_keeps_the_resident_workgroups():
    """hipOccupancyMaxActiveBlocksPerMultiprocessor at W = 320 threads, zero gel map, lean and full: the fused kernel of k = 61 / 33 / 17 with
    the largest role's dynamic LDS holds as many workgroups per CU as the least of the three per-level instantiations as they are
    launched - with one filter copy per wave, which is what pipe_plan then takes - and the instantiation without the copies does too."""
    import torch

    from tacex_amd import _lib

    torch.cuda.init()
    lib = _lib.load_library()
    occ = lib.hipOccupancyMaxActiveBlocksPerMultiprocessor  # (resolved through the library's own dependency on the HIP runtime)
    occ.restype, occ.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_size_t]

    def blocks(name, threads, lds):
        assert lds <= 48 * 1024
        n = C.c_int(0)
        assert occ(C.byref(n), C.addressof(C.c_char.in_dll(lib, name)), threads, lds) == 0, name
        return n.value

    W, waves = 320, 5
    for lean in (True, False):
        per_level, lds_mid, lds_wave = [], 0, 0
        for K in (61, 33, 17):
            lds, copy = _lds_bytes(K, W)
            per_level.append(max(blocks(_level_kernel(K, K == 61, lean, False), W, lds), blocks(_level_kernel(K, K == 61, lean, True), W, lds + waves * copy),
                                 blocks(_level_kernel(K, K == 61, lean, True), W, lds + copy)))
            lds_mid, lds_wave = max(lds_mid, lds), max(lds_wave, lds + waves * copy)
        fused_wave, fused_old = blocks(_pipe_kernel(lean, True), W, lds_wave), blocks(_pipe_kernel(lean, False), W, lds_mid)
        print(f"W={W} lean={lean}: per level {per_level}, fused with a copy per wave {fused_wave} ({lds_wave} B), without copies {fused_old} ({lds_mid} B)")
        assert min(per_level) >= 1
        assert fused_wave >= min(per_level), (lean, per_level, fused_wave)
        assert fused_old >= min(per_level), (lean, per_level, fused_old)
