"""GPU: the matrix-core band levels with their Toeplitz weights read from a copy of the level's filter in LDS (TACEX_BAND_WLDS,
the WLDS instantiations of blur_mfma_kernel in taxim_mfma.hip) against the lane-indexed weight tables from global memory, bit for bit.

The f32 weights and the order of the MFMAs are the same, so every output must be equal array for array.  TACEX_BAND_WLDS and
TACEX_BAND_LEAN are read once per process: the settings run in child processes, side by side (module fixture, shared by the tests):
  WLDS 1 / 0 with LEAN 1: every shape with the shipped zero gel map (GZ lean instantiations) and with a dome for a gel map (GZ = false)
  WLDS 1 / 0 with LEAN 0: every shape with the zero gel map (GZ full instantiations; a non-zero gel map never runs lean)
Shapes: (64,128) with k = 117 / 61 / 33 / 15 and (80,128) with k = 61 / 33 / 17, the smallest frames whose levels all run on the
matrix cores (two waves: one filter copy per wave); 240x320 with contacts on column 0, on column W - 1 and across the full width
plus a frame without contact; 64x640, the smallest frame on which k = 117 runs ten waves wide (one filter copy per workgroup, behind
a barrier, where ten copies would cost a resident workgroup).

test_resident_workgroups_do_not_drop asks the runtime, in this process, for the workgroups per CU of the new and the old
instantiation of every default level with their dynamic LDS sizes (restated from launch_mfma_tiles)."""
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
GELS = ("zero", "dome")
OUTPUTS = ("Z", "M", "rgb", "rgb_t", "z_t", "m_t", "srgb")  # deform | streaming tail | tiled tail | sensor

_SCRIPT = r'''
import shutil, sys
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, REPO); sys.path.insert(0, REPO + "/tests")
import taxim_route_cases as rc
from tacex_amd import GelSightSensor, GelSightSensorCfg, _lib
from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg
from tacex_amd.simulation_approaches.gpu_taxim.sim import Taxim

out_path, tmp, gels = sys.argv[1], Path(sys.argv[2]), sys.argv[3].split(",")
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


def with_dome(folder, name):
    """A copy of the calibration folder whose gel map is a dome (non-zero everywhere but at its apex)."""
    dst = tmp / f"dome_{name}"
    shutil.copytree(folder, dst)
    shape = np.load(dst / "gelmap.npy").shape
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float32)
    np.save(dst / "gelmap.npy", (-((yy - (shape[0] - 1) / 2) ** 2 + (xx - (shape[1] - 1) / 2) ** 2) / 4000.0).astype(np.float32))
    return dst


def run(tag, tx, sensor, hm):
    H, W = hm.shape[-2:]
    n, shape = hm.shape[0], (H, W)
    fmin, ind = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    rows = torch.full((n, 4), 77, dtype=torch.int32, device="cuda")
    _lib.check(lib.tacex_indentation_depth(hm.data_ptr(), 0.0045, 0.024, fmin.data_ptr(), ind.data_ptr(), rows.data_ptr(), n, H, W,
                                           torch.cuda.current_stream().cuda_stream), "tacex_indentation_depth")
    tx.set_fused_tail(shape, 1)
    Z, M = tx.deform(hm, ind)
    rgb = tx.render_direct(hm, False, ind).clone()
    tx.set_fused_tail(shape, 2)
    z_t, m_t = torch.empty(n, H, W, device="cuda"), torch.empty(n, H, W, dtype=torch.uint8, device="cuda")
    rgb_t = tx.render_direct(hm, False, ind, z_out=z_t, mask_out=m_t).clone()
    tx.set_fused_tail(shape, 1)
    sensor.set_camera_depth(hm / 1000.0)
    sensor.update(0.01, force_recompute=True)
    srgb = sensor.data.output["tactile_rgb"].clone()
    torch.cuda.synchronize()
    for k, v in (("Z", Z), ("M", M), ("rgb", rgb), ("rgb_t", rgb_t), ("z_t", z_t), ("m_t", m_t), ("srgb", srgb), ("rows", rows)):
        res[tag + "__" + k] = v.cpu().numpy()


for name in NAMES:
    if name == EDGE:
        H, W, base, frames, n_band = 240, 320, Path(CALIB), edge_frames(240, 320), 3
    else:
        case = WIDE_CASE if name == WIDE else rc.BY_NAME[name]
        H, W = case.shape
        base, frames, n_band = rc.calib_folder(case, Path(CALIB), tmp), rc.band_skip_frames(H, W), len(case.levels.split())
    for gel in gels:
        folder = with_dome(base, name) if gel == "dome" else base
        tx = Taxim(calib_folder=folder, backend="hip", device="cuda:0")
        routes = tx.level_routes((H, W))
        assert routes["levels"][:n_band] == ["mfma"] * n_band, routes
        res[f"{name}__{gel}__ksize"] = np.array(routes["ksize"][:n_band])
        n = frames.shape[0]
        cfg = GelSightSensorCfg(num_envs=n, sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(W, H), clipping_range=(0.024, 0.029)),
                                data_types=["tactile_rgb", "height_map"],
                                optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(folder), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                                                  tactile_img_res=(W, H), device="cuda:0"),
                                marker_motion_sim_cfg=None, device="cuda:0")
        sensor = GelSightSensor(cfg)
        sensor.initialize()
        run(f"{name}__{gel}", tx, sensor, torch.from_numpy(frames).cuda())
np.savez(out_path, **res)
'''


@pytest.fixture(scope="module")
def runs(calib_dir, tmp_path_factory):
    """{(wlds, lean): results of the child with TACEX_BAND_WLDS=wlds TACEX_BAND_LEAN=lean} (read-only); the four children run at once."""
    from conftest import REPO

    tmp = tmp_path_factory.mktemp("band_weights")
    script = tmp / "band_weights_run.py"
    script.write_text(f"REPO = {str(REPO)!r}\nCALIB = {str(calib_dir)!r}\nEDGE = {EDGE!r}\nWIDE = {WIDE!r}\nNAMES = {NAMES!r}\n" + _SCRIPT)
    procs = {}
    for wlds in ("1", "0"):
        for lean in ("1", "0"):
            work = tmp / f"w{wlds}l{lean}"
            work.mkdir()
            gels = ",".join(GELS if lean == "1" else GELS[:1])
            procs[wlds, lean] = (work / "out.npz", subprocess.Popen(
                [sys.executable, str(script), str(work / "out.npz"), str(work), gels], env=dict(os.environ, TACEX_BAND_WLDS=wlds, TACEX_BAND_LEAN=lean),
                stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    outs = {}
    for key, (out, p) in procs.items():
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, f"TACEX_BAND_WLDS={key[0]} TACEX_BAND_LEAN={key[1]}: {err[-3000:]}"
        outs[key] = np.load(out)
    return outs


def test_cases_reach_the_levels_they_name(runs):
    """Kernel sizes of the matrix-core levels per shape; the frames hold contact (and one of each set none)."""
    b = runs["0", "1"]
    want = {"80x128-S320": [61, 33, 17], "64x128-S640": [117, 61, 33, 15], EDGE: [61, 33, 17], WIDE: [117, 61, 33, 15]}
    for name in NAMES:
        for gel in GELS:
            assert b[f"{name}__{gel}__ksize"].tolist() == want[name], (name, gel)
        M = b[f"{name}__zero__M"]
        assert M[:3].reshape(3, -1).any(axis=1).all() and not M[3].any(), name
        assert np.abs(b[f"{name}__zero__Z"]).max() > 0.1
        assert not np.array_equal(b[f"{name}__zero__Z"], b[f"{name}__dome__Z"]), f"{name}: the dome changes nothing"
    rows = b[f"{EDGE}__zero__rows"]  # contact rectangle of frame_rows_kernel: first / last row, first / last column
    assert rows[0, 2] == 0 and rows[0, 3] < 160 and rows[1, 2] > 160 and rows[1, 3] == 319 and tuple(rows[2, 2:]) == (0, 319) and rows[3, 1] < 0, rows


@pytest.mark.parametrize("lean", ("1", "0"))
@pytest.mark.parametrize("name", NAMES)
def test_lds_weights_are_bit_identical(runs, name, lean):
    """TACEX_BAND_WLDS=1 against =0 at the same TACEX_BAND_LEAN: deformed gel and mask of deform(), RGB of the streaming and of the
    tiled tail (with its gel and mask frames) and of a sensor update; zero gel map, and (lean = 1 children) the dome."""
    a, b = runs["1", lean], runs["0", lean]
    for gel in (GELS if lean == "1" else GELS[:1]):
        for k in OUTPUTS:
            np.testing.assert_array_equal(a[f"{name}__{gel}__{k}"], b[f"{name}__{gel}__{k}"], err_msg=f"{name} {gel} {k}")


# ---- resident workgroups per CU ------------------------------------------------------------------------------------------------
def _kernel(K, first, gz, lean, wlds):
    """Itanium name of blur_mfma_kernel<K, FIRST, 1, GZ, LEAN, WLDS>(BlurArgs): the host-side handle of the instantiation."""
    b = lambda v: f"Lb{int(v)}E"
    return f"_ZN5tacex16blur_mfma_kernelILi{K}E{b(first)}Li1E{b(gz)}{b(lean)}{b(wlds)}EEvNS_8BlurArgsE"


def _lds_bytes(K, W):
    """(dynamic LDS of the instantiation without the filter copy, bytes of one copy) as launch_mfma_tiles computes them."""
    R = (K - 1) // 2
    RA = (R + 7) & ~7
    pitch = W + 2 * RA + 4
    if ((pitch >> 2) & 1) == 0:
        pitch += 4
    return 16 * pitch * 4, ((2 * RA + 31 + 15) & ~15) * 4


DEFAULT_LEVELS = [(320, K, K == 61) for K in (61, 33, 17)] + [(640, K, K == 117) for K in (117, 61, 33, 15)]


def test_resident_workgroups_do_not_drop():
    """hipOccupancyMaxActiveBlocksPerMultiprocessor of every default level (320x240: k = 61 / 33 / 17, 640x480: 117 / 61 / 33 / 15;
    zero gel map lean and full, and the general gel map) at W threads: the WLDS instantiation with one filter copy per wave or with
    one per workgroup - launch_mfma_tiles takes whichever places more workgroups, the copy per wave on a tie - holds at least as many
    workgroups per CU as the old instantiation.  k = 61 at W = 320 must keep them with the copy per wave; k = 117 at W = 640 keeps
    them with one of the two."""
    import torch

    from tacex_amd import _lib

    torch.cuda.init()
    lib = _lib.load_library()
    occ = lib.hipOccupancyMaxActiveBlocksPerMultiprocessor  # (resolved through the library's own dependency on the HIP runtime)
    occ.restype, occ.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_size_t]
    set_attr = lib.hipFuncSetAttribute
    set_attr.restype, set_attr.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int]

    def blocks(name, threads, lds):
        f = C.addressof(C.c_char.in_dll(lib, name))
        if lds > 48 * 1024:
            assert set_attr(f, 8, lds) == 0, name  # hipFuncAttributeMaxDynamicSharedMemorySize
        n = C.c_int(0)
        assert occ(C.byref(n), f, threads, lds) == 0, name
        return n.value

    for W, K, first in DEFAULT_LEVELS:
        lds, copy = _lds_bytes(K, W)
        for gz, lean in ((True, True), (True, False), (False, False)):
            old = blocks(_kernel(K, first, gz, lean, False), W, lds)
            per_wave = blocks(_kernel(K, first, gz, lean, True), W, lds + (W // 64) * copy)
            per_wg = blocks(_kernel(K, first, gz, lean, True), W, lds + copy)
            print(f"W={W} k={K} gz={gz} lean={lean}: old {old} per-wave copy {per_wave} per-workgroup copy {per_wg}")
            assert old >= 1
            assert max(per_wave, per_wg) >= old, (W, K, gz, lean, old, per_wave, per_wg)
            if (W, K) == (320, 61):
                assert per_wave >= old, (W, K, gz, lean, old, per_wave)
