"""Sensor camera model on the CPU: the ABI (symbols, refusals before any GPU call), the host draw function against the NumPy
restatement (tests/camera_model_ref.py), the Python layer's argument checks, and the statistics the contract promises, measured on the
restatement (the GPU tests compare the kernel with it bit for bit)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
from camera_model_ref import S, camera_frame, frame_draws, group_draws, profile_row
from conftest import REPO


def _lib_and_module():
    from tacex_amd import _lib

    return _lib.load_library(), _lib


def test_symbols_declared_exported_and_bound():
    lib, _lib = _lib_and_module()
    txt = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "tacex_hip.h").read_text(), flags=re.S)
    for name, nargs in (("tacex_camera_model", 13), ("tacex_camera_noise_draw", 6)):
        decl = re.search(name + r"\s*\(([^)]*)\)", txt)
        assert decl, f"{name} is not declared in include/tacex_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs
    hdr = int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", (REPO / "include" / "tacex_hip.h").read_text()).group(1))
    assert lib.tacex_abi_version() == hdr == _lib.ABI_VERSION == 20


def test_the_translation_unit_is_built_without_fp_contraction():
    from tacex_amd import _build

    assert "camera_model.hip" in _build.SOURCES and (REPO / "tacex_amd" / "csrc" / "camera_model.hip").exists()
    assert "-ffp-contract=off" in _build.FILE_FLAGS["camera_model.hip"]


def test_exported_from_the_package():
    import tacex_amd

    assert {"CameraProfile", "TactileCameraModel"} <= set(tacex_amd.__all__)
    assert tacex_amd.TactileCameraModel.__module__ == "tacex_amd.camera_model"
    assert hasattr(tacex_amd.GelSightSensor, "camera_image")


# arguments of a valid call (the pointers are never dereferenced: every case below is refused before any GPU call)
_OK = dict(rgb=0x1000, prof=0x2000, P=1, ids=None, seed=1, off=0, call=0, out=0x3000, dt=0, B=1, H=4, W=4)


@pytest.mark.parametrize("change, word", [
    (dict(rgb=None), b"rgb_dev"), (dict(prof=None), b"profiles_dev"), (dict(out=None), b"out_dev"),
    (dict(P=0), b"num_profiles"), (dict(P=-3), b"num_profiles"),
    (dict(B=0), b"num_frames"), (dict(B=-1), b"num_frames"), (dict(H=0), b"height"), (dict(W=0), b"width"), (dict(W=-5), b"width"),
    (dict(dt=2), b"out_dtype"), (dict(dt=-1), b"out_dtype"),
    (dict(dt=1, out=0x1000), b"out_dev == rgb_dev"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_return_2_and_name_the_argument(change, word):
    lib, _lib = _lib_and_module()
    a = dict(_OK, **change)
    rc = lib.tacex_camera_model(a["rgb"], a["prof"], a["P"], a["ids"], a["seed"], a["off"], a["call"], a["out"], a["dt"], a["B"], a["H"],
                                a["W"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_camera_model" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "tacex_camera_model")


def test_noise_draw_refuses_a_null_output():
    lib, _ = _lib_and_module()
    assert lib.tacex_camera_noise_draw(1, 0, 0, 0, 0, None) == 2 and b"tacex_camera_noise_draw" in lib.tacex_last_error()


DRAW_CASES = [(0, 0, 0, 0), (7, 3, 11, 19199), (0x1234567_89ABCDEF, 2 ** 32 - 1, 5, 1), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1),
              (2 ** 32 + 5, 100, 9, 76799), (2 ** 32, 0, 1, 2 ** 31)]


@pytest.mark.parametrize("fixed", [0, 1])
@pytest.mark.parametrize("seed, frame, call, group", DRAW_CASES)
def test_host_draws_equal_the_restatement(seed, frame, call, group, fixed):
    lib, _ = _lib_and_module()
    out = (C.c_int32 * 12)()
    assert lib.tacex_camera_noise_draw(seed, frame, call, group, fixed, out) == 0
    want = group_draws(seed, frame, call, [group], fixed_pattern=bool(fixed))[0]
    assert list(out) == [int(v) for v in want]
    assert all(-510 <= v <= 510 for v in out)


def test_fixed_pattern_draws_do_not_change_with_call_and_the_others_do():
    lib, _ = _lib_and_module()
    a, b = (C.c_int32 * 12)(), (C.c_int32 * 12)()
    for seed, frame, _, group in DRAW_CASES:
        assert lib.tacex_camera_noise_draw(seed, frame, 3, group, 1, a) == 0 and lib.tacex_camera_noise_draw(seed, frame, 4, group, 1, b) == 0
        assert list(a) == list(b)
        assert lib.tacex_camera_noise_draw(seed, frame, 3, group, 0, a) == 0 and lib.tacex_camera_noise_draw(seed, frame, 4, group, 0, b) == 0
        assert list(a) != list(b)
        assert lib.tacex_camera_noise_draw(seed, frame, 0, group, 1, b) == 0 and list(a) != list(b)  # stream 4.. is not stream 0..


def test_draw_addressing_of_the_restatement():
    """Sample j of a group is word j % 4 of the Philox call with counter word 1 = j / 4 (+ 4 for the fixed pattern)."""
    from marker_pattern_ref import philox4x32

    seed, frame, call, g = 2 ** 40 + 17, 9, 6, 123
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    for fixed in (False, True):
        d = group_draws(seed, frame, call, [g], fixed)[0]
        for j in range(12):
            w = int(philox4x32(np.array([g, j // 4 + (4 if fixed else 0), frame, 0 if fixed else call], dtype=np.uint32), key)[j % 4])
            assert d[j] == sum((w >> s) & 0xFF for s in (0, 8, 16, 24)) - 510
    assert S == np.float32(1.0 / np.sqrt(21845.0)) and S.dtype == np.float32


def test_python_argument_checks():
    from tacex_amd import CameraProfile, TactileCameraModel
    from tacex_amd._lib import TacexHipError

    row = CameraProfile(color_matrix=[[0.9, 0.1, 0], [0, 1, 0], [0.05, 0, 0.95]], offset=[0.01, 0, -0.01], read_noise=0.02, shot_noise=1e-3,
                        fixed_pattern=0.01).row()
    assert row.dtype == np.float32 and row.shape == (16,) and row[15] == 0
    np.testing.assert_array_equal(row, profile_row([[0.9, 0.1, 0], [0, 1, 0], [0.05, 0, 0.95]], [0.01, 0, -0.01], 0.02, 1e-3, 0.01))
    np.testing.assert_array_equal(CameraProfile.identity().row(), profile_row())
    np.testing.assert_array_equal(CameraProfile(offset=0.25).row()[9:12], np.float32([0.25] * 3))
    for bad in (dict(color_matrix=np.eye(4)), dict(offset=[0, 1]), dict(read_noise=-0.1), dict(shot_noise=float("nan")), dict(fixed_pattern=-1)):
        with pytest.raises(ValueError):
            CameraProfile(**bad).row()
    ident = [CameraProfile.identity()]
    with pytest.raises(ValueError):
        TactileCameraModel([], 2, "cuda")
    with pytest.raises(ValueError):
        TactileCameraModel([np.zeros(16)], 2, "cuda")
    with pytest.raises(ValueError):
        TactileCameraModel(ident, 0, "cuda")
    with pytest.raises(ValueError):
        TactileCameraModel(ident, 2, "cuda", dtype=torch.float16)
    with pytest.raises(ValueError):
        TactileCameraModel(ident, 2, "cuda", seed=-1)
    with pytest.raises(ValueError):
        TactileCameraModel(ident, 2, "cuda", frame_offset=2 ** 32 - 1)
    with pytest.raises(TacexHipError):  # no CPU path
        TactileCameraModel(ident, 2, "cpu")


# ---- statistics of the contract, on the restatement: one 240 x 320 frame at constant 0.5, identity colour, read sigma 0.02 ----------
H, W, SIGMA = 240, 320, 0.02
N = H * W * 3


@pytest.fixture(scope="module")
def noise_frames():
    rgb = np.full((H, W, 3), 0.5, dtype=np.float32)
    row = profile_row(read_noise=SIGMA)
    f = lambda frame, call: camera_frame(rgb, row, 2 ** 33 + 12345, frame, call, u8=False).astype(np.float64) - 0.5  # noqa: E731
    return {"f0c0": f(0, 0), "f1c0": f(1, 0), "f0c1": f(0, 1)}


def test_noise_has_the_nominal_deviation_and_zero_mean(noise_frames):
    for name, e in noise_frames.items():
        ratio = e.std() / SIGMA
        print(f"{name}: std / nominal = {ratio:.5f}, mean * sqrt(N) / sigma = {e.mean() * np.sqrt(N) / SIGMA:.3f}, max |e| / sigma = {np.abs(e).max() / SIGMA:.3f}")
        assert abs(ratio - 1) < 0.01  # the estimate's standard error at N = 230400 is 0.15 %
        assert abs(e.mean()) < 5 * SIGMA / np.sqrt(N)
        # nothing is clamped: the largest draw is 510 / sqrt(21845) = 3.45 sigma, far inside [0, 1] around 0.5
        assert np.abs(e).max() <= 3.46 * SIGMA and np.abs(e).max() < 0.5


def test_noise_is_uncorrelated_between_frames_and_between_calls(noise_frames):
    a = noise_frames["f0c0"].ravel()
    for other in ("f1c0", "f0c1"):
        rho = np.corrcoef(a, noise_frames[other].ravel())[0, 1]
        print(f"f0c0 vs {other}: |rho| sqrt(N) = {abs(rho) * np.sqrt(N):.3f}")
        assert abs(rho) * np.sqrt(N) < 5
