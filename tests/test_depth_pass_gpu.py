"""The depth -> height map pass off the two tuned resolutions: `tacex_height_map_from_depth` and `tacex_indentation_depth` through
the C ABI against the plain reference of tests/depth_pass_ref.py - height map, frame minimum, indentation and camera bytes bit for bit,
the contact row / column ranges exact where the row kernel tracks them and never narrower than the truth anywhere (band skipping
relies on that).  One shape per piece of index logic in frame_rows_kernel / frame_min_kernel (depth_pass_ref.SHAPES)."""
import numpy as np
import pytest
import torch

import depth_pass_ref as ref

pytestmark = pytest.mark.gpu

HM_GUARD, U8_GUARD, ROW_GUARD, SCALAR_GUARD = -12345.0, 0xA5, 77, -54321.0


@pytest.fixture(scope="module")
def lib():
    from tacex_amd import _lib

    return _lib.load_library()


def _guarded(B, frame, dtype, fill):
    """(B + 1) * frame elements of `fill`: the call owns the first B * frame, the rest must survive it."""
    return torch.full(((B + 1) * frame,), fill, dtype=dtype, device="cuda")


def _split(t, B, frame):
    a = t.cpu().numpy()
    return a[:B * frame], a[B * frame:]


def _check_ranges(got, true, H, W, route, where):
    """got / true (B, 4): containment always; equality as far as the route tracks the range."""
    for g, t in zip(got, true):
        if t[1] >= 0:
            assert g[0] <= t[0] and g[1] >= t[1] and g[2] <= t[2] and g[3] >= t[3], f"{where}: reported {g} does not contain {t}"
        assert 0 <= g[0] <= H and -1 <= g[1] < H and 0 <= g[2] <= W and -1 <= g[3] < W, f"{where}: {g} outside the frame"
    if route == "full":
        want = np.tile(np.array([0, H - 1, 0, W - 1], np.int32), (len(true), 1))
    else:
        want = true.copy()
        if route == "conservative":
            want[:, 2], want[:, 3] = 0, W - 1
    np.testing.assert_array_equal(got, want, err_msg=where)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("shape", list(ref.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_height_map_from_depth_equals_reference(lib, shape):
    from tacex_amd import _lib

    H, W = shape
    route, npix = ref.SHAPES[shape], H * W
    narrow, wide = ref.depth_frames(H, W), ref.depth_frames_wide(H, W)
    sets = {True: (narrow, ref.reference(narrow), ref.camera_bytes(narrow)), False: (wide, ref.reference(wide), None)}
    # (camera bytes, indentation, ranges): frame_rows needs indent_mm; without frame_rows every shape runs frame_min_kernel
    variants = [(True, True, True), (False, True, True), (True, True, False), (False, True, False), (False, False, False)]
    for in_range in (True, False):
        depth, (hm_w, fmin_w, ind_w, rng_w), u8_w = sets[in_range]
        for with_u8, with_ind, with_rows in variants:
            if with_u8 and not in_range:
                continue  # the float -> uint8 conversion is defined inside the clipping range only
            for idx in ref.batches(len(depth)):
                B = len(idx)
                where = f"{H}x{W} frames {idx} u8={with_u8} indent={with_ind} rows={with_rows}"
                d = torch.from_numpy(np.ascontiguousarray(depth[idx])).cuda()
                hm = _guarded(B, npix, torch.float32, HM_GUARD)
                u8 = _guarded(B, npix, torch.uint8, U8_GUARD)
                rows = _guarded(B, 4, torch.int32, ROW_GUARD)
                fmin = _guarded(B, 1, torch.float32, SCALAR_GUARD)
                ind = _guarded(B, 1, torch.float32, SCALAR_GUARD)
                _lib.check(lib.tacex_height_map_from_depth(
                    _lib.ptr(d), ref.NEAR, ref.FAR, ref.GELPAD_H, ref.GELPAD_DMIN, _lib.ptr(hm), _lib.ptr(fmin), _lib.ptr(ind) if with_ind else 0,
                    _lib.ptr(u8) if with_u8 else 0, _lib.ptr(rows) if with_rows else 0, B, H, W, _stream()), where)
                got, guard = _split(hm, B, npix)
                np.testing.assert_array_equal(got.reshape(B, H, W), hm_w[idx], err_msg=where)
                assert (guard == np.float32(HM_GUARD)).all(), where
                got, guard = _split(fmin, B, 1)
                np.testing.assert_array_equal(got, fmin_w[idx], err_msg=where)
                assert guard[0] == np.float32(SCALAR_GUARD), where
                got, guard = _split(ind, B, 1)
                assert guard[0] == np.float32(SCALAR_GUARD), where
                if with_ind:
                    np.testing.assert_array_equal(got, ind_w[idx], err_msg=where)
                else:
                    assert (got == np.float32(SCALAR_GUARD)).all(), where
                got, guard = _split(u8, B, npix)
                assert (guard == U8_GUARD).all(), where
                if with_u8:
                    np.testing.assert_array_equal(got.reshape(B, H, W), u8_w[idx], err_msg=where)
                else:
                    assert (got == U8_GUARD).all(), where
                got, guard = _split(rows, B, 4)
                assert (guard == ROW_GUARD).all(), where
                if with_rows:
                    _check_ranges(got.reshape(B, 4), rng_w[idx], H, W, route, where)
                else:
                    assert (got == ROW_GUARD).all(), where


@pytest.mark.parametrize("shape", list(ref.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_indentation_depth_equals_reference(lib, shape):
    """The same pass on an existing mm height map, frames with negative heights and a -0.0 included (the unsigned atomicMax branch of
    the row / column minima)."""
    from tacex_amd import _lib

    H, W = shape
    route, npix = ref.SHAPES[shape], H * W
    mm = ref.mm_frames(H, W)
    fmin_w, ind_w, rng_w = ref.reference_mm(mm)
    for with_rows in (True, False):
        for idx in ref.batches(len(mm)):
            B = len(idx)
            where = f"{H}x{W} frames {idx} rows={with_rows}"
            src = np.ascontiguousarray(mm[idx])
            d = torch.from_numpy(src).cuda()
            rows = _guarded(B, 4, torch.int32, ROW_GUARD)
            fmin = _guarded(B, 1, torch.float32, SCALAR_GUARD)
            ind = _guarded(B, 1, torch.float32, SCALAR_GUARD)
            _lib.check(lib.tacex_indentation_depth(_lib.ptr(d), ref.GELPAD_H, ref.GELPAD_DMIN, _lib.ptr(fmin), _lib.ptr(ind),
                                                   _lib.ptr(rows) if with_rows else 0, B, H, W, _stream()), where)
            assert d.cpu().numpy().tobytes() == src.tobytes(), f"{where}: the input was written"
            got, guard = _split(fmin, B, 1)
            np.testing.assert_array_equal(got, fmin_w[idx], err_msg=where)
            assert guard[0] == np.float32(SCALAR_GUARD), where
            got, guard = _split(ind, B, 1)
            np.testing.assert_array_equal(got, ind_w[idx], err_msg=where)
            assert guard[0] == np.float32(SCALAR_GUARD), where
            got, guard = _split(rows, B, 4)
            assert (guard == ROW_GUARD).all(), where
            if with_rows:
                _check_ranges(got.reshape(B, 4), rng_w[idx], H, W, route, where)
            else:
                assert (got == ROW_GUARD).all(), where
