"""The plain reference of the depth -> height map pass (tests/depth_pass_ref.py) checked on the CPU: the vectorised contact ranges against
a pixel-by-pixel loop, every input family against the property it is named for, and the shape table against the block-size rule."""
import numpy as np
import pytest

import depth_pass_ref as ref

F32 = np.float32


def _ranges_by_loop(hm):
    """First / last contact row and column of every frame, one pixel at a time (TT:441 in float32)."""
    B, H, W = hm.shape
    out = []
    for b in range(B):
        m = F32(np.inf)
        for i in range(H):
            for j in range(W):
                m = min(m, hm[b, i, j])
        d = F32(m / F32(1000)) - F32(ref.GELPAD_DMIN)
        d = F32(0) if d < 0 else d
        press = F32((F32(ref.GELPAD_H) - d) * F32(1000)) if d <= F32(ref.GELPAD_H) else F32(0)
        lo, hi, clo, chi = H, -1, W, -1
        for i in range(H):
            for j in range(W):
                if F32(F32(hm[b, i, j] - m) - press) < 0:
                    lo, hi, clo, chi = min(lo, i), max(hi, i), min(clo, j), max(chi, j)
        out.append((lo, hi, clo, chi))
    return np.array(out, np.int32)


@pytest.mark.parametrize("shape", [(13, 20), (7, 9)])
def test_vectorised_ranges_equal_the_pixel_loop(shape):
    H, W = shape
    hm = ref.height_map(ref.depth_frames(H, W))
    _, _, _, got = ref.reference(ref.depth_frames(H, W))
    np.testing.assert_array_equal(got, _ranges_by_loop(hm))
    mm = ref.mm_frames(H, W)
    np.testing.assert_array_equal(ref.reference_mm(mm)[2], _ranges_by_loop(mm))
    # random contact patterns as well: a third of the pixels below the press plane
    rng = np.random.RandomState(H * W)
    noisy = np.where(rng.rand(4, H, W) < 0.3, F32(28.1), F32(29.0)).astype(F32)
    noisy[3, 2:, :] = F32(29.0)
    noisy[:, 1, 1] = F32(28.0)
    np.testing.assert_array_equal(ref.reference_mm(noisy)[2], _ranges_by_loop(noisy))


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_families_have_the_property_they_are_named_for(shape):
    H, W = shape
    depth = ref.depth_frames(H, W)
    finite = depth[np.isfinite(depth)]
    assert finite.min() >= F32(ref.NEAR) and finite.max() <= F32(ref.FAR) and not np.isneginf(depth).any()  # camera bytes are defined
    hm, fmin, ind, rng = ref.reference(depth)
    by = {f.__name__: k for k, f in enumerate(ref.MM_FAMILIES)}
    C = ref.shifted(hm, fmin, ind) < 0
    k = by["sphere_dent"]
    assert C[k].any() and not C[k].all() and ind[k] > 0
    k = by["row0_only"]
    assert C[k, 0].any() and not C[k, 1:].any() and tuple(rng[k, :2]) == (0, 0)
    k = by["last_row_and_column"]
    assert C[k, H - 1].any() and C[k, :, W - 1].any() and not C[k, :H - 1, :W - 1].any()
    assert tuple(rng[k]) == (H // 2, H - 1, W // 2, W - 1)
    k = by["corner_pixel"]
    assert C[k].sum() == 1 and C[k, H - 1, W - 1] and tuple(rng[k]) == (H - 1, H - 1, W - 1, W - 1)
    k = by["no_contact"]
    assert not C[k].any() and ind[k] == 0 and fmin[k] == F32(29.0) and tuple(rng[k]) == (H, -1, W, -1)
    k = by["closer_than_case"]
    assert C[k].all() and ind[k] == F32(4.5) and fmin[k] < F32(24.0)
    k = len(ref.MM_FAMILIES)  # inf_patches
    assert np.isposinf(depth[k]).any() and (hm[k][np.isinf(depth[k])] == F32(29.0)).all() and np.isfinite(hm).all()
    assert C[k].any() and (C[k] != C[by["sphere_dent"]]).any()  # the unseen quarter takes contact pixels away
    # the frames without camera bytes do leave the clipping range
    wide = ref.depth_frames_wide(H, W)
    assert wide[0].min() > F32(ref.FAR) and wide[1].max() < F32(ref.NEAR) and np.isneginf(wide[2]).sum() == 1
    # heights below zero and the signed zero
    mm = ref.mm_frames(H, W)
    fm, im, rm = ref.reference_mm(mm)
    k = len(ref.MM_FAMILIES)
    assert (mm[k] < 0).sum() >= 2 and fm[k] == F32(-3.0) and im[k] == F32(4.5)
    assert np.signbit(mm[k, H // 2, W // 4]) and mm[k, H // 2, W // 4] == 0  # the -0.0
    assert tuple(rm[k]) == (H // 2, H - 1, W // 4, W - 1)
    assert np.signbit(mm[k + 1, 0, 0]) and fm[k + 1] == 0 and tuple(rm[k + 1]) == (0, H - 1, 0, W // 2)


def test_shape_table_follows_the_block_size_rule():
    for (H, W), cols in ref.SHAPES.items():
        assert ref.columns_route(H, W) == cols, (H, W)
    assert ref.columns_route(240, 320) == "exact" and ref.columns_route(480, 640) == "exact"  # the two tuned sizes
    assert ref.columns_route(2048, 4) == "exact" and ref.columns_route(2049, 4) == "full"


def test_camera_bytes_truncate_like_the_reference():
    d = np.array([[[0.020, 0.029, np.inf, 0.0245]]], F32)
    # ((mm - 20) / 29) * 255 truncated: 0, 79, 79 (inf -> far plane), 39
    np.testing.assert_array_equal(ref.camera_bytes(d), np.array([[[0, 79, 79, 39]]], np.uint8))


def test_batches_cover_every_frame():
    for n in (7, 8):
        b = ref.batches(n)
        assert {len(x) for x in b} == {1, 3} and set(sum(b, [])) == set(range(n))
