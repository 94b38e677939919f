"""Plain float32 restatement of the depth -> height map pass (GS:581-593, GS:565-575, TS:115-131, TT:441) and the deterministic
input families its tests run on.  TEST INFRASTRUCTURE: shared by tests/test_depth_pass_ref.py (CPU) and tests/test_depth_pass_gpu.py.

Everything is NumPy float32 in the kernels' operation order (csrc/taxim_kernels.hip: frame_min_kernel / frame_rows_kernel):
  hm     = where(isinf(depth), far, depth) * 1000
  fmin   = min over the frame of hm
  indent = TaximOracle.indentation_depth(hm)
  S      = (hm - fmin) - indent
  rows   = first / last row holding a pixel with S < 0, (H, -1) without one; columns likewise, (W, -1)
"""
import numpy as np

F32 = np.float32

GELPAD_H, GELPAD_DMIN = 0.0045, 0.024
# camera clipping range of the tests: every family below stays inside [NEAR, FAR] (or is +inf), so that the float -> uint8 conversion of
# the camera bytes is defined; the frame "closer than the sensor case" (23.5 mm < GELPAD_DMIN) needs NEAR below the case
NEAR, FAR = 0.020, 0.029

# (H, W) -> how the pass reports the contact columns: "exact", "conservative" = (0, W - 1) with exact rows, "full" = rows (0, H - 1) and
# columns (0, W - 1) (no row kernel: W % 4 != 0 or H > 2048).  One piece of index logic per shape.
SHAPES = {
    (250, 320): "exact",         # first loop, partial last batch (250 = 5 * 48 + 10), 960 threads
    (37, 640): "exact",          # the same at 160 float4s per row (37 = 24 + 13)
    (100, 384): "exact",         # 960 threads at 96 float4s per row
    (50, 16): "exact",           # a wave spans 16 rows; H < rows per iteration
    (1100, 64): "exact",         # H > 1024: second trip of the LDS loops
    (2048, 4): "exact",          # H at the LDS limit, one float4 per row
    (30, 40): "conservative",    # second loop, fewer float4s than one block
    (130, 96): "conservative",   # second loop, one outer iteration
    (200, 192): "conservative",  # second loop, three outer iterations, partial last block
    (5, 2304): "conservative",   # W > 2048 at 576 threads
    (3, 4100): "conservative",   # more than 1024 float4s per row
    (2049, 4): "full",           # H past the LDS limit: frame_min_kernel + fill_rows_kernel, npix % 4 == 0
    (50, 70): "full",            # W % 4 != 0, npix % 4 == 0
    (7, 9): "full",              # npix % 4 == 3
}


def columns_route(H, W):
    """The block-size rule of frame_rows_block_threads and the cols_ok test of frame_rows_kernel, restated."""
    if W % 4 != 0 or H > 2048:
        return "full"
    w4 = W // 4
    nt = (1024 // w4) * w4 if w4 <= 1024 else 1024
    if nt < 512 or nt % 64:
        nt = 1024
    return "exact" if W <= 2048 and nt % w4 == 0 else "conservative"


def height_map(depth_m, far_m=FAR):
    d = np.asarray(depth_m, F32)
    return (np.where(np.isinf(d), F32(far_m), d) * F32(1000.0)).astype(F32)


def frame_min(hm):
    return np.asarray(hm, F32).min(axis=(-2, -1))


def indentation(hm):
    from oracle.taxim_oracle import TaximOracle

    return TaximOracle.indentation_depth(hm, GELPAD_H, GELPAD_DMIN)


def shifted(hm, fmin=None, indent=None):
    hm = np.asarray(hm, F32)
    fmin = frame_min(hm) if fmin is None else np.asarray(fmin, F32)
    indent = indentation(hm) if indent is None else np.asarray(indent, F32)
    return ((hm - fmin.reshape(-1, 1, 1)) - indent.reshape(-1, 1, 1)).astype(F32)


def contact_ranges(S):
    """(B, 4) int32: first / last row and first / last column with S < 0; (H, -1, W, -1) for a frame without one."""
    C = np.asarray(S) < 0
    B, H, W = C.shape
    out = np.empty((B, 4), np.int32)
    for b in range(B):
        r, c = np.flatnonzero(C[b].any(1)), np.flatnonzero(C[b].any(0))
        out[b] = (r[0], r[-1], c[0], c[-1]) if len(r) else (H, -1, W, -1)
    return out


def camera_bytes(depth_m, near_m=NEAR, far_m=FAR):
    """GS:565-575 with the reference's own torch statements on the CPU (Python double products as scalar operands)."""
    import torch

    d = torch.from_numpy(np.ascontiguousarray(depth_m, dtype=F32))
    n = torch.where(torch.isinf(d), torch.tensor(far_m), d).clone()
    n *= 1000.0
    n -= near_m * 1000
    n /= far_m * 1000
    return (n * 255).type(dtype=torch.uint8).numpy()


def reference(depth_m):
    """hm, fmin, indent, true contact ranges of a (B, H, W) depth image in metres."""
    hm = height_map(depth_m)
    fmin, ind = frame_min(hm), indentation(hm)
    return hm, fmin, ind, contact_ranges(shifted(hm, fmin, ind))


def reference_mm(hm_mm):
    hm = np.asarray(hm_mm, F32)
    fmin, ind = frame_min(hm), indentation(hm)
    return fmin, ind, contact_ranges(shifted(hm, fmin, ind))


# -- input families: (H, W) -> (H, W) float32 height in mm -----------------------------------------------------------------------------
# far plane 29.0 mm, contact at 28.2 mm or below: indent = (4.5 - (min - 24)) mm > 0 and S < 0 exactly on the marked pixels
_FAR_MM, _HIT_MM = F32(29.0), F32(28.2)


def _flat(H, W):
    return np.full((H, W), _FAR_MM, F32)


def sphere_dent(H, W):
    yy, xx = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    r = F32(max(2.0, 0.3 * min(H, W)))
    q = ((yy - F32(int(0.45 * H))) ** 2 + (xx - F32(int(0.55 * W))) ** 2) / (r * r)
    return np.where(q < 1, F32(28.0) + F32(0.9) * q, _FAR_MM).astype(F32)


def row0_only(H, W):
    m = _flat(H, W)
    m[0, W // 3:W // 3 + max(1, W // 4)] = _HIT_MM
    return m


def last_row_and_column(H, W):
    m = _flat(H, W)
    m[H - 1, W // 2:] = _HIT_MM
    m[H // 2:, W - 1] = _HIT_MM
    return m


def corner_pixel(H, W):
    m = _flat(H, W)
    m[H - 1, W - 1] = _HIT_MM
    return m


def no_contact(H, W):
    return _flat(H, W)


def closer_than_case(H, W):
    return np.full((H, W), F32(23.5), F32)


def negative_ramp(H, W):
    """Heights below zero (and a -0.0): the unsigned atomicMax branch of the row / column minima."""
    m = np.full((H, W), F32(5.0), F32)
    m[H // 2, W // 4:] = -(np.arange(W - W // 4, dtype=F32) / F32(W))  # starts with -0.0
    m[H - 1, W - 1] = F32(-3.0)
    return m


def negative_zero(H, W):
    """-0.0 next to +0.0 as the smallest heights: the frame minimum is a zero, the rest lies above the press plane."""
    m = np.full((H, W), F32(6.0), F32)
    m[0, 0] = F32(-0.0)
    m[H - 1, W // 2] = F32(0.0)
    return m


MM_FAMILIES = [sphere_dent, row0_only, last_row_and_column, corner_pixel, no_contact, closer_than_case]
NEGATIVE_FAMILIES = [negative_ramp, negative_zero]


def inf_patches(H, W):
    """Depth in metres: the sphere dent with its top-left part, deepest pixel included, unseen by the camera (+inf -> far plane,
    GS:585-588)."""
    d = (sphere_dent(H, W) / F32(1000.0)).astype(F32)
    d[:int(0.45 * H) + 1, :int(0.55 * W) + 1] = np.inf
    return d


def depth_frames(H, W):
    """(7, H, W) float32 depth in metres, one frame per family, all inside [NEAR, FAR] or +inf."""
    return np.stack([(f(H, W) / F32(1000.0)).astype(F32) for f in MM_FAMILIES] + [inf_patches(H, W)])


def depth_frames_wide(H, W):
    """(3, H, W) depth outside the clipping range (no camera bytes for these): beyond the far plane, nearer than NEAR, -inf."""
    a = (sphere_dent(H, W) / F32(1000.0)).astype(F32) + F32(0.004)
    b = (last_row_and_column(H, W) / F32(1000.0)).astype(F32) - F32(0.015)
    c = (corner_pixel(H, W) / F32(1000.0)).astype(F32)
    c[0, 0] = -np.inf
    return np.stack([a, b, c])


def mm_frames(H, W):
    """(8, H, W) float32 height maps in mm for tacex_indentation_depth: the six families plus the two with negative heights."""
    return np.stack([f(H, W) for f in MM_FAMILIES + NEGATIVE_FAMILIES])


def batches(n):
    """Frame indices of the calls on n frames: B = 3 batches that cover every frame, then one B = 1 call per frame."""
    tri = [[i % n, (i + 1) % n, (i + 2) % n] for i in range(0, n, 3)]
    return tri + [[i] for i in range(n)]
