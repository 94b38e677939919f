"""NumPy restatement of `tacex_contact_points`, written from the function's comment in include/tacex_hip.h: which pixel is a contact
pixel, its rank, which rank a slot takes (with the Philox offset), and a point's float32 operations, every one rounded on its own.
Also the input frames of the GPU tests."""
import numpy as np
from marker_pattern_ref import philox4x32

f32 = np.float32
TAG = 0x70747363


def contact_mask(hm, frame_min, indent, min_depth_mm=0.0, labels=None, label=-1, rect=None):
    """One frame -> (mask (H,W) bool, S (H,W) f32, d (H,W) f32).  `rect` [row lo, row hi, col lo, col hi]: pixels outside are not looked at."""
    hm = np.asarray(hm, dtype=f32)
    H, W = hm.shape
    with np.errstate(invalid="ignore"):
        S = ((hm - f32(frame_min)).astype(f32) - f32(indent)).astype(f32)
        d = np.where(S < 0, -S, f32(0)).astype(f32)  # a NaN compares false
        mask = d > f32(min_depth_mm)
    if label >= 0:
        mask &= np.asarray(labels) == label
    if rect is not None:
        r0, r1, c0, c1 = max(int(rect[0]), 0), min(int(rect[1]), H - 1), max(int(rect[2]), 0), min(int(rect[3]), W - 1)
        inside = np.zeros((H, W), dtype=bool)
        if r0 <= r1 and c0 <= c1:
            inside[r0:r1 + 1, c0:c1 + 1] = True
        mask &= inside
    return mask, S, d


def jitter_offset(seed, g, call, N):
    """o = (uint64(w) * N) >> 32 with w word 0 of Philox(ctr (lo32(g), hi32(g), call, TAG), key (lo32(seed), hi32(seed)))."""
    g = int(g) & (2 ** 64 - 1)  # two's complement
    seed = int(seed)
    w = philox4x32(np.array([g & 0xFFFFFFFF, g >> 32, int(call) & 0xFFFFFFFF, TAG], dtype=np.uint64),
                   np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))
    return (int(w[0]) * int(N)) >> 32


def slot_ranks(N, K, pad, o=0):
    """(ranks (K,) int64 with -1 for an invalid slot, V)."""
    k = np.arange(K, dtype=object)  # Python integers: no overflow
    if N == 0:
        return np.full(K, -1, dtype=np.int64), 0
    if N > K:
        return np.array([(int(x) * N + o) // K for x in k], dtype=np.int64), K
    if pad:
        return np.arange(K, dtype=np.int64) % N, K
    r = np.arange(K, dtype=np.int64)
    return np.where(r < N, r, -1), N


def _ceil_div(a, b):
    return -((-a) // b)


def inverse_slot_range(r, N, K, o):
    """[lo, hi) of the slots whose source is rank r, for N > K."""
    return _ceil_div(r * K - o, N), _ceil_div((r + 1) * K - o, N)


def points_frame(hm, frame_min, indent, pixmm, K, pad=0, min_depth_mm=0.0, labels=None, label=-1, pose=None, unit=1.0, jitter=False, seed=0,
                 g=0, call=0, rect=None):
    """One frame -> dict(points (K,3), normals (K,3), depth (K,), pixels (K,2) int32, labels (K,) uint8, count (2,) int32)."""
    hm = np.asarray(hm, dtype=f32)
    H, W = hm.shape
    pixmm, unit = f32(pixmm), f32(unit)
    mask, S, d = contact_mask(hm, frame_min, indent, min_depth_mm, labels, label, rect)
    ii, jj = np.nonzero(mask)  # row-major order of the whole frame
    N = int(ii.size)
    o = jitter_offset(seed, g, call, N) if (jitter and N > K) else 0
    ranks, V = slot_ranks(N, K, pad, o)
    ok = ranks >= 0
    i, j = ii[ranks[ok]], jj[ranks[ok]]
    out = dict(points=np.zeros((K, 3), f32), normals=np.zeros((K, 3), f32), depth=np.zeros(K, f32), pixels=np.full((K, 2), -1, np.int32),
               labels=np.full(K, 255, np.uint8), count=np.array([N, V], np.int32))
    if not ok.any():
        return out
    cx0, cy0 = f32(W - 1) / f32(2), f32(H - 1) / f32(2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = ((j.astype(f32) - cx0).astype(f32) * pixmm).astype(f32)
        y = ((i.astype(f32) - cy0).astype(f32) * pixmm).astype(f32)
        z = S[i, j]
        gx, gy = np.zeros(i.size, f32), np.zeros(i.size, f32)
        if W > 1:
            jl, jr = np.maximum(j - 1, 0), np.minimum(j + 1, W - 1)
            gx = ((hm[i, jr] - hm[i, jl]).astype(f32) / ((jr - jl).astype(f32) * pixmm).astype(f32)).astype(f32)
        if H > 1:
            il, ir = np.maximum(i - 1, 0), np.minimum(i + 1, H - 1)
            gy = ((hm[ir, j] - hm[il, j]).astype(f32) / ((ir - il).astype(f32) * pixmm).astype(f32)).astype(f32)
        s = np.sqrt((((gx * gx).astype(f32) + (gy * gy).astype(f32)).astype(f32) + f32(1)).astype(f32)).astype(f32)
        n = np.stack([(gx / s).astype(f32), (gy / s).astype(f32), (f32(-1) / s).astype(f32)], axis=-1)
        q = np.stack([(unit * x).astype(f32), (unit * y).astype(f32), (unit * z).astype(f32)], axis=-1)
        if pose is not None:
            P = np.asarray(pose, dtype=f32).reshape(3, 4)
            p2, n2 = np.empty_like(q), np.empty_like(n)
            for r in range(3):
                p2[:, r] = ((((P[r, 0] * q[:, 0]).astype(f32) + (P[r, 1] * q[:, 1]).astype(f32)).astype(f32)
                             + (P[r, 2] * q[:, 2]).astype(f32)).astype(f32) + P[r, 3]).astype(f32)
                n2[:, r] = (((P[r, 0] * n[:, 0]).astype(f32) + (P[r, 1] * n[:, 1]).astype(f32)).astype(f32) + (P[r, 2] * n[:, 2]).astype(f32)).astype(f32)
            q, n = p2, n2
    out["points"][ok], out["normals"][ok], out["depth"][ok] = q, n, d[i, j]
    out["pixels"][ok] = np.stack([i, j], axis=-1).astype(np.int32)
    out["labels"][ok] = 0 if labels is None else np.asarray(labels)[i, j]
    return out


def points_batch(hm, frame_min, indent, pixmm, K, pad=0, min_depth_mm=0.0, labels=None, label=-1, pose=None, unit=1.0, jitter=False, seed=0,
                 frame_offset=0, call=0, rects=None):
    """(B,H,W) -> dict of (B,...) arrays."""
    frames = [points_frame(hm[b], frame_min[b], indent[b], pixmm, K, pad, min_depth_mm, None if labels is None else labels[b], label,
                           None if pose is None else pose[b], unit, jitter, seed, frame_offset + b, call, None if rects is None else rects[b])
              for b in range(hm.shape[0])]
    return {k: np.stack([f[k] for f in frames]) for k in frames[0]}


# ---- input frames of the GPU tests: fmin = 0.25, indent = 0.5, the gel's rest surface at 0.75 mm, background 2 mm above it ------------
FMIN, INDENT, REST, BACK = f32(0.25), f32(0.5), f32(0.75), f32(2.75)
BLOCK = 256  # the kernel's workgroup size (a wave walks 64 items of four pixels at a time)


def flat_frames(B, H, W):
    return np.full((B, H, W), BACK, dtype=f32), np.full(B, FMIN, f32), np.full(B, INDENT, f32)


def press(hm, b, lin, seed=0):
    """Lower the pixels at linear indices `lin` of frame b below the rest surface by 0.15 .. 0.45 mm (a smooth bump plus a hash of the
    index, so that neighbouring depths differ and gradients are not zero)."""
    H, W = hm.shape[1:]
    lin = np.asarray(lin, dtype=np.int64)
    i, j = lin // W, lin % W
    depth = 0.25 + 0.1 * np.sin(0.37 * i + 0.11 * seed) * np.cos(0.23 * j) + 0.1 * (((lin * 2654435761 + seed) >> 7) % 1000) / 1000.0
    hm[b].reshape(-1)[lin] = (REST - depth).astype(f32)
    return hm


def rotation(axis, angle):
    """Rodrigues: (3,3) float64."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def pose_rows(B, general=True):
    """(B,12) f32 [R | t] rows: identity, or a different rotation and translation per env."""
    rows = np.zeros((B, 3, 4), dtype=f32)
    for b in range(B):
        R = rotation((1.0 + b, -2.0, 0.5 * b + 0.3), 0.7 + 0.9 * b) if general else np.eye(3)
        t = (0.01 * (b + 1), -0.02, 0.3 + 0.05 * b) if general else (0, 0, 0)
        rows[b, :, :3], rows[b, :, 3] = R, t
    return rows.reshape(B, 12)
