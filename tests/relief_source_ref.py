"""NumPy float32 restatement of `tacex_height_map_from_relief` (include/tacex_hip.h): TEST INFRASTRUCTURE ONLY.

Written from the header's text, one rounding to float32 per operation, in the order of its parentheses.  The HIP kernel
(tacex_amd/csrc/relief_source.hip, built with -ffp-contract=off) must agree bit for bit; `frame_outputs` restates what
`tacex_indentation_depth` reports for a map (csrc/frame_rows.h)."""
import numpy as np

F32 = np.float32
TWO30 = F32(1073741824.0)


def library(tiles):
    """[(height (Th,Tw) f32, pitch_mm, wrap, anchor (u0, v0) or None)] -> (texels (N,), tiles_i (P,4) int32, tiles_f (P,4) f32)."""
    texels, ti, tf, first = [], [], [], 0
    for h, pitch, wrap, anchor in tiles:
        h = np.asarray(h, F32)
        Th, Tw = h.shape
        u0, v0 = ((Tw - 1) / 2.0, (Th - 1) / 2.0) if anchor is None else anchor
        ti.append([first, Th, Tw, int(bool(wrap))])
        tf.append([pitch, h[np.isfinite(h)].max(), u0, v0])
        texels.append(h.reshape(-1))
        first += h.size
    return np.concatenate(texels).astype(F32), np.asarray(ti, np.int32), np.asarray(tf, F32)


def _sample(x, y, tex, Th, Tw, wrap, tf, p, gel_top, far_clip):
    pitch, top, u0, v0 = (F32(v) for v in tf)
    m00, m01, m02, m10, m11, m12, press, t0, tx, ty, carrier, R, gain, du, dv = (F32(v) for v in p[:15])
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((m00 * x) + (m01 * y)) + m02
        v = ((m10 * x) + (m11 * y)) + m12
        s = (u - u0) * pitch
        t = (v - v0) * pitch
        carrier = 1 if carrier == F32(1) else (2 if carrier == F32(2) else 0)
        if carrier in (1, 2):
            q = (s * s) + (t * t) if carrier == 1 else t * t
            RR = R * R
            c = np.where(q <= RR, R - np.sqrt(np.maximum(RR - q, F32(0))), F32(np.inf)).astype(F32)
        else:
            c = np.zeros_like(u)
        uu, vv = u + du, v + dv
        ok = (np.abs(uu) < TWO30) & (np.abs(vv) < TWO30)
        us, vs = np.where(ok, uu, F32(0)), np.where(ok, vv, F32(0))
        fu, fv = np.floor(us), np.floor(vs)
        a, b = us - fu, vs - fv
        i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
        if wrap:
            i0, j0 = np.mod(i0, Tw), np.mod(j0, Th)
            i1, j1 = np.mod(i0 + 1, Tw), np.mod(j0 + 1, Th)
        else:
            ok &= (us >= F32(0)) & (us <= F32(Tw - 1)) & (vs >= F32(0)) & (vs <= F32(Th - 1))
            i0, j0 = np.clip(i0, 0, Tw - 1), np.clip(j0, 0, Th - 1)  # (the lower clip only keeps the indices of !ok samples legal)
            i1, j1 = np.minimum(i0 + 1, Tw - 1), np.minimum(j0 + 1, Th - 1)
        T = tex.reshape(Th, Tw)
        h00, h01, h10, h11 = T[j0, i0], T[j0, i1], T[j1, i0], T[j1, i1]
        ga, gb = F32(1) - a, F32(1) - b
        h = (((h00 * ga) + (h01 * a)) * gb) + (((h10 * ga) + (h11 * a)) * b)
        h = np.where(ok, h, F32(-np.inf)).astype(F32)
        depth = (((F32(gel_top) - press) + c) + (gain * (top - h))) + ((t0 + (tx * x)) + (ty * y))
        return np.where(depth < F32(far_clip), depth, F32(far_clip)).astype(F32)


def height_map(texels, tiles_i, tiles_f, ids, pose, H, W, gel_top_mm=28.5, far_clip_mm=29.0, samples=1):
    """(B, H, W) float32: the contract, frame by frame.  ids None: tile 0."""
    assert samples in (1, 4)
    texels, pose = np.asarray(texels, F32), np.asarray(pose, F32)
    B = pose.shape[0]
    y, x = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    out = np.empty((B, H, W), F32)
    for b in range(B):
        k = 0 if ids is None else int(ids[b])
        if not 0 <= k < tiles_i.shape[0]:
            out[b] = F32(far_clip_mm)
            continue
        first, Th, Tw, wrap = (int(v) for v in tiles_i[k])
        one = lambda xs, ys: _sample(xs, ys, texels[first:first + Th * Tw], Th, Tw, wrap, tiles_f[k], pose[b], gel_top_mm, far_clip_mm)
        if samples == 1:
            out[b] = one(x, y)
        else:
            q = F32(0.25)
            d0, d1, d2, d3 = one(x - q, y - q), one(x + q, y - q), one(x - q, y + q), one(x + q, y + q)
            out[b] = ((d0 + d1) + (d2 + d3)) * q
    return out


def frame_outputs(hm, gelpad_height, gelpad_to_camera_min_distance, block_cols_ok=None):
    """(frame_min (B,), indent (B,), rows (B,4) int32) of `tacex_indentation_depth` with ranges for maps with W % 4 == 0 and
    H <= 2048: S = (min of the row or column - frame min) - indent < 0 marks contact; (H, -1) / (W, -1) without any; the column
    range is the whole frame when the row kernel's block is no multiple of the row's float4 count."""
    hm = np.asarray(hm, F32)
    B, H, W = hm.shape
    gh, gd = F32(gelpad_height), F32(gelpad_to_camera_min_distance)
    if block_cols_ok is None:
        w4 = W // 4
        nt = (1024 // w4) * w4 if w4 <= 1024 else 1024
        if nt < 512 or nt & 63:
            nt = 1024
        block_cols_ok = W <= 2048 and nt % w4 == 0
    fmin = hm.reshape(B, -1).min(axis=1).astype(F32)
    d = np.maximum(fmin / F32(1000.0) - gd, F32(0))
    indent = np.where(d <= gh, (gh - d) * F32(1000.0), F32(0)).astype(F32)
    rows = np.empty((B, 4), np.int32)
    for b in range(B):
        r = np.nonzero(((hm[b].min(axis=1) - fmin[b]) - indent[b]) < 0)[0]
        rows[b, :2] = (r[0], r[-1]) if r.size else (H, -1)
        if block_cols_ok:
            c = np.nonzero(((hm[b].min(axis=0) - fmin[b]) - indent[b]) < 0)[0]
            rows[b, 2:] = (c[0], c[-1]) if c.size else (W, -1)
        else:
            rows[b, 2:] = (0, W - 1)
    return fmin, indent, rows


def pose_rows(tiles_f, ids, cx, cy, yaw, press_mm, pixmm=0.0295, scale=1.0, tilt=(0.0, 0.0), carrier=0, radius_mm=0.0, gain=1.0,
              shift=(0.0, 0.0)):
    """(B,16) float32 pose rows by the formulas of `ReliefHeightMapSource.set_pose`, in float64 and rounded once (a test chooses its
    poses with this; the kernel is pinned against `height_map` for whatever pose it is given).  Arguments broadcast over B."""
    ids = np.asarray(ids)
    B = ids.shape[0]
    f = np.asarray(tiles_f, np.float64)[np.clip(ids, 0, len(tiles_f) - 1)]
    bc = lambda v: np.broadcast_to(np.asarray(v, np.float64), (B,))
    cx, cy, yaw, scale = bc(cx), bc(cy), bc(yaw), bc(scale)
    k = pixmm / (f[:, 0] * scale)
    p = np.zeros((B, 16), np.float64)
    p[:, 0], p[:, 1] = k * np.cos(yaw), k * np.sin(yaw)
    p[:, 3], p[:, 4] = -k * np.sin(yaw), k * np.cos(yaw)
    p[:, 2] = f[:, 2] - (p[:, 0] * cx + p[:, 1] * cy)
    p[:, 5] = f[:, 3] - (p[:, 3] * cx + p[:, 4] * cy)
    p[:, 6] = bc(press_mm)
    p[:, 8], p[:, 9] = bc(tilt[0]), bc(tilt[1])
    p[:, 7] = -(p[:, 8] * cx + p[:, 9] * cy)
    p[:, 10], p[:, 11], p[:, 12] = bc(carrier), bc(radius_mm), bc(gain)
    p[:, 13], p[:, 14] = bc(shift[0]), bc(shift[1])
    return p.astype(F32)
