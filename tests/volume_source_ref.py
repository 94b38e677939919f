"""NumPy float32 restatement of `tacex_height_map_from_sdf` (include/tacex_hip.h): TEST INFRASTRUCTURE ONLY.

Written from the header's text, one rounding to float32 per operation, in the order of its parentheses.  The rays of a frame are
marched together under masks, so every pixel sees the sequence of roundings a lane of the HIP kernel
(tacex_amd/csrc/volume_source.hip, built with -ffp-contract=off) sees: the two must agree bit for bit.  `frame_outputs` of
relief_source_ref.py restates what `tacex_indentation_depth` reports for the map."""
import numpy as np

F32 = np.float32
TWO30 = F32(1073741824.0)


def library(volumes):
    """[(sdf (D,Hv,Wv) f32, pitch_mm, anchor (i0, j0, k0) or None, step_scale)] -> (voxels (N,), vi (P,4) int32, vf (P,8) f32)."""
    voxels, vi, vf, first = [], [], [], 0
    for s, pitch, anchor, step in volumes:
        s = np.asarray(s, F32)
        D, Hv, Wv = s.shape
        i0, j0, k0 = ((Wv - 1) / 2.0, (Hv - 1) / 2.0, (D - 1) / 2.0) if anchor is None else anchor
        vi.append([first, D, Hv, Wv])
        vf.append([pitch, i0, j0, k0, step, 0, 0, 0])
        voxels.append(s.reshape(-1))
        first += s.size
    return np.concatenate(voxels).astype(F32), np.asarray(vi, np.int32), np.asarray(vf, F32)


def half_space(shape=(2, 2, 2), pitch=1.0):
    """sdf = -z_obj on a (D, Hv, Wv) grid: the object fills z_obj > 0."""
    D = shape[0]
    z = (np.arange(D, dtype=np.float64) - (D - 1) / 2.0) * pitch
    return np.broadcast_to(-z[:, None, None], shape).astype(F32)


def three_volumes():
    """[(sdf, pitch_mm, anchor, step_scale)] of unequal, non-cubic grids: a half space on 2x2x2 at 1 mm; a capsule along x (radius
    0.35, segment 2.5 mm) on 5x9x17 at 0.25 mm, its anchor off centre, step_scale 0.5; the unit ball on 24^3 at 0.1 mm."""
    grid = lambda n, pitch: (np.arange(n, dtype=np.float64) - (n - 1) / 2.0) * pitch  # noqa: E731
    z, y, x = grid(5, 0.25)[:, None, None], grid(9, 0.25)[None, :, None], grid(17, 0.25)[None, None, :]
    cap = (np.sqrt((x - np.clip(x, -1.25, 1.25)) ** 2 + y * y + z * z) - 0.35).astype(F32)
    g = grid(24, 0.1)
    ball = (np.sqrt(g[None, None, :] ** 2 + g[None, :, None] ** 2 + g[:, None, None] ** 2) - 1.0).astype(F32)
    return [(half_space(), 1.0, None, 1.0), (cap, 0.25, (7.0, 4.5, 2.0), 0.5), (ball, 0.1, None, 1.0)]


def _frame(voxels, vi_row, vf_row, r, H, W, pixmm, near, far, max_steps, tol, stats):
    """One frame whose id is valid: (H, W) float32."""
    out = np.full((H, W), far, F32)
    first, D, Hv, Wv = (int(v) for v in vi_row)
    if first < 0 or min(D, Hv, Wv) < 2 or first + D * Hv * Wv > voxels.shape[0]:
        return out
    N = (Wv, Hv, D)
    pitch, step_scale = F32(vf_row[0]), F32(vf_row[4])
    anchor = [F32(vf_row[1]), F32(vf_row[2]), F32(vf_row[3])]
    r = np.asarray(r, F32)
    tx, ty, tz, scale, level = r[9], r[10], r[11], r[12], r[13]
    with np.errstate(all="ignore"):
        g = scale * pitch
        inv = F32(1) / g
        vox = g
        ax = [(r[a] * pixmm) * inv for a in range(3)]
        ay = [(r[3 + a] * pixmm) * inv for a in range(3)]
        az = [r[6 + a] * inv for a in range(3)]
        q0 = [anchor[a] - ((((r[a] * tx) + (r[3 + a] * ty)) + (r[6 + a] * tz)) * inv) for a in range(3)]
        par = [not (np.abs(az[a]) >= F32(1e-12)) for a in range(3)]
        ia = [F32(0) if par[a] else F32(1) / az[a] for a in range(3)]
        hmax = [F32(N[a] - 1) for a in range(3)]
        ok = bool(g > 0) and bool(step_scale > 0) and bool(np.abs(level) < TWO30)
        ok = ok and all(bool(np.abs(c) < TWO30) for c in ax + ay + az + q0)
        if not ok:
            return out
        y, x = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
        b = [(q0[a] + (x * ax[a])) + (y * ay[a]) for a in range(3)]
        lo, hi = np.full((H, W), near, F32), np.full((H, W), far, F32)
        active = np.ones((H, W), bool)
        for a in range(3):
            active &= np.abs(b[a]) < TWO30
            if par[a]:
                active &= (b[a] >= F32(0)) & (b[a] <= hmax[a])
            else:
                t1, t2 = (F32(0) - b[a]) * ia[a], (hmax[a] - b[a]) * ia[a]
                tn, tf = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
                lo, hi = np.where(tn > lo, tn, lo), np.where(tf < hi, tf, hi)
        active &= lo <= hi
        vol = voxels[first:first + D * Hv * Wv].reshape(D, Hv, Wv)
        lerp = lambda p, q, t: p + (t * (q - p))  # noqa: E731
        # the active pixels as flat arrays; `live` shrinks as rays end
        live = np.flatnonzero(active.reshape(-1))
        depth = out.reshape(-1)
        z, hi_l = lo.reshape(-1)[live], hi.reshape(-1)[live]
        bl = [c.reshape(-1)[live] for c in b]
        stats["covered"] += live.size
        for n in range(max_steps):
            if live.size == 0:
                break
            stats["taps"] += live.size
            m, w = [], []
            for a in range(3):
                c = bl[a] + (z * az[a])
                c = np.where(c > F32(0), c, F32(0))
                c = np.where(c < hmax[a], c, hmax[a]).astype(F32)
                ma = np.minimum(np.floor(c).astype(np.int64), N[a] - 2)
                m.append(ma)
                w.append(c - ma.astype(F32))
            v = lambda dz, dy, dx: vol[m[2] + dz, m[1] + dy, m[0] + dx]  # noqa: E731
            e = [[lerp(v(dz, dy, 0), v(dz, dy, 1), w[0]) for dy in (0, 1)] for dz in (0, 1)]
            f = [lerp(e[dz][0], e[dz][1], w[1]) for dz in (0, 1)]
            s = lerp(f[0], f[1], w[2])
            d = ((s - level) * scale) * step_scale
            hit = d < tol
            depth[live[hit]] = z[hit]
            stats["hits"] += int(hit.sum())
            if n == 0:
                stats["entered_inside"] += int(hit.sum())
            z = z + d
            gone = ~hit & ~(z <= hi_l)
            keep = ~hit & ~gone
            if n == max_steps - 1:
                graze = keep & (d < vox)
                depth[live[graze]] = z[graze]
                stats["grazing"] += int(graze.sum())
                stats["unconverged"] += int(keep.sum())
            live, z, hi_l, bl = live[keep], z[keep], hi_l[keep], [c[keep] for c in bl]
        out = depth.reshape(H, W)
        return np.where(out < far, out, far).astype(F32)


def height_map(voxels, vi, vf, ids, pose, H, W, pixmm=0.0295, near_clip_mm=24.0, far_clip_mm=29.0, max_steps=32, tol_mm=1e-4,
               stats=None):
    """(B, H, W) float32: the contract, frame by frame.  ids None: volume 0.  `stats` (a dict) collects debug counts over the
    call: covered (pixels with a non-empty interval), taps, hits, entered_inside (hits of the first tap), unconverged (rays that
    used every tap), grazing (those of them the grazing-ray rule turned into a depth)."""
    voxels, pose = np.asarray(voxels, F32), np.asarray(pose, F32)
    stats = {} if stats is None else stats
    for k in ("covered", "taps", "hits", "entered_inside", "unconverged", "grazing"):
        stats.setdefault(k, 0)
    B = pose.shape[0]
    out = np.empty((B, H, W), F32)
    for b in range(B):
        k = 0 if ids is None else int(ids[b])
        if not 0 <= k < vi.shape[0]:
            out[b] = F32(far_clip_mm)
            continue
        out[b] = _frame(voxels, vi[k], vf[k], pose[b], H, W, F32(pixmm), F32(near_clip_mm), F32(far_clip_mm), int(max_steps),
                        F32(tol_mm), stats)
    return out


def quat_matrix(q):
    """Rotation matrix (float64) of the quaternion (w, x, y, z), normalised first."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def pose_row(R, t_mm, scale=1.0, level_mm=0.0):
    """(16,) float32 pose row from a rotation matrix (object -> camera), a translation [mm], scale and level."""
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t_mm, np.float64), [scale, level_mm, 0.0, 0.0]]).astype(F32)
