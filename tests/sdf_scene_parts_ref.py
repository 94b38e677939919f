"""NumPy float32 restatement of `tacex_height_map_from_sdf_scene_parts` (include/tacex_hip.h): TEST INFRASTRUCTURE ONLY.

The march of tests/sdf_scene_ref.py - its slots, tile votes, clipping, tap and smooth minimum are imported, not written again - with
the owner of the header's contract beside the field.  In every evaluation of the fold `own` starts at 255; a slot s that is evaluated
(live for the pixel's tile, and not skipped by the "hard union too far away" rule) sets own = s exactly when the comparison inside
smin takes its second argument, with f the value before the fold:
    union: u < f        subtract: u < -f        intersect: -u < -f
with or without a blend.  s is the slot's index in 0..K-1.  The owner written for a pixel is `own` of the evaluation that assigned
its depth (the f < tol hit, or the grazing-ray rule), and 255 wherever the stored height is the far clip."""
import numpy as np
import sdf_scene_ref as S

F32 = S.F32
NO_OWNER = 255
KINDS = ("union", "blended union", "subtract", "blended subtract", "intersect", "blended intersect")


def _frame(slots, H, W, pixmm, near, far, max_steps, tol):
    out, owner = np.full(H * W, far, F32), np.full(H * W, NO_OWNER, np.uint8)
    vox_env = S.TWO30
    for s in slots:
        if s is not None and s["op"] == S.UNION:
            vox_env = s["vox"] if s["vox"] < vox_env else vox_env
    y, x = (c.reshape(-1) for c in np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij"))
    tile_of = lambda t: np.repeat(np.repeat(t, S.TILE_H, 0), S.TILE_W, 1)[:H, :W].reshape(-1)  # noqa: E731
    rays = []  # per non-empty slot: (slot index, slot, live per pixel, b, lo, hi, meets)
    for index, s in enumerate(slots):
        if s is None:
            continue
        b, lo_s, hi_s, meets = S._clip(s, x, y, near, far)
        rays.append((index, s, tile_of(S._tile_live(s, H, W, pixmm)), b, lo_s, hi_s, meets))
    # a tile without a live union slot is far clip: none of its pixels has an interval below
    lo, hi, active = np.zeros(H * W, F32), np.zeros(H * W, F32), np.zeros(H * W, bool)
    for _, s, live_px, b, lo_s, hi_s, meets in rays:
        if s["op"] != S.UNION:
            continue
        m = live_px & meets
        lo = np.where(m & (~active | (lo_s < lo)), lo_s, lo)
        hi = np.where(m & (~active | (hi_s > hi)), hi_s, hi)
        active |= m
    live = np.flatnonzero(active)
    z, hi_l = lo[live], hi[live]
    for n in range(max_steps):
        if live.size == 0:
            break
        f = np.full(live.size, S.TWO30, F32)
        own = np.full(live.size, NO_OWNER, np.uint8)
        for index, s, live_px, b, lo_s, hi_s, meets in rays:
            on = live_px[live]
            if not on.any():
                continue
            q = [b[a][live] + (z * s["az"][a]) for a in range(3)]
            m, w, ex = [], [], []
            for a in range(3):
                c = np.where(q[a] > F32(0), q[a], F32(0))
                c = np.where(c < s["hmax"][a], c, s["hmax"][a]).astype(F32)
                ma = np.minimum(np.floor(c).astype(np.int64), s["N"][a] - 2)
                m.append(ma)
                w.append(c - ma.astype(F32))
                ex.append(q[a] - c)
            inside = meets[live] & (z >= lo_s[live]) & (z <= hi_s[live])
            e2 = (((ex[0] * ex[0]) + (ex[1] * ex[1])) + (ex[2] * ex[2])) * s["vox2"]
            hard_union = s["op"] == S.UNION and not s["blend"] > 0
            skip = ~inside & (np.sqrt(e2) >= f) if hard_union else np.zeros(live.size, bool)
            evaluated = on & ~skip
            vol = s["vol"]
            v = lambda dz, dy, dx: vol[m[2] + dz, m[1] + dy, m[0] + dx]  # noqa: E731
            e = [[S._lerp(v(dz, dy, 0), v(dz, dy, 1), w[0]) for dy in (0, 1)] for dz in (0, 1)]
            g = [S._lerp(e[dz][0], e[dz][1], w[1]) for dz in (0, 1)]
            t = S._lerp(g[0], g[1], w[2])
            u = ((t - s["level"]) * s["scale"]) * s["step_scale"]
            p = np.where(u > F32(0), u, F32(0))
            u = np.where(inside, u, np.sqrt(e2 + (p * p))).astype(F32)
            k = s["blend"]
            if s["op"] == S.UNION:
                takes, new = u < f, S._smin(f, u, k)
            elif s["op"] == S.SUBTRACT:
                takes, new = u < -f, -S._smin(-f, u, k)
            else:
                takes, new = -u < -f, -S._smin(-f, -u, k)
            own = np.where(evaluated & takes, np.uint8(index), own)
            f = np.where(evaluated, new, f)
        hit = f < tol
        out[live[hit]], owner[live[hit]] = z[hit], own[hit]
        z = z + f
        keep = ~hit & (z <= hi_l)
        if n == max_steps - 1:
            graze = keep & (f < vox_env)
            out[live[graze]], owner[live[graze]] = z[graze], own[graze]
        live, z, hi_l = live[keep], z[keep], hi_l[keep]
    shown = out < far
    return np.where(shown, out, far).astype(F32).reshape(H, W), np.where(shown, owner, np.uint8(NO_OWNER)).reshape(H, W)


def height_and_part_map(voxels, vi, vf, part_ids, part_pose, part_ops, H, W, pixmm=0.0295, near_clip_mm=24.0, far_clip_mm=29.0, max_steps=32,
                        tol_mm=1e-4):
    """((B, H, W) float32 height map, (B, H, W) uint8 owner): the contract, frame by frame; arguments as `sdf_scene_ref.height_map`."""
    voxels, part_pose = np.asarray(voxels, F32), np.asarray(part_pose, F32)
    part_ids, part_ops = np.asarray(part_ids), np.asarray(part_ops)
    B, K = part_ids.shape
    hm, owner = np.empty((B, H, W), F32), np.empty((B, H, W), np.uint8)
    with np.errstate(all="ignore"):
        for b in range(B):
            slots = [S._slot(voxels, vi, vf, int(part_ids[b, k]), int(part_ops[b, k]), part_pose[b, k], F32(pixmm)) for k in range(K)]
            hm[b], owner[b] = _frame(slots, H, W, F32(pixmm), F32(near_clip_mm), F32(far_clip_mm), int(max_steps), F32(tol_mm))
    return hm, owner


def owner_kinds(owner, part_ops, part_pose):
    """(B, 6) pixels per env owned by a slot of each of `KINDS` (operation, hard or blended)."""
    B, K = np.asarray(part_ops).shape
    counts = np.zeros((B, 6), np.int64)
    for b in range(B):
        for k in range(K):
            if 0 <= part_ops[b, k] <= 2:
                counts[b, 2 * int(part_ops[b, k]) + int(part_pose[b, k, 14] > 0)] += int((owner[b] == k).sum())
    return counts
