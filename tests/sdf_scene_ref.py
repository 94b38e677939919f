"""NumPy float32 restatement of `tacex_height_map_from_sdf_scene` (include/tacex_hip.h): TEST INFRASTRUCTURE ONLY.

Written from the header's text, one rounding to float32 per operation, in the order of its parentheses.  The rays of a frame are
marched together under masks - a slot takes part in a pixel's fold where it is live for the pixel's 32 x 8 tile -, so every pixel sees
the sequence of roundings a lane of the HIP kernel (tacex_amd/csrc/sdf_scene.hip, built with -ffp-contract=off) sees: the two must
agree bit for bit.  `library`, `three_volumes`, `quat_matrix` and `pose_row` are those of volume_source_ref.py."""
import numpy as np
from volume_source_ref import library, pose_row, quat_matrix, three_volumes  # noqa: F401

F32 = np.float32
TWO30 = F32(1073741824.0)
TILE_W, TILE_H = 32, 8
UNION, SUBTRACT, INTERSECT = 0, 1, 2
OP_NAMES = ("union", "subtract", "intersect")
STATS = ("covered", "taps", "hits", "entered_inside", "unconverged", "grazing", "changed_union", "changed_subtract", "changed_intersect",
         "blended", "outside", "outside_skipped", "tiles", "dead_tiles", "empty_slots", "culled_slots", "overlap_rays", "subtract_only_rays")


def scene_row(R, t_mm, scale=1.0, level_mm=0.0, blend_mm=0.0):
    """(16,) float32 slot pose row: `pose_row` with blend_mm in its place."""
    r = pose_row(R, t_mm, scale, level_mm)
    r[14] = blend_mm
    return r


def _slot(voxels, vi, vf, idv, op, r, pixmm):
    """The slot's coefficients (a dict), or None when the slot is empty."""
    r = np.asarray(r, F32)
    blend = r[14]
    if not (0 <= op <= 2) or not bool(np.abs(blend) < TWO30) or not 0 <= idv < vi.shape[0]:
        return None
    first, D, Hv, Wv = (int(v) for v in vi[idv])
    if first < 0 or min(D, Hv, Wv) < 2 or first + D * Hv * Wv > voxels.shape[0]:
        return None
    N = (Wv, Hv, D)
    pitch, step_scale = F32(vf[idv, 0]), F32(vf[idv, 4])
    anchor = [F32(vf[idv, 1]), F32(vf[idv, 2]), F32(vf[idv, 3])]
    tx, ty, tz, scale, level = r[9], r[10], r[11], r[12], r[13]
    g = scale * pitch
    inv = F32(1) / g
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
        return None
    # the image of the grid's box: the bounding rectangle of its eight corners [mm]
    X, Y = [], []
    for c in range(8):
        o = [(((hmax[a] if c >> a & 1 else F32(0)) - anchor[a]) * g) for a in range(3)]
        X.append((((r[0] * o[0]) + (r[1] * o[1])) + (r[2] * o[2])) + tx)
        Y.append((((r[3] * o[0]) + (r[4] * o[1])) + (r[5] * o[2])) + ty)
    return dict(op=int(op), blend=blend, N=N, ax=ax, ay=ay, az=az, q0=q0, par=par, ia=ia, hmax=hmax, scale=scale, level=level,
                step_scale=step_scale, vox=g, vox2=g * g, rect=(min(X), max(X), min(Y), max(Y)),
                vol=voxels[first:first + D * Hv * Wv].reshape(D, Hv, Wv))


def _tile_live(s, H, W, pixmm):
    """(tile rows, tile columns) bool: the slot is live for the tile."""
    ty, tx = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    if s["op"] == INTERSECT:
        return np.ones((ty, tx), bool)
    xmin, xmax, ymin, ymax = s["rect"]
    margin = pixmm + s["blend"] if s["blend"] > 0 else pixmm
    tc, tr = np.arange(tx), np.arange(ty)
    x0, x1 = (TILE_W * tc).astype(F32) * pixmm, (TILE_W * tc + (TILE_W - 1)).astype(F32) * pixmm
    y0, y1 = (TILE_H * tr).astype(F32) * pixmm, (TILE_H * tr + (TILE_H - 1)).astype(F32) * pixmm
    in_x = (xmax + margin >= x0) & (xmin - margin <= x1)
    in_y = (ymax + margin >= y0) & (ymin - margin <= y1)
    return in_y[:, None] & in_x[None, :]


def _clip(s, x, y, near, far):
    """The pixel's ray in the slot's grid: (b[3], lo, hi, meets)."""
    b = [(s["q0"][a] + (x * s["ax"][a])) + (y * s["ay"][a]) for a in range(3)]
    lo, hi = np.full(x.shape, near, F32), np.full(x.shape, far, F32)
    meets = np.ones(x.shape, bool)
    for a in range(3):
        meets &= np.abs(b[a]) < TWO30
        if s["par"][a]:
            meets &= (b[a] >= F32(0)) & (b[a] <= s["hmax"][a])
        else:
            t1, t2 = (F32(0) - b[a]) * s["ia"][a], (s["hmax"][a] - b[a]) * s["ia"][a]
            tn, tf = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
            lo, hi = np.where(tn > lo, tn, lo), np.where(tf < hi, tf, hi)
    meets &= lo <= hi
    return b, lo, hi, meets


def _smin(a, b, k):
    mn = np.where(b < a, b, a)
    if k > 0:
        t = k - np.abs(a - b)
        t = np.where(t > F32(0), t, F32(0))
        h = t / k
        mn = mn - ((h * h) * (k * F32(0.25)))
    return mn.astype(F32)


def _lerp(p, q, t):
    return p + (t * (q - p))


def _frame(slots, H, W, pixmm, near, far, max_steps, tol, stats):
    out = np.full(H * W, far, F32)
    some = [s for s in slots if s is not None]
    stats["empty_slots"] += len(slots) - len(some)
    tiles_y, tiles_x = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    stats["tiles"] += tiles_y * tiles_x
    vox_env = TWO30
    for s in some:
        if s["op"] == UNION:
            vox_env = s["vox"] if s["vox"] < vox_env else vox_env
    y, x = (c.reshape(-1) for c in np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij"))
    tile_of = lambda t: np.repeat(np.repeat(t, TILE_H, 0), TILE_W, 1)[:H, :W].reshape(-1)  # noqa: E731
    union_tiles = np.zeros((tiles_y, tiles_x), bool)
    rays = []  # per non-empty slot: (slot, live per pixel, b, lo, hi, meets)
    for s in some:
        t = _tile_live(s, H, W, pixmm)
        stats["culled_slots"] += int((~t).sum())
        if s["op"] == UNION:
            union_tiles |= t
        b, lo_s, hi_s, meets = _clip(s, x, y, near, far)
        rays.append((s, tile_of(t), b, lo_s, hi_s, meets))
    stats["dead_tiles"] += int((~union_tiles).sum())
    met = [r[5] for r in rays]
    if met:
        stats["overlap_rays"] += int((np.sum(met, 0) >= 2).sum())
        only = np.zeros(H * W, bool)
        for r in rays:
            only |= r[5] & (r[0]["op"] == SUBTRACT)
        for r in rays:
            only &= ~(r[5] & (r[0]["op"] == UNION))
        stats["subtract_only_rays"] += int(only.sum())
    # the interval: over the live union slots the ray meets
    lo, hi, active = np.zeros(H * W, F32), np.zeros(H * W, F32), np.zeros(H * W, bool)
    for s, live_px, b, lo_s, hi_s, meets in rays:
        if s["op"] != UNION:
            continue
        m = live_px & meets
        lo = np.where(m & (~active | (lo_s < lo)), lo_s, lo)
        hi = np.where(m & (~active | (hi_s > hi)), hi_s, hi)
        active |= m
    live = np.flatnonzero(active)
    stats["covered"] += live.size
    z, hi_l = lo[live], hi[live]
    for n in range(max_steps):
        if live.size == 0:
            break
        f = np.full(live.size, TWO30, F32)
        for s, live_px, b, lo_s, hi_s, meets in rays:
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
            hard_union = s["op"] == UNION and not s["blend"] > 0
            skip = ~inside & (np.sqrt(e2) >= f) if hard_union else np.zeros(live.size, bool)
            tapped = on & ~skip
            stats["taps"] += int(tapped.sum())
            stats["outside"] += int((tapped & ~inside).sum())
            stats["outside_skipped"] += int((on & skip).sum())
            vol = s["vol"]
            v = lambda dz, dy, dx: vol[m[2] + dz, m[1] + dy, m[0] + dx]  # noqa: E731
            e = [[_lerp(v(dz, dy, 0), v(dz, dy, 1), w[0]) for dy in (0, 1)] for dz in (0, 1)]
            g = [_lerp(e[dz][0], e[dz][1], w[1]) for dz in (0, 1)]
            t = _lerp(g[0], g[1], w[2])
            u = ((t - s["level"]) * s["scale"]) * s["step_scale"]
            p = np.where(u > F32(0), u, F32(0))
            u = np.where(inside, u, np.sqrt(e2 + (p * p))).astype(F32)
            k = s["blend"]
            if s["op"] == UNION:
                new = _smin(f, u, k)
            elif s["op"] == SUBTRACT:
                new = -_smin(-f, u, k)
            else:
                new = -_smin(-f, -u, k)
            new = np.where(tapped, new, f)
            changed = new.view(np.uint32) != f.view(np.uint32)
            stats["changed_" + OP_NAMES[s["op"]]] += int(changed.sum())
            if k > 0:
                hard = {UNION: np.where(u < f, u, f), SUBTRACT: np.where(-u > f, -u, f), INTERSECT: np.where(u > f, u, f)}[s["op"]]
                stats["blended"] += int((tapped & (new != hard)).sum())
            f = new
        hit = f < tol
        out[live[hit]] = z[hit]
        stats["hits"] += int(hit.sum())
        if n == 0:
            stats["entered_inside"] += int(hit.sum())
        z = z + f
        gone = ~hit & ~(z <= hi_l)
        keep = ~hit & ~gone
        if n == max_steps - 1:
            graze = keep & (f < vox_env)
            out[live[graze]] = z[graze]
            stats["grazing"] += int(graze.sum())
            stats["unconverged"] += int(keep.sum())
        live, z, hi_l = live[keep], z[keep], hi_l[keep]
    return np.where(out < far, out, far).astype(F32).reshape(H, W)


def height_map(voxels, vi, vf, part_ids, part_pose, part_ops, H, W, pixmm=0.0295, near_clip_mm=24.0, far_clip_mm=29.0, max_steps=32,
               tol_mm=1e-4, stats=None):
    """(B, H, W) float32: the contract, frame by frame.  part_ids, part_ops (B, K), part_pose (B, K, 16).  `stats` (a dict)
    collects debug counts over the call: covered (pixels with an interval), taps (slot evaluations that read voxels), hits,
    entered_inside (hits of the first step), unconverged (rays that used every step), grazing (those of them the grazing-ray rule
    turned into a depth), changed_union / _subtract / _intersect (folds that changed f), blended (folds a blend width changed),
    outside (taps through the bound outside a box), outside_skipped (hard unions too far away to matter: no tap), tiles, dead_tiles
    (tiles without a live union slot), empty_slots, culled_slots (slot x tile pairs that are not live), overlap_rays (pixels whose
    ray meets two boxes or more), subtract_only_rays (pixels whose ray meets a subtract slot's box and no union slot's)."""
    voxels, part_pose = np.asarray(voxels, F32), np.asarray(part_pose, F32)
    part_ids, part_ops = np.asarray(part_ids), np.asarray(part_ops)
    stats = {} if stats is None else stats
    for k in STATS:
        stats.setdefault(k, 0)
    B, K = part_ids.shape
    out = np.empty((B, H, W), F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            slots = [_slot(voxels, vi, vf, int(part_ids[b, k]), int(part_ops[b, k]), part_pose[b, k], F32(pixmm)) for k in range(K)]
            out[b] = _frame(slots, H, W, F32(pixmm), F32(near_clip_mm), F32(far_clip_mm), int(max_steps), F32(tol_mm), stats)
    return out


# ---- the scene of the GPU tests (tests/test_sdf_scene_gpu.py; tests/test_sdf_scene.py asserts what it exercises) ----------------------
GEL_TOP, NEAR, FAR, TOL = 28.5, 24.0, 29.0, 1e-4
TILT, TURN = (0.9, 0.3, -0.2, 0.25), (0.8, -0.25, 0.5, 0.3)
HALF, CAPSULE, BALL = 0, 1, 2  # the volumes of `three_volumes`
NUM_ENVS = 7


def scene_pixmm(H, W):
    return 3.0 / min(H, W)  # the frame's shorter side spans 3 mm


def gpu_scene(H, W, K=8):
    """(part_ids (7, K) int32, part_ops (7, K) int32, part_pose (7, K, 16) float32): the first K of eight slots per env, in mm about
    the frame centre, on the volumes of `three_volumes` (half space 2x2x2 at 1 mm, capsule 5x9x17 at 0.25 mm with step_scale 0.5,
    unit ball 24^3 at 0.1 mm):
      0 a ball; a capsule cut out of it; the ball again beside it, blended; id -1; id P; op 7; a ball beyond the frame's right edge;
        a half space intersected (what lies nearer than 28.25 mm is cut away, inside its 3 mm cube)
      1 no union slot at all: a ball subtracted, a capsule intersected, ...
      2 a subtraction first; a capsule straddling the near clip; a ball; a small ball cut out with a blended rim
      3 a NaN pose; the tilted half space; a dimple; a blended capsule; the capsule again
      4 a ball beyond the far clip (taps, no hit); a smaller ball; intersected with a third, blended
      5 a ball beyond the frame; a subtracted ball in the frame (rays that meet only its box); nothing else
      6 the capsule at the near clip; a blended ball; an op of -1"""
    pix = scene_pixmm(H, W)
    c = np.array([0.5 * W * pix, 0.5 * H * pix])
    E, T, U = np.eye(3), quat_matrix(TILT), quat_matrix(TURN)
    at = lambda z, dx=0.0, dy=0.0: [c[0] + dx, c[1] + dy, z]  # noqa: E731
    none = (-1, UNION, scene_row(E, at(28.0)))
    cap_near = scene_row(E, at(NEAR + 0.9 * 0.35 * (16.0 * pix)), scale=16.0 * pix)  # (its radius is 0.35 * scale)
    nan = scene_row(T, at(GEL_TOP - 0.4 + 1.0))
    nan[4] = np.nan
    envs = [
        [(BALL, UNION, scene_row(T, at(29.1))), (CAPSULE, SUBTRACT, scene_row(E, at(28.2, 0.2))),
         (BALL, UNION, scene_row(U, at(29.0, 0.9, 0.3), blend_mm=0.3)), none, (3, UNION, scene_row(T, at(29.1))),
         (BALL, 7, scene_row(T, at(29.1))), (BALL, UNION, scene_row(T, at(29.1, W * pix + 2.0))),
         (HALF, INTERSECT, scene_row(E, at(28.25), scale=3.0))],
        [(BALL, SUBTRACT, scene_row(T, at(29.1))), (CAPSULE, INTERSECT, scene_row(E, at(28.6))), (BALL, SUBTRACT, scene_row(U, at(28.9, 0.4))),
         (HALF, INTERSECT, scene_row(T, at(28.3))), none, none, (CAPSULE, SUBTRACT, scene_row(U, at(28.7))), none],
        [(CAPSULE, SUBTRACT, scene_row(E, at(28.5))), (CAPSULE, UNION, cap_near), (BALL, UNION, scene_row(T, at(29.1, -0.5))),
         (BALL, SUBTRACT, scene_row(U, at(28.3, -0.5, 0.2), scale=0.5, blend_mm=0.2)), none, none, none, none],
        [(BALL, UNION, nan), (HALF, UNION, scene_row(T, at(28.3), scale=1.2, level_mm=0.1)),
         (BALL, SUBTRACT, scene_row(E, at(28.0, 0.2), scale=0.6)), (CAPSULE, UNION, scene_row(U, at(28.9, -0.6), blend_mm=0.25)),
         (CAPSULE, UNION, scene_row(E, at(29.0, 0.0, 0.5))), none, none, none],
        [(BALL, UNION, scene_row(U, at(FAR + 0.05 + 1.0))), (BALL, UNION, scene_row(T, at(29.2, 0.4), scale=0.8)),
         (BALL, INTERSECT, scene_row(E, at(29.2), scale=0.9, blend_mm=0.1)), none, none, none, none, none],
        [(BALL, UNION, scene_row(T, at(29.1, W * pix + 2.0))), (BALL, SUBTRACT, scene_row(T, at(29.1))), none, none, none, none, none, none],
        [(CAPSULE, UNION, cap_near), (BALL, UNION, scene_row(T, at(29.0, 0.5), blend_mm=0.4)), (BALL, -1, scene_row(T, at(29.0))), none, none,
         none, none, none]]
    ids = np.array([[s[0] for s in env[:K]] for env in envs], np.int32)
    ops = np.array([[s[1] for s in env[:K]] for env in envs], np.int32)
    pose = np.stack([np.stack([s[2] for s in env[:K]]) for env in envs]).astype(F32)
    return ids, ops, pose
