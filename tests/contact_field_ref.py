"""NumPy restatement of `tacex_contact_field`, written from the function's comment in include/tacex_hip.h: per-pixel terms in
float32 with every operation rounded on its own, sums in float64.  Also the analytic inputs of the closed-form tests."""
import numpy as np

f32 = np.float32


def gel_row(k_n, k_t=0.0, mu=0.0):
    return np.array([k_n, k_t, mu, 0.0], dtype=f32)


def pixel_area(pixmm):
    return f32(np.float64(f32(pixmm)) ** 2 * 1e-6)


def contact_pixels(hm, frame_min, indent, gel, slip, pixmm):
    """One frame: hm (H,W) f32 -> dict of (H,W) arrays d, p, tx, ty (f32), slips (bool), fx, fy, fn (f32)."""
    hm = np.asarray(hm, dtype=f32)
    H, W = hm.shape
    pixmm = f32(pixmm)
    kn, kt, mu = (f32(v) for v in gel[:3])
    dx, dy, dth, cx, cy = (f32(v) for v in (slip if slip is not None else np.zeros(5)))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        S = (hm - f32(frame_min)) - f32(indent)
        d = np.where(S < 0, -S, f32(0)).astype(f32)
        p = (kn * d).astype(f32)
        jj, ii = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
        rx = ((jj - cx) * pixmm).astype(f32)
        ry = ((ii - cy) * pixmm).astype(f32)
        ux = (dx - (dth * ry).astype(f32)).astype(f32)
        uy = (dy + (dth * rx).astype(f32)).astype(f32)
        n = np.sqrt(((ux * ux).astype(f32) + (uy * uy).astype(f32)).astype(f32)).astype(f32)
        stick = (kt * n).astype(f32)
        cone = (mu * p).astype(f32)
        on = d > 0
        slips = on & (stick >= cone)
        s = (np.minimum(stick, cone) / n).astype(f32)
        shear = on & (n != 0)
        tx = np.where(shear, (ux * s).astype(f32), f32(0)).astype(f32)
        ty = np.where(shear, (uy * s).astype(f32), f32(0)).astype(f32)
    a = pixel_area(pixmm)
    z = f32(0)
    return dict(d=d, p=p, tx=tx, ty=ty, slips=slips, on=on, stick=stick, cone=cone,
                fx=np.where(on, (tx * a).astype(f32), z), fy=np.where(on, (ty * a).astype(f32), z), fn=np.where(on, (p * a).astype(f32), z))


def contact_frame(hm, frame_min, indent, gel, slip, pixmm, grid=(1, 1)):
    """One frame -> (record (16,) f64, cells (rows,cols,3) f64 - round to float32 to compare -, image (H,W,3) f32,
    abs (16,) f64: the sum of |terms| behind every record slot that is a plain sum, for tolerances)."""
    px = contact_pixels(hm, frame_min, indent, gel, slip, pixmm)
    H, W = px["d"].shape
    rows, cols = grid
    on = px["on"]
    fx, fy, fn, p, d = (px[k].astype(np.float64) for k in ("fx", "fy", "fn", "p", "d"))
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cx0, cy0 = (W - 1) / 2.0, (H - 1) / 2.0
    mm = np.float64(f32(pixmm))
    m = mm * 1e-3
    rec, ab = np.zeros(16), np.zeros(16)
    sfx, sfy, sfn = fx.sum(), fy.sum(), fn.sum()
    rec[0], rec[1], rec[2] = sfx, sfy, -sfn
    rec[3] = -((fn * ii).sum() - cy0 * sfn) * m
    rec[4] = ((fn * jj).sum() - cx0 * sfn) * m
    rec[5] = (((fy * jj).sum() - cx0 * sfy) - ((fx * ii).sum() - cy0 * sfx)) * m
    rec[6] = sfn
    cnt = float(on.sum())
    rec[7] = cnt * np.float64(pixel_area(pixmm))
    rec[8] = cnt
    rec[11] = float(px["d"].max()) if cnt else 0.0
    rec[12] = d.sum() * (mm * mm)
    rec[13] = float(px["slips"].sum())
    sp = p.sum()
    x, y, ang, asp = cx0, cy0, 0.0, 0.0
    if sp > 0:
        x, y = (p * jj).sum() / sp, (p * ii).sum() / sp
        m20 = (p * jj * jj).sum() / sp - x * x
        m02 = (p * ii * ii).sum() / sp - y * y
        m11 = (p * jj * ii).sum() / sp - x * y
        ang = 0.5 * np.arctan2(2.0 * m11, m20 - m02)
        mean, half = 0.5 * (m20 + m02), 0.5 * (m20 - m02)
        rad = np.sqrt(half * half + m11 * m11)
        lmax, lmin = mean + rad, mean - rad
        if lmax > 0:
            asp = np.sqrt(max(lmin, 0.0) / lmax)
        ab[14] = lmax - lmin  # (for the comparison of slot 14: meaningful only where the axes differ)
    rec[9], rec[10], rec[14], rec[15] = x, y, ang, asp
    ab[0], ab[1], ab[2], ab[6] = np.abs(fx).sum(), np.abs(fy).sum(), sfn, sfn
    ab[3] = ((fn * ii).sum() + cy0 * sfn) * m
    ab[4] = ((fn * jj).sum() + cx0 * sfn) * m
    ab[5] = ((np.abs(fy) * jj).sum() + cx0 * np.abs(fy).sum() + (np.abs(fx) * ii).sum() + cy0 * np.abs(fx).sum()) * m
    ab[12] = rec[12]
    ci = (np.arange(H) * rows) // H
    cj = (np.arange(W) * cols) // W
    cells = np.zeros((rows, cols, 3))
    for c, v in enumerate((fx, fy, -fn)):
        np.add.at(cells[:, :, c], (ci[:, None], cj[None, :]), v)
    image = np.stack([px["tx"], px["ty"], np.where(on, -px["p"], f32(0))], axis=-1).astype(f32)
    return rec, cells, image, ab


def contact_batch(hm, frame_min, indent, gels, gel_ids, slip, pixmm, grid=(1, 1)):
    """(B,H,W) -> record (B,16), cells (B,rows,cols,3) f64, image (B,H,W,3) f32, abs (B,16).  An id outside the table: zeros."""
    B, H, W = hm.shape
    rec, ab = np.zeros((B, 16)), np.zeros((B, 16))
    cells = np.zeros((B, grid[0], grid[1], 3))
    image = np.zeros((B, H, W, 3), dtype=f32)
    for b in range(B):
        g = 0 if gel_ids is None else int(gel_ids[b])
        if 0 <= g < len(gels):
            rec[b], cells[b], image[b], ab[b] = contact_frame(hm[b], frame_min[b], indent[b], gels[g], None if slip is None else slip[b], pixmm, grid)
    return rec, cells, image, ab


def borderline_pixels(hm, frame_min, indent, gel, slip, pixmm, rel=1e-5):
    """Number of contact pixels whose stick / slip decision is within `rel` of the cone."""
    px = contact_pixels(hm, frame_min, indent, gel, slip, pixmm)
    st, co = px["stick"].astype(np.float64), px["cone"].astype(np.float64)
    return int((px["on"] & (np.abs(st - co) < rel * np.maximum(np.abs(st), np.abs(co)))).sum()), int(px["on"].sum())


# ---- analytic height maps (mm): an indenter pressed `press` mm below the gel's rest plane at height 0; background at 0 ----------
def sphere_map(H, W, R, press, cx, cy, pixmm, dtype=np.float64):
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    r2 = (jj - cx) ** 2 + (ii - cy) ** 2
    prof = (R - np.sqrt(np.maximum(R * R - r2, 0.0))) * pixmm
    return np.where(r2 <= R * R, np.minimum(prof - press, 0.0), 0.0).astype(dtype)


def cylinder_map(H, W, R, press, cx, cy, angle, half_len, pixmm, dtype=np.float64):
    """A cylinder of radius R px lying in the image plane, axis along `angle` (against the x axis), 2 half_len px long."""
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dx, dy = jj - cx, ii - cy
    along = dx * np.cos(angle) + dy * np.sin(angle)
    across = -dx * np.sin(angle) + dy * np.cos(angle)
    prof = (R - np.sqrt(np.maximum(R * R - across ** 2, 0.0))) * pixmm
    return np.where((np.abs(across) <= R) & (np.abs(along) <= half_len), np.minimum(prof - press, 0.0), 0.0).astype(dtype)


def frame_scalars(hm):
    """(frame_min, indent) such that S = (hm - frame_min) - indent is < 0 exactly below the rest plane 0: frame_min = min(hm),
    indent = -min(hm) (the press depth), as the sensor's depth pass gives for a pad whose rest plane is the far clip."""
    mn = f32(np.asarray(hm, dtype=f32).min())
    return mn, f32(-mn)


# ---- the input frames of the GPU tests (built on the CPU, so that a CPU test can vet them) -----------------------------------------
GEL_TOP_MM, FAR_CLIP_MM = 28.5, 29.0
GELS = np.stack([gel_row(3.0e4, 1.2e4, 0.6), gel_row(8.0e4, 5.0e4, 0.35), gel_row(1.5e4, 0.0, 0.9)])
FRAME_KINDS = ("sphere", "cylinder", "edge", "two_spheres", "none", "full", "clip_left", "clip_right", "clip_top", "clip_bottom")


def case_pixmm(H):
    return 0.0295 * 240.0 / H


def case_frame(kind, H, W, seed=0):
    """(H,W) f32 height map [mm] in the sensor's convention (camera depth: gel top at 28.5 mm, background at the 29 mm far clip)."""
    from tacex_amd.utils.synthetic import dense_contact_depth_maps, synthetic_depth_maps

    if kind in ("sphere", "cylinder", "edge", "two_spheres"):
        return synthetic_depth_maps(1, H, W, seed=seed + 11, flat_fraction=0.0, kinds=(kind,))[0][0].numpy()
    if kind == "none":
        return np.full((H, W), FAR_CLIP_MM, dtype=f32)
    if kind == "full":  # a wavy plate below the press plane over the whole image
        return dense_contact_depth_maps(1, H, W, seed=seed + 5)[0][0].numpy()
    cx, cy = {"clip_left": (1.5, 0.45 * H), "clip_right": (W - 2.25, 0.55 * H), "clip_top": (0.4 * W, 0.75), "clip_bottom": (0.6 * W, H - 1.5)}[kind]
    R, press = 0.3 * H, 0.9
    depth = GEL_TOP_MM + sphere_map(H, W, R, press + 1.0, cx, cy, case_pixmm(H)) + 1.0  # the cap's lowest point `press` below the gel top
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    depth = np.where((jj - cx) ** 2 + (ii - cy) ** 2 <= R * R, depth, FAR_CLIP_MM)
    return np.minimum(depth, FAR_CLIP_MM).astype(f32)


def case_batch(H, W, B, start=0):
    kinds = [FRAME_KINDS[(start + k) % len(FRAME_KINDS)] for k in range(B)]
    return np.stack([case_frame(k, H, W, seed=start + n) for n, k in enumerate(kinds)]), kinds


def case_slip(B, H, W, start=0):
    """Slip rows cycling through translation, twist, both and none, about a point near the image centre."""
    rows = [(0.03, -0.02, 0.0), (0.0, 0.0, 0.05), (-0.015, 0.04, -0.08), (0.0, 0.0, 0.0)]
    return np.array([[*rows[(start + b) % 4], 0.5 * W + 0.7 * b - 1.3, 0.5 * H - 0.9 * b + 0.6] for b in range(B)], dtype=f32)


def indentation_depth(hm, gelpad_height=0.0045, min_distance=0.024):
    """(frame_min, indent) of TS:115-131 in float32 (the library's tacex_indentation_depth; for vetting cases on the CPU)."""
    fmin = hm.reshape(hm.shape[0], -1).min(axis=1).astype(f32)
    d = np.maximum((fmin / f32(1000.0)).astype(f32) - f32(min_distance), f32(0))
    ind = np.where(d <= f32(gelpad_height), ((f32(gelpad_height) - d) * f32(1000.0)).astype(f32), f32(0)).astype(f32)
    return fmin, ind
