"""NumPy restatement of the sensor lens model's contract (include/tacex_hip.h, `tacex_lens_model`, `tacex_lens_camera_model` and
`tacex_lens_points`): the per-pixel float32 arithmetic of the gather, every operation rounded on its own in the order the header
writes, and the float64 fixed-point inverse for points.  Written from that comment, not from the kernel: the tests compare the two
bit for bit (image) and to 1e-9 px (points)."""
import numpy as np
from camera_model_ref import IDENTITY_ROW as CAMERA_IDENTITY_ROW
from camera_model_ref import camera_frame

F = np.float32
IDENTITY_ROW = np.zeros(16, dtype=np.float32)
POINT_ITERATIONS = 24  # TACEX_LENS_POINT_ITERATIONS


def profile_row(k1=0.0, k2=0.0, p1=0.0, p2=0.0, rotation_deg=0.0, scale=1.0, shear=0.0, matrix=None, shift_px=(0.0, 0.0),
                centre_px=(0.0, 0.0), vignette=(0.0, 0.0), softness=(0.0, 0.0)):
    """[k1, k2, p1, p2, e00, e01, e10, e11, tx, ty, cx, cy, v1, v2, b0, b2] with E = A - I,
    A = scale * [[cos, -sin], [sin, cos]] @ [[1, shear], [0, 1]] formed in float64 (or `matrix`), rounded to float32 once."""
    if matrix is None:
        t = np.deg2rad(np.float64(rotation_deg))
        A = np.float64(scale) * (np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.array([[1.0, np.float64(shear)], [0.0, 1.0]]))
    else:
        A = np.asarray(matrix, dtype=np.float64).reshape(2, 2)
    E = A - np.eye(2)
    return np.array([k1, k2, p1, p2, E[0, 0], E[0, 1], E[1, 0], E[1, 1], shift_px[0], shift_px[1], centre_px[0], centre_px[1],
                     vignette[0], vignette[1], softness[0], softness[1]], dtype=np.float64).astype(np.float32)


def _clampf(x, lo, hi):
    """min(max(x, lo), hi) with C's fmaxf / fminf (a NaN operand gives the other one)"""
    return np.fmin(np.fmax(x, F(lo)), F(hi))


def source_positions(row, H, W):
    """(u, v, r2) float32 (H,W): the source position of every output pixel before the softness taps, and r2."""
    k1, k2, p1, p2, e00, e01, e10, e11, tx, ty, cx, cy = (F(v) for v in np.asarray(row, dtype=np.float32)[:12])
    s = F(2.0) / F(W)
    hw, hh = F(W) * F(0.5), F(H) * F(0.5)
    jf = np.broadcast_to(np.arange(W, dtype=np.float32)[None, :], (H, W))
    i_f = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W))
    px = ((jf + F(0.5)) - hw) - cx
    py = ((i_f + F(0.5)) - hh) - cy
    xn, yn = px * s, py * s
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    rad = (k1 + k2 * r2) * r2
    dx = (xn * rad + (p1 + p1) * xy) + p2 * (r2 + (xx + xx))
    dy = (yn * rad + p1 * (r2 + (yy + yy))) + (p2 + p2) * xy
    ou = ((e00 * px + e01 * py) + hw * dx) + tx
    ov = ((e10 * px + e11 * py) + hw * dy) + ty
    u, v = jf + ou, i_f + ov
    for a in (px, r2, dx, ou, u, v):
        assert a.dtype == np.float32
    return u, v, r2


def _tap(img, u, v):
    """bilinear tap of img (H,W,3) at float32 positions (u, v) (H',W'), edge replicate"""
    H, W, _ = img.shape
    with np.errstate(invalid="ignore"):
        u = np.where(np.abs(u) <= np.finfo(np.float32).max, u, F(0))
        v = np.where(np.abs(v) <= np.finfo(np.float32).max, v, F(0))
    x0f, y0f = np.floor(u), np.floor(v)
    fx, fy = (u - x0f)[..., None], (v - y0f)[..., None]
    x0 = _clampf(x0f, -1, W).astype(np.int64)
    y0 = _clampf(y0f, -1, H).astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    gx, gy = F(1) - fx, F(1) - fy
    out = (a * gx + b * fx) * gy + (c * gx + d * fx) * fy
    assert out.dtype == np.float32
    return out


def lens_frame(rgb, row):
    """One frame (H,W,3) float32 through the lens of profile row (16,) -> (H,W,3) float32."""
    img = np.ascontiguousarray(rgb, dtype=np.float32)
    H, W, _ = img.shape
    row = np.asarray(row, dtype=np.float32)
    v1, v2, b0, b2 = (F(x) for x in row[12:16])
    u, v, r2 = source_positions(row, H, W)
    if b0 == 0 and b2 == 0:
        col = _tap(img, u, v)
    else:
        hs = F(0.5) * _clampf(b0 + b2 * r2, 0, 4)
        um, up, vm, vp = u - hs, u + hs, v - hs, v + hs
        col = (((_tap(img, um, vm) + _tap(img, up, vm)) + _tap(img, um, vp)) + _tap(img, up, vp)) * F(0.25)
    g = _clampf(F(1) + (v1 + v2 * r2) * r2, 0, 1)
    out = g[..., None] * col
    assert out.dtype == np.float32
    return out


def lens_batch(rgb, profiles, ids):
    """rgb (B,H,W,3), profiles (P,16), ids (B,) or None -> (B,H,W,3); an id outside [0, P) is the identity profile."""
    profiles = np.asarray(profiles, dtype=np.float32).reshape(-1, 16)
    out = []
    for b in range(rgb.shape[0]):
        i = 0 if ids is None else int(ids[b])
        out.append(lens_frame(rgb[b], profiles[i] if 0 <= i < profiles.shape[0] else IDENTITY_ROW))
    return np.stack(out)


def lens_camera_batch(rgb, lens_profiles, lens_ids, camera_profiles, camera_ids, seed, call, u8, frame_offset=0):
    """The fused form: camera_frame(lens_frame(...)) per frame."""
    lens_profiles = np.asarray(lens_profiles, dtype=np.float32).reshape(-1, 16)
    camera_profiles = np.asarray(camera_profiles, dtype=np.float32).reshape(-1, 16)
    out = []
    for b in range(rgb.shape[0]):
        i = 0 if lens_ids is None else int(lens_ids[b])
        k = 0 if camera_ids is None else int(camera_ids[b])
        mid = lens_frame(rgb[b], lens_profiles[i] if 0 <= i < lens_profiles.shape[0] else IDENTITY_ROW)
        crow = camera_profiles[k] if 0 <= k < camera_profiles.shape[0] else CAMERA_IDENTITY_ROW
        out.append(camera_frame(mid, crow, seed, frame_offset + b, call, u8))
    return np.stack(out)


def displacement(row, x, y, H, W):
    """float64 (ou, ov) at real-valued output positions (x = column j, y = row i): source = (x, y) + (ou, ov)."""
    k1, k2, p1, p2, e00, e01, e10, e11, tx, ty, cx, cy = (np.float64(v) for v in np.asarray(row, dtype=np.float32)[:12])
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s = 2.0 / np.float64(W)
    hw, hh = np.float64(W) * 0.5, np.float64(H) * 0.5
    px = ((x + 0.5) - hw) - cx
    py = ((y + 0.5) - hh) - cy
    xn, yn = px * s, py * s
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    rad = (k1 + k2 * r2) * r2
    dx = (xn * rad + (p1 + p1) * xy) + p2 * (r2 + (xx + xx))
    dy = (yn * rad + p1 * (r2 + (yy + yy))) + (p2 + p2) * xy
    ou = ((e00 * px + e01 * py) + hw * dx) + tx
    ov = ((e10 * px + e11 * py) + hw * dy) + ty
    return ou, ov


def lens_points(xy, row, H, W, iterations=POINT_ITERATIONS):
    """xy (...,2) float64 ideal image pixels (x = column, y = row) -> where the lens shows them: q with q + displacement(q) = xy,
    by `iterations` rounds of q <- xy - displacement(q) from q = xy."""
    xy = np.asarray(xy, dtype=np.float64)
    x, y = xy[..., 0], xy[..., 1]
    qx, qy = x.copy(), y.copy()
    for _ in range(iterations):
        ou, ov = displacement(row, qx, qy, H, W)
        qx, qy = x - ou, y - ov
    return np.stack([qx, qy], -1)


def profile_set(W):
    """The six profiles of the test set, as keyword arguments of `profile_row` / `LensProfile`, for a frame W columns wide."""
    return [dict(),                                                                                  # 1 identity
            dict(shift_px=(3.0, -2.0)),                                                              # 2 pure integer shift
            dict(k1=-0.15, k2=0.03, rotation_deg=1.5, scale=1.02),                                   # 3 radial + rotation + scale
            dict(p1=0.01, p2=-0.008, centre_px=(4.5, -3.25), vignette=(-0.25, -0.05)),               # 4 tangential, centre, vignette
            dict(k1=0.08, k2=-0.01, p1=0.004, shift_px=(0.4, 0.7), softness=(0.5, 1.5)),             # 5 softness with distortion
            dict(shift_px=(2.0 * W, 0.0))]                                                           # 6 every tap clamped to an edge
