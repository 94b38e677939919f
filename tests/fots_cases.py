"""Constructed inputs for the FOTS marker kernels (tests/test_fots_kernels_gpu.py) and the NumPy halves of its checks.

Nothing here touches the GPU: the input builders, the two-rounding / single-rounding centre emulation and the partials
splitter are exercised on their own by tests/test_fots_cases.py.  A case is a marker grid plus a multi-step sequence of
(Z, mask, indent, theta) batches; the expected values come from oracle.fots_oracle.FOTSOracle.step_from_deformation.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from oracle.fots_oracle import FOTSOracle

F32 = np.float32
MM2PIX = 19.58
STATS_DTYPE = np.dtype([("zmax", "<f4"), ("count", "<i4"), ("sum_row", "<i4"), ("sum_col", "<i4")])  # FotsReduce, 16 bytes
THETA_MAX = 60 / 180.0 * math.pi


# ---- centres: int(t * mm2pix + half) ---------------------------------------------------------------------------------------
def centroid_mm(mean_px, half, mm2pix=MM2PIX):
    """FS:139-141 in float32: (mean - half) / mm2pix."""
    return (F32(mean_px) - F32(half)) / F32(mm2pix)


def centre_two_roundings(t, half, mm2pix=MM2PIX) -> int:
    """What NumPy float32 scalars give (MM:177-178,194-195): product rounded, sum rounded, int()."""
    return int(F32(F32(t) * F32(mm2pix)) + F32(half))


def centre_single_rounding(t, half, mm2pix=MM2PIX) -> int:
    """What a fused multiply-add gives: the exact product (two float32 factors multiply exactly in float64) plus half, rounded
    once (the float64 sum of a 48-bit product and a small half-integer is exact at these magnitudes)."""
    return int(F32(np.float64(F32(t)) * np.float64(F32(mm2pix)) + np.float64(F32(half))))


def flipping_centroids(n: int, mm2pix=MM2PIX):
    """Integer centroid coordinates in [0, n) whose centre a fused multiply-add truncates to the pixel before."""
    half = n / 2
    out = []
    for c in range(n):
        t = centroid_mm(c, half, mm2pix)
        a, b = centre_two_roundings(t, half, mm2pix), centre_single_rounding(t, half, mm2pix)
        if a != b:
            assert a == c and b == c - 1, (n, c, a, b)
            out.append(c)
    return out


# ---- masks ---------------------------------------------------------------------------------------------------------------
def rect_mask(H, W, row, col, half_rows, half_cols):
    """Rectangle symmetric about pixel (row, col): the centroid is exactly (row, col)."""
    assert 0 <= row - half_rows and row + half_rows < H and 0 <= col - half_cols and col + half_cols < W, (row, col, half_rows, half_cols)
    m = np.zeros((H, W), np.uint8)
    m[row - half_rows:row + half_rows + 1, col - half_cols:col + half_cols + 1] = 1
    return m


def block100_mask(H, W, row0, col0, frac_rows=0, frac_cols=0):
    """A 10 x 10 block with top-left pixel (row0, col0), one corner pixel moved right by `frac_cols` columns and another moved
    down by `frac_rows` rows: 100 pixels with centroid exactly (row0 + 4.5 + frac_rows / 100, col0 + 4.5 + frac_cols / 100)."""
    assert 0 <= frac_rows < 100 and 0 <= frac_cols < 100
    m = np.zeros((H, W), np.uint8)
    m[row0:row0 + 10, col0:col0 + 10] = 1
    if frac_cols:
        m[row0, col0 + 9] = 0
        m[row0, col0 + 9 + frac_cols] = 1
    if frac_rows:
        m[row0 + 9, col0] = 0
        m[row0 + 9 + frac_rows, col0] = 1
    assert m.sum() == 100
    return m


def block100_at(H, W, row0, col0, d_rows, d_cols):
    """block100_mask displaced by a (possibly negative, two-decimal) number of pixels per axis from (row0, col0)."""
    ir, ic = math.floor(d_rows), math.floor(d_cols)
    fr, fc = round((d_rows - ir) * 100), round((d_cols - ic) * 100)
    return block100_mask(H, W, row0 + ir, col0 + ic, fr, fc)


def smooth_gel(H, W, B, seed, scale=1.0, offset=0.0):
    """A deformed gel that differs at every pixel and per env (so a wrong pixel / env lookup changes a marker)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, H, W), F32)
    for e in range(B):
        a, b, c, d = rs.uniform(0.5, 2.0, 4)
        out[e] = (offset - scale * (a * np.sin(xx / (7.0 + b)) * np.cos(yy / (5.0 + c)) + d * 0.01 * (xx + yy) / (H + W))
                  + 0.001 * rs.rand(H, W)).astype(F32)
    return out


# ---- statistics ----------------------------------------------------------------------------------------------------------
def true_stats(Z, M) -> np.ndarray:
    """(B,) records (zmax, count, sum_row, sum_col) of NumPy on the frames themselves."""
    Z = np.asarray(Z, F32)
    M = np.asarray(M) != 0
    B = Z.shape[0]
    s = np.zeros(B, STATS_DTYPE)
    for e in range(B):
        r, c = np.nonzero(M[e])
        s[e] = (Z[e].max(), len(r), r.sum(dtype=np.int64), c.sum(dtype=np.int64))
    return s


def split_partials(stats: np.ndarray, per_env: int, seed: int) -> np.ndarray:
    """Spread each env's statistics over a random subset of `per_env` records (B, per_env); the remaining records are the
    identity (-inf, 0, 0, 0) - what a wave that saw no pixel writes.  The maximum sits in one random record, the other used
    records hold smaller values; the integer sums are cut at random points."""
    rs = np.random.RandomState(seed)
    B = len(stats)
    out = np.zeros((B, per_env), STATS_DTYPE)
    out["zmax"] = -np.inf
    for e in range(B):
        k = rs.randint(1, per_env + 1)
        slots = rs.permutation(per_env)[:k]
        z = stats["zmax"][e]
        zs = (z - np.abs(rs.rand(k)).astype(F32) * F32(3.0) - F32(1e-3)).astype(F32)
        zs[rs.randint(k)] = z
        out["zmax"][e, slots] = zs
        for f in ("count", "sum_row", "sum_col"):
            total = int(stats[f][e])
            cuts = np.sort(rs.randint(0, total + 1, k - 1)) if k > 1 else np.zeros(0, np.int64)
            parts = np.diff(np.concatenate(([0], cuts, [total])))
            out[f][e, slots] = parts
    return out


def combine_partials(p: np.ndarray) -> np.ndarray:
    s = np.zeros(p.shape[0], STATS_DTYPE)
    s["zmax"] = p["zmax"].max(1)
    for f in ("count", "sum_row", "sum_col"):
        s[f] = p[f].sum(1, dtype=np.int64)
    return s


def compact_inputs(Z, M, mx, my):
    """(B, n_markers) values of Z / mask at the marker pixels (markers outside the image: 0, never read)."""
    B, H, W = Z.shape
    inside = (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
    zp = np.zeros((B, len(mx)), F32)
    mp = np.zeros((B, len(mx)), np.uint8)
    zp[:, inside] = Z[:, my[inside], mx[inside]]
    mp[:, inside] = np.asarray(M, np.uint8)[:, my[inside], mx[inside]]
    return zp, mp


# ---- cases ---------------------------------------------------------------------------------------------------------------
def default_grid(W, H, ncol=11, nrow=9):
    """The reference's grid (MM:59-76) scaled with the resolution."""
    x0, y0 = 15 * W // 320, 26 * H // 240
    xi = np.linspace(x0, W - x0, ncol, dtype=int)
    yi = np.linspace(y0, H - y0, nrow, dtype=int)
    gx, gy = np.meshgrid(xi, yi)
    return gx.reshape(-1).astype(np.int32), gy.reshape(-1).astype(np.int32)


def mesh_grid(xs, ys):
    gx, gy = np.meshgrid(np.asarray(xs), np.asarray(ys))
    return gx.reshape(-1).astype(np.int32), gy.reshape(-1).astype(np.int32)


@dataclass
class Case:
    name: str
    H: int
    W: int
    ncol: int
    nrow: int
    mx: np.ndarray
    my: np.ndarray
    steps: list = field(default_factory=list)  # of (Z (B,H,W) f32, M (B,H,W) u8, indent (B,) f32, theta (B,) f32)
    info: dict = field(default_factory=dict)   # what the case's own "did it exercise its branch" assertions need

    @property
    def B(self):
        return self.steps[0][0].shape[0]


def make_oracle(case: Case) -> FOTSOracle:
    """FOTSOracle on the case's own marker grid (no Taxim oracle behind it: only step_from_deformation is used)."""
    fo = FOTSOracle(SimpleNamespace(W=case.W, H=case.H), case.B, num_markers_col=case.ncol, num_markers_row=case.nrow)
    fo.mm.init_x = case.mx.reshape(case.nrow, case.ncol).astype(np.int64)
    fo.mm.init_y = case.my.reshape(case.nrow, case.ncol).astype(np.int64)
    fo.marker_data = np.zeros((case.B, 2, case.ncol * case.nrow, 2), F32)
    fo.marker_data[:, 0] = fo.mm.init_marker_pos().astype(F32)
    return fo


def run_oracle(case: Case):
    """Per step: (marker_data (B,2,M,2) f32, marker_data64 (B,M,2), traj_state (B,8) f32, true statistics (B,))."""
    fo = make_oracle(case)
    out = []
    for Z, M, indent, theta in case.steps:
        md = fo.step_from_deformation(Z, M, indent, theta).copy()
        out.append((md, fo.marker_data64.copy(), fo.traj_state.copy(), true_stats(Z, M)))
    return out


def _stack(frames):
    return np.ascontiguousarray(np.stack(frames))


def case_integer_centroids(H, W) -> Case:
    """Case 1: rectangles symmetric about a pixel, two steps with theta 0 -> 0.3.  Envs: both steps on a flipping centroid;
    neither; only the first (the shear centre); only the last (the twist centre)."""
    rows, cols = flipping_centroids(H), flipping_centroids(W)
    s = W // 320
    hr, hc = 20 * s, 30 * s
    if (H, W) == (240, 320):
        flip = [(48, 62), (35, 56), (41, 49)]
    else:
        flip = [(r, c) for r in rows for c in cols if hr <= r < H - hr and hc <= c < W - hc][:40:13]
    assert len(flip) >= 3 and all(r in rows and c in cols for r, c in flip), (flip, rows, cols)
    calm = [(H // 2, W // 2), (H // 2 + 10 * s, W // 2 - 17 * s)]
    assert all(r not in rows and c not in cols for r, c in calm)
    seq = [(p, p) for p in flip] + [(p, p) for p in calm]
    seq += [(flip[0], calm[0]), (flip[1], calm[1])]   # only the first step's centroid flips: the shear centre
    seq += [(calm[0], flip[0]), (calm[1], flip[2])]   # only the last: the twist centre
    seq += [(flip[0], flip[1])]
    B = len(seq)
    mx, my = default_grid(W, H)
    c = Case(f"integer_centroids_{W}x{H}", H, W, 11, 9, mx, my)
    Z = smooth_gel(H, W, B, seed=11)
    for k in range(2):
        M = _stack([rect_mask(H, W, *seq[e][k], hr, hc) for e in range(B)])
        c.steps.append((Z * F32(1.0 + 0.1 * k), M, np.full(B, 0.5, F32), np.full(B, 0.3 * k, F32)))
    c.info = {"seq": seq, "flip": flip, "calm": calm}
    return c


SHEAR_PX = (-25, -10.4, -10, -3.7, -0.6, 0, 0.6, 9.99, 10, 25)


def case_shear_domain() -> Case:
    """Case 2: every pair (dy, dx) of SHEAR_PX as the centroid displacement of step 1, the reversed pairs at step 2."""
    H, W = 240, 320
    R0, C0 = 60, 100
    mx, my = mesh_grid(C0 - 28 + 8 * np.arange(16), R0 - 28 + 8 * np.arange(8))  # every 10 x 10 block in reach holds a marker
    pairs = [(dy, dx) for dy in SHEAR_PX for dx in SHEAR_PX]
    B = len(pairs)
    c = Case("shear_domain", H, W, 16, 8, mx, my)
    Z = smooth_gel(H, W, B, seed=22)
    ind, th = np.full(B, 1.0, F32), np.zeros(B, F32)
    c.steps.append((Z, _stack([block100_mask(H, W, R0, C0)] * B), ind, th))
    c.steps.append((Z, _stack([block100_at(H, W, R0, C0, dy, dx) for dy, dx in pairs]), ind, th))
    c.steps.append((Z, _stack([block100_at(H, W, R0, C0, dy, dx) for dy, dx in pairs[::-1]]), ind, th))
    c.info = {"pairs": pairs}
    return c


TWIST_RAD = (-2.0, -math.pi / 3 - 1e-3, -math.pi / 3, -0.4, 0.0, 0.4, math.pi / 3, math.pi / 3 + 1e-3, 2.0)


def case_twist_domain() -> Case:
    """Case 3: theta_last - theta_0 over TWIST_RAD, from three different theta_0."""
    H, W = 240, 320
    mx, my = default_grid(W, H)
    t0s = (0.0, -0.7, 1.3)
    combos = [(t0, d) for t0 in t0s for d in TWIST_RAD]
    B = len(combos)
    c = Case("twist_domain", H, W, 11, 9, mx, my)
    Z = smooth_gel(H, W, B, seed=33)
    m = np.zeros((H, W), np.uint8)
    m[70:151, 101:220] = 1   # centroid (110, 160): 25 markers inside
    m[70, 101] = 0           # ... nudged off the integer
    M = _stack([m] * B)
    ind = np.full(B, 0.8, F32)
    th0 = np.array([t0 for t0, _ in combos], F32)
    th1 = np.array([F32(t0) + F32(d) for t0, d in combos], F32)
    c.steps.append((Z, M, ind, th0))
    c.steps.append((Z, M, ind, th1))
    c.info = {"combos": combos}
    return c


def case_bookkeeping() -> Case:
    """Case 4: six steps; env 0 in contact throughout, 1 joins at step 2, 2 lifts off at step 2 and re-touches elsewhere from
    step 3, 3 never in contact, 4 pressed on a patch that holds no marker."""
    H, W = 240, 320
    mx, my = default_grid(W, H)
    B, steps = 5, 6
    c = Case("bookkeeping", H, W, 11, 9, mx, my)
    rs = np.random.RandomState(44)
    for k in range(steps):
        Z = smooth_gel(H, W, B, seed=440 + k)
        M = np.zeros((B, H, W), np.uint8)
        ind = np.zeros(B, F32)
        M[0] = rect_mask(H, W, 100 + 3 * k, 150 - 2 * k, 30, 40); ind[0] = 0.4 + 0.1 * k
        if k >= 2:
            M[1] = rect_mask(H, W, 60, 80 + 4 * k, 25, 25); M[1, 0, 0] = 1; ind[1] = 1.0
        if k < 2:
            M[2] = rect_mask(H, W, 160, 60 + 5 * k, 35, 35); ind[2] = 0.7
        elif k > 2:
            M[2] = rect_mask(H, W, 70 + k, 240 - k, 35, 35); M[2, 5, 7] = 1; ind[2] = 0.9
        M[3] = rect_mask(H, W, 120, 160, 30, 30) if k % 2 else 0   # a mask without indentation must be ignored
        M[4, 30 + k:34 + k, 20:24] = 1; ind[4] = 0.2               # between the markers at x = 15 / 44, y = 26 / 49
        c.steps.append((Z, M, ind, rs.uniform(-0.5, 0.5, B).astype(F32)))
    return c


def case_grid(name, H, W, ncol, nrow, mx=None, my=None, full_mask=False, seed=5) -> Case:
    """Case 5: three steps of a moving, turning rectangle (or the full frame) on a given marker grid."""
    if mx is None:
        mx, my = default_grid(W, H, ncol, nrow)
    c = Case(name, H, W, ncol, nrow, np.asarray(mx, np.int32), np.asarray(my, np.int32))
    B = 2
    for k in range(3):
        Z = smooth_gel(H, W, B, seed=seed * 10 + k)
        if full_mask:
            M = np.ones((B, H, W), np.uint8)
            if k:
                M[:, 3:3 + k, 5:5 + 3 * k] = 0  # the centroid moves a little (no marker of the grids used sits there)
        else:
            M = _stack([rect_mask(H, W, H // 2 + 2 * k, W // 2 - 4 * k, H // 3, W // 3),
                        rect_mask(H, W, H // 3 + k, W // 3 + 3 * k, H // 4, W // 4)])
            M[:, 1, 2] = 1
        c.steps.append((Z, M, np.array([0.5, 1.5], F32), np.array([0.1 * k, -0.25 * k], F32)))
    return c


def case_batch(B, seed=6) -> Case:
    """Case 6: B envs at 40 x 30 with every state mixed (in contact / not / no marker hit / clamped shear and twist), the
    largest zmax owned by the last env."""
    H, W = 30, 40
    mx, my = mesh_grid([5, 15, 25, 35], [5, 15, 25])
    c = Case(f"batch_{B}", H, W, 4, 3, mx, my)
    rs = np.random.RandomState(seed + B)
    kind = rs.randint(0, 5, B)  # 0 never in contact, 1 always, 2 lifts off at step 1, 3 no marker hit, 4 joins at step 1
    kind[B - 1] = 1
    base = smooth_gel(H, W, 1, seed=seed)[0]
    for k in range(3):
        Z = (base[None] * rs.uniform(0.5, 2.0, (B, 1, 1)) + rs.uniform(-1, 1, (B, 1, 1))).astype(F32)
        Z[B - 1] += F32(50.0)
        Z[B - 1, H - 1, W - 1] += F32(1.0)
        M = np.zeros((B, H, W), np.uint8)
        ind = np.zeros(B, F32)
        for e in range(B):
            kd = kind[e]
            if kd == 3:
                r, cc = rs.randint(7, 12), rs.randint(7, 13)
                M[e, r:r + 3, cc:cc + 2] = 1  # rows 7..13, cols 7..14: between the markers at 5 and 15
                ind[e] = 0.3
                continue
            r0, r1 = sorted(rs.randint(0, H, 2)); c0, c1 = sorted(rs.randint(0, W, 2))
            M[e, r0:r1 + 1, c0:c1 + 1] = 1
            M[e, rs.randint(H), rs.randint(W)] = 1
            on = kd == 1 or (kd == 2 and k != 1) or (kd == 4 and k >= 1)
            ind[e] = rs.uniform(0.1, 2.0) if on else 0.0
        c.steps.append((Z, M, ind, rs.uniform(-2.0, 2.0, B).astype(F32)))
    c.info = {"kind": kind}
    return c


STAT_SHAPES = ((240, 320), (480, 640), (30, 40), (50, 72))
STAT_MASKS = ("empty", "full", "first_pixel", "last_pixel", "one_row", "one_col", "random_1pct", "random_50pct")
STAT_GELS = ("random", "max_at_last_pixel", "all_negative")


def case_statistics(H, W) -> Case:
    """Case 7: one env per (mask, gel) pair, one step.  The empty mask goes with indent == 0 (in contact with no mask pixel the
    reference's centroid is NaN and its int() raises: that input has no expected value)."""
    mx, my = mesh_grid([0, W // 2, W - 1], [0, H // 2, H - 1])
    c = Case(f"statistics_{W}x{H}", H, W, 3, 3, mx, my)
    rs = np.random.RandomState(7 + H)
    frames, masks, ind, combos = [], [], [], []
    for mk in STAT_MASKS:
        for gk in STAT_GELS:
            m = np.zeros((H, W), np.uint8)
            if mk == "full": m[:] = 1
            elif mk == "first_pixel": m[0, 0] = 1
            elif mk == "last_pixel": m[H - 1, W - 1] = 1
            elif mk == "one_row": m[H - 2, :] = 1
            elif mk == "one_col": m[:, W - 1] = 1
            elif mk == "random_1pct": m[:] = rs.rand(H, W) < 0.01; m[H // 2, W // 3] = 1
            elif mk == "random_50pct": m[:] = rs.rand(H, W) < 0.5
            z = rs.randn(H, W).astype(F32)
            if gk == "max_at_last_pixel": z[H - 1, W - 1] = F32(9.25)
            elif gk == "all_negative": z = (-np.abs(z) - F32(0.125)).astype(F32)
            frames.append(z); masks.append(m); ind.append(0.0 if mk == "empty" else 0.6); combos.append((mk, gk))
    B = len(frames)
    c.steps.append((_stack(frames), _stack(masks), np.array(ind, F32), np.linspace(-1, 1, B).astype(F32)))
    c.info = {"combos": combos}
    return c
