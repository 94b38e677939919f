"""Inputs that pin the Taxim shading bin by bin (tests/test_taxim_bin_cases.py on the CPU, tests/test_taxim_bins_gpu.py on the GPU).

Nothing here touches the GPU.  The shading step turns a gradient into (magnitude bin, direction bin) and reads one of nb x nb
polynomial records; three kinds of input reach every record, every bin edge and every wave-uniform shortcut of the streaming tail:

LATTICE (straight into `Taxim.shade`).  The frame is tiled by 3 x 3 cells.  The centre (1, 1) of a cell has four private
neighbours, so its gradient is set on its own: the top neighbour holds dzdx / gsy, the left one dzdy / gsx (the kernel's scales,
`grad_scales`), the other two stay 0.  With "all else 0" the four pixels that see ONE of those two values have an axis-aligned
gradient, which lies exactly on a direction-bin edge (124 % 4 == 0): 4 of every 9 pixels would be left out by the margin rule.
The cell's corner (2, 2) - no neighbour of any centre - therefore holds a filler CORNER * t / gsx: each of those pixels then sees a
second component, its direction is generic, and the share the rule leaves out stays under the cap the GPU test asserts (2 %; the CPU
test measures it with both oracles).  The last lattice column is moved to W - 2, so that the replicate padding of the gradient maps
(rows 0 / H-1, columns 0 / W-1) carries the bins of a centre on all four sides.

FACETS (through `render_direct` / `deform`).  A tilted plane with the whole frame in contact is restored at every pyramid level, so
only the final blur touches it: every interior pixel (frame minus final-blur radius + 1) carries the plane's gradient.

COMPOSITES.  A facet on the right half of a flat in-contact plane ("half"), and a 4-column facet strip in a flat plane ("strip", once
at a 4-column lane-group boundary and once at the seam column of `taxim_route_cases.seams`): one facet lane group in a wave that is
flat everywhere else, which is what the wave-uniform shortcuts of the streaming tail branch on.

ROWS (`row_threshold_frames`).  A frame in contact everywhere never TAKES the streaming tail's magnitude shortcut (see there), so the
facets cannot show a shifted threshold; a dent in an otherwise untouched gel, scaled until the steepest pixel of one row lies 4 tau_mag
beside the first magnitude-bin edge, does.  These frames are shaded with a marked table (`marked_calib_folder`), in which no two
neighbouring records are alike.

THE MARGIN RULE (`margins`).  The kernels evaluate in float32 what the float64 oracle evaluates exactly; a pixel is compared where
the oracle's grad_mag / grad_dir lie farther from the nearest bin edge than
    tau_mag = dt / (1 + t^2) + 1e-6 rad,   tau_dir = dt / t + 2e-6 rad,   dt = 8 ulp32(max |Z| of the frame) max(gsy, gsx).
dt is the gradient's error from heights rounded to float32; the constants are float32 evaluation error, not measurements: ulp32(2 pi)
= 4.8e-7 enters twice (the sum with pi, the product with 1 / y_binr), and the reference's own float32 atan / atan2 are good to about
1 ulp (1.2e-7 at pi / 2).  The lower edge of magnitude bin 0 is no edge.  Pixels with t == 0 in the oracle are compared, their record
is (0, 62); pixels with 0 < t^2 < 1e-30 are not compared with the oracle (the kernels flush t^2 < FLT_MIN to the flat record, the
reference computes a direction from a denormal).

EDGE OFFSETS.  The edge families put every record EDGE_OFFSET = 1e-4 of a bin width inside an edge (1.3e-6 rad in magnitude, 5.1e-6
rad in direction).  dt belongs to the FRAME: a centre that shares its frame with steeper ones has a tau above that offset (at 96 x 128
a frame holds eleven magnitude bins; in the first one tau_dir of bin 0 is 1.8e-5 rad beside bin 10, and 1e-6 + dt / 2 alone exceeds
1.3e-6 rad around t = 1).  Such a centre (EDGE_OFFSET below 1.1 tau) is placed 2 tau inside the edge, tau from the rule above with the frame's
own heights (`family`) - derived, never fitted to a kernel; the widest offsets are printed by the CPU test.  Two edges are no edges:
the lower edge of magnitude bin 0 (mag_lo puts bin 0 at a tenth of its width, where the direction is still well-conditioned) and the
upper edge of magnitude bin 123, which is t = infinity (mag_hi stops at t = T_MAX = 1e3, 1e-3 rad below it: a steeper centre would
raise the dt of its whole frame above the other centres' bins).
"""
from __future__ import annotations

import math

import numpy as np

import taxim_route_cases as rc

F32 = np.float32
NB = 125
NREC = NB - 1                      # two-sided bins per axis: bin 124 is t = infinity / dir = +pi
X_BINR = 0.5 * math.pi / (NB - 1)
Y_BINR = 2.0 * math.pi / (NB - 1)
EDGE_OFFSET = 1e-4                 # of a bin width
T_MAX = 1e3                        # steepest lattice centre of the mag_hi family
CORNER = 0.37                      # filler of a cell's corner, as a gradient component relative to the cell's t
FLAT = (0, 62)                     # the record of a zero gradient
TINY_T2 = 1e-30                    # below it (and above 0) the oracle is no reference
LATTICE_SHAPE, LATTICE_FRAMES = (96, 128), 12
FAMILIES = ("centres", "mag_lo", "mag_hi", "dir_lo", "dir_hi")


def grad_scales(params, shape):
    """(gsy, gsx) = 0.5 H / calib_h / pixmm, 0.5 W / calib_w / pixmm: gradient per mm of height difference across two pixels."""
    H, W = shape
    return 0.5 * H / params.calib_h / params.pixmm, 0.5 * W / params.calib_w / params.pixmm


def gradient_of(mag, dr):
    """(dzdx, dzdy) with atan(|.|) = mag and atan2(dzdx, dzdy) = dr."""
    t = np.tan(np.asarray(mag, np.float64))
    return t * np.sin(dr), t * np.cos(dr)


def bin_point(im, idd, fm=0.5, fd=0.5):
    """grad_mag / grad_dir at the fractions (fm, fd) of the bins (im, idd)."""
    return (np.asarray(im) + fm) * X_BINR, (np.asarray(idd) + fd) * Y_BINR - math.pi


# ---- lattice -------------------------------------------------------------------------------------------------------------------
def lattice_sites(shape):
    """Rows and columns of the centres: 1, 4, 7, ...; the last column is W - 2 (its cell is up to two columns wider)."""
    def axis(n):
        c = np.arange(1, n - 1, 3)
        return c if c[-1] == n - 2 else np.append(c[n - 2 - c >= 3], n - 2)

    return axis(shape[0]), axis(shape[1])


def lattice_from_gradients(shape, dzdx, dzdy, gs, corner=CORNER):
    """float32 Z (frames, H, W) and the (frame, y, x) of every centre, centre i carrying the gradient (dzdx[i], dzdy[i]); signed zeros
    are kept.  Frames are filled in order; the unused cells of the last one stay flat."""
    H, W = shape
    gsy, gsx = gs
    rows, cols = lattice_sites(shape)
    dzdx, dzdy = np.asarray(dzdx, np.float64), np.asarray(dzdy, np.float64)
    n, per = len(dzdx), len(rows) * len(cols)
    k = np.arange(n)
    f, r = k // per, k % per
    y, x = rows[r // len(cols)], cols[r % len(cols)]
    Z = np.zeros((int(f.max()) + 1, H, W), F32)
    Z[f, y - 1, x] = (dzdx / gsy).astype(F32)
    Z[f, y, x - 1] = (dzdy / gsx).astype(F32)
    regular = (y % 3 == 1) & (x % 3 == 1)  # the moved last column / row has no corner of its own
    Z[f[regular], y[regular] + 1, x[regular] + 1] = (corner * np.hypot(dzdx, dzdy) / gsx).astype(F32)[regular]
    return Z, np.stack([f, y, x], 1)


def lattice_frames(shape, mags, dirs, gs):
    """The lattice for centres of given grad_mag / grad_dir (rad)."""
    return lattice_from_gradients(shape, *gradient_of(mags, dirs), gs)


def ulp32(v):
    return np.spacing(np.asarray(v, F32)).astype(np.float64)


def tau(zmax, t, gs):
    """(tau_mag, tau_dir) of the margin rule for gradients of size t in a frame whose heights reach zmax."""
    dt = 8.0 * ulp32(zmax) * max(gs)
    with np.errstate(divide="ignore"):
        return dt / (1.0 + t * t) + 1e-6, dt / t + 2e-6


def records():
    """Every two-sided record (im, idd), magnitude-major: the steep ones share the last frames."""
    im, idd = np.divmod(np.arange(NREC * NREC), NREC)
    return im, idd


def family(name, shape, gs):
    """One lattice family: dict Z, sites (n, 3), im, idd (the intended records), mag, dir, off_mag, off_dir (offsets from the edge in
    bin widths, where the family has one)."""
    assert name in FAMILIES
    im, idd = records()
    rows, cols = lattice_sites(shape)
    frame = np.arange(len(im)) // (len(rows) * len(cols))
    off_m = np.full(len(im), EDGE_OFFSET)
    off_d = np.full(len(im), EDGE_OFFSET)
    for _ in range(4):  # the offsets follow tau, tau follows the frame's heights, which follow the offsets: settles at once
        fm = {"mag_lo": np.where(im == 0, 0.1, off_m), "mag_hi": 1.0 - off_m}.get(name, 0.5)
        fd = {"dir_lo": off_d, "dir_hi": 1.0 - off_d}.get(name, 0.5)
        mag, dr = bin_point(im, idd, fm, fd)
        mag = np.minimum(mag, math.atan(T_MAX))
        gx, gy = gradient_of(mag, dr)
        t = np.hypot(gx, gy)
        zabs = np.maximum(np.abs(gx) / gs[0], np.abs(gy) / gs[1])
        zmax = np.array([zabs[frame == f].max() for f in range(frame.max() + 1)])[frame]
        tm, td = tau(zmax, t, gs)
        # (1.1 tau: rounding the heights to float32 moves a centre by up to 3e-8 rad in magnitude, 6e-8 rad in direction)
        off_m = np.where(EDGE_OFFSET * X_BINR > 1.1 * tm, EDGE_OFFSET, 2.0 * tm / X_BINR)
        off_d = np.where(EDGE_OFFSET * Y_BINR > 1.1 * td, EDGE_OFFSET, 2.0 * td / Y_BINR)
    Z, sites = lattice_from_gradients(shape, gx, gy, gs)
    return {"Z": Z, "sites": sites, "im": im, "idd": idd, "mag": mag, "dir": dr, "off_mag": off_m, "off_dir": off_d}


def t_unit(gs_axis, ref_scale):
    """float32 heights (above, below) of a pixel whose gradient is 1 exactly in the kernel's arithmetic, float32((above - below) gs),
    AND in the reference's, (below / pixmm - above / pixmm) / 2 * N / calib_n negated (`ref_scale` = (pixmm, N, calib_n)) - or None.
    No single height does that with the shipped calibration (0.295 mm gives 1 and 1 - 6e-8): the pair is searched for."""
    pixmm, n, calib_n = ref_scale
    d = F32(1.0 / gs_axis)
    for j in range(1, 1 << 14):
        below = F32(j) * F32(2.0 ** -12)
        above = F32(below + d)
        kern = F32(F32(above - below) * F32(gs_axis))
        ref = F32(F32(F32(above / F32(pixmm)) - F32(below / F32(pixmm))) / F32(2.0)) * F32(n) / F32(calib_n)
        if kern == F32(1) and ref == F32(1):
            return float(above), float(below)
    return None


def special_points(params, shape):
    """(names, dzdx, dzdy) of the special family.  An axis-aligned direction lies exactly on a bin edge (dir = 0 -> 62.0, +-pi/2 ->
    93.0 / 31.0, +pi -> 124, -pi from a -0.0 row gradient -> 0), t = 1 on the magnitude edge 62.0 ("t 1" is a placeholder here:
    special_frames sets it from the pair of heights of `t_unit`)."""
    pts = [("dir 0", 0.0, 0.5), ("dir +pi/2", 0.5, 0.0), ("dir -pi/2", -0.5, 0.0), ("dir +pi", 0.0, -0.5), ("dir -pi", -0.0, -0.5),
           ("t 1", 1.0, 0.0), ("zero", 0.0, 0.0), ("tiny", 1e-20, 1e-20), ("tiny -", -1e-20, 1e-20)]
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            q = f"{'+' if sx > 0 else '-'}{'+' if sy > 0 else '-'}"
            pts += [("diag " + q, 0.3 * sx, 0.3 * sy), ("1e-12 " + q, 1e-12 * sx, 1e-12 * sy), ("1e3 " + q, 1e3 * sx, 1e3 * sy)]
    names, gx, gy = zip(*pts)
    return list(names), np.array(gx), np.array(gy)


def special_frames(params, shape):
    """The special family, ONE POINT PER FRAME (their sizes span 23 decades; sharing a frame would not matter to the float32
    restatement they are held to, but keeps every frame's neighbours readable): names, Z (n, H, W), sites (n, 3).  Each point sits on
    the lattice's first centre (1, 1) AND on its last (H - 2, W - 2), so all four borders replicate it."""
    names, gx, gy = special_points(params, shape)
    gs = grad_scales(params, shape)
    H, W = shape
    rows, cols = lattice_sites(shape)
    per = len(rows) * len(cols)
    Zs, sites = [], []
    for i in range(len(names)):
        ax, ay = np.zeros(per), np.zeros(per)
        ax[[0, per - 1]], ay[[0, per - 1]] = gx[i], gy[i]
        z, s = lattice_from_gradients(shape, ax, ay, gs, corner=0.0)
        if names[i] == "t 1":
            pair = t_unit(gs[0], (params.pixmm, H, params.calib_h))
            assert pair is not None, "no pair of float32 heights gives t = 1 on both float32 paths"
            for y, x in ((1, 1), (H - 2, W - 2)):
                z[0, y - 1, x], z[0, y + 1, x] = pair
        Zs.append(z[0])
        sites += [(i, 1, 1), (i, H - 2, W - 2)]
    return names, np.stack(Zs), np.array(sites)


# ---- facets and composites -------------------------------------------------------------------------------------------------------
def _press(hm, contact_scale):
    span = hm.max(axis=(-2, -1)).astype(np.float64) - hm.min(axis=(-2, -1))
    return (1.05 * span / (1.0 - contact_scale) + 1.0).astype(F32)


def _plane(shape, mag, dr, gs, y0, x0):
    """Heights whose deformed gel (= height - constant, all in contact) has the gradient of (mag, dr) around (y0, x0)."""
    H, W = shape
    gx, gy = gradient_of(mag, dr)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return -gx / (2.0 * gs[0]) * (yy - y0) - gy / (2.0 * gs[1]) * (xx - x0)  # dzdx = (Z[y-1] - Z[y+1]) gsy, dzdy likewise


def facet_frames(case, mags, dirs, gs, contact_scale=0.4):
    """(hm (n, H, W) float32 mm, press (n,) float32): one tilted plane per (mag, dir), the whole frame in contact."""
    H, W = case.shape
    hm = np.stack([_plane(case.shape, m, d, gs, 0.5 * (H - 1), 0.5 * (W - 1)) for m, d in zip(mags, dirs)]).astype(F32)
    return hm, _press(hm, contact_scale)


def strip_columns(case):
    """First column of the 4-column strips: one at a lane-group boundary away from every seam, one at the seam column."""
    xs = rc.seams(*case.shape)[1]
    return (xs // 2) & ~3, xs


def composite_frames(case, mags, dirs, kind, gs, contact_scale=0.4):
    """(hm, press, facet) - facet (n, H, W) bool marks the facet's columns.  kind "half": the facet is the right half of a flat
    in-contact plane; "strip": four columns of it, two frames per target (strip_columns)."""
    H, W = case.shape
    hms, facet = [], []
    for m, d in zip(mags, dirs):
        for x0, x1 in ([(W // 2, W)] if kind == "half" else [(c, c + 4) for c in strip_columns(case)]):
            hm = np.zeros((H, W))
            hm[:, x0:x1] = _plane(case.shape, m, d, gs, 0.5 * (H - 1), x0)[:, x0:x1]
            f = np.zeros((H, W), bool)
            f[:, x0:x1] = True
            hms.append(hm)
            facet.append(f)
    hm = np.stack(hms).astype(F32)
    return hm, _press(hm, contact_scale), np.stack(facet)


def interior(case):
    """Frame minus a border of final-blur radius + 1: where only the plane itself enters a facet pixel's gradient."""
    b = (case.ksize[-1] - 1) // 2 + 1
    m = np.zeros(case.shape, bool)
    m[b:case.H - b, b:case.W - b] = True
    return m


def facet_targets():
    """(im, idd) of the facet set: every magnitude bin 0..123 with direction bin (37 im + 5) % 124, then all 124 direction bins at
    magnitude bin 0 (the streaming tail's LDS records) and at magnitude bin 1 (the first gathered record): 372 frames."""
    k = np.arange(NREC)
    return np.concatenate([k, 0 * k, 0 * k + 1]), np.concatenate([(37 * k + 5) % NREC, k, k])


COMPOSITE_MAGS = (0, 1, 5, 40, 90, 118)
COMPOSITE_DIRS = (38, 58, 100)  # one direction bin per third of the circle, none axis-aligned, each with a bin-0 record that differs from bin 1's


def composite_targets():
    im, idd = np.meshgrid(COMPOSITE_MAGS, COMPOSITE_DIRS, indexing="ij")
    return im.ravel(), idd.ravel()


def marked_calib_folder(case, calib_dir, tmp_dir):
    """rc.calib_folder with a MARKED table: every record's constant term is moved by 0.004 * ((3 im + 5 idd) % 16 - 8) in RGB units
    (at most 0.032: nothing reaches the clip), so that two neighbouring records differ by 0.012 or more at every pixel - 100 times the
    RGB tolerance.  The shipped table holds identical records in neighbouring bins for many directions (record_gap): a wrong bin there
    changes nothing, and the streaming tail shows its bins through the RGB alone."""
    import shutil

    src = rc.calib_folder(case, calib_dir, tmp_dir)
    folder = tmp_dir / f"calib_marked_{case.name}"
    if not folder.exists():
        shutil.copytree(src, folder)
        d = dict(np.load(src / "polycalib.npz"))
        im, idd = np.mgrid[0:NB, 0:NB]
        mark = 255.0 * 0.004 * ((3 * im + 5 * idd) % 16 - 8)
        for k in ("grad_b", "grad_g", "grad_r"):
            d[k] = d[k].copy()
            d[k][..., 5] += mark.astype(d[k].dtype)
        np.savez(folder / "polycalib.npz", **d)
    return folder


def record_gap(oracle, im_a, im_b):
    """(nb, H, W): per direction bin and pixel, the largest channel difference between the shading of magnitude bins im_a and im_b.
    The streaming tail shows its bins through the RGB alone, and the shipped table holds the SAME record in neighbouring magnitude
    bins for many directions (82 of 125 between bins 0 and 1; 13 514 distinct records in all): a probe of a bin edge has to sit in a
    direction where the two records differ."""
    I = np.einsum("cmdk,hwk->cmdhw", oracle.poly[:, [im_a, im_b]].astype(np.float64), oracle.feat.astype(np.float64))
    return np.abs(I[:, 0] - I[:, 1]).max(axis=0)


def threshold_dirs(oracle, n=8):
    """The n direction bins whose records of magnitude bins 0 and 1 differ most (median over the frame), axis neighbours left out."""
    gap = np.median(record_gap(oracle, 0, 1).reshape(NB, -1), axis=1)
    gap[[0, 30, 31, 61, 62, 92, 93, 123, 124]] = -1.0
    return np.sort(np.argsort(gap)[-n:])


def threshold_points(gs, zmax, dir_bins):
    """Facets at t = tan(x_binr) shifted by -+ 4 tau_mag, in the given directions: (mags, dirs, im) with im = 0 below and 1 above -
    the threshold of the streaming tail's magnitude shortcut (`mag0_t2`) and of its LDS / gathered records."""
    n = len(dir_bins)
    tm, _ = tau(zmax, math.tan(X_BINR), gs)
    dirs = bin_point(0, np.asarray(dir_bins))[1]
    mags = np.concatenate([np.full(n, X_BINR - 4.0 * tm), np.full(n, X_BINR + 4.0 * tm)])
    return mags, np.concatenate([dirs, dirs]), np.repeat([0, 1], n)


ROW_CASE = "80x128-S320"  # streaming <9,5,3,5> behind MFMA levels, one strip: a wave holds a whole row
ROW_DOME = (44, 6, 3)     # centre row, contact radius, distance of the probed row from the contact's edge (pixels)
ROW_SHEARS = (0.5, -0.5, 0.8, -0.8, 1.1, -1.1, 1.4, -1.4, 0.3, -0.3)  # tried in this order
ROW_GAP = 1e-3            # the records on the two sides of the edge differ by at least this at the probed pixel (10 x the RGB tolerance)


def _row_frames(case, oracle, shear):
    H, W = case.shape
    cy, r, gap = ROW_DOME
    y = cy - r - gap
    gs = grad_scales(oracle.p, case.shape)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    # The dent sits a third into the row: with one strip of W = 128, lane 0 holds the mirrored columns 12..10 and lane 63 the
    # mirrored columns 77..75 (halo of 10 pixels, 3 pixels per lane), and the gel must be ~0 at BOTH for the wave to take the shortcut
    # (asserted on the CPU).  Its centre lies between pixels: a pixel exactly on the bottom of a symmetric dent has t == 0 in
    # float64 and a direction made of round-off in float32.
    variants = [(W // 3 + dx + 0.2, side) for dx in (1, 2, 3) for side in (1, -1)]
    base = np.stack([np.minimum(((yy - cy - 0.3) ** 2 + (xx - cx - shear * (yy - cy - 0.3)) ** 2) / r**2, 4.0)
                     for cx, _ in variants])  # heights above the dent's bottom for a press depth of 1
    Z1, _ = oracle.gel_pad_deformation(oracle.shifted_height_map(base.astype(F32), np.ones(len(base), F32)))
    _, mag1, _, _, idd1 = oracle.shade(Z1, True)
    x = mag1[:, y, :].argmax(axis=1)
    t1 = np.tan(mag1[np.arange(len(x)), y, x])
    z1 = np.abs(Z1).max(axis=(1, 2))
    side = np.array([s for _, s in variants], np.float64)
    s = math.tan(X_BINR) / t1
    for _ in range(3):  # tau follows the frame's heights, which follow the scale
        tm, _ = tau(s * z1, math.tan(X_BINR), gs)
        s = np.tan(X_BINR + side * 4.0 * tm) / t1
    return (base * s[:, None, None]).astype(F32), s.astype(F32), [(y, sd) for _, sd in variants], x, idd1[np.arange(len(x)), y, x]


def row_threshold_frames(case, oracle):
    """Frames that reach the streaming tail's magnitude shortcut where it is TAKEN.  A frame that is in contact everywhere never
    takes it: the wave's outermost lanes blur against the zero the lane shift feeds them, and at a deformed gel of -press that is a
    gradient far above the threshold - the wave evaluates every magnitude (correct, and why the facets above cannot show a shifted
    threshold).  Here a small paraboloid dent sits in a gel that is 0 at the row ends, and ONE row above it is probed: the dent's
    depth is scaled (the deformed gel is linear in it: the contact mask does not change) until the row's steepest pixel lies 4 tau_mag
    above (side +1: it alone must make the wave evaluate, and carries bin 1) or below (side -1: the whole row is bin 0) the first
    magnitude-bin edge.  The dent's column takes each of the three pixel slots of a lane.  The dent is sheared - the steepest pixel
    of a row above it then does not look along an image axis (a bin edge) - by the first of ROW_SHEARS that puts every probed pixel
    into a direction bin whose records of magnitude bins 0 and 1 differ there (record_gap).  Returns hm, press, [(row, side)]."""
    gap01 = record_gap(oracle, 0, 1)
    for shear in ROW_SHEARS:
        hm, press, rows, x, idd = _row_frames(case, oracle, shear)
        if all(gap01[d, y, xi] >= ROW_GAP for (y, _), xi, d in zip(rows, x, idd)):
            return hm, press, rows
    raise AssertionError("no shear of ROW_SHEARS puts the probed pixels into a direction whose records differ")


# ---- the margin rule -------------------------------------------------------------------------------------------------------------
def margins(oracle, Z):
    """Which pixels of Z (frames, H, W; the lattice's heights or the float64 oracle's deformed gel) must agree with the float64
    oracle: dict rgb, im, idd, mag, dir (oracle.shade), `flat` (t == 0: record FLAT, compared), `tiny` (0 < t^2 < 1e-30: not
    compared), `compare` (flat, or farther than tau from every bin edge)."""
    assert oracle.blur_mode == "direct"
    Z = np.asarray(Z)
    rgb, mag, dr, im, idd = oracle.shade(Z, True)
    gs = grad_scales(oracle.p, (oracle.H, oracle.W))
    flat = mag == 0.0                        # atan(t) == 0 only at t == 0
    tiny = ~flat & (mag * mag < TINY_T2)     # atan(t) == t down there
    zmax = np.abs(Z).max(axis=(-2, -1), keepdims=True)
    t = np.tan(mag)
    tm, td = tau(np.broadcast_to(zmax, mag.shape), t, gs)
    um, ud = mag / X_BINR, (dr + math.pi) / Y_BINR
    fm, fd = um - np.floor(um), ud - np.floor(ud)
    d_mag = np.where(im == 0, 1.0 - fm, np.minimum(fm, 1.0 - fm)) * X_BINR  # (the lower edge of magnitude bin 0 is no edge)
    d_dir = np.minimum(fd, 1.0 - fd) * Y_BINR
    compare = flat | (~tiny & (d_mag > tm) & (d_dir > td))
    return {"rgb": rgb, "im": im, "idd": idd, "mag": mag, "dir": dr, "flat": flat, "tiny": tiny, "compare": compare}


def z_tolerance(Z):
    """Per-frame bound on |Z - Zo| in mm: the project's 1e-5 mm, or 4 ulp32 of the frame's max |Z| where that is larger (a steep facet
    spans metres: 1e-5 mm is below ONE ulp of such heights)."""
    return np.maximum(1e-5, 4.0 * ulp32(np.abs(Z).max(axis=(-2, -1))))


# ---- the float64 oracle's results, computed once per case, kind and process ---------------------------------------------------------
FACET_CASES = ("48x64-S320", "40x80-S320", "64x128-S640", "33x70-S320")
_REFERENCE: dict = {}


def reference(case, kind, calib_dir, tmp_dir):
    """kind "facets" (facet_targets), "threshold" (threshold_points), "rows" (row_threshold_frames), "half" / "strip"
    (composite_targets): dict folder, oracle, hm,
    press, Z, M, `m` (margins of Z), interior and - facets / threshold - the intended bins im, idd per frame.  Shared by every test of
    a process: the arrays are read-only."""
    key = (case.name, kind)
    ref = _REFERENCE.get(key)
    if ref is None:
        from oracle.taxim_oracle import TaximOracle

        folder = (marked_calib_folder if kind == "rows" else rc.calib_folder)(case, calib_dir, tmp_dir)
        o = TaximOracle(folder, case.shape, "direct")
        gs, cs = grad_scales(o.p, case.shape), o.p.sim["contact_scale"]
        ref = {"folder": folder, "oracle": o, "gs": gs, "interior": interior(case)}
        if kind == "facets":
            ref["im"], ref["idd"] = facet_targets()
            ref["hm"], ref["press"] = facet_frames(case, *bin_point(ref["im"], ref["idd"]), gs, cs)
        elif kind == "threshold":
            mags, dirs, ref["im"] = threshold_points(gs, 1.5, threshold_dirs(o))  # (heights of these frames: the press depth, 1 to 2 mm - asserted on the CPU)
            ref["idd"] = np.floor((dirs + math.pi) / Y_BINR).astype(np.int64)
            ref["hm"], ref["press"] = facet_frames(case, mags, dirs, gs, cs)
        elif kind == "rows":
            ref["hm"], ref["press"], ref["rows"] = row_threshold_frames(case, o)
        else:
            ref["hm"], ref["press"], ref["facet"] = composite_frames(case, *bin_point(*composite_targets()), kind, gs, cs)
        ref["Z"], ref["M"] = o.gel_pad_deformation(o.shifted_height_map(ref["hm"], ref["press"]))
        ref["m"] = margins(o, ref["Z"])
        for v in list(ref.values()) + list(ref["m"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCE[key] = ref
    return ref


def site_mask(shape_fhw, sites):
    m = np.zeros(shape_fhw, bool)
    m[sites[:, 0], sites[:, 1], sites[:, 2]] = True
    return m
