"""Cases that put the Taxim shadow branch (taxim_shadow.hip: shade_raw_kernel, fill_kernel, shadow_ray_kernel, blur_nhwc3_kernel) off
320x240 / 640x480 (tests/test_taxim_shadow_gpu.py).  Nothing here touches the GPU; tests/test_taxim_shadow_cases.py checks on the CPU
that every case is what it claims to be.

With the shipped calibration a frame below roughly 200 px gets 1x1 dilation rounds, hence no ring and no shadow sample at all.  Every
small case therefore runs on a calibration folder of its own whose shadow parameters are given IN PIXELS (divided by the case's own W
along x, H along y): dilation window, ray steps, shadow blur, and a short deformation pyramid.  "Curved" cases replace the all-zero
gel map by an off-centre dome (gel down to about -1.5 mm) and press deep enough for the contact mask to survive on it.

BOUNDS holds the RGB bound of each case against the float64 oracle: max(1e-6, 4 x max|f32 - f64|) of the oracle's own shadow branch
evaluated with float32 and with float64 image blurs, on the same-bin field of the case (test_taxim_shadow_cases.py recomputes it).
1e-6 is the figure of test_shadow_branch_vs_reference_and_oracle; the factor 4 allows for another, equivalent summation order and
fma contraction."""
from __future__ import annotations

import json
import math
import shutil
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import taxim_route_cases as rc

F32 = np.float32
FAR_MM = rc.FAR_MM

PYR_SHORT = ([1.75, 1.0, 0.55], 1.0)   # kernel sizes [9,5,3 | 5]
PYR_640 = ([3.5, 2.0, 1.1], 2.0)       # [15,9,5 | 9]: the tail of the 640x480 level set


@dataclass(frozen=True)
class Case:
    H: int
    W: int
    attach: tuple | None     # shadow_attachment_kernel_size in px (w, h); None = the shipped calibration folder as it is
    step: tuple | None       # shadow_step in px (w_rel * W, h_rel * H): step_y = step[0], step_x = step[1] (sic, TT:300-305)
    sblur: tuple | None      # shadow_blur_sigma in px (w, h)
    gel: str                 # "flat" (the shipped all-zero map) or "curved" (off-centre dome)
    win: tuple               # dilation window (left, right, top, bottom)
    sblur_k: tuple           # shadow blur kernel size (kw, kh)
    final_k: int             # final blur kernel size
    rem: int                 # H * W % 256: threads of the last block of the per-pixel kernels beyond the frame (0: none)
    pyr: tuple | None = PYR_SHORT
    ring: bool = True
    extra_frames: tuple = ()  # frame kinds in front of the standard four
    note: str = ""

    @property
    def name(self) -> str:
        return f"{self.H}x{self.W}-{self.gel}"

    @property
    def shape(self):
        return (self.H, self.W)

    @property
    def frames(self) -> tuple:  # the last frame is the one rendered alone (B = 1): it holds contact
        std = ("deep", "deepcorners", "none", "deepseam") if self.gel == "curved" else ("synthetic", "corners", "none", "seam")
        return self.extra_frames + std

    @property
    def step_xy(self) -> tuple:  # (step_x, step_y) as the kernel gets them
        return None if self.step is None else (self.step[1], self.step[0])

    @property
    def unequal_steps(self) -> bool:
        return self.step is not None and self.step[0] != self.step[1]

    @property
    def footprint(self) -> tuple:  # (rows, columns) of the two image blurs combined
        return (self.sblur_k[1] + self.final_k - 1, self.sblur_k[0] + self.final_k - 1)


CASES = (
    Case(33, 70, (2.5, 2.5), (0.625, 0.625), (0.55, 0.55), "flat", (1, 2, 1, 2), (3, 3), 5, 6, note="npix % 256 = 6; W % 4 != 0; the 320x240 window"),
    Case(37, 68, (1.0, 2.5), (0.5, 0.75), (1.0, 0.55), "flat", (0, 0, 1, 2), (5, 3), 5, 212, note="window along y only; unequal steps; blur 5x3; odd H"),
    Case(37, 68, (1.0, 2.5), (0.5, 0.75), (1.0, 0.55), "curved", (0, 0, 1, 2), (5, 3), 5, 212, note="... with a non-zero gel map in the height bin"),
    Case(48, 64, (2.5, 1.0), (0.75, 0.5), (0.55, 1.0), "curved", (1, 2, 0, 0), (3, 5), 5, 0, note="window along x only; steps the other way round; blur 3x5"),
    Case(16, 16, (2.5, 2.5), (0.625, 0.625), (0.55, 0.55), "flat", (1, 2, 1, 2), (3, 3), 5, 0, note="the 31 px ray is longer than the frame"),
    Case(9, 12, (2.5, 2.5), (0.625, 0.625), (0.55, 0.55), "curved", (1, 2, 1, 2), (3, 3), 5, 108, note="image bytes no multiple of 256: ShadowLayout padding"),
    Case(40, 400, (5.0, 5.0), (1.25, 1.25), (1.1, 1.1), "flat", (4, 4, 4, 4), (5, 5), 9, 128, pyr=PYR_640, extra_frames=("inset",),
         note="the 640x480 parameter set on a wide strip; a contact just inside the right border, whose rays leave there"),
    Case(50, 70, (0.5, 0.5), (0.625, 0.625), (0.55, 0.55), "flat", (0, 0, 0, 0), (3, 3), 5, 172, ring=False, note="1x1 rounds: no ring, two blurs only"),
    Case(243, 324, None, None, None, "flat", (1, 2, 1, 2), (3, 3), 5, 140, pyr=None, note="shipped folder just off 320x240 (npix % 256 = 140); many frames"),
)
BY_NAME = {c.name: c for c in CASES}
MANY_FRAMES_CASE, MANY_FRAMES_B = "243x324-flat", 72  # B*H*W*3 > 65536 * 256: fill_kernel's grid-stride loop takes a second trip

# RGB bound per case (see the module docstring), recomputed and compared by test_taxim_shadow_cases.py::test_protocol_conditioning_and_bounds.
# The oracle's float32 and float64 evaluations differ by 1.19e-7 (one float32 spacing below 1) in every case but 40x400 (1.79e-7), so each
# bound is the floor of 1e-6.
BOUNDS = {
    "33x70-flat": 1e-6, "37x68-flat": 1e-6, "37x68-curved": 1e-6, "48x64-curved": 1e-6, "16x16-flat": 1e-6, "9x12-curved": 1e-6,
    "40x400-flat": 1e-6, "50x70-flat": 1e-6, "243x324-flat": 1e-6,
}


# ---- calibration folders ---------------------------------------------------------------------------------------------------
def dome(shape_hw) -> np.ndarray:
    """The dome of test_curved_gel_map_general_path with its apex moved off the centre by non-integer amounts (gel map in calibration
    pixels; after the oracle's shift the far corner lies about -1.5 mm below the apex)."""
    h, w = shape_hw
    yy, xx = np.mgrid[0:h, 0:w].astype(F32)
    cy, cx = (h - 1) / 2 + 37.3, (w - 1) / 2 - 52.6
    return (-((yy - F32(cy)) ** 2 + (xx - F32(cx)) ** 2) / F32(4000.0)).astype(F32)


def calib_folder(case: Case, calib_dir: Path, tmp_dir: Path) -> Path:
    """The folder TaximOracle AND Taxim read for this case."""
    if case.attach is None and case.gel == "flat":
        return Path(calib_dir)
    folder = Path(tmp_dir) / f"calib_shadow_{case.name}"
    if not folder.exists():
        shutil.copytree(calib_dir, folder)
        params = json.loads((folder / "params.json").read_text())
        sim, (H, W) = params["simulator"], case.shape
        if case.attach is not None:
            pyr, fin = case.pyr
            sim["shadow_attachment_kernel_size_rel"] = [case.attach[0] / W, case.attach[1] / H]
            sim["shadow_step_rel"] = [case.step[0] / W, case.step[1] / H]
            sim["shadow_blur_sigma_rel"] = [case.sblur[0] / W, case.sblur[1] / H]
            sim["deform_pyramid_sigma_rel"] = [[s / W for s in pyr], [s / H for s in pyr]]
            sim["deform_final_sigma_rel"] = [fin / W, fin / H]
        (folder / "params.json").write_text(json.dumps(params, indent=2))
        if case.gel == "curved":
            np.save(folder / "gelmap.npy", dome(np.load(folder / "gelmap.npy").shape))
    return folder


# ---- frames ------------------------------------------------------------------------------------------------------------------
DEEP = 3.6  # a curved case presses this many times deeper, so that contact reaches below the dome's rim and keeps its shrunken mask


def _deepen(hm: np.ndarray) -> np.ndarray:
    return FAR_MM - (FAR_MM - hm) * DEEP


def frames(case: Case) -> np.ndarray:
    """(B, H, W) float32 camera depth in mm, one frame per entry of case.frames."""
    from tacex_amd.utils.synthetic import synthetic_depth_maps

    H, W = case.shape
    out = []
    for kind in case.frames:
        if kind in ("synthetic", "deep"):
            hm = synthetic_depth_maps(1, H, W, seed=1000 * H + W, flat_fraction=0.0)[0][0].numpy().astype(np.float64)
        elif kind in ("corners", "deepcorners"):
            hm = rc._corners(H, W)
        elif kind in ("seam", "deepseam"):
            hm = rc._seam(H, W)
        elif kind == "none":
            hm = np.full((H, W), FAR_MM)
        elif kind == "inset":  # a cone whose ring still has pixels between it and the right border
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
            r = max(3, min(H, W) // 7)
            d = np.hypot(yy - H // 2, xx - (W - 3 - r))
            hm = np.where(d < r, 27.9 + 0.3 * d / r, FAR_MM)
        else:
            raise ValueError(kind)
        out.append(_deepen(hm) if kind.startswith("deep") else hm)
    return np.stack(out).astype(F32)


# ---- the kernel's normals, restated in NumPy float32 ---------------------------------------------------------------------------
def standin_bins(o, Z32: np.ndarray):
    """shade_raw_kernel's bins with exact arctan / arctan2 in place of its fast approximations: central differences of the float32 gel at
    the clamped pixel times gsy / gsx, sqrt, atan, atan2, floor(x * (1 / bin width)), clamped to the table."""
    Z = np.asarray(Z32, F32)
    H, W = Z.shape[-2:]
    gsy = F32(0.5 * H / o.p.calib_h / float(F32(o.p.pixmm)))
    gsx = F32(0.5 * W / o.p.calib_w / float(F32(o.p.pixmm)))
    yc, xc = np.clip(np.arange(H), 1, H - 2), np.clip(np.arange(W), 1, W - 2)
    dzdx = ((Z[..., yc - 1, :][..., xc] - Z[..., yc + 1, :][..., xc]) * gsy).astype(F32)
    dzdy = ((Z[..., yc, :][..., xc - 1] - Z[..., yc, :][..., xc + 1]) * gsx).astype(F32)
    t = np.sqrt((dzdx * dzdx + dzdy * dzdy).astype(F32)).astype(F32)
    mag = np.arctan(t).astype(F32)
    dr = np.where(t != 0, np.arctan2(dzdx, dzdy), F32(0)).astype(F32)
    nb = o.p.num_bins
    x_binr, y_binr = F32(0.5 * math.pi / (nb - 1)), F32(2 * math.pi / (nb - 1))
    inv_x, inv_y = F32(1.0 / float(x_binr)), F32(1.0 / float(y_binr))
    im = np.clip(np.floor(mag * inv_x).astype(np.int64), 0, nb - 1)
    idd = np.clip(np.floor((dr + F32(3.14159274101257324)) * inv_y).astype(np.int64), 0, nb - 1)
    return im, idd


def oracle_bins(o, Z32: np.ndarray):
    """The bins the oracle's shadow branch shades a float32 deformed gel with (shade_with_shadow)."""
    Zf = np.asarray(Z32, F32)
    return o.bins(*o.normals(-(Zf / F32(o.p.pixmm))))


def same_bin_field(case: Case, im, idd, im_o, id_o) -> np.ndarray:
    """Pixels whose whole footprint of the two image blurs (mirrored at the border: the frame's outside counts as equal) was shaded
    from the same polynomial record on both sides."""
    from scipy import ndimage

    same = (np.asarray(im) == im_o) & (np.asarray(idd) == id_o)
    st = np.ones(case.footprint)
    return np.stack([ndimage.binary_erosion(same[b], structure=st, border_value=1) for b in range(same.shape[0])])


# ---- the oracle's results, computed once per case and process ------------------------------------------------------------------
_REFERENCE: dict = {}


def reference(case: Case, calib_dir: Path, tmp_dir: Path) -> dict:
    """folder, tables (build_taxim_tables), shadow (build_shadow_tables), oracle, hm, indent, the float64 oracle's Z and M, Z32 =
    Z.astype(float32), shadow_map / gdir = oracle.shadow_map(Z32, M), ring, samples (oracle.shadow_samples).  Shared by every test of
    a process; callers must not write into the arrays."""
    ref = _REFERENCE.get(case.name)
    if ref is None:
        from oracle.taxim_oracle import TaximOracle
        from tacex_amd.calibration import build_shadow_tables, build_taxim_tables

        folder = calib_folder(case, calib_dir, tmp_dir)
        o = TaximOracle(folder, case.shape, "direct")
        hm = frames(case)
        indent = o.indentation_depth(hm)
        Z, M = o.gel_pad_deformation(o.shifted_height_map(hm, indent))
        Z32 = Z.astype(F32)
        smap, gdir = o.shadow_map(Z32, M)
        tables = build_taxim_tables(folder, case.shape)
        ref = {"folder": folder, "tables": tables, "shadow": build_shadow_tables(folder, tables), "oracle": o, "hm": hm, "indent": indent,
               "Z": Z, "M": M, "Z32": Z32, "shadow_map": smap, "gdir": gdir.astype(F32), "ring": o.ring(M),
               "samples": o.shadow_samples(Z32, M, gdir)}
        for v in list(ref.values()) + list(ref["samples"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCE[case.name] = ref
    return ref


def bound(case: Case) -> float:
    return BOUNDS[case.name]


def measure_bound(case: Case, ref: dict):
    """(bound, field share of all pixels, field share of the pixels that receive a shadow sample) from the oracle and the NumPy
    stand-in of the kernel's normals alone."""
    o, Z32, M = ref["oracle"], ref["Z32"], ref["M"]
    field = same_bin_field(case, *standin_bins(o, Z32), *oracle_bins(o, Z32))
    hit = np.isfinite(ref["shadow_map"]).any(-1)
    d = np.abs(o.shade_with_shadow(Z32, M, work_dtype=F32).astype(np.float64) - o.shade_with_shadow(Z32, M).astype(np.float64))
    err = float(d[field].max())
    return max(1e-6, 4.0 * err), float(field.mean()), (float(field[hit].mean()) if hit.any() else float("nan"))
