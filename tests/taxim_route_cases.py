"""Cases that put every Taxim blur route and both fused tails off the two tuned resolutions (tests/test_taxim_routes_gpu.py).

Nothing here touches the GPU: the case table, the calibration folders the cases run on, their input frames, a Python restatement
of the host predicates that pick a level's kernel and a pass's ending (taxim_kernels.hip `blur_level_route`, taxim_mfma.hip
`mfma_supported`, taxim_tail.hip `tail_levels`, taxim_stream.hip `stream_supported` / `stream_geometry_t`, at their default
environment) and the oracle's results per case are exercised on their own by tests/test_taxim_route_cases.py.

The tuned kernels are eligible wherever the w and h taps of a level are bit-equal.  With the shipped calibration that is every
4:3 frame; every other frame gets a calibration folder of its own whose `deform_pyramid_sigma_rel` / `deform_final_sigma_rel`
give the same sigma IN PIXELS along both axes (SIGMA_SETS).
"""
from __future__ import annotations

import json
import shutil
from dataclasses import dataclass
from pathlib import Path

import numpy as np

F32 = np.float32

# sigmas in pixels: pyramid levels | final blur -> kernel sizes (asserted per case by the CPU test)
SIGMA_SETS = {
    "S320": ([15.25, 7.75, 4.0, 1.75, 1.0, 0.55], 1.0),   # [61,33,17,9,5,3,5]: the 320x240 level set
    "S640": ([30.5, 15.5, 8.0, 3.5, 2.0, 1.1], 2.0),      # [117,61,33,15,9,5,9]: the 640x480 level set
    "T4": ([4.0, 1.75, 1.0, 0.55], 1.0),                  # [17,9,5,3,5]
    "T4s": ([1.75, 1.75, 1.0, 0.55], 1.0),                # [9,9,5,3,5]
    "T3s": ([3.5, 3.5, 2.0, 1.1], 2.0),                   # [15,15,9,5,9]
    "F4": ([1.75, 1.0, 0.55], 1.0),                       # [9,5,3,5]: nothing in front of the tail
}

FRAMES = ("synthetic", "corners", "none", "seam")  # the last frame is the one rendered alone (B = 1): it holds contact
STRONG_MIN = 300  # strong-gradient pixels (oracle, grad_mag > 1e-3) from which the >= 99 % same-bin share is asserted


@dataclass(frozen=True)
class Case:
    H: int
    W: int
    sigmas: str | None       # key of SIGMA_SETS, None = the shipped calibration
    ksize: tuple             # kernel size per level
    levels: str              # route per level in front of the tail: M mfma, B band, L3 / L6 band_loop_384 / _640, G generic
    n_fused: int             # levels in the fused tail (0: none)
    tail: str                # how a plain render ends: stream, tiled or shade
    strong: bool             # the oracle shows >= STRONG_MIN strong-gradient pixels over the case's frames
    frames: tuple = FRAMES
    note: str = ""

    @property
    def name(self) -> str:
        return f"{self.H}x{self.W}-{self.sigmas or 'shipped'}"

    @property
    def shape(self):
        return (self.H, self.W)

    @property
    def level_routes(self) -> list:
        names = {"M": "mfma", "B": "band", "L3": "band_loop_384", "L6": "band_loop_640", "G": "generic"}
        return [names[t] for t in self.levels.split()] + ["tail"] * self.n_fused

    @property
    def tail_frames(self) -> str:  # ending of a render with z_out / mask_out, and of deform()
        return "tiled" if self.n_fused else "shade"


K320, K640 = (61, 33, 17, 9, 5, 3, 5), (117, 61, 33, 15, 9, 5, 9)
CASES = (
    Case(32, 64, "S320", K320, "M M M", 4, "stream", True, note="k=61 at its smallest frame: window mirrored at top and bottom at once; one 64-column wave, one strip"),
    Case(48, 64, "S320", K320, "M M M", 4, "stream", True, note="three bands; tile rows 32 + 16"),
    Case(80, 128, "S320", K320, "M M M", 4, "stream", True, note="five bands (zero-band skipping), two waves (zero-block skipping)"),
    Case(64, 128, "S640", K640, "M M M M", 3, "stream", True, note="k=117 at its smallest frame (R=58 < 64, RA=64 < 128); <9,5,9>"),
    Case(40, 80, "S320", K320, "B B B", 4, "stream", True, note="unrolled band kernels, W % 64 != 0, H % 32 = 8"),
    Case(40, 400, "S320", K320, "L6 G G", 4, "stream", True, note="looped kernel, 640-thread form; seven tile columns; strips 3 x 136"),
    Case(37, 68, "S320", K320, "G G G", 4, "stream", True, note="generic levels feeding a tail; odd H; W % 16 != 0"),
    Case(33, 70, "S320", K320, "G G G G G G G", 0, "shade", True, note="W % 4 != 0: shade alone, k=61 generic"),
    Case(16, 16, "T4s", (9, 9, 5, 3, 5), "G", 4, "stream", True, note="smallest streaming frame; a strip narrower than its halo"),
    Case(20, 168, "T4", (17, 9, 5, 3, 5), "G", 4, "stream", True, note="one strip of exactly VW"),
    Case(20, 172, "T4", (17, 9, 5, 3, 5), "G", 4, "stream", True, note="two strips of 88"),
    Case(24, 340, "T4", (17, 9, 5, 3, 5), "G", 4, "stream", True, note="three strips"),
    Case(10, 12, "T4s", (9, 9, 5, 3, 5), "G", 4, "tiled", True, note="H = summed radii + 1 of <9,5,3,5>; H < 16: tiled only"),
    Case(8, 8, "T4s", (9, 9, 5, 3, 5), "G G G G G", 0, "shade", False, note="H, W <= summed radii: no tail (was admitted)"),
    Case(9, 12, "T4s", (9, 9, 5, 3, 5), "G G G G G", 0, "shade", True, note="H = summed radii: no tail (was admitted)"),
    Case(12, 8, "T4s", (9, 9, 5, 3, 5), "G G G G G", 0, "shade", False, note="W < summed radii: no tail (was admitted)"),
    Case(11, 12, "T3s", (15, 15, 9, 5, 9), "G G", 3, "tiled", True, note="H = summed radii + 1 of <9,5,9>; tiled only"),
    Case(10, 12, "T3s", (15, 15, 9, 5, 9), "G G G G G", 0, "shade", True, note="H = summed radii of <9,5,9>: no tail"),
    Case(48, 64, "F4", (9, 5, 3, 5), "G B B B", 0, "shade", True, note="four levels, nothing in front of the tail: no tail (read a null input)"),
    Case(243, 324, None, K320, "G G G", 4, "stream", True, note="odd H; W % 64 = 4; two strips of 164; segmented strips"),
    Case(252, 336, None, (63, 35, 19, 9, 5, 3, 5), "L3 L3 G", 4, "stream", True, note="looped <384> as first and later level; strips 2 x 168"),
    Case(192, 256, None, (49, 27, 15, 7, 5, 3, 5), "L3 G M G B B B", 0, "shade", True, note="k=49 looped first; MFMA k=15 in the middle; shade alone"),
    Case(288, 384, None, (73, 39, 21, 9, 5, 3, 5), "L3 L3 G", 4, "stream", True, note="W = 384, the launch_band limit"),
    Case(432, 576, None, (105, 57, 31, 15, 9, 5, 9), "L6 L6 G M", 3, "stream", True, note="MFMA k=15 at nine waves; <9,5,9> at H % 32 = 16"),
    Case(483, 644, None, (117, 63, 33, 15, 9, 5, 9), "G G G G", 3, "stream", True, frames=("corners+seam",), note="<9,5,9> with W % 64 = 4; four strips of 164"),
)
BY_NAME = {c.name: c for c in CASES}
BAND_SKIP_CASES = ("80x128-S320", "64x128-S640", "432x576-shipped")


# ---- calibration folders ---------------------------------------------------------------------------------------------------
def calib_folder(case: Case, calib_dir: Path, tmp_dir: Path) -> Path:
    """The folder TaximOracle AND Taxim read for this case: the shipped one, or a copy under tmp_dir whose params.json holds the
    case's sigma set relative to its own frame (sigma_rel = sigma_px / W along x, / H along y)."""
    if case.sigmas is None:
        return Path(calib_dir)
    folder = Path(tmp_dir) / f"calib_{case.name}"
    if not folder.exists():
        shutil.copytree(calib_dir, folder)
        pyr, fin = SIGMA_SETS[case.sigmas]
        params = json.loads((folder / "params.json").read_text())
        params["simulator"]["deform_pyramid_sigma_rel"] = [[s / case.W for s in pyr], [s / case.H for s in pyr]]
        params["simulator"]["deform_final_sigma_rel"] = [fin / case.W, fin / case.H]
        (folder / "params.json").write_text(json.dumps(params, indent=2))
    return folder


# ---- the host predicates, restated (default environment) ---------------------------------------------------------------------
def mfma_supported(k, first, H, W):
    if W % 64 or W < 64 or W > 640 or H % 16:
        return False
    R = (k - 1) // 2
    if R >= H or R > W - 1 or ((R + 7) & ~7) >= W:
        return False
    return k in ((61, 117) if first else (117, 61, 33, 17, 15, 9))


def band_supported(k, first, H, W):
    if W % 16 or W < 32 or H < 2 or W > 384:
        return False
    R = (k - 1) // 2
    if R >= H or R + 1 > W - 1 or k not in (3, 5, 9, 15, 17, 33, 61):
        return False
    return (not first) or k == 61


def band_loop_supported(k, H, W):
    R = (k - 1) // 2
    return W % 16 == 0 and 32 <= W <= 640 and R < H and ((R + 1) & ~1) <= W - 1 and k >= 35


def level_route(k, same_taps, first, H, W) -> str:
    if same_taps and mfma_supported(k, first, H, W):
        return "mfma"
    unrolled = band_supported(k, first, H, W)
    if same_taps and band_loop_supported(k, H, W) and not unrolled:
        return "band_loop_384" if W <= 384 else "band_loop_640"
    return "band" if same_taps and unrolled else "generic"


def tail_levels(ksize, same_taps, H, W) -> int:
    """taxim_tail.hip `tail_levels` with both conditions this table guards: a band level stays in front of the fused set, and the
    frame exceeds the set's summed radii."""
    n = len(ksize)
    if H < 8 or W < 8 or W % 4 or n < 4 or not all(same_taps[-4:]):
        return 0
    last = tuple(ksize[-4:])
    want = 4 if last == (9, 5, 3, 5) else 3 if last == (15, 9, 5, 9) else 0
    if want == 0 or want >= n:
        return 0
    sum_r = sum((k - 1) // 2 for k in ksize[n - want:])
    return want if H > sum_r and W > sum_r else 0


def expected_routes(ksize, same_taps, H, W) -> dict:
    """The dict Taxim.level_routes() returns, from the restated predicates."""
    n, nf = len(ksize), tail_levels(ksize, same_taps, H, W)
    levels = [level_route(ksize[l], same_taps[l], l == 0, H, W) for l in range(n - nf)] + ["tail"] * nf
    stream = nf > 0 and H >= 16 and W >= 16 and W % 4 == 0
    return {"ksize": list(ksize), "levels": levels, "tail": "stream" if stream else "tiled" if nf else "shade",
            "tail_frames": "tiled" if nf else "shade"}


STREAM_VW = 168  # widest strip of the streaming instantiations <9,5,3,5> and <9,5,9>
TILE_W, TILE_H = 64, 32


def stream_strips(W):
    """(strips, strip width) of the streaming tail (stream_geometry_t)."""
    ns = -(-W // STREAM_VW)
    sw = (-(-W // ns) + 3) & ~3
    if sw > STREAM_VW:
        ns += 1
        sw = (-(-W // ns) + 3) & ~3
    return ns, sw


def seams(H, W):
    """(row, column) the seam frame's bars cross: the first tile seam row and the first strip seam column (the tile seam column /
    the frame's middle where there is one strip / tile only)."""
    ns, sw = stream_strips(W)
    xs = sw if ns > 1 else (TILE_W if W > TILE_W else W // 2)
    ys = TILE_H if H > TILE_H else H // 2
    return ys, xs


def tiled_obs_fusable(H, W, n_fused, oh=32, ow=32) -> bool:
    """taxim_tail.hip `obs_fusable`: can the LDS-tiled tail reduce the (oh, ow) policy observation itself (else: two-pass resize)?"""
    if n_fused == 0 or W % 4:
        return False
    nry, ncx, ky, kx = (8, 11, 16, 24) if n_fused == 4 else (6, 7, 32, 44)

    def longest(n_in, n_out):
        sc = F32(n_in) / F32(n_out)
        sup = max(sc, F32(1.0))
        cnt = []
        for o in range(n_out):
            c = sc * (F32(o) + F32(0.5))
            cnt.append(min(n_in, int(c + sup + F32(0.5))) - max(0, int(c - sup + F32(0.5))))
        return max(cnt)

    scy, scx = F32(H) / F32(oh), F32(W) / F32(ow)
    return bool(F32(32.0) / scy + F32(3.0) <= nry and F32(64.0) / scx + F32(3.0) <= ncx and longest(H, oh) <= ky and longest(W, ow) <= kx)


# ---- frames ------------------------------------------------------------------------------------------------------------------
FAR_MM = 29.0


def _corners(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rc = max(2, min(H, W) // 5)
    hm = np.full((H, W), FAR_MM)
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        d = np.hypot(yy - cy, xx - cx)
        hm = np.where(d < rc, 27.9 + 0.3 * d / rc, hm)  # a cone per corner, every pixel of it deep enough for the shrunken mask
    return hm


def _seam(H, W):
    ys, xs = seams(H, W)
    t = 1 if min(H, W) < 16 else 2
    hm = np.full((H, W), FAR_MM)
    hm[max(0, ys - t):ys + t, max(0, xs - W // 4):xs + W // 4] = 27.5  # across the strip seam column
    hm[max(0, ys - H // 4):ys + H // 4, max(0, xs - t):xs + t] = 27.5  # across the tile seam row
    return hm


def frames(case: Case) -> np.ndarray:
    """(B, H, W) float32 camera depth in mm, one frame per entry of case.frames."""
    from tacex_amd.utils.synthetic import synthetic_depth_maps

    H, W = case.shape
    out = []
    for kind in case.frames:
        if kind == "synthetic":
            out.append(synthetic_depth_maps(1, H, W, seed=1000 * H + W, flat_fraction=0.0)[0][0].numpy().astype(np.float64))
        elif kind == "corners":
            out.append(_corners(H, W))
        elif kind == "seam":
            out.append(_seam(H, W))
        elif kind == "corners+seam":
            out.append(np.minimum(_corners(H, W), _seam(H, W)))
        elif kind == "none":
            out.append(np.full((H, W), FAR_MM))
        else:
            raise ValueError(kind)
    return np.stack(out).astype(F32)


def check_frame_properties(case: Case, M: np.ndarray):
    """The frames are what they claim to be, from the oracle's (shrunken) contact mask alone."""
    H, W = case.shape
    ys, xs = seams(H, W)
    for b, kind in enumerate(case.frames):
        m = M[b]
        if kind == "none":
            assert not m.any(), (case.name, kind)
        if kind == "synthetic":
            assert m.any(), (case.name, kind)
        if "corners" in kind:
            assert m[0, 0] and m[0, W - 1] and m[H - 1, 0] and m[H - 1, W - 1], (case.name, kind)
        if "seam" in kind:
            assert 0 < ys < H and 0 < xs < W and m[ys - 1:ys + 1, xs - 1:xs + 1].all(), (case.name, kind, ys, xs)
            assert m[ys, :xs].any() and m[ys, xs:].any() and m[:ys, xs].any() and m[ys:, xs].any(), (case.name, kind)


# ---- the oracle's results, computed once per case and process ------------------------------------------------------------------
_REFERENCE: dict = {}


def reference(case: Case, calib_dir: Path, tmp_dir: Path) -> dict:
    """folder, tables (build_taxim_tables), hm, indent and the float64 oracle's Z, M, rgb, grad_mag, bins of the case's frames.
    Shared by every test of a process; callers must not write into the arrays."""
    ref = _REFERENCE.get(case.name)
    if ref is None:
        from oracle.taxim_oracle import TaximOracle
        from tacex_amd.calibration import build_taxim_tables

        folder = calib_folder(case, calib_dir, tmp_dir)
        o = TaximOracle(folder, case.shape, "direct")
        hm = frames(case)
        indent = o.indentation_depth(hm)
        Z, M = o.gel_pad_deformation(o.shifted_height_map(hm, indent))
        rgb, mag, _, im, idd = o.shade(Z, True)
        ref = {"folder": folder, "tables": build_taxim_tables(folder, case.shape), "oracle": o, "hm": hm, "indent": indent, "Z": Z, "M": M,
               "rgb": rgb, "mag": mag, "im": im, "idd": idd, "strong": mag > 1e-3}
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCE[case.name] = ref
    return ref


def band_skip_frames(H, W) -> np.ndarray:
    """Small contacts at the top border, at the bottom border and in the middle, and a frame without contact: most 16-row bands of
    the band levels see no contact row in their window."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r = max(4.0, H / 30.0)
    out = []
    for cy, cx in ((2, W // 3), (H - 3, 2 * W // 3), (H // 2, W // 2)):
        d = np.hypot(yy - cy, xx - cx)
        out.append(np.where(d < r, 28.0 + 0.02 * d, FAR_MM))
    out.append(np.full((H, W), FAR_MM))
    return np.stack(out).astype(F32)
