"""Small deterministic relief tiles for `ReliefHeightMapSource` (NumPy, no random numbers): textures a GelSight is pressed on.  Heights
are in mm above the carrier, 0 at the lowest point of a wrapping tile; every generator returns a `ReliefTile`."""
from __future__ import annotations

import numpy as np

from ..relief_source import ReliefTile


def _grid(rows: int, cols: int):
    if int(rows) < 1 or int(cols) < 1:
        raise ValueError(f"relief tile of {rows} x {cols} texels")
    return np.meshgrid(np.arange(int(rows), dtype=np.float64), np.arange(int(cols), dtype=np.float64), indexing="ij")


def from_array(height_mm, pitch_mm: float, wrap: bool = True, anchor=None) -> ReliefTile:
    """Any (rows, cols) array of heights [mm] (a scanned coin, a rendered logo); -inf marks texels without material."""
    return ReliefTile(np.array(height_mm, dtype=np.float32), pitch_mm, wrap, anchor)


def weave(size: int = 64, threads: int = 4, amplitude_mm: float = 0.12, pitch_mm: float = 0.02) -> ReliefTile:
    """Plain weave: `threads` warp and weft threads per side, each a raised cosine band, going over and under by turns."""
    if int(threads) < 2 or int(threads) % 2:
        raise ValueError(f"weave: threads = {threads} (an even number: the over / under pattern repeats every two threads)")
    v, u = _grid(size, size)
    p = size / float(threads)
    a, b = u / p, v / p  # thread coordinates
    warp = 0.5 * (1.0 + np.cos(2.0 * np.pi * a)) * (0.5 + 0.5 * np.cos(np.pi * (a + b)))  # threads along v, on top where a + b is even
    weft = 0.5 * (1.0 + np.cos(2.0 * np.pi * b)) * (0.5 - 0.5 * np.cos(np.pi * (a + b)))  # threads along u, on top where it is odd
    h = np.maximum(warp, weft)
    return ReliefTile((amplitude_mm * h / h.max()).astype(np.float32), pitch_mm, True)


def knurl(size: int = 64, pitch_texels: int = 16, depth_mm: float = 0.15, pitch_mm: float = 0.02) -> ReliefTile:
    """Diamond knurling: pyramids on a grid turned by 45 degrees."""
    v, u = _grid(size, size)
    p = float(pitch_texels)
    d1, d2 = np.mod(u + v, p) / p, np.mod(u - v, p) / p
    h = np.minimum(1.0 - np.abs(2.0 * d1 - 1.0), 1.0 - np.abs(2.0 * d2 - 1.0))
    return ReliefTile((depth_mm * h).astype(np.float32), pitch_mm, True)


def grooves(size: int = 64, period_texels: int = 8, depth_mm: float = 0.1, pitch_mm: float = 0.02) -> ReliefTile:
    """Parallel ridges along the tile's u (a thread, a file): a raised cosine across v."""
    v, _ = _grid(size, size)
    h = 0.5 * (1.0 + np.cos(2.0 * np.pi * v / float(period_texels)))
    return ReliefTile((depth_mm * h).astype(np.float32), pitch_mm, True)


def dots(size: int = 64, spacing_texels: int = 32, radius_texels: float = 10.0, pitch_mm: float = 0.02) -> ReliefTile:
    """Hemispherical studs on a square grid (braille-like): height sqrt(r^2 - d^2) inside a stud, 0 between them."""
    v, u = _grid(size, size)
    s = float(spacing_texels)
    du, dv = np.mod(u, s) - 0.5 * (s - 1.0), np.mod(v, s) - 0.5 * (s - 1.0)
    q = radius_texels ** 2 - (du * du + dv * dv)
    return ReliefTile((pitch_mm * np.sqrt(np.maximum(q, 0.0))).astype(np.float32), pitch_mm, True)


def disc_stamp(size: int = 96, rings: int = 4, depth_mm: float = 0.12, pitch_mm: float = 0.02) -> ReliefTile:
    """A round stamp (a coin): concentric ridges inside a circle, no material (-inf) outside it; does not wrap."""
    v, u = _grid(size, size)
    c = 0.5 * (size - 1.0)
    r = np.sqrt((u - c) ** 2 + (v - c) ** 2) / (0.5 * size)
    h = depth_mm * 0.5 * (1.0 + np.cos(2.0 * np.pi * rings * r))
    h = np.where(r <= 1.0, h, -np.inf)
    return ReliefTile(h.astype(np.float32), pitch_mm, False)
