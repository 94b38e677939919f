"""Plain NumPy float32 restatement of the gel memory (`tacex_gel_memory`, include/tacex_hip.h; csrc/gel_memory.hip) and the input
sequences its tests run on.  TEST INFRASTRUCTURE: shared by tests/test_gel_memory.py (CPU) and tests/test_gel_memory_gpu.py.

The contract, per frame, with z0 = float32((gelpad_to_camera_min_distance + gelpad_height) * 1000) [mm] (sum and product in double),
K = 1 or 2 branches of per-pixel float32 state m_k laid out (B, K, H, W), zero after a reset, and the frame's row
[a1, c1, a2, c2, floor_mm, 0, 0, 0] of the coefficient table (an id outside [0, P): all zero):
    t = z0 - hm,  d = t if t > 0 else 0                    (a NaN gives 0)
    m_k' = (a_k * m_k) + (c_k * d)                         two products and a sum, each rounded to float32
    if d == 0 and m_k' < floor_mm:  m_k' = 0
    M = m_1' (K = 1) or m_1' + m_2' (K = 2);  r = z0 - M
    hm' = r if (M > 0 and r < hm) else hm                  in place
    live'[b] = 1 iff a state element of frame b is non-zero
Host side, in float64 and then rounded to float32: a_k = exp(-dt / tau_k) (0 when tau_k == 0), c_k = (1 - a_k) * w_k.
A frame entering with live == 0 and no pixel with d > 0 comes out of these statements unchanged with a zero state (the kernel skips
its state traffic).  frame_min, indent and rows of hm' are `depth_pass_ref.reference_mm(hm')`.
"""
import math

import numpy as np

import depth_pass_ref as dref

F32 = np.float32
GELPAD_H, GELPAD_DMIN = dref.GELPAD_H, dref.GELPAD_DMIN
DT = 1.0 / 60.0


def rest_plane(gelpad_h=GELPAD_H, gelpad_dmin=GELPAD_DMIN):
    return F32((float(gelpad_dmin) + float(gelpad_h)) * 1000.0)


def coefficient_row(tau, weight, floor_mm, dt):
    """[a1, c1, a2, c2, floor_mm, 0, 0, 0] float32, computed in float64."""
    row = np.zeros(8, np.float64)
    for k in range(2):
        a = math.exp(-float(dt) / float(tau[k])) if tau[k] > 0 else 0.0
        row[2 * k], row[2 * k + 1] = a, (1.0 - a) * float(weight[k])
    row[4] = float(floor_mm)
    return row.astype(F32)


class GelMemoryRef:
    """State, map and live flags of B frames; `step(hm)` is one call of tacex_gel_memory."""

    def __init__(self, B, H, W, K, table, ids, z0=None):
        self.K, self.z0 = int(K), rest_plane() if z0 is None else F32(z0)
        self.table, self.ids = np.asarray(table, F32).reshape(-1, 8), np.asarray(ids, np.int64).reshape(B)
        self.state = np.zeros((B, self.K, H, W), F32)
        self.live = np.zeros((B,), np.int32)

    def reset(self, env_ids=None):
        sel = slice(None) if env_ids is None else list(env_ids)
        self.state[sel] = 0
        self.live[sel] = 0

    def imprint(self):
        return self.state[:, 0].copy() if self.K == 1 else (self.state[:, 0] + self.state[:, 1]).astype(F32)

    def step(self, hm):
        """-> hm' (a new array); state and live advance."""
        hm = np.asarray(hm, F32)
        out = np.empty_like(hm)
        z0 = self.z0
        for b in range(hm.shape[0]):
            i = self.ids[b]
            row = self.table[i] if 0 <= i < len(self.table) else np.zeros(8, F32)
            h = hm[b]
            with np.errstate(invalid="ignore"):
                t = (z0 - h).astype(F32)
                d = np.where(t > 0, t, F32(0)).astype(F32)
                ms = []
                for k in range(self.K):
                    a, c, floor = F32(row[2 * k]), F32(row[2 * k + 1]), F32(row[4])
                    m = ((a * self.state[b, k]).astype(F32) + (c * d).astype(F32)).astype(F32)
                    m[(d == 0) & (m < floor)] = 0
                    self.state[b, k] = m
                    ms.append(m)
                M = ms[0] if self.K == 1 else (ms[0] + ms[1]).astype(F32)
                r = (z0 - M).astype(F32)
                out[b] = np.where((M > 0) & (r < h), r, h)
            self.live[b] = int((self.state[b] != 0).any())
        return out


def outputs(hm):
    """frame_min, indent, true contact ranges of the rewritten map."""
    return dref.reference_mm(hm)


def closed_form(d0, weights, a, n, j):
    """Hold d0 for n steps, release for j: M = sum_k w_k d0 (1 - a_k^n) a_k^j, in float64 (a: the float32 coefficients, widened)."""
    return sum(float(w) * float(d0) * (1.0 - float(ak) ** n) * float(ak) ** j for w, ak in zip(weights, a))


# -- input sequences ------------------------------------------------------------------------------------------------------------------
# profiles of the tests (tau_s, weight, floor_mm): a slow two-branch gel, and a fast one whose state flushes to zero inside three release steps
PROFILES = [((0.05, 0.4), (0.5, 0.3), 1e-4), ((DT / 3.0, DT / 4.0), (0.6, 0.2), 1e-4)]
IDS = [0, 1, 7]  # frame 2: an id outside [0, P)


def table(dt=DT, profiles=PROFILES):
    return np.stack([coefficient_row(t, w, f, dt) for t, w, f in profiles])


def _deeper(m, by=0.2):
    return np.where(m < dref._FAR_MM, m - F32(by), m).astype(F32)


def sequence(H, W):
    """(6, 3, H, W) float32 height maps [mm]: press, deeper, slide sideways by three pixels, release, release, release.
    Frame 0: the sphere dent; frame 1: the corner pixel; frame 2: no contact, then the sphere dent from the slide step for one step."""
    s, c, n = dref.sphere_dent(H, W), dref.corner_pixel(H, W), dref.no_contact(H, W)
    steps = [
        [s, c, n],
        [_deeper(s), _deeper(c), n],
        [np.roll(_deeper(s), 3, axis=1), np.roll(_deeper(c), -3, axis=1), s],
        [n, n, n], [n, n, n], [n, n, n],
    ]
    return np.stack([np.stack(f) for f in steps]).astype(F32)
