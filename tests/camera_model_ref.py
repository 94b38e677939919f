"""NumPy restatement of the sensor camera model's contract (include/tacex_hip.h, `tacex_camera_model`): the Philox-addressed integer
draws and the per-pixel float32 arithmetic, every operation rounded on its own in the order the header writes.  Written from that
comment, not from the kernel: the tests compare the two bit for bit."""
import numpy as np
from marker_pattern_ref import philox4x32

F = np.float32
S = F(1.0 / np.sqrt(21845.0))
IDENTITY_ROW = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1] + [0] * 7, dtype=np.float32)


def profile_row(color_matrix=None, offset=0.0, read_noise=0.0, shot_noise=0.0, fixed_pattern=0.0):
    m = np.eye(3, dtype=np.float32) if color_matrix is None else np.asarray(color_matrix, dtype=np.float32)
    o = np.broadcast_to(np.asarray(offset, dtype=np.float32), (3,))
    return np.concatenate([m.reshape(9), o, np.array([read_noise, shot_noise, fixed_pattern, 0.0], dtype=np.float32)]).astype(np.float32)


def group_draws(seed, frame, call, groups, fixed_pattern=False):
    """(G,12) int32: draw j of every group in `groups` = byte sum of word j % 4 of Philox(counter (g, j / 4 [+ 4], frame, call [0])) - 510."""
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    g = np.asarray(groups, dtype=np.uint64).reshape(-1)
    out = np.empty((g.size, 12), dtype=np.int32)
    for q in range(3):
        stream = np.full_like(g, 4 + q if fixed_pattern else q)
        ctr = np.stack([g, stream, np.full_like(g, int(frame) & 0xFFFFFFFF), np.full_like(g, 0 if fixed_pattern else int(call))], -1)
        w = philox4x32(ctr, key).astype(np.uint32)  # (G,4)
        bsum = (w & 0xFF) + ((w >> 8) & 0xFF) + ((w >> 16) & 0xFF) + (w >> 24)
        out[:, 4 * q:4 * q + 4] = bsum.astype(np.int32) - 510
    return out


def frame_draws(seed, frame, call, npix, fixed_pattern=False):
    """(npix,3) int32 draws of one frame's pixels, row-major."""
    G = (npix + 3) // 4
    return group_draws(seed, frame, call, np.arange(G), fixed_pattern).reshape(G * 4, 3)[:npix]


def camera_frame(rgb, row, seed, frame, call, u8):
    """One frame (H,W,3) float32 under profile row (16,) -> (H,W,3) float32 in [0,1] or uint8."""
    H, W, _ = rgb.shape
    x = np.ascontiguousarray(rgb, dtype=np.float32).reshape(H * W, 3)
    row = np.asarray(row, dtype=np.float32)
    M, o, read, s, sf = row[:9].reshape(3, 3), row[9:12], row[12], row[13], row[14]
    d = frame_draws(seed, frame, call, H * W).astype(np.float32)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    out = np.empty_like(x)
    if sf != 0:
        df = frame_draws(seed, frame, 0, H * W, fixed_pattern=True).astype(np.float32)
        fs = F(sf * S)
    rr = F(read * read)
    for c in range(3):
        a = ((M[c, 0] * r + M[c, 1] * g) + M[c, 2] * b) + o[c]
        if sf != 0:
            a = a * (F(1) + fs * df[:, c])
        a = np.minimum(np.maximum(a, F(0)), F(1))
        sig = np.sqrt(rr + s * a)
        v = a + (sig * S) * d[:, c]
        out[:, c] = np.minimum(np.maximum(v, F(0)), F(1))
    assert out.dtype == np.float32
    out = out.reshape(H, W, 3)
    return np.floor(F(255) * out + F(0.5)).astype(np.uint8) if u8 else out


def camera_batch(rgb, profiles, ids, seed, call, u8, frame_offset=0):
    """rgb (B,H,W,3), profiles (P,16), ids (B,) or None -> (B,H,W,3); an id outside [0, P) is the identity profile."""
    profiles = np.asarray(profiles, dtype=np.float32).reshape(-1, 16)
    out = []
    for b in range(rgb.shape[0]):
        i = 0 if ids is None else int(ids[b])
        row = profiles[i] if 0 <= i < profiles.shape[0] else IDENTITY_ROW
        out.append(camera_frame(rgb[b], row, seed, frame_offset + b, call, u8))
    return np.stack(out)
