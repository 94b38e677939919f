"""NumPy restatement of the marker pattern library's per-launch semantics (include/tacex_hip.h, `tacex_fem_marker_flow_library`):
Philox4x32-10, the uniforms and Box-Muller normals drawn from it, and mask / lost tracking / noise / selection for ONE env.
Written from the contract, not from the kernel: the tests compare the two."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # Random123 Philox4x32 multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # key increments
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32(ctr, key):
    """ctr (...,4), key (2,) or (...,2) of uint32 -> (...,4) uint32; ten rounds."""
    c = np.asarray(ctr, dtype=np.uint64) & MASK32
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64) & MASK32, c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def uniform(w):
    return (np.asarray(w, dtype=np.float64) + 0.5) * 2.0 ** -32


def box_muller(a, b):
    r = np.sqrt(-2.0 * np.log(a))
    return r * np.cos(2 * np.pi * b), r * np.sin(2 * np.pi * b)


def draws(seed, env, t, num_markers):
    """(U (M,), subset key (M,) uint32, normals (M,4): init u, init v, current u, current v) of draw `t` of env `env`."""
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    m = np.arange(num_markers, dtype=np.uint64)
    ctr = lambda stream: np.stack([m, np.full_like(m, stream), np.full_like(m, env), np.full_like(m, t)], -1)  # noqa: E731
    r0, r1 = philox4x32(ctr(0), key), philox4x32(ctr(1), key)
    n0, n1 = box_muller(uniform(r1[:, 0]), uniform(r1[:, 1]))
    n2, n3 = box_muller(uniform(r1[:, 2]), uniform(r1[:, 3]))
    return uniform(r0[:, 0]), r0[:, 1], np.stack([n0, n1, n2, n3], -1)


def flow_one_env(init_uv, curr_uv, seed, env, t, prob, sigma, height, width, K, normalize_div=0.0):
    """init_uv, curr_uv (M,2) projections of the env's pattern (the `count` real rows only).
    -> flow (2,K,2), number of survivors, chosen (K,) marker id per slot (-1: none)."""
    M = init_uv.shape[0]
    U, key, N = draws(seed, env, t, M)
    u0, v0 = init_uv[:, 0], init_uv[:, 1]
    alive = (u0 > 5) & (u0 < height) & (v0 > 5) & (v0 < width) & (U > prob)
    val = np.concatenate([init_uv, curr_uv], 1) + sigma * N  # (M,4)
    surv = np.where(alive)[0]
    n = surv.size
    chosen = np.full(K, -1, dtype=np.int64)
    if n >= K:
        order = np.lexsort((surv, key[surv]))  # ascending (key, m)
        chosen[:] = surv[order[:K]]
    elif n > 0:
        chosen[:n] = surv
        chosen[n:] = surv[-1]
    flow = np.zeros((2, K, 2))
    if n > 0:
        flow[0], flow[1] = val[chosen, :2], val[chosen, 2:]
    if normalize_div > 0:
        flow = flow / normalize_div - 1.0
    return flow, n, chosen


def flow_batch(init_uv, curr_uv, counts, pattern_ids, seed, t, prob, sigma, height, width, K, normalize_div=0.0, envs=None):
    """init_uv / curr_uv (B,Mmax,2) per env on its OWN pattern, counts (P,), pattern_ids (B,), t (B,) -> flow (B,2,K,2), n (B,), chosen (B,K)."""
    B = init_uv.shape[0]
    envs = range(B) if envs is None else envs
    out = [flow_one_env(init_uv[i, :counts[pattern_ids[i]]], curr_uv[i, :counts[pattern_ids[i]]], seed, e, int(t[i]), prob, sigma, height,
                        width, K, normalize_div) for i, e in enumerate(envs)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.stack([o[2] for o in out])
