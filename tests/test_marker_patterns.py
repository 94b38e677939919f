"""Marker pattern library, the parts that need no GPU: the Philox4x32-10 generator (the C entry runs the function the kernel calls), the
header / binding / export agreement at ABI 20, the C ABI's argument checks that return before any device call, host validation of pattern
ids, the cfg fields, and the library's construction on the test pad (deterministic in the seed; the counts the GPU tests rely on)."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

from marker_pattern_ref import box_muller, draws, flow_one_env, philox4x32, uniform

# Random123's known answers for philox4x32_10 (kat_vectors): counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
RANGES = dict(marker_interval_range=(1.95, 2.15), marker_rotation_range=0.1, marker_translation_range=(1.0, 1.0),
              marker_pos_shift_range=(0.1, 0.1))


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers_in_the_library_and_in_the_restatement(ctr, key, want):
    from tacex_amd import _lib

    lib = _lib.load_library()
    out = (C.c_uint32 * 4)()
    assert lib.tacex_philox4x32((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
    assert tuple(out) == want
    assert tuple(int(v) for v in philox4x32(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))) == want
    assert lib.tacex_philox4x32(None, (C.c_uint32 * 2)(*key), out) == 2 and b"tacex_philox4x32" in lib.tacex_last_error()


def test_library_and_restatement_agree_on_the_counters_the_kernel_uses():
    """(m, stream, e, t) with a 64-bit seed split into the key: a batch of them, word for word."""
    from tacex_amd import _lib

    lib = _lib.load_library()
    seed = 0x123456789abcdef
    key = (seed & 0xffffffff, seed >> 32)
    ctrs = np.array([(m, s, e, t) for m in (0, 1, 1023) for s in (0, 1) for e in (0, 7, 511) for t in (0, 1, 0xffffffff)], dtype=np.uint32)
    ref = philox4x32(ctrs, np.array(key, dtype=np.uint32))
    for c, r in zip(ctrs, ref):
        out = (C.c_uint32 * 4)()
        assert lib.tacex_philox4x32((C.c_uint32 * 4)(*(int(v) for v in c)), (C.c_uint32 * 2)(*key), out) == 0
        assert tuple(out) == tuple(int(v) for v in r)
    # the uniform never reaches 0 or 1, and Box-Muller of the extreme words is finite
    lo, hi = uniform(np.uint32(0)), uniform(np.uint32(0xffffffff))
    assert 0.0 < lo == 0.5 * 2.0 ** -32 and hi == 1.0 - 0.5 * 2.0 ** -32 < 1.0
    assert all(np.isfinite(v) for v in box_muller(lo, hi) + box_muller(hi, lo))
    U, k, N = draws(seed, 3, 9, 64)
    assert U.shape == (64,) and k.dtype == np.uint32 and N.shape == (64, 4) and np.isfinite(N).all()


def test_header_binding_and_exports_agree_at_abi_20():
    from conftest import REPO
    from tacex_amd import _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    lib = _lib.load_library()
    assert int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == lib.tacex_abi_version() == 20
    for name in ("tacex_fem_marker_flow_library", "tacex_philox4x32"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name not in _lib.MISSING_SYMBOLS
    # one ctypes argument per parameter the header declares
    decl = re.search(r"\bint\s+tacex_fem_marker_flow_library\s*\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["tacex_fem_marker_flow_library"][1]) == 31
    assert _lib.SIGNATURES["tacex_fem_marker_flow_library"][1][12] is C.c_uint64  # the seed


def _call(lib, P=1, Mmax=8, prob=0.0, sigma=0.0, null=None, B=1, K=4):
    """tacex_fem_marker_flow_library with dummy non-null HOST pointers: every case here must return before any HIP call."""
    buf = np.zeros(64)
    a = [buf.ctypes.data] * 12
    args = [a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], P, Mmax, a[8], a[9], 0, 340.0, 325.0, 160.0, 125.0, prob, sigma, 240, 320, 0.0,
            a[10], a[11], None, None, B, 10, 5, K, None]
    if null is not None:
        args[null] = None
    return lib.tacex_fem_marker_flow_library(*args)


def test_argument_errors_return_2_with_a_message_before_any_device_call():
    from tacex_amd import _lib

    lib = _lib.load_library()
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11):  # x, surf_ids, cam_pos, cam_rot_inv, ref surface, tri, weights, count, pattern_ids, draws
        assert _call(lib, null=i) == 2 and b"null argument" in lib.tacex_last_error(), i
    assert _call(lib, null=23) == 2 and b"null argument" in lib.tacex_last_error()  # neither flow output
    assert _call(lib, Mmax=1025) == 2 and b"1025 markers" in lib.tacex_last_error() and b"LDS" in lib.tacex_last_error()
    assert _call(lib, Mmax=0) == 2 and b"0 markers" in lib.tacex_last_error()
    assert _call(lib, P=0) == 2 and b"0 patterns" in lib.tacex_last_error()
    for bad in (-0.01, 1.5, float("nan")):
        assert _call(lib, prob=bad) == 2 and b"probability" in lib.tacex_last_error()
    for bad in (-1e-9, float("nan")):
        assert _call(lib, sigma=bad) == 2 and b"sigma" in lib.tacex_last_error()
    assert _call(lib, B=0) == 0 and _call(lib, K=0) == 0  # nothing to do: no launch


def test_pattern_id_validation_is_host_side():
    from tacex_amd.simulation_approaches.fem_based.sim.tactile_sensor_uipc import VisionTactileSensorUIPC, check_pattern_ids

    assert check_pattern_ids(None, 5, 3).tolist() == [0, 1, 2, 0, 1] and check_pattern_ids([2, 0, 1], 3, 3).dtype == np.int32
    for bad in ([0, 1], [0, 1, 3], [0, -1, 0], [0.0, 1.0, 0.0]):
        with pytest.raises(ValueError):
            check_pattern_ids(bad, 3, 3)
    # the setter goes through it before it touches the device tensor
    stub = SimpleNamespace(patterns=SimpleNamespace(num_patterns=2), pattern_ids=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="outside the library"):
        VisionTactileSensorUIPC.set_pattern_ids(stub, [0, 2, 1])
    with pytest.raises(RuntimeError):
        VisionTactileSensorUIPC.set_pattern_ids(SimpleNamespace(patterns=None), [0])


def test_cfg_carries_the_library_fields():
    from tacex_amd.simulation_approaches.fem_based import ManiSkillSimulatorCfg

    c = ManiSkillSimulatorCfg()
    assert (c.marker_patterns, c.marker_seed) == (0, 0)
    assert ManiSkillSimulatorCfg(marker_patterns=4, marker_seed=7).marker_patterns == 4


def _test_pad():
    from tacex_amd.uipc.uipc_object import UipcObject, gelpad_box_mesh

    P, Tt = gelpad_box_mesh(10, 8, 3, size=(0.030, 0.018, 0.0045))
    P = P - np.array([0.011, 0.009, 0.0])
    tri_global = UipcObject.surface_triangles(SimpleNamespace(tets=Tt))
    surf = np.unique(tri_global.reshape(-1))
    remap = -np.ones(len(P), dtype=np.int64)
    remap[surf] = np.arange(len(surf))
    return P[surf] - np.array([0.0, 0.0, -0.024]), remap[tri_global].astype(np.int32)  # surface in the camera frame, local triangles


def test_library_construction_is_deterministic_in_the_seed_and_has_the_counts_the_gpu_tests_use():
    from oracle.fem_oracle import marker_uv
    from tacex_amd.simulation_approaches.fem_based.sim.tactile_sensor_uipc import (build_marker_patterns, gen_marker_grid,
                                                                                    gen_marker_weight)

    surf, tris = _test_pad()
    assert surf.shape == (270, 3)
    a = build_marker_patterns(8, surf, tris, rng=np.random.RandomState(0), **RANGES)
    b = build_marker_patterns(8, surf, tris, rng=np.random.RandomState(0), **RANGES)
    c = build_marker_patterns(8, surf, tris, rng=np.random.RandomState(1), **RANGES)
    assert all(np.array_equal(x, y) for x, y in ((a.tri, b.tri), (a.wgt, b.wgt), (a.count, b.count)))
    assert not np.array_equal(a.wgt, c.wgt)
    assert a.tri.dtype == np.int32 and a.wgt.dtype == np.float64 and a.count.dtype == np.int32
    assert a.num_patterns == 8 and a.max_markers == a.count.max() and a.tri.shape == a.wgt.shape == (8, a.max_markers, 3)
    assert 91 <= a.count.min() and a.count.max() <= 120
    # pattern k is the k-th draw from the ONE RandomState, in order; padding rows are zero
    rng = np.random.RandomState(0)
    for k in range(8):
        idx, wgt = gen_marker_weight(gen_marker_grid(rng=rng, **RANGES), surf, tris)
        n = a.count[k]
        assert n == idx.shape[0] and np.array_equal(a.tri[k, :n], idx) and np.array_equal(a.wgt[k, :n], wgt)
        assert not a.tri[k, n:].any() and not a.wgt[k, n:].any()
    # in-image markers per pattern at rest: with K = 60 both the padding and the subset branch occur
    uv = [marker_uv(surf[None], a.tri[k, :a.count[k]], a.wgt[k, :a.count[k]])[0] for k in range(8)]
    inimg = [int(((u[:, 0] > 5) & (u[:, 0] < 240) & (u[:, 1] > 5) & (u[:, 1] < 320)).sum()) for u in uv]
    assert inimg == [56, 69, 64, 64, 56, 64, 56, 71]
    # a library of one from degenerate ranges is the static grid
    one = build_marker_patterns(1, surf, tris, rng=np.random.RandomState(3))
    idx, wgt = gen_marker_weight(gen_marker_grid(), surf, tris)
    assert np.array_equal(one.tri[0], idx) and np.array_equal(one.wgt[0], wgt)
    with pytest.raises(ValueError, match="at least one"):
        build_marker_patterns(0, surf, tris)
    with pytest.raises(ValueError, match="1024"):  # a 0.5 mm grid: thousands of markers over the pad
        build_marker_patterns(1, surf, tris, marker_interval_range=(0.5, 0.5))


def test_restatement_selection_branches():
    """The restatement itself on a hand-made env: subset = the K smallest (key, m) in that order, padding repeats the last survivor, nothing
    left gives zeros (-1 normalised), and the mask keeps the reference's axis swap."""
    M = 12
    init = np.stack([np.linspace(10, 200, M), np.linspace(20, 300, M)], 1)
    init[0] = (3.0, 50.0)     # u <= 5: out
    init[1] = (239.5, 319.5)  # just inside
    init[2] = (240.0, 100.0)  # u == H: out (u is compared with the HEIGHT)
    curr = init + 1.0
    U, key, _ = draws(11, 2, 5, M)
    alive = np.array([False, True, False] + [True] * (M - 3))
    f, n, ch = flow_one_env(init, curr, 11, 2, 5, 0.0, 0.0, 240, 320, 4)
    surv = np.where(alive)[0]
    assert n == surv.size == 10
    assert ch.tolist() == sorted(surv.tolist(), key=lambda m: (int(key[m]), m))[:4]
    assert np.array_equal(f[0], init[ch]) and np.array_equal(f[1], curr[ch])
    f, n, ch = flow_one_env(init, curr, 11, 2, 5, 0.0, 0.0, 240, 320, 16)
    assert ch.tolist() == surv.tolist() + [surv[-1]] * 6 and np.array_equal(f[1, 10:], np.repeat(curr[surv[-1:]], 6, 0))
    f, n, ch = flow_one_env(init, curr, 11, 2, 5, 1.0, 0.5, 240, 320, 4, normalize_div=160.0)
    assert n == 0 and (ch == -1).all() and (f == -1.0).all()
    f, n, ch = flow_one_env(init, curr, 11, 2, 5, 0.5, 0.0, 240, 320, 16)
    assert n == int((alive & (U > 0.5)).sum())
