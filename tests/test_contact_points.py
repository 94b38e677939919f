"""Contact point cloud on the CPU: the NumPy restatement (tests/contact_points_ref.py) against brute force - ranks, the slot map and
its inverse, the valid count and the invalid fill -, its contact count against the contact field's, the Philox offset against the
library's host generator, the ABI (symbol, refusals before any GPU call) and the Python layer's argument checks."""
import ctypes as C
import re

import numpy as np
import pytest
from conftest import REPO
import contact_points_ref as R
from contact_field_ref import GELS, case_batch, case_pixmm, contact_frame, indentation_depth

NARGS = 26


def _lib_and_module():
    from tacex_amd import _lib

    return _lib.load_library(), _lib


# ---- the restatement against brute force ---------------------------------------------------------------------------------------------
def test_ranks_follow_nonzero_order_and_the_fill_of_invalid_slots():
    rng = np.random.default_rng(3)
    H, W, K = 9, 13, 20
    hm, fmin, ind = R.flat_frames(1, H, W)
    lin = np.sort(rng.choice(H * W, 11, replace=False))
    R.press(hm, 0, lin)
    for pad in (0, 1):
        out = R.points_frame(hm[0], fmin[0], ind[0], 0.03, K, pad=pad)
        assert out["count"].tolist() == [11, K if pad else 11]
        pix = out["pixels"]
        want = np.stack([lin // W, lin % W], -1)
        assert np.array_equal(pix[:11], want)  # rank r = the r-th pixel of np.nonzero
        if pad:
            assert np.array_equal(pix, want[np.arange(K) % 11]) and (out["labels"] == 0).all()
        else:
            assert (pix[11:] == -1).all() and (out["labels"][11:] == 255).all() and (out["labels"][:11] == 0).all()
            assert not out["points"][11:].any() and not out["normals"][11:].any() and not out["depth"][11:].any()
        assert (out["depth"][:11] > 0).all() and np.array_equal(out["points"][:11, 2], -out["depth"][:11])
        nrm = np.linalg.norm(out["normals"][:11].astype(np.float64), axis=1)
        assert np.abs(nrm - 1).max() < 1e-6 and (out["normals"][:11, 2] < 0).all()
    # x, y: the pixel centre from the image centre, in mm
    out = R.points_frame(hm[0], fmin[0], ind[0], 0.03, K)
    np.testing.assert_allclose(out["points"][:11, 0], (lin % W - (W - 1) / 2) * 0.03, rtol=1e-6)
    np.testing.assert_allclose(out["points"][:11, 1], (lin // W - (H - 1) / 2) * 0.03, rtol=1e-6)


def test_slot_map_and_its_inverse_for_every_small_n_and_k():
    """N in 1..70, K in 1..40, o in {0, 1, N // 2, N - 1}: for N > K the slot map is strictly increasing and below N, and the inverse
    range formula names exactly the slot map's sources; V and the invalid slots in every N / K / pad combination."""
    for N in range(0, 71):
        for K in range(1, 41):
            for pad in (0, 1):
                ranks, V = R.slot_ranks(N, K, pad, 0)
                assert V == (0 if N == 0 else K if (N >= K or pad) else N)
                assert int((ranks >= 0).sum()) == V and (ranks[:V] >= 0).all()
                if 0 < N <= K:
                    assert np.array_equal(ranks[:V], np.arange(V) % N)
            if N <= K:
                continue
            for o in sorted({0, 1, N // 2, N - 1}):
                ranks, V = R.slot_ranks(N, K, 0, o)
                assert V == K and (np.diff(ranks) > 0).all() and ranks[0] >= 0 and ranks[-1] < N, (N, K, o)
                source_of = {}
                for r in range(N):
                    lo, hi = R.inverse_slot_range(r, N, K, o)
                    assert 0 <= hi - lo <= 1 and 0 <= lo and hi <= K, (N, K, o, r)
                    for k in range(lo, hi):
                        source_of[k] = r
                assert [source_of[k] for k in range(K)] == ranks.tolist(), (N, K, o)


def test_slot_map_does_not_overflow_at_the_largest_sizes():
    N, K = 2 ** 31 - 1, 16384
    ranks, V = R.slot_ranks(N, K, 0, N - 1)
    assert V == K and ranks[-1] == ((K - 1) * N + N - 1) // K < N and (np.diff(ranks) > 0).all()


def test_contact_count_is_the_contact_fields():
    H, W = 24, 32
    hm, kinds = case_batch(H, W, 10)
    fmin, ind = indentation_depth(hm)
    out = R.points_batch(hm, fmin, ind, case_pixmm(H), 64)
    for b, kind in enumerate(kinds):
        rec, _, _, _ = contact_frame(hm[b], fmin[b], ind[b], GELS[0], None, case_pixmm(H))
        assert out["count"][b, 0] == rec[8], kind
    assert (out["count"][:, 0] > 64).any() and (out["count"][:, 0] == 0).any()


def test_labels_filter_and_min_depth():
    H, W = 8, 8
    hm, fmin, ind = R.flat_frames(1, H, W)
    R.press(hm, 0, np.arange(16, 48))
    labels = np.zeros((H, W), np.uint8)
    labels[:, 4:] = 3
    labels[3, :] = 255
    every = R.points_frame(hm[0], fmin[0], ind[0], 0.03, 64, labels=labels)
    assert every["count"][0] == 32 and set(every["labels"][:32].tolist()) == {0, 3, 255}
    parts = [R.points_frame(hm[0], fmin[0], ind[0], 0.03, 64, labels=labels, label=l) for l in (0, 3)]
    assert [p["count"][0] for p in parts] == [12, 12]
    assert all((p["labels"][:12] == l).all() for p, l in zip(parts, (0, 3)))
    deep = R.points_frame(hm[0], fmin[0], ind[0], 0.03, 64, min_depth_mm=0.3)
    assert 0 < deep["count"][0] < 32 and (deep["depth"][:deep["count"][0]] > np.float32(0.3)).all()


def test_offset_matches_the_host_philox():
    lib, _ = _lib_and_module()
    u32x4, u32x2 = C.c_uint32 * 4, C.c_uint32 * 2
    for seed, g, call, N in [(0, 0, 0, 1000), (0x1234567890ABCDEF, 5, 7, 76800), (2 ** 64 - 1, -3, 2 ** 32 - 1, 2 ** 31 - 1), (9, 2 ** 40 + 17, 3, 12345)]:
        gu = g & (2 ** 64 - 1)
        out = u32x4()
        assert lib.tacex_philox4x32(u32x4(gu & 0xFFFFFFFF, gu >> 32, call, R.TAG), u32x2(seed & 0xFFFFFFFF, seed >> 32), out) == 0
        o = R.jitter_offset(seed, g, call, N)
        assert o == (out[0] * N) >> 32 and 0 <= o < N
    offs = {R.jitter_offset(11, g, c, 5000) for g in range(8) for c in range(4)}
    assert len(offs) > 24  # the offset moves with env and call


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbol_declared_exported_and_bound():
    lib, _lib = _lib_and_module()
    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"tacex_contact_points\s*\(([^)]*)\)", txt)
    assert decl, "tacex_contact_points is not declared in include/tacex_hip.h"
    assert hasattr(lib, "tacex_contact_points") and "tacex_contact_points" in _lib.SIGNATURES
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["tacex_contact_points"][1]) == NARGS
    assert int(re.search(r"#define\s+TACEX_CONTACT_POINTS_MAX\s+(\d+)", hdr).group(1)) == 16384
    assert lib.tacex_abi_version() == int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_the_translation_unit_is_built_without_fp_contraction():
    from tacex_amd import _build

    assert "contact_points.hip" in _build.SOURCES and (REPO / "tacex_amd" / "csrc" / "contact_points.hip").exists()
    assert "-ffp-contract=off" in _build.FILE_FLAGS["contact_points.hip"]


def test_exported_from_the_package():
    import tacex_amd

    assert {"ContactPoints", "TactileContactPoints"} <= set(tacex_amd.__all__)
    assert tacex_amd.TactileContactPoints.__module__ == "tacex_amd.contact_points"
    assert hasattr(tacex_amd.GelSightSensor, "contact_points") and hasattr(tacex_amd.GelSightSensor, "contact_field")
    for name in ("num_contact", "num_valid", "valid"):
        assert isinstance(getattr(tacex_amd.ContactPoints, name), property), name


# arguments of a valid call (the pointers are never dereferenced: every case below is refused before any GPU call)
_OK = dict(hm=0x1000, fmin=0x2000, ind=0x3000, rects=None, labels=None, label=-1, pixmm=0.03, mind=0.0, K=8, pad=0, pose=None, unit=1.0, jitter=0,
           seed=0, off=0, call=0, pts=0x4000, nrm=None, dep=None, pix=None, lab=None, cnt=None, B=1, H=4, W=8)
NAN = float("nan")


@pytest.mark.parametrize("change, word", [
    (dict(hm=None), b"hm_mm_dev"), (dict(fmin=None), b"frame_min_dev"), (dict(ind=None), b"indent_mm_dev"), (dict(pts=None), b"points_dev"),
    (dict(B=0), b"num_frames"), (dict(B=-1), b"num_frames"), (dict(H=0), b"height"), (dict(W=0), b"width"), (dict(W=-5), b"width"),
    (dict(H=65536, W=32768), b"exceeds"),
    (dict(pixmm=0.0), b"pixmm"), (dict(pixmm=-0.03), b"pixmm"), (dict(pixmm=NAN), b"pixmm"),
    (dict(unit=0.0), b"unit"), (dict(unit=-1.0), b"unit"), (dict(unit=NAN), b"unit"),
    (dict(mind=-0.1), b"min_depth_mm"), (dict(mind=NAN), b"min_depth_mm"),
    (dict(K=0), b"max_points"), (dict(K=-3), b"max_points"), (dict(K=16385), b"max_points"),
    (dict(pad=2), b"pad"), (dict(pad=-1), b"pad"),
    (dict(label=-2), b"label"), (dict(label=255), b"label"), (dict(label=255, labels=0x7000), b"label"),
    (dict(label=0), b"labels_dev"), (dict(label=254), b"labels_dev"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_refusals_return_2_and_name_the_argument(change, word):
    lib, _lib = _lib_and_module()
    a = dict(_OK, **change)
    rc = lib.tacex_contact_points(a["hm"], a["fmin"], a["ind"], a["rects"], a["labels"], a["label"], a["pixmm"], a["mind"], a["K"], a["pad"], a["pose"],
                                  a["unit"], a["jitter"], a["seed"], a["off"], a["call"], a["pts"], a["nrm"], a["dep"], a["pix"], a["lab"], a["cnt"],
                                  a["B"], a["H"], a["W"], None)
    assert rc == 2
    msg = lib.tacex_last_error()
    assert b"tacex_contact_points" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "tacex_contact_points")


def test_python_value_errors_come_before_the_device_is_looked_at():
    from tacex_amd import TactileContactPoints
    from tacex_amd._lib import TacexHipError

    dev = "cuda:99"  # never looked at
    for bad in (dict(num_frames=0), dict(num_frames=-2), dict(max_points=0), dict(max_points=16385), dict(pixmm=0.0), dict(pixmm=NAN),
                dict(min_depth_mm=-1e-3), dict(min_depth_mm=NAN), dict(pad="wrap"), dict(pad=1), dict(unit=0.0), dict(unit=float("inf")),
                dict(seed=-1), dict(seed=2 ** 64), dict(frame_offset=2 ** 63), dict(frame_offset=-2 ** 63 - 1)):
        kw = dict(dict(num_frames=2), **bad)
        with pytest.raises(ValueError):
            TactileContactPoints(device=dev, **kw)
    with pytest.raises(TacexHipError):  # no CPU path
        TactileContactPoints(2, "cpu")
