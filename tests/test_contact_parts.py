"""Per-part contact records on the CPU: the NumPy restatement of `tacex_contact_field_parts` (tests/contact_parts_ref.py) against the
restatement of `tacex_contact_field` - one label is the whole frame, the labels' plain sums add up to it, a label >= L enters nothing,
a label's record does not see another label's slip -, the C ABI's argument checks (no GPU call is made) and the Python layer's."""
import ctypes as C
import re

import numpy as np
import pytest
import contact_field_ref as R
import contact_parts_ref as P
from conftest import REPO

f32 = np.float32
NAME = "tacex_contact_field_parts"
PLAIN_SUMS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13)


def _frames(H, W, B, start):
    hm, kinds = R.case_batch(H, W, B, start)
    fmin, ind = R.indentation_depth(hm)
    return hm, fmin, ind, kinds


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("H, W, start", [(24, 32, 0), (37, 53, 5)])
def test_one_label_is_the_whole_frame(H, W, start):
    B = 5
    hm, fmin, ind, kinds = _frames(H, W, B, start)
    slip = R.case_slip(B, H, W, start)
    labels = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        gel = R.GELS[b % 3]
        want_rec, _, want_img, _ = R.contact_frame(hm[b], fmin[b], ind[b], gel, slip[b], R.case_pixmm(H))
        rec, img, _ = P.parts_frame(hm[b], fmin[b], ind[b], gel, labels[b], 1, slip[b:b + 1], R.case_pixmm(H))
        assert np.array_equal(_bits(rec[0]), _bits(want_rec)) and np.array_equal(_bits(img), _bits(want_img)), (b, kinds[b])


@pytest.mark.parametrize("kind", ["halves", "checker"])
@pytest.mark.parametrize("L", [2, 3, 8])
def test_with_one_slip_row_the_labels_add_up_to_the_frame(kind, L):
    H, W, B, start = 37, 53, 5, 0
    hm, fmin, ind, kinds = _frames(H, W, B, start)
    slip = R.case_slip(B, H, W, start)
    labels = P.case_labels(kind, hm, fmin, ind, L)
    assert (labels < L).all()
    split = 0
    for b in range(B):
        gel = R.GELS[b % 3]
        want_rec, _, want_img, ab = R.contact_frame(hm[b], fmin[b], ind[b], gel, slip[b], R.case_pixmm(H))
        rec, img, _ = P.parts_frame(hm[b], fmin[b], ind[b], gel, labels[b], L, np.repeat(slip[b:b + 1], L, 0), R.case_pixmm(H))
        for k in PLAIN_SUMS:
            assert abs(rec[:, k].sum() - want_rec[k]) <= 1e-12 * ab[k], (b, k, rec[:, k].sum(), want_rec[k])
        assert rec[:, 11].max() == want_rec[11]
        assert np.array_equal(_bits(img), _bits(want_img))
        split += int((rec[:, 8] > 0).sum() >= 2)
    assert split >= 3, "the label maps do not split the contact patches"


def test_a_label_outside_enters_no_record_and_gets_no_shear():
    H, W, B, L = 48, 64, 4, 2  # (sphere, cylinder, edge, two spheres: each patch holds 20 pixels of either sort and more)
    hm, fmin, ind, kinds = _frames(H, W, B, 0)
    slip = P.case_part_slip(B, L, H, W)
    labels = P.case_labels("some_255", hm, fmin, ind, L)
    for b in range(B):
        gel = R.GELS[0]
        rec, img, _ = P.parts_frame(hm[b], fmin[b], ind[b], gel, labels[b], L, slip[b], R.case_pixmm(H))
        px = R.contact_pixels(hm[b], fmin[b], ind[b], gel, None, R.case_pixmm(H))
        out = labels[b] >= L
        assert (out & px["on"]).sum() >= 20 and (~out & px["on"]).sum() >= 20, kinds[b]
        assert rec[:, 8].sum() == (~out & px["on"]).sum()
        assert not img[out][:, :2].any() and np.array_equal(img[out][:, 2], np.where(px["on"], -px["p"], f32(0))[out])
        assert img[~out & px["on"]][:, :2].any()
        # the same frame with those pixels lifted out of contact: the same records
        lifted = np.where(out, f32(R.FAR_CLIP_MM), hm[b])
        rec2, _, _ = P.parts_frame(lifted, fmin[b], ind[b], gel, labels[b], L, slip[b], R.case_pixmm(H))
        assert np.array_equal(_bits(rec), _bits(rec2))


def test_a_labels_slip_is_its_own():
    H, W, B, L = 24, 32, 2, 2
    hm, fmin, ind, kinds = _frames(H, W, B, 0)
    slip = P.case_part_slip(B, L, H, W)
    other = slip.copy()
    other[:, 1] = [0.5, -0.4, 0.3, 3.0, 4.0]
    labels = P.case_labels("halves", hm, fmin, ind, L)
    a = P.parts_batch(hm, fmin, ind, R.GELS, [0, 1], labels, L, slip, R.case_pixmm(H))
    b = P.parts_batch(hm, fmin, ind, R.GELS, [0, 1], labels, L, other, R.case_pixmm(H))
    assert np.array_equal(_bits(a[0][:, 0]), _bits(b[0][:, 0])) and not np.array_equal(a[0][:, 1, :2], b[0][:, 1, :2])
    assert np.array_equal(_bits(a[1][labels == 0]), _bits(b[1][labels == 0]))
    assert (a[0][:, :, 8] > 0).all()


# ---- ABI and Python layer -------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_exports():
    from tacex_amd import _build, _lib

    hdr = (REPO / "include" / "tacex_hip.h").read_text()
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", hdr).group(1)
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 17 == len(decl.split(","))
    for want, text in zip(args, decl.split(",")):
        assert want is (C.c_void_p if "*" in text else C.c_int if re.search(r"\bint\b", text) else C.c_float), text
    assert hasattr(_lib.load_library(), NAME)
    assert int(re.search(r"#define\s+TACEX_ABI_VERSION\s+(\d+)", hdr).group(1)) == _lib.ABI_VERSION == 20
    assert "contact_parts.hip" in _build.SOURCES and "-ffp-contract=off" in _build.FILE_FLAGS["contact_parts.hip"]
    # one copy of the pixel's terms and of the record's reduction: both units include it, neither defines them
    assert (_build.CSRC / "contact_terms.h").exists()
    for unit in ("contact_field.hip", "contact_parts.hip"):
        text = (_build.CSRC / unit).read_text()
        assert '#include "contact_terms.h"' in text and "ContactPixel contact_pixel(" not in text and "atan2" not in text, unit


def test_the_entry_point_refuses_before_any_gpu_call():
    from tacex_amd import _lib

    lib = _lib.load_library()
    rec, img = np.full((2, 3, 16), -5.0), np.full((2, 8, 12, 3), -3.0, f32)
    one = 16
    good = dict(hm=one, fmin=one, ind=one, gels=one, P=1, ids=one, labels=one, L=3, slip=one, pix=0.0295, rows=one, rec=rec.ctypes.data,
                img=img.ctypes.data, B=2, H=8, W=12)

    def call(**kw):
        a = good | kw
        return getattr(lib, NAME)(a["hm"], a["fmin"], a["ind"], a["gels"], a["P"], a["ids"], a["labels"], a["L"], a["slip"], a["pix"], a["rows"],
                                  a["rec"], a["img"], a["B"], a["H"], a["W"], 0)

    cases = [(dict(hm=0), "null hm_mm_dev"), (dict(fmin=0), "null frame_min_dev"), (dict(ind=0), "null indent_mm_dev"),
             (dict(gels=0), "null gels_dev"), (dict(labels=0), "null labels_dev"), (dict(rec=0), "null record_dev"),
             (dict(P=0), "num_gels = 0"), (dict(B=0), "num_frames = 0"), (dict(B=-1), "num_frames = -1"), (dict(H=0), "height = 0"),
             (dict(W=0), "width = 0"), (dict(L=0), "num_labels = 0"), (dict(L=9), "num_labels = 9"), (dict(L=-2), "num_labels = -2"),
             (dict(pix=0.0), "pixmm = 0"), (dict(pix=float("nan")), "pixmm")]
    for kw, text in cases:
        assert call(**kw) == 2, kw
        msg = lib.tacex_last_error().decode()
        assert NAME + ":" in msg and text in msg, (kw, msg)
        assert (rec == -5.0).all() and (img == -3.0).all(), kw


def test_python_layer():
    import inspect

    import torch
    from tacex_amd import ContactField, GelSightSensor, PartContactField, TactileContactModel

    assert list(inspect.signature(TactileContactModel.parts).parameters)[1:] == ["hm", "frame_min", "indent", "labels", "num_labels", "slip",
                                                                                "frame_rows", "image"]
    assert inspect.signature(GelSightSensor.contact_field).parameters["parts"].default is None
    rec = torch.arange(2 * 3 * 16, dtype=torch.float64).reshape(2, 3, 16)
    f = PartContactField(rec, None)
    assert isinstance(f, ContactField) and f.cells is None and f.image is None
    flat = ContactField(rec.reshape(6, 16), None, None)
    for name in ("force", "normal_force", "friction_force", "torque", "contact_area", "num_contact", "centre_of_pressure", "max_penetration",
                 "volume", "num_slipping", "slip_ratio", "patch_angle", "patch_aspect"):
        got, want = getattr(f, name), getattr(flat, name)
        assert got.shape[:2] == (2, 3) and torch.equal(got.reshape(want.shape), want), name
