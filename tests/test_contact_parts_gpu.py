"""Per-part contact records on the GPU: `tacex_contact_field_parts` against its NumPy restatement (tests/contact_parts_ref.py) on
label maps that split every contact patch, against `tacex_contact_field` bit for bit with one label, its invariances (rectangles,
batch, repetition, an unaligned image), gel ids outside the table, and through the sensor on an `SdfSceneSource` with a part map."""
import numpy as np
import pytest
import torch
import contact_parts_ref as P
from contact_field_ref import GELS, borderline_pixels, case_pixmm
from test_contact_field_gpu import _inputs, _model, _same_bits, _sensor, _sensor_model

pytestmark = pytest.mark.gpu


def _labels(kind, hm, fmin, ind, L):
    return torch.from_numpy(P.case_labels(kind, hm.cpu().numpy(), fmin.cpu().numpy(), ind.cpu().numpy(), L)).cuda()


def _part_slip(B, L, H, W, start):
    return torch.from_numpy(P.case_part_slip(B, L, H, W, start)).cuda()


def _same_parts(f, g):
    return _same_bits(f.record, g.record) and (f.image is None) == (g.image is None) and (f.image is None or _same_bits(f.image, g.image))


def _check(field, hm, fmin, ind, ids, labels, L, slip, pixmm):
    hm_n, fmin_n, ind_n, lab_n = hm.cpu().numpy(), fmin.cpu().numpy(), ind.cpu().numpy(), labels.cpu().numpy()
    slip_n = None if slip is None else slip.cpu().numpy()
    rec, image, ab = P.parts_batch(hm_n, fmin_n, ind_n, GELS, ids, lab_n, L, slip_n, pixmm)
    got, img = field.record.cpu().numpy(), field.image.cpu().numpy()
    assert got.shape == rec.shape and img.shape == image.shape and img.dtype == np.float32
    differ = img.view(np.uint32) != image.view(np.uint32)
    print(f"image: {int(differ.sum())} of {differ.size} values differ")
    assert not differ.any(), "the traction image is not bit-equal"
    for b in range(hm_n.shape[0]):
        for l in range(L):
            g, r, a = got[b, l], rec[b, l], ab[b, l]
            for k in (0, 1, 2, 3, 4, 5, 6, 12):  # the plain sums
                assert abs(g[k] - r[k]) <= 1e-12 * a[k], (b, l, k, g[k], r[k], 1e-12 * a[k])
            assert g[8] == r[8] and g[11] == r[11] and g[7] == r[7], (b, l, g, r)
            for k in (9, 10, 15):
                assert abs(g[k] - r[k]) <= 1e-9, (b, l, k, g[k], r[k])
            if a[14] > 1.0:  # the axes differ: the angle is defined
                d = (g[14] - r[14] + np.pi / 2) % np.pi - np.pi / 2
                assert abs(d) <= 1e-9, (b, l, g[14], r[14])
            nb = 0  # stick / slip: the counts may differ by the pixels a 1-ulp difference decides
            if 0 <= ids[b] < len(GELS):
                lifted = np.where(lab_n[b] == l, hm_n[b], np.float32(1e6))  # (the others out of contact)
                nb, nc = borderline_pixels(lifted, fmin_n[b], ind_n[b], GELS[ids[b]], None if slip_n is None else slip_n[b, l], pixmm)
                assert nb <= 0.005 * nc
            assert abs(g[13] - r[13]) <= nb, (b, l, g[13], r[13], nb)
    return rec


@pytest.mark.parametrize("kind, L", [("halves", 2), ("checker", 3), ("some_255", 2), ("checker", 8)])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("H, W, start", [(24, 32, 0), (37, 53, 5), (48, 64, 2)])
def test_batch_against_the_restatement(H, W, start, B, kind, L):
    start = start + (0 if B == 5 else 3 * B)
    hm, fmin, ind, rows, _, ids, kinds = _inputs(H, W, B, start)
    labels, slip = _labels(kind, hm, fmin, ind, L), _part_slip(B, L, H, W, start)
    field = _model(B, H, (1, 1), ids).parts(hm, fmin, ind, labels, L, slip=slip, frame_rows=rows, image=True)
    rec = _check(field, hm, fmin, ind, ids, labels, L, slip, case_pixmm(H))
    if B > 1:
        assert ((rec[:, :, 8] > 0).sum(1) >= 2).any(), "no contact patch is split"


@pytest.mark.parametrize("H, W, start", [(24, 32, 0), (37, 53, 5), (48, 64, 2)])
def test_one_label_is_tacex_contact_field(H, W, start):
    B = 5
    hm, fmin, ind, rows, slip, ids, kinds = _inputs(H, W, B, start)
    m = _model(B, H, (1, 1), ids)
    labels = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    for r in (rows, None):
        want = m(hm, fmin, ind, slip=slip, frame_rows=r, image=True)
        got = m.parts(hm, fmin, ind, labels, 1, slip=slip[:, None, :].contiguous(), frame_rows=r, image=True)
        assert got.record.shape == (B, 1, 16) and _same_bits(got.record[:, 0].contiguous(), want.record) and _same_bits(got.image, want.image)
    none = m.parts(hm, fmin, ind, labels, 1, frame_rows=rows, image=True)  # no slip table: no shear
    assert _same_parts(none, m.parts(hm, fmin, ind, labels, 1, slip=torch.zeros((B, 1, 5), device="cuda"), frame_rows=rows, image=True))
    assert _same_bits(none.record[:, 0].contiguous(), m(hm, fmin, ind, frame_rows=rows).record)


@pytest.mark.parametrize("H, W", [(24, 32), (37, 53)])
def test_rectangle_repeat_batch_and_image_alignment(H, W):
    B, L = 5, 3
    for start in (0, 5):
        hm, fmin, ind, rows, _, ids, kinds = _inputs(H, W, B, start)
        labels, slip = _labels("some_255", hm, fmin, ind, L), _part_slip(B, L, H, W, start)
        m = _model(B, H, (1, 1), ids)
        want = m.parts(hm, fmin, ind, labels, L, slip=slip, frame_rows=rows, image=True)
        assert _same_parts(want, m.parts(hm, fmin, ind, labels, L, slip=slip, frame_rows=None, image=True)), "the contact rectangle changed an output"
        assert _same_parts(want, m.parts(hm, fmin, ind, labels, L, slip=slip, frame_rows=rows, image=True)), "the same call twice differs"
        lean = m.parts(hm, fmin, ind, labels, L, slip=slip, frame_rows=rows)
        assert lean.image is None and _same_bits(lean.record, want.record)
        for k in range(B):  # env k alone
            one = _model(1, H, (1, 1), ids[k:k + 1]).parts(hm[k:k + 1].contiguous(), fmin[k:k + 1].contiguous(), ind[k:k + 1].contiguous(),
                                                           labels[k:k + 1].contiguous(), L, slip=slip[k:k + 1].contiguous(),
                                                           frame_rows=rows[k:k + 1].contiguous(), image=True)
            assert _same_bits(one.record, want.record[k:k + 1]) and _same_bits(one.image, want.image[k:k + 1]), f"env {k} ({kinds[k]}) depends on its batch"
        # another label's slip changes nothing of label 0's record
        other = slip.clone()
        other[:, 1:] = torch.tensor([0.4, -0.3, 0.2, 3.0, 4.0], device="cuda")
        assert _same_bits(m.parts(hm, fmin, ind, labels, L, slip=other, frame_rows=rows).record[:, 0].contiguous(), want.record[:, 0].contiguous())
        # the image one float into its storage, the height map one float and the labels one byte into theirs: the same bits, in place
        guard = 16
        store = torch.full((guard + 1 + B * H * W * 3 + guard,), -7.0, device="cuda")
        img_off = store[guard + 1:guard + 1 + B * H * W * 3].view(B, H, W, 3)
        hm_off = torch.zeros(B * H * W + 4, device="cuda")[1:1 + B * H * W].view(B, H, W)
        hm_off.copy_(hm)
        lab_off = torch.zeros(B * H * W + 4, dtype=torch.uint8, device="cuda")[1:1 + B * H * W].view(B, H, W)
        lab_off.copy_(labels)
        assert img_off.data_ptr() % 16 != 0 and hm_off.data_ptr() % 16 != 0 and lab_off.data_ptr() % 4 != 0
        for h, lab in ((hm, labels), (hm_off, lab_off)):
            store.fill_(-7.0)
            got = m.parts(h, fmin, ind, lab, L, slip=slip, frame_rows=rows, image=img_off)
            assert got.image.data_ptr() == img_off.data_ptr() and _same_parts(got, want)
            assert (store[:guard + 1] == -7.0).all().item() and (store[guard + 1 + B * H * W * 3:] == -7.0).all().item()


def test_ids_outside_the_table_report_zeros():
    H, W, B, L = 24, 32, 3, 2
    hm, fmin, ind, rows, _, _, kinds = _inputs(H, W, B, 0)
    labels, slip = _labels("halves", hm, fmin, ind, L), _part_slip(B, L, H, W, 0)
    ids = [-1, 1, 3]
    for r in (rows, None):
        f = _model(B, H, (1, 1), ids).parts(hm, fmin, ind, labels, L, slip=slip, frame_rows=r, image=True)
        for b in (0, 2):
            assert not f.record[b].any().item() and not f.image[b].any().item()
        assert (f.normal_force[1] > 0).all().item()
        _check(f, hm, fmin, ind, ids, labels, L, slip, case_pixmm(H))


def test_python_layer_refuses_bad_arguments():
    from tacex_amd._lib import TacexHipError

    B, H, W = 2, 8, 12
    m = _model(B, 240, (1, 1))
    hm, v = torch.zeros((B, H, W), device="cuda"), torch.zeros(B, device="cuda")
    labels = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda")
    for L in (0, 9, -1):
        with pytest.raises(ValueError, match=f"num_labels = {L}"):
            m.parts(hm, v, v, labels, L)
    for bad in (labels.int(), labels[:1], labels[:, :, :8], torch.zeros((B, W, H), dtype=torch.uint8, device="cuda").permute(0, 2, 1)):
        with pytest.raises(ValueError, match="labels"):
            m.parts(hm, v, v, bad, 2)
    with pytest.raises(ValueError, match="slip"):
        m.parts(hm, v, v, labels, 2, slip=torch.zeros((B, 5), device="cuda"))
    with pytest.raises(ValueError, match="slip"):
        m.parts(hm, v, v, labels, 2, slip=torch.zeros((B, 3, 5), device="cuda"))
    with pytest.raises(ValueError, match="frame_rows"):
        m.parts(hm, v, v, labels, 2, frame_rows=torch.zeros((B, 4), device="cuda"))
    with pytest.raises(TacexHipError):
        m.parts(hm, v, v, labels.cpu(), 2)
    f = m.parts(hm, v, v, labels, 2)
    assert f.image is None and f.cells is None and not f.record[..., :9].any().item() and f.slip_ratio.shape == (B, 2)
    assert torch.equal(f.centre_of_pressure.cpu(), torch.tensor([[[(W - 1) / 2, (H - 1) / 2]] * 2] * B, dtype=torch.float64))


# ---- through the sensor ------------------------------------------------------------------------------------------------------
PIX, SH, SW = 0.0295, 240, 320


def _scene(part_map):
    """Two envs of three slots: slot 0 a ball that stands in the hole of a plate - slot 1 the plate, a union, slot 2 the hole, a
    subtraction.  The fold cuts the hole out of the ball too: the ball's cap rises out of the hole's sphere and stays."""
    from tacex_amd import SdfSceneSource
    from tacex_amd.utils import sdf_volumes as Vol

    src = SdfSceneSource([Vol.box((6.0, 4.0, 1.0), 0.1), Vol.sphere(1.0, 0.05)], 2, "cuda", num_slots=3, pixmm=PIX, part_map=part_map)
    flat = (1.0, 0.0, 0.0, 0.0)
    src.set_part(0, volume_id=1, op="union")
    src.set_part(1, volume_id=0, op="union")
    src.set_part(2, volume_id=1, op="subtract")
    src.set_pose(1, 160.0, 120.0, flat, press_mm=torch.tensor([0.4, 0.5]))
    near_face = src.part_pose[:, 1, 11] - 0.5
    src.set_pose(2, 170.0, 125.0, flat, z_mm=near_face, scale=0.6)
    src.set_pose(0, 170.0, 125.0, flat, z_mm=near_face - 0.55, scale=0.35)
    return src


def test_sensor_reports_each_parts_wrench(calib_dir):
    from tacex_amd import PartContactField
    from tacex_amd.sdf_scene import part_slip

    B, K = 2, 3
    model = _sensor_model(B)  # gels 0 and 1: both have a shear stiffness
    src, plain_src = _scene(True), _scene(False)
    s, plain = _sensor(calib_dir, B), _sensor(calib_dir, B)
    s.set_height_map_source(src)
    plain.set_height_map_source(plain_src)
    for sensor in (s, plain):
        sensor.update(0.01, force_recompute=True)
    with pytest.raises(ValueError, match="part_map=True"):
        plain.contact_field(model, parts=plain_src)
    reference = src.part_pose.clone()  # first contact
    for source in (src, plain_src):  # the ball slides 0.1 mm along x and turns; plate and hole stand still
        source.part_pose[:, 0, 9] += 0.1
    for sensor in (s, plain):
        sensor.update(0.01, force_recompute=True)
    for key in ("tactile_rgb", "height_map"):  # the part map changes no output of the sensor
        assert torch.equal(s.data.output[key], plain.data.output[key]), key
    owner = src.part_map
    assert owner.shape == (B, SH, SW) and all((owner == k).sum().item() >= 100 for k in range(K)), [(owner == k).sum().item() for k in range(K)]
    slip = part_slip(src.part_pose, reference, PIX)
    assert slip.shape == (B, K, 5) and (slip[:, 0, 0] - 0.1).abs().max().item() < 1e-6 and not slip[:, 1:, :3].any().item()
    f = s.contact_field(model, slip=slip, parts=src, image=True)
    assert isinstance(f, PartContactField) and f.record.shape == (B, K, 16) and f.image.shape == (B, SH, SW, 3)
    assert not f.friction_force[:, 1].any().item() and not f.friction_force[:, 2].any().item()  # the rim stands still
    assert (f.friction_force[:, 0, 0] > 0).all().item() and (f.normal_force[:, :2] > 0).all().item()
    whole = plain.contact_field(model, slip=slip[:, 0].contiguous())
    total = f.normal_force.sum(1)
    assert ((total - whole.normal_force).abs() <= 1e-12 * whole.normal_force).all().item(), (total, whole.normal_force)
    assert torch.equal(f.num_contact.sum(1), whole.num_contact)
    # a (B,5) table is repeated for every slot: then the parts' plain sums add up to the whole frame's
    same = s.contact_field(model, slip=slip[:, 0].contiguous(), parts=src)
    got, want = same.friction_force.sum(1), whole.friction_force
    assert ((got - want).abs() <= 1e-12 * whole.record[:, 6:7]).all().item(), (got, want)
    assert _same_bits(same.record[:, 0].contiguous(), f.record[:, 0].contiguous())
    # the owner shows no shear outside slot 0 in the image
    shear = f.image[..., :2].abs().sum(-1) > 0
    assert shear.any().item() and (owner[shear] == 0).all().item()
