"""Contact force field on the GPU: `tacex_contact_field` against its NumPy restatement (tests/contact_field_ref.py, written from the
header's contract) - sphere, cylinder, wedge, two spheres, no contact, full contact, contact clipped by every border; gel ids in and
out of the table; slip rows with translation, twist, both and none; the 16-byte and the dword path; grids from 1 x 1 to one cell per
pixel; the contact rectangle, repeatability, batch independence; and through the sensor."""
import numpy as np
import pytest
import torch
from contact_field_ref import GELS, borderline_pixels, case_batch, case_pixmm, case_slip, contact_batch

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -24


def _gels():
    from tacex_amd import ContactGel

    return [ContactGel(*(float(v) for v in row[:3])) for row in GELS]


def _model(B, H, grid, ids=None, pixmm=None):
    from tacex_amd import TactileContactModel

    m = TactileContactModel(_gels(), B, "cuda", pixmm=case_pixmm(H) if pixmm is None else pixmm, grid=grid)
    assert np.array_equal(m.gels.cpu().numpy(), GELS)
    if ids is not None:
        m.gel_ids.copy_(torch.tensor(ids, dtype=torch.int32))
    return m


def _depth_pass(hm: torch.Tensor):
    """frame_min, indent, contact rectangles of the library's own pass (gelpad 4.5 mm, 24 mm to the camera)."""
    from tacex_amd import _lib

    lib = _lib.load_library()
    B, H, W = hm.shape
    fmin, ind = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    rows = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
    _lib.check(lib.tacex_indentation_depth(_lib.ptr(hm), 0.0045, 0.024, _lib.ptr(fmin), _lib.ptr(ind), _lib.ptr(rows), B, H, W,
                                           _lib.current_stream_handle(hm.device)), "tacex_indentation_depth")
    return fmin, ind, rows


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same_field(f, g):
    return _same_bits(f.record, g.record) and _same_bits(f.cells, g.cells) and (f.image is None) == (g.image is None) and \
        (f.image is None or _same_bits(f.image, g.image))


def _check(field, hm, fmin, ind, ids, slip, pixmm, grid):
    """Every assertion of the kernel against the restatement, for one call."""
    hm_n, fmin_n, ind_n = hm.cpu().numpy(), fmin.cpu().numpy(), ind.cpu().numpy()
    slip_n = None if slip is None else slip.cpu().numpy()
    rec, cells, image, ab = contact_batch(hm_n, fmin_n, ind_n, GELS, ids, slip_n, pixmm, grid)
    got = field.record.cpu().numpy()
    B = hm_n.shape[0]
    if field.image is not None:
        img = field.image.cpu().numpy()
        assert img.shape == image.shape and img.dtype == np.float32
        assert np.array_equal(img[..., 2].view(np.uint32), image[..., 2].view(np.uint32)), "normal traction differs"
        tnorm = np.hypot(image[..., 0].astype(np.float64), image[..., 1].astype(np.float64))
        err = np.abs(img[..., :2].astype(np.float64) - image[..., :2].astype(np.float64)).max(axis=-1)
        print(f"shear traction: max |err| / |t_ref| = {(err / np.maximum(tnorm, 1e-300)).max():.3e} (bound {4 * ULP32:.3e}), "
              f"{np.count_nonzero(err)} of {err.size} pixels differ")
        assert (err <= 4 * ULP32 * tnorm).all()
    for b in range(B):
        for k in (0, 1, 2, 3, 4, 5, 6, 12):  # the plain sums
            tol = 1e-12 * ab[b, k]
            assert abs(got[b, k] - rec[b, k]) <= tol, (b, k, got[b, k], rec[b, k], tol)
        assert got[b, 8] == rec[b, 8] and got[b, 11] == rec[b, 11] and got[b, 7] == rec[b, 7], (b, got[b], rec[b])
        for k in (9, 10, 15):
            assert abs(got[b, k] - rec[b, k]) <= 1e-9, (b, k, got[b, k], rec[b, k])
        if ab[b, 14] > 1.0:  # lambda_max - lambda_min > 1 px^2: the axis is defined
            d = (got[b, 14] - rec[b, 14] + np.pi / 2) % np.pi - np.pi / 2
            assert abs(d) <= 1e-9, (b, got[b, 14], rec[b, 14])
        # stick / slip: the counts may differ by the pixels a 1-ulp difference decides
        nb = 0
        if ids is None or 0 <= ids[b] < len(GELS):
            nb, nc = borderline_pixels(hm_n[b], fmin_n[b], ind_n[b], GELS[0 if ids is None else ids[b]], None if slip_n is None else slip_n[b], pixmm)
            assert nb <= 0.005 * nc
        assert abs(got[b, 13] - rec[b, 13]) <= nb, (b, got[b, 13], rec[b, 13], nb)
    c_got = field.cells.cpu().numpy()
    c_ref = cells.astype(np.float32)
    assert c_got.shape == c_ref.shape and c_got.dtype == np.float32
    assert (np.abs(c_got.astype(np.float64) - c_ref.astype(np.float64)) <= np.spacing(np.abs(c_ref)).astype(np.float64)).all(), "cells differ by more than one float32 ulp"
    # the cells of an env sum to the net force (each cell was rounded to float32 once)
    csum = c_got.astype(np.float64).sum(axis=(1, 2))
    cabs = np.abs(c_got.astype(np.float64)).sum(axis=(1, 2))
    assert (np.abs(csum - got[:, 0:3]) <= ULP32 * cabs + 1e-12 * ab[:, 0:3]).all()
    return rec


def _inputs(H, W, B, start):
    hm_n, kinds = case_batch(H, W, B, start)
    hm = torch.from_numpy(hm_n).cuda()
    fmin, ind, rows = _depth_pass(hm)
    slip = torch.from_numpy(case_slip(B, H, W, start)).cuda()
    ids = [(start + b) % len(GELS) for b in range(B)]
    return hm, fmin, ind, rows, slip, ids, kinds


# 24x32 and 48x64: 16-byte loads; 37x53: dword loads (W % 4 != 0, the last item of a row is partial), 5 bands with a partial last one.
# The ten frame kinds are spread over the cases by `start`.
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("H, W, start", [(24, 32, 0), (37, 53, 5), (48, 64, 2)])
def test_batch_against_the_restatement(H, W, start, B):
    start = start + (0 if B == 5 else 3 * B)
    hm, fmin, ind, rows, slip, ids, kinds = _inputs(H, W, B, start)
    print(kinds)
    field = _model(B, H, (5, 7), ids)(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
    _check(field, hm, fmin, ind, ids, slip, case_pixmm(H), (5, 7))


@pytest.mark.parametrize("grid", [(1, 1), (5, 7), (9, 11), (24, 32)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("start", [0, 5])
def test_grids_on_24x32(grid, start):
    H, W, B = 24, 32, 5
    hm, fmin, ind, rows, slip, ids, kinds = _inputs(H, W, B, start)
    field = _model(B, H, grid, ids)(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
    _check(field, hm, fmin, ind, ids, slip, case_pixmm(H), grid)


def test_the_tuned_size_240x320_with_the_marker_grid():
    H, W, B = 240, 320, 2
    hm, fmin, ind, rows, slip, ids, kinds = _inputs(H, W, B, 6)  # clipped by the left and the right border
    field = _model(B, H, (9, 11), ids)(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
    rec = _check(field, hm, fmin, ind, ids, slip, case_pixmm(H), (9, 11))
    assert (rec[:, 8] > 1000).all()


def test_a_wide_image_takes_more_than_64_kib_of_lds():
    """9 x 1000 with three cell columns: 8 (12 W + 24 cols) = 96.6 KB of LDS per workgroup, two bands (the second of one row)."""
    H, W, B = 9, 1000, 1
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    hm_n = np.minimum(28.5 - 0.8 + 2e-6 * (jj - 613.2) ** 2 + 0.01 * (ii - 3.6) ** 2, 29.0).astype(np.float32)[None]
    hm = torch.from_numpy(hm_n).cuda()
    fmin, ind, rows = _depth_pass(hm)
    slip = torch.tensor([[0.02, 0.01, 0.01, 600.0, 4.0]], device="cuda")
    field = _model(B, H, (2, 3), [0], pixmm=0.0295)(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
    rec = _check(field, hm, fmin, ind, [0], slip, 0.0295, (2, 3))
    assert rec[0, 8] > 2000


@pytest.mark.parametrize("H, W", [(24, 32), (37, 53)])
def test_rectangle_repeat_and_batch_independence(H, W):
    B = 5
    for start in (0, 5):
        hm, fmin, ind, rows, slip, ids, kinds = _inputs(H, W, B, start)
        m = _model(B, H, (5, 7), ids)
        with_rows = m(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
        without = m(hm, fmin, ind, slip=slip, frame_rows=None, image=True)
        again = m(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
        assert _same_field(with_rows, without), "the contact rectangle changed an output"
        assert _same_field(with_rows, again), "the same call twice differs"
        lean = m(hm, fmin, ind, slip=slip, frame_rows=rows, image=False)  # no image: the same record and cells, nothing else written
        assert lean.image is None and _same_bits(lean.record, with_rows.record) and _same_bits(lean.cells, with_rows.cells)
        for k in range(B):  # env k alone
            one = _model(1, H, (5, 7), ids[k:k + 1])(hm[k:k + 1].contiguous(), fmin[k:k + 1].contiguous(), ind[k:k + 1].contiguous(),
                                                       slip=slip[k:k + 1].contiguous(), frame_rows=rows[k:k + 1].contiguous(), image=True)
            assert _same_bits(one.record, with_rows.record[k:k + 1]) and _same_bits(one.cells, with_rows.cells[k:k + 1]) \
                and _same_bits(one.image, with_rows.image[k:k + 1]), f"env {k} ({kinds[k]}) depends on its batch"


def test_an_image_buffer_is_written_in_place_and_unaligned_views_give_the_same_bits():
    H, W, B = 24, 32, 3
    hm, fmin, ind, rows, slip, ids, kinds = _inputs(H, W, B, 1)
    m = _model(B, H, (5, 7), ids)
    want = m(hm, fmin, ind, slip=slip, frame_rows=rows, image=True)
    guard = 16
    store = torch.full((guard + B * H * W * 3 + guard,), -7.0, device="cuda")
    img = store[guard:guard + B * H * W * 3].view(B, H, W, 3)
    got = m(hm, fmin, ind, slip=slip, frame_rows=rows, image=img)
    assert got.image.data_ptr() == img.data_ptr() and _same_field(got, want)
    assert (store[:guard] == -7.0).all().item() and (store[-guard:] == -7.0).all().item()
    # the height map one float into its storage, the image one float into its own: the dword path
    hm_store = torch.zeros(B * H * W + 4, device="cuda")
    hm_off = hm_store[1:1 + B * H * W].view(B, H, W)
    hm_off.copy_(hm)
    store.fill_(-7.0)
    img_off = store[guard + 1:guard + 1 + B * H * W * 3].view(B, H, W, 3)
    assert hm_off.data_ptr() % 16 != 0 and img_off.data_ptr() % 16 != 0
    got = m(hm_off, fmin, ind, slip=slip, frame_rows=rows, image=img_off)
    assert _same_field(got, want)
    assert (store[:guard + 1] == -7.0).all().item() and (store[guard + 1 + B * H * W * 3:] == -7.0).all().item()


def test_ids_outside_the_table_report_zeros():
    H, W, B = 24, 32, 3
    hm, fmin, ind, rows, slip, _, kinds = _inputs(H, W, B, 0)
    ids = [-1, 1, 3]
    for r in (rows, None):
        f = _model(B, H, (5, 7), ids)(hm, fmin, ind, slip=slip, frame_rows=r, image=True)
        for b in (0, 2):
            assert not f.record[b].any().item() and not f.cells[b].any().item() and not f.image[b].any().item()
        assert f.record[1, 6].item() > 0
        _check(f, hm, fmin, ind, ids, slip, case_pixmm(H), (5, 7))


def test_no_slip_table_means_no_shear():
    H, W, B = 37, 53, 3
    hm, fmin, ind, rows, _, ids, kinds = _inputs(H, W, B, 0)
    m = _model(B, H, (5, 7), ids)
    f = m(hm, fmin, ind, slip=None, frame_rows=rows, image=True)
    assert not f.record[:, 0:2].any().item() and not f.image[..., 0:2].any().item() and not f.cells[..., 0:2].any().item()
    zero = torch.zeros((B, 5), device="cuda")
    assert _same_field(f, m(hm, fmin, ind, slip=zero, frame_rows=rows, image=True))
    _check(f, hm, fmin, ind, ids, None, case_pixmm(H), (5, 7))


def test_python_layer_refuses_bad_tensors():
    from tacex_amd._lib import TacexHipError

    B, H, W = 2, 8, 12
    m = _model(B, 240, (2, 3))
    hm, v = torch.zeros((B, H, W), device="cuda"), torch.zeros(B, device="cuda")
    for bad in (hm[:1], hm.double(), hm.permute(0, 2, 1), hm[:, :, ::2]):
        with pytest.raises(ValueError):
            m(bad, v, v)
    with pytest.raises(ValueError):
        m(hm, v[:1], v)
    with pytest.raises(ValueError):
        m(hm, v, v, slip=torch.zeros((B, 4), device="cuda"))
    with pytest.raises(ValueError):
        m(hm, v, v, frame_rows=torch.zeros((B, 4), device="cuda"))
    with pytest.raises(ValueError):
        m(hm, v, v, image=torch.zeros((B, H, W, 3), device="cuda", dtype=torch.float64))
    with pytest.raises(TacexHipError):
        m(hm.cpu(), v, v)
    with pytest.raises(ValueError):  # a grid larger than the image
        _model(B, 240, (9, 11))(hm, v, v)
    g = torch.Generator(device="cuda").manual_seed(3)
    ids = m.randomize(generator=g).clone()
    assert ids.dtype == torch.int32 and ((ids >= 0) & (ids < 3)).all().item()
    m.randomize(env_ids=[1], generator=g)
    assert m.gel_ids[0] == ids[0] and 0 <= int(m.gel_ids[1]) < 3
    f = m(hm, v, v)
    assert f.image is None and not f.record[:, :9].any().item() and f.slip_ratio.shape == (B,)
    assert torch.equal(f.centre_of_pressure.cpu(), torch.tensor([[(W - 1) / 2, (H - 1) / 2]] * B, dtype=torch.float64))


# ---- through the sensor ------------------------------------------------------------------------------------------------------
def _sensor(calib_dir, B, markers=False):
    from tacex_amd import GelSightSensor, GelSightSensorCfg
    from tacex_amd.simulation_approaches.fots import FOTSMarkerSimulatorCfg
    from tacex_amd.simulation_approaches.gpu_taxim import TaximSimulatorCfg

    cfg = GelSightSensorCfg(
        num_envs=B, data_types=["tactile_rgb", "height_map"] + (["marker_motion"] if markers else []),
        sensor_camera_cfg=GelSightSensorCfg.SensorCameraCfg(resolution=(320, 240), clipping_range=(0.024, 0.029)),
        optical_sim_cfg=TaximSimulatorCfg(calib_folder_path=str(calib_dir), gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024,
                                          tactile_img_res=(320, 240), device="cuda"),
        marker_motion_sim_cfg=FOTSMarkerSimulatorCfg(tactile_img_res=(320, 240), device="cuda") if markers else None,
        device="cuda")
    return GelSightSensor(cfg)


def _sensor_model(B):
    from tacex_amd import TactileContactModel
    from tacex_amd.utils.synthetic import PIXMM

    m = TactileContactModel(_gels(), B, "cuda", pixmm=PIXMM, grid=(9, 11))
    m.gel_ids.copy_(torch.arange(B, dtype=torch.int32) % 3)
    return m


def _own_buffers(s, model, slip=None):
    """The model on the sensor's own height map, with a depth pass of its own."""
    hm = s.data.output["height_map"]
    fmin, ind, rows = _depth_pass(hm)
    assert torch.equal(ind, s.indentation_depth)
    return model(hm, fmin, ind, slip=slip, frame_rows=rows, image=True), (hm, fmin, ind)


def test_sensor_contact_field_after_a_camera_depth_a_height_map_and_a_source(calib_dir):
    from tacex_amd import IndenterHeightMapSource
    from tacex_amd.utils.synthetic import PIXMM, synthetic_depth_maps

    B, H, W = 3, 240, 320
    model = _sensor_model(B)
    depth_mm = synthetic_depth_maps(B, H, W, seed=5, flat_fraction=0.0)[0]
    # camera depth
    s = _sensor(calib_dir, B)
    s.set_camera_depth(depth_mm.cuda() / 1000.0)
    s.update(0.01, force_recompute=True)
    rgb = s.data.output["tactile_rgb"].clone()
    f = s.contact_field(model, image=True)
    want, (hm, fmin, ind) = _own_buffers(s, model)
    assert _same_field(f, want) and (f.normal_force > 0).all().item() and not f.friction_force.any().item()
    _check(f, hm, fmin, ind, [0, 1, 2], None, PIXMM, (9, 11))
    assert torch.equal(s.data.output["tactile_rgb"], rgb)
    # the same frames rendered without the call in between
    s2 = _sensor(calib_dir, B)
    s2.set_camera_depth(depth_mm.cuda() / 1000.0)
    s2.update(0.01, force_recompute=True)
    assert torch.equal(s2.data.output["tactile_rgb"], rgb)
    # set_height_map
    s4 = _sensor(calib_dir, B)
    s4.initialize()
    s4.set_height_map(torch.roll(s.data.output["height_map"], shifts=(7, -9), dims=(1, 2)).contiguous())
    s4.update(0.01, force_recompute=True)
    f = s4.contact_field(model, image=True)
    want, _ = _own_buffers(s4, model)
    assert _same_field(f, want) and (f.normal_force > 0).all().item()
    # an analytic source
    s3 = _sensor(calib_dir, B)
    src = IndenterHeightMapSource(B, "cuda", pixmm=PIXMM)
    src.set("sphere", cx=torch.tensor([150.0, 190.0, 30.0]), cy=torch.tensor([110.0, 130.0, 200.0]), r=torch.tensor([60.0, 45.0, 50.0]),
            press_mm=torch.tensor([0.8, 1.2, 0.5]))
    s3.set_height_map_source(src)
    s3.update(0.01, force_recompute=True)
    f = s3.contact_field(model, slip=torch.tensor([[0.02, 0.0, 0.0, 150.0, 110.0]] * B, device="cuda"))
    want, _ = _own_buffers(s3, model, slip=torch.tensor([[0.02, 0.0, 0.0, 150.0, 110.0]] * B, device="cuda"))
    assert f.image is None and _same_bits(f.record, want.record) and _same_bits(f.cells, want.cells)
    assert (f.friction_force[:2, 0] > 0).all().item() and (f.num_slipping[:2] > 0).all().item()
    assert not f.friction_force[2].any().item() and f.num_slipping[2].item() == 0  # gel 2 has no shear stiffness


def test_sensor_with_fots_takes_its_slip_from_the_trajectory(calib_dir):
    from tacex_amd import GelSightSensorGroup, slip_from_fots
    from tacex_amd.utils.synthetic import synthetic_depth_maps

    B, H, W = 3, 240, 320
    model = _sensor_model(B)
    depth = synthetic_depth_maps(B, H, W, seed=9, flat_fraction=0.0, kinds=("sphere",))[0].cuda() / 1000.0
    s, ref = _sensor(calib_dir, B, markers=True), _sensor(calib_dir, B, markers=True)
    for t in range(3):  # the indenter shears and yaws
        for k, sensor in enumerate((s, ref)):
            sensor.set_camera_depth(torch.roll(depth, shifts=(2 * t, 3 * t), dims=(1, 2)).contiguous())
            sensor.marker_motion_simulator.set_indenter_yaw(torch.full((B,), 0.04 * t).cuda())
            sensor.update(0.01, force_recompute=True)
        f = s.contact_field(model, image=True)
    slip = slip_from_fots(s.marker_motion_simulator)
    traj = s.marker_motion_simulator._traj_state.cpu().numpy()
    assert (traj[:, 0] == 3).all()
    got = slip.cpu().numpy()
    np.testing.assert_allclose(got[:, 0], traj[:, 4] - traj[:, 1], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 2], 0.08, rtol=0, atol=1e-6)
    mm2pix = s.marker_motion_simulator.cfg.mm_to_pixel  # the depth image moved 6 px in x and 4 px in y; the centroids are in FOTS's mm
    assert (np.abs(got[:, 0] - 6 / mm2pix) < 1.5 / mm2pix).all() and (np.abs(got[:, 1] - 4 / mm2pix) < 1.5 / mm2pix).all()
    np.testing.assert_allclose(got[:, 3], traj[:, 4] * mm2pix + W / 2, rtol=0, atol=1e-3)
    np.testing.assert_allclose(got[:, 4], traj[:, 5] * mm2pix + H / 2, rtol=0, atol=1e-3)
    want, (hm, fmin, ind) = _own_buffers(s, model, slip=slip)
    assert _same_field(f, want)
    assert (f.friction_force[:2].abs().sum(dim=1) > 0).all().item() and (f.torque[:2, 2] != 0).all().item()  # (gel 2 has no shear stiffness)
    # the call in between changed nothing the sensor produces
    for key in ("tactile_rgb", "marker_motion", "height_map"):
        assert torch.equal(s.data.output[key], ref.data.output[key]), key
    # a grouped sensor refuses; the model takes the group's buffers
    mem = [_sensor(calib_dir, B), _sensor(calib_dir, B)]
    GelSightSensorGroup(mem)
    with pytest.raises(RuntimeError):
        mem[0].contact_field(model)
