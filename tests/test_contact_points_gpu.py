"""Contact point cloud on the GPU: `tacex_contact_points` against its NumPy restatement (tests/contact_points_ref.py, written from the
header's contract).  `count`, `pixels`, `labels`, `points`, `depth` and `normals` are compared bit for bit (hipcc's float32 divide and
square root are correctly rounded, as NumPy's are): contact sets at the seams of the kernel's walk, every relation of N to K, both
pads, the Philox offset, contact rectangles, labels, poses, a NaN pixel, a depth threshold, unaligned maps, and through the sensor."""
import numpy as np
import pytest
import torch
import contact_points_ref as R
from contact_field_ref import case_frame, case_pixmm

pytestmark = pytest.mark.gpu

PIXMM = 0.03
SHAPES = [(3, 17, 23), (2, 64, 64), (2, 1, 40), (2, 40, 1), (1, 240, 320)]
KEYS = ("count", "pixels", "labels", "points", "depth", "normals")


def _model(B, K, **kw):
    from tacex_amd import TactileContactPoints

    kw.setdefault("pixmm", PIXMM)
    return TactileContactPoints(B, "cuda", max_points=K, **kw)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _numpy(cloud):
    return {k: None if getattr(cloud, k) is None else getattr(cloud, k).cpu().numpy().copy() for k in KEYS}


def _bits(a):
    return a.view({4: np.uint32, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what=""):
    """Bit for bit, every output; a NaN normal (a NaN neighbour in the gradient) against a NaN normal."""
    for k in KEYS:
        g, w = got[k], want[k]
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        differ = _bits(g) != _bits(w)
        if g.dtype.kind == "f":
            differ &= ~(np.isnan(g) & np.isnan(w))
        if k == "normals":
            print(f"{what}: {int(differ.sum())} of {differ.size} normal components differ")
        assert not differ.any(), (what, k, int(differ.sum()), np.argwhere(differ)[:4].tolist())


def _launch(hm, fmin, ind, K, rects=None, labels=None, label=-1, pose="identity", **kw):
    """One call of a fresh model on NumPy inputs -> the outputs as NumPy arrays."""
    m = _model(hm.shape[0], K, **kw)
    if pose is None:
        m.pose = None
    elif not isinstance(pose, str):
        m.pose.copy_(_cuda(pose))
    return _numpy(m(_cuda(hm), _cuda(fmin), _cuda(ind), frame_rows=_cuda(rects), labels=_cuda(labels), label=label))


def _ref(hm, fmin, ind, K, rects=None, labels=None, label=-1, pose="identity", pad="zero", pixmm=PIXMM, min_depth_mm=0.0, unit=1.0, seed=None,
         frame_offset=0, call=0):
    B = hm.shape[0]
    pose = None if pose is None else R.pose_rows(B, general=False) if isinstance(pose, str) else pose
    return R.points_batch(hm, fmin, ind, pixmm, K, pad == "repeat", min_depth_mm, labels, label, pose, unit, seed is not None, seed or 0, frame_offset,
                          call, rects)


def _seams(H, W):
    """Linear pixel indices on both sides of every seam of the kernel's walk over a whole frame: lanes 63 | 64 of a wave, one step of a
    wave (64 items of four pixels), the workgroup's 256 threads, and where one wave's quarter of the items ends and the next begins."""
    groups = (W + 3) // 4
    items = H * groups
    per_wave = ((items + 63) // 64 + 3) // 4 * 64
    lin = {63, 64, R.BLOCK - 1, R.BLOCK, 4 * 64 - 1, 4 * 64, 4 * R.BLOCK - 1, 4 * R.BLOCK}
    for w in (1, 2, 3):
        it = w * per_wave
        if it < items:
            first = (it // groups) * W + (it % groups) * 4
            lin |= {first - 1, first, first + 1}
    return np.array(sorted(x for x in lin if 0 <= x < H * W), dtype=np.int64)


def _sets(H, W):
    n = H * W
    seams = _seams(H, W)
    runs = np.unique(np.concatenate([np.arange(max(s - 5, 0), min(s + 6, n)) for s in seams])) if seams.size else np.arange(0)
    return {"none": np.arange(0), "one": np.array([n // 3]), "ends": np.array([0, n - 1]), "seams": seams, "runs": runs, "full": np.arange(n)}


def _frames(B, H, W, lin):
    hm, fmin, ind = R.flat_frames(B, H, W)
    for b in range(B):
        R.press(hm, b, lin, seed=b)
    return hm, fmin, ind


@pytest.mark.parametrize("pad", ["zero", "repeat"])
@pytest.mark.parametrize("B, H, W", SHAPES, ids=lambda v: str(v))
def test_contact_sets_and_every_relation_of_n_to_k(B, H, W, pad):
    for name, lin in _sets(H, W).items():
        N = int(lin.size)
        if name != "none" and N == 0:
            continue
        hm, fmin, ind = _frames(B, H, W, lin)
        Ks = {5} if N == 0 else {max(N - 1, 1), N, N + 1}  # N = K + 1, K, K - 1
        if name == "full":
            Ks |= {7, 64, 100}
        for K in sorted(k for k in Ks if k <= 16384):
            got, want = _launch(hm, fmin, ind, K, pad=pad), _ref(hm, fmin, ind, K, pad=pad)
            assert (want["count"][:, 0] == N).all()
            _same(got, want, f"{name} N={N} K={K}")


@pytest.mark.parametrize("pad", ["zero", "repeat"])
def test_more_slots_than_pixels_and_the_largest_k(pad):
    B, H, W = 3, 17, 23  # K = 16384 > H W: 64 KiB of LDS
    for name in ("full", "seams", "none"):
        hm, fmin, ind = _frames(B, H, W, _sets(H, W)[name])
        _same(_launch(hm, fmin, ind, 16384, pad=pad), _ref(hm, fmin, ind, 16384, pad=pad), name)
    hm, fmin, ind = _frames(1, 240, 320, np.arange(240 * 320))  # N > K = 16384
    _same(_launch(hm, fmin, ind, 16384, pad=pad, seed=5), _ref(hm, fmin, ind, 16384, pad=pad, seed=5), "240x320 full")


def _sensor_frames(H, W):
    """A sphere and a wedge in the sensor's convention (camera depth in mm), with the library's own depth pass."""
    from test_contact_field_gpu import _depth_pass

    hm = np.stack([case_frame("sphere", H, W, seed=1), case_frame("edge", H, W, seed=2), case_frame("none", H, W), case_frame("clip_left", H, W)])
    fmin, ind, rows = _depth_pass(_cuda(hm))
    return hm, fmin.cpu().numpy(), ind.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("H, W", [(17, 23), (64, 64), (240, 320)])
def test_sphere_and_wedge_with_the_depth_pass_rectangles(H, W):
    hm, fmin, ind, rows = _sensor_frames(H, W)
    pix = case_pixmm(H)
    for K in (8, 1024):
        for pad in ("zero", "repeat"):
            want = _ref(hm, fmin, ind, K, pad=pad, pixmm=pix)
            assert want["count"][0, 0] > 8 and want["count"][1, 0] > 8 and want["count"][2, 0] == 0
            got = _launch(hm, fmin, ind, K, rects=rows, pad=pad, pixmm=pix)
            _same(got, want, f"K={K} {pad}, rectangles")
            _same(_launch(hm, fmin, ind, K, pad=pad, pixmm=pix), got, f"K={K} {pad}, whole frames")


def test_rectangles_at_every_corner_empty_and_beyond_the_image():
    B, H, W, K = 6, 17, 23, 12
    hm, fmin, ind = R.flat_frames(B, H, W)
    rects = np.zeros((B, 4), np.int32)
    boxes = [(0, 4, 0, 5), (0, 3, W - 6, W - 1), (H - 5, H - 1, 0, 6), (H - 4, H - 1, W - 5, W - 1)]
    for b, (r0, r1, c0, c1) in enumerate(boxes):  # a patch in every corner, the rectangle its bounding box
        ii, jj = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing="ij")
        R.press(hm, b, (ii * W + jj).reshape(-1), seed=b)
        rects[b] = (r0, r1, c0, c1)
    R.press(hm, 4, np.arange(40, 90))
    rects[4] = (-7, H + 3, -2, W + 9)  # clamped to the image
    R.press(hm, 5, np.arange(40, 90))
    rects[5] = (H, -1, W, -1)  # empty: no pixel is read, whatever the map holds
    got = _launch(hm, fmin, ind, K, rects=rects)
    _same(got, _ref(hm, fmin, ind, K, rects=rects), "rectangles")
    assert got["count"][5].tolist() == [0, 0] and (got["pixels"][5] == -1).all() and not got["points"][5].any()
    whole = _launch(hm[:5], fmin[:5], ind[:5], K)
    for k in KEYS:
        assert np.array_equal(_bits(got[k][:5]), _bits(whole[k])), k


def test_jitter_two_seeds_two_calls_and_the_frame_offset():
    B, H, W, K = 3, 64, 64, 100
    hm, fmin, ind = _frames(B, H, W, np.arange(300, 3500))
    firsts = set()
    for seed in (3, 2 ** 63 + 11):
        for off in (0, 2 ** 40 + 5, -2):
            m = _model(B, K, seed=seed, frame_offset=off)
            for call in (0, 1):
                got = _numpy(m(_cuda(hm), _cuda(fmin), _cuda(ind)))
                _same(got, _ref(hm, fmin, ind, K, seed=seed, frame_offset=off, call=call), f"seed {seed} offset {off} call {call}")
                firsts |= {(b, tuple(got["pixels"][b, 0])) for b in range(B)}
                for b in range(B):  # env b of the batch is a one-env call at frame_offset + b
                    one = _model(1, K, seed=seed, frame_offset=off + b)
                    one.call = call
                    alone = _numpy(one(_cuda(hm[b:b + 1]), _cuda(fmin[b:b + 1]), _cuda(ind[b:b + 1])))
                    for k in KEYS:
                        assert np.array_equal(_bits(alone[k][0]), _bits(got[k][b])), (k, b)
            assert m.call == 2
    assert len(firsts) > 20  # the subsample starts elsewhere per env, seed, offset and call
    plain = _model(B, K)  # no seed: rank 0 first, and no counter
    a = _numpy(plain(_cuda(hm), _cuda(fmin), _cuda(ind)))
    assert plain.call == 0 and (a["pixels"][:, 0] == [300 // W, 300 % W]).all()


def test_labels_every_one_and_a_255_region():
    B, H, W, K = 3, 17, 23, 64
    hm, fmin, ind = _frames(B, H, W, np.arange(30, 300))
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    labels = np.stack([((ii + 2 * b) // 5 % 2 * 3).astype(np.uint8) for b in range(B)])  # bands of 0 and 3
    labels[:, 6:9, 10:16] = 255
    labels[:, 12, :] = 7
    every = _launch(hm, fmin, ind, K, labels=labels)
    _same(every, _ref(hm, fmin, ind, K, labels=labels), "label -1")
    assert {0, 3, 7, 255} <= set(every["labels"].reshape(-1).tolist())
    for label in (0, 3, 254):
        got = _launch(hm, fmin, ind, K, labels=labels, label=label)
        _same(got, _ref(hm, fmin, ind, K, labels=labels, label=label), f"label {label}")
        v = got["count"][:, 1]
        assert all((got["labels"][b, :v[b]] == label).all() for b in range(B)) and (label == 254) == (not v.any())
    # labels one byte into their storage: the byte path
    store = torch.zeros(B * H * W + 4, dtype=torch.uint8, device="cuda")
    off = store[1:1 + B * H * W].view(B, H, W)
    off.copy_(_cuda(labels))
    m = _model(B, K)
    _same(_numpy(m(_cuda(hm), _cuda(fmin), _cuda(ind), labels=off, label=3)), _ref(hm, fmin, ind, K, labels=labels, label=3), "unaligned labels")
    # on a width of whole float4 groups too: the 32-bit label load
    hm4, fmin4, ind4 = _frames(2, 16, 24, np.arange(20, 300))
    lab4 = ((np.arange(16)[:, None] + np.arange(24)[None, :]) % 4).astype(np.uint8)[None].repeat(2, 0)
    lab4[:, 5:8, 3:11] = 255
    for label in (-1, 0, 3):
        _same(_launch(hm4, fmin4, ind4, K, labels=lab4, label=label), _ref(hm4, fmin4, ind4, K, labels=lab4, label=label), f"16x24 label {label}")
    off4 = torch.zeros(2 * 16 * 24 + 4, dtype=torch.uint8, device="cuda")[1:1 + 2 * 16 * 24].view(2, 16, 24)
    off4.copy_(_cuda(lab4))
    _same(_numpy(_model(2, K)(_cuda(hm4), _cuda(fmin4), _cuda(ind4), labels=off4, label=3)), _ref(hm4, fmin4, ind4, K, labels=lab4, label=3), "16x24 unaligned labels")


@pytest.mark.parametrize("H, W", [(17, 23), (64, 64)])
def test_poses_units_a_depth_threshold_and_no_normals(H, W):
    B, K = 3, 50
    hm, fmin, ind = _frames(B, H, W, np.arange(20, min(H * W - 5, 900)))
    general = R.pose_rows(B)
    for pose, unit in ((None, 1.0), ("identity", 1.0), (general, 1e-3), (None, 1e-3)):
        got = _launch(hm, fmin, ind, K, pose=pose, unit=unit)
        _same(got, _ref(hm, fmin, ind, K, pose=pose, unit=unit), f"pose {type(pose).__name__} unit {unit}")
    moved, plain = _launch(hm, fmin, ind, K, pose=general, unit=1e-3), _launch(hm, fmin, ind, K, pose=None)
    Rm, t = general.reshape(B, 3, 4)[:, :, :3].astype(np.float64), general.reshape(B, 3, 4)[:, :, 3].astype(np.float64)
    want = np.einsum("brc,bkc->bkr", Rm, plain["points"].astype(np.float64) * 1e-3) + t[:, None, :]
    assert np.abs(moved["points"] - want).max() < 1e-6 and np.array_equal(moved["depth"], plain["depth"])
    assert np.abs(np.linalg.norm(moved["normals"].astype(np.float64), axis=-1) - 1).max() < 1e-5
    deep = _launch(hm, fmin, ind, K, min_depth_mm=0.3)
    _same(deep, _ref(hm, fmin, ind, K, min_depth_mm=0.3), "min_depth_mm")
    assert (deep["count"][:, 0] < plain["count"][:, 0]).all() and (deep["depth"][deep["pixels"][..., 0] >= 0] > np.float32(0.3)).all()
    bare = _launch(hm, fmin, ind, K, normals=False)
    assert bare["normals"] is None
    _same(bare, plain, "without normals")


def test_a_nan_pixel_is_no_contact_pixel():
    B, H, W, K = 2, 17, 23, 400
    hm, fmin, ind = _frames(B, H, W, np.arange(40, 200))
    hm[0, 4, 7] = np.nan
    hm[1, 0, 0] = np.nan
    got = _launch(hm, fmin, ind, K)
    _same(got, _ref(hm, fmin, ind, K), "NaN")
    assert got["count"][:, 0].tolist() == [159, 160] and not (got["pixels"][0] == [4, 7]).all(-1).any()
    assert np.isnan(got["normals"][0]).any() and not np.isnan(got["points"]).any() and not np.isnan(got["depth"]).any()


@pytest.mark.parametrize("H, W", [(16, 24), (17, 23)])
def test_an_unaligned_height_map_gives_the_same_bits(H, W):
    B, K = 2, 40
    hm, fmin, ind = _frames(B, H, W, np.arange(10, 350))
    want = _launch(hm, fmin, ind, K)
    store = torch.zeros(B * H * W + 4, device="cuda")
    off = store[1:1 + B * H * W].view(B, H, W)
    off.copy_(_cuda(hm))
    assert off.data_ptr() % 16 != 0
    got = _numpy(_model(B, K)(off, _cuda(fmin), _cuda(ind)))
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    _same(want, _ref(hm, fmin, ind, K), f"{H}x{W}")


def test_the_model_reuses_its_buffers_and_refuses_bad_tensors():
    from tacex_amd import ContactPoints
    from tacex_amd._lib import TacexHipError

    B, H, W, K = 2, 8, 12, 9
    m = _model(B, K)
    hm_n, fmin_n, ind_n = _frames(B, H, W, np.arange(5, 11))
    hm, v, w = _cuda(hm_n), _cuda(fmin_n), _cuda(ind_n)
    a = m(hm, v, w)
    ptrs = [getattr(a, k).data_ptr() for k in KEYS]
    assert isinstance(a, ContactPoints) and a.points.shape == (B, K, 3) and a.pixels.dtype == torch.int32 and a.labels.dtype == torch.uint8
    assert a.num_contact.tolist() == [6, 6] and a.num_valid.tolist() == [6, 6]
    assert a.valid.dtype == torch.bool and a.valid.tolist() == [[True] * 6 + [False] * 3] * B
    b = m(torch.full_like(hm, float(R.BACK)), v, w)  # the same buffers, now empty
    assert [getattr(b, k).data_ptr() for k in KEYS] == ptrs and not a.valid.any().item() and (a.pixels == -1).all().item()
    for bad in (hm[:1], hm.double(), hm.permute(0, 2, 1), hm[:, :, ::2]):
        with pytest.raises(ValueError, match="hm"):
            m(bad, v, w)
    with pytest.raises(ValueError, match="frame_min"):
        m(hm, v[:1], w)
    with pytest.raises(ValueError, match="frame_rows"):
        m(hm, v, w, frame_rows=torch.zeros((B, 4), device="cuda"))
    with pytest.raises(ValueError, match="labels"):
        m(hm, v, w, labels=torch.zeros((B, H, W), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="label"):
        m(hm, v, w, label=0)
    with pytest.raises(ValueError, match="label"):
        m(hm, v, w, labels=torch.zeros((B, H, W), dtype=torch.uint8, device="cuda"), label=255)
    with pytest.raises(TacexHipError):
        m(hm.cpu(), v, w)
    m.pose = torch.zeros((B, 9), device="cuda")
    with pytest.raises(ValueError, match="pose"):
        m(hm, v, w)


# ---- through the sensor ------------------------------------------------------------------------------------------------------
def test_sensor_contact_points_with_an_indenter_source(calib_dir):
    from tacex_amd import GelSightSensorGroup, IndenterHeightMapSource
    from tacex_amd.utils.synthetic import PIXMM as SENSOR_PIXMM
    from test_contact_field_gpu import _depth_pass, _sensor, _sensor_model

    B, K = 3, 512
    s = _sensor(calib_dir, B)
    src = IndenterHeightMapSource(B, "cuda", pixmm=SENSOR_PIXMM)
    src.set("sphere", cx=torch.tensor([150.0, 190.0, 30.0]), cy=torch.tensor([110.0, 130.0, 200.0]), r=torch.tensor([60.0, 45.0, 50.0]),
            press_mm=torch.tensor([0.8, 1.2, 0.5]))
    s.set_height_map_source(src)
    s.update(0.01, force_recompute=True)
    rgb = s.data.output["tactile_rgb"].clone()
    model = _model(B, K, pixmm=SENSOR_PIXMM, unit=1e-3)
    got = _numpy(s.contact_points(model))
    hm = s.data.output["height_map"]
    fmin, ind, rows = _depth_pass(hm)
    want = _ref(hm.cpu().numpy(), fmin.cpu().numpy(), ind.cpu().numpy(), K, pixmm=SENSOR_PIXMM, unit=1e-3)
    _same(got, want, "sensor")
    field = s.contact_field(_sensor_model(B))
    assert np.array_equal(got["count"][:, 0], field.num_contact.cpu().numpy().astype(np.int32)) and (got["count"][:2, 0] > K).all()
    centre = got["points"][:, :, :2].astype(np.float64).mean(1) / (SENSOR_PIXMM * 1e-3) + [(320 - 1) / 2, (240 - 1) / 2]
    assert np.abs(centre[:2] - [[150.0, 110.0], [190.0, 130.0]]).max() < 2.0  # the cloud sits on the indenter
    assert torch.equal(s.data.output["tactile_rgb"], rgb)
    mem = [_sensor(calib_dir, B), _sensor(calib_dir, B)]
    GelSightSensorGroup(mem)
    with pytest.raises(RuntimeError):
        mem[0].contact_points(model)


def test_sensor_per_part_clouds_partition_the_whole_cloud(calib_dir):
    from tacex_amd import SdfSceneSource
    from tacex_amd.utils import sdf_volumes as Vol
    from test_contact_field_gpu import _sensor

    B, K, pix = 2, 16384, 0.0295
    flat = (1.0, 0.0, 0.0, 0.0)

    def scene(part_map):
        src = SdfSceneSource([Vol.box((2.0, 1.5, 1.0), 0.1), Vol.sphere(1.0, 0.05)], B, "cuda", num_slots=2, pixmm=pix, part_map=part_map)
        src.set_part(0, volume_id=1, op="union")
        src.set_part(1, volume_id=0, op="union")
        src.set_pose(0, 100.0, 90.0, flat, press_mm=torch.tensor([0.4, 0.5]))
        src.set_pose(1, 215.0, 150.0, flat, press_mm=torch.tensor([0.3, 0.2]))
        return src

    src, plain_src = scene(True), scene(False)
    s, plain = _sensor(calib_dir, B), _sensor(calib_dir, B)
    s.set_height_map_source(src)
    plain.set_height_map_source(plain_src)
    for sensor in (s, plain):
        sensor.update(0.01, force_recompute=True)
    model = _model(B, K, pixmm=pix)
    with pytest.raises(ValueError, match="part_map=True"):
        plain.contact_points(model, parts=plain_src)
    whole = _numpy(s.contact_points(model, parts=src))
    bare = _numpy(plain.contact_points(model))
    for k in ("count", "pixels", "points", "depth", "normals"):  # the labels change nothing but the labels
        assert np.array_equal(_bits(whole[k]), _bits(bare[k])), k
    assert (whole["count"][:, 0] > 500).all() and (whole["count"][:, 0] <= K).all()
    parts = [_numpy(s.contact_points(model, parts=src, label=l)) for l in (0, 1)]
    for b in range(B):
        n = whole["count"][b, 0]
        lab = whole["labels"][b, :n]
        assert set(lab.tolist()) == {0, 1}, set(lab.tolist())
        for l in (0, 1):
            m = parts[l]["count"][b, 0]
            assert m == (lab == l).sum() > 100 and (parts[l]["labels"][b, :m] == l).all()
            assert np.array_equal(parts[l]["pixels"][b, :m], whole["pixels"][b, :n][lab == l])
            assert np.array_equal(_bits(parts[l]["points"][b, :m]), _bits(whole["points"][b, :n][lab == l]))
