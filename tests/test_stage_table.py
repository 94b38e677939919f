"""The stage layer's shared Python pieces (tacex_amd/_stage.py) on CPU tensors: the profile table with its ids, `randomize`,
`assign`, the check before a launch, and the check of a tensor argument."""
import numpy as np
import pytest
import torch

from tacex_amd import _stage
from tacex_amd._lib import TacexHipError

P, C, B = 5, 4, 3
CPU = torch.device("cpu")


def _table(p=P, b=B):
    rows = np.arange(p * C, dtype=np.float32).reshape(p, C)
    return _stage.ProfileTable("Model", "rows", "ids", rows, b, "cpu"), rows


def test_ids_start_at_zero_and_rows_are_the_table():
    t, rows = _table()
    assert t.ids.dtype == torch.int32 and t.ids.shape == (B,) and not t.ids.any()
    assert t.rows.dtype == torch.float32 and np.array_equal(t.rows.numpy(), rows)
    assert t.device == CPU and t.width == C
    ids, r = t.check()
    assert ids is t.ids and r is t.rows


def test_randomize_reproduces_the_seeded_draw():
    t, _ = _table()
    want = torch.randint(0, P, (B,), dtype=torch.int32, generator=torch.Generator().manual_seed(11))
    got = t.randomize(generator=torch.Generator().manual_seed(11))
    assert got is t.ids and got.dtype == torch.int32 and torch.equal(got, want)
    assert len(set(want.tolist())) > 1  # (a draw that could tell one env from another)
    # a subset: the same call with the subset's length, the other ids untouched
    t.ids.copy_(torch.tensor([7, 8, 9], dtype=torch.int32))
    one = torch.randint(0, P, (1,), dtype=torch.int32, generator=torch.Generator().manual_seed(12))
    ptr = t.ids.data_ptr()
    got = t.randomize(env_ids=[1], generator=torch.Generator().manual_seed(12))
    assert got.data_ptr() == ptr and got.tolist() == [7, int(one[0]), 9]


def test_assign_keeps_the_storage_when_the_shape_stays():
    t, rows = _table()
    ptr = t.rows.data_ptr()
    t.assign(rows + 1)
    assert t.rows.data_ptr() == ptr and np.array_equal(t.rows.numpy(), rows + 1)
    more = np.ones((P + 2, C), dtype=np.float32)
    t.assign(more)
    assert t.rows.data_ptr() != ptr and t.rows.shape == (P + 2, C) and np.array_equal(t.rows.numpy(), more)
    t.check()
    assert 0 <= int(t.randomize(generator=torch.Generator().manual_seed(1)).max()) < P + 2


@pytest.mark.parametrize("spoil", [
    lambda t: setattr(t, "ids", t.ids.long()),                                   # dtype
    lambda t: setattr(t, "ids", torch.zeros(B + 1, dtype=torch.int32)),          # length
    lambda t: setattr(t, "ids", torch.zeros(2 * B, dtype=torch.int32)[::2]),     # a view with a stride
    lambda t: setattr(t, "ids", [0] * B),                                        # not a tensor
    lambda t: setattr(t, "rows", torch.zeros((P, C + 1))),                       # width
    lambda t: setattr(t, "rows", t.rows.double()),
    lambda t: setattr(t, "rows", torch.zeros((0, C))),                           # no row at all
], ids=["ids-dtype", "ids-length", "ids-stride", "ids-list", "rows-width", "rows-dtype", "rows-empty"])
def test_check_refuses_what_a_kernel_cannot_take(spoil):
    t, _ = _table()
    spoil(t)
    with pytest.raises(ValueError, match="Model: (ids|rows) must stay"):
        t.check()


def test_check_refuses_a_table_on_another_device():
    t, _ = _table()
    t.ids = torch.zeros(B, dtype=torch.int32, device="meta")
    with pytest.raises(TacexHipError, match="ids is on meta"):
        t.check()


def test_table_attr_reads_and_assigns_the_tables_tensors():
    class Model:
        gels, gel_ids = _stage.table_attr("rows"), _stage.table_attr("ids")

        def __init__(self):
            self._table = _table()[0]

    m = Model()
    assert m.gels is m._table.rows and m.gel_ids is m._table.ids
    m.gel_ids = new = torch.ones(B, dtype=torch.int32)
    assert m._table.ids is new and m._table.check()[0] is new


def test_check_tensor_rule():
    ok = torch.zeros((B, 6, 8, 3))
    shape = (B, "H", "W", 3)
    assert _stage.check_tensor("Model", "rgb", ok, shape, torch.float32, CPU) is ok
    for bad in (ok[:1], ok[..., :2], ok[:, :0], ok[0], ok.double(), ok.permute(0, 2, 1, 3), ok[:, ::2, ::2][:, :, :, :], None, ok.numpy()):
        with pytest.raises(ValueError, match=r"Model: rgb must be a contiguous \(3, H, W, 3\) torch.float32 tensor"):
            _stage.check_tensor("Model", "rgb", bad, shape, torch.float32, CPU)
    with pytest.raises(ValueError, match=r"\(3,\) torch.int32"):
        _stage.check_tensor("Model", "ids", torch.zeros(B), (B,), torch.int32, CPU)
    meta = torch.zeros((B, 6, 8, 3), device="meta")
    with pytest.raises(TacexHipError, match="rgb is on meta, the model on cpu"):
        _stage.check_tensor("Model", "rgb", meta, shape, torch.float32, CPU)
    # shape, dtype and stride come before the device; a call site may name another exception for the device
    with pytest.raises(ValueError):
        _stage.check_tensor("Model", "rgb", meta.double(), shape, torch.float32, CPU)
    with pytest.raises(ValueError, match="is on meta"):
        _stage.check_tensor("Model", "rgb", meta, shape, torch.float32, CPU, on_device=ValueError)


def test_profile_list_and_the_constructor_preamble():
    class Prof:
        def row(self):
            return np.zeros(C, dtype=np.float32)

    one = Prof()
    assert _stage.profile_list("Model", "profiles", one, Prof) == [one]
    assert _stage.profile_list("Model", "profiles", (one, one), Prof) == [one, one]
    for bad in ([], [np.zeros(C)], [one, None]):
        with pytest.raises(ValueError, match="Model: profiles must be a non-empty sequence of Prof"):
            _stage.profile_list("Model", "profiles", bad, Prof)
    with pytest.raises(ValueError, match="num_frames = 0"):  # (before the device is looked at)
        _stage.open_stage("Model", "profiles", "profile_ids", one, Prof, 0, "cpu")
    with pytest.raises(TacexHipError, match="GPU only"):
        _stage.open_stage("Model", "profiles", "profile_ids", one, Prof, 2, "cpu")


# ---- LibrarySource: the base of the relief and SDF height-map sources ----

def _relief():
    from tacex_amd import ReliefHeightMapSource, ReliefTile

    tiles = [ReliefTile(np.zeros((2, 3), np.float32), 0.02), ReliefTile(np.ones((4, 2), np.float32), 0.05, wrap=False)]
    return ReliefHeightMapSource, tiles, (dict(cx_px=4, cy_px=3, yaw=0.0, press_mm=0.5), 6, 0.5)


def _sdf():
    from tacex_amd import SdfVolume, SdfVolumeSource

    z = np.indices((2, 3, 4))[0].astype(np.float32) - 0.5
    return SdfVolumeSource, [SdfVolume(z, 1.0), SdfVolume(z[:, :2, :2], 0.5)], (dict(cx_px=4, cy_px=3, quat_wxyz=(1, 0, 0, 0), z_mm=28.0), 11, 28.0)


SOURCES = pytest.mark.parametrize("make", [_relief, _sdf], ids=["relief", "sdf"])


@SOURCES
def test_library_source_value_errors_come_before_the_device(make):
    cls, entries, _ = make()
    name = cls.__name__
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match=f"{name}: pixmm must be > 0"):
            cls(entries, B, "cpu", pixmm=bad)
    with pytest.raises(ValueError, match=f"{name}: .* must be a non-empty sequence"):
        cls([], B, "cpu")
    with pytest.raises(ValueError, match=f"{name}: num_frames = 0"):
        cls(entries, 0, "cpu")
    with pytest.raises(TacexHipError, match=f"{name} runs on the GPU only"):
        cls(entries, B, "cpu")


def _on_cpu(monkeypatch, make):
    """The source built by its own constructor on CPU tensors (open_stage without its device rule and without the library), its one
    launch replaced by a record of the arguments."""
    cls, entries, _ = make()

    def open_stage(owner, rows_name, ids_name, profiles, pcls, num_frames, device):
        rows = np.stack([p.row() for p in profiles])
        return None, _stage.ProfileTable(owner, rows_name, ids_name, rows, num_frames, device)

    monkeypatch.setattr(_stage, "open_stage", open_stage)

    class Probe(cls):
        def _launch(self, *args):
            self.launched = args

    return Probe(entries, B, "cpu"), entries


@SOURCES
def test_library_source_constructor_tail(monkeypatch, make):
    src, entries = _on_cpu(monkeypatch, make)
    payload, table_i, table_f, ids = (getattr(src, n) for n in src._names)
    arrays = [e.validate() for e in entries]
    assert src.device == CPU and src.num_envs == B and src.writes_frame_rows
    assert payload.dtype == torch.float32 and np.array_equal(payload.numpy(), np.concatenate([a.reshape(-1) for a in arrays]))
    assert table_i.dtype == torch.int32 and table_i.shape == (2, 4)
    assert table_i[:, 0].tolist() == [0, arrays[0].size]  # each entry's first payload element
    assert [tuple(r[1:1 + a.ndim]) for r, a in zip(table_i.tolist(), arrays)] == [a.shape for a in arrays]
    assert np.array_equal(table_f.numpy(), np.stack([e.row() for e in entries]))
    assert ids.dtype == torch.int32 and ids.shape == (B,) and not ids.any()
    assert src.pose.shape == (B, 16) and src.pose.dtype == torch.float32
    got = src.randomize(generator=torch.Generator().manual_seed(3))
    assert got is ids and torch.equal(got, torch.randint(0, 2, (B,), dtype=torch.int32, generator=torch.Generator().manual_seed(3)))
    pose_kw, column, value = make()[2]  # set_pose: scalars become one value per env (per_env)
    src.set_pose(**pose_kw)
    assert src.pose[:, column].tolist() == [value] * B
    src.set_pose(**{**pose_kw, "cx_px": torch.tensor([1.0, 2.0, 3.0])})
    assert len(set(src.pose.sum(1).tolist())) == B


@SOURCES
def test_library_source_fill_checks_its_arguments_then_launches(monkeypatch, make):
    src, _ = _on_cpu(monkeypatch, make)
    name = type(src).__mro__[1].__name__
    payload, table_i, table_f, ids = src._names
    good = dict(hm=torch.zeros((B, 6, 8)), frame_min=torch.zeros(B), indent=torch.zeros(B), rows=torch.zeros((B, 4), dtype=torch.int32))
    assert src.fill(good["hm"], good["frame_min"], good["indent"], 0.0045, 0.024, rows=good["rows"]) is good["hm"]
    assert [a is b for a, b in zip(src.launched[:8], [getattr(src, payload), getattr(src, table_i), getattr(src, table_f), getattr(src, ids),
                                                       good["hm"], good["frame_min"], good["indent"], good["rows"]])] == [True] * 8
    assert src.launched[8:] == (0.0045, 0.024)
    src.fill(good["hm"], good["frame_min"], None, 0.0045, 0.024)  # indent and rows are optional
    assert src.launched[6] is None and src.launched[7] is None
    del src.launched
    spoiled = {
        "hm": [torch.zeros((B + 1, 6, 8)), torch.zeros((B, 6)), torch.zeros((B, 6, 8)).double(), torch.zeros((B, 6, 16))[:, :, ::2], None],
        "frame_min": [torch.zeros(B + 1), torch.zeros((B, 1)), torch.zeros(B, dtype=torch.int32), torch.zeros(2 * B)[::2], None],
        "indent": [torch.zeros(B - 1), torch.zeros(B).double(), torch.zeros(2 * B)[::2]],
        "rows": [torch.zeros((B, 4)), torch.zeros((B, 3), dtype=torch.int32), torch.zeros((B, 8), dtype=torch.int32)[:, ::2]],
    }
    for arg, bads in spoiled.items():
        for bad in bads:
            with pytest.raises(ValueError, match=f"{name}: {arg} must be a contiguous .* tensor, got"):
                src.fill(**{**good, arg: bad}, gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024)
    with pytest.raises(TacexHipError, match=f"{name}: hm is on meta"):
        src.fill(**{**good, "hm": torch.zeros((B, 6, 8), device="meta")}, gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024)
    # what the caller writes in place must keep its shape, dtype and stride
    for attr, bads in {"pose": [torch.zeros((B, 15)), torch.zeros((B, 16)).double(), torch.zeros((B, 32))[:, ::2]],
                       table_i: [getattr(src, table_i).long(), getattr(src, table_i)[:1]],
                       payload: [getattr(src, payload).double(), getattr(src, payload)[::2]],
                       table_f: [getattr(src, table_f)[:1].clone(), getattr(src, table_f).double()],
                       ids: [getattr(src, ids).long()]}.items():
        kept = getattr(src, attr)
        for bad in bads:
            setattr(src, attr, bad)
            with pytest.raises(ValueError, match=f"{name}: {attr} must stay a contiguous"):
                src.fill(**good, gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024)
        setattr(src, attr, kept)
    assert not hasattr(src, "launched")  # (no refused call got as far as the launch)
    src.fill(**good, gelpad_height=0.0045, gelpad_to_camera_min_distance=0.024)
    assert src.launched[4] is good["hm"]


def test_per_env_argument():
    assert torch.equal(_stage.per_env(2, 3, CPU), torch.full((3,), 2.0, dtype=torch.float64))
    t = torch.tensor([1.0, 2.0, 3.0])
    got = _stage.per_env(t, 3, CPU)
    assert got.dtype == torch.float64 and got.tolist() == [1.0, 2.0, 3.0]
    assert _stage.per_env(torch.tensor(5), 3, CPU).tolist() == [5.0] * 3


def test_depth_sources_share_one_fill():
    from tacex_amd import height_map_source as hs

    fill = hs._SimCameraDepthSource.fill
    assert hs.MeshLibraryDepthSource.fill is fill and hs.FemSurfaceDepthSource.fill is fill and hs.AffineBodyDepthSource.fill is fill
    assert not hasattr(hs.MeshDepthSource, "fill")
