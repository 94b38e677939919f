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
