"""The owner of a hit on the GPU: `tacex_height_map_from_sdf_scene_parts` against its NumPy restatement
(tests/sdf_scene_parts_ref.py) - heights bit for bit, part map byte for byte -, against the plain entry point in all four outputs, an
env alone against the env in a batch, and two calls against each other."""
import numpy as np
import pytest
import torch
import sdf_scene_ref as S
from test_sdf_scene_gpu import GD, GH, _load, _outputs, _same
from test_sdf_scene_parts import restated

pytestmark = pytest.mark.gpu

F32 = np.float32
GEL_TOP, NEAR, FAR, TOL = S.GEL_TOP, S.NEAR, S.FAR, S.TOL
SHAPES = [(24, 32), (30, 40), (9, 4), (8, 2048)]
B = S.NUM_ENVS


def _source(n, H, W, K, max_steps=32, part_map=True):
    from tacex_amd import SdfSceneSource, SdfVolume

    return SdfSceneSource([SdfVolume(*v) for v in S.three_volumes()], n, "cuda", num_slots=K, pixmm=S.scene_pixmm(H, W), gel_top_mm=GEL_TOP,
                          near_clip_mm=NEAR, far_clip_mm=FAR, max_steps=max_steps, tol_mm=TOL, part_map=part_map)


def _fill(src, n, H, W):
    out = _outputs(n, H, W)
    src.fill(out[0], out[1], out[2], GH, GD, rows=out[3])
    return out


@pytest.mark.parametrize("max_steps", [1, 8, 32])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_restatement(H, W, K, max_steps):
    want_hm, want_owner = restated(H, W, K, max_steps)
    src = _source(B, H, W, K, max_steps)
    assert src.part_map is None  # until the first fill
    _load(src, *S.gpu_scene(H, W, K))
    hm = _fill(src, B, H, W)[0]
    got, owner = hm.cpu().numpy(), src.part_map.cpu().numpy()
    assert owner.shape == (B, H, W) and owner.dtype == np.uint8
    for b in range(B):
        bad = np.flatnonzero(got[b].view(np.uint32) != want_hm[b].view(np.uint32))
        assert bad.size == 0, (b, bad.size, [(int(q) // W, int(q) % W, got[b].flat[q], want_hm[b].flat[q]) for q in bad[:4]])
        bad = np.flatnonzero(owner[b] != want_owner[b])
        assert bad.size == 0, (b, bad.size, [(int(q) // W, int(q) % W, owner[b].flat[q], want_owner[b].flat[q]) for q in bad[:4]])
    # the second fill writes the same tensor in place
    kept = src.part_map
    kept.fill_(99)
    src.fill(hm, *_outputs(B, H, W)[1:3], GH, GD)
    assert src.part_map is kept and np.array_equal(kept.cpu().numpy(), want_owner)


@pytest.mark.parametrize("H,W", SHAPES + [(250, 320)])
def test_the_parts_entry_keeps_the_plain_entrys_bits(H, W):
    for K, max_steps in ((1, 32), (3, 8), (8, 1), (8, 32)):
        scene = S.gpu_scene(H, W, K)
        plain, parts = _source(B, H, W, K, max_steps, part_map=False), _source(B, H, W, K, max_steps)
        _load(plain, *scene)
        _load(parts, *scene)
        want, got = _fill(plain, B, H, W), _fill(parts, B, H, W)
        assert plain.part_map is None
        assert all(_same(g, w) for g, w in zip(got, want)), (K, max_steps, [i for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)])
        far = got[0] == FAR
        assert torch.equal(parts.part_map == 255, far) and (parts.part_map[~far] < K).all().item()
        assert (~far).any().item() or K == 1 or max_steps == 1


def test_an_env_alone_equals_the_env_in_a_batch_and_a_call_repeats():
    H, W, K = 30, 40, 8
    ids, ops, pose = S.gpu_scene(H, W, K)
    batch = _source(B, H, W, K)
    _load(batch, ids, ops, pose)
    want = _fill(batch, B, H, W)
    owner = batch.part_map.clone()
    assert np.array_equal(owner.cpu().numpy(), restated(H, W, K, 32)[1])
    batch.part_map.fill_(7)
    again = _fill(batch, B, H, W)
    assert all(_same(g, w) for g, w in zip(again, want)) and torch.equal(batch.part_map, owner)  # two calls: the same bytes
    alone = _source(1, H, W, K)
    for b in range(B):
        _load(alone, ids[b:b + 1], ops[b:b + 1], pose[b:b + 1])
        got = _fill(alone, 1, H, W)
        assert all(_same(g[0], w[b]) for g, w in zip(got, want)) and torch.equal(alone.part_map[0], owner[b]), b


def test_fill_checks_the_part_map():
    n, H, W, K = 2, 24, 32, 3
    src = _source(n, H, W, K)
    _fill(src, n, H, W)
    assert (src.part_map == 255).all().item()  # (nothing placed yet: every slot is empty)
    src.part_map = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="part_map must stay"):
        _fill(src, n, H, W)
