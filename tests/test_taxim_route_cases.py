"""CPU: the case table of tests/taxim_route_cases.py is what it claims to be - kernel sizes and bit-equal w / h taps from the
calibration folder of every case, the routes of the table against the restated host predicates, the frame properties from the
oracle's mask, and which cases carry enough strong-gradient pixels for the same-bin share."""
import numpy as np
import pytest

import taxim_route_cases as rc


@pytest.fixture(scope="module")
def calib_tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("route_calib")


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_case_table(case, calib_dir, calib_tmp):
    ref = rc.reference(case, calib_dir, calib_tmp)
    t = ref["tables"]
    assert tuple(t.ksize_w) == tuple(t.ksize_h) == case.ksize
    same = [np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(t.taps_w, t.taps_h)]
    assert all(same), "w and h taps must be bit-equal: the tuned routes are not eligible otherwise"
    if case.sigmas is not None:  # the oracle reads the same folder: same sigmas in pixels along both axes
        pyr, fin = rc.SIGMA_SETS[case.sigmas]
        got = np.array(ref["oracle"].pyr_sigmas + [ref["oracle"].final_sigma])
        np.testing.assert_allclose(got, np.array([(s, s) for s in pyr + [fin]]), rtol=1e-12)
    # the table's routes are what the predicates (as restated) give ...
    want = rc.expected_routes(case.ksize, same, case.H, case.W)
    assert want["levels"] == case.level_routes and want["tail"] == case.tail and want["tail_frames"] == case.tail_frames, want
    # ... and the table's geometry notes hold
    ns, sw = rc.stream_strips(case.W)
    assert ns * sw >= case.W > (ns - 1) * sw and sw <= rc.STREAM_VW and sw % 4 == 0
    # frames
    assert ref["hm"].shape == (len(case.frames), case.H, case.W) and len(case.frames) in (1, 4)
    rc.check_frame_properties(case, ref["M"])
    assert ref["indent"][list(case.frames).index("none")] == 0 if "none" in case.frames else True
    assert case.frames[-1] != "none", "the frame rendered alone holds contact"
    n_strong = int(ref["strong"].sum())
    assert (n_strong >= rc.STRONG_MIN) == case.strong, n_strong
    assert np.abs(ref["Z"]).max() > 0.1


def test_table_covers_what_it_is_for():
    """Every route and ending appears, off the tuned sizes; the strip and tile geometry named in the notes is the restated one."""
    assert len({c.name for c in rc.CASES}) == len(rc.CASES)
    assert not any(c.shape in ((240, 320), (480, 640)) for c in rc.CASES)
    routes = {r for c in rc.CASES for r in c.level_routes}
    assert routes == {"mfma", "band", "band_loop_384", "band_loop_640", "generic", "tail"}
    assert {(c.tail, c.n_fused) for c in rc.CASES} == {("stream", 4), ("stream", 3), ("tiled", 4), ("tiled", 3), ("shade", 0)}
    strips = {c.shape: rc.stream_strips(c.W) for c in rc.CASES}
    assert strips[(40, 400)] == (3, 136) and strips[(20, 168)] == (1, 168) and strips[(20, 172)] == (2, 88) and strips[(24, 340)][0] == 3
    assert strips[(243, 324)] == (2, 164) and strips[(252, 336)] == (2, 168) and strips[(483, 644)] == (4, 164) and strips[(16, 16)] == (1, 16)
    # no case has the tile geometry (TH | H and TW | W) or the strip widths (160 at both) of the tuned sizes in its tail
    for c in rc.CASES:
        if c.n_fused:
            assert c.H % rc.TILE_H or c.W % rc.TILE_W or rc.stream_strips(c.W)[1] != 160, c.name
    # the guards of tail_levels: frames at and one past the summed radii, and a level set with nothing in front of its tail
    by = rc.BY_NAME
    assert by["10x12-T4s"].n_fused == 4 and by["9x12-T4s"].n_fused == by["8x8-T4s"].n_fused == by["12x8-T4s"].n_fused == 0
    assert by["11x12-T3s"].n_fused == 3 and by["10x12-T3s"].n_fused == 0 and by["48x64-F4"].n_fused == 0
    assert all(n in by for n in rc.BAND_SKIP_CASES)


def test_restated_predicates_at_the_tuned_sizes():
    """The restatement gives what the tuned sizes are known to run: matrix-core levels, then <9,5,3,5> / <9,5,9> streaming."""
    t = [True] * 7
    assert rc.expected_routes(rc.K320, t, 240, 320) == {"ksize": list(rc.K320), "levels": ["mfma"] * 3 + ["tail"] * 4, "tail": "stream", "tail_frames": "tiled"}
    assert rc.expected_routes(rc.K640, t, 480, 640) == {"ksize": list(rc.K640), "levels": ["mfma"] * 4 + ["tail"] * 3, "tail": "stream", "tail_frames": "tiled"}
    assert rc.expected_routes(rc.K320, [False] * 7, 240, 320)["levels"] == ["generic"] * 7  # sigma_w != sigma_h: nothing tuned
    assert rc.tiled_obs_fusable(240, 320, 4) and rc.tiled_obs_fusable(480, 640, 3) and not rc.tiled_obs_fusable(80, 128, 4)
    bs = rc.band_skip_frames(80, 128)
    assert bs.shape == (4, 80, 128) and (bs[3] == rc.FAR_MM).all() and bs[0, 0].min() < 28.5 and bs[1, -1].min() < 28.5 and bs[2, 40].min() < 28.5
