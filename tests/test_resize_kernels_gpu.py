"""The four antialiased-resize kernels (taxim_kernels.hip: resize_aa_kernel, resize_aa_v4_kernel, resize_aa_v_kernel, resize_aa_h_kernel)
against the float64 restatement of the same algorithm, oracle.taxim_oracle.resize_bilinear_aa, at 1e-5 absolute - the project's own
figure for the observation resize.  Inputs are uniform in [0, 1], unsmoothed.  Where the float32 window of the kernels (`aa_window`)
and the float64 one differ by a tap, that tap's weight is float32 round-off: it cannot explain a miss of 1e-5.

Routes, as `run_resize_aa` picks them: no temp -> one kernel; a temp -> vertical pass into (B, dh, sw, C), float4 lanes when sw * C is a
multiple of 4 (resize_aa_v4_kernel, taps unrolled by four with a remainder loop) else one float per lane (resize_aa_v_kernel), then
the horizontal pass (resize_aa_h_kernel).  Destination and temp lie between sentinels; the temp has exactly (B, dh, sw, C) elements."""
import numpy as np
import pytest
import torch

from oracle.taxim_oracle import _aa_weights, resize_bilinear_aa
from test_taxim_routes_gpu import Guarded

TOL = 1e-5

# (sh, sw) -> (dh, dw)
SINGLE = (
    ((480, 640), (33, 70)),     # the tuned frame to an odd observation
    ((241, 323), (7, 9)),       # about 35 x 36 taps per output
    ((3, 3), (7, 5)),           # smallest frame, up
    ((5, 300), (5, 17)),        # dh == sh: weights 1 and 0 along y
    ((17, 19), (17, 19)),       # identity
    ((24, 32), (243, 324)),     # up-sampling by a non-integer factor
)
BIG = ((40, 52), (4100, 4100))  # more outputs than the 65 536 blocks x 256 threads the grid is capped at: the grid-stride loop's second trip
# (sh, sw, C) -> (dh, dw)
TWO_PASS_V4 = (
    ((243, 324, 3), (32, 32)),
    ((37, 68, 3), (8, 8)),
    ((24, 32, 4), (48, 64)),    # up-sampling: fewer than four taps, the unrolled loop never runs
)
TWO_PASS_V = (
    ((33, 70, 3), (8, 8)),
    ((50, 70, 1), (13, 9)),
    ((9, 13, 3), (20, 30)),     # up-sampling
)


# temp AND destination beyond the capped grid: the second trip of resize_aa_v_kernel's and resize_aa_h_kernel's grid-stride loops.  Many
# small frames, not one large one: the kernels form tap positions in float32 (as torch's float32 kernel does), whose spacing at 4100 px
# is 4.9e-4 - a 4101 px row through the same route came out 1.2e-4 from the float64 oracle for that reason alone.
TWO_PASS_BIG_B, TWO_PASS_BIG = 21600, ((9, 13, 3), (20, 14))


def _tap_counts(n_in, n_out):
    return {len(w) for _, w in _aa_weights(n_in, n_out)}


def test_resize_cases_are_what_they_are_for():
    """CPU: the routes' conditions and the vertical tap counts, from the oracle's weights."""
    for (sh, sw, C), _ in TWO_PASS_V4:
        assert sw * C % 4 == 0
    for (sh, sw, C), _ in TWO_PASS_V:
        assert sw * C % 4 != 0
    yc = set().union(*(_tap_counts(sh, dh) for (sh, _, _), (dh, _) in TWO_PASS_V4))
    assert {c % 4 for c in yc if c >= 4} == {0, 1, 2, 3}, yc  # every remainder behind the unrolled loop
    assert any(c < 4 for c in yc), yc                          # ... and the remainder loop alone
    assert any(dh > sh for (sh, _, _), (dh, _) in TWO_PASS_V4) and any(dh > sh for (sh, _, _), (dh, _) in TWO_PASS_V)
    assert max(_tap_counts(241, 7)) >= 35 and max(_tap_counts(323, 9)) >= 36
    assert all(w.max() == 1.0 and w.sum() == 1.0 for _, w in _aa_weights(5, 5))  # dh == sh: two taps of weight 1 and 0
    assert BIG[1][0] * BIG[1][1] > 65536 * 256
    (_, sw, C), (dh, dw) = TWO_PASS_BIG
    assert sw * C % 4 != 0 and TWO_PASS_BIG_B * dh * sw * C > 65536 * 256 and TWO_PASS_BIG_B * dh * dw * C > 65536 * 256
    x = np.random.default_rng(0).random((2, 3, 5))
    np.testing.assert_array_equal(resize_bilinear_aa(x, (3, 5)), x)


def _resize(x, out_hw, tmp: bool, planar: bool):
    """x (B, sh, sw, C) on the GPU -> (B, dh, dw, C) through the C entry points, into guarded buffers."""
    from tacex_amd import _lib

    lib = _lib.load_library()
    B, sh, sw, C = x.shape
    dh, dw = out_hw
    dst = Guarded((B, dh, dw, C))
    st = torch.cuda.current_stream().cuda_stream
    if planar:
        assert C == 1 and not tmp
        _lib.check(lib.tacex_resize_bilinear_aa(x.data_ptr(), sh, sw, dst.t.data_ptr(), dh, dw, B, st), "tacex_resize_bilinear_aa")
    else:
        scratch = Guarded((B, dh, sw, C)) if tmp else None
        _lib.check(lib.tacex_resize_bilinear_aa_nhwc(x.data_ptr(), sh, sw, dst.t.data_ptr(), dh, dw, C, B, scratch.t.data_ptr() if tmp else 0, st),
                   "tacex_resize_bilinear_aa_nhwc")
    torch.cuda.synchronize()
    what = f"resize {tuple(x.shape)} -> {out_hw} tmp={tmp}"
    if tmp:
        scratch.check(what + " temp")
    return dst.check(what + " dst")


def _input(B, sh, sw, C, seed):
    return torch.rand((B, sh, sw, C), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _check(x, out_hw, got, what):
    want = np.moveaxis(resize_bilinear_aa(np.moveaxis(x.numpy(), 3, 1), out_hw), 1, 3)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"{what}: max|kernel - float64| {err:.3e}")
    assert err <= TOL, what
    assert np.ptp(want) > 100 * TOL  # (the outputs differ from each other by far more than the tolerance)


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", SINGLE, ids=lambda v: "x".join(map(str, v)))
def test_single_pass_kernel(src, dst):
    """resize_aa_kernel: C = 1 through tacex_resize_bilinear_aa (two planes), C = 3 through the channels-last entry without a temp."""
    x1, x3 = _input(2, *src, 1, seed=1), _input(2, *src, 3, seed=3)
    _check(x1, dst, _resize(x1.cuda(), dst, tmp=False, planar=True), f"single pass C=1 {src}->{dst}")
    _check(x3, dst, _resize(x3.cuda(), dst, tmp=False, planar=False), f"single pass C=3 {src}->{dst}")


@pytest.mark.gpu
def test_single_pass_kernel_grid_stride_loop():
    """16.81 million outputs on a grid capped at 65 536 x 256 threads: the first 33 536 threads compute a second element."""
    src, dst = BIG
    x = _input(1, *src, 1, seed=5)
    _check(x, dst, _resize(x.cuda(), dst, tmp=False, planar=True), f"single pass C=1 {src}->{dst}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("src,dst", TWO_PASS_V4 + TWO_PASS_V, ids=lambda v: "x".join(map(str, v)))
def test_two_pass_kernels(src, dst, B):
    """Vertical pass (float4 kernel for the first three cases, scalar kernel for the others) and horizontal pass through a temp of exactly
    (B, dh, sw, C) elements; the same input through the single kernel as well."""
    sh, sw, C = src
    x = _input(B, sh, sw, C, seed=7 + B)
    route = "v4" if sw * C % 4 == 0 else "v"
    _check(x, dst, _resize(x.cuda(), dst, tmp=True, planar=False), f"two pass ({route}) B={B} {src}->{dst}")
    _check(x, dst, _resize(x.cuda(), dst, tmp=False, planar=False), f"single pass B={B} {src}->{dst}")


@pytest.mark.gpu
def test_two_pass_kernels_grid_stride_loops():
    """21 600 frames: a temp of 16.85 million and a destination of 18.14 million elements on grids capped at 65 536 x 256 threads, so both
    passes of the scalar route take a second trip (the float4 kernel would need a 268 MB temp for its own: left to the shapes above)."""
    src, dst = TWO_PASS_BIG
    x = _input(TWO_PASS_BIG_B, *src, seed=11)
    _check(x, dst, _resize(x.cuda(), dst, tmp=True, planar=False), f"two pass (v) B={TWO_PASS_BIG_B} {src}->{dst}")
