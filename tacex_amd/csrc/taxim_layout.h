// Where everything sits in the caller's Taxim workspaces: the render workspace of tacex_taxim_render / _deform / _render_obs, the shadow
// branch's extra regions behind it, and the part of the observation scratch the library may use.  Plain C++17 with no HIP include
// (tests/taxim_layout_check.cpp builds it with a host compiler); every offset and total is computed HERE and nowhere else, so a region
// cannot be added to a size and forgotten in an address.  All numbers are bytes from the workspace base, every region 256-byte aligned.
#pragma once
#include <stddef.h>

namespace tacex {

inline size_t taxim_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

// tacex_taxim_workspace_bytes: Z ping | Z pong | generic-path temp (B,H,W f32 each) | shift_a | shift_b | pdepth (B f32 each, written only
// with TACEX_FLAG_NO_SHIFT) | contact rows / columns (B,4 int32) of the library's own minimum pass.
// A pass of B frames walked in chunks lays every chunk out with PassLayout(n), n <= B, on the same base; `rows` is written once for the
// whole batch with PassLayout(B): it lies behind everything a chunk lays out because every term grows with the frame count.
// Z ping / Z pong are NOT complete images: a lean band level (BlurArgs::zero_bands_unread) leaves the 16-row bands it knows to be zero
// unwritten, so they hold stale data of earlier passes.  Every reader of these two buffers redirects its loads by the same contact
// ranges (the lean V-pass of the next level, issue_row of the streaming tail) and never sees them; a new reader must do the same.
struct PassLayout {
  size_t z[2], tmp, shift_a, shift_b, pdepth, rows, total;
  PassLayout(int H, int W, int B) {
    const size_t img = taxim_align((size_t)B * H * W * sizeof(float)), vec = taxim_align((size_t)B * sizeof(float));
    z[0] = 0;
    z[1] = img;
    tmp = 2 * img;
    shift_a = 3 * img;
    shift_b = shift_a + vec;
    pdepth = shift_b + vec;
    rows = pdepth + vec;
    total = rows + taxim_align((size_t)B * 4 * sizeof(int));
  }
};

// tacex_taxim_shadow_workspace_bytes, offsets from the END of the pass layout (PassLayout::total):
// deformed gel 1 | mask 1 (u8, one image slot) | gdir 1 | raw 3 | shadow 3 | tmp 3
struct ShadowLayout {
  size_t z, mask, gdir, raw, shadow, tmp, total;
  ShadowLayout(int H, int W, int B) {
    const size_t img = taxim_align((size_t)B * H * W * sizeof(float));
    z = 0;
    mask = img;
    gdir = 2 * img;
    raw = 3 * img;
    shadow = 6 * img;
    tmp = 9 * img;
    total = 12 * img;
  }
};

// The head of the caller's observation scratch (tacex_taxim_render_obs), in floats: the temp of the two-pass resize, which the fused
// tails use for their partial sums where those fit.  Behind it the float observation when the caller wants uint8.
inline size_t obs_resize_floats(int H, int W, int oh, int ow, int B) {
  const size_t v = (size_t)H * ow, h = (size_t)oh * W;
  return (size_t)B * (v > h ? v : h) * 3;
}
// what the caller provides
inline size_t obs_scratch_floats(int H, int W, int oh, int ow, int B) { return obs_resize_floats(H, W, oh, ow, B) + (size_t)B * oh * ow * 3; }

}  // namespace tacex
