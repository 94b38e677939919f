// Band-kernel argument block and the matrix-core dispatch shared by taxim_kernels.hip and taxim_mfma.hip
// (the MFMA instantiations are a translation unit of their own: they dominate the build time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tacex_internal.h"

namespace tacex {

struct BlurArgs {
  const float* src;     // (B,H,W) previous level; unused when FIRST
  const float* hm;      // (B,H,W) height map (mm)
  const float* gel;     // (H,W)
  const float* shift_a; // (B,) S = (hm - shift_a) - shift_b
  const float* shift_b; // (B,)
  const float* pdepth;  // (B,) P
  float* dst;           // (B,H,W)
  uint8_t* mask_out;    // (B,H,W) nullable
  const float* taps;    // (K,); MFMA kernel: the level's taps_mfma_dev
  int H, W, B;
  int pitch;            // LDS row pitch in float2 units (even, == 2 mod 32)
  int padx;             // left padding in float2 units (even, >= (K-1)/2)
  float contact_scale;
  int restore;          // apply Z[M] = J[M]
  int row0, nbands;     // MFMA kernel: first row and band count of this launch
  const int* rows_ext;  // (B,4) first / last frame row | first / last frame column with a non-zero level-0 input, nullable (MFMA kernel:
                        // zero-band and zero-block skipping)
  int ext_grow;         // rows by which the non-zero range of THIS level's input has grown (sum of the previous levels' radii)
  int ext_grow_x;       // columns, likewise
  int lean;             // MFMA kernel, zero gel map and rows_ext only: lanes whose pixels lie outside the contact rectangle (grown by
                        // ext_grow / ext_grow_x for a later level's input) fetch nothing and use the +0.0f / "no contact" they would have read
  int zero_bands_unread;  // with `lean`: every reader of dst knows the skipped bands from rows_ext and never loads them - a skipped band
                          // returns without storing its zeros (dst keeps whatever it held there)
  int wlds;             // MFMA kernel: launch the WLDS instantiation - band weights from the zero-padded filter behind the lane tables in
                        // `taps`, copied into LDS (host side of the switch; launch_mfma_tiles sets wlds_shared)
  int wlds_shared;      // WLDS: 1 = one copy of the filter per workgroup behind a barrier, 0 = one per wave, no barrier
};

bool mfma_supported(int k, bool first, int H, int W);
hipError_t dispatch_mfma(int k, bool first, const BlurArgs& a, hipStream_t st);

// Pipe kernel (taxim_mfma.hip): level r of one chunk of frames for every r in one launch - roles[r] is that level's argument block as
// run_blur_level fills it, over its own chunk; B == 0: the role has no chunk in this launch.  All roles: zero gel map, the same `lean`.
bool mfma_pipe_supported(const int* ks, int n, int H, int W);  // the level set (kernel sizes, level 0 first) has an instantiation
// *ok: the fused kernel holds as many workgroups per CU on the current device as the per-level launches (asked once per device and width)
hipError_t mfma_pipe_resident(const int* ks, int n, int H, int W, bool lean, bool wlds, bool* ok);
hipError_t dispatch_mfma_pipe(const int* ks, int n, int H, int W, bool lean, bool wlds, const BlurArgs* roles, hipStream_t st);

}  // namespace tacex
