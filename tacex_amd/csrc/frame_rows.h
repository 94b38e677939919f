// Device code of the contact row / column range of a frame, shared by the depth pass's row kernel (frame_rows_kernel,
// taxim_kernels.hip) and the gel memory kernel (gel_memory.hip): both keep the row and column minima of a frame in LDS and
// derive frame minimum, indentation depth (TS:116-129) and the four ranges from them with the statements below, so that the two
// report the same bits for the same map.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "taxim_device.h"

namespace tacex {

constexpr int kFrameRowsMaxH = 2048;  // rows (and columns) whose minima fit the two LDS arrays

// Block size of a row kernel: a multiple of the row's float4 count, so that every thread keeps to four columns (whole waves, enough
// of them; else 1024 threads and the kernel reports every column as contact).
inline int frame_rows_block_threads(int W) {
  const int w4 = W >> 2;
  int nt = w4 <= 1024 ? (1024 / w4) * w4 : 1024;
  if (nt < 512 || (nt & 63)) nt = 1024;
  return nt;
}

// (block-uniform) true when a thread's float4s t, t + blockDim, ... all lie in ONE column group and the columns fit LDS
__device__ __forceinline__ bool frame_rows_cols_ok(int W) { return W <= kFrameRowsMaxH && (blockDim.x % (W >> 2)) == 0; }

// Minimum into an LDS slot through integer atomics on the float pattern (patterns of values >= 0 or +inf order like the values;
// negative ones the other way round as unsigned).  A minimum does not depend on the order of its operands.
__device__ __forceinline__ void lds_min_f32(int* slot, float v) {
  if (v >= 0.0f) atomicMin(slot, __float_as_int(v + 0.0f));  // (+ 0: a -0 must not pass for INT_MIN)
  else atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(v));
}

// A wave's 64 consecutive float4s lie in rows r_first .. r_last (wave-uniform): reduce inside the wave per row (DPP scan, the
// minimum lands in lane 63), one LDS atomic per row and wave.  m: the lane's minimum, r: its row (-1: none).
__device__ __forceinline__ void frame_rows_row_minima(int* rowmin_i, int lane, float m, int r, int r_first, int r_last) {
  for (int rr = r_first; rr <= r_last; ++rr) {
    const float mr = wave_scan_min_lane63(r == rr ? m : INFINITY);
    if (lane == 63) lds_min_f32(&rowmin_i[rr], mr);
  }
}

// TS:116-129: indentation depth [mm] of a frame whose minimum is m [mm]
__device__ __forceinline__ float indentation_from_min(float m, float gelpad_h, float gelpad_dmin) {
  float d = m / 1000.0f - gelpad_dmin;
  d = d < 0.0f ? 0.0f : d;
  return d <= gelpad_h ? (gelpad_h - d) * 1000.0f : 0.0f;
}

// One wave (all 64 lanes), after the block has synchronised on the minima: frame minimum, press depth and the ranges.
// indent_out != nullptr: the press depth is the indentation depth computed here, else press_in[b] (0 without it).
// rows_out may be nullptr (minimum and depth alone).
__device__ __forceinline__ void frame_rows_finish(const float* rowmin, const float* colmin, int H, int W, bool cols_ok, int lane, int b,
                                                  float gelpad_h, float gelpad_dmin, const float* __restrict__ press_in,
                                                  float* __restrict__ fmin_out, float* __restrict__ indent_out,
                                                  int* __restrict__ rows_out) {
  float m = INFINITY;
  for (int r = lane; r < H; r += 64) m = fminf(m, rowmin[r]);
  m = wave_min(m);
  float press = 0.0f;
  if (indent_out) press = indentation_from_min(m, gelpad_h, gelpad_dmin);
  else if (press_in) press = press_in[b];
  int lo = H, hi = -1;
  for (int r = lane; r < H; r += 64)
    if (((rowmin[r] - m) - press) < 0.0f) { lo = min(lo, r); hi = max(hi, r); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
  int clo = 0, chi = W - 1;
  if (cols_ok) {
    clo = W; chi = -1;
    for (int c = lane; c < W; c += 64)
      if (((colmin[c] - m) - press) < 0.0f) { clo = min(clo, c); chi = max(chi, c); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { clo = min(clo, __shfl_xor(clo, o, 64)); chi = max(chi, __shfl_xor(chi, o, 64)); }
  }
  if (lane == 0) {
    fmin_out[b] = m;
    if (indent_out) indent_out[b] = press;
    if (rows_out) { rows_out[4 * b] = lo; rows_out[4 * b + 1] = hi; rows_out[4 * b + 2] = clo; rows_out[4 * b + 3] = chi; }
  }
}

}  // namespace tacex
