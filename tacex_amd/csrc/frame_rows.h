// Device code of a frame's minimum, indentation depth (TS:116-129) and contact row / column ranges: ONE copy of every step that the
// kernels which read or fill a height map share, so that all of them report the same bits for the same map.
//   frame_rows_walk            the frame as one run of float4s, batched loads, row minima to LDS: frame_rows_kernel
//                              (taxim_kernels.hip), both passes of gel_memory_rows_kernel (gel_memory.hip)
//   FrameMinima                the two LDS arrays, a thread's four column minima, the column atomics: the two above and
//                              relief_height_map_kernel (relief_source.hip), which generates its float4s in a loop of its own
//   frame_rows_finish          minimum, press depth and the four ranges from the LDS minima: all three
//   frame_block_min +          minimum and depth alone, without ranges: frame_min_kernel, indenter_height_map_kernel
//   indentation_from_min       (taxim_kernels.hip), gel_memory_flat_kernel
// A new height-map source: frame_rows_walk, or a loop of its own around FrameMinima, then frame_rows_finish.
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

// The row and column minima of a frame: the two LDS arrays (kFrameRowsMaxH floats each, handled as float patterns) and the minima
// of the four columns a thread keeps to while cols_ok.
struct FrameMinima {
  int* rowmin_i;
  int* colmin_i;
  float cm[4];
  __device__ __forceinline__ FrameMinima(float* rowmin, float* colmin)
      : rowmin_i(reinterpret_cast<int*>(rowmin)), colmin_i(reinterpret_cast<int*>(colmin)) {}
  // everything to +inf; the block synchronises before the first minimum goes to LDS
  __device__ __forceinline__ void init(int H, int W, bool cols_ok) {
    for (int r = threadIdx.x; r < H; r += blockDim.x) rowmin_i[r] = 0x7f800000;  // +inf
    if (cols_ok)
      for (int c = threadIdx.x; c < W; c += blockDim.x) colmin_i[c] = 0x7f800000;
    cm[0] = cm[1] = cm[2] = cm[3] = INFINITY;
  }
  // minimum of one float4 of the thread's columns, the column minima kept up
  __device__ __forceinline__ float of(const v4f& v) {
    cm[0] = fminf(cm[0], v[0]); cm[1] = fminf(cm[1], v[1]); cm[2] = fminf(cm[2], v[2]); cm[3] = fminf(cm[3], v[3]);
    return fminf(fminf(v[0], v[1]), fminf(v[2], v[3]));
  }
  // (cols_ok only) the thread's columns cg .. cg + 3: the same integer atomics on the float pattern as the row minima
  __device__ __forceinline__ void columns(int cg) {
#pragma unroll
    for (int k = 0; k < 4; ++k) lds_min_f32(&colmin_i[cg + k], cm[k]);
  }
};

// The frame as ONE run of float4s, thread t takes t, t + blockDim, ... in batches of NB whose loads are issued back to back (clamped
// index instead of a predicate: one basic block), so every lane of every load is busy and several loads are in flight per thread.
// load(q) fetches what float4 q needs (q clamped to the frame), elem(data, q, valid) handles it and returns the lane's minimum
// (+inf when !valid); the row minima go to LDS here.  H * w4 float4s, w4 = W / 4; cols_ok = frame_rows_cols_ok(W).
template <int NB, class Load, class Elem>
__device__ __forceinline__ void frame_rows_walk(int H, int w4, bool cols_ok, int* rowmin_i, int lane, Load load, Elem elem) {
  using T = decltype(load(0));
  const int n4 = H * w4;
  if (cols_ok) {
    // The block size is a multiple of the row's float4 count: float4 q = base + t of a thread lies in row base / w4 + t / w4 and the
    // rows advance by blockDim / w4 per iteration - no division inside the loop (three of them, ~60 of its ~200 instructions
    // before; with the ds_bpermute reductions the pass was VALU-bound at 4.6 TB/s).
    const int rstep = blockDim.x / w4, rt = threadIdx.x / w4;
    const int w0 = threadIdx.x & ~63;
    const int rfw = __builtin_amdgcn_readfirstlane(w0 / w4), rlw = __builtin_amdgcn_readfirstlane((w0 + 63) / w4);
    for (int rb0 = 0; rb0 < H; rb0 += NB * rstep) {  // (wave-uniform trip counts: the wave reductions need every lane)
      T vb[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) vb[u] = load(min((rb0 + u * rstep) * w4 + (int)threadIdx.x, n4 - 1));
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int rb = rb0 + u * rstep;
        if (rb >= H) break;  // (block-uniform)
        const int r = rb + rt;
        const float m = elem(vb[u], rb * w4 + (int)threadIdx.x, r < H);
        if (rb + rfw < H) frame_rows_row_minima(rowmin_i, lane, m, r < H ? r : -1, rb + rfw, min(rb + rlw, H - 1));
      }
    }
  } else {
    for (int base0 = 0; base0 < n4; base0 += NB * blockDim.x) {
      T vb[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) vb[u] = load(min(base0 + u * (int)blockDim.x + (int)threadIdx.x, n4 - 1));
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int base = base0 + u * blockDim.x;
        if (base >= n4) break;  // (block-uniform)
        const int q = base + threadIdx.x;
        const bool valid = q < n4;
        const float m = elem(vb[u], q, valid);
        const int q0 = base + (threadIdx.x & ~63);
        if (q0 < n4) frame_rows_row_minima(rowmin_i, lane, m, valid ? q / w4 : -1, q0 / w4, min(q0 + 63, n4 - 1) / w4);
      }
    }
  }
}

// Minimum over the block, valid in every lane of wave 0; red: 16 floats of LDS
__device__ __forceinline__ float frame_block_min(float m, float* red) {
  m = wave_min(m);
  __syncthreads();  // (red may still be read from the previous reduction)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  float v = (threadIdx.x & 63) < (blockDim.x >> 6) ? red[threadIdx.x & 63] : INFINITY;
  return wave_min(v);
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
