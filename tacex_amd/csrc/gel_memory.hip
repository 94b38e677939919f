// Gel memory on the optical path: the viscoelastic residual imprint of the elastomer, per env (tacex_gel_memory; the contract is
// the comment of that call in include/tacex_hip.h, restated in tests/gel_memory_ref.py).  The height map of a step is rewritten in
// place from K Prony branches of per-pixel state; frame minimum, indentation depth and contact ranges of the REWRITTEN map come out
// of the same launch, with the statements of the depth pass's row kernel (frame_rows.h).
//
// One workgroup per frame, two passes:
//   pass 1 reads the map (4 B/px), keeps its row / column minima in LDS and finds out whether any pixel is pressed (d > 0).  A frame
//          without one whose live flag is 0 is DEAD: its state is all zero and stays so, its map is left as it is - the minima of
//          pass 1 are its outputs and no state byte moves.  The common case at sparse contact.
//   pass 2 (live frames) streams the map again (L2 / MALL permitting) with the K state planes, 16 bytes per lane where W % 4 == 0,
//          writes both and redoes the minima on what it writes: 4 + 4 + 8 K + 4 B/px in all.
// No atomics across workgroups, a fixed order inside one: the same inputs give the same bits in any batch.
// Built with -ffp-contract=off (_build.FILE_FLAGS): a * m + c * d is two products and a sum, each rounded to float32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage_args.h"
#include "tacex_internal.h"
#include "taxim_device.h"
#include "frame_rows.h"

namespace tacex {
namespace {

struct GelArgs {
  float* hm;           // (B,H,W) in place
  float* state;        // (B,K,H,W)
  int* live;           // (B,)
  const float* coef;   // (P,8) [a1, c1, a2, c2, floor_mm, 0, 0, 0]
  const int* ids;      // (B,) or nullptr (profile 0)
  float* fmin;         // (B,)
  float* indent;       // (B,)
  int* rows;           // (B,4) or nullptr
  int P, H, W;
  float z0, gelpad_h, gelpad_dmin;
};

struct GelCoef { float a1, c1, a2, c2, floor_mm; };

__device__ __forceinline__ GelCoef gel_coef(const GelArgs& a, int b) {
  GelCoef c{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // an id outside [0, P): the all-zero profile
  if (const float* p = stage_row(a.coef, a.ids, a.P, 8, b)) {
    c.a1 = p[0]; c.c1 = p[1]; c.a2 = p[2]; c.c2 = p[3]; c.floor_mm = p[4];
  }
  return c;
}

__device__ __forceinline__ bool gel_pressed(float hm, float z0) { return (z0 - hm) > 0.0f; }  // (false for a NaN)

// one pixel of the contract: returns the output height, updates the branch states, nz |= "a state element is non-zero"
template <int K>
__device__ __forceinline__ float gel_pixel(float hm, float& m1, float& m2, const GelCoef& c, float z0, int& nz) {
  const float t = z0 - hm;
  const float d = t > 0.0f ? t : 0.0f;
  m1 = (c.a1 * m1) + (c.c1 * d);
  if (d == 0.0f && m1 < c.floor_mm) m1 = 0.0f;
  float M = m1;
  nz |= (m1 != 0.0f);
  if (K == 2) {
    m2 = (c.a2 * m2) + (c.c2 * d);
    if (d == 0.0f && m2 < c.floor_mm) m2 = 0.0f;
    M = m1 + m2;
    nz |= (m2 != 0.0f);
  }
  const float r = z0 - M;
  return (M > 0.0f && r < hm) ? r : hm;
}

template <int K> struct GelQuad { v4f h, m1, m2; };

// W % 4 == 0 and H <= kFrameRowsMaxH: minima per row and column, the outputs of frame_rows_kernel
template <int K>
__global__ __launch_bounds__(1024) void gel_memory_rows_kernel(GelArgs a) {
  __shared__ float rowmin[kFrameRowsMaxH];
  __shared__ float colmin[kFrameRowsMaxH];
  __shared__ int flag[2];  // [0] a pixel is pressed, [1] a state element is non-zero after the update
  const int b = blockIdx.x, H = a.H, W = a.W, w4 = W >> 2;
  const size_t npix = (size_t)H * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool cols_ok = frame_rows_cols_ok(W);
  const float z0 = a.z0;
  v4f* __restrict__ hm4 = reinterpret_cast<v4f*>(a.hm + (size_t)b * npix);
  FrameMinima mn(rowmin, colmin);
  mn.init(H, W, cols_ok);
  if (threadIdx.x < 2) flag[threadIdx.x] = 0;
  __syncthreads();
  // pass 1: the map alone
  int pressed = 0;
  frame_rows_walk<4>(H, w4, cols_ok, mn.rowmin_i, lane, [&](int q) { return hm4[q]; },
                     [&](const v4f& v, int q, bool valid) -> float {
                       if (!valid) return INFINITY;
                       pressed |= gel_pressed(v[0], z0) | gel_pressed(v[1], z0) | gel_pressed(v[2], z0) | gel_pressed(v[3], z0);
                       return mn.of(v);
                     });
  if (cols_ok) mn.columns((threadIdx.x % w4) * 4);
  if (pressed) flag[0] = 1;
  __syncthreads();
  const bool dead = flag[0] == 0 && a.live[b] == 0;  // (block-uniform)
  if (!dead) {
    // pass 2: map and state, rewritten; minima of what is written
    const GelCoef c = gel_coef(a, b);
    v4f* __restrict__ s1 = reinterpret_cast<v4f*>(a.state + ((size_t)b * K) * npix);
    v4f* __restrict__ s2 = reinterpret_cast<v4f*>(a.state + ((size_t)b * K + (K - 1)) * npix);
    mn.init(H, W, cols_ok);
    __syncthreads();
    int nz = 0;
    frame_rows_walk<2>(H, w4, cols_ok, mn.rowmin_i, lane,
                       [&](int q) {
                         GelQuad<K> g;
                         g.h = hm4[q]; g.m1 = s1[q];
                         if (K == 2) g.m2 = s2[q];
                         return g;
                       },
                       [&](GelQuad<K>& g, int q, bool valid) -> float {
                         if (!valid) return INFINITY;
                         v4f o;
       #pragma unroll
                         for (int k = 0; k < 4; ++k) {
                           float m1 = g.m1[k], m2 = K == 2 ? g.m2[k] : 0.0f;
                           o[k] = gel_pixel<K>(g.h[k], m1, m2, c, z0, nz);
                           g.m1[k] = m1;
                           if (K == 2) g.m2[k] = m2;
                         }
                         hm4[q] = o; s1[q] = g.m1;
                         if (K == 2) s2[q] = g.m2;
                         return mn.of(o);
                       });
    if (cols_ok) mn.columns((threadIdx.x % w4) * 4);
    if (nz) flag[1] = 1;
    __syncthreads();
    if (threadIdx.x == 0) a.live[b] = flag[1];
  }
  if (wave == 0)
    frame_rows_finish(rowmin, colmin, H, W, cols_ok, lane, b, a.gelpad_h, a.gelpad_dmin, nullptr, a.fmin, a.indent, a.rows);
}

// Any other geometry (W % 4 != 0: scalar; H > kFrameRowsMaxH: VEC): the frame minimum alone, every row and column reported as
// contact - what tacex_indentation_depth does there (frame_min_kernel + fill_rows_kernel).
template <int K, bool VEC>
__global__ __launch_bounds__(1024) void gel_memory_flat_kernel(GelArgs a) {
  __shared__ float red[16];
  __shared__ int flag[2];
  typedef typename std::conditional<VEC, v4f, float>::type T;
  constexpr int N = VEC ? 4 : 1;
  const int b = blockIdx.x;
  const size_t npix = (size_t)a.H * a.W;
  const size_t n = npix / N;  // (VEC: W % 4 == 0)
  const float z0 = a.z0;
  T* __restrict__ hm = reinterpret_cast<T*>(a.hm + (size_t)b * npix);
  if (threadIdx.x < 2) flag[threadIdx.x] = 0;
  auto lane_of = [](const T& v, int k) -> float { if constexpr (VEC) return v[k]; else return v; };
  float m = INFINITY;
  int pressed = 0;
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
    const T v = hm[i];
#pragma unroll
    for (int k = 0; k < N; ++k) { const float h = lane_of(v, k); pressed |= gel_pressed(h, z0); m = fminf(m, h); }
  }
  m = frame_block_min(m, red);  // (its barriers also order flag's initialisation)
  if (pressed) flag[0] = 1;
  __syncthreads();
  const bool dead = flag[0] == 0 && a.live[b] == 0;  // (block-uniform)
  if (!dead) {
    const GelCoef c = gel_coef(a, b);
    T* __restrict__ s1 = reinterpret_cast<T*>(a.state + ((size_t)b * K) * npix);
    T* __restrict__ s2 = reinterpret_cast<T*>(a.state + ((size_t)b * K + (K - 1)) * npix);
    int nz = 0;
    m = INFINITY;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
      const T h = hm[i];
      T p1 = s1[i], p2 = p1, o = h;
      if (K == 2) p2 = s2[i];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        float m1 = lane_of(p1, k), m2 = K == 2 ? lane_of(p2, k) : 0.0f;
        const float r = gel_pixel<K>(lane_of(h, k), m1, m2, c, z0, nz);
        if constexpr (VEC) { o[k] = r; p1[k] = m1; p2[k] = m2; } else { o = r; p1 = m1; p2 = m2; }
        m = fminf(m, r);
      }
      hm[i] = o; s1[i] = p1;
      if (K == 2) s2[i] = p2;
    }
    m = frame_block_min(m, red);
    if (nz) flag[1] = 1;
    __syncthreads();
    if (threadIdx.x == 0) a.live[b] = flag[1];
  }
  if (threadIdx.x == 0) {
    a.fmin[b] = m;
    a.indent[b] = indentation_from_min(m, a.gelpad_h, a.gelpad_dmin);
    if (a.rows) { a.rows[4 * b] = 0; a.rows[4 * b + 1] = a.H - 1; a.rows[4 * b + 2] = 0; a.rows[4 * b + 3] = a.W - 1; }
  }
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_gel_memory(float* hm_mm_dev, float* state_dev, int32_t* live_dev, const float* coef_dev, int num_profiles,
                                const int32_t* profile_ids_dev, float z0_mm, float gelpad_height_m,
                                float gelpad_to_camera_min_distance_m, float* frame_min_dev, float* indent_mm_dev,
                                int32_t* frame_rows_dev, int num_frames, int height, int width, int terms, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_gel_memory";
  if (null_arg(fn, "hm_mm_dev", hm_mm_dev) || null_arg(fn, "state_dev", state_dev) || null_arg(fn, "live_dev", live_dev) ||
      null_arg(fn, "coef_dev", coef_dev) || null_arg(fn, "frame_min_dev", frame_min_dev) || null_arg(fn, "indent_mm_dev", indent_mm_dev)) return 2;
  if (terms != 1 && terms != 2) { set_error("tacex_gel_memory: terms = %d (must be 1 or 2)", terms); return 2; }
  if (not_positive(fn, "num_profiles", num_profiles) || not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) ||
      not_positive(fn, "width", width)) return 2;
  const bool vec = width % 4 == 0;
  if (vec && ((uintptr_t)hm_mm_dev % 16 != 0 || (uintptr_t)state_dev % 16 != 0)) {
    set_error("tacex_gel_memory: hm_mm_dev and state_dev must be 16-byte aligned when width %% 4 == 0");
    return 2;
  }
  GelArgs a{};
  a.hm = hm_mm_dev; a.state = state_dev; a.live = live_dev; a.coef = coef_dev; a.ids = profile_ids_dev;
  a.fmin = frame_min_dev; a.indent = indent_mm_dev; a.rows = frame_rows_dev;
  a.P = num_profiles; a.H = height; a.W = width;
  a.z0 = z0_mm; a.gelpad_h = gelpad_height_m; a.gelpad_dmin = gelpad_to_camera_min_distance_m;
  const dim3 grid((unsigned int)num_frames);
  hipStream_t st = (hipStream_t)stream;
  const char* what;
  if (vec && height <= kFrameRowsMaxH) {
    what = "gel_memory_rows_kernel";
    const dim3 block(frame_rows_block_threads(width));
    if (terms == 1) hipLaunchKernelGGL(gel_memory_rows_kernel<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(gel_memory_rows_kernel<2>, grid, block, 0, st, a);
  } else {
    what = "gel_memory_flat_kernel";
    const dim3 block(1024);
    if (vec) {
      if (terms == 1) hipLaunchKernelGGL((gel_memory_flat_kernel<1, true>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((gel_memory_flat_kernel<2, true>), grid, block, 0, st, a);
    } else {
      if (terms == 1) hipLaunchKernelGGL((gel_memory_flat_kernel<1, false>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((gel_memory_flat_kernel<2, false>), grid, block, 0, st, a);
    }
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, what);
}
