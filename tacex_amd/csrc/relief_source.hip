// Relief tile library as a height-map source (tacex_height_map_from_relief; the contract is the comment of that call in
// include/tacex_hip.h, restated in tests/relief_source_ref.py).  Every env presses its own tile of a library - a height field in mm
// sampled bilinearly, on a flat, spherical or cylindrical carrier, under a pose the caller writes in place - straight into the height
// map; frame minimum, indentation depth and contact ranges of the map come out of the same launch, with the statements of the depth
// pass's row kernel (frame_rows.h).
//
// One workgroup per frame with frame_rows_block_threads(W) threads.  A thread owns float4 groups of the frame: where the block is a
// multiple of the row's float4 count it keeps to four columns and its row advances by a constant, else (x, y) advance by a constant
// pair with one carry; no division per group.  Pose, tile row and the wrap / carrier / "no tile" branches depend on blockIdx alone:
// the compiler keeps them in SGPRs and the branches are wave-uniform.  The texels are gathered with plain global loads (four taps
// per sample, neighbours along a row for neighbouring lanes at moderate scale): L2 serves a tile that fits it, the Infinity Cache a
// larger library.  4 B/px written, nothing else streamed.
// Built with -ffp-contract=off (_build.FILE_FLAGS): every product and sum of the contract is rounded to float32 on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage_args.h"
#include "tacex_internal.h"
#include "taxim_device.h"
#include "frame_rows.h"

namespace tacex {
namespace {

struct ReliefArgs {
  const float* texels;   // all tiles back to back
  const int* tiles_i;    // (P,4) [first texel, rows, cols, wrap]
  const float* tiles_f;  // (P,4) [pitch_mm, top_mm, u0, v0]
  const int* ids;        // (B,) or nullptr (tile 0)
  const float* pose;     // (B,16)
  float* hm;             // (B,H,W)
  float* fmin;           // (B,)
  float* indent;         // (B,) or nullptr
  int* rows;             // (B,4) or nullptr
  int P, H, W;
  float gel_top, far_clip, gelpad_h, gelpad_dmin;
};

// what a frame's samples need: wave-uniform, loaded once
struct ReliefFrame {
  const float* tex;  // the tile's first texel
  int Th, Tw, wrap, carrier;
  unsigned mu, mv, bu, bv;  // non-negative modulo by Tw / Th: reciprocal and bias (relief_mod)
  float wmax, hmax;         // float(Tw - 1), float(Th - 1)
  float pitch, top, u0, v0;
  float m00, m01, m02, m10, m11, m12, t0, tx, ty, R, RR, gain, du, dv;
  float base, far_clip;  // gel_top - press
};

// floor(2^32 / d) (2^32 - 1 for d == 1) and a multiple of d that is >= 2^30: with them (i + bias) % d costs two multiplies.
// n = i + bias lies in [0, 2^32) for |i| < 2^30; q = umulhi(n, m) is floor(n / d) or one less (n (2^32 / d - m) < 2^32), so the
// remainder needs one conditional subtraction.
__device__ __forceinline__ void relief_mod_setup(int d, unsigned& m, unsigned& bias) {
  m = d == 1 ? 0xffffffffu : (unsigned)(0x100000000ull / (unsigned)d);
  bias = (unsigned)d * ((0x40000000u + (unsigned)d - 1u) / (unsigned)d);
}
__device__ __forceinline__ int relief_mod(int i, unsigned d, unsigned m, unsigned bias) {
  const unsigned n = (unsigned)i + bias;
  unsigned r = n - __umulhi(n, m) * d;
  if (r >= d) r -= d;
  return (int)r;
}

// one sample of the contract at (x, y): the clamped depth
__device__ __forceinline__ float relief_sample(const ReliefFrame& f, float x, float y) {
  const float u = ((f.m00 * x) + (f.m01 * y)) + f.m02;
  const float v = ((f.m10 * x) + (f.m11 * y)) + f.m12;
  float c = 0.0f;
  if (f.carrier != 0) {
    const float t = (v - f.v0) * f.pitch;
    float q = t * t;
    if (f.carrier == 1) {
      const float s = (u - f.u0) * f.pitch;
      q = (s * s) + q;
    }
    if (!(q <= f.RR)) return f.far_clip;  // c = +inf: far clip whatever the texels say, no tap is read
    c = f.R - sqrtf(fmaxf(f.RR - q, 0.0f));
  }
  const float uu = u + f.du, vv = v + f.dv;
  float h = -INFINITY;
  if (fabsf(uu) < 1073741824.0f && fabsf(vv) < 1073741824.0f) {
    const float fu = floorf(uu), fv = floorf(vv);
    const float a = uu - fu, b = vv - fv;
    int i0 = (int)fu, j0 = (int)fv, i1, j1;
    bool inside = true;
    if (f.wrap) {
      i0 = relief_mod(i0, (unsigned)f.Tw, f.mu, f.bu);
      j0 = relief_mod(j0, (unsigned)f.Th, f.mv, f.bv);
      i1 = i0 + 1 == f.Tw ? 0 : i0 + 1;
      j1 = j0 + 1 == f.Th ? 0 : j0 + 1;
    } else {
      inside = uu >= 0.0f && uu <= f.wmax && vv >= 0.0f && vv <= f.hmax;
      i0 = min(i0, f.Tw - 1);  // (no-ops below 2^24 texels a side, where float(Tw - 1) is exact)
      j0 = min(j0, f.Th - 1);
      i1 = min(i0 + 1, f.Tw - 1);
      j1 = min(j0 + 1, f.Th - 1);
    }
    if (inside) {
      const float* r0 = f.tex + j0 * f.Tw;
      const float* r1 = f.tex + j1 * f.Tw;
      const float h00 = r0[i0], h01 = r0[i1], h10 = r1[i0], h11 = r1[i1];
      const float ga = 1.0f - a, gb = 1.0f - b;
      h = (((h00 * ga) + (h01 * a)) * gb) + (((h10 * ga) + (h11 * a)) * b);
    }
  }
  const float depth = (((f.base + c) + (f.gain * (f.top - h))) + ((f.t0 + (f.tx * x)) + (f.ty * y)));
  return depth < f.far_clip ? depth : f.far_clip;  // (a NaN: far clip)
}

template <int SAMPLES>
__device__ __forceinline__ float relief_pixel(const ReliefFrame& f, float x, float y) {
  if (SAMPLES == 1) return relief_sample(f, x, y);
  const float xm = x - 0.25f, xp = x + 0.25f, ym = y - 0.25f, yp = y + 0.25f;
  const float d0 = relief_sample(f, xm, ym), d1 = relief_sample(f, xp, ym);
  const float d2 = relief_sample(f, xm, yp), d3 = relief_sample(f, xp, yp);
  return ((d0 + d1) + (d2 + d3)) * 0.25f;
}

template <int SAMPLES>
__global__ __launch_bounds__(1024) void relief_height_map_kernel(ReliefArgs a) {
  __shared__ float rowmin[kFrameRowsMaxH];
  __shared__ float colmin[kFrameRowsMaxH];
  const int b = blockIdx.x, H = a.H, W = a.W, w4 = W >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool cols_ok = frame_rows_cols_ok(W);
  FrameMinima mn(rowmin, colmin);
  mn.init(H, W, cols_ok);

  // the frame's tile and pose (blockIdx alone: scalar loads)
  ReliefFrame f;
  const int id = a.ids ? a.ids[b] : 0;
  bool none = !(id >= 0 && id < a.P);  // no such tile: far clip everywhere, the library is not touched
  f.far_clip = a.far_clip;
  if (!none) {
    const int* ti = a.tiles_i + 4 * (size_t)id;
    const float* tf = a.tiles_f + 4 * (size_t)id;
    f.tex = a.texels + ti[0];
    f.Th = ti[1]; f.Tw = ti[2]; f.wrap = ti[3];
    f.pitch = tf[0]; f.top = tf[1]; f.u0 = tf[2]; f.v0 = tf[3];
    none = f.Th < 1 || f.Tw < 1 || ti[0] < 0;  // (a table row the host would not have written)
  }
  if (!none) {
    relief_mod_setup(f.Tw, f.mu, f.bu);
    relief_mod_setup(f.Th, f.mv, f.bv);
    f.wmax = (float)(f.Tw - 1); f.hmax = (float)(f.Th - 1);
    const float* p = a.pose + 16 * (size_t)b;
    f.m00 = p[0]; f.m01 = p[1]; f.m02 = p[2]; f.m10 = p[3]; f.m11 = p[4]; f.m12 = p[5];
    f.base = a.gel_top - p[6];
    f.t0 = p[7]; f.tx = p[8]; f.ty = p[9];
    f.carrier = p[10] == 1.0f ? 1 : (p[10] == 2.0f ? 2 : 0);
    f.R = p[11]; f.RR = f.R * f.R;
    f.gain = p[12]; f.du = p[13]; f.dv = p[14];
  }
  v4f* __restrict__ out4 = reinterpret_cast<v4f*>(a.hm + (size_t)b * ((size_t)H * W));
  // one float4 of the frame at columns x .. x + 3 of row y: computed, stored, the lane's minimum returned
  auto group = [&](int q, int x, int y) -> float {
    v4f o;
    if (none) {
      o[0] = o[1] = o[2] = o[3] = f.far_clip;
    } else {
      const float yf = (float)y;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = relief_pixel<SAMPLES>(f, (float)(x + k), yf);
    }
    out4[q] = o;
    return mn.of(o);
  };
  __syncthreads();
  if (cols_ok) {
    // the block is a multiple of the row's float4 count: a thread keeps its columns, its row advances by blockDim / w4
    const int rstep = blockDim.x / w4, rt = threadIdx.x / w4, x = ((int)threadIdx.x - rt * w4) << 2;
    const int w0 = threadIdx.x & ~63;
    const int rfw = __builtin_amdgcn_readfirstlane(w0 / w4), rlw = __builtin_amdgcn_readfirstlane((w0 + 63) / w4);
    for (int rb = 0; rb < H; rb += rstep) {  // (block-uniform trip count: the wave reductions need every lane)
      const int r = rb + rt;
      const float m = r < H ? group(rb * w4 + (int)threadIdx.x, x, r) : INFINITY;
      if (rb + rfw < H) frame_rows_row_minima(mn.rowmin_i, lane, m, r < H ? r : -1, rb + rfw, min(rb + rlw, H - 1));
    }
    mn.columns(x);
  } else {
    // any other row length: float4 q = t, t + blockDim, ...; (x4, y) advance by (sx, sy) with one carry
    const int n4 = H * w4;
    const int sy = blockDim.x / w4, sx = blockDim.x - sy * w4;
    int y = threadIdx.x / w4, x4 = threadIdx.x - y * w4;
    const int w0 = threadIdx.x & ~63;
    int yf0 = __builtin_amdgcn_readfirstlane(w0 / w4), xf0 = __builtin_amdgcn_readfirstlane(w0 - (w0 / w4) * w4);  // the wave's first float4
    for (int base = 0; base < n4; base += blockDim.x) {
      const int q = base + threadIdx.x;
      const bool valid = q < n4;
      const float m = valid ? group(q, x4 << 2, y) : INFINITY;
      if (base + w0 < n4) {
        const int ql = min(base + w0 + 63, n4 - 1) - (base + w0);  // the wave's last float4, counted from its first
        frame_rows_row_minima(mn.rowmin_i, lane, m, valid ? y : -1, yf0, yf0 + (xf0 + ql) / w4);
      }
      x4 += sx; y += sy;
      if (x4 >= w4) { x4 -= w4; ++y; }
      xf0 += sx; yf0 += sy;
      if (xf0 >= w4) { xf0 -= w4; ++yf0; }
    }
  }
  __syncthreads();
  if (wave == (int)(blockDim.x >> 6) - 1)
    frame_rows_finish(rowmin, colmin, H, W, cols_ok, lane, b, a.gelpad_h, a.gelpad_dmin, nullptr, a.fmin, a.indent, a.rows);
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_height_map_from_relief(const float* texels_dev, const int32_t* tiles_i_dev, const float* tiles_f_dev, int num_tiles,
                                            const int32_t* relief_ids_dev, const float* pose_dev, float gel_top_mm, float far_clip_mm,
                                            float gelpad_height_m, float gelpad_to_camera_min_distance_m, float* hm_mm_dev,
                                            float* frame_min_dev, float* indent_mm_dev, int32_t* frame_rows_dev, int num_frames,
                                            int height, int width, int samples, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_height_map_from_relief";
  if (null_arg(fn, "texels_dev", texels_dev) || null_arg(fn, "tiles_i_dev", tiles_i_dev) || null_arg(fn, "tiles_f_dev", tiles_f_dev) ||
      null_arg(fn, "pose_dev", pose_dev) || null_arg(fn, "hm_mm_dev", hm_mm_dev) || null_arg(fn, "frame_min_dev", frame_min_dev)) return 2;
  if (not_positive(fn, "num_tiles", num_tiles) || not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) ||
      not_positive(fn, "width", width)) return 2;
  if (not_frame_rows_geometry(fn, height, width)) return 2;
  if (samples != 1 && samples != 4) { set_error("%s: samples = %d (must be 1 or 4)", fn, samples); return 2; }
  if (not_aligned16(fn, "hm_mm_dev", hm_mm_dev)) return 2;
  ReliefArgs a{};
  a.texels = texels_dev; a.tiles_i = tiles_i_dev; a.tiles_f = tiles_f_dev; a.ids = relief_ids_dev; a.pose = pose_dev;
  a.hm = hm_mm_dev; a.fmin = frame_min_dev; a.indent = indent_mm_dev; a.rows = frame_rows_dev;
  a.P = num_tiles; a.H = height; a.W = width;
  a.gel_top = gel_top_mm; a.far_clip = far_clip_mm; a.gelpad_h = gelpad_height_m; a.gelpad_dmin = gelpad_to_camera_min_distance_m;
  const dim3 grid((unsigned int)num_frames), block(frame_rows_block_threads(width));
  hipStream_t st = (hipStream_t)stream;
  if (samples == 1) hipLaunchKernelGGL(relief_height_map_kernel<1>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(relief_height_map_kernel<4>, grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "relief_height_map_kernel");
}
