// Sensor lens model (tacex_lens_model, tacex_lens_camera_model, tacex_lens_points): what the short wide-angle lens of a GelSight
// and the mounting of one unit do to the rendered frame - Brown-Conrady distortion, a mounting shift / rotation / scale, vignetting
// and a radially growing softness - as ONE gather per frame batch.  The contract - the order of every float32 operation - is the
// comment of tacex_lens_model in include/tacex_hip.h; tests/lens_model_ref.py restates that comment in NumPy and the two agree bit
// for bit.  This file is compiled with -ffp-contract=off (tacex_amd/_build.py): every product and sum below rounds on its own.
//
// Per pixel: ~45 float32 operations for the source position, then one bilinear tap (4 source pixels, four 12-byte loads) or, where
// the frame's profile has softness, the mean of four taps.  The taps are 12-byte NHWC pixels at data-dependent addresses: plain
// dword loads (merged to dwordx3), clamped to the frame (nothing outside the input is read).  Neighbouring pixels read neighbouring
// source pixels, so the taps hit the vector cache and L2; HBM sees each input line about once.
// A workgroup of 256 threads takes 1024 consecutive pixels of ONE frame (grid = blocks per frame x frames): the frame's lens id,
// lens row and camera row are wave-uniform loads, and the one-tap / four-tap branch is uniform.  Two assignments of pixels to lanes:
//   lens_model_kernel  a thread takes ONE group of four consecutive output pixels - the group the camera model addresses its Philox
//                      draws by (camera_group.h), so the fused kernels hand a gathered group straight to camera_group() and are
//                      bit-equal to the two launches.  Vector path (output base 16-byte aligned and H W % 4 == 0; the input's
//                      alignment does not matter): three 16-byte stores (float32) or one 12-byte store of the packed bytes (uint8);
//                      scalar path: dword / byte stores, bounds-checked per pixel.  Same bits;
//   lens_rows_kernel   the lens alone on the vector path: lane l of a wave takes pixels l, l + 64, l + 128, l + 192 of the wave's
//                      256, so that the lanes of one load or store instruction touch neighbouring pixels.  Same bits.
// No LDS.  Value offsets are 64-bit.  A gather cannot run in place: out_dev == rgb_dev is refused.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "camera_group.h"
#include "stage_args.h"
#include "tacex_hip.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

constexpr int kLensBlock = 256;

struct LensRow {
  float k1, k2, p1, p2, e00, e01, e10, e11, tx, ty, cx, cy, v1, v2, b0, b2;
};

struct LensArgs {
  const float* rgb;       // (B,H,W,3)
  const float* profiles;  // (P,16)
  const int32_t* ids;     // (B,) or nullptr
  void* out;              // (B,H,W,3) float32, or uint8 (fused)
  unsigned int npix;      // H W (< 2^31)
  unsigned int groups;    // ceil(npix / 4)
  unsigned int blocks_per_frame;
  int num_profiles;
  int H, W;
  float s, hw, hh;        // 2 / W (divided on the host), W / 2, H / 2
  CameraTable cam;        // the fused kernels only
};

__device__ inline LensRow load_lens_row(const float* profiles, const int32_t* ids, int num_profiles, unsigned int frame) {
  LensRow L{};  // an id outside [0, P): the identity profile, all zero
  const int id = ids ? ids[frame] : 0;  // (written out, not stage_row(): profiles/stage_layer_isa.md)
  if (id >= 0 && id < num_profiles) {
    const float* __restrict__ r = profiles + (size_t)id * 16;
    L.k1 = r[0]; L.k2 = r[1]; L.p1 = r[2]; L.p2 = r[3]; L.e00 = r[4]; L.e01 = r[5]; L.e10 = r[6]; L.e11 = r[7];
    L.tx = r[8]; L.ty = r[9]; L.cx = r[10]; L.cy = r[11]; L.v1 = r[12]; L.v2 = r[13]; L.b0 = r[14]; L.b2 = r[15];
  }
  return L;
}

// one bilinear tap at (u, v) of the frame at `f`, edge replicate
__device__ inline void lens_tap(const float* __restrict__ f, int H, int W, float u, float v, float c[3]) {
  u = fabsf(u) <= FLT_MAX ? u : 0.0f;  // not finite: 0
  v = fabsf(v) <= FLT_MAX ? v : 0.0f;
  const float x0f = floorf(u), y0f = floorf(v);
  const float fx = u - x0f, fy = v - y0f;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  // clamped in float before the conversion (a far-away position must not overflow an int), then to the frame
  int x0 = (int)fminf(fmaxf(x0f, -1.0f), (float)W), y0 = (int)fminf(fmaxf(y0f, -1.0f), (float)H);
  const int x1 = min(max(x0 + 1, 0), W - 1), y1 = min(max(y0 + 1, 0), H - 1);
  x0 = min(max(x0, 0), W - 1); y0 = min(max(y0, 0), H - 1);
  const unsigned int r0 = (unsigned int)y0 * (unsigned int)W, r1 = (unsigned int)y1 * (unsigned int)W;  // < npix
  const float* pa = f + (size_t)(r0 + (unsigned int)x0) * 3;
  const float* pb = f + (size_t)(r0 + (unsigned int)x1) * 3;
  const float* pc = f + (size_t)(r1 + (unsigned int)x0) * 3;
  const float* pd = f + (size_t)(r1 + (unsigned int)x1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = (pa[k] * gx + pb[k] * fx) * gy + (pc[k] * gx + pd[k] * fx) * fy;
}

// output pixel (i, j) -> its colour through the lens
template <bool kSoft>
__device__ inline void lens_pixel(const LensArgs& a, const LensRow& L, const float* __restrict__ f, int i, int j, float c[3]) {
  const float jf = (float)j, fi = (float)i;
  const float px = ((jf + 0.5f) - a.hw) - L.cx, py = ((fi + 0.5f) - a.hh) - L.cy;
  const float xn = px * a.s, yn = py * a.s;
  const float xx = xn * xn, yy = yn * yn, xy = xn * yn;
  const float r2 = xx + yy;
  const float rad = (L.k1 + L.k2 * r2) * r2;
  const float dx = (xn * rad + (L.p1 + L.p1) * xy) + L.p2 * (r2 + (xx + xx));
  const float dy = (yn * rad + L.p1 * (r2 + (yy + yy))) + (L.p2 + L.p2) * xy;
  const float ou = ((L.e00 * px + L.e01 * py) + a.hw * dx) + L.tx;
  const float ov = ((L.e10 * px + L.e11 * py) + a.hw * dy) + L.ty;
  const float u = jf + ou, v = fi + ov;
  if constexpr (kSoft) {
    const float hs = 0.5f * fminf(fmaxf(L.b0 + L.b2 * r2, 0.0f), 4.0f);
    const float um = u - hs, up = u + hs, vm = v - hs, vp = v + hs;
    float t0[3], t1[3], t2[3], t3[3];
    lens_tap(f, a.H, a.W, um, vm, t0);
    lens_tap(f, a.H, a.W, up, vm, t1);
    lens_tap(f, a.H, a.W, um, vp, t2);
    lens_tap(f, a.H, a.W, up, vp, t3);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (((t0[k] + t1[k]) + t2[k]) + t3[k]) * 0.25f;
  } else {
    lens_tap(f, a.H, a.W, u, v, c);
  }
  const float g = fminf(fmaxf(1.0f + (L.v1 + L.v2 * r2) * r2, 0.0f), 1.0f);
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = g * c[k];
}

// the first n / 3 pixels of group g of the frame at `f` through the lens -> px[12] (the rest 0)
template <bool kSoft>
__device__ inline void lens_group(const LensArgs& a, const LensRow& L, const float* __restrict__ f, unsigned int g, int n, float px[12]) {
  const unsigned int p0 = g * 4u;
  int i = (int)(p0 / (unsigned int)a.W);
  int j = (int)(p0 - (unsigned int)i * (unsigned int)a.W);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (3 * q < n) {
      lens_pixel<kSoft>(a, L, f, i, j, px + 3 * q);
    } else {
      px[3 * q] = px[3 * q + 1] = px[3 * q + 2] = 0.0f;
    }
    if (++j == a.W) { j = 0; ++i; }
  }
}

// kMode 0: the lens alone (float32); 1: lens + camera model, float32; 2: lens + camera model, uint8.
// Four waves per SIMD asked for: left alone the scheduler hoists all 48 (one tap) or 192 (four taps) loads of a thread's four pixels
// and takes 185 VGPRs (2 waves per SIMD); at 4 it keeps 112 - 114 without scratch, from 6 on it spills.
template <int kMode, bool kVec>
__global__ __launch_bounds__(kLensBlock, 4) void lens_model_kernel(LensArgs a) {
  const unsigned int frame = blockIdx.x / a.blocks_per_frame;
  const unsigned int g = (blockIdx.x - frame * a.blocks_per_frame) * kLensBlock + threadIdx.x;
  if (g >= a.groups) return;
  const LensRow L = load_lens_row(a.profiles, a.ids, a.num_profiles, frame);
  const unsigned int left = a.npix - g * 4u;
  const int n = (!kVec && left < 4u) ? (int)left * 3 : 12;  // values of this group inside the frame
  const size_t f0 = (size_t)frame * (size_t)a.npix * 3;     // first value of the frame in the batch
  const float* __restrict__ f = a.rgb + f0;
  float px[12];
  if (L.b0 != 0.0f || L.b2 != 0.0f) lens_group<true>(a, L, f, g, n, px);  // uniform over the workgroup
  else lens_group<false>(a, L, f, g, n, px);
  if constexpr (kMode != 0) {
    const CameraProfileRow p = load_camera_profile(a.cam, frame);
    camera_group(a.cam, p, a.cam.frame_offset + frame, g, px);
  }
  const size_t v0 = f0 + (size_t)g * 12;
  if constexpr (kVec) store_group_vec<kMode == 2>(a.out, v0, px);
  else store_group_scalar<kMode == 2>(a.out, v0, px, n);
}

// The lens alone on the vector path (H W % 4 == 0, 16-byte aligned output).  A wave owns 256 consecutive pixels and lane l takes
// pixels l, l + 64, l + 128, l + 192 of them: the 64 lanes of a tap load read neighbouring 12-byte pixels (about 768 contiguous
// bytes, 6 - 7 cache lines) where one group per lane reads every fourth pixel (3 KiB, 24 - 48 lines per instruction), and a store
// instruction writes 768 contiguous bytes.  Same bits as lens_model_kernel<0, .>: the arithmetic per pixel is the same.  Measured on
// 2048 frames of 320 x 240: 0.81 ms against 1.30 ms for one group per lane.  The fused kernels keep one group per
// lane: handing the colours to the camera model's group layout through LDS made them slower than the two launches (1.51 against
// 1.35 ms for lens_model_kernel<2, true>).
__global__ __launch_bounds__(kLensBlock, 4) void lens_rows_kernel(LensArgs a) {
  const unsigned int frame = blockIdx.x / a.blocks_per_frame;
  const unsigned int lane = threadIdx.x & 63u;
  const unsigned int first = (blockIdx.x - frame * a.blocks_per_frame) * (kLensBlock * 4u) + (threadIdx.x & ~63u) * 4u;  // of the wave
  const LensRow L = load_lens_row(a.profiles, a.ids, a.num_profiles, frame);
  const size_t f0 = (size_t)frame * (size_t)a.npix * 3;  // first value of the frame in the batch
  const float* __restrict__ f = a.rgb + f0;
  float* __restrict__ out = static_cast<float*>(a.out) + f0;
  const bool soft = L.b0 != 0.0f || L.b2 != 0.0f;  // uniform over the workgroup
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned int p = first + lane + 64u * q;
    if (p < a.npix) {
      const int i = (int)(p / (unsigned int)a.W);
      const int j = (int)(p - (unsigned int)i * (unsigned int)a.W);
      float c[3];
      if (soft) lens_pixel<true>(a, L, f, i, j, c);
      else lens_pixel<false>(a, L, f, i, j, c);
      float* dst = out + (size_t)p * 3;
      dst[0] = c[0]; dst[1] = c[1]; dst[2] = c[2];
    }
  }
}

struct PointArgs {
  const double* xy;       // (B,N,2)
  const float* profiles;  // (P,16)
  const int32_t* ids;     // (B,) or nullptr
  double* out;            // (B,N,2); may be xy
  unsigned int n;         // points per frame
  unsigned int blocks_per_frame;
  int num_profiles;
  double s, hw, hh;       // 2 / W (divided on the host), W / 2, H / 2
};

// one point per thread: q + displacement(q) = xy by TACEX_LENS_POINT_ITERATIONS rounds of q <- xy - displacement(q), float64
__global__ __launch_bounds__(kLensBlock) void lens_points_kernel(PointArgs a) {
  const unsigned int frame = blockIdx.x / a.blocks_per_frame;
  const unsigned int m = (blockIdx.x - frame * a.blocks_per_frame) * kLensBlock + threadIdx.x;
  if (m >= a.n) return;
  const LensRow L = load_lens_row(a.profiles, a.ids, a.num_profiles, frame);
  const double k1 = L.k1, k2 = L.k2, p1 = L.p1, p2 = L.p2, e00 = L.e00, e01 = L.e01, e10 = L.e10, e11 = L.e11;
  const double tx = L.tx, ty = L.ty, cx = L.cx, cy = L.cy;
  const size_t o = ((size_t)frame * a.n + m) * 2;
  const double x = a.xy[o], y = a.xy[o + 1];
  double qx = x, qy = y;
  for (int it = 0; it < TACEX_LENS_POINT_ITERATIONS; ++it) {
    const double px = ((qx + 0.5) - a.hw) - cx, py = ((qy + 0.5) - a.hh) - cy;
    const double xn = px * a.s, yn = py * a.s;
    const double xx = xn * xn, yy = yn * yn, xyn = xn * yn;
    const double r2 = xx + yy;
    const double rad = (k1 + k2 * r2) * r2;
    const double dx = (xn * rad + (p1 + p1) * xyn) + p2 * (r2 + (xx + xx));
    const double dy = (yn * rad + p1 * (r2 + (yy + yy))) + (p2 + p2) * xyn;
    const double ou = ((e00 * px + e01 * py) + a.hw * dx) + tx;
    const double ov = ((e10 * px + e11 * py) + a.hw * dy) + ty;
    qx = x - ou; qy = y - ov;
  }
  a.out[o] = qx; a.out[o + 1] = qy;
}

// the checks the three entry points share (`src` is rgb_dev or xy_dev)
bool lens_refused(const char* fn, const char* src_name, const void* src_dev, const float* profiles_dev, int num_profiles, const void* out_dev,
                  int num_frames, int height, int width) {
  return null_arg(fn, src_name, src_dev) || null_arg(fn, "profiles_dev", profiles_dev) || null_arg(fn, "out_dev", out_dev) ||
         not_positive(fn, "num_profiles", num_profiles) || not_positive(fn, "num_frames", num_frames) ||
         not_positive(fn, "height", height) || not_positive(fn, "width", width);
}

// the checks the two image entry points share; fills `a` (all but `cam`) when they pass
int lens_check_and_fill(const char* fn, const float* rgb_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev,
                        void* out_dev, int num_frames, int height, int width, LensArgs* a) {
  if (lens_refused(fn, "rgb_dev", rgb_dev, profiles_dev, num_profiles, out_dev, num_frames, height, width)) return 2;
  if (out_dev == (const void*)rgb_dev) { set_error("%s: out_dev == rgb_dev (a gather cannot run in place)", fn); return 2; }
  const long long npix = (long long)height * width;
  const long long groups = (npix + 3) / 4;
  FrameLaunch fl;
  if (!frame_launch(groups, npix, kLensBlock, num_frames, &fl)) return refuse_image_launch(fn, num_frames, height, width);
  a->rgb = rgb_dev; a->profiles = profiles_dev; a->ids = profile_ids_dev; a->out = out_dev;
  a->npix = (unsigned int)npix; a->groups = (unsigned int)groups; a->blocks_per_frame = fl.blocks_per_frame;
  a->num_profiles = num_profiles; a->H = height; a->W = width;
  a->s = 2.0f / (float)width; a->hw = (float)width * 0.5f; a->hh = (float)height * 0.5f;
  return 0;
}

template <int kMode>
int lens_launch(const LensArgs& a, int num_frames, hipStream_t st, const char* what) {
  const bool vec = ((uintptr_t)a.out % 16 == 0) && (a.npix % 4 == 0);
  const dim3 grid(a.blocks_per_frame * (unsigned int)num_frames), block(kLensBlock);
  if (!vec) {
    hipLaunchKernelGGL((lens_model_kernel<kMode, false>), grid, block, 0, st, a);
  } else if constexpr (kMode == 0) {
    hipLaunchKernelGGL(lens_rows_kernel, grid, block, 0, st, a);
  } else {
    hipLaunchKernelGGL((lens_model_kernel<kMode, true>), grid, block, 0, st, a);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, what);
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_lens_model(const float* rgb_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev,
                                float* out_dev, int num_frames, int height, int width, void* stream) {
  using namespace tacex;
  LensArgs a{};
  const int rc = lens_check_and_fill("tacex_lens_model", rgb_dev, profiles_dev, num_profiles, profile_ids_dev, out_dev, num_frames, height,
                                     width, &a);
  if (rc) return rc;
  return lens_launch<0>(a, num_frames, (hipStream_t)stream, "lens_model_kernel");
}

extern "C" int tacex_lens_camera_model(const float* rgb_dev, const float* lens_profiles_dev, int num_lens_profiles,
                                       const int32_t* lens_profile_ids_dev, const float* profiles_dev, int num_profiles,
                                       const int32_t* profile_ids_dev, uint64_t seed, uint32_t frame_offset, uint32_t call, void* out_dev,
                                       int out_dtype, int num_frames, int height, int width, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_lens_camera_model";
  if (null_arg(fn, "lens_profiles_dev", lens_profiles_dev) || not_positive(fn, "num_lens_profiles", num_lens_profiles) ||
      null_arg(fn, "profiles_dev", profiles_dev) || not_positive(fn, "num_profiles", num_profiles)) return 2;
  LensArgs a{};
  const int rc = lens_check_and_fill(fn, rgb_dev, lens_profiles_dev, num_lens_profiles, lens_profile_ids_dev, out_dev, num_frames, height,
                                     width, &a);
  if (rc) return rc;
  if (out_dtype != 0 && out_dtype != 1) { set_error("%s: out_dtype = %d (0: float32, 1: uint8)", fn, out_dtype); return 2; }
  a.cam.profiles = profiles_dev; a.cam.ids = profile_ids_dev; a.cam.num_profiles = num_profiles;
  a.cam.key0 = (uint32_t)(seed & 0xffffffffull); a.cam.key1 = (uint32_t)(seed >> 32); a.cam.frame_offset = frame_offset; a.cam.call = call;
  hipStream_t st = (hipStream_t)stream;
  return out_dtype == 1 ? lens_launch<2>(a, num_frames, st, "lens_camera_model_kernel") : lens_launch<1>(a, num_frames, st, "lens_camera_model_kernel");
}

extern "C" int tacex_lens_points(const double* xy_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev,
                                 double* out_dev, int num_frames, int num_points, int height, int width, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_lens_points";
  if (lens_refused(fn, "xy_dev", xy_dev, profiles_dev, num_profiles, out_dev, num_frames, height, width) ||
      not_positive(fn, "num_points", num_points)) return 2;
  FrameLaunch fl;
  if (!frame_launch(num_points, num_points, kLensBlock, num_frames, &fl)) return refuse_points_launch(fn, num_frames, num_points);
  PointArgs a{};
  a.xy = xy_dev; a.profiles = profiles_dev; a.ids = profile_ids_dev; a.out = out_dev;
  a.n = (unsigned int)num_points; a.blocks_per_frame = fl.blocks_per_frame; a.num_profiles = num_profiles;
  a.s = 2.0 / (double)width; a.hw = (double)width * 0.5; a.hh = (double)height * 0.5;
  hipLaunchKernelGGL(lens_points_kernel, dim3(fl.grid), dim3(kLensBlock), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "lens_points_kernel");
}
