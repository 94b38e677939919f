// Sensor camera model (tacex_camera_model): per-env colour response, fixed-pattern gain, read + shot noise and the 8-bit quantisation
// of a delivered frame, applied to the float32 `tactile_rgb` batch in ONE streaming pass (12 B / pixel in, 3 or 12 B / pixel out).
// The contract - the order of every float32 operation and the addressing of every random draw - is the comment of tacex_camera_model
// in include/tacex_hip.h; tests/camera_model_ref.py restates that comment in NumPy and the two agree bit for bit.  This file is
// compiled with -ffp-contract=off (tacex_amd/_build.py): every product and sum below rounds on its own.
//
// Draws are addressed per GROUP of four consecutive pixels of a frame (Philox counter = group, stream, frame, call), so the mapping of
// threads to groups is a tuning choice that cannot change the image.  A thread takes ONE group (48 bytes in), on one of two paths:
//   vector path  three 16-byte loads, then three 16-byte stores (float32 output) or one 12-byte store of the packed bytes (uint8
//                output): a wave reads 3072 and writes 3072 / 768 contiguous bytes.  (Four groups per thread and three 16-byte
//                stores of 16 packed pixels measured 2 - 6 % SLOWER on 2048 frames of 320 x 240: 122 VGPRs instead of 48 halve the
//                waves per SIMD, and the kernel is bound by its integer work, not by store issue - DESIGN 4.0.12a);
//   scalar path  dword loads and dword / byte stores, bounds-checked per pixel: taken when a base pointer is not 16-byte aligned or
//                H W is no multiple of 4 (the last group of a frame is partial and frames start unaligned).  Same bits.
// A workgroup stays inside one frame (grid = blocks per frame x frames), so the frame's profile id and its 16-float profile row are
// wave-uniform loads (scalar registers, once per wave); the fixed-pattern Philox calls are skipped by a uniform branch when the
// frame's sigma_f is 0.  All loads of a thread precede its stores and no two threads share a pixel: in-place float32 is safe.
// No LDS.  Value offsets are 64-bit (4096 frames of 320 x 240 x 3 floats exceed 2^32 bytes).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "camera_group.h"
#include "stage_args.h"
#include "tacex_hip.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

constexpr int kCameraBlock = 256;

// (the draws, the per-group arithmetic and the stores are in camera_group.h, shared with lens_model.hip)
struct CameraArgs {
  const float* rgb;          // (B,H,W,3); may alias `out` (float32 output only)
  CameraTable cam;           // profiles (P,16), ids (B,) or nullptr, Philox key, frame_offset, call
  void* out;                 // (B,H,W,3) float32 or uint8
  long long npix;            // H W
  unsigned int groups;       // ceil(npix / 4)
  unsigned int blocks_per_frame;
};


// Vector path: one group per thread, three 16-byte loads, then three 16-byte stores (float32) or one 12-byte store of the packed
// bytes (uint8).  Requires both base pointers 16-byte aligned and npix % 4 == 0 (every frame then starts 16-byte aligned in the
// input and 4-byte aligned in a uint8 output, and no group is partial).
template <bool kU8>
__global__ __launch_bounds__(kCameraBlock) void camera_model_vec_kernel(CameraArgs a) {
  const unsigned int frame = blockIdx.x / a.blocks_per_frame;
  const unsigned int g = (blockIdx.x - frame * a.blocks_per_frame) * kCameraBlock + threadIdx.x;
  if (g >= a.groups) return;
  const CameraProfileRow p = load_camera_profile(a.cam, frame);
  const size_t v0 = ((size_t)frame * (size_t)a.npix + (size_t)g * 4) * 3;  // first value of the group in the batch
  const float4* src = reinterpret_cast<const float4*>(a.rgb + v0);
  float px[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float4 t = src[i];
    px[4 * i] = t.x; px[4 * i + 1] = t.y; px[4 * i + 2] = t.z; px[4 * i + 3] = t.w;
  }
  camera_group(a.cam, p, a.cam.frame_offset + frame, g, px);
  store_group_vec<kU8>(a.out, v0, px);
}

// Scalar path: one group per thread, any alignment, any npix (pixels past the frame's end are neither loaded nor stored).
template <bool kU8>
__global__ __launch_bounds__(kCameraBlock) void camera_model_scalar_kernel(CameraArgs a) {
  const unsigned int frame = blockIdx.x / a.blocks_per_frame;
  const unsigned int g = (blockIdx.x - frame * a.blocks_per_frame) * kCameraBlock + threadIdx.x;
  if (g >= a.groups) return;
  const CameraProfileRow p = load_camera_profile(a.cam, frame);
  const long long left = a.npix - (long long)g * 4;
  const int n = left < 4 ? (int)left * 3 : 12;  // values of this group inside the frame
  const size_t v0 = ((size_t)frame * (size_t)a.npix + (size_t)g * 4) * 3;
  float px[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) px[i] = i < n ? a.rgb[v0 + i] : 0.0f;
  camera_group(a.cam, p, a.cam.frame_offset + frame, g, px);
  store_group_scalar<kU8>(a.out, v0, px, n);
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_camera_model(const float* rgb_dev, const float* profiles_dev, int num_profiles, const int32_t* profile_ids_dev,
                                  uint64_t seed, uint32_t frame_offset, uint32_t call, void* out_dev, int out_dtype, int num_frames,
                                  int height, int width, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_camera_model";
  if (null_arg(fn, "rgb_dev", rgb_dev) || null_arg(fn, "profiles_dev", profiles_dev) || null_arg(fn, "out_dev", out_dev) ||
      not_positive(fn, "num_profiles", num_profiles) || not_positive(fn, "num_frames", num_frames) ||
      not_positive(fn, "height", height) || not_positive(fn, "width", width)) return 2;
  if (out_dtype != 0 && out_dtype != 1) { set_error("tacex_camera_model: out_dtype = %d (0: float32, 1: uint8)", out_dtype); return 2; }
  if (out_dtype == 1 && out_dev == (const void*)rgb_dev) {
    set_error("tacex_camera_model: out_dev == rgb_dev needs out_dtype 0 (a uint8 frame cannot overwrite its float32 input)");
    return 2;
  }
  const bool u8 = out_dtype == 1;
  const long long npix = (long long)height * width;
  const long long groups = (npix + 3) / 4;
  const bool vec = ((uintptr_t)rgb_dev % 16 == 0) && ((uintptr_t)out_dev % 16 == 0) && (npix % 4 == 0);
  FrameLaunch fl;  // one group per thread on both paths
  if (!frame_launch(groups, groups, kCameraBlock, num_frames, &fl)) return refuse_image_launch(fn, num_frames, height, width);
  CameraArgs a{};
  a.rgb = rgb_dev; a.out = out_dev;
  a.cam.profiles = profiles_dev; a.cam.ids = profile_ids_dev; a.cam.num_profiles = num_profiles;
  a.cam.key0 = (uint32_t)(seed & 0xffffffffull); a.cam.key1 = (uint32_t)(seed >> 32); a.cam.frame_offset = frame_offset; a.cam.call = call;
  a.npix = npix; a.groups = (unsigned int)groups; a.blocks_per_frame = fl.blocks_per_frame;
  const dim3 grid(fl.grid), block(kCameraBlock);
  hipStream_t st = (hipStream_t)stream;
  if (vec && u8) hipLaunchKernelGGL(camera_model_vec_kernel<true>, grid, block, 0, st, a);
  else if (vec) hipLaunchKernelGGL(camera_model_vec_kernel<false>, grid, block, 0, st, a);
  else if (u8) hipLaunchKernelGGL(camera_model_scalar_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(camera_model_scalar_kernel<false>, grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "camera_model_kernel");
}

extern "C" int tacex_camera_noise_draw(uint64_t seed, uint32_t frame, uint32_t call, uint32_t group, int fixed_pattern, int32_t out[12]) {
  using namespace tacex;
  if (!out) { set_error("tacex_camera_noise_draw: null out"); return 2; }
  // the function the kernels call, compiled for the host
  camera_noise_draw((uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), frame, call, group, fixed_pattern != 0, out);
  return 0;
}
