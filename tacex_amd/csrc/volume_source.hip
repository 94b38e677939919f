// Signed-distance volume library as a height-map source (tacex_height_map_from_sdf; the contract is the comment of that call in
// include/tacex_hip.h, restated in tests/volume_source_ref.py).  Every env presses its own volume of a library - a grid of signed
// distances sampled trilinearly and sphere-traced along the optical axis between the clip planes, under a full rigid pose, uniform
// scale and iso level the caller writes in place.  The cost per pixel does not depend on how detailed the object is.
//
// A workgroup of 256 threads marches a 32 x 8 tile of one frame: four waves, each on a 16 x 4 patch of NEIGHBOURING pixels, so the
// eight loads of a tap fall into a few cache lines per instruction and the rays of a wave end after similar step counts (lanes that
// own four consecutive pixels make every tap instruction touch 64 lines: DESIGN 4.0.2b).  Frame, volume row, pose and the twelve ray
// coefficients depend on blockIdx alone: scalar loads, wave-uniform branches.  A patch whose pixels all miss the grid's box (or lie
// outside the frame) has no active lane and skips the loop without a tap.  Frame minimum, indentation depth and contact ranges come
// from the kernel of tacex_indentation_depth, launched behind the marching kernel on the same stream.
// Built with -ffp-contract=off (_build.FILE_FLAGS): every product and sum of the contract is rounded to float32 on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdf_tap.h"
#include "stage_args.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

struct SdfArgs {
  const float* voxels;  // all grids back to back
  const int* vi;        // (P,4) [first voxel, D, Hv, Wv]
  const float* vf;      // (P,8) [pitch_mm, i0, j0, k0, step_scale, 0, 0, 0]
  const int* ids;       // (B,) or nullptr (volume 0)
  const float* pose;    // (B,16)
  float* hm;            // (B,H,W)
  int num_voxels, P, H, W, tiles_x, tiles, max_steps;
  float pixmm, near_clip, far_clip, tol;
};

__global__ __launch_bounds__(256) void sdf_height_map_kernel(SdfArgs a) {
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int tr = tile / a.tiles_x, tc = tile - tr * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tc * kSdfTileW + (wave & 1) * 16 + (lane & 15);
  const int y = tr * kSdfTileH + (wave >> 1) * 4 + (lane >> 4);
  const bool in_frame = x < a.W && y < a.H;
  const float far_clip = a.far_clip;

  // the frame's volume, pose and ray coefficients (blockIdx alone; sdf_tap.h: shared with the scene source)
  int first, N[3];
  float ax[3], ay[3], az[3], q0[3], ia[3], hmax[3], scale, level, step_scale, vox;
  bool par[3];
  const bool none = !sdf_load_slot(a.ids ? a.ids[b] : 0, a.vi, a.vf, a.P, a.num_voxels, a.pose + 16 * (size_t)b, a.pixmm, &first, N, ax, ay,
                                   az, q0, ia, hmax, par, &scale, &level, &step_scale, &vox);
  float* __restrict__ out = a.hm + (size_t)b * ((size_t)a.H * (size_t)a.W) + (size_t)y * (size_t)a.W + (size_t)x;
  if (none) {
    if (in_frame) *out = far_clip;
    return;
  }

  // the pixel's ray in voxel coordinates and its interval
  const float xf = (float)x, yf = (float)y;
  float bq[3], lo = a.near_clip, hi = far_clip;
  bool active = in_frame;
#pragma unroll
  for (int k = 0; k < 3; ++k) bq[k] = (q0[k] + (xf * ax[k])) + (yf * ay[k]);
  active = active && sdf_clip(bq, ia, hmax, par, &lo, &hi);  // (sdf_tap.h: shared with the scene source)

  float depth = far_clip;
  if (active) {
    const float* __restrict__ vol = a.voxels + first;
    const int sy = N[0], sz = N[1] * N[0];
    float z = lo;
    for (int n = 0; n < a.max_steps; ++n) {
      int m[3];
      float w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) sdf_cell(bq[k] + (z * az[k]), hmax[k], N[k], &m[k], &w[k]);
      const float s = sdf_tap(vol, sy, sz, m, w);  // (sdf_tap.h: shared with the scene source)
      const float d = ((s - level) * scale) * step_scale;
      if (d < a.tol) { depth = z; break; }
      z = z + d;
      if (!(z <= hi)) break;
      if (n == a.max_steps - 1 && d < vox) depth = z;  // the grazing-ray rule
    }
  }
  if (in_frame) *out = depth < far_clip ? depth : far_clip;
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_height_map_from_sdf(const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev, const float* volumes_f_dev,
                                         int num_volumes, const int32_t* volume_ids_dev, const float* pose_dev, float pixmm,
                                         float near_clip_mm, float far_clip_mm, int max_steps, float tol_mm, float gelpad_height_m,
                                         float gelpad_to_camera_min_distance_m, float* hm_mm_dev, float* frame_min_dev,
                                         float* indent_mm_dev, int32_t* frame_rows_dev, int num_frames, int height, int width,
                                         void* stream) {
  using namespace tacex;
  const char* fn = "tacex_height_map_from_sdf";
  if (null_arg(fn, "voxels_dev", voxels_dev) || null_arg(fn, "volumes_i_dev", volumes_i_dev) ||
      null_arg(fn, "volumes_f_dev", volumes_f_dev) || null_arg(fn, "pose_dev", pose_dev) || null_arg(fn, "hm_mm_dev", hm_mm_dev) ||
      null_arg(fn, "frame_min_dev", frame_min_dev)) return 2;
  if (not_positive(fn, "num_voxels", num_voxels) || not_positive(fn, "num_volumes", num_volumes) ||
      not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) || not_positive(fn, "width", width)) return 2;
  if (not_frame_rows_geometry(fn, height, width)) return 2;
  if (!(pixmm > 0.0f)) { set_error("%s: pixmm = %g (must be > 0)", fn, (double)pixmm); return 2; }
  if (max_steps < 1 || max_steps > 128) { set_error("%s: max_steps = %d (must be 1..128)", fn, max_steps); return 2; }
  if (!(tol_mm > 0.0f)) { set_error("%s: tol_mm = %g (must be > 0)", fn, (double)tol_mm); return 2; }
  if (!(near_clip_mm < far_clip_mm)) {
    set_error("%s: near_clip_mm = %g, far_clip_mm = %g (near must be below far)", fn, (double)near_clip_mm, (double)far_clip_mm);
    return 2;
  }
  if (not_aligned16(fn, "hm_mm_dev", hm_mm_dev)) return 2;
  SdfArgs a{};
  a.tiles_x = (width + kSdfTileW - 1) / kSdfTileW;
  a.tiles = a.tiles_x * ((height + kSdfTileH - 1) / kSdfTileH);
  if ((long long)a.tiles * num_frames > 0x7fffffffll) return refuse_image_launch(fn, num_frames, height, width);
  a.voxels = voxels_dev; a.vi = volumes_i_dev; a.vf = volumes_f_dev; a.ids = volume_ids_dev; a.pose = pose_dev; a.hm = hm_mm_dev;
  a.num_voxels = num_voxels; a.P = num_volumes; a.H = height; a.W = width; a.max_steps = max_steps;
  a.pixmm = pixmm; a.near_clip = near_clip_mm; a.far_clip = far_clip_mm; a.tol = tol_mm;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sdf_height_map_kernel, dim3((unsigned int)(a.tiles * num_frames)), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "sdf_height_map_kernel");
  // frame minimum, indentation depth, contact ranges: the statements of tacex_indentation_depth (the row kernel's geometry here)
  const char* what = "";
  e = run_frame_outputs(hm_mm_dev, false, nullptr, frame_min_dev, indent_mm_dev, nullptr, nullptr, frame_rows_dev, num_frames, height, width,
                        0.f, 0.f, 0.f, gelpad_height_m, gelpad_to_camera_min_distance_m, st, &what);
  return e == hipSuccess ? 0 : fail_hip(e, what);
}
