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

#include "stage_args.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

constexpr int kSdfTileW = 32, kSdfTileH = 8;  // 2 x 2 waves of 16 x 4 pixels
constexpr float kSdfTwo30 = 1073741824.0f;

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

__device__ __forceinline__ float sdf_lerp(float p, float q, float t) { return p + (t * (q - p)); }

__global__ __launch_bounds__(256) void sdf_height_map_kernel(SdfArgs a) {
  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int tr = tile / a.tiles_x, tc = tile - tr * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tc * kSdfTileW + (wave & 1) * 16 + (lane & 15);
  const int y = tr * kSdfTileH + (wave >> 1) * 4 + (lane >> 4);
  const bool in_frame = x < a.W && y < a.H;
  const float far_clip = a.far_clip;

  // the frame's volume, pose and ray coefficients (blockIdx alone)
  const int id = a.ids ? a.ids[b] : 0;
  bool none = !(id >= 0 && id < a.P);  // no such volume: far clip everywhere, the library is not touched
  int first = 0, N[3] = {2, 2, 2};
  float pitch = 0.f, anchor[3] = {0.f, 0.f, 0.f}, step_scale = 0.f;
  if (!none) {
    const int* vi = a.vi + 4 * (size_t)id;
    const float* vf = a.vf + 8 * (size_t)id;
    first = vi[0]; N[2] = vi[1]; N[1] = vi[2]; N[0] = vi[3];
    pitch = vf[0]; anchor[0] = vf[1]; anchor[1] = vf[2]; anchor[2] = vf[3]; step_scale = vf[4];
    none = first < 0 || N[0] < 2 || N[1] < 2 || N[2] < 2 ||
           (long long)first + (long long)N[2] * N[1] * N[0] > (long long)a.num_voxels;  // (a table row the host would not have written)
  }
  float ax[3], ay[3], az[3], q0[3], ia[3], hmax[3], scale = 0.f, level = 0.f, vox = 0.f;
  bool par[3];
  if (!none) {
    const float* r = a.pose + 16 * (size_t)b;
    const float tx = r[9], ty = r[10], tz = r[11];
    scale = r[12]; level = r[13];
    const float g = scale * pitch;
    const float inv = 1.0f / g;
    vox = g;
    bool ok = g > 0.0f && step_scale > 0.0f && fabsf(level) < kSdfTwo30;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ax[k] = (r[k] * a.pixmm) * inv;
      ay[k] = (r[3 + k] * a.pixmm) * inv;
      az[k] = r[6 + k] * inv;
      q0[k] = anchor[k] - ((((r[k] * tx) + (r[3 + k] * ty)) + (r[6 + k] * tz)) * inv);
      par[k] = !(fabsf(az[k]) >= 1e-12f);
      ia[k] = par[k] ? 0.0f : 1.0f / az[k];
      hmax[k] = (float)(N[k] - 1);
      ok = ok && fabsf(ax[k]) < kSdfTwo30 && fabsf(ay[k]) < kSdfTwo30 && fabsf(az[k]) < kSdfTwo30 && fabsf(q0[k]) < kSdfTwo30;
    }
    none = !ok;
  }
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
  for (int k = 0; k < 3; ++k) {
    bq[k] = (q0[k] + (xf * ax[k])) + (yf * ay[k]);
    active = active && fabsf(bq[k]) < kSdfTwo30;
    if (par[k]) {
      active = active && bq[k] >= 0.0f && bq[k] <= hmax[k];
    } else {
      const float t1 = (0.0f - bq[k]) * ia[k], t2 = (hmax[k] - bq[k]) * ia[k];
      const float tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
      lo = tn > lo ? tn : lo;
      hi = tf < hi ? tf : hi;
    }
  }
  active = active && lo <= hi;

  float depth = far_clip;
  if (active) {
    const float* __restrict__ vol = a.voxels + first;
    const int sy = N[0], sz = N[1] * N[0];
    float z = lo;
    for (int n = 0; n < a.max_steps; ++n) {
      int m[3];
      float w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float c = bq[k] + (z * az[k]);
        c = c > 0.0f ? c : 0.0f;  // (a NaN: 0 - the index stays legal whatever the pose)
        c = c < hmax[k] ? c : hmax[k];
        m[k] = min((int)floorf(c), N[k] - 2);
        w[k] = c - (float)m[k];
      }
      const float* v = vol + ((m[2] * sz + m[1] * sy) + m[0]);
      const float v000 = v[0], v001 = v[1], v010 = v[sy], v011 = v[sy + 1];
      const float v100 = v[sz], v101 = v[sz + 1], v110 = v[sz + sy], v111 = v[sz + sy + 1];
      const float e00 = sdf_lerp(v000, v001, w[0]), e01 = sdf_lerp(v010, v011, w[0]);
      const float e10 = sdf_lerp(v100, v101, w[0]), e11 = sdf_lerp(v110, v111, w[0]);
      const float f0 = sdf_lerp(e00, e01, w[1]), f1 = sdf_lerp(e10, e11, w[1]);
      const float s = sdf_lerp(f0, f1, w[2]);
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
