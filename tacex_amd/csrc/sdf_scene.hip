// Scenes of signed-distance volumes as a height-map source (tacex_height_map_from_sdf_scene; the contract is the comment of that call
// in include/tacex_hip.h, restated in tests/sdf_scene_ref.py).  Every env holds K slots, each a volume of the library under its own
// rigid pose, scale, iso level and blend width, folded into one field by union, subtraction and intersection DURING the march: a
// plate with a hole, a bolt in a nut, two parts filleted together.  The trilinear tap, the box clip and the per-slot coefficients are
// those of the volume source (sdf_tap.h); a scene whose only slot is a hard union gives that source's bits.
//
// Geometry as in volume_source.hip: 256 threads march a 32 x 8 tile of one frame, four waves on 16 x 4 patches of neighbouring pixels.
// The first K lanes of a workgroup's first wave each work out one slot - coefficients, whether it is empty, whether its grid's box
// meets the tile - into a small LDS table, and a ballot gives the tile's live slots as a bit mask.  Frame, slot data and mask depend on
// blockIdx alone: the loops over the mask's bits (scalar) and the branches on a slot's operation are wave-uniform, and the table is
// read at wave-uniform addresses (broadcast LDS reads).  What a ray needs of a slot at every step - its coordinates at z = 0 and its
// interval in the slot's box, five floats - stays in LDS per lane for the first kSceneCached live slots (conflict-free reads) and is
// worked out again from the table for the others: registers cannot be indexed by a list that differs from tile to tile.  A tile no
// union slot's box meets writes the far clip without a tap.
// sdf_scene_kernel<true> (tacex_height_map_from_sdf_scene_parts) also says which slot every pixel shows: `own`, one more register in
// the step loop, follows the comparison inside scene_smin at every fold, and the lane stores one byte beside its depth.  The plain
// instantiation is the kernel as it was: nothing of the owner is compiled into it.
// Built with -ffp-contract=off (_build.FILE_FLAGS): every product and sum of the contract is rounded to float32 on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdf_tap.h"
#include "stage_args.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

constexpr int kSceneMaxSlots = 8;
constexpr int kSceneCached = 3;  // live slots of a tile whose per-lane ray data stay in LDS (15 KiB: the VGPRs still bound the occupancy)
// a slot's row of the float table ...
enum { kAx = 0, kAy = 3, kAz = 6, kQ0 = 9, kIa = 12, kHmax = 15, kScale = 18, kLevel = 19, kStep = 20, kVox = 21, kBlend = 22, kVox2 = 23, kSlotFloats = 24 };
// ... and of the int table (kState: 0 empty, 1 not empty, 2 live for this tile)
enum { kFirst = 0, kN = 1, kOp = 4, kPar = 5, kState = 6, kSlotInts = 8 };
enum { kUnion = 0, kSubtract = 1, kIntersect = 2 };

struct SceneArgs {
  const float* voxels;  // all grids back to back
  const int* vi;        // (P,4) [first voxel, D, Hv, Wv]
  const float* vf;      // (P,8) [pitch_mm, i0, j0, k0, step_scale, 0, 0, 0]
  const int* ids;       // (B,K)
  const float* pose;    // (B,K,16)
  const int* ops;       // (B,K)
  float* hm;            // (B,H,W)
  uint8_t* parts;       // (B,H,W) the owner of every pixel (sdf_scene_kernel<true> alone)
  int num_voxels, P, K, H, W, tiles_x, tiles, max_steps;
  float pixmm, near_clip, far_clip, tol;
};

// smin_k(a, b) of the contract: the plain minimum unless k > 0
__device__ __forceinline__ float scene_smin(float a, float b, float k) {
  float mn = b < a ? b : a;
  if (k > 0.0f) {
    float t = k - fabsf(a - b);
    t = t > 0.0f ? t : 0.0f;
    const float h = t / k;
    mn = mn - ((h * h) * (k * 0.25f));
  }
  return mn;
}

// the pixel's ray in the grid of the slot with table rows T, I: its coordinates at z = 0 and its interval in the slot's box
__device__ __forceinline__ bool scene_slot_ray(const float* T, const int* I, float xf, float yf, float near_clip, float far_clip, float bq[3],
                                               float* lo, float* hi) {
  float ia[3], hmax[3];
  bool par[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    bq[k] = (T[kQ0 + k] + (xf * T[kAx + k])) + (yf * T[kAy + k]);
    ia[k] = T[kIa + k]; hmax[k] = T[kHmax + k]; par[k] = (I[kPar] >> k) & 1;
  }
  *lo = near_clip; *hi = far_clip;
  return sdf_clip(bq, ia, hmax, par, lo, hi);
}

constexpr int kSceneNoOwner = 255;

template <bool IDS>
__global__ __launch_bounds__(256) void sdf_scene_kernel(SceneArgs a) {
  __shared__ float tab[kSceneMaxSlots][kSlotFloats];
  __shared__ int itab[kSceneMaxSlots][kSlotInts];
  __shared__ float ray[kSceneCached][5][256];  // per lane: a cached slot's b[3], lo, hi
  __shared__ unsigned masks[2];                // live slots, live union slots
  __shared__ float vox_min;                    // the smallest voxel [camera mm] over the env's non-empty union slots

  const int b = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)a.tiles);
  const int tr = tile / a.tiles_x, tc = tile - tr * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tc * kSdfTileW + (wave & 1) * 16 + (lane & 15);
  const int y = tr * kSdfTileH + (wave >> 1) * 4 + (lane >> 4);
  const bool in_frame = x < a.W && y < a.H;
  const float far_clip = a.far_clip;

  // wave 0, one slot per lane: coefficients, empty or not, live for this tile or not; then a vote
  if (wave == 0) {
    int state = 0, op = -1;
    float vox = kSdfTwo30;
    if (lane < a.K) {
      const int s = lane;
      const size_t slot = (size_t)b * (size_t)a.K + (size_t)s;
      const float* r = a.pose + 16 * slot;
      const int id = a.ids[slot];
      op = a.ops[slot];
      const float blend = r[14];
      int first, N[3];
      float ax[3], ay[3], az[3], q0[3], ia[3], hmax[3], scale, level, step_scale;
      bool par[3];
      const bool asked = op >= kUnion && op <= kIntersect && fabsf(blend) < kSdfTwo30;
      const bool some = sdf_load_slot(asked ? id : -1, a.vi, a.vf, a.P, a.num_voxels, r, a.pixmm, &first, N, ax, ay, az, q0, ia, hmax, par, &scale, &level,
                                   &step_scale, &vox);
      state = some ? 1 : 0;
      if (some) {
        // the box's eight corners in the image [mm]: their bounding rectangle against the tile's
        const float* vf = a.vf + 8 * (size_t)id;
        float xmin = 0.f, xmax = 0.f, ymin = 0.f, ymax = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float o0 = (((c & 1) ? hmax[0] : 0.0f) - vf[1]) * vox, o1 = (((c & 2) ? hmax[1] : 0.0f) - vf[2]) * vox;
          const float o2 = (((c & 4) ? hmax[2] : 0.0f) - vf[3]) * vox;
          const float X = (((r[0] * o0) + (r[1] * o1)) + (r[2] * o2)) + r[9], Y = (((r[3] * o0) + (r[4] * o1)) + (r[5] * o2)) + r[10];
          xmin = (c == 0 || X < xmin) ? X : xmin; xmax = (c == 0 || X > xmax) ? X : xmax;
          ymin = (c == 0 || Y < ymin) ? Y : ymin; ymax = (c == 0 || Y > ymax) ? Y : ymax;
        }
        const float margin = blend > 0.0f ? a.pixmm + blend : a.pixmm;
        const float x0 = (float)(tc * kSdfTileW) * a.pixmm, x1 = (float)(tc * kSdfTileW + (kSdfTileW - 1)) * a.pixmm;
        const float y0 = (float)(tr * kSdfTileH) * a.pixmm, y1 = (float)(tr * kSdfTileH + (kSdfTileH - 1)) * a.pixmm;
        const bool meets = xmax + margin >= x0 && xmin - margin <= x1 && ymax + margin >= y0 && ymin - margin <= y1;
        if (op == kIntersect || meets) state = 2;  // (an intersection empties every tile its box does not meet: always live)
      }
      float* T = tab[s];
      int* I = itab[s];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        T[kAx + k] = ax[k]; T[kAy + k] = ay[k]; T[kAz + k] = az[k]; T[kQ0 + k] = q0[k]; T[kIa + k] = ia[k]; T[kHmax + k] = hmax[k];
        I[kN + k] = N[k];
      }
      T[kScale] = scale; T[kLevel] = level; T[kStep] = step_scale; T[kVox] = vox; T[kBlend] = blend; T[kVox2] = vox * vox;
      I[kFirst] = first; I[kOp] = op; I[kPar] = (par[0] ? 1 : 0) | (par[1] ? 2 : 0) | (par[2] ? 4 : 0); I[kState] = state;
    }
    const unsigned live_mask = (unsigned)__ballot(state == 2), union_mask = (unsigned)__ballot(state >= 1 && op == kUnion);
    float vmin = (state >= 1 && op == kUnion) ? vox : kSdfTwo30;  // (lanes 0..7 hold the slots: a minimum over eight lanes)
#pragma unroll
    for (int d = 1; d < kSceneMaxSlots; d <<= 1) {
      const float other = __shfl_xor(vmin, d);
      vmin = other < vmin ? other : vmin;
    }
    if (lane == 0) { masks[0] = live_mask; masks[1] = live_mask & union_mask; vox_min = vmin; }
  }
  __syncthreads();
  const unsigned live_mask = (unsigned)__builtin_amdgcn_readfirstlane((int)masks[0]);
  const size_t pixel = (size_t)b * ((size_t)a.H * (size_t)a.W) + (size_t)y * (size_t)a.W + (size_t)x;
  float* __restrict__ out = a.hm + pixel;
  if (masks[1] == 0) {  // no union slot meets the tile: nothing to hit
    if (in_frame) {
      *out = far_clip;
      if constexpr (IDS) a.parts[pixel] = (uint8_t)kSceneNoOwner;
    }
    return;
  }

  // the pixel's interval: from the first entry into a live union slot's box to the last exit from one
  const float xf = (float)x, yf = (float)y;
  float lo = 0.f, hi = 0.f;
  bool active = false;
  int c = 0;
  for (unsigned rest = live_mask; rest; rest &= rest - 1, ++c) {
    const int s = __ffs(rest) - 1;
    const bool is_union = itab[s][kOp] == kUnion;
    if (!is_union && c >= kSceneCached) continue;
    float bq[3], lo_s, hi_s;
    const bool meets = scene_slot_ray(tab[s], itab[s], xf, yf, a.near_clip, far_clip, bq, &lo_s, &hi_s);
    if (meets && is_union) {
      lo = (!active || lo_s < lo) ? lo_s : lo;
      hi = (!active || hi_s > hi) ? hi_s : hi;
      active = true;
    }
    if (c < kSceneCached) {  // (a ray that misses the box: an interval no z lies in)
      ray[c][0][threadIdx.x] = bq[0]; ray[c][1][threadIdx.x] = bq[1]; ray[c][2][threadIdx.x] = bq[2];
      ray[c][3][threadIdx.x] = meets ? lo_s : INFINITY; ray[c][4][threadIdx.x] = meets ? hi_s : -INFINITY;
    }
  }
  active = active && in_frame;

  float depth = far_clip;
  int owner = kSceneNoOwner;  // (IDS) `own` of the evaluation that assigned the depth
  if (active) {
    const float vox = vox_min;
    float z = lo;
    for (int n = 0; n < a.max_steps; ++n) {
      float f = kSdfTwo30;
      int own = kSceneNoOwner;  // (IDS) the last slot whose value the comparison inside scene_smin took
      c = 0;
      for (unsigned rest = live_mask; rest; rest &= rest - 1, ++c) {
        const int s = __ffs(rest) - 1;
        const float* T = tab[s];
        const int* I = itab[s];
        const int op = I[kOp];
        const float blend = T[kBlend];
        float bq[3], lo_s, hi_s;
        if (c < kSceneCached) {  // the first live slots' rays were kept per lane
          bq[0] = ray[c][0][threadIdx.x]; bq[1] = ray[c][1][threadIdx.x]; bq[2] = ray[c][2][threadIdx.x];
          lo_s = ray[c][3][threadIdx.x]; hi_s = ray[c][4][threadIdx.x];
        } else if (!scene_slot_ray(T, I, xf, yf, a.near_clip, far_clip, bq, &lo_s, &hi_s)) {
          lo_s = INFINITY; hi_s = -INFINITY;
        }
        const bool inside = z >= lo_s && z <= hi_s;  // the point lies in the slot's box
        int m[3];
        float w[3], ex[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float q = bq[k] + (z * T[kAz + k]);
          ex[k] = q - sdf_cell(q, T[kHmax + k], I[kN + k], &m[k], &w[k]);
        }
        float e2 = 0.0f;
        if (!inside) {
          e2 = (((ex[0] * ex[0]) + (ex[1] * ex[1])) + (ex[2] * ex[2])) * T[kVox2];
          // a hard union at least as far away as the field so far cannot lower it (the bound below is >= sqrt(e2)): no tap
          if (op == kUnion && !(blend > 0.0f) && sqrtf(e2) >= f) continue;
        }
        const float t = sdf_tap(a.voxels + I[kFirst], I[kN], I[kN + 1] * I[kN], m, w);
        float u = ((t - T[kLevel]) * T[kScale]) * T[kStep];
        if (!inside) {  // the bound outside the box: the tap at the nearest point of the box and the distance to it
          const float p = u > 0.0f ? u : 0.0f;
          u = sqrtf(e2 + (p * p));
        }
        if constexpr (IDS) {  // scene_smin(p, q, .) takes q when q < p
          const bool takes = op == kUnion ? u < f : op == kSubtract ? u < -f : -u < -f;
          own = takes ? s : own;
        }
        if (op == kUnion) f = scene_smin(f, u, blend);
        else if (op == kSubtract) f = -scene_smin(-f, u, blend);
        else f = -scene_smin(-f, -u, blend);
      }
      if (f < a.tol) { depth = z; owner = own; break; }
      z = z + f;
      if (!(z <= hi)) break;
      if (n == a.max_steps - 1 && f < vox) { depth = z; owner = own; }  // the grazing-ray rule
    }
  }
  if (in_frame) {
    *out = depth < far_clip ? depth : far_clip;
    if constexpr (IDS) a.parts[pixel] = (uint8_t)(depth < far_clip ? owner : kSceneNoOwner);
  }
}

// both entry points: the checks, the march (with the part map when part_map_dev is given), the frame outputs
int run_sdf_scene(const char* fn, const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev, const float* volumes_f_dev, int num_volumes,
                  const int32_t* part_ids_dev, const float* part_pose_dev, const int32_t* part_ops_dev, int num_slots, float pixmm,
                  float near_clip_mm, float far_clip_mm, int max_steps, float tol_mm, float gelpad_height_m,
                  float gelpad_to_camera_min_distance_m, float* hm_mm_dev, float* frame_min_dev, float* indent_mm_dev, int32_t* frame_rows_dev,
                  uint8_t* part_map_dev, bool with_parts, int num_frames, int height, int width, void* stream) {
  if (null_arg(fn, "voxels_dev", voxels_dev) || null_arg(fn, "volumes_i_dev", volumes_i_dev) ||
      null_arg(fn, "volumes_f_dev", volumes_f_dev) || null_arg(fn, "part_ids_dev", part_ids_dev) ||
      null_arg(fn, "part_pose_dev", part_pose_dev) || null_arg(fn, "part_ops_dev", part_ops_dev) || null_arg(fn, "hm_mm_dev", hm_mm_dev) ||
      null_arg(fn, "frame_min_dev", frame_min_dev)) return 2;
  if (with_parts && null_arg(fn, "part_map_dev", part_map_dev)) return 2;
  if (not_positive(fn, "num_voxels", num_voxels) || not_positive(fn, "num_volumes", num_volumes) ||
      not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) || not_positive(fn, "width", width)) return 2;
  if (num_slots < 1 || num_slots > kSceneMaxSlots) { set_error("%s: num_slots = %d (must be 1..%d)", fn, num_slots, kSceneMaxSlots); return 2; }
  if (not_frame_rows_geometry(fn, height, width)) return 2;
  if (!(pixmm > 0.0f)) { set_error("%s: pixmm = %g (must be > 0)", fn, (double)pixmm); return 2; }
  if (max_steps < 1 || max_steps > 128) { set_error("%s: max_steps = %d (must be 1..128)", fn, max_steps); return 2; }
  if (!(tol_mm > 0.0f)) { set_error("%s: tol_mm = %g (must be > 0)", fn, (double)tol_mm); return 2; }
  if (!(near_clip_mm < far_clip_mm)) {
    set_error("%s: near_clip_mm = %g, far_clip_mm = %g (near must be below far)", fn, (double)near_clip_mm, (double)far_clip_mm);
    return 2;
  }
  if (not_aligned16(fn, "hm_mm_dev", hm_mm_dev)) return 2;
  SceneArgs a{};
  a.tiles_x = (width + kSdfTileW - 1) / kSdfTileW;
  a.tiles = a.tiles_x * ((height + kSdfTileH - 1) / kSdfTileH);
  if ((long long)a.tiles * num_frames > 0x7fffffffll) return refuse_image_launch(fn, num_frames, height, width);
  a.voxels = voxels_dev; a.vi = volumes_i_dev; a.vf = volumes_f_dev; a.ids = part_ids_dev; a.pose = part_pose_dev; a.ops = part_ops_dev;
  a.hm = hm_mm_dev; a.parts = part_map_dev; a.num_voxels = num_voxels; a.P = num_volumes; a.K = num_slots; a.H = height; a.W = width;
  a.max_steps = max_steps; a.pixmm = pixmm; a.near_clip = near_clip_mm; a.far_clip = far_clip_mm; a.tol = tol_mm;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned int)(a.tiles * num_frames)), block(256);
  if (with_parts) hipLaunchKernelGGL(sdf_scene_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(sdf_scene_kernel<false>, grid, block, 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "sdf_scene_kernel");
  // frame minimum, indentation depth, contact ranges: the statements of tacex_indentation_depth (the row kernel's geometry here)
  const char* what = "";
  e = run_frame_outputs(hm_mm_dev, false, nullptr, frame_min_dev, indent_mm_dev, nullptr, nullptr, frame_rows_dev, num_frames, height, width,
                        0.f, 0.f, 0.f, gelpad_height_m, gelpad_to_camera_min_distance_m, st, &what);
  return e == hipSuccess ? 0 : fail_hip(e, what);
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_height_map_from_sdf_scene(const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev, const float* volumes_f_dev,
                                               int num_volumes, const int32_t* part_ids_dev, const float* part_pose_dev,
                                               const int32_t* part_ops_dev, int num_slots, float pixmm, float near_clip_mm, float far_clip_mm,
                                               int max_steps, float tol_mm, float gelpad_height_m, float gelpad_to_camera_min_distance_m,
                                               float* hm_mm_dev, float* frame_min_dev, float* indent_mm_dev, int32_t* frame_rows_dev,
                                               int num_frames, int height, int width, void* stream) {
  return tacex::run_sdf_scene("tacex_height_map_from_sdf_scene", voxels_dev, num_voxels, volumes_i_dev, volumes_f_dev, num_volumes, part_ids_dev,
                              part_pose_dev, part_ops_dev, num_slots, pixmm, near_clip_mm, far_clip_mm, max_steps, tol_mm, gelpad_height_m,
                              gelpad_to_camera_min_distance_m, hm_mm_dev, frame_min_dev, indent_mm_dev, frame_rows_dev, nullptr, false,
                              num_frames, height, width, stream);
}

extern "C" int tacex_height_map_from_sdf_scene_parts(const float* voxels_dev, int num_voxels, const int32_t* volumes_i_dev,
                                                     const float* volumes_f_dev, int num_volumes, const int32_t* part_ids_dev,
                                                     const float* part_pose_dev, const int32_t* part_ops_dev, int num_slots, float pixmm,
                                                     float near_clip_mm, float far_clip_mm, int max_steps, float tol_mm, float gelpad_height_m,
                                                     float gelpad_to_camera_min_distance_m, float* hm_mm_dev, float* frame_min_dev,
                                                     float* indent_mm_dev, int32_t* frame_rows_dev, uint8_t* part_map_dev, int num_frames,
                                                     int height, int width, void* stream) {
  return tacex::run_sdf_scene("tacex_height_map_from_sdf_scene_parts", voxels_dev, num_voxels, volumes_i_dev, volumes_f_dev, num_volumes,
                              part_ids_dev, part_pose_dev, part_ops_dev, num_slots, pixmm, near_clip_mm, far_clip_mm, max_steps, tol_mm,
                              gelpad_height_m, gelpad_to_camera_min_distance_m, hm_mm_dev, frame_min_dev, indent_mm_dev, frame_rows_dev,
                              part_map_dev, true, num_frames, height, width, stream);
}
