// The trilinear tap of a signed-distance grid, shared by the volume source (volume_source.hip) and the scene source (sdf_scene.hip):
// one copy of the clamp into the grid's box, the eight loads and the seven lerps of the contract of tacex_height_map_from_sdf
// (include/tacex_hip.h).  Both units are built with -ffp-contract=off: every product and sum is rounded to float32 on its own.
#pragma once
#include <hip/hip_runtime.h>

namespace tacex {

constexpr int kSdfTileW = 32, kSdfTileH = 8;  // 2 x 2 waves of 16 x 4 pixels
constexpr float kSdfTwo30 = 1073741824.0f;

__device__ __forceinline__ float sdf_lerp(float p, float q, float t) { return p + (t * (q - p)); }

// A volume of the library under a pose row r (16 floats): its grid (first voxel, N = (Wv, Hv, D)) and the coefficients of the rays
// q[k](z) = ((q0[k] + x * ax[k]) + y * ay[k]) + z * az[k] in voxel coordinates, with ia[k] = 1 / az[k] (par[k]: too small to divide
// by), hmax[k] = N[k] - 1 and vox = scale * pitch, one voxel in camera mm.  false - and the library is not read - for an id outside
// [0, P), a table row the host would not have written, or a pose that fails the contract's checks (a NaN or inf fails them).
__device__ __forceinline__ bool sdf_load_slot(int id, const int* vi_table, const float* vf_table, int P, int num_voxels, const float* r, float pixmm,
                                              int* first, int N[3], float ax[3], float ay[3], float az[3], float q0[3], float ia[3],
                                              float hmax[3], bool par[3], float* scale, float* level, float* step_scale, float* vox) {
  *first = 0; N[0] = N[1] = N[2] = 2;
  *scale = *level = *step_scale = *vox = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) { ax[k] = ay[k] = az[k] = q0[k] = ia[k] = 0.f; hmax[k] = 1.f; par[k] = true; }
  if (!(id >= 0 && id < P)) return false;  // no such volume
  const int* vi = vi_table + 4 * (size_t)id;
  const float* vf = vf_table + 8 * (size_t)id;
  *first = vi[0]; N[2] = vi[1]; N[1] = vi[2]; N[0] = vi[3];
  const float pitch = vf[0], anchor[3] = {vf[1], vf[2], vf[3]};
  *step_scale = vf[4];
  if (*first < 0 || N[0] < 2 || N[1] < 2 || N[2] < 2 || (long long)*first + (long long)N[2] * N[1] * N[0] > (long long)num_voxels) return false;
  const float tx = r[9], ty = r[10], tz = r[11];
  *scale = r[12]; *level = r[13];
  const float g = *scale * pitch;
  const float inv = 1.0f / g;
  *vox = g;
  bool ok = g > 0.0f && *step_scale > 0.0f && fabsf(*level) < kSdfTwo30;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ax[k] = (r[k] * pixmm) * inv;
    ay[k] = (r[3 + k] * pixmm) * inv;
    az[k] = r[6 + k] * inv;
    q0[k] = anchor[k] - ((((r[k] * tx) + (r[3 + k] * ty)) + (r[6 + k] * tz)) * inv);
    par[k] = !(fabsf(az[k]) >= 1e-12f);
    ia[k] = par[k] ? 0.0f : 1.0f / az[k];
    hmax[k] = (float)(N[k] - 1);
    ok = ok && fabsf(ax[k]) < kSdfTwo30 && fabsf(ay[k]) < kSdfTwo30 && fabsf(az[k]) < kSdfTwo30 && fabsf(q0[k]) < kSdfTwo30;
  }
  return ok;
}

// the ray q[k](z) = bq[k] + z * az[k] (ia[k] = 1 / az[k], par[k]: the ray runs along the box's faces of axis k) against the grid's box
// [0, hmax[k]], clipping [*lo, *hi] in place: false when the interval is empty or a coordinate is not below 2^30
__device__ __forceinline__ bool sdf_clip(const float bq[3], const float ia[3], const float hmax[3], const bool par[3], float* lo, float* hi) {
  bool some = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    some = some && fabsf(bq[k]) < kSdfTwo30;
    if (par[k]) {
      some = some && bq[k] >= 0.0f && bq[k] <= hmax[k];
    } else {
      const float t1 = (0.0f - bq[k]) * ia[k], t2 = (hmax[k] - bq[k]) * ia[k];
      const float tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
      *lo = tn > *lo ? tn : *lo;
      *hi = tf < *hi ? tf : *hi;
    }
  }
  return some && *lo <= *hi;
}

// q clamped into [0, hmax]: the lower cell index m (the upper neighbour m + 1 stays in the grid) and the weight w; returns the
// clamped coordinate
__device__ __forceinline__ float sdf_cell(float q, float hmax, int n, int* m, float* w) {
  float c = q > 0.0f ? q : 0.0f;  // (a NaN: 0 - the index stays legal whatever the pose)
  c = c < hmax ? c : hmax;
  *m = min((int)floorf(c), n - 2);
  *w = c - (float)*m;
  return c;
}

// the grid `vol` with strides sy (one y step) and sz (one z step), interpolated x then y then z
__device__ __forceinline__ float sdf_tap(const float* __restrict__ vol, int sy, int sz, const int m[3], const float w[3]) {
  const float* v = vol + ((m[2] * sz + m[1] * sy) + m[0]);
  const float v000 = v[0], v001 = v[1], v010 = v[sy], v011 = v[sy + 1];
  const float v100 = v[sz], v101 = v[sz + 1], v110 = v[sz + sy], v111 = v[sz + sy + 1];
  const float e00 = sdf_lerp(v000, v001, w[0]), e01 = sdf_lerp(v010, v011, w[0]);
  const float e10 = sdf_lerp(v100, v101, w[0]), e11 = sdf_lerp(v110, v111, w[0]);
  const float f0 = sdf_lerp(e00, e01, w[1]), f1 = sdf_lerp(e10, e11, w[1]);
  return sdf_lerp(f0, f1, w[2]);
}

}  // namespace tacex
