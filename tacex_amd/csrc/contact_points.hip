// Contact point cloud of the optical path (tacex_contact_points): a fixed-size set of K surface points per env, sampled evenly from
// the contact pixels of the height map - ONE launch, a stream compaction without atomics or global scratch.  The contract - which
// pixel is a contact pixel, the rank of one, which rank a slot takes, every float32 operation of a point - is the comment of
// tacex_contact_points in include/tacex_hip.h; tests/contact_points_ref.py restates it in NumPy.  This file is compiled with
// -ffp-contract=off (tacex_amd/_build.py): every product and sum below rounds on its own.
//
// Shape: one workgroup of 256 threads per FRAME (the frame index is wave-uniform), in three phases.  The frame's contact rectangle
// (the whole frame without one) is a row-major sequence of ITEMS of four consecutive pixels of a row (one 16-byte load each on the
// vector path); wave w walks the w-th quarter of that sequence in steps of 64 items, so a wave meets its pixels in rank order.
//   1. count    every thread counts the contact pixels of its items; DPP scan per wave, the four wave totals through LDS: N, and the
//               rank of every wave's first contact pixel.
//   2. select   the walk again with a running rank base per wave: the four pixel predicates of the wave's 64 items go through
//               __ballot, mbcnt gives a lane the number of contact pixels in the lanes below it, __popcll advances the base - a lane
//               knows the rank r of each of its contact pixels with no barrier and no LDS.  A pixel that is the source of a slot
//               writes its linear index to sel[slot] in LDS: slot r when N <= K, else the slot of the inverse formula, of which there
//               is at most one (quotient and remainder of the running rank are carried: a multiplication per item, a carry per pixel).
//   3. points   slot-centric: thread k reads sel[k] (sel[k mod N] for repeat), taps the height map and stores - only K pixels pay
//               for the gradient, the square root and the divisions, and a wave's stores are consecutive slots.
// Frames are independent workgroups and a frame's result is a function of its own pixels: the same bits in every batch and call.
// The price is two reads of the rectangle (the second from L2) and, for a batch of fewer frames than the GPU has room for
// workgroups, idle CUs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "stage_args.h"
#include "tacex_hip.h"
#include "tacex_internal.h"
#include "tacex_philox.h"
#include "wave_ops.h"

namespace tacex {
namespace {

constexpr int kCpBlock = 256;
constexpr int kCpWaves = kCpBlock / 64;
constexpr int kCpGroup = 4;  // items whose loads a thread issues together

struct ContactPointsArgs {
  const float* hm;        // (B,H,W)
  const float* fmin;      // (B,)
  const float* indent;    // (B,)
  const int32_t* rects;   // (B,4) or nullptr
  const uint8_t* labels;  // (B,H,W) or nullptr
  const float* pose;      // (B,12) or nullptr
  float* points;          // (B,K,3)
  float* normals;         // (B,K,3) or nullptr
  float* depth;           // (B,K) or nullptr
  int32_t* pixels;        // (B,K,2) or nullptr
  uint8_t* labels_out;    // (B,K) or nullptr
  int32_t* count;         // (B,2) or nullptr
  float pixmm, min_depth, unit;
  int label, K, pad, jitter, H, W;
  uint64_t seed;
  int64_t frame_offset;
  uint32_t call;
};

// what the walk of a frame needs (uniform over the workgroup)
struct CpFrame {
  const float* hm;
  const uint8_t* labels;  // nullptr when the label filter is off
  float fmin, indent, min_depth;
  int label, W, r0, c0, c1, g0;
  unsigned groups, magic;  // items per rectangle row, and floor((2^32 - 1) / groups)
};

// lanes below this one whose bit is set in m, added to acc
__device__ __forceinline__ unsigned lanes_below(unsigned long long m, unsigned acc) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, acc));
}

// Item idx of the rectangle -> its row i, first column j0 and height map / label values.  idx / groups by one multiplication: with
// magic = floor((2^32 - 1) / groups) the high word of idx * magic is the quotient or one below it for every idx < 2^32.
template <bool kVec>
__device__ __forceinline__ void load_item(const CpFrame& f, unsigned idx, int& i, int& j0, float (&h)[4], unsigned& lab) {
  unsigned q = __umulhi(idx, f.magic), r = idx - q * f.groups;
  if (r >= f.groups) { q += 1; r -= f.groups; }
  i = f.r0 + (int)q;
  j0 = (f.g0 + (int)r) * 4;
  const size_t o = (size_t)i * f.W + j0;
  lab = 0;
  if constexpr (kVec) {
    const float4 v = *reinterpret_cast<const float4*>(f.hm + o);
    h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
    if (f.labels) lab = *reinterpret_cast<const uint32_t*>(f.labels + o);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in_row = j0 + k < f.W;
      h[k] = in_row ? f.hm[o + k] : 0.0f;  // past the row's end: masked by the column range below
      if (f.labels && in_row) lab |= (unsigned)f.labels[o + k] << (8 * k);
    }
  }
}

// bit k: pixel (i, j0 + k) is a contact pixel
__device__ __forceinline__ unsigned item_contact(const CpFrame& f, int j0, const float (&h)[4], unsigned lab) {
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = j0 + k;
    const float S = (h[k] - f.fmin) - f.indent;
    const float d = S < 0.0f ? -S : 0.0f;  // a NaN compares false
    const bool pass = !f.labels || (int)((lab >> (8 * k)) & 255u) == f.label;
    if (j >= f.c0 && j <= f.c1 && d > f.min_depth && pass) m |= 1u << k;
  }
  return m;
}

template <bool kVec>
__global__ __launch_bounds__(kCpBlock) void contact_points_kernel(ContactPointsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int cp_sel[];  // (K) linear pixel index of every slot's source
  __shared__ int s_wave[kCpWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned int frame = blockIdx.x;
  const int H = a.H, W = a.W, K = a.K;

  // ---- the frame's scalars (uniform over the workgroup) ----
  int r0 = 0, r1 = H - 1, c0 = 0, c1 = W - 1;
  if (a.rects) {  // clamped to the image: a rectangle can skip pixels, never address outside the frame
    const int32_t* q = a.rects + (size_t)frame * 4;
    r0 = max(q[0], 0); r1 = min(q[1], H - 1); c0 = max(q[2], 0); c1 = min(q[3], W - 1);
  }
  const bool any = r0 <= r1 && c0 <= c1;
  const size_t fbase = (size_t)frame * (size_t)H * (size_t)W;
  const float* __restrict__ hm = a.hm + fbase;
  CpFrame f;
  f.hm = hm;
  f.labels = (a.labels && a.label >= 0) ? a.labels + fbase : nullptr;
  f.fmin = a.fmin[frame]; f.indent = a.indent[frame]; f.min_depth = a.min_depth;
  f.label = a.label; f.W = W; f.r0 = r0; f.c0 = c0; f.c1 = c1; f.g0 = c0 >> 2;
  f.groups = any ? (unsigned)((c1 >> 2) - (c0 >> 2) + 1) : 1u;
  f.magic = 0xffffffffu / f.groups;
  const unsigned items = any ? (unsigned)(r1 - r0 + 1) * f.groups : 0u;  // <= H * W < 2^31
  // wave w walks items [first, last): the w-th quarter of the sequence, in whole steps of 64
  const unsigned steps = (items + 63u) / 64u, per_wave = (steps + kCpWaves - 1) / kCpWaves;
  const unsigned first = min((unsigned)wave * per_wave * 64u, items), last = min(first + per_wave * 64u, items);

  // ---- 1. count ----
  int mine = 0;
  for (unsigned base = first; base < last; base += 64u * kCpGroup) {
    int i[kCpGroup], j0[kCpGroup];
    float h[kCpGroup][4];
    unsigned lab[kCpGroup];
    bool in[kCpGroup];
#pragma unroll
    for (int n = 0; n < kCpGroup; ++n) {
      const unsigned idx = base + 64u * n + lane;
      in[n] = idx < last;
      if (in[n]) load_item<kVec>(f, idx, i[n], j0[n], h[n], lab[n]);
    }
#pragma unroll
    for (int n = 0; n < kCpGroup; ++n)
      if (in[n]) mine += __popc(item_contact(f, j0[n], h[n], lab[n]));
  }
  mine = wave_scan_add_lane63(mine);
  if (lane == 63) s_wave[wave] = mine;
  __syncthreads();
  int N = 0, rank = 0;  // contact pixels of the frame; rank of this wave's first one
#pragma unroll
  for (int w = 0; w < kCpWaves; ++w) {
    if (w == wave) rank = N;
    N += s_wave[w];
  }

  // ---- the offset of the subsample ----
  uint64_t off = 0;
  if (a.jitter && N > K) {
    const uint64_t g = (uint64_t)(a.frame_offset + (int64_t)frame);
    const uint32_t ctr[4] = {(uint32_t)g, (uint32_t)(g >> 32), a.call, 0x70747363u};
    const uint32_t key[2] = {(uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    off = ((uint64_t)w[0] * (uint64_t)N) >> 32;
  }

  // ---- 2. select ----
  // N > K: rank r starts at slot ceil((r K - off) / N) = floor((r K + (N - 1 - off)) / N), the numerator never negative.  The wave
  // carries quotient and remainder of its running rank (one 64-bit division per wave); a lane, `below` <= 252 ranks further, and the
  // next step, at most 256 ranks further, add at most 2^22 to the remainder: a 32-bit quotient by one multiplication (div_n).
  const bool sub = N > K;
  const unsigned Nu = (unsigned)N, Ku = (unsigned)K, magic_n = 0xffffffffu / (sub ? Nu : 1u);
  unsigned slot_w = 0, rem_w = 0;  // slot and remainder at which the wave's running rank starts
  if (sub) {
    const uint64_t num = (uint64_t)rank * Ku + ((uint64_t)(Nu - 1u) - off);
    slot_w = (unsigned)(num / Nu);
    rem_w = (unsigned)(num - (uint64_t)slot_w * Nu);
  }
  // t < 2^32 -> t / N, t left as t mod N
  auto div_n = [&](unsigned& t) {
    unsigned q = __umulhi(t, magic_n);
    t -= q * Nu;
    if (t >= Nu) { q += 1; t -= Nu; }
    return q;
  };
  for (unsigned base = first; base < last; base += 64u * kCpGroup) {
    int i[kCpGroup], j0[kCpGroup];
    float h[kCpGroup][4];
    unsigned lab[kCpGroup];
    bool in[kCpGroup];
#pragma unroll
    for (int n = 0; n < kCpGroup; ++n) {
      const unsigned idx = base + 64u * n + lane;
      in[n] = idx < last;
      if (in[n]) load_item<kVec>(f, idx, i[n], j0[n], h[n], lab[n]);
    }
#pragma unroll
    for (int n = 0; n < kCpGroup; ++n) {
      const unsigned m = in[n] ? item_contact(f, j0[n], h[n], lab[n]) : 0u;
      unsigned below = 0, total = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned long long bal = __ballot((m >> k) & 1u);
        below = lanes_below(bal, below);
        total += (unsigned)__popcll(bal);
      }
      if (m) {
        const int p0 = i[n] * W + j0[n];
        if (!sub) {
          int r = rank + (int)below;  // rank of the item's first contact pixel
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if ((m >> k) & 1u) {
              if (r < K) cp_sel[r] = p0 + k;  // (r < N <= K unless the map changed between the two walks)
              r += 1;
            }
        } else {
          unsigned rem = rem_w + below * Ku;
          unsigned slot = slot_w + div_n(rem);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!((m >> k) & 1u)) continue;
            rem += Ku;  // rank r + 1 adds K < N: one carry at most
            if (rem >= Nu) {  // the next rank starts at the next slot: this pixel is the source of `slot`
              rem -= Nu;
              if (slot < Ku) cp_sel[slot] = p0 + k;  // (always, unless the map changed between the two walks)
              slot += 1;
            }
          }
        }
      }
      rank += (int)total;
      if (sub) {
        rem_w += total * Ku;
        slot_w += div_n(rem_w);
      }
    }
  }
  __syncthreads();

  // ---- 3. points ----
  const float fmin = f.fmin, indent = f.indent, pixmm = a.pixmm, unit = a.unit;
  const float cx0 = (float)(W - 1) / 2.0f, cy0 = (float)(H - 1) / 2.0f;
  float R[12];
  if (a.pose) {
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k] = a.pose[(size_t)frame * 12 + k];
  }
  const uint8_t* labels = a.labels ? a.labels + fbase : nullptr;
  const size_t obase = (size_t)frame * (size_t)K;
  for (int k = tid; k < K; k += kCpBlock) {
    int src = -1;
    if (sub || k < N) src = cp_sel[k];
    else if (a.pad && N > 0) src = cp_sel[k % N];
    if ((unsigned)src >= (unsigned)(H * W)) src = -1;  // (no slot's source is outside the frame unless the map changed between the two walks)
    float p[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f}, d = 0.0f;
    int pi = -1, pj = -1;
    unsigned lab = 255u;
    if (src >= 0) {
      pi = src / W; pj = src - pi * W;
      const float S = (hm[src] - fmin) - indent;
      d = S < 0.0f ? -S : 0.0f;
      float q[3] = {((float)pj - cx0) * pixmm * unit, ((float)pi - cy0) * pixmm * unit, unit * S};
      float gx = 0.0f, gy = 0.0f;
      if (W > 1) {
        const int jl = max(pj - 1, 0), jr = min(pj + 1, W - 1);
        gx = (hm[src - pj + jr] - hm[src - pj + jl]) / ((float)(jr - jl) * pixmm);
      }
      if (H > 1) {
        const int il = max(pi - 1, 0), ir = min(pi + 1, H - 1);
        gy = (hm[(size_t)ir * W + pj] - hm[(size_t)il * W + pj]) / ((float)(ir - il) * pixmm);
      }
      const float s = sqrtf((gx * gx + gy * gy) + 1.0f);
      float n3[3] = {gx / s, gy / s, -1.0f / s};
      if (a.pose) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          p[r] = ((R[4 * r] * q[0] + R[4 * r + 1] * q[1]) + R[4 * r + 2] * q[2]) + R[4 * r + 3];
          nrm[r] = (R[4 * r] * n3[0] + R[4 * r + 1] * n3[1]) + R[4 * r + 2] * n3[2];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) { p[r] = q[r]; nrm[r] = n3[r]; }
      }
      lab = labels ? (unsigned)labels[src] : 0u;
    }
    const size_t o = obase + k;
    a.points[o * 3] = p[0]; a.points[o * 3 + 1] = p[1]; a.points[o * 3 + 2] = p[2];
    if (a.normals) { a.normals[o * 3] = nrm[0]; a.normals[o * 3 + 1] = nrm[1]; a.normals[o * 3 + 2] = nrm[2]; }
    if (a.depth) a.depth[o] = d;
    if (a.pixels) { a.pixels[o * 2] = pi; a.pixels[o * 2 + 1] = pj; }
    if (a.labels_out) a.labels_out[o] = (uint8_t)lab;
  }
  if (tid == 0 && a.count) {
    a.count[(size_t)frame * 2] = N;
    a.count[(size_t)frame * 2 + 1] = N == 0 ? 0 : (N >= K || a.pad) ? K : N;
  }
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_contact_points(const float* hm_mm_dev, const float* frame_min_dev, const float* indent_mm_dev, const int32_t* frame_rows_dev,
                                    const uint8_t* labels_dev, int label, float pixmm, float min_depth_mm, int max_points, int pad,
                                    const float* pose_dev, float unit, int jitter, uint64_t seed, int64_t frame_offset, uint32_t call,
                                    float* points_dev, float* normals_dev, float* depth_dev, int32_t* pixels_dev, uint8_t* labels_out_dev,
                                    int32_t* count_dev, int num_frames, int height, int width, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_contact_points";
  if (null_arg(fn, "hm_mm_dev", hm_mm_dev) || null_arg(fn, "frame_min_dev", frame_min_dev) || null_arg(fn, "indent_mm_dev", indent_mm_dev) ||
      null_arg(fn, "points_dev", points_dev) || not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) ||
      not_positive(fn, "width", width)) return 2;
  if ((long long)height * width > 0x7fffffffll) return refuse_image_launch(fn, num_frames, height, width);
  if (!(pixmm > 0.0f)) { set_error("%s: pixmm = %g (must be > 0)", fn, (double)pixmm); return 2; }
  if (!(unit > 0.0f)) { set_error("%s: unit = %g (must be > 0)", fn, (double)unit); return 2; }
  if (!(min_depth_mm >= 0.0f)) { set_error("%s: min_depth_mm = %g (must be >= 0)", fn, (double)min_depth_mm); return 2; }
  if (max_points < 1 || max_points > TACEX_CONTACT_POINTS_MAX) {
    set_error("%s: max_points = %d outside [1, %d]", fn, max_points, TACEX_CONTACT_POINTS_MAX);
    return 2;
  }
  if (pad != 0 && pad != 1) { set_error("%s: pad = %d (0: zero fill, 1: repeat)", fn, pad); return 2; }
  if (label < -1 || label > 254) { set_error("%s: label = %d outside [-1, 254]", fn, label); return 2; }
  if (label >= 0 && !labels_dev) { set_error("%s: label = %d needs labels_dev, which is null", fn, label); return 2; }
  ContactPointsArgs a{};
  a.hm = hm_mm_dev; a.fmin = frame_min_dev; a.indent = indent_mm_dev; a.rects = frame_rows_dev; a.labels = labels_dev; a.pose = pose_dev;
  a.points = points_dev; a.normals = normals_dev; a.depth = depth_dev; a.pixels = pixels_dev; a.labels_out = labels_out_dev; a.count = count_dev;
  a.pixmm = pixmm; a.min_depth = min_depth_mm; a.unit = unit;
  a.label = label; a.K = max_points; a.pad = pad; a.jitter = jitter != 0; a.H = height; a.W = width;
  a.seed = seed; a.frame_offset = frame_offset; a.call = call;
  const bool vec = width % 4 == 0 && (uintptr_t)hm_mm_dev % 16 == 0 && (label < 0 || (uintptr_t)labels_dev % 4 == 0);
  const void* kern = vec ? (const void*)contact_points_kernel<true> : (const void*)contact_points_kernel<false>;
  const size_t lds = (size_t)max_points * sizeof(int);
  if (lds > 48 * 1024) {  // an opt-in per kernel and device, inside what a workgroup can get
    static size_t avail_vec[64] = {}, avail_scalar[64] = {}, granted_vec[64] = {}, granted_scalar[64] = {};
    size_t limit = 0;
    hipError_t e = dynamic_lds_limit(kern, vec ? avail_vec : avail_scalar, &limit);
    if (e != hipSuccess) return fail_hip(e, "contact_points_kernel (LDS limit)");
    if (lds > limit) {
      set_error("%s: max_points = %d needs %zu bytes of LDS per workgroup (limit %zu)", fn, max_points, lds, limit);
      return 2;
    }
    e = ensure_dynamic_lds(kern, lds, vec ? granted_vec : granted_scalar);
    if (e != hipSuccess) return fail_hip(e, "contact_points_kernel (dynamic LDS)");
  }
  const dim3 grid((unsigned int)num_frames), block(kCpBlock);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(contact_points_kernel<true>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(contact_points_kernel<false>, grid, block, lds, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "contact_points_kernel");
}
