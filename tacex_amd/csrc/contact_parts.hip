// Per-part contact records of the optical path (tacex_contact_field_parts): the per-pixel terms of tacex_contact_field with the slip
// row of the pixel's LABEL, reduced to one 16-slot record per (frame, label), optionally written out as a traction image - ONE launch.
// The contract is the comment of the call in include/tacex_hip.h; tests/contact_parts_ref.py restates it in NumPy.  Compiled with
// -ffp-contract=off (tacex_amd/_build.py).  The pixel's terms and the record's reduction are those of contact_field.hip
// (contact_terms.h: one copy).
//
// Shape: one workgroup of 256 threads per (FRAME, LABEL), walking the frame's contact rectangle in bands of kBandRows rows with the
// thread-to-pixel map of contact_field.hip - items of four consecutive pixels of a row, thread t takes items t, t + 256, ... of a band -
// and keeping the pixels of its label.  A thread meets its pixels in the order contact_field_kernel meets them, so with one label that
// holds every pixel a record is that kernel's, bit for bit; no sum uses an atomic, and nothing is handed between workgroups.  The L
// workgroups of a frame each read the frame's height map and labels (5 B / pixel, from L2 after the first).
//   image   a pixel is stored by the workgroup of its label, a pixel whose label is >= L - no shear, no record - and every pixel
//           outside the contact rectangle (zeros) by label 0's: every pixel is written exactly once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "contact_terms.h"
#include "stage_args.h"
#include "tacex_hip.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

constexpr int kPartsMaxLabels = 8;

struct ContactPartsArgs {
  const float* hm;         // (B,H,W)
  const float* fmin;       // (B,)
  const float* indent;     // (B,)
  const float* gels;       // (P,4)
  const int32_t* gel_ids;  // (B,) or nullptr
  const uint8_t* labels;   // (B,H,W)
  const float* slip;       // (B,L,5) or nullptr
  const int32_t* rects;    // (B,4) or nullptr
  double* record;          // (B,L,16)
  float* image;            // (B,H,W,3) or nullptr
  float pixmm, area;       // area = float32(pixmm^2 1e-6) [m^2]
  int num_gels, L, H, W;
};

template <bool kVec>
__global__ __launch_bounds__(kCfBlock) void contact_parts_kernel(ContactPartsArgs a) {
  __shared__ double s_red[kCfWaves * kCfRed];
  const int tid = threadIdx.x;
  const unsigned int frame = blockIdx.x / (unsigned)a.L;
  const int label = (int)(blockIdx.x - frame * (unsigned)a.L);
  const int H = a.H, W = a.W, W4 = (W + 3) >> 2;

  // ---- the frame's scalars and the label's slip row (uniform over the workgroup) ----
  ContactFrame f;
  f.fmin = a.fmin[frame]; f.indent = a.indent[frame];
  const float* g = stage_row(a.gels, a.gel_ids, a.num_gels, 4, frame);
  const bool valid = g != nullptr;
  f.kn = f.kt = f.mu = 0.0f;
  if (valid) { f.kn = g[0]; f.kt = g[1]; f.mu = g[2]; }
  f.dx = f.dy = f.dth = f.cx = f.cy = 0.0f;
  if (a.slip) { const float* s = a.slip + ((size_t)frame * a.L + label) * 5; f.dx = s[0]; f.dy = s[1]; f.dth = s[2]; f.cx = s[3]; f.cy = s[4]; }
  int r0 = 0, r1 = H - 1, c0 = 0, c1 = W - 1;
  if (a.rects) {  // clamped to the image: a rectangle can skip pixels, never address outside the frame
    const int32_t* q = a.rects + (size_t)frame * 4;
    r0 = max(q[0], 0); r1 = min(q[1], H - 1); c0 = max(q[2], 0); c1 = min(q[3], W - 1);
  }
  if (!valid) r1 = -1;  // an id outside the table: nothing is in contact
  const bool any = r0 <= r1 && c0 <= c1;
  const int g0 = c0 >> 2, g1 = c1 >> 2;  // first / last item of a row that the rectangle touches

  const size_t fbase = (size_t)frame * (size_t)H * (size_t)W;
  const float* __restrict__ hm = a.hm + fbase;
  const uint8_t* __restrict__ labels = a.labels + fbase;
  float* img = a.image ? a.image + fbase * 3 : nullptr;
  const bool fills = img && label == 0;  // label 0's workgroup writes what belongs to no label's

  double acc[kCfSums];
#pragma unroll
  for (int k = 0; k < kCfSums; ++k) acc[k] = 0.0;
  int count = 0, nslip = 0;
  float dmax = 0.0f;

  // thread t's items of a band are t, t + 256, ...: (row of the band, item of the row) advance by (step_r, step_g), no division per item
  const int step_r = kCfBlock / W4, step_g = kCfBlock - step_r * W4;
  const int first_r = tid / W4, first_g = tid - first_r * W4;

  const int nbands = (H + kBandRows - 1) / kBandRows;
  for (int b = 0; b < nbands; ++b) {
    const int i_lo = b * kBandRows, nrow = min(kBandRows, H - i_lo);
    const bool hit = any && i_lo <= r1 && i_lo + nrow - 1 >= r0;  // uniform
    if (!(hit || fills)) continue;
    for (int r = first_r, g = first_g; r < nrow;) {
      int gr[kCfGroup], gg[kCfGroup];
      bool gin[kCfGroup];
      float h[kCfGroup][4];
      int lab[kCfGroup][4];
#pragma unroll
      for (int n = 0; n < kCfGroup; ++n) {
        gr[n] = r; gg[n] = g;
        const int i = i_lo + r;
        gin[n] = r < nrow && hit && i >= r0 && i <= r1 && g >= g0 && g <= g1;
        g += step_g; r += step_r;
        if (g >= W4) { g -= W4; r += 1; }
      }
#pragma unroll
      for (int n = 0; n < kCfGroup; ++n) {
        if (!gin[n]) continue;
        const size_t o = (size_t)(i_lo + gr[n]) * W + gg[n] * 4;
        if constexpr (kVec) {
          const float4 v = *reinterpret_cast<const float4*>(hm + o);
          const uint32_t q = *reinterpret_cast<const uint32_t*>(labels + o);
          h[n][0] = v.x; h[n][1] = v.y; h[n][2] = v.z; h[n][3] = v.w;
#pragma unroll
          for (int k = 0; k < 4; ++k) lab[n][k] = (int)((q >> (8 * k)) & 255u);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool in_row = gg[n] * 4 + k < W;
            h[n][k] = in_row ? hm[o + k] : f.fmin + f.indent;  // past the row's end: never counted
            lab[n][k] = in_row ? (int)labels[o + k] : 255;
          }
        }
      }
#pragma unroll
      for (int n = 0; n < kCfGroup; ++n) {
        if (gr[n] >= nrow) continue;
        const int i = i_lo + gr[n], j = gg[n] * 4;
        const size_t o = (size_t)i * W + j;
        if (!gin[n]) {  // outside the rectangle: zeros, by label 0's workgroup
          if (fills) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (kVec || j + k < W) { img[(o + k) * 3] = 0.0f; img[(o + k) * 3 + 1] = 0.0f; img[(o + k) * 3 + 2] = 0.0f; }
          }
          continue;
        }
        double iP = 0.0, iPj = 0.0, iFn = 0.0, iFx = 0.0;  // sums over the item, which lies in one row: their products with i come once
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in_row = kVec || j + k < W;
          const bool mine = lab[n][k] == label, orphan = lab[n][k] >= a.L;
          const ContactPixel c = contact_pixel(f, a.pixmm, h[n][k], i, j + k);
          const bool on = c.d > 0.0f && in_row;
          if (on && mine) {
            const float fx = c.tx * a.area, fy = c.ty * a.area, fn = c.p * a.area;
            const double dj = (double)(j + k), dp = (double)c.p, dfn = (double)fn, dfy = (double)fy, pj = dp * dj;
            iP += dp; iPj += pj; iFn += dfn; iFx += (double)fx;
            acc[kFy] += dfy; acc[kD] += (double)c.d;
            acc[kPjj] += pj * dj; acc[kFnj] += dfn * dj; acc[kFyj] += dfy * dj;
            count += 1; nslip += c.slip ? 1 : 0;
            dmax = fmaxf(dmax, c.d);
          }
          if (img && in_row && (mine || (orphan && label == 0))) {
            float* d = img + (o + k) * 3;
            d[0] = on && mine ? c.tx : 0.0f; d[1] = on && mine ? c.ty : 0.0f; d[2] = on ? -c.p : 0.0f;
          }
        }
        const double di = (double)i, pi = iP * di;
        acc[kFx] += iFx; acc[kFn] += iFn; acc[kP] += iP; acc[kPj] += iPj;
        acc[kPi] += pi; acc[kPii] += pi * di; acc[kPij] += iPj * di; acc[kFni] += iFn * di; acc[kFxi] += iFx * di;
      }
    }
  }
  contact_record(acc, count, nslip, dmax, s_red, a.record + ((size_t)frame * a.L + label) * 16, valid, H, W, a.pixmm, a.area);
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_contact_field_parts(const float* hm_mm_dev, const float* frame_min_dev, const float* indent_mm_dev, const float* gels_dev,
                                         int num_gels, const int32_t* gel_ids_dev, const uint8_t* labels_dev, int num_labels,
                                         const float* slip_dev, float pixmm, const int32_t* frame_rows_dev, double* record_dev, float* image_dev,
                                         int num_frames, int height, int width, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_contact_field_parts";
  if (null_arg(fn, "hm_mm_dev", hm_mm_dev) || null_arg(fn, "frame_min_dev", frame_min_dev) || null_arg(fn, "indent_mm_dev", indent_mm_dev) ||
      null_arg(fn, "gels_dev", gels_dev) || null_arg(fn, "labels_dev", labels_dev) || null_arg(fn, "record_dev", record_dev) ||
      not_positive(fn, "num_gels", num_gels) || not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) ||
      not_positive(fn, "width", width)) return 2;
  if (num_labels < 1 || num_labels > kPartsMaxLabels) {
    set_error("%s: num_labels = %d (must be 1..%d)", fn, num_labels, kPartsMaxLabels);
    return 2;
  }
  if (!(pixmm > 0.0f)) { set_error("%s: pixmm = %g (must be > 0)", fn, (double)pixmm); return 2; }
  if ((long long)num_frames * num_labels > 0x7fffffffll) return refuse_image_launch(fn, num_frames, height, width);
  ContactPartsArgs a{};
  a.hm = hm_mm_dev; a.fmin = frame_min_dev; a.indent = indent_mm_dev; a.gels = gels_dev; a.gel_ids = gel_ids_dev; a.labels = labels_dev;
  a.slip = slip_dev; a.rects = frame_rows_dev; a.record = record_dev; a.image = image_dev;
  a.pixmm = pixmm; a.area = (float)((double)pixmm * (double)pixmm * 1e-6);
  a.num_gels = num_gels; a.L = num_labels; a.H = height; a.W = width;
  const bool vec = width % 4 == 0 && (uintptr_t)hm_mm_dev % 16 == 0 && (uintptr_t)labels_dev % 4 == 0;
  const dim3 grid((unsigned int)num_frames * (unsigned int)num_labels), block(kCfBlock);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(contact_parts_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(contact_parts_kernel<false>, grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "contact_parts_kernel");
}
