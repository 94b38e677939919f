// What the two contact kernels share (contact_field.hip: one record per frame; contact_parts.hip: one record per frame and label):
// a frame's scalars, the per-pixel traction of the definition (tacex_contact_field in include/tacex_hip.h) and the reduction of a
// workgroup's per-thread sums to the 16-slot record.  One copy of each: a pixel's terms and a record's slots are the same float32 and
// float64 operations in both, in the same order.  Both units are compiled with -ffp-contract=off (tacex_amd/_build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace tacex {

constexpr int kCfBlock = 256;
constexpr int kCfWaves = kCfBlock / 64;
constexpr int kBandRows = 8;
constexpr int kCfGroup = 4;   // items whose loads a thread issues together
constexpr int kCfSums = 14;
constexpr int kCfRed = 18;  // doubles per wave in the LDS exchange: 14 sums, count, slipping count, maximum, one spare

// float64 sums of a frame (each term is a float32 value widened to float64, or its product with pixel indices formed in float64)
enum { kFx = 0, kFy, kFn, kP, kD, kPj, kPi, kPjj, kPii, kPij, kFni, kFnj, kFyj, kFxi };

struct ContactFrame {
  float fmin, indent, kn, kt, mu, dx, dy, dth, cx, cy;
};

struct ContactPixel {
  float d, p, tx, ty;
  bool slip;
};

// one pixel of the definition (include/tacex_hip.h); h is the height map value, (i, j) its row and column
__device__ inline ContactPixel contact_pixel(const ContactFrame& f, float pixmm, float h, int i, int j) {
  ContactPixel o;
  const float S = (h - f.fmin) - f.indent;
  o.d = S < 0.0f ? -S : 0.0f;  // a NaN compares false
  o.p = f.kn * o.d;
  o.tx = 0.0f; o.ty = 0.0f; o.slip = false;
  if (o.d > 0.0f) {
    const float rx = ((float)j - f.cx) * pixmm, ry = ((float)i - f.cy) * pixmm;
    const float ux = f.dx - f.dth * ry, uy = f.dy + f.dth * rx;
    const float n = sqrtf(ux * ux + uy * uy);
    const float stick = f.kt * n, cone = f.mu * o.p;
    o.slip = stick >= cone;
    if (n != 0.0f) {
      const float s = fminf(stick, cone) / n;
      o.tx = ux * s; o.ty = uy * s;
    }
  }
  return o;
}

// The record of a workgroup's pixels from its threads' sums: wave shuffles (fixed tree), then the waves in order by thread 0, which
// also finishes the record (centre of pressure, torque, principal axis of the pressure).  Every thread of the workgroup calls it
// (one barrier); s_red holds kCfWaves * kCfRed doubles of LDS; `valid` false (a gel id outside the table) writes zeros.
__device__ inline void contact_record(double (&acc)[kCfSums], int count, int nslip, float dmax, double* s_red, double* rec, bool valid, int H,
                                      int W, float pixmm, float area) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kCfSums; ++k) acc[k] += __shfl_down(acc[k], off, 64);
    count += __shfl_down(count, off, 64);
    nslip += __shfl_down(nslip, off, 64);
    dmax = fmaxf(dmax, __shfl_down(dmax, off, 64));
  }
  if (lane == 0) {
    double* w = s_red + wave * kCfRed;
#pragma unroll
    for (int k = 0; k < kCfSums; ++k) w[k] = acc[k];
    w[14] = (double)count; w[15] = (double)nslip; w[16] = (double)dmax;
  }
  __syncthreads();
  if (tid != 0) return;
  double s[kCfRed];
  for (int k = 0; k < 17; ++k) s[k] = s_red[k];
  for (int w = 1; w < kCfWaves; ++w) {
    const double* q = s_red + w * kCfRed;
    for (int k = 0; k < 16; ++k) s[k] += q[k];
    s[16] = fmax(s[16], q[16]);
  }
  if (!valid) {
    for (int k = 0; k < 16; ++k) rec[k] = 0.0;
    return;
  }
  const double cx0 = (double)(W - 1) / 2.0, cy0 = (double)(H - 1) / 2.0;
  const double mm = (double)pixmm, m = mm * 1e-3;  // pixel pitch [mm], [m]
  rec[0] = s[kFx]; rec[1] = s[kFy]; rec[2] = -s[kFn];
  rec[3] = -(s[kFni] - cy0 * s[kFn]) * m;                                       // sum ry fz
  rec[4] = (s[kFnj] - cx0 * s[kFn]) * m;                                        // - sum rx fz
  rec[5] = ((s[kFyj] - cx0 * s[kFy]) - (s[kFxi] - cy0 * s[kFx])) * m;           // sum rx fy - ry fx
  rec[6] = s[kFn];
  rec[7] = s[14] * (double)area;
  rec[8] = s[14];
  rec[11] = s[16];
  rec[12] = s[kD] * (mm * mm);
  rec[13] = s[15];
  double copx = cx0, copy = cy0, angle = 0.0, aspect = 0.0;
  if (s[kP] > 0.0) {
    copx = s[kPj] / s[kP]; copy = s[kPi] / s[kP];
    const double m20 = s[kPjj] / s[kP] - copx * copx, m02 = s[kPii] / s[kP] - copy * copy, m11 = s[kPij] / s[kP] - copx * copy;
    angle = 0.5 * atan2(2.0 * m11, m20 - m02);
    const double mean = 0.5 * (m20 + m02), half = 0.5 * (m20 - m02), rad = sqrt(half * half + m11 * m11);
    const double lmax = mean + rad, lmin = mean - rad;
    if (lmax > 0.0) aspect = sqrt(fmax(lmin, 0.0) / lmax);
  }
  rec[9] = copx; rec[10] = copy; rec[14] = angle; rec[15] = aspect;
}

}  // namespace tacex
