// Contact force field of the optical path (tacex_contact_field): elastic-foundation (Winkler) normal pressure and regularised
// Coulomb shear per pixel of the height map, reduced per env (a 16-slot record) and per cell of a coarse tactile grid, optionally
// written out as a traction image - ONE launch, 4 B / pixel read (only inside the contact rectangle when frame_rows is given).
// The contract - every float32 operation and what each float64 sum holds - is the comment of tacex_contact_field in
// include/tacex_hip.h; tests/contact_field_ref.py restates it in NumPy.  This file is compiled with -ffp-contract=off
// (tacex_amd/_build.py): every product and sum below rounds on its own.
//
// Shape: one workgroup of 256 threads per FRAME, walking the frame in bands of kBandRows rows.  A band is kBandRows x ceil(W / 4)
// items of four consecutive pixels of a row; thread t takes items t, t + 256, ... (one 16-byte load each on the vector path).
// The mapping of pixels to threads and the order in which a thread meets its pixels depend on (H, W) alone - not on the batch, the
// contact rectangle, the grid or which outputs are asked for - and no sum uses an atomic: a frame's outputs are the same bits
// in every call.  The contact rectangle only SKIPS items (and whole bands) whose terms are zero, which changes no float64 sum.
//   record  14 float64 sums, two counts and a maximum per thread in registers -> wave shuffles (fixed tree) -> LDS, added in wave
//           order by thread 0, which also finishes the record (centre of pressure, torque, principal axis of the pressure).
//   cells   the band's pixel forces go to an LDS tile; thread (row of the band, cell column, chunk of 32 pixels) adds its run of
//           pixels in float64, thread (cell column) adds chunks and rows into the carried sum of the cell row in progress and
//           stores a cell when the frame row that ends its cell row has been added.  Two barriers per band that holds contact,
//           none for the others.
//   image   stored by the thread that computed the pixel; zeros outside the contact rectangle.
// Frames are independent workgroups: nothing is handed between workgroups, so there is no flag, counter or second kernel.  The
// price is that a batch of fewer frames than the GPU has room for workgroups (4 per CU) leaves CUs idle, and that a frame's bands
// run one after the other, each exposing a memory round trip - measured in DESIGN 4.0.12a.1.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "contact_terms.h"
#include "stage_args.h"
#include "tacex_hip.h"
#include "tacex_internal.h"

namespace tacex {
namespace {

constexpr int kCfChunk = 32;  // pixels of a cell run that one thread adds

struct ContactArgs {
  const float* hm;         // (B,H,W)
  const float* fmin;       // (B,)
  const float* indent;     // (B,)
  const float* gels;       // (P,4)
  const int32_t* gel_ids;  // (B,) or nullptr
  const float* slip;       // (B,5) or nullptr
  const int32_t* rects;    // (B,4) or nullptr
  double* record;          // (B,16)
  float* cells;            // (B,rows,cols,3) or nullptr
  float* image;            // (B,H,W,3) or nullptr
  float pixmm, area;       // area = float32(pixmm^2 1e-6) [m^2]
  int num_gels, H, W, rows, cols;
  int chunks;              // chunks of kCfChunk pixels per cell run: ceil(ceil(W / cols) / kCfChunk)
};

template <bool kVec>
__global__ __launch_bounds__(kCfBlock) void contact_field_kernel(ContactArgs a) {
  extern __shared__ __attribute__((aligned(16))) char cf_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned int frame = blockIdx.x;
  const int H = a.H, W = a.W, W4 = (W + 3) >> 2, Wp = W4 * 4;
  const bool want_cells = a.cells != nullptr;
  // LDS carve (every offset a multiple of 16): wave exchange | carried cell row | cell column starts | row runs of the band | pixel forces of the band
  double* s_red = reinterpret_cast<double*>(cf_smem);
  double* s_carry = s_red + kCfWaves * kCfRed;
  int* s_col = reinterpret_cast<int*>(s_carry + (((size_t)a.cols * 3 + 1) & ~(size_t)1));
  double* s_run = reinterpret_cast<double*>(s_col + (((size_t)a.cols + 1 + 3) & ~(size_t)3));
  float* s_tile = reinterpret_cast<float*>(s_run + (((size_t)kBandRows * a.cols * a.chunks * 3 + 1) & ~(size_t)1));

  // ---- the frame's scalars (uniform over the workgroup) ----
  ContactFrame f;
  f.fmin = a.fmin[frame]; f.indent = a.indent[frame];
  const float* g = stage_row(a.gels, a.gel_ids, a.num_gels, 4, frame);
  const bool valid = g != nullptr;
  f.kn = f.kt = f.mu = 0.0f;
  if (valid) { f.kn = g[0]; f.kt = g[1]; f.mu = g[2]; }
  f.dx = f.dy = f.dth = f.cx = f.cy = 0.0f;
  if (a.slip) { const float* s = a.slip + (size_t)frame * 5; f.dx = s[0]; f.dy = s[1]; f.dth = s[2]; f.cx = s[3]; f.cy = s[4]; }
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
  float* img = a.image ? a.image + fbase * 3 : nullptr;
  float* cells = want_cells ? a.cells + (size_t)frame * a.rows * a.cols * 3 : nullptr;

  double acc[kCfSums];
#pragma unroll
  for (int k = 0; k < kCfSums; ++k) acc[k] = 0.0;
  int count = 0, nslip = 0;
  float dmax = 0.0f;

  if (want_cells) {
    for (int cj = tid; cj < a.cols; cj += kCfBlock) s_carry[3 * cj] = s_carry[3 * cj + 1] = s_carry[3 * cj + 2] = 0.0;  // column cj is thread cj % 256's alone
    // first pixel column of every cell column: pixel j belongs to cell column (j cols) / W (read behind a band's first barrier)
    for (int cj = tid; cj <= a.cols; cj += kCfBlock) s_col[cj] = (int)(((unsigned)cj * (unsigned)W + (unsigned)a.cols - 1u) / (unsigned)a.cols);
  }
  // thread t's items of a band are t, t + 256, ...: (row of the band, item of the row) advance by (step_r, step_g), no division per item
  const int step_r = kCfBlock / W4, step_g = kCfBlock - step_r * W4;
  const int first_r = tid / W4, first_g = tid - first_r * W4;
  // cell row of the band's first frame row and e = (i rows) mod H: row i ends its cell row when e + rows >= H
  int band_ci = 0, band_e = 0;

  const int nbands = (H + kBandRows - 1) / kBandRows;
  for (int b = 0; b < nbands; ++b) {
    const int i_lo = b * kBandRows, nrow = min(kBandRows, H - i_lo);
    const bool hit = any && i_lo <= r1 && i_lo + nrow - 1 >= r0;  // uniform
    if (hit || img) {
      // items in groups of kCfGroup: the group's loads are issued together, then the pixels are worked off (a thread has
      // ceil(8 W4 / 256) items per band: one group up to W = 512)
      for (int r = first_r, g = first_g; r < nrow;) {
        int gr[kCfGroup], gg[kCfGroup];
        bool gin[kCfGroup];
        float h[kCfGroup][4];
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
            h[n][0] = v.x; h[n][1] = v.y; h[n][2] = v.z; h[n][3] = v.w;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[n][k] = (gg[n] * 4 + k < W) ? hm[o + k] : f.fmin + f.indent;  // past the row's end: never counted
          }
        }
#pragma unroll
        for (int n = 0; n < kCfGroup; ++n) {
          if (gr[n] >= nrow) continue;
          const int i = i_lo + gr[n], j = gg[n] * 4;
          const size_t o = (size_t)i * W + j;
          float px[12];  // (tx, ty, -p) of the four pixels
#pragma unroll
          for (int k = 0; k < 12; ++k) px[k] = 0.0f;
          if (gin[n]) {
            float frc[12];  // (fx, fy, fz) [N] of the four pixels
            double iP = 0.0, iPj = 0.0, iFn = 0.0, iFx = 0.0;  // sums over the item, which lies in one row: their products with i come once
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const ContactPixel c = contact_pixel(f, a.pixmm, h[n][k], i, j + k);
              const bool on = c.d > 0.0f && (kVec || j + k < W);
              const float fx = on ? c.tx * a.area : 0.0f, fy = on ? c.ty * a.area : 0.0f, fn = on ? c.p * a.area : 0.0f;
              frc[3 * k] = fx; frc[3 * k + 1] = fy; frc[3 * k + 2] = -fn;
              if (on) {
                px[3 * k] = c.tx; px[3 * k + 1] = c.ty; px[3 * k + 2] = -c.p;
                const double dj = (double)(j + k), dp = (double)c.p, dfn = (double)fn, dfy = (double)fy, pj = dp * dj;
                iP += dp; iPj += pj; iFn += dfn; iFx += (double)fx;
                acc[kFy] += dfy; acc[kD] += (double)c.d;
                acc[kPjj] += pj * dj; acc[kFnj] += dfn * dj; acc[kFyj] += dfy * dj;
                count += 1; nslip += c.slip ? 1 : 0;
                dmax = fmaxf(dmax, c.d);
              }
            }
            const double di = (double)i, pi = iP * di;
            acc[kFx] += iFx; acc[kFn] += iFn; acc[kP] += iP; acc[kPj] += iPj;
            acc[kPi] += pi; acc[kPii] += pi * di; acc[kPij] += iPj * di; acc[kFni] += iFn * di; acc[kFxi] += iFx * di;
            if (want_cells) {
              float4* t = reinterpret_cast<float4*>(s_tile + ((size_t)gr[n] * Wp + j) * 3);
              t[0] = make_float4(frc[0], frc[1], frc[2], frc[3]);
              t[1] = make_float4(frc[4], frc[5], frc[6], frc[7]);
              t[2] = make_float4(frc[8], frc[9], frc[10], frc[11]);
            }
          }
          if (img) {
            if constexpr (kVec) {
              float4* d = reinterpret_cast<float4*>(img + o * 3);
              d[0] = make_float4(px[0], px[1], px[2], px[3]);
              d[1] = make_float4(px[4], px[5], px[6], px[7]);
              d[2] = make_float4(px[8], px[9], px[10], px[11]);
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (j + k < W) { img[(o + k) * 3] = px[3 * k]; img[(o + k) * 3 + 1] = px[3 * k + 1]; img[(o + k) * 3 + 2] = px[3 * k + 2]; }
            }
          }
        }
      }
    }
    if (!want_cells) continue;
    if (hit) {
      __syncthreads();  // the band's tile is complete
      // chunk q (kCfChunk pixels) of the run of cell column cj in band row r, inside the items the rectangle touches
      const int CK = a.cols * a.chunks;
      for (int k = tid; k < nrow * CK; k += kCfBlock) {
        const int r = (int)((unsigned)k / (unsigned)CK), m = k - r * CK, cj = (int)((unsigned)m / (unsigned)a.chunks), q = m - cj * a.chunks;
        const int i = i_lo + r;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        if (i >= r0 && i <= r1) {
          const int ja = s_col[cj] + q * kCfChunk, jb = min(ja + kCfChunk, s_col[cj + 1]);
          const int j_lo = max(ja, g0 * 4), j_hi = min(jb, g1 * 4 + 4);
          const float* t = s_tile + (size_t)r * Wp * 3;
          for (int j = j_lo; j < j_hi; ++j) { sx += (double)t[3 * j]; sy += (double)t[3 * j + 1]; sz += (double)t[3 * j + 2]; }
        }
        s_run[3 * k] = sx; s_run[3 * k + 1] = sy; s_run[3 * k + 2] = sz;
      }
      __syncthreads();  // the runs are complete (and every read of the tile is done before the next band writes it)
    }
    // chunks and rows of the band into the carried cell row; a cell is stored when the last frame row of its cell row has been added
    for (int cj = tid; cj < a.cols; cj += kCfBlock) {
      double cx = s_carry[3 * cj], cy = s_carry[3 * cj + 1], cz = s_carry[3 * cj + 2];
      int ci = band_ci, e = band_e;
      for (int r = 0; r < nrow; ++r) {
        if (hit) {
          const double* s = s_run + ((size_t)r * a.cols + cj) * a.chunks * 3;
          for (int q = 0; q < a.chunks; ++q) { cx += s[3 * q]; cy += s[3 * q + 1]; cz += s[3 * q + 2]; }
        }
        e += a.rows;
        if (e >= H) {
          float* c = cells + ((size_t)ci * a.cols + cj) * 3;
          c[0] = (float)cx; c[1] = (float)cy; c[2] = (float)cz;
          cx = cy = cz = 0.0;
          e -= H; ci += 1;
        }
      }
      s_carry[3 * cj] = cx; s_carry[3 * cj + 1] = cy; s_carry[3 * cj + 2] = cz;
    }
    for (int r = 0; r < nrow; ++r) {
      band_e += a.rows;
      if (band_e >= H) { band_e -= H; band_ci += 1; }
    }
  }

  // ---- the record: wave shuffles (fixed tree), then the waves in order (contact_terms.h) ----
  contact_record(acc, count, nslip, dmax, s_red, a.record + (size_t)frame * 16, valid, H, W, a.pixmm, a.area);
}

int contact_field_chunks(int W, int cols) { return ((W + cols - 1) / cols + kCfChunk - 1) / kCfChunk; }

size_t contact_field_lds_bytes(int W, int cols, bool want_cells) {
  size_t n = (size_t)kCfWaves * kCfRed * sizeof(double);
  if (!want_cells) return n;
  n += (((size_t)cols * 3 + 1) & ~(size_t)1) * sizeof(double);
  n += (((size_t)cols + 1 + 3) & ~(size_t)3) * sizeof(int);
  n += (((size_t)kBandRows * cols * contact_field_chunks(W, cols) * 3 + 1) & ~(size_t)1) * sizeof(double);
  n += (size_t)kBandRows * (size_t)((W + 3) / 4 * 4) * 3 * sizeof(float);
  return n;
}

}  // namespace
}  // namespace tacex

extern "C" int tacex_contact_field(const float* hm_mm_dev, const float* frame_min_dev, const float* indent_mm_dev, const float* gels_dev,
                                   int num_gels, const int32_t* gel_ids_dev, const float* slip_dev, float pixmm,
                                   const int32_t* frame_rows_dev, int grid_rows, int grid_cols, double* record_dev, float* cells_dev,
                                   float* image_dev, int num_frames, int height, int width, void* stream) {
  using namespace tacex;
  const char* fn = "tacex_contact_field";
  if (null_arg(fn, "hm_mm_dev", hm_mm_dev) || null_arg(fn, "frame_min_dev", frame_min_dev) || null_arg(fn, "indent_mm_dev", indent_mm_dev) ||
      null_arg(fn, "gels_dev", gels_dev) || null_arg(fn, "record_dev", record_dev) || not_positive(fn, "num_gels", num_gels) ||
      not_positive(fn, "num_frames", num_frames) || not_positive(fn, "height", height) || not_positive(fn, "width", width)) return 2;
  if (!(pixmm > 0.0f)) { set_error("tacex_contact_field: pixmm = %g (must be > 0)", (double)pixmm); return 2; }
  if (grid_rows < 1 || grid_rows > height) { set_error("tacex_contact_field: grid_rows = %d outside [1, height = %d]", grid_rows, height); return 2; }
  if (grid_cols < 1 || grid_cols > width) { set_error("tacex_contact_field: grid_cols = %d outside [1, width = %d]", grid_cols, width); return 2; }
  const size_t lds = contact_field_lds_bytes(width, grid_cols, cells_dev != nullptr);
  if (lds > 128 * 1024) {
    set_error("tacex_contact_field: width = %d with grid_cols = %d needs %zu bytes of LDS per workgroup (limit 131072)", width, grid_cols, lds);
    return 2;
  }
  ContactArgs a{};
  a.hm = hm_mm_dev; a.fmin = frame_min_dev; a.indent = indent_mm_dev; a.gels = gels_dev; a.gel_ids = gel_ids_dev; a.slip = slip_dev;
  a.rects = frame_rows_dev; a.record = record_dev; a.cells = cells_dev; a.image = image_dev;
  a.pixmm = pixmm; a.area = (float)((double)pixmm * (double)pixmm * 1e-6);
  a.num_gels = num_gels; a.H = height; a.W = width; a.rows = grid_rows; a.cols = grid_cols;
  a.chunks = contact_field_chunks(width, grid_cols);
  const bool vec = width % 4 == 0 && (uintptr_t)hm_mm_dev % 16 == 0 && (uintptr_t)image_dev % 16 == 0;
  static size_t granted_vec[64] = {}, granted_scalar[64] = {};
  const void* kern = vec ? (const void*)contact_field_kernel<true> : (const void*)contact_field_kernel<false>;
  hipError_t e = ensure_dynamic_lds(kern, lds, vec ? granted_vec : granted_scalar);
  if (e != hipSuccess) return fail_hip(e, "contact_field_kernel (dynamic LDS)");
  const dim3 grid((unsigned int)num_frames), block(kCfBlock);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(contact_field_kernel<true>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(contact_field_kernel<false>, grid, block, lds, st, a);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "contact_field_kernel");
}
