// Matrix-core (v_mfma_f32_16x16x4_f32) band kernels of the Taxim pyramid levels - see the banner below; the contact rule: taxim_device.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "tacex_internal.h"
#include "taxim_blur.h"
#include "taxim_device.h"

namespace tacex {

// ------------------------------------------------------------------------------------------------
// MFMA band kernel: the separable Gaussian as two banded-Toeplitz matrix products on the matrix cores, with
// v_mfma_f32_16x16x4_f32 (f32 in / f32 accumulate, bit-identical to a k-ordered fmaf chain, 32 cycles per 1024 MACs).
//   band   = NTILE x 16 rows x W columns of one frame; a 16-row tile contracts over WIN = 16 + 2 RA rows / columns,
//            RA = R rounded up to 8 (zero taps beyond R)
//   V-pass : Out[16 x 64] = Tv[16 x WIN] * In[WIN x 64] per tile and 64-column super-block (one per wave).  In comes
//            straight from global / L2: ONE 16-byte load per lane and k-step feeds 4 MFMAs of EVERY tile whose window
//            holds the row (column j of block v is column c0 + 4 j + v, so the four accumulators of a lane hold 4
//            adjacent columns -> 16-byte LDS stores).  k-step ks of lane group g = lane >> 4 contracts window row
//            4 ks + g, so tile t uses union k-steps [4 t, 4 t + KS) with the SAME weight table.  The L2 -> L1 read
//            amplification (16 NTILE + 2 RA) / (16 NTILE) is what bounds the k = 61 level: 5x at NTILE = 1, 3x at 2.
//   H-pass : Out^T[16 cols x 16 rows] = Th^T * Mid^T per 16-column block, Mid from LDS.  Here k-step ks of lane group g
//            contracts window column KS g + ks (each group walks CONSECUTIVE columns: one ds_read_b128 = four k-steps),
//            and the transposed product leaves a lane with four consecutive columns of one row, so the masked restore
//            and the 16-byte global stores run straight from the accumulators.
// Band weights per lane (0 outside the band), i = lane & 15:
//   V: wl[ks] = w[4 ks + g - RA - i + R]    H: wl[ks] = w[KS g + ks - RA - i + R]     (host tables, [2][KS][64])
// WLDS: the two tables are a re-indexing of ONE zero-padded copy of the filter (mfma_wpad_index, tacex_internal.h), 384 B at
// K = 61 against 10 KB of tables.  The workgroup copies it into LDS behind `mid` (one or two 4-byte loads per lane) and reads
// every wl[ks] from there - many lanes per word, a broadcast - so that the V-pass window and the restore are the only vector
// loads left.  Same f32 weights, same MFMA order: bit-identical.  One copy per WAVE (no barrier: a wave's LDS operations complete
// in order) where that keeps the workgroups per CU, one per WORKGROUP behind a barrier otherwise (BlurArgs::wlds_shared).  The
// press depth and, where the registers allow (HPRE), the H-pass weights are fetched ahead of the barrier: neither depends on `mid`.
// Useful MACs / issued MACs = K / WIN (0.76 at K = 61, 0.69 at 33, 0.53 at 17).
// ------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
#ifndef TACEX_MFMA_CH
#define TACEX_MFMA_CH 4
#endif
#ifndef TACEX_MFMA_FENCE
#define TACEX_MFMA_FENCE 0
#endif
// H-pass contraction map: 0 = window column KS g + ks (one ds_read_b128 per four k-steps, default), 1 = 4 ks + g like the
// V-pass (taps of every output column added in the same order; one ds_read_b32 per k-step, measured 3-5 % slower and
// without an observable difference in the bins of flat regions)
#ifndef TACEX_MFMA_H_CONSEC
#define TACEX_MFMA_H_CONSEC 0
#endif

// LEAN (GZ with rows_ext only, BlurArgs::lean): the loads of the V-pass window and of the masked restore go through raw buffer
// descriptors of the frame, and a lane whose four pixels cannot matter - outside the contact rectangle [lo, hi] x [clo, chi] of
// frame_rows_kernel for the height map, outside the rectangle grown by ext_grow / ext_grow_x for the previous level - gets an
// out-of-range offset: the load returns 0 without touching memory.  That 0 IS the value the full load finds for a previous level
// (stored +0.0f); for the height map the operand J = min(S, 0) = +0.0f is selected / the mask bit cleared by the same predicate
// (S >= 0 outside the rectangle: it comes from the same float32 expression).  No branch encloses a load, an LDS read or an MFMA:
// the instruction stream is the one of the full kernel with buffer_load in place of global_load.
// The body is a device function: blur_mfma_kernel runs it over its own grid (block index and count from blockIdx / gridDim),
// blur_mfma_pipe_kernel (PIPE) runs the bodies of several levels, of different chunks of frames, side by side in sub-ranges of one grid
// and hands each its role-local block index and block count.
template <int K, bool FIRST, int NTILE, bool GZ, bool LEAN, bool WLDS, bool PIPE = false>
__device__ __forceinline__ void blur_mfma_body(const BlurArgs a, int block, int nblocks) {
  static_assert(GZ || !LEAN, "the lean loads need J = min(S, 0)");
  static_assert(!WLDS || !TACEX_MFMA_H_CONSEC, "WLDS reads the H weights in the default contraction map");
  constexpr unsigned kNoLoad = 0x80000000u;  // buffer offset beyond every frame: the range check drops the load, the lane reads 0
  constexpr int TH = 16 * NTILE;
  constexpr int R = (K - 1) / 2, RA = (R + 7) & ~7, WIN = 16 + 2 * RA, KS = WIN / 4;
  constexpr int KU = KS + 4 * (NTILE - 1);  // k-steps over the union window of the band's tiles
#ifndef TACEX_MFMA_CH61
#define TACEX_MFMA_CH61 TACEX_MFMA_CH
#endif
#ifndef TACEX_MFMA_CH117
#define TACEX_MFMA_CH117 TACEX_MFMA_CH
#endif
  constexpr int CH = K == 61 ? TACEX_MFMA_CH61 : (K == 117 ? TACEX_MFMA_CH117 : TACEX_MFMA_CH), NCH = KU / CH;  // k-steps per software-pipeline chunk
  static_assert(KU % CH == 0 && KS % 4 == 0, "window");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* mid = reinterpret_cast<float*>(smem_raw);  // TH x pitch, columns padded by RA on both sides
  const int H = a.H, W = a.W, pitch = a.pitch;
  const int lid = PIPE ? xcd_remap(block, nblocks) : xcd_remap(blockIdx.x, gridDim.x);
  const int frame = lid / a.nbands;
  const int band = lid - frame * a.nbands;
  // the last band of a frame is shifted up when TH does not divide H: its first rows recompute (identically) what the
  // band above stores - cheaper than a second, nearly empty launch for the remainder
  const int by0 = min(a.row0 + band * TH, H - TH);
  const size_t fo = (size_t)frame * H * W;
  const float* __restrict__ src = FIRST ? a.hm + fo : a.src + fo;
  const float* __restrict__ hm = a.hm + fo;
  const float* __restrict__ gel = a.gel;
  if constexpr (GZ) {
    // Zero-band skipping: with a zero gel map the pyramid input J = min(S, 0) is non-zero only on the frame's contact rows
    // [lo, hi] (frame_rows_kernel), and level l's input only within ext_grow rows of them.  A band whose whole window lies
    // outside has an exactly zero blur and no contact pixel to restore: store zeros, read nothing.  (Reflect padding cannot
    // bring a non-zero row in: a mirrored row index -k maps to row k, which the window contains as well.)
    if (LEAN || a.rows_ext != nullptr) {
      const int lo = a.rows_ext[4 * frame] - a.ext_grow, hi = a.rows_ext[4 * frame + 1] + a.ext_grow;
      if (by0 - R > hi || by0 + TH - 1 + R < lo) {
        if constexpr (LEAN)
          if (a.zero_bands_unread) return;  // no reader loads these rows (run_band_levels)
        const int w4 = W >> 2;
        for (int i = threadIdx.x; i < TH * w4; i += blockDim.x) {
          const int r = i / w4, c = i - r * w4;
          reinterpret_cast<v4f*>(a.dst + fo + (size_t)(by0 + r) * W)[c] = (v4f)(0.0f);
          if (a.mask_out) reinterpret_cast<uchar4*>(a.mask_out + fo + (size_t)(by0 + r) * W)[c] = (uchar4){0, 0, 0, 0};
        }
        return;
      }
    }
  }
  const float sa = a.shift_a[frame], sb = a.shift_b[frame];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // one 64-column super-block per wave
  const int li = lane & 15, g = lane >> 4;
  const int c0 = wid << 6;
  // Zero-BLOCK skipping (round 5): the same argument along x.  This level's input is non-zero only in the columns [in_lo, in_hi] =
  // the frame's contact columns grown by the previous levels' radii: a wave whose 64 columns lie outside has an exactly zero
  // V-pass result (it stores zeros - and zeros into the mirrored padding it owns - without loading or multiplying anything), and a
  // wave whose columns lie more than R outside has an exactly zero H-pass result and no contact pixel to restore (stores zeros,
  // reads neither the LDS rows nor the height map).  With a contact patch of ~90 columns two of the five waves of a 320-wide band
  // take these paths.  (Mirrored x-padding cannot bring a non-zero column in: position -c maps to column c, inside the window too.)
#ifndef TACEX_MFMA_BLOCK_SKIP_MIN_K
#define TACEX_MFMA_BLOCK_SKIP_MIN_K 0  // (A/B hook: levels below this kernel size are compiled without the block tests)
#endif
  // LEAN: the frame's contact rectangle and the frame-sized buffer descriptors (wave-uniform: kernel arguments and the block index)
  int ct_lo = 0, ct_hi = 0, ct_clo = 0, ct_chi = 0;
  __amdgpu_buffer_rsrc_t src_rs, hm_rs;
  if constexpr (LEAN) {
    ct_lo = a.rows_ext[4 * frame]; ct_hi = a.rows_ext[4 * frame + 1];
    ct_clo = a.rows_ext[4 * frame + 2]; ct_chi = a.rows_ext[4 * frame + 3];
    src_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, H * W * (int)sizeof(float), 0x00020000);
    hm_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(hm), 0, H * W * (int)sizeof(float), 0x00020000);
  }
  bool v_need = true, h_need = true;
  if constexpr (GZ && K >= TACEX_MFMA_BLOCK_SKIP_MIN_K) {
    if (LEAN || a.rows_ext != nullptr) {
      const int in_lo = a.rows_ext[4 * frame + 2] - a.ext_grow_x, in_hi = a.rows_ext[4 * frame + 3] + a.ext_grow_x;
      v_need = !(c0 + 63 < in_lo || c0 > in_hi);
      h_need = !(c0 + 63 < in_lo - R || c0 > in_hi + R);
#ifdef TACEX_MFMA_NO_BLOCK_SKIP  // (A/B hook)
      v_need = h_need = true;
#endif
    }
  }

  // WLDS: the zero-padded filter (behind the lane tables in a.taps) into LDS behind `mid`; index clamped, not predicated: the
  // lanes beyond the last entry store that entry again
  const float* wts = nullptr;
  if constexpr (WLDS) {
    constexpr int NP = mfma_wpad_floats(K);
    float* wcopy = mid + TH * pitch + (a.wlds_shared ? 0 : wid * NP);
    const float* __restrict__ wpad = a.taps + 2 * KS * 64;
#pragma unroll
    for (int j = 0; j < (NP + 63) / 64; ++j) {
      const int idx = min(lane + 64 * j, NP - 1);
      wcopy[idx] = wpad[idx];
    }
    if (a.wlds_shared) __syncthreads();  // (workgroup-uniform; every wave that got here takes part, whatever its v_need / h_need)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    wts = wcopy + mfma_wpad_index(0, li);
  }
  // H-pass operands that do not depend on `mid`: WLDS fetches the press depth ahead of the barrier (behind the V-pass chain).
  // HPRE: the weights too, where the instantiation stays within 64 VGPRs with them live across the barrier (hipcc 7.x, gfx950: lean
  // k = 17 / 15 / 9 65 and lean non-first k = 61 67 with them, 61 / 60 without; k = 117 holds 36 of them: 71).  The four restore loads
  // ahead of the barrier cost 68 / 68 / 78 / 98 VGPRs at k = 17 / 33 / 61 / 117 (16 more registers live through the whole H chain,
  // which otherwise takes them over from the weights it has used up): not built.
#ifndef TACEX_MFMA_WLDS_HPRE
#define TACEX_MFMA_WLDS_HPRE 1  // (A/B hook: 0 = every instantiation reads the H weights behind the barrier)
#endif
  // PIPE (a role of blur_mfma_pipe_kernel): the lean k = 33 level reads them behind the barrier - with both lean levels holding them across it
  // the fused kernel needs 68 VGPRs, or spills one at 64 (profiles/band_pipeline.md).
  constexpr bool HPRE = WLDS && TACEX_MFMA_WLDS_HPRE && (LEAN ? ((K == 33 && !PIPE) || (K == 61 && FIRST)) : K <= 61);
  float wh[WLDS ? KS : 1];
  float pd_pre = 0.0f;
  auto read_wh = [&]() {
    static_for<0, KS / 4>([&](auto mc) {
      constexpr int m = decltype(mc)::value;
      const float* wq = wts + mfma_h_window_col(KS, g, 4 * m);  // four consecutive k-steps = four consecutive window columns
      wh[4 * m] = wq[0]; wh[4 * m + 1] = wq[1]; wh[4 * m + 2] = wq[2]; wh[4 * m + 3] = wq[3];
    });
  };

  // ---- V-pass ----
  {
    float wl[KS];
    static_for<0, KS>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      if constexpr (WLDS) wl[ks] = wts[4 * ks + g];
      else wl[ks] = a.taps[ks * 64 + lane];
    });
    f32x4 acc[NTILE][4];
#pragma unroll
    for (int t = 0; t < NTILE; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[t][v] = (f32x4)(0.0f);
    const int rb = by0 - RA + g;
    const unsigned coff = (unsigned)(c0 + 4 * li);
    v4f xb[2][CH], gb[FIRST ? 2 : 1][FIRST ? CH : 1];
    // LEAN: rows / columns in which this level's input can be non-zero; `vin`: the lane's window row of a k-step lies inside
    const int vr_lo = ct_lo - a.ext_grow, vr_hi = ct_hi + a.ext_grow;
    const bool vcol = LEAN & ((int)coff + 3 >= ct_clo - a.ext_grow_x) & ((int)coff <= ct_chi + a.ext_grow_x);  // (&: no short-circuit branches)
    bool vin[2][(LEAN && FIRST) ? CH : 1];
    auto issue = [&](auto chunk_c) {
      constexpr int chunk = decltype(chunk_c)::value;
      static_for<0, CH>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        int yy = reflect_idx(rb + 4 * (chunk * CH + c), H);
        yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);  // zero-weight rows beyond the reflect range: any finite data
        const unsigned off = (unsigned)yy * (unsigned)W + coff;
        if constexpr (LEAN) {
          const bool in = vcol & (yy >= vr_lo) & (yy <= vr_hi);
          xb[chunk & 1][c] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(src_rs, in ? off * 4u : kNoLoad, 0, 0));
          if constexpr (FIRST) vin[chunk & 1][c] = in;
        } else {
          xb[chunk & 1][c] = *reinterpret_cast<const v4f*>(src + off);
        }
        if constexpr (FIRST) gb[chunk & 1][c] = GZ ? (v4f)(0.0f) : *reinterpret_cast<const v4f*>(gel + off);  // GZ: gel == 0 everywhere
      });
    };
    if (v_need) {
    issue(std::integral_constant<int, 0>{});
    static_for<0, NCH>([&](auto chunk_c) {
      constexpr int chunk = decltype(chunk_c)::value;
      if constexpr (TACEX_MFMA_FENCE) __builtin_amdgcn_sched_barrier(0);
      if constexpr (chunk + 1 < NCH) issue(std::integral_constant<int, chunk + 1>{});
      if constexpr (TACEX_MFMA_FENCE) __builtin_amdgcn_sched_barrier(0);
      static_for<0, CH>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        constexpr int ku = chunk * CH + c;
        v4f x = xb[chunk & 1][c];
        if constexpr (FIRST) {  // the level's input J (TT:441, TT:454).  fminf, not the inline-asm fmin_raw: the hazard
          const v4f gq = gb[chunk & 1][c];  // recognizer cannot see asm feeding an MFMA
#pragma unroll
          for (int k = 0; k < 4; ++k) x[k] = contact_input<false>(contact_shifted(x[k], sa, sb), gq[k]);
          if constexpr (LEAN) {  // nothing was loaded: J = +0.0f, what min(S, 0) gives outside the contact rectangle
            const bool in = vin[chunk & 1][c];
            x.x = in ? x.x : 0.0f; x.y = in ? x.y : 0.0f; x.z = in ? x.z : 0.0f; x.w = in ? x.w : 0.0f;
          }
        }
        static_for<0, NTILE>([&](auto tc) {
          constexpr int t = decltype(tc)::value;
          constexpr int ks = ku - 4 * t;
          if constexpr (ks >= 0 && ks < KS) {
            const float w = wl[ks];
            acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x.x, acc[t][0], 0, 0, 0);
            acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x.y, acc[t][1], 0, 0, 0);
            acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x.z, acc[t][2], 0, 0, 0);
            acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x.w, acc[t][3], 0, 0, 0);
          }
        });
      });
    });
    }
    if constexpr (WLDS) {  // behind the V-pass chain (its weights are dead), ahead of the barrier: the latency overlaps the wait
      if constexpr (HPRE) read_wh();
      pd_pre = a.pdepth[frame];
    }
    // D layout: column (lane & 15), row 4 (lane >> 4) + reg.  The lanes next to the left / right image border also write
    // the mirrored x-padding (torch 'reflect': position -c <- c, (W-1)+c <- (W-1)-c, c = 1..RA), so one barrier suffices.
    const int cx = c0 + 4 * li;
#pragma unroll
    for (int t = 0; t < NTILE; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* rowp = mid + (16 * t + 4 * g + r) * pitch + RA;
        const float e[4] = {acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]};
        *reinterpret_cast<v4f*>(rowp + cx) = (v4f){e[0], e[1], e[2], e[3]};
        if (cx <= RA) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (cx + v >= 1 && cx + v <= RA) rowp[-(cx + v)] = e[v];
        }
        if (cx + 3 >= W - 1 - RA) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (cx + v >= W - 1 - RA && cx + v <= W - 2) rowp[2 * (W - 1) - (cx + v)] = e[v];
        }
      }
  }
  __syncthreads();
  // ---- H-pass + masked restore: per tile, four adjacent 16-column blocks per wave (four independent chains) ----
  {
    float wl[KS];
    if constexpr (WLDS && !HPRE) read_wh();
    static_for<0, KS>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      if constexpr (WLDS) wl[ks] = wh[ks];
      else wl[ks] = a.taps[((TACEX_MFMA_H_CONSEC ? 0 : KS) + ks) * 64 + lane];
    });
    const float thr = contact_threshold(WLDS ? pd_pre : a.pdepth[frame], a.contact_scale);
    if (!h_need) {  // (wave-uniform) exactly zero output, no contact pixel in these columns
#pragma unroll
      for (int t = 0; t < NTILE; ++t) {
        const int hrow = TACEX_MFMA_H_CONSEC ? li : mfma_h_row(li);
        const size_t p0 = (size_t)(by0 + 16 * t + hrow) * W + c0 + 4 * g;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          *reinterpret_cast<v4f*>(a.dst + fo + p0 + 16 * n) = (v4f)(0.0f);
          if (a.mask_out) *reinterpret_cast<uchar4*>(a.mask_out + fo + p0 + 16 * n) = (uchar4){0, 0, 0, 0};
        }
      }
      return;
    }
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
      f32x4 acc[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[n] = (f32x4)(0.0f);
      // restore operands: issued ahead of the MFMA chain so their latency hides behind it
      const int hrow = TACEX_MFMA_H_CONSEC ? li : mfma_h_row(li);  // tile row of this lane (see mfma_h_window_col)
      const size_t p0 = (size_t)(by0 + 16 * t + hrow) * W + c0 + 4 * g;
      v4f hv[4], gv[4];
      // LEAN: only a lane whose row lies on the contact rows and whose four columns meet the contact columns can restore a pixel
      const int orow = by0 + 16 * t + hrow;
      const bool hrow_in = LEAN & (orow >= ct_lo) & (orow <= ct_hi);
      bool hin[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if constexpr (LEAN) {
          const int oc = c0 + 4 * g + 16 * n;
          hin[n] = hrow_in & (oc + 3 >= ct_clo) & (oc <= ct_chi);
          hv[n] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(hm_rs, hin[n] ? (unsigned)(p0 + 16 * n) * 4u : kNoLoad, 0, 0));
        } else {
          hin[n] = true;
          hv[n] = *reinterpret_cast<const v4f*>(hm + p0 + 16 * n);
        }
        gv[n] = GZ ? (v4f)(0.0f) : *reinterpret_cast<const v4f*>(gel + p0 + 16 * n);
      }
      if constexpr (TACEX_MFMA_H_CONSEC) {
        // k-step ks of lane group g contracts window column 4 ks + g (same map, same table as the V-pass): every output
        // column then adds its taps in the SAME order 0..K-1, so a flat input gives a bit-exactly flat output (no
        // round-off texture for the shading to turn into noise bins).  One ds_read_b32 per block and k-step.
        const float* arow = mid + (16 * t + li) * pitch + g + c0;
        static_for<0, KS>([&](auto kc) {
          constexpr int ks = decltype(kc)::value;
          float q[4];
#pragma unroll
          for (int n = 0; n < 4; ++n) q[n] = arow[16 * n + 4 * ks];
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[ks], q[n], acc[n], 0, 0, 0);
        });
      } else {
        const float* arow = mid + (16 * t + hrow) * pitch + c0;  // window column mfma_h_window_col(KS, g, 4 m ..) of block n: + 16 n
        static_for<0, KS / 4>([&](auto mc) {
          constexpr int m = decltype(mc)::value;
          const int hcol = mfma_h_window_col(KS, g, 4 * m);
          v4f q[4];
#pragma unroll
          for (int n = 0; n < 4; ++n) q[n] = *reinterpret_cast<const v4f*>(arow + 16 * n + hcol);
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[4 * m], q[n].x, acc[n], 0, 0, 0);
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[4 * m + 1], q[n].y, acc[n], 0, 0, 0);
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[4 * m + 2], q[n].z, acc[n], 0, 0, 0);
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[4 * m + 3], q[n].w, acc[n], 0, 0, 0);
        });
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        v4f o;
        uint8_t mk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float S = contact_shifted(hv[n][k], sa, sb);
          const float J = contact_input<false>(S, gv[n][k]);
          const bool M = contact_mask(S, J, gv[n][k], thr) & hin[n];
          o[k] = contact_restore(a.restore, M, J, acc[n][k]);
          mk[k] = M ? 1 : 0;
        }
        *reinterpret_cast<v4f*>(a.dst + fo + p0 + 16 * n) = o;
        if (a.mask_out) *reinterpret_cast<uchar4*>(a.mask_out + fo + p0 + 16 * n) = (uchar4){mk[0], mk[1], mk[2], mk[3]};
      }
    }
  }
}

template <int K, bool FIRST, int NTILE, bool GZ, bool LEAN, bool WLDS>
__global__ __launch_bounds__(640) void blur_mfma_kernel(BlurArgs a) {
  blur_mfma_body<K, FIRST, NTILE, GZ, LEAN, WLDS>(a, blockIdx.x, gridDim.x);
}

// PIPE KERNEL: the levels of SUCCESSIVE chunks of frames in one grid.  The levels of one frame depend on each other, the chunks of a pass
// do not: level 0 of chunk n, level 1 of chunk n - 1, level 2 of chunk n - 2 .. are independent work ("roles").  Role r owns the blocks
// [first[r], first[r + 1]) of the grid, of which the first nblocks[r] run the body of level r with their role-local index; the rest
// (each range is padded to a multiple of 8, so that block % 8 - the XCD - is the same in the role as in the grid and xcd_remap keeps
// the bands of a frame on one XCD) return at once.  A role without a chunk has no blocks.  No workgroup waits for another: order between
// the launches comes from the stream.  The role is workgroup-uniform, so each body keeps its own barrier.
struct PipeArgs {
  BlurArgs role[kPipeMaxRoles];
  int first[kPipeMaxRoles + 1];
  int nblocks[kPipeMaxRoles];
};

template <bool GZ, bool LEAN, bool WLDS, int R, int K, int... KN>
__device__ __forceinline__ void pipe_role(const PipeArgs& p, int b) {
  if (b < p.first[R + 1]) {
    const int lb = b - p.first[R];
    if (lb < p.nblocks[R]) blur_mfma_body<K, R == 0, 1, GZ, LEAN, WLDS, true>(p.role[R], lb, p.nblocks[R]);
    return;
  }
  if constexpr (sizeof...(KN) > 0) pipe_role<GZ, LEAN, WLDS, R + 1, KN...>(p, b);
}

template <bool GZ, bool LEAN, bool WLDS, int K0, int... KN>
// (eight waves per SIMD - 64 VGPRs, six workgroups of five waves per CU like the levels - asked for: left alone the allocator takes 66-68)
__global__ __launch_bounds__(640, 8) void blur_mfma_pipe_kernel(PipeArgs p) {
  pipe_role<GZ, LEAN, WLDS, 0, K0, KN...>(p, (int)blockIdx.x);
}

static void mfma_geometry(int K, BlurArgs* a) {
  const int RA = ((K - 1) / 2 + 7) & ~7;
  a->row0 = 0;
  a->nbands = a->H / 16;
  a->padx = RA;
  a->pitch = a->W + 2 * RA + 4;  // (as launch_mfma_tiles)
  if (((a->pitch >> 2) & 1) == 0) a->pitch += 4;
}

// Workgroups per CU of a level as launch_mfma_tiles launches it: the most of {lane tables, filter copy per wave, copy per workgroup}.
// *n_min becomes the lesser of itself and that count.
template <int K, bool FIRST, bool GZ, bool LEAN>
static hipError_t level_resident(int W, bool wlds, int* n_min) {
  BlurArgs g{}; g.H = 16; g.W = W;
  mfma_geometry(K, &g);
  const size_t lds = (size_t)16 * g.pitch * sizeof(float), wbytes = (size_t)mfma_wpad_floats(K) * sizeof(float);
  auto kern = blur_mfma_kernel<K, FIRST, 1, GZ, LEAN, false>;
  static size_t granted[64] = {};
  int n = 0;
  if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds, granted); e != hipSuccess) return e;
  if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kern), W, lds); e != hipSuccess) return e;
  if constexpr (!TACEX_MFMA_H_CONSEC) {
    if (wlds) {
      auto kern_w = blur_mfma_kernel<K, FIRST, 1, GZ, LEAN, true>;
      static size_t granted_w[64] = {};
      if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern_w), lds + (size_t)(W / 64) * wbytes, granted_w); e != hipSuccess) return e;
      for (const size_t l : {lds + (size_t)(W / 64) * wbytes, lds + wbytes}) {
        int m = 0;
        if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&m, reinterpret_cast<const void*>(kern_w), W, l); e != hipSuccess) return e;
        if (m > n) n = m;
      }
    }
  }
  if (n < *n_min) *n_min = n;
  return hipSuccess;
}

// How a pipe kernel is launched on a device at a width: decided once (PipePlan::W), like the WLDS mode of launch_mfma_tiles.
// mode 1: every role takes its filter copy per wave; 2: per workgroup where the per-wave copies would not fit the launch's LDS (the
// largest role's `mid` + one copy), per wave elsewhere; 0: lane tables; -1: the fused kernel would hold fewer workgroups per CU than
// the per-level launches do - not launched, the caller keeps the per-level schedule.
struct PipePlan { int W, mode; size_t lds; int shared[kPipeMaxRoles]; };

template <bool GZ, bool LEAN, int K0, int... KN>
static hipError_t pipe_plan(int W, bool wlds, const PipePlan** out) {
  constexpr int N = 1 + sizeof...(KN);
  constexpr int ks[N] = {K0, KN...};
  static PipePlan plans[64][2] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  PipePlan& pl = plans[dev][wlds ? 1 : 0];
  *out = &pl;
  if (pl.W == W) return hipSuccess;
  // what the per-level launches hold today: the least of the roles
  int n_ref = 1 << 30, r = 0;
  hipError_t e = level_resident<K0, true, GZ, LEAN>(W, wlds, &n_ref);
  ((e = e != hipSuccess ? e : level_resident<KN, false, GZ, LEAN>(W, wlds, &n_ref)), ...);
  if (e != hipSuccess) return e;
  size_t mid[N], wb[N], lds_mid = 0, lds_wave = 0, lds_wg = 0;
  for (r = 0; r < N; ++r) {
    BlurArgs g{}; g.H = 16; g.W = W;
    mfma_geometry(ks[r], &g);
    mid[r] = (size_t)16 * g.pitch * sizeof(float);
    wb[r] = (size_t)mfma_wpad_floats(ks[r]) * sizeof(float);
    lds_mid = mid[r] > lds_mid ? mid[r] : lds_mid;
    lds_wave = mid[r] + (W / 64) * wb[r] > lds_wave ? mid[r] + (W / 64) * wb[r] : lds_wave;
    lds_wg = mid[r] + wb[r] > lds_wg ? mid[r] + wb[r] : lds_wg;
  }
  auto kern = blur_mfma_pipe_kernel<GZ, LEAN, false, K0, KN...>;
  static size_t granted[64] = {}, granted_w[64] = {};
  pl.mode = -1;
  if constexpr (!TACEX_MFMA_H_CONSEC) {
    if (wlds) {
      auto kern_w = blur_mfma_pipe_kernel<GZ, LEAN, true, K0, KN...>;
      if (e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern_w), lds_wave, granted_w); e != hipSuccess) return e;
      int n_wave = 0, n_wg = 0;
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_wave, reinterpret_cast<const void*>(kern_w), W, lds_wave);
      if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_wg, reinterpret_cast<const void*>(kern_w), W, lds_wg);
      if (e != hipSuccess) return e;
      if (n_wave >= n_ref) { pl.mode = 1; pl.lds = lds_wave; }
      else if (n_wg >= n_ref) { pl.mode = 2; pl.lds = lds_wg; }
      for (r = 0; r < N; ++r) pl.shared[r] = (pl.mode == 2 && mid[r] + (W / 64) * wb[r] > lds_wg) ? 1 : 0;
    }
  }
  if (pl.mode < 0) {
    if (e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_mid, granted); e != hipSuccess) return e;
    int n_old = 0;
    if (e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_old, reinterpret_cast<const void*>(kern), W, lds_mid); e != hipSuccess) return e;
    if (n_old >= n_ref) { pl.mode = 0; pl.lds = lds_mid; }
  }
  pl.W = W;
  return hipSuccess;
}

template <bool GZ, bool LEAN, int K0, int... KN>
static hipError_t launch_pipe(const BlurArgs* roles, int W, bool wlds, hipStream_t st) {
  constexpr int N = 1 + sizeof...(KN);
  constexpr int ks[N] = {K0, KN...};
  const PipePlan* pl = nullptr;
  if (hipError_t e = pipe_plan<GZ, LEAN, K0, KN...>(W, wlds, &pl); e != hipSuccess) return e;
  if (pl->mode < 0) return hipErrorInvalidConfiguration;
  PipeArgs p{};
  int at = 0;
  for (int r = 0; r < N; ++r) {
    p.role[r] = roles[r];
    mfma_geometry(ks[r], &p.role[r]);
    p.role[r].wlds_shared = pl->shared[r];
    p.first[r] = at;
    p.nblocks[r] = roles[r].B > 0 ? p.role[r].nbands * roles[r].B : 0;
    at += (p.nblocks[r] + 7) & ~7;
  }
  for (int r = N; r <= kPipeMaxRoles; ++r) p.first[r] = at;
  if (at == 0) return hipSuccess;
  if constexpr (!TACEX_MFMA_H_CONSEC) {
    if (pl->mode > 0) {
      hipLaunchKernelGGL((blur_mfma_pipe_kernel<GZ, LEAN, true, K0, KN...>), dim3(at), dim3(W), pl->lds, st, p);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((blur_mfma_pipe_kernel<GZ, LEAN, false, K0, KN...>), dim3(at), dim3(W), pl->lds, st, p);
  return hipGetLastError();
}

template <int K, bool FIRST, int NTILE, bool GZ, bool LEAN = false>
static hipError_t launch_mfma_tiles(BlurArgs a, int row0, int nbands, hipStream_t st) {
  constexpr int TH = 16 * NTILE, R = (K - 1) / 2, RA = (R + 7) & ~7;
  a.row0 = row0;
  a.nbands = nbands;
  a.padx = RA;
  a.pitch = a.W + 2 * RA + 4;  // multiple of 4 with an odd quotient: the 16 rows of a ds_read_b128 hit distinct bank groups
  if (((a.pitch >> 2) & 1) == 0) a.pitch += 4;
  static const size_t lds_pad = getenv("TACEX_MFMA_LDS_PAD") ? (size_t)atoi(getenv("TACEX_MFMA_LDS_PAD")) * 1024 : 0;  // occupancy A/B hook
  const size_t lds = (size_t)TH * a.pitch * sizeof(float) + lds_pad;
  auto kern = blur_mfma_kernel<K, FIRST, NTILE, GZ, LEAN, false>;
  static size_t granted[64] = {};
  if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds, granted); e != hipSuccess) return e;
  if constexpr (!TACEX_MFMA_H_CONSEC) {
    if (a.wlds) {
      // WLDS: the filter copy behind `mid` - one per wave where the runtime still places as many workgroups on a CU as of the
      // instantiation without it (and no fewer than with one copy), else one per workgroup (a barrier more), else the lane tables.
      // Decided once per device and width.
      auto kern_w = blur_mfma_kernel<K, FIRST, NTILE, GZ, LEAN, true>;
      const size_t wbytes = (size_t)mfma_wpad_floats(K) * sizeof(float);
      const size_t lds_w[3] = {0, lds + (size_t)(a.W / 64) * wbytes, lds + wbytes};
      static size_t granted_w[64] = {};
      static struct { int W, mode; } plan[64] = {};
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
      if (plan[dev].W != a.W) {
        if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern_w), lds_w[1], granted_w); e != hipSuccess) return e;
        int n_old = 0, n_wave = 0, n_wg = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_old, reinterpret_cast<const void*>(kern), a.W, lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_wave, reinterpret_cast<const void*>(kern_w), a.W, lds_w[1]);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_wg, reinterpret_cast<const void*>(kern_w), a.W, lds_w[2]);
        if (e != hipSuccess) return e;
        plan[dev].mode = (n_wave >= n_old && n_wave >= n_wg) ? 1 : (n_wg >= n_old ? 2 : 0);
        plan[dev].W = a.W;
      }
      if (const int mode = plan[dev].mode) {
        a.wlds_shared = mode == 2 ? 1 : 0;
        hipLaunchKernelGGL(kern_w, dim3(nbands * a.B), dim3(a.W), lds_w[mode], st, a);
        return hipGetLastError();
      }
    }
  }
  hipLaunchKernelGGL(kern, dim3(nbands * a.B), dim3(a.W), lds, st, a);
  return hipGetLastError();
}

// Band height: NTILE = 1 (16 rows).  Taller bands (NTILE = 2 / 3, shared V-pass loads: 3x / 2.3x instead of 5x L2 -> L1
// read amplification at k = 61) are supported by the kernel and were measured 3-8 % SLOWER at 256 x 320x240 (fewer,
// longer workgroups per CU), so only NTILE = 1 is instantiated.  a.gel == nullptr selects the all-zero-gel variant.
#ifndef TACEX_MFMA_NT117
#define TACEX_MFMA_NT117 1  // A/B: band height (16-row tiles) of the k = 117 level (640x480: 9x L2 -> L1 read amplification at 1, 5x at 2)
#endif
#ifndef TACEX_MFMA_NT61
#define TACEX_MFMA_NT61 1
#endif
template <int K, bool FIRST>
static hipError_t launch_mfma(const BlurArgs& a, hipStream_t st) {
  constexpr int NT = K == 117 ? TACEX_MFMA_NT117 : (K == 61 ? TACEX_MFMA_NT61 : 1);
  if (NT > 1 && a.H % (16 * NT) == 0 && a.W > 320) {  // (taller bands only where the window is many times the band: the 640-wide levels)
    if (a.gel == nullptr && a.lean && a.rows_ext) return launch_mfma_tiles<K, FIRST, NT, true, true>(a, 0, a.H / (16 * NT), st);
    if (a.gel == nullptr) return launch_mfma_tiles<K, FIRST, NT, true>(a, 0, a.H / (16 * NT), st);
    return launch_mfma_tiles<K, FIRST, NT, false>(a, 0, a.H / (16 * NT), st);
  }
  if (a.gel == nullptr && a.lean && a.rows_ext) return launch_mfma_tiles<K, FIRST, 1, true, true>(a, 0, a.H / 16, st);
  if (a.gel == nullptr) return launch_mfma_tiles<K, FIRST, 1, true>(a, 0, a.H / 16, st);
  return launch_mfma_tiles<K, FIRST, 1, false>(a, 0, a.H / 16, st);
}

// TACEX_BLUR_MFMA: 1 (default) = matrix-core band kernels where compiled (k = 117 / 61 / 33 / 17), 0 = VALU band kernels only
static int mfma_enabled() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("TACEX_BLUR_MFMA"); v = e ? atoi(e) : 1; }
  return v;
}

bool mfma_supported(int k, bool first, int H, int W) {
  if (!mfma_enabled() || W % 64 != 0 || W < 64 || W > 640 || H % 16 != 0) return false;
  const int R = (k - 1) / 2;
  if (R >= H || R > W - 1 || ((R + 7) & ~7) >= W) return false;
  if (first) return k == 61 || k == 117;
  return k == 117 || k == 61 || k == 33 || k == 17 || k == 15 || k == 9;
}

hipError_t dispatch_mfma(int k, bool first, const BlurArgs& a, hipStream_t st) {
  if (first) return k == 117 ? launch_mfma<117, true>(a, st) : launch_mfma<61, true>(a, st);
  switch (k) {
    case 117: return launch_mfma<117, false>(a, st);
    case 61: return launch_mfma<61, false>(a, st);
    case 33: return launch_mfma<33, false>(a, st);
    case 17: return launch_mfma<17, false>(a, st);
    case 15: return launch_mfma<15, false>(a, st);
    case 9: return launch_mfma<9, false>(a, st);
    default: return hipErrorInvalidValue;
  }
}

// The pipe kernel is instantiated for the default level set of W = 320, {61, 33, 17}, with the zero gel map and 16-row bands; everything
// else keeps the per-level launches.  Not for {117, 61, 33, 15} (W = 640): its lean instantiations need 66 - 76 VGPRs, and spill 2 - 6 of
// them when held to 64 (profiles/band_pipeline.md).
bool mfma_pipe_supported(const int* ks, int n, int H, int W) {
  if (TACEX_MFMA_H_CONSEC || TACEX_MFMA_NT61 != 1) return false;
  for (int l = 0; l < n; ++l)
    if (!mfma_supported(ks[l], l == 0, H, W)) return false;
  return n == 3 && ks[0] == 61 && ks[1] == 33 && ks[2] == 17;
}

hipError_t mfma_pipe_resident(const int* ks, int n, int H, int W, bool lean, bool wlds, bool* ok) {
  *ok = false;
  if (!mfma_pipe_supported(ks, n, H, W)) return hipErrorInvalidValue;
  const PipePlan* pl = nullptr;
  const hipError_t e = lean ? pipe_plan<true, true, 61, 33, 17>(W, wlds, &pl) : pipe_plan<true, false, 61, 33, 17>(W, wlds, &pl);
  *ok = e == hipSuccess && pl->mode >= 0;
  return e;
}

hipError_t dispatch_mfma_pipe(const int* ks, int n, int H, int W, bool lean, bool wlds, const BlurArgs* roles, hipStream_t st) {
  if (!mfma_pipe_supported(ks, n, H, W)) return hipErrorInvalidValue;
  return lean ? launch_pipe<true, true, 61, 33, 17>(roles, W, wlds, st) : launch_pipe<true, false, 61, 33, 17>(roles, W, wlds, st);
}

}  // namespace tacex
