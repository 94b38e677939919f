// FEM device layer: the small kernels around a time step - env launch order, predictor, velocity, reset, attachment aims - and the
// FEM-driven marker kernels (K18).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "tacex_philox.h"

namespace tacex {

// Launch order of the envs for the next Newton launch: counting sort (descending) by the work of the env's previous step,
// key = PCG iterations + 6 per Newton iteration (gradient, block assembly and line search cost about six sweeps), from the
// step_info rows the previous tacex_fem_step left behind (zeros before the first step: index order).  One workgroup; the order
// inside a bucket is whatever the atomics give - it only decides WHEN an env runs, never what it computes.
__global__ __launch_bounds__(1024) void fem_env_order_kernel(const double* __restrict__ step_info, int B, int* __restrict__ order) {
  constexpr int kKeys = 2048;
  __shared__ int hist[kKeys], start[kKeys];
  for (int k = threadIdx.x; k < kKeys; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  auto key_of = [&](int b) {
    const double w = step_info[(size_t)b * 4 + 3] + 6.0 * step_info[(size_t)b * 4 + 0];
    return (w >= 0.0 && w < (double)(kKeys - 1)) ? (int)w : (w >= (double)(kKeys - 1) ? kKeys - 1 : 0);  // (NaN -> 0)
  };
  for (int b = threadIdx.x; b < B; b += blockDim.x) atomicAdd(&hist[key_of(b)], 1);
  __syncthreads();
  if (threadIdx.x < 64) {  // exclusive scan from the heaviest key down, one wave: 32 keys per lane + a lane scan
    const int lane = threadIdx.x;
    int loc = 0;
    for (int k = 0; k < kKeys / 64; ++k) loc += hist[kKeys - 1 - (lane * (kKeys / 64) + k)];
    int inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    int acc = inc - loc;
    for (int k = 0; k < kKeys / 64; ++k) {
      const int key = kKeys - 1 - (lane * (kKeys / 64) + k);
      start[key] = acc;
      acc += hist[key];
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x) order[atomicAdd(&start[key_of(b)], 1)] = b;
}

// backward-Euler predictor of tacex_fem_step: x_prev = x, x_tilde = x + dt v + dt^2 g (US:250-252: what world.advance() starts from)
__global__ __launch_bounds__(256) void fem_predict_kernel(const double* __restrict__ x, const double* __restrict__ v, double* __restrict__ xt,
                                                          double* __restrict__ xprev, double* __restrict__ dxg, size_t n3, int B,
                                                          double dt, double g0, double g1, double g2, const double* __restrict__ ind,
                                                          const double* __restrict__ ind_prev, double* __restrict__ disp, int have_prev) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B && dxg) dxg[i] = INFINITY;
  if (i < (size_t)B && ind && disp) {  // how far the env's indenter moved since the last step (friction slides relative to it)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      // (a NaN in the env's previous position = "none": tacex_fem_reset_envs marks a reset env so - wherever the caller puts its
      //  indenter before the next step, friction sees no sliding in that step, like the first step of a fresh scene)
      const double d = have_prev ? ind[i * 8 + 1 + k] - ind_prev[i * 3 + k] : 0.0;
      disp[i * 3 + k] = d == d ? d : 0.0;
    }
  }
  if (i >= n3) return;
  const int k = (int)(i % 3);
  const double xi = x[i];
  xprev[i] = xi;
  xt[i] = xi + dt * v[i] + dt * dt * (k == 0 ? g0 : (k == 1 ? g1 : g2));
}
__global__ __launch_bounds__(256) void fem_velocity_kernel(const double* __restrict__ x, const double* __restrict__ xprev,
                                                           double* __restrict__ v, size_t n3, double inv_dt, const double* __restrict__ ind,
                                                           double* __restrict__ ind_prev, int B) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n3) v[i] = (x[i] - xprev[i]) * inv_dt;
  if (i < (size_t)B && ind && ind_prev) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ind_prev[i * 3 + k] = ind[i * 8 + 1 + k];
  }
}

// ------------------------------------------------------------------------------------------------
// Attachment animation (UA:364-428): per step and env, aim = R(q) offset + p for every attached vertex, written straight into
// the constraint arrays the Newton kernels read (`aim_position`, `is_constrained`) - the reference computes it with
// IsaacLab's `transform_points` in float32 on the GPU, copies it to the host and hands it to libuipc's animator callback
// (UA:365-385).  One lane per (env, attachment point); float32 rotation like the reference, widened to float64 on store.
// ------------------------------------------------------------------------------------------------
// per-env reset (tacex_fem_reset_envs): one workgroup per listed env
__global__ __launch_bounds__(256) void fem_reset_envs_kernel(const int* __restrict__ ids, const double* __restrict__ pos, const double* __restrict__ rest,
                                                             double* __restrict__ x, double* __restrict__ v, double* __restrict__ step_info,
                                                             double* __restrict__ ind_prev, int V, int B) {
  const int b = ids ? ids[blockIdx.x] : (int)blockIdx.x;
  if (b < 0 || b >= B) return;
  const size_t o = (size_t)b * V * 3;
  for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) {
    x[o + k] = pos ? pos[(size_t)blockIdx.x * V * 3 + k] : rest[k];
    v[o + k] = 0.0;
  }
  if (threadIdx.x < 4 && step_info) step_info[(size_t)b * 4 + threadIdx.x] = 0.0;
  if (threadIdx.x < 3 && ind_prev) ind_prev[(size_t)b * 3 + threadIdx.x] = __builtin_nan("");
}

__global__ __launch_bounds__(128) void fem_attachment_aim_kernel(const float* __restrict__ body_pos, const float* __restrict__ body_quat,
                                                                 const float* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                                 double* __restrict__ aim, uint8_t* __restrict__ constrained,
                                                                 double* __restrict__ aim_compact, int A, int V) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  const float qw = body_quat[b * 4 + 0], qx = body_quat[b * 4 + 1], qy = body_quat[b * 4 + 2], qz = body_quat[b * 4 + 3];
  // isaaclab.utils.math.matrix_from_quat: two_s = 2 / |q|^2, rows of R
  const float two_s = 2.0f / (qw * qw + qx * qx + qy * qy + qz * qz);
  const float r00 = 1.0f - two_s * (qy * qy + qz * qz), r01 = two_s * (qx * qy - qz * qw), r02 = two_s * (qx * qz + qy * qw);
  const float r10 = two_s * (qx * qy + qz * qw), r11 = 1.0f - two_s * (qx * qx + qz * qz), r12 = two_s * (qy * qz - qx * qw);
  const float r20 = two_s * (qx * qz - qy * qw), r21 = two_s * (qy * qz + qx * qw), r22 = 1.0f - two_s * (qx * qx + qy * qy);
  const float ox = offsets[a * 3 + 0], oy = offsets[a * 3 + 1], oz = offsets[a * 3 + 2];
  const float x = (r00 * ox + r01 * oy + r02 * oz) + body_pos[b * 3 + 0];
  const float y = (r10 * ox + r11 * oy + r12 * oz) + body_pos[b * 3 + 1];
  const float z = (r20 * ox + r21 * oy + r22 * oz) + body_pos[b * 3 + 2];
  const int v = idx[a];
  double* o = aim + ((size_t)b * V + v) * 3;
  o[0] = (double)x; o[1] = (double)y; o[2] = (double)z;
  constrained[(size_t)b * V + v] = 1;
  if (aim_compact) {
    double* c = aim_compact + ((size_t)b * A + a) * 3;
    c[0] = (double)x; c[1] = (double)y; c[2] = (double)z;
  }
}

// ---- K18: FEM-driven markers: barycentric surface point + pinhole projection (VT:347-366) ------------------------
__global__ __launch_bounds__(128) void fem_marker_uv_kernel(const double* __restrict__ pos, const int* __restrict__ tri,
                                                            const double* __restrict__ wgt, double fx, double fy,
                                                            double cx, double cy, double* __restrict__ uv, int Vs, int M) {
  const int mi = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (mi >= M) return;
  const double* p = pos + (size_t)b * Vs * 3;
  double q[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = tri[mi * 3 + k];
    const double w = wgt[mi * 3 + k];
    q[0] += w * p[v * 3 + 0]; q[1] += w * p[v * 3 + 1]; q[2] += w * p[v * 3 + 2];
  }
  uv[((size_t)b * M + mi) * 2 + 0] = fx * q[0] / q[2] + cx;
  uv[((size_t)b * M + mi) * 2 + 1] = fy * q[1] / q[2] + cy;
}

// The whole of gen_marker_flow's per-step part (VT:354-413, the static marker grid of the shipped cfgs) in ONE launch, one workgroup per env:
// surface vertices out of the FEM state -> camera frame (VT:142-187: R_inv (x - cam_pos)) -> barycentric point -> pinhole projection of ALL
// M markers (kept: `curr_marker_uv`), then the step's subset: flow[b, 0, k] = init_uv[b, sel[k]], flow[b, 1, k] = uv[b, sel[k]], optionally
// normalised (VT:407-409: / (W / 2) - 1), as float64 and / or float32 (the plugin's marker_data).  Replaces thirteen launches (index, subtract,
// batched GEMM, contiguous copy, projection, two gathers, stack, normalise, cast; 120 us of C4's 1.27 ms step: profiles/r06_experiments.md 11).
__global__ __launch_bounds__(256) void fem_marker_flow_kernel(const double* __restrict__ xg, const long long* __restrict__ surf_ids,
                                                              const double* __restrict__ cam_pos, const double* __restrict__ cam_rot_inv,
                                                              const int* __restrict__ tri, const double* __restrict__ wgt, double fx, double fy,
                                                              double cx, double cy, const double* __restrict__ init_uv,
                                                              const long long* __restrict__ sel, double norm_div, double* __restrict__ curr_uv,
                                                              double* __restrict__ flow, float* __restrict__ flow32, int V, int M, int K) {
  extern __shared__ double muv[];  // (M,2) this env's projections
  const int b = blockIdx.x;
  const double* x = xg + (size_t)b * V * 3;
  const double* cp = cam_pos + (size_t)b * 3;
  const double* R = cam_rot_inv + (size_t)b * 9;
  for (int mi = threadIdx.x; mi < M; mi += blockDim.x) {
    double q[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long v = surf_ids[tri[mi * 3 + k]];
      const double w = wgt[mi * 3 + k];
      const double d0 = x[v * 3] - cp[0], d1 = x[v * 3 + 1] - cp[1], d2 = x[v * 3 + 2] - cp[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) q[i] += w * (R[i * 3] * d0 + R[i * 3 + 1] * d1 + R[i * 3 + 2] * d2);
    }
    const double u = fx * q[0] / q[2] + cx, vv = fy * q[1] / q[2] + cy;
    muv[mi * 2] = u; muv[mi * 2 + 1] = vv;
    if (curr_uv) { curr_uv[((size_t)b * M + mi) * 2] = u; curr_uv[((size_t)b * M + mi) * 2 + 1] = vv; }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * K; k += blockDim.x) {
    const int which = k / K, kk = k - which * K;  // 0: initial, 1: current
    const long long s = sel[kk];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      double val = which == 0 ? init_uv[((size_t)b * M + s) * 2 + c] : muv[s * 2 + c];
      if (norm_div > 0.0) val = val / norm_div - 1.0;
      const size_t o = (((size_t)b * 2 + which) * K + kk) * 2 + c;
      if (flow) flow[o] = val;
      if (flow32) flow32[o] = (float)val;
    }
  }
}

// gen_marker_flow with the reference's whole randomisation interface (VT:354-413: random grid, lost tracking, noise, random subset) for a
// batch, in ONE launch and with every env on a marker pattern and a random stream of its own.  A library of P marker patterns (grid draws of
// gen_marker_grid + gen_marker_weight, built once on the host) lies on the device; env e follows pattern k = pattern_ids[e] (an id outside
// [0, P) reads pattern 0) and takes draw number t = draws[e].  One workgroup per env:
//   1. every marker m < count[k]: initial (u, v) from the reference surface (fem_marker_uv_kernel's arithmetic) and current (u, v) from the
//      FEM state (fem_marker_flow_kernel's arithmetic);
//   2. in-image mask on the env's OWN initial projection, 5 < u < H and 5 < v < W (sic, VT:382-387);
//   3. lost tracking: m survives iff U > lose_prob;  4. sigma * N added to the four values of a survivor (four independent normals);
//   5. n survivors: n >= K: the survivor whose (key, m) has rank r < K goes to slot r (a uniform K-subset in random order); 0 < n < K: the
//      survivors in marker order, padded with the last; n == 0: zeros;  then / norm_div - 1 if norm_div > 0, the zero case included;
//   6. draws[e] = t + 1.
// Random numbers: Philox4x32-10, key (seed lo, seed hi), counter (m, stream, e, t): stream 0 word 0 -> U, word 1 -> subset key; stream 1
// words (0,1) -> Box-Muller pair for the initial (u, v), words (2,3) -> for the current (u, v).  Nothing depends on B or the launch shape.
// LDS: 40 B per marker - the survivor's four values by marker id, and the compact (marker-ordered) survivor list with its keys.
__global__ __launch_bounds__(256) void fem_marker_flow_library_kernel(
    const double* __restrict__ xg, const long long* __restrict__ surf_ids, const double* __restrict__ cam_pos, const double* __restrict__ cam_rot_inv,
    const double* __restrict__ ref_cam, const int* __restrict__ lib_tri, const double* __restrict__ lib_wgt, const int* __restrict__ lib_count,
    int P, int Mmax, const int* __restrict__ pattern_ids, unsigned int* __restrict__ draws, unsigned int seed_lo, unsigned int seed_hi, double fx,
    double fy, double cx, double cy, double lose_prob, double sigma, double img_h, double img_w, double norm_div, double* __restrict__ curr_uv,
    double* __restrict__ flow, float* __restrict__ flow32, int* __restrict__ num_tracked, int V, int Vs, int K) {
  extern __shared__ double mlib_smem[];
  double* s_val = mlib_smem;                                              // (Mmax,4) init u, init v, current u, current v (noise added)
  unsigned int* s_key = reinterpret_cast<unsigned int*>(s_val + (size_t)Mmax * 4);  // (Mmax) subset key of the p-th survivor
  int* s_list = reinterpret_cast<int*>(s_key + Mmax);                      // (Mmax) marker id of the p-th survivor
  __shared__ int s_cnt[16];                                               // survivors per (pass, wave)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int pat = pattern_ids[b];
  if (pat < 0 || pat >= P) pat = 0;
  int M = lib_count[pat];
  M = M < 0 ? 0 : (M > Mmax ? Mmax : M);
  const int* tri = lib_tri + (size_t)pat * Mmax * 3;
  const double* wgt = lib_wgt + (size_t)pat * Mmax * 3;
  const unsigned int t = draws[b];
  const unsigned int key[2] = {seed_lo, seed_hi};
  const double* x = xg + (size_t)b * V * 3;
  const double* cp = cam_pos + (size_t)b * 3;
  const double* R = cam_rot_inv + (size_t)b * 9;
  const double* p = ref_cam + (size_t)b * Vs * 3;
  bool keep[4];
  unsigned int skey[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int mi = tid + j * 256;
    keep[j] = false;
    skey[j] = 0;
    if (mi < M) {
      int tv[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = tri[mi * 3 + k];
        tv[k] = v < 0 ? 0 : (v >= Vs ? Vs - 1 : v);
      }
      // initial projection: fem_marker_uv_kernel
      double q0[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = tv[k];
        const double w = wgt[mi * 3 + k];
        q0[0] += w * p[v * 3 + 0]; q0[1] += w * p[v * 3 + 1]; q0[2] += w * p[v * 3 + 2];
      }
      double iu = fx * q0[0] / q0[2] + cx, iv = fy * q0[1] / q0[2] + cy;
      // current projection: fem_marker_flow_kernel
      double q[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const long long v = surf_ids[tv[k]];
        const double w = wgt[mi * 3 + k];
        const double d0 = x[v * 3] - cp[0], d1 = x[v * 3 + 1] - cp[1], d2 = x[v * 3 + 2] - cp[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] += w * (R[i * 3] * d0 + R[i * 3 + 1] * d1 + R[i * 3 + 2] * d2);
      }
      double u = fx * q[0] / q[2] + cx, vv = fy * q[1] / q[2] + cy;
      if (curr_uv) { curr_uv[((size_t)b * Mmax + mi) * 2] = u; curr_uv[((size_t)b * Mmax + mi) * 2 + 1] = vv; }
      const unsigned int c0[4] = {(unsigned int)mi, 0u, (unsigned int)b, t};
      unsigned int r0[4];
      philox4x32_10(c0, key, r0);
      keep[j] = iu > 5.0 && iu < img_h && iv > 5.0 && iv < img_w && philox_uniform(r0[0]) > lose_prob;
      skey[j] = r0[1];
      if (keep[j] && sigma > 0.0) {
        const unsigned int c1[4] = {(unsigned int)mi, 1u, (unsigned int)b, t};
        unsigned int r1[4];
        philox4x32_10(c1, key, r1);
        const double kTwoPi = 6.283185307179586;
        const double ra = sqrt(-2.0 * log(philox_uniform(r1[0]))), ta = kTwoPi * philox_uniform(r1[1]);
        const double rb = sqrt(-2.0 * log(philox_uniform(r1[2]))), tb = kTwoPi * philox_uniform(r1[3]);
        const double n0 = ra * cos(ta), n1 = ra * sin(ta), n2 = rb * cos(tb), n3 = rb * sin(tb);
        // (products rounded on their own, then added: what the NumPy restatement computes)
        iu = __dadd_rn(iu, __dmul_rn(sigma, n0)); iv = __dadd_rn(iv, __dmul_rn(sigma, n1));
        u = __dadd_rn(u, __dmul_rn(sigma, n2)); vv = __dadd_rn(vv, __dmul_rn(sigma, n3));
      }
      s_val[mi * 4] = iu; s_val[mi * 4 + 1] = iv; s_val[mi * 4 + 2] = u; s_val[mi * 4 + 3] = vv;
    } else if (mi < Mmax && curr_uv) {
      curr_uv[((size_t)b * Mmax + mi) * 2] = 0.0; curr_uv[((size_t)b * Mmax + mi) * 2 + 1] = 0.0;
    }
  }
  // survivor compaction in marker order: a workgroup prefix sum over (pass, wave) ballots
  unsigned long long bal[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bal[j] = __ballot(keep[j]);
    if (lane == 0) s_cnt[j * 4 + wave] = __popcll(bal[j]);
  }
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) n += s_cnt[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (keep[j]) {
      int pos = __popcll(bal[j] & ((1ull << lane) - 1ull));
      for (int i = 0; i < j * 4 + wave; ++i) pos += s_cnt[i];
      s_list[pos] = tid + j * 256;
      s_key[pos] = skey[j];
    }
  }
  __syncthreads();
  if (tid == 0) {
    draws[b] = t + 1u;
    if (num_tracked) num_tracked[b] = n;
  }
  double* fl = flow ? flow + (size_t)b * 4 * K : nullptr;
  float* fl32 = flow32 ? flow32 + (size_t)b * 4 * K : nullptr;
  auto put = [&](int slot, const double* v4) {  // v4: init u, init v, current u, current v; nullptr: zeros
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double val = v4 ? v4[c] : 0.0;
      if (norm_div > 0.0) val = val / norm_div - 1.0;
      const size_t o = ((size_t)(c >> 1) * K + slot) * 2 + (c & 1);
      if (fl) fl[o] = val;
      if (fl32) fl32[o] = (float)val;
    }
  };
  if (n >= K) {
    for (int ps = tid; ps < n; ps += 256) {
      const unsigned int kp = s_key[ps];
      int r = 0;
      for (int qs = 0; qs < n; ++qs) {
        const unsigned int kq = s_key[qs];
        r += (kq < kp || (kq == kp && qs < ps)) ? 1 : 0;  // (survivors are listed in marker order: qs < ps is m_q < m_p)
      }
      if (r < K) put(r, s_val + (size_t)s_list[ps] * 4);
    }
  } else if (n > 0) {
    const double* last = s_val + (size_t)s_list[n - 1] * 4;
    for (int s = tid; s < K; s += 256) put(s, s < n ? s_val + (size_t)s_list[s] * 4 : last);
  } else {
    for (int s = tid; s < K; s += 256) put(s, nullptr);
  }
}

}  // namespace tacex
