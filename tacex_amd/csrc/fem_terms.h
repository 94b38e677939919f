// FEM device layer: element terms (K17a), the energy and gradient kernels and the per-env pieces the streaming kernels share.
#pragma once
#include "fem_device.h"

namespace tacex {

// cyclic Jacobi eigen-decomposition of a symmetric 9x9 (PSD-projection path only; arrays live in scratch)
// (forced inline: with ONE caller the compiler inlined it by itself; the element kernel now has two PSD instantiations, and called
// out of line the 12 x 12 block of the caller went to scratch as well - 1860 against 384 B/lane)
__device__ __forceinline__ void jacobi_psd9(double* A) {
  double V[81];
  for (int i = 0; i < 81; ++i) V[i] = (i / 9 == i % 9) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int p = 0; p < 9; ++p) {
      dia += A[p * 9 + p] * A[p * 9 + p];
      for (int q = p + 1; q < 9; ++q) off += A[p * 9 + q] * A[p * 9 + q];
    }
    if (off <= 1e-30 * (dia + 1e-300)) break;
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double apq = A[p * 9 + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (A[q * 9 + q] - A[p * 9 + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < 9; ++k) {
          const double akp = A[k * 9 + p], akq = A[k * 9 + q];
          A[k * 9 + p] = cs * akp - sn * akq;
          A[k * 9 + q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 9; ++k) {
          const double apk = A[p * 9 + k], aqk = A[q * 9 + k];
          A[p * 9 + k] = cs * apk - sn * aqk;
          A[q * 9 + k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < 9; ++k) {
          const double vkp = V[k * 9 + p], vkq = V[k * 9 + q];
          V[k * 9 + p] = cs * vkp - sn * vkq;
          V[k * 9 + q] = sn * vkp + cs * vkq;
        }
      }
  }
  double w[9];
  for (int i = 0; i < 9; ++i) w[i] = A[i * 9 + i] > 0.0 ? A[i * 9 + i] : 0.0;
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) {
      double sacc = 0.0;
      for (int k = 0; k < 9; ++k) sacc += V[i * 9 + k] * w[k] * V[j * 9 + k];
      A[i * 9 + j] = sacc;
    }
}

// ---- K17a: element terms, one tet per lane, SoA outputs ---------------------------------------------------
template <bool PROJECT_PSD, bool MAT>
__global__ __launch_bounds__(256) void fem_element_terms_kernel(FemDev m, const double* __restrict__ x,
                                                                double* __restrict__ energy, double* __restrict__ grad,
                                                                double* __restrict__ hess, FemMat mat) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= m.T) return;
  (void)env_material<MAT>(m, mat, b);  // (a bad id is reported by the step kernels)
  int v[4];
  double Di[9], F[9], r[12];
  load_tet(m, t, v, Di);
  deformation_gradient(x + (size_t)b * m.V * 3, v, Di, F);
  TetState s;
  tet_state(m, F, s);
  shape_rows(Di, r);
  const double vol = m.vol[t];
  const size_t T = m.T;
  if (energy) energy[(size_t)b * T + t] = vol * psi_of(m, s);
  if (grad) {
    double g[12];
    element_gradient(s, r, vol, g);
#pragma unroll
    for (int k = 0; k < 12; ++k) grad[((size_t)b * 12 + k) * T + t] = g[k];
  }
  if (!hess) return;
  if constexpr (!PROJECT_PSD) {
    // column j = (vertex u, component k): dF = e_k (x) r_u ; H[:, j] = vol * (dP : dF_i)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double dF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dP[9];
        dF[k * 3 + 0] = r[u * 3 + 0]; dF[k * 3 + 1] = r[u * 3 + 1]; dF[k * 3 + 2] = r[u * 3 + 2];
        apply_dP(m, s, dF, dP);
        const int j = u * 3 + k;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const double h = vol * (dP[i * 3 + 0] * r[w * 3 + 0] + dP[i * 3 + 1] * r[w * 3 + 1] + dP[i * 3 + 2] * r[w * 3 + 2]);
            hess[((size_t)b * 144 + (w * 3 + i) * 12 + j) * T + t] = h;
          }
      }
    return;
  } else {
  // PSD projection of the 9x9 F-space Hessian (row-major vec(F) index q = i*3 + m), then H12 = vol G^T H9+ G
  double H9[81];
  for (int q = 0; q < 9; ++q) {
    double dF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dP[9];
    dF[q] = 1.0;
    apply_dP(m, s, dF, dP);
    for (int p = 0; p < 9; ++p) H9[p * 9 + q] = dP[p];
  }
  for (int p = 0; p < 9; ++p)
    for (int q = p + 1; q < 9; ++q) { const double a = 0.5 * (H9[p * 9 + q] + H9[q * 9 + p]); H9[p * 9 + q] = a; H9[q * 9 + p] = a; }
  jacobi_psd9(H9);
  for (int u = 0; u < 4; ++u)
    for (int k = 0; k < 3; ++k) {
      double dP[9];  // H9 * vec(dF_j), dF_j = e_k (x) r_u
      for (int p = 0; p < 9; ++p)
        dP[p] = H9[p * 9 + k * 3 + 0] * r[u * 3 + 0] + H9[p * 9 + k * 3 + 1] * r[u * 3 + 1] + H9[p * 9 + k * 3 + 2] * r[u * 3 + 2];
      const int j = u * 3 + k;
      for (int w = 0; w < 4; ++w)
        for (int i = 0; i < 3; ++i) {
          const double h = vol * (dP[i * 3 + 0] * r[w * 3 + 0] + dP[i * 3 + 1] * r[w * 3 + 1] + dP[i * 3 + 2] * r[w * 3 + 2]);
          hess[((size_t)b * 144 + (w * 3 + i) * 12 + j) * T + t] = h;
        }
    }
  }
}

__device__ double env_energy(const FemDev& m, const double* x, const double* xt, const uint8_t* cons, const double* aim,
                             double* sh, const IndMesh& im, const double* ind = nullptr, const double* fl = nullptr, const double* xn = nullptr,
                             const double* disp = nullptr) {
  double e = 0.0;
  for (int t = threadIdx.x; t < m.T; t += blockDim.x) {
    int v[4];
    double Di[9], F[9];
    load_tet(m, t, v, Di);
    deformation_gradient(x, v, Di, F);
    TetState s;
    tet_state(m, F, s);
    e += m.dt * m.dt * m.vol[t] * psi_of(m, s);
  }
  for (int v = threadIdx.x; v < m.V; v += blockDim.x) {
    const double mv = m.mass[v];
    double q = 0.0, qc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double d = x[v * 3 + i] - xt[v * 3 + i];
      q += d * d;
      if (cons && cons[v]) { const double c = x[v * 3 + i] - aim[v * 3 + i]; qc += c * c; }
    }
    e += 0.5 * mv * q + 0.5 * m.strength * mv * qc;
    if (ind && m.area) e += m.dt * m.dt * contact_eval(m, im, ind, m.area[v], x + v * 3).e;
    if (fl) e += m.dt * m.dt * friction_eval(m.fric_mu, m.fric_eps, fl + (size_t)v * 4, x + v * 3, xn + v * 3, disp, false).e;
  }
  return block_sum(e, sh);
}

// per-tet gradients (scaled by dt^2) into ge (12,T) of this env
__device__ void env_tet_gradients(const FemDev& m, const double* x, double* ge) {
  for (int t = threadIdx.x; t < m.T; t += blockDim.x) {
    int v[4];
    double Di[9], F[9], r[12], g[12];
    load_tet(m, t, v, Di);
    deformation_gradient(x, v, Di, F);
    TetState s;
    tet_state(m, F, s);
    shape_rows(Di, r);
    element_gradient(s, r, m.dt * m.dt * m.vol[t], g);
#pragma unroll
    for (int k = 0; k < 12; ++k) ge[(size_t)k * m.T + t] = g[k];
  }
}

// atomics-free nodal assembly: vertex v sums its incident tets' local rows
__device__ __forceinline__ void gather_vertex(const FemDev& m, const double* ge, int v, double out[3]) {
  out[0] = out[1] = out[2] = 0.0;
  for (int e = m.vt_off[v]; e < m.vt_off[v + 1]; ++e) {
    const int code = m.vt_idx[e];
    const int t = code >> 2, l = code & 3;
    out[0] += ge[(size_t)(l * 3 + 0) * m.T + t];
    out[1] += ge[(size_t)(l * 3 + 1) * m.T + t];
    out[2] += ge[(size_t)(l * 3 + 2) * m.T + t];
  }
}

template <bool MAT>
__global__ __launch_bounds__(512) void fem_energy_kernel(FemDev m, const double* x, const double* xt,
                                                         const uint8_t* cons, const double* aim, double* E, FemMat mat) {
  __shared__ double sh[17];
  const int b = blockIdx.x;
  (void)env_material<MAT>(m, mat, b);  // (a bad id is reported by the step kernels)
  const size_t o = (size_t)b * m.V * 3;
  const double* ind = m.indenters ? m.indenters + (size_t)b * 8 : nullptr;
  bool bad;
  const IndMesh im = env_mesh<true>(m, b, ind, bad);
  const double e = env_energy(m, x + o, xt + o, cons ? cons + (size_t)b * m.V : nullptr, aim ? aim + o : nullptr, sh, im, ind);
  if (threadIdx.x == 0) E[b] = e;
}

template <bool MAT>
__global__ __launch_bounds__(512) void fem_gradient_kernel(FemDev m, const double* x, const double* xt,
                                                           const uint8_t* cons, const double* aim, double* g,
                                                           double* ws_ge /* (B,12,T) */, FemMat mat) {
  const int b = blockIdx.x;
  (void)env_material<MAT>(m, mat, b);  // (a bad id is reported by the step kernels)
  const size_t o = (size_t)b * m.V * 3;
  double* ge = ws_ge + (size_t)b * 12 * m.T;
  bool bad;
  const IndMesh im = env_mesh<true>(m, b, m.indenters ? m.indenters + (size_t)b * 8 : nullptr, bad);
  env_tet_gradients(m, x + o, ge);
  __syncthreads();
  for (int v = threadIdx.x; v < m.V; v += blockDim.x) {
    double a[3];
    gather_vertex(m, ge, v, a);
    const double mv = m.mass[v];
    const bool c = cons && cons[(size_t)b * m.V + v];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double gi = a[i] + mv * (x[o + v * 3 + i] - xt[o + v * 3 + i]);
      if (c) gi += m.strength * mv * (x[o + v * 3 + i] - aim[o + v * 3 + i]);
      g[o + v * 3 + i] = gi;
    }
    if (m.indenters && m.area) {
      const ContactEval ce = contact_eval(m, im, m.indenters + (size_t)b * 8, m.area[v], x + o + v * 3);
      if (ce.active)
#pragma unroll
        for (int i = 0; i < 3; ++i) g[o + v * 3 + i] += m.dt * m.dt * ce.b1 * ce.n[i];
    }
  }
}

}  // namespace tacex
