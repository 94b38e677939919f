// FEM device layer: the elastic preconditioner blocks of every env, assembled ahead of the CU-resident Newton launch.
#pragma once
#include "fem_device.h"

namespace tacex {

// ---- elastic preconditioner blocks of every env, ahead of the Newton launch (round 5) ------------------------------------------
// Per vertex the 3x3 diagonal block D (upper triangle, 6) of dt^2 K at the state the launch starts from and the block E (9) towards
// its chain successor (tacex_fem_set_chains): (V,16) doubles per env in the workspace, read by fem_newton_lds_kernel in every
// Newton iteration of the launch (the blocks that change by orders of magnitude between iterations - barrier curvature, friction -
// are added there, fresh).  One workgroup per env, x and the (V,15) accumulators in LDS (71 KB at 495 vertices: two envs per CU, a
// 512-env shard in one round); rounds 3-4 ran this inside the first Newton iteration of fem_newton_lds_kernel.
//   ATOM:  tet-centric - every tet's state is computed once, its shares of the four diagonal blocks and of the chain blocks are
//          added with ds_add_f64 (summation order depends on wave timing: round-off level run-to-run differences);
//   !ATOM: vertex-centric over the incidence list in a FIXED order (tacex_fem_set_deterministic) - the tet state is recomputed per
//          incident vertex, four times the arithmetic, bit-identical runs.
// dxg / dx_tol: envs that converged in an earlier launch of the time step are skipped (same protocol as the Newton kernels).
// Blocks of the element Hessian in closed form.  With dF = e_k (x) r_B (row k of dF = r_B) contracted against r_A, the 9x9 Hessian
// of the Stable Neo-Hookean density (apply_dP: a dF + b (F:dF) F + lam (C:dF) C + c dC[dF]) gives the 3x3 block
//     B(A, B)[i][k] = a (r_A . r_B) delta_ik + b u_A[i] u_B[k] + lam w_A[i] w_B[k] + c eps_ikn g[n],
//     u = F r,  w = C r (C = cofactor matrix),  g = F (r_A x r_B)
// (the last term is d2J/dF2 = eps eps F contracted with r_A, r_B: antisymmetric, zero for A = B).  A diagonal block costs two
// matrix-vector products and six entries of three FMAs instead of three apply_dP calls (~100 f64 operations each) and their
// contractions: the assembly kernel went from 70 to 43 us per 512 envs (profiles/r05_experiments.md section 8); verified against the
// oracle's dpk1 to 1e-16 relative.
struct TetBlocks {
  double u[4][3], w[4][3], n2[4];
};
__device__ __forceinline__ void tet_blocks(const TetState& s, const double r[12], TetBlocks& tb) {
#pragma unroll
  for (int l = 0; l < 4; ++l) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      tb.u[l][i] = s.F[i * 3 + 0] * r[l * 3 + 0] + s.F[i * 3 + 1] * r[l * 3 + 1] + s.F[i * 3 + 2] * r[l * 3 + 2];
      tb.w[l][i] = s.C[i * 3 + 0] * r[l * 3 + 0] + s.C[i * 3 + 1] * r[l * 3 + 1] + s.C[i * 3 + 2] * r[l * 3 + 2];
    }
    tb.n2[l] = r[l * 3 + 0] * r[l * 3 + 0] + r[l * 3 + 1] * r[l * 3 + 1] + r[l * 3 + 2] * r[l * 3 + 2];
  }
}
// Row `l2` of a 4-row table with a RUNTIME l2 as an exact blend (weights 1.0 / 0.0) of constant-indexed reads: a runtime index sends
// the array to scratch, and a chain of selects is folded back into one by the optimiser (select of loads -> load of a selected address).
#define TB_SEL(arr, l2, i) (((l2) == 0 ? 1.0 : 0.0) * arr[0][i] + ((l2) == 1 ? 1.0 : 0.0) * arr[1][i] + ((l2) == 2 ? 1.0 : 0.0) * arr[2][i] + \
                            ((l2) == 3 ? 1.0 : 0.0) * arr[3][i])
#define R_SEL(r, l2, j) (((l2) == 0 ? 1.0 : 0.0) * r[j] + ((l2) == 1 ? 1.0 : 0.0) * r[3 + (j)] + ((l2) == 2 ? 1.0 : 0.0) * r[6 + (j)] + \
                         ((l2) == 3 ? 1.0 : 0.0) * r[9 + (j)])
// the off-diagonal block (vertex l, vertex l2) of the tet: E[i * 3 + k]
__device__ __forceinline__ void tet_block_offdiag(const FemDev& m, const TetState& s, const double r[12], const TetBlocks& tb, const double (&ul)[3],
                                                   const double (&wl)[3], const double (&rl)[3], int l2, double E[9]) {
  const double u2[3] = {TB_SEL(tb.u, l2, 0), TB_SEL(tb.u, l2, 1), TB_SEL(tb.u, l2, 2)};
  const double w2[3] = {TB_SEL(tb.w, l2, 0), TB_SEL(tb.w, l2, 1), TB_SEL(tb.w, l2, 2)};
  const double r2[3] = {R_SEL(r, l2, 0), R_SEL(r, l2, 1), R_SEL(r, l2, 2)};
  const double dot = rl[0] * r2[0] + rl[1] * r2[1] + rl[2] * r2[2];
  const double x3[3] = {rl[1] * r2[2] - rl[2] * r2[1], rl[2] * r2[0] - rl[0] * r2[2], rl[0] * r2[1] - rl[1] * r2[0]};
  double g[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) g[n] = s.c * (s.F[n * 3 + 0] * x3[0] + s.F[n * 3 + 1] * x3[1] + s.F[n * 3 + 2] * x3[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) E[i * 3 + k] = s.b * ul[i] * u2[k] + m.lam * wl[i] * w2[k];
  const double ad = s.a * dot;
  E[0] += ad; E[4] += ad; E[8] += ad;
  E[1] += g[2]; E[2] -= g[1]; E[3] -= g[2]; E[5] += g[0]; E[6] += g[1]; E[7] -= g[0];
}

template <bool ATOM, bool MAT>
__global__ __launch_bounds__(512) void fem_assemble_blocks_kernel(FemDev m, const double* __restrict__ xg, double* __restrict__ lagg,
                                                                   const double* __restrict__ dxg, double dx_tol, FemMat mat) {
  extern __shared__ __attribute__((aligned(16))) double alds[];
  constexpr int NT = 512;
  const int V = m.V, T = m.T, b = blockIdx.x, tid = threadIdx.x;
  if (dxg && dxg[b] <= dx_tol) return;
  (void)env_material<MAT>(m, mat, b);  // (a bad id is reported by the step kernels)
  double* xs = alds;           // (V,3)
  double* xa = xs + 3 * V;     // (V,15) accumulators (ATOM)
  const double* x = xg + (size_t)b * V * 3;
  double* lagw = lagg + (size_t)b * 16 * V;  // (V,16): D upper triangle (6) | E (9) | pad, one 128-byte record per vertex
  for (int k = tid; k < 3 * V; k += NT) xs[k] = x[k];
  if constexpr (ATOM)
    for (int k = tid; k < 15 * V; k += NT) xa[k] = 0.0;
  __syncthreads();
  const double dt2 = m.dt * m.dt;
  if constexpr (ATOM) {
    for (int t = tid; t < T; t += NT) {
      int v[4];
      double Di[9], F[9], r[12], vol_t;
      load_tet_blk(m, t, v, Di, vol_t);
      deformation_gradient(xs, v, Di, F);
      TetState s;
      tet_state(m, F, s);
      shape_rows(Di, r);
      TetBlocks tb;
      tet_blocks(s, r, tb);
      const double sc = dt2 * vol_t;
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        double* q = xa + v[l] * 15;
        const double ul[3] = {tb.u[l][0], tb.u[l][1], tb.u[l][2]}, wl[3] = {tb.w[l][0], tb.w[l][1], tb.w[l][2]};
        const double an = s.a * tb.n2[l];
        // upper triangle: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> q[0..5]
        atomicAdd(&q[0], sc * (an + s.b * ul[0] * ul[0] + m.lam * wl[0] * wl[0]));
        atomicAdd(&q[1], sc * (s.b * ul[0] * ul[1] + m.lam * wl[0] * wl[1]));
        atomicAdd(&q[2], sc * (s.b * ul[0] * ul[2] + m.lam * wl[0] * wl[2]));
        atomicAdd(&q[3], sc * (an + s.b * ul[1] * ul[1] + m.lam * wl[1] * wl[1]));
        atomicAdd(&q[4], sc * (s.b * ul[1] * ul[2] + m.lam * wl[1] * wl[2]));
        atomicAdd(&q[5], sc * (an + s.b * ul[2] * ul[2] + m.lam * wl[2] * wl[2]));
        const int nv = m.ch_next ? m.ch_next[v[l]] : -1;
        const int l2 = nv < 0 ? -1 : (v[0] == nv ? 0 : (v[1] == nv ? 1 : (v[2] == nv ? 2 : (v[3] == nv ? 3 : -1))));
        if (l2 >= 0) {  // this tet also holds the chain successor of vertex l: its share of the block (v_l, next(v_l))
          const double rl[3] = {r[l * 3 + 0], r[l * 3 + 1], r[l * 3 + 2]};
          double E[9];
          tet_block_offdiag(m, s, r, tb, ul, wl, rl, l2, E);
#pragma unroll
          for (int k = 0; k < 9; ++k) atomicAdd(&q[6 + k], sc * E[k]);
        }
      }
    }
    __syncthreads();
    for (int k = tid; k < 16 * V; k += NT) {  // (V,15) -> (V,16): coalesced stores
      const int vv = k >> 4, j = k & 15;
      lagw[k] = j < 15 ? xa[vv * 15 + j] : 0.0;
    }
  } else {
    for (int vtx = tid; vtx < V; vtx += NT) {
      double D[6] = {0, 0, 0, 0, 0, 0};
      double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      const int nv = m.ch_next ? m.ch_next[vtx] : -1;
      for (int e = m.vt_off[vtx], e_end = m.vt_off[vtx + 1]; e < e_end; ++e) {
        const int code = m.vt_idx[e];
        const int t = code >> 2, l = code & 3;
        int v[4];
        double Di[9], F[9], r[12], vol_t;
        load_tet_rec(m, t, v, Di, vol_t);  // (vertex order: every lane another tet - the AoS record, not 14 scattered SoA loads)
        deformation_gradient(xs, v, Di, F);
        TetState s;
        tet_state(m, F, s);
        shape_rows(Di, r);
        const double sc = dt2 * vol_t;
        const double rl[3] = {R_SEL(r, l, 0), R_SEL(r, l, 1), R_SEL(r, l, 2)};
        double ul[3], wl[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          ul[i] = s.F[i * 3 + 0] * rl[0] + s.F[i * 3 + 1] * rl[1] + s.F[i * 3 + 2] * rl[2];
          wl[i] = s.C[i * 3 + 0] * rl[0] + s.C[i * 3 + 1] * rl[1] + s.C[i * 3 + 2] * rl[2];
        }
        const double an = s.a * (rl[0] * rl[0] + rl[1] * rl[1] + rl[2] * rl[2]);
        D[0] += sc * (an + s.b * ul[0] * ul[0] + m.lam * wl[0] * wl[0]);
        D[1] += sc * (s.b * ul[0] * ul[1] + m.lam * wl[0] * wl[1]);
        D[2] += sc * (s.b * ul[0] * ul[2] + m.lam * wl[0] * wl[2]);
        D[3] += sc * (an + s.b * ul[1] * ul[1] + m.lam * wl[1] * wl[1]);
        D[4] += sc * (s.b * ul[1] * ul[2] + m.lam * wl[1] * wl[2]);
        D[5] += sc * (an + s.b * ul[2] * ul[2] + m.lam * wl[2] * wl[2]);
        const int l2 = nv < 0 ? -1 : (v[0] == nv ? 0 : (v[1] == nv ? 1 : (v[2] == nv ? 2 : (v[3] == nv ? 3 : -1))));
        if (l2 >= 0) {  // this tet also holds the chain successor: its share of the block (v, next)
          TetBlocks tb;
          tet_blocks(s, r, tb);
          double Et[9];
          tet_block_offdiag(m, s, r, tb, ul, wl, rl, l2, Et);
#pragma unroll
          for (int k = 0; k < 9; ++k) E[k] += sc * Et[k];
        }
      }
      double* q = lagw + (size_t)vtx * 16;
#pragma unroll
      for (int k = 0; k < 6; ++k) q[k] = D[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) q[6 + k] = E[k];
      q[15] = 0.0;
    }
  }
}

}  // namespace tacex
