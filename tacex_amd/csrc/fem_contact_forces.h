// FEM device layer: the contact forces of the gelpad at a state and their net wrench per env (tacex_fem_contact_forces).
//
// What the step solves and then drops: how hard the indenter presses, where, and how much of it is shear.  Per surface vertex the
// terms are the solver's own - contact_eval (barrier), friction_lag_ipc + friction_eval (IPC's lagged friction) - evaluated once more
// at the given state; nothing of the math is restated here.  Forces act ON THE PAD, in newtons (the energy terms' gradients are
// dt^2-scaled, b1 and the friction gradient are not); the force on the indenter is the negative.
#pragma once
#include "fem_device.h"

namespace tacex {

// The record of one env, (B,16) f64:
//   0..2 sum f_n | 3..5 sum f_f | 6..8 torque sum (x_v - ref) x (f_n + f_f) | 9 sum lam_v | 10 contact area | 11 active vertices |
//   12..14 centre of pressure sum lam_v x_v / sum lam_v (ref where sum lam = 0) | 15 smallest gap over the surface vertices (+inf: none)
constexpr int kWrenchSlots = 16;
constexpr int kWrenchSums = 15;  // partial sums of a thread: slots 0..11, then sum lam_v (x_v - ref) in 12..14

// One workgroup per env, 256 threads, vertices strided over the threads like fem_contact_gaps_kernel.  Fixed-order reduction, no float
// atomics: the partial sums of a thread run over its vertices in ascending order, a wave adds its 64 lanes by a butterfly of lane
// exchanges (every lane ends with the same bits: a + b = b + a), and one thread per slot adds the four waves in wave order through LDS.
// Nothing of another env is read: an env's record does not depend on the batch it shares.
// xprev / disp / ind_prev: the step's start positions (B,V,3), the indenter displacement of that step (B,3) and the indenter position
// that step ended with (B,3), all in the step workspace (StepLayout); nullptr = no friction.  A NaN in the env's ind_prev row =
// its friction reference was cleared (tacex_fem_reset_envs) and it has not stepped since: no friction.  (A reset clears the friction
// reference only: the normal part is whatever the barrier gives at the reset state against the indenter where the caller has it.)
__global__ __launch_bounds__(256) void fem_contact_forces_kernel(FemDev m, const double* __restrict__ xg, const double* __restrict__ xprev,
                                                                 const double* __restrict__ disp, const double* __restrict__ ind_prev,
                                                                 const double* __restrict__ refp, double* __restrict__ wrench,
                                                                 double* __restrict__ vforce, FemMat mat) {
  __shared__ double sh[4][kWrenchSums + 1];
  const int b = blockIdx.x;
  env_material<true>(m, mat, b);  // (the env's own friction ratio; a bad id reads material 0, as in the step)
  const double* ind = m.indenters ? m.indenters + (size_t)b * 8 : nullptr;
  bool bad;
  const IndMesh im = env_mesh<true>(m, b, ind, bad);
  double ref[3] = {0.0, 0.0, 0.0};
  if (refp) { ref[0] = uniform_f64(refp[(size_t)b * 3]); ref[1] = uniform_f64(refp[(size_t)b * 3 + 1]); ref[2] = uniform_f64(refp[(size_t)b * 3 + 2]); }
  bool fric = ind && xprev && disp && ind_prev && m.fric_mu > 0.0;
  // The indenter row the lag is taken against: kind, radius and axis of the env's row, the POSITION the last step ended with (ind_prev
  // of the workspace; friction_lag_ipc moves it back by disp to where the step started) - not the row's own, which the caller may have
  // moved since that step: the friction part is a function of what the step stored.
  double indl[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double dsp[3] = {0.0, 0.0, 0.0};
  if (fric) {
#pragma unroll
    for (int k = 0; k < 8; ++k) indl[k] = uniform_f64(ind[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double ip = uniform_f64(ind_prev[(size_t)b * 3 + k]);
      if (ip != ip) fric = false;
      indl[1 + k] = ip;
      dsp[k] = uniform_f64(disp[(size_t)b * 3 + k]);
    }
  }
  double acc[kWrenchSums];
#pragma unroll
  for (int k = 0; k < kWrenchSums; ++k) acc[k] = 0.0;
  double gmin = INFINITY;
  for (int v = threadIdx.x; v < m.V; v += blockDim.x) {
    const size_t o = ((size_t)b * m.V + v) * 3;
    const double x3[3] = {xg[o], xg[o + 1], xg[o + 2]};
    const double w = m.area ? m.area[v] : 0.0;
    double fn[3] = {0.0, 0.0, 0.0}, ff[3] = {0.0, 0.0, 0.0};
    const ContactEval c = contact_eval<true>(m, im, ind, w, x3);  // (w = 0, an interior vertex: nothing is evaluated)
    if (c.d < 1e299) gmin = fmin(gmin, c.d);
    if (!c.penetrating) {  // a vertex at or beyond the surface contributes nothing (it shows in the smallest gap)
      if (c.active) {
        const double lam = -c.b1;
#pragma unroll
        for (int k = 0; k < 3; ++k) fn[k] = lam * c.n[k];
        acc[9] += lam; acc[10] += w; acc[11] += 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[12 + k] += lam * (x3[k] - ref[k]);
      }
      if (fric && w > 0.0) {
        const double xn3[3] = {xprev[o], xprev[o + 1], xprev[o + 2]};
        double fv[4];
        fv[0] = friction_lag_ipc<true>(m, im, indl, w, dsp, xn3, fv + 1);
        const FricEval f = friction_eval(m.fric_mu, m.fric_eps, fv, x3, xn3, dsp, false);
#pragma unroll
        for (int k = 0; k < 3; ++k) ff[k] = -f.g[k];
      }
    }
    const double ft[3] = {fn[0] + ff[0], fn[1] + ff[1], fn[2] + ff[2]};
    const double r[3] = {x3[0] - ref[0], x3[1] - ref[1], x3[2] - ref[2]};
    double tq[3];
    cross3(r, ft, tq);
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc[k] += fn[k]; acc[3 + k] += ff[k]; acc[6 + k] += tq[k]; }
    if (vforce) { vforce[o] = ft[0]; vforce[o + 1] = ft[1]; vforce[o + 2] = ft[2]; }
  }
#pragma unroll
  for (int k = 0; k < kWrenchSums; ++k)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc[k] += __shfl_xor(acc[k], s, 64);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) gmin = fmin(gmin, __shfl_xor(gmin, s, 64));
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kWrenchSums; ++k) sh[wid][k] = acc[k];
    sh[wid][kWrenchSums] = gmin;
  }
  __syncthreads();
  if (threadIdx.x < kWrenchSlots) {
    const int k = threadIdx.x;
    double out;
    if (k == 15) {
      out = fmin(fmin(sh[0][15], sh[1][15]), fmin(sh[2][15], sh[3][15]));
    } else {
      out = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
      if (k >= 12) {
        const double sl = ((sh[0][9] + sh[1][9]) + sh[2][9]) + sh[3][9];
        const double rk = k == 12 ? ref[0] : (k == 13 ? ref[1] : ref[2]);
        out = sl > 0.0 ? rk + out / sl : rk;
      }
    }
    wrench[(size_t)b * kWrenchSlots + k] = out;
  }
}

}  // namespace tacex
