// FEM device layer: the contact forces of the ball scene (gelpad + one affine body + ground, fem_ball.h) at a state and their wrenches per
// env (tacex_fem_ball_contact_forces).
//
// What fem_ball_newton_kernel balances and then drops: the force the pad puts on the body, what the ground returns, the shear the pad
// feels.  Every term is the step's own - the pairs, the cull, the friction law and the normal force are the functions of
// fem_ball_pairs.h that the step calls; the ground barrier of both bodies and IPC's lagged friction of all of them are applied here -
// evaluated once at (x, q) and reduced per env.  A contact force on a state row is -(1 / dt^2) d/d row of the term's share of the
// incremental potential, in newtons: what oracle/abd_oracle.py BallScene.gradient adds for these terms, divided by -dt^2.
#pragma once
#include "fem_ball_pairs.h"

namespace tacex {

// The record of one env, (B,44) f64, world frame, forces ON the body named first:
//   0..2 pad <- body: sum of the barrier forces on the pad rows (mollifier term included) | 3..5 pad <- body: sum of the pair contacts'
//   friction on the pad rows | 6..8 torque of 0..5 on the pad, sum (x_row - ref) x f_row | 9 sum lam over the active pairs | 10 active
//   pairs | 11 flags (0, kBallFlagOverflow) | 12..14 centre of pressure sum lam_k c_k / sum lam_k, c_k the pad-side closest point (ref
//   where sum lam = 0) | 15 smallest distance of an active pair (+inf: none) | 16..18 active pairs of kind 0 / 1 / 2 | 19 0 |
//   20..31 body: generalised contact force on its rows (p, c_1, c_2, c_3): pairs + their friction + ground + ground friction |
//   32..34 body <- ground: friction (x, y) and normal (z) | 35 / 36 / 37 sum lam, count and smallest gap of the body's ground contacts |
//   38..40 pad <- ground | 41 / 42 count and smallest gap of the pad's ground contacts (+inf: none) | 43 0
constexpr int kBallForceSlots = 44;

// One workgroup per env, 256 threads, one launch.  Pass 0 stands at (x, q): barrier forces of the pairs and of the ground.  Pass 1 (friction)
// stands at the state the last step started from, (x_prev, q_lag): every active pair and ground contact THERE is a lagged contact (lam, n and
// the coefficients frozen, what take_lag stores in fem_ball_newton_kernel), its friction force at (x, q) follows at once from the sliding
// since then - no record is kept.  The pad rows slide from x_prev, the body rows by q - q_ref (q_ref: q_lag for a free body, the pose
// the step measured the body's motion from for a kinematic one; null: not at all).  A NaN in the env's q_lag row: its friction reference was cleared (tacex_fem_ball_reset_envs), no friction.
// Both passes cull with the step's ball_cull, at reach d_hat (no CCD here) and with the ball triangles tested by their corners' bounding
// box (the step has their spheres at hand); lists in LDS, capacity kBallMaxCand, an overflow sets kBallFlagOverflow in slot 11.  Slots are
// handed out with LDS atomics (the order of the candidates, and with it the order of a thread's partial sums, varies between runs):
// results agree to round-off, not bit for bit.
// Reduction: per-thread partial sums, a wave butterfly, the four waves added in wave order through LDS.  The optional per-vertex forces
// accumulate in LDS (f64 atomic adds) and are written once.
// dynamic LDS: ball surface points (nv,3) | per-vertex forces (V,3) when vforce is given (ball_force_lds_bytes)
__host__ __device__ inline size_t ball_force_lds_bytes(int V, int nv, bool vertex_forces) {
  return ((size_t)3 * nv + (vertex_forces ? (size_t)3 * V : 0)) * sizeof(double);
}

__global__ __launch_bounds__(256) void fem_ball_contact_forces_kernel(BallDev bd, int V, double fric_mu, double fric_eps, const double* __restrict__ xg,
                                                                      const double* __restrict__ qg, const double* __restrict__ xprevg,
                                                                      const double* __restrict__ qlagg, const double* __restrict__ qrefg,
                                                                      const double* __restrict__ refp, double* __restrict__ rec,
                                                                      double* __restrict__ vforce) {
  extern __shared__ __attribute__((aligned(16))) double bcf_lds[];
  __shared__ double sh[17], red[4][kBallForceSlots + 3];
  __shared__ double qs[12], qls[12], dq[12];  // q | the lag's q | q - q_ref: how far the body rows slid
  __shared__ int n_cpv, n_cpt, n_cpe, n_cbv, n_cbt, n_cbe, s_flags;
  __shared__ unsigned short cpv[kBallMaxCand], cpt[kBallMaxCand], cpe[kBallMaxCand];  // candidate pad vertices / triangles / edges
  __shared__ unsigned short cbv[kBallMaxCand], cbt[kBallMaxCand], cbe[kBallMaxCand];  // candidate ball vertices / triangles / edges
  constexpr int NT = 256;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = bd.nv;
  const size_t o = (size_t)b * V * 3;
  const double* x = xg + o;
  const double* xprev = xprevg ? xprevg + o : nullptr;
  double* xb = bcf_lds;
  double* vfl = vforce ? bcf_lds + (size_t)3 * nv : nullptr;
  const double dhat = bd.dhat, kap = bd.kappa, L = bd.dhat;
  bool fric = fric_mu > 0.0 && xprev != nullptr && qlagg != nullptr;
  double ref[3] = {0.0, 0.0, 0.0};
  if (refp) { ref[0] = refp[(size_t)b * 3]; ref[1] = refp[(size_t)b * 3 + 1]; ref[2] = refp[(size_t)b * 3 + 2]; }
  if (tid < 12) {
    const double qv = qg[(size_t)b * 12 + tid];
    qs[tid] = qv;
    qls[tid] = fric ? qlagg[(size_t)b * 12 + tid] : 0.0;
    dq[tid] = (fric && qrefg) ? qv - qrefg[(size_t)b * 12 + tid] : 0.0;
  }
  if (tid == 0) s_flags = 0;
  if (vfl)
    for (int k = tid; k < 3 * V; k += NT) vfl[k] = 0.0;
  __syncthreads();
  if (fric) {
    bool cleared = false;
#pragma unroll
    for (int k = 0; k < 12; ++k) cleared = cleared || qls[k] != qls[k] || dq[k] != dq[k];
    if (cleared) fric = false;  // (the same for every thread of the env)
  }

  double acc[kBallForceSlots];
#pragma unroll
  for (int k = 0; k < kBallForceSlots; ++k) acc[k] = 0.0;
  double dmin = INFINITY, gmin_b = INFINITY, gmin_p = INFINITY;

  // a force on a pad row: the net force (slot0 = 0: barrier, 3: friction; -1: ground, not part of the pad <- body wrench), its torque
  // about ref, the vertex's own sum
  auto pad_row = [&](int row, const double f[3], int slot0) {
    if (slot0 >= 0) {
      const double r[3] = {x[row * 3] - ref[0], x[row * 3 + 1] - ref[1], x[row * 3 + 2] - ref[2]};
      double tq[3];
      cross3(r, f, tq);
#pragma unroll
      for (int k = 0; k < 3; ++k) { if (slot0 == 0) acc[k] += f[k]; else acc[3 + k] += f[k]; acc[6 + k] += tq[k]; }
    }
    if (vfl) {
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicAdd(&vfl[row * 3 + k], f[k]);
    }
  };
  // friction force per unit coefficient of a lagged contact (lam, n) whose rows slid by rel: -mu lam f1(|u|) / |u| u, u the tangential part
  auto friction = [&](double lam, const double n[3], const double rel[3], double ff[3]) {
    double u[3], f0, fa, fb;
    ball_tangential(rel, n, u);
    ball_fric_law(sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), fric_eps, f0, fa, fb);
#pragma unroll
    for (int k = 0; k < 3; ++k) ff[k] = -fric_mu * lam * fa * u[k];
  };

  const int npass = fric ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const double* xp = pass ? xprev : x;   // the state the pass stands at
    const double* qq = pass ? qls : qs;
    __syncthreads();  // (the previous pass no longer reads xb and the lists)
    ball_points(bd, qq, xb, tid, NT);
    __syncthreads();
    // ---- ground, both bodies (fem_ball.h: the nodal gradient's ground part and its lag) ----
    if (bd.ground) {
      for (int k = tid; k < bd.nsv; k += NT) {
        const int v = bd.psv[k];
        const double w = bd.parea[v], gap = xp[v * 3 + 2] - bd.gh;
        if (!(gap > 0.0 && gap < dhat)) continue;
        double bb, b1, b2;
        barrier3(gap / dhat, bb, b1, b2);
        const double lam = ball_contact_lambda(kap, w, b1, dhat);
        if (pass == 0) {
          const double f[3] = {0.0, 0.0, lam};
          acc[40] += lam; acc[41] += 1.0;
          gmin_p = fmin(gmin_p, gap);
          pad_row(v, f, -1);
        } else {
          const double nz[3] = {0.0, 0.0, 1.0};
          const double rel[3] = {x[v * 3] - xp[v * 3], x[v * 3 + 1] - xp[v * 3 + 1], x[v * 3 + 2] - xp[v * 3 + 2]};
          double ff[3];
          friction(lam, nz, rel, ff);
          acc[38] += ff[0]; acc[39] += ff[1];
          pad_row(v, ff, -1);
        }
      }
      for (int k = tid; k < nv; k += NT) {
        const double gap = xb[k * 3 + 2] - bd.gh;
        if (!(gap > 0.0 && gap < dhat)) continue;
        double bb, b1, b2;
        barrier3(gap / dhat, bb, b1, b2);
        const double lam = ball_contact_lambda(kap, bd.area[k], b1, dhat);
        double f[3] = {0.0, 0.0, lam};
        if (pass == 0) {
          acc[34] += lam; acc[35] += lam; acc[36] += 1.0;
          gmin_b = fmin(gmin_b, gap);
        } else {
          const double nz[3] = {0.0, 0.0, 1.0};
          double rel[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
            for (int i = 0; i < 3; ++i) rel[i] += bd.Y[k * 4 + a4] * dq[a4 * 3 + i];
          friction(lam, nz, rel, f);
          acc[32] += f[0]; acc[33] += f[1];
        }
#pragma unroll
        for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
          for (int i = 0; i < 3; ++i) acc[20 + a4 * 3 + i] += bd.Y[k * 4 + a4] * f[i];
      }
    }
    // ---- candidates at reach d_hat; a ball triangle by the bounding box of its corners ----
    BallCull cl = {cpv, cpt, cpe, cbv, cbt, cbe, &n_cpv, &n_cpt, &n_cpe, &n_cbv, &n_cbt, &n_cbe, &s_flags};
    ball_cull<NT>(bd, cl, xp, qq, xb, L, sh, tid, [&](int t, const double* lo, const double* hi) __attribute__((always_inline)) {
      const int* tr = bd.tri + t * 3;
      bool in = true;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double a = xb[tr[0] * 3 + i], b2 = xb[tr[1] * 3 + i], c2 = xb[tr[2] * 3 + i];
        in = in && fmax(a, fmax(b2, c2)) >= lo[i] && fmin(a, fmin(b2, c2)) <= hi[i];
      }
      return in;
    });
    // ---- pairs of the three kinds over the candidates' products, one strided loop ----
    const int n0 = cl.npv * cl.nbt, n1 = cl.nbv * cl.npt, n2 = bd.ee ? cl.npe * cl.nbe : 0;
    for (int k = tid; k < n0 + n1 + n2; k += NT) {
      int kind, i, j;
      if (k < n0) { kind = 0; i = cpv[k / cl.nbt]; j = cbt[k % cl.nbt]; }
      else if (k < n0 + n1) { const int r = k - n0; kind = 1; i = cbv[r / cl.npt]; j = cpt[r % cl.npt]; }
      else { const int r = k - n0 - n1; kind = 2; i = cpe[r / cl.nbe]; j = cbe[r % cl.nbe]; }
      if (ball_pair_far(kind, i, j, xp, xb, bd, L)) continue;
      BallPairEval e;
      if (!ball_pair_eval<false>(kind, i, j, xp, xb, bd, e)) continue;
      double bb, b1, b2;
      barrier3(e.d / dhat, bb, b1, b2);
      const double lam = ball_contact_lambda(kap, e.w, b1, dhat);
      double fu[3];  // the force per unit coefficient: lam n (barrier) or the friction force of the lagged contact
      if (pass == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) fu[c] = lam * e.n[c];
        acc[9] += lam; acc[10] += 1.0;
        acc[16] += kind == 0 ? 1.0 : 0.0; acc[17] += kind == 1 ? 1.0 : 0.0; acc[18] += kind == 2 ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[12 + c] += lam * (e.cp[c] - ref[c]);
        dmin = fmin(dmin, e.d);
        if (e.molg > 0.0) {  // the mollifier's own term kappa w0 b m'(c) grad c on the four end points
          const double f = kap * e.molg * bb;
          const double f0[3] = {f * e.ga[0], f * e.ga[1], f * e.ga[2]}, f1[3] = {-f * e.ga[0], -f * e.ga[1], -f * e.ga[2]};
          pad_row(e.prow[0], f0, 0);
          pad_row(e.prow[1], f1, 0);
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[20 + a4 * 3 + c] -= f * e.yd[a4] * e.gbq[c];
        }
      } else {
        double rel[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
          for (int c = 0; c < 3; ++c) rel[c] += e.cq[a4] * dq[a4 * 3 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          if (e.prow[r] >= 0)
#pragma unroll
            for (int c = 0; c < 3; ++c) rel[c] += e.pco[r] * (x[e.prow[r] * 3 + c] - xp[e.prow[r] * 3 + c]);
        friction(lam, e.n, rel, fu);
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if (e.prow[r] < 0) continue;
        const double f[3] = {e.pco[r] * fu[0], e.pco[r] * fu[1], e.pco[r] * fu[2]};
        pad_row(e.prow[r], f, pass == 0 ? 0 : 3);
      }
#pragma unroll
      for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[20 + a4 * 3 + c] += e.cq[a4] * fu[c];
    }
  }

  // ---- reduction ----
#pragma unroll
  for (int k = 0; k < kBallForceSlots; ++k)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc[k] += __shfl_xor(acc[k], s, 64);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    dmin = fmin(dmin, __shfl_xor(dmin, s, 64));
    gmin_b = fmin(gmin_b, __shfl_xor(gmin_b, s, 64));
    gmin_p = fmin(gmin_p, __shfl_xor(gmin_p, s, 64));
  }
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kBallForceSlots; ++k) red[wid][k] = acc[k];
    red[wid][kBallForceSlots] = dmin; red[wid][kBallForceSlots + 1] = gmin_b; red[wid][kBallForceSlots + 2] = gmin_p;
  }
  __syncthreads();
  if (tid < kBallForceSlots) {
    const int k = tid;
    double out = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    const int mk = k == 15 ? kBallForceSlots : (k == 37 ? kBallForceSlots + 1 : (k == 42 ? kBallForceSlots + 2 : -1));
    if (mk >= 0) out = fmin(fmin(red[0][mk], red[1][mk]), fmin(red[2][mk], red[3][mk]));
    else if (k == 11) out = (double)s_flags;
    else if (k == 19 || k == 43) out = 0.0;
    else if (k >= 12 && k <= 14) {
      const double sl = ((red[0][9] + red[1][9]) + red[2][9]) + red[3][9];
      const double rk = k == 12 ? ref[0] : (k == 13 ? ref[1] : ref[2]);
      out = sl > 0.0 ? rk + out / sl : rk;
    }
    rec[(size_t)b * kBallForceSlots + k] = out;
  }
  if (vfl)
    for (int k = tid; k < 3 * V; k += NT) vforce[o + k] = vfl[k];
}

// a reset env has no friction reference until it steps: NaN in its q_prev row (every reader of that row in a step runs behind the
// step's predictor, which rewrites it; fem_ball_contact_forces_kernel tests for it)
__global__ __launch_bounds__(64) void fem_ball_clear_friction_ref_kernel(const int* __restrict__ ids, double* __restrict__ qprev, int B) {
  const int b = ids ? ids[blockIdx.x] : (int)blockIdx.x;
  if (b < 0 || b >= B) return;
  if (threadIdx.x < 12) qprev[(size_t)b * 12 + threadIdx.x] = __builtin_nan("");
}

}  // namespace tacex
