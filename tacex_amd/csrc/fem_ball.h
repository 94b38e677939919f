// The reference's own UIPC scene on the GPU (second slice):
// the gelpad (Stable Neo-Hookean tets, soft position constraints) + ONE FREE AFFINE-BODY BALL per env + the ground half-space, in IPC
// contact through point-triangle pairs in both directions and edge-edge pairs.  Reference call sites: ball_rolling_uipc.py:71-92 (ground_height 0.001,
// d_hat 5e-4, the ball as AffineBodyConstitutionCfg), uipc_object.py:62-74,456-466 (m_kappa 100 MPa, kinematic = False),
// uipc_sim.py:192-201 (ground + one default contact model).  The arithmetic is libuipc's, which is not in the reference tree: this
// follows oracle/abd_oracle.py (PARITY UNPINNED) term by term -
//   * the ball's 12 degrees of freedom are FOUR MORE ROWS of the env's state: y = (x_0 .. x_{V-1}, p, c_1, c_2, c_3), a surface point
//     of the ball is Y_b . (p, c_1, c_2, c_3) with Y_b = (1, X_b); inertia 1/2 (q - q~)^T (S (x) I) (q - q~), orthogonality energy
//     kappa vol |A^T A - I|^2 with its Gauss-Newton Hessian 4 kappa vol [delta_mn A A^T + c_n c_m^T];
//   * barrier kappa w b(d / d_hat) on every pair (pad surface vertex, ball triangle) and (ball vertex, pad surface triangle) closer
//     than d_hat, on every EDGE-EDGE pair (pad surface edge, ball edge) closer than d_hat (segment-segment distance, weight = the mean
//     of the two edge areas, IPC's mollifier of nearly parallel pairs), and of the ground against the surface vertices of both bodies;
//     Hessians b'' grad d grad d^T;
//   * lagged Coulomb friction of every one of those contacts (the cfg's one default contact model, US:103-124 / 192-201): normal force,
//     normal and barycentric weights frozen at the state the step starts from, sliding measured relative to it (IPC's lag);
//   * matrix-free PCG, every vector in LDS (tet rows by ds_add_f64, the tet state recomputed from x); preconditioner = the pad's vertex
//     chains (block-tridiagonal LDL^T through the thickness; a chain of one vertex = a 3 x 3 block) + the additive coarse correction of
//     the pad's coarse space (tacex_fem_set_coarse_space) + the EXACT inverse of the 12 x 12 ball block;
//   * step bound: ground gaps (linear), additive CCD on the listed pairs, no surface point further than 0.9 d_hat per iteration;
//   * backtracking line search on the plain incremental potential; convergence on the unscaled direction: velocity_tol * dt on the
//     position rows AND transrate_tol * dt on the ball's affine rows (UipcSimCfg.newton, uipc_sim.py:62-66).
// One workgroup (512 threads) per env, the whole Newton loop of a time step in ONE launch.  x and the six PCG vectors live in LDS for the
// whole launch; while an iteration's system is set up the idle PCG vectors hold the gradient, the pad's 3 x 3 blocks and, in the line
// search, the candidate; the workspace block (L2 / HBM) keeps the pair list and records, the ball's surface points and the direction for
// the step bound.  Pair candidates are rebuilt once per Newton iteration at reach 2.8 d_hat, which no pair
// outside can cross into d_hat within one bounded step, so the line search's energies are exact.  (The CU-resident kernel of the
// prescribed-indenter scenes keeps ALL per-vertex state in registers and is at its register limit: this scene got a kernel of its own.)
// The scene's tables, closest points, barrier and CCD, the evaluation of a pair, the candidate cull, the contact record and the friction
// law are fem_ball_pairs.h's, shared with the force report (fem_ball_contact_forces.h); here: the kernel and the two row kernels.

#pragma once
#include "fem_ball_pairs.h"  // BallDev, closest points, barrier, CCD, ball_pair_eval, ball_cull, the contact record, friction law

namespace tacex {

// dynamic LDS: x (V,3) | p (V + 4,3) | H.p accumulators = H.p (V,3) | z (V,3) | r (V + 4,3) | d (V + 4,3) (doubles) || chain factors (V,15)
// (floats) || chain successor / predecessor (V each, u16): every vector of the PCG loop, 104 KB at 495 vertices
__host__ __device__ inline size_t ball_lds_bytes(int V) {
  return ((((size_t)18 * V + 36) * sizeof(double) + (size_t)15 * V * sizeof(float) + (size_t)2 * V * sizeof(unsigned short)) + 15) & ~(size_t)15;
}

// mode 0: Newton loop of a time step; mode 1: energy and gradient at (x, q) only (terms entry point of the C ABI: tests)
#ifndef TACEX_BALL_WG_PER_CU
#define TACEX_BALL_WG_PER_CU 2  // waves per SIMD the kernel is compiled for (2 = one env per CU; A/B: 4 = two envs co-resident at <= 128 VGPRs, profiles/r06_experiments.md section 5)
#endif
template <int NT_>
__global__ __launch_bounds__(NT_, NT_ >= 512 ? TACEX_BALL_WG_PER_CU : 1) void fem_ball_newton_kernel(FemDev m, BallDev bd, double* xg, const double* xtg, double* qg, const double* qtg,
                                                              const uint8_t* consg, const double* aimg, double* wsg, int pcg_max_iter,
                                                              double pcg_tol_rate, int ls_max_iter, int max_newton, double dx_tol, double dc_tol,
                                                              double* step_info, int mode, double* e_out, double* g_out, const double* xprevg,
                                                              const double* qprevg, const int* env_order, const double* blkg) {
  extern __shared__ __attribute__((aligned(16))) double ball_lds[];  // x (V,3) | p (V + 4,3) | H.p accumulators (V,3): ball_lds_bytes()
  __shared__ double sh[17], sh2[16];
  __shared__ double gb[12], Bm[144], B0[144], Lc[144], Bi[144], YY[16], qs[12], qts[12], rhs12[12];
  __shared__ double crc[3 * kFemMaxCoarse], cyc[3 * kFemMaxCoarse];  // coarse residual / correction of the two-level preconditioner
  __shared__ double Hw[NT_ / 64 * 12];  // per-wave partial sums of the ball rows of H.p over the pair / friction records (one copy: 61 records x 12 atomic adds on 12 addresses)
  __shared__ double cpart[6 * kFemMaxCoarse];                        // ... the two halves of the coarse solve's sums
  __shared__ double qps[12], Hpq[12], zq[12];  // ... | the ball rows of H.p and of z  // the ball rows the time step started from (friction slides relative to them)
  __shared__ int n_cpv, n_cpt, n_cpe, n_cbv, n_cbt, n_cbe, n_pairs, n_act, n_fric, s_flags;
  __shared__ unsigned short cpv[kBallMaxCand], cpt[kBallMaxCand], cpe[kBallMaxCand];  // candidate pad vertices / triangles / edges (indices < 32768)
  __shared__ unsigned short cbv[kBallMaxCand], cbt[kBallMaxCand], cbe[kBallMaxCand];  // candidate ball vertices / triangles / edges
  // env_order: envs sorted by the solver work of their previous step, heaviest first (fem_env_order_kernel): a shard brings two envs
  // per CU, the launch ends with whatever the last-started ones need
  const int b = env_order ? env_order[blockIdx.x] : (int)blockIdx.x;
  constexpr int NT = NT_, NWV = NT_ / 64;  // threads / waves per env: 512 / 8 (two waves per SIMD, 256 VGPRs each) or 256 / 4 (one wave per SIMD with the whole register file)
  const int tid = threadIdx.x;
  const int V = m.V, T = m.T, nv = bd.nv, nt = bd.nt, VN = V + 4;
  const size_t o = (size_t)b * V * 3;
  double* x = xg + o;
  const double* xt = xtg + o;
  double* q = qg + (size_t)b * 12;
  const double* qt = qtg + (size_t)b * 12;
  const uint8_t* cons = consg ? consg + (size_t)b * V : nullptr;
  const double* aim = aimg ? aimg + o : nullptr;
  double* ws = wsg + (size_t)b * ball_ws_doubles(V, T, nv, nt);
  double* cbp = ws;                    // (V) ground curvature of the pad vertices at x (dt^2-scaled)
  double* xb = cbp + V;                // (nv,3) ball surface points at x
  double* xbc = xb + (size_t)3 * nv;   // ... at the candidate
  double* dxb = xbc + (size_t)3 * nv;  // ... their displacement along the Newton direction
  double* bts = dxb + (size_t)3 * nv;  // (nt,4) bounding sphere of every ball triangle at x
  int* plist = reinterpret_cast<int*>(bts + (size_t)4 * nt);  // (kBallMaxPairs) ball_pair_code
  double* arec = reinterpret_cast<double*>(plist + kBallMaxPairs);
  double* frec = arec + (size_t)kBallMaxActive * kBallRec;  // lagged friction contacts of the step (ball_rec_store, head = lam)
  double* fM = frec + (size_t)kBallMaxFric * kBallRec;      // their 3 x 3 Hessians at x (6 each, dt^2 mu lam [a T + (b - a) t t^T])
  // LAGGED COULOMB FRICTION of every contact (Li et al. 2020 eq. 18-20; US:103-124 friction ratio / eps_velocity, tacex_fem_set_friction): the
  // contacts of the state the step STARTS from - active pairs of both kinds, ground contacts of both bodies - are frozen as (normal force,
  // normal, coefficients of the relative displacement) in the first Newton iteration (x = x_n there) and slide relative to that state
  const double* xprev = xprevg ? xprevg + o : nullptr;
  const bool fric = m.fric_mu > 0.0 && xprev != nullptr && qprevg != nullptr;
  const double f_eps = m.fric_eps, f_mu = m.fric_mu;
  const double kUp[3] = {0.0, 0.0, 1.0};  // the ground's normal
  double* xs = ball_lds;           // (V,3) x of the iteration: the tet state is recomputed from it in every H.p (no cached F in HBM)
  double* ps = xs + 3 * V;         // (V + 4,3) PCG direction
  double* acc = ps + 3 * VN;       // (V,3) per-vertex sums of the tets' rows (ds_add_f64)
  double* rsl = acc + 3 * V;       // (V,3) z: the chain solve's r, then y, then z (in place), + the coarse correction
  double* rL = rsl + 3 * V;        // (V + 4,3) PCG residual
  double* dL = rL + 3 * VN;        // (V + 4,3) PCG solution (the Newton direction)
  // While an iteration's system is SET UP the PCG vectors are idle: the gradient (3 (V + 4)) and the pad's diagonal blocks (V,9) are built in
  // their place - hundreds of f64 atomic adds per iteration (pair / friction rows) then hit LDS instead of memory, and the chain
  // factorisation reads its blocks from LDS.  vg = dL's slot (rL = -vg, dL = 0 is the hand-over, element by element); Dinv = acc | z | the pad
  // rows of r, all read for the last time by the chain factorisation, one barrier before r is written.
  double* const vg = dL;
  double* const ycl = ps;  // line-search candidate (pad rows): the PCG direction's slot, idle between the PCG loop and the next one
  double* const Dinv = acc;
  float* cf = reinterpret_cast<float*>(dL + 3 * VN);                      // (V,15) chain factors: S^-1 (upper triangle, 6) | G (9)
  unsigned short* cnx = reinterpret_cast<unsigned short*>(cf + 15 * V);   // (V) chain successor, 0xffff = none
  unsigned short* cpr = cnx + V;                                           // (V) predecessor
  // elastic preconditioner blocks of the step: D (upper triangle) | E = A(v, next(v)) per vertex, assembled for all envs by
  // fem_assemble_blocks_kernel ahead of this launch at the state the step starts from ((V,16) per env; nullptr: mass blocks only)
  const double* blk = blkg ? blkg + (size_t)b * 16 * V : nullptr;
  const int nch = m.ch_next ? m.nch : V;
  for (int v = tid; v < V; v += NT) {
    cnx[v] = (unsigned short)(m.ch_next ? m.ch_next[v] : -1);
    cpr[v] = (unsigned short)(m.ch_prev ? m.ch_prev[v] : -1);
  }
  const double dt2 = m.dt * m.dt, dhat = bd.dhat, kk = dt2 * bd.kappa;
  const double L = dhat * (1.0 + kCcdSlack * kBallReach), R = kBallReach * dhat;

  if (tid < 12) { qs[tid] = q[tid]; qts[tid] = qt[tid]; qps[tid] = fric ? qprevg[(size_t)b * 12 + tid] : 0.0; }
  if (tid == 0) { s_flags = 0; n_fric = 0; }
  __syncthreads();

  auto fric_u = [&](const double* rc, const double* xx, const double* qq, double u[3]) {  // tangential relative displacement since the step's start
    const int* ri = ball_rec_rows(rc);
    double rel[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
      for (int i = 0; i < 3; ++i) rel[i] += rc[4 + a4] * (qq[a4 * 3 + i] - qps[a4 * 3 + i]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (ri[r] >= 0)
#pragma unroll
        for (int i = 0; i < 3; ++i) rel[i] += rc[8 + r] * (xx[ri[r] * 3 + i] - xprev[ri[r] * 3 + i]);
    ball_tangential(rel, rc + 1, u);
  };
  // energy of the state (xx pad vertices in global memory, qq ball rows in LDS, xbb its surface points): every term of
  // oracle/abd_oracle.py BallScene.energy; the pairs are those of the iteration's list
  auto energy = [&](const double* xx, const double* qq, const double* xbb) -> double {
    double e = 0.0;
    for (int t = tid; t < T; t += NT) {
      int v[4];
      double Di[9], F[9];
      load_tet(m, t, v, Di);
      deformation_gradient(xx, v, Di, F);
      TetState s;
      tet_state(m, F, s);
      e += dt2 * m.vol[t] * psi_of(m, s);
    }
    for (int v = tid; v < V; v += NT) {
      const double mv = m.mass[v];
      double qd = 0.0, qc = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double d = xx[v * 3 + i] - xt[v * 3 + i];
        qd += d * d;
        if (cons && cons[v]) { const double c = xx[v * 3 + i] - aim[v * 3 + i]; qc += c * c; }
      }
      e += 0.5 * mv * qd + 0.5 * m.strength * mv * qc;
      const double w = bd.parea[v];
      if (bd.ground && w > 0.0) {
        double bb, b1, b2;
        barrier3((xx[v * 3 + 2] - bd.gh) / dhat, bb, b1, b2);
        e += kk * w * bb;
      }
    }
    if (bd.ground)
      for (int k = tid; k < nv; k += NT) {
        double bb, b1, b2;
        barrier3((xbb[k * 3 + 2] - bd.gh) / dhat, bb, b1, b2);
        e += kk * bd.area[k] * bb;
      }
    if (tid == 0) {
      double ei = 0.0;
      for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) {
          double dd = 0.0;
#pragma unroll
          for (int i = 0; i < 3; ++i) dd += (qq[a * 3 + i] - qts[a * 3 + i]) * (qq[c * 3 + i] - qts[c * 3 + i]);
          ei += bd.S[a * 4 + c] * dd;
        }
      double eo = 0.0;
      for (int k = 0; k < 3; ++k)
        for (int l = 0; l < 3; ++l) {
          const double r = qq[3 + k * 3] * qq[3 + l * 3] + qq[4 + k * 3] * qq[4 + l * 3] + qq[5 + k * 3] * qq[5 + l * 3] - (k == l ? 1.0 : 0.0);
          eo += r * r;
        }
      e += 0.5 * ei + dt2 * bd.kv * eo;
    }
    const int np = n_pairs;
    for (int k = tid; k < np; k += NT) {
      int kind, pi, tj;
      ball_pair_decode(plist[k], kind, pi, tj);
      BallPairEval pe;  // (the energy takes d and w: the coefficients are dropped where this is inlined)
      if (!ball_pair_eval<true>(kind, pi, tj, xx, xbb, bd, pe)) continue;  // (w = 0: an exactly parallel edge pair - mollified away, whatever its distance)
      double bb, b1, b2;
      barrier3(pe.d / dhat, bb, b1, b2);
      e += kk * pe.w * bb;
    }
    if (fric) {
      const int nf = n_fric;
      for (int k = tid; k < nf; k += NT) {
        const double* rc = frec + (size_t)k * kBallRec;
        double u[3];
        fric_u(rc, xx, qq, u);
        double f0, fa, fb;
        ball_fric_law(sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), f_eps, f0, fa, fb);
        e += dt2 * f_mu * rc[0] * f0;
      }
    }
    return block_sum(e, sh);
  };
  // block-wide sum with ONE barrier (two alternating rows of wave partials: the row written two calls ago cannot still be read, a
  // barrier lies in between) - the PCG loop runs two of these per iteration
  int bphase = 0;
  auto bsum = [&](double v) -> double {
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) v += __shfl_xor(v, o2, 64);
    double* row = sh2 + 8 * (bphase & 1);
    ++bphase;
    if ((tid & 63) == 0) row[tid >> 6] = v;
    __syncthreads();
    double sv = 0.0;
#pragma unroll
    for (int w8 = 0; w8 < NWV; ++w8) sv += row[w8];
    return sv;
  };
  const bool coarse = m.nc > 0 && m.cn_off && m.ac_inv && (mode & 2) == 0;  // (mode bit 1: block Jacobi alone, A/B)
  // z = M^-1 r, everything in LDS (r = rL; z = rsl on the pad rows, zq on the ball rows): chain solve z = L^-T S^-1 L^-1 r in place (down the
  // chain y_i = r_i - G_{i-1}^T y_{i-1}, back up z_i = S_i^-1 y_i - G_i z_{i+1}) + the additive coarse correction P A_c^-1 P^T r of the
  // pad's coarse space (restriction by ds_add_f64 from the vertices' own 8 (node, weight) pairs) + the exact inverse of the ball block.
  // Returns r . z.
#ifdef TACEX_BALL_CLOCK  // debug build: cycles inside the PCG loop (sweep | vertex + records | dot + update | restriction + chains | coarse solve | prolongation + sum)
  long long pck[7] = {0, 0, 0, 0, 0, 0, 0}, pt0 = 0;
#define PCG_TICK0() do { pt0 = __builtin_readcyclecounter(); } while (0)
#define PCG_TICK(k) do { const long long n_ = __builtin_readcyclecounter(); pck[k] += n_ - pt0; pt0 = n_; } while (0)
#else
#define PCG_TICK0() do { } while (0)
#define PCG_TICK(k) do { } while (0)
#endif
  auto solve_chain = [&](int ch) {  // block-tridiagonal L D L^T solve along one vertex chain, in place in rsl (factors cf in LDS)
    chain_solve<true>(m.ch_next ? m.ch_head[ch] : ch, rsl, rsl, cf, cnx, cpr);
  };
  // z = M^-1 r (r in rL, z in rsl | zq); returns r . z.  Phases: (A) copy + restriction r_c = P^T r; (B) coarse solve on waves 0-5 WHILE waves 6-7
  // solve the chains; (C) the coarse solve's two halves; (D) prolongation + r . z.
  auto precondition = [&]() -> double {
    const int nc3 = 3 * m.nc;
    const int lane = tid & 63, wave = tid >> 6;
    PCG_TICK0();
    for (int k = tid; k < 3 * V; k += NT) rsl[k] = rL[k];
    if (coarse) {  // restriction, node by node over the node's vertex list (G lanes per node, as coarse_correct(); the first cut added 12 000 LDS
                   // atomics onto 180 addresses per application)
      restrict_to_coarse<false>(m, rL, crc, coarse_lanes_per_node(NT, m.nc), tid);
    }
    __syncthreads();
    PCG_TICK(3);
    double part = 0.0;
    if (tid < 12) {
      double zz = 0.0;
#pragma unroll
      for (int k = 0; k < 12; ++k) zz += Bi[tid * 12 + k] * rL[V * 3 + k];
      zq[tid] = zz;
      part += rL[V * 3 + tid] * zz;
    }
    constexpr int MW = NWV >= 8 ? 6 : 3, HALVES = MW / 3;  // waves of the coarse solve (three output chunks x one or two halves of the sum); the rest solve the chains
    if (coarse && NWV > MW) {
      // y_c = A_c^-1 r_c, a (3 nc)^2 <= 192^2 f64 matrix in L2.  The matrix is symmetric: lane = OUTPUT index, the loop runs down a COLUMN
      // block - every load instruction reads 512 contiguous bytes, eight of them in flight, no cross-lane reduction.  Six waves: three
      // output chunks of 64 x two halves of the sum.  (A thread walking its own row: 32 of a PCG iteration's 110 kcycles with the 60-node
      // grid - 180 dependent steps, 64 cache lines per load instruction; a wave per row with shuffles: 36.)
      if (wave < MW) {
        const int r = (wave % 3) * 64 + lane, jp = wave / 3;
        const int j0 = jp * (192 / HALVES), j1 = min(nc3, j0 + 192 / HALVES);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (r < nc3) {
          int jj = j0;
          for (; jj + 8 <= j1; jj += 8) {
            double a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = m.ac_inv[(size_t)(jj + u) * nc3 + r];
            s0 += a[0] * crc[jj] + a[4] * crc[jj + 4];
            s1 += a[1] * crc[jj + 1] + a[5] * crc[jj + 5];
            s2 += a[2] * crc[jj + 2] + a[6] * crc[jj + 6];
            s3 += a[3] * crc[jj + 3] + a[7] * crc[jj + 7];
          }
          for (; jj < j1; ++jj) s0 += m.ac_inv[(size_t)jj * nc3 + r] * crc[jj];
          cpart[jp * 3 * kFemMaxCoarse + r] = (s0 + s1) + (s2 + s3);
        }
      } else {  // ... while the last two waves solve the chains
        for (int ch = tid - MW * 64; ch < nch; ch += NT - MW * 64) solve_chain(ch);
      }
      __syncthreads();
      for (int k = tid; k < nc3; k += NT) cyc[k] = cpart[k] + (HALVES > 1 ? cpart[3 * kFemMaxCoarse + k] : 0.0);
      __syncthreads();
      for (int k = tid; k < nc3; k += NT) part += crc[k] * cyc[k];
    } else {
      for (int ch = tid; ch < nch; ch += NT) solve_chain(ch);
      __syncthreads();
    }
    PCG_TICK(4);
    for (int v = tid; v < V; v += NT) {
      double z0 = rsl[v * 3], z1 = rsl[v * 3 + 1], z2 = rsl[v * 3 + 2];
      part += rL[v * 3] * z0 + rL[v * 3 + 1] * z1 + rL[v * 3 + 2] * z2;  // (the chain part; the coarse part of r . z is crc . cyc above)
      if (coarse) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int nd = m.cv_node[v * 8 + k];
          const double w = m.cv_w[v * 8 + k];
          z0 += w * cyc[nd * 3]; z1 += w * cyc[nd * 3 + 1]; z2 += w * cyc[nd * 3 + 2];
        }
        rsl[v * 3] = z0; rsl[v * 3 + 1] = z1; rsl[v * 3 + 2] = z2;
      }
    }
    const double rzv = bsum(part);
    PCG_TICK(5);
    return rzv;
  };

#ifdef TACEX_BALL_CLOCK  // debug build: cycles of the phases of a step, printed by env 0 (scripts/r06/ball_clock.sh)
  long long bck[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bt0 = __builtin_readcyclecounter();
  long long sck[4] = {0, 0, 0, 0}, st0 = 0;
#define SUB_TICK0() do { st0 = __builtin_readcyclecounter(); } while (0)
#define SUB_TICK(k) do { const long long n_ = __builtin_readcyclecounter(); sck[k] += n_ - st0; st0 = n_; } while (0)
#define BALL_TICK(k) do { const long long n_ = __builtin_readcyclecounter(); bck[k] += n_ - bt0; bt0 = n_; } while (0)
#else
#define BALL_TICK(k) do { } while (0)
#define SUB_TICK0() do { } while (0)
#define SUB_TICK(k) do { } while (0)
#endif
  ball_points(bd, qs, xb, tid, NT);
  for (int k = tid; k < 3 * V; k += NT) xs[k] = x[k];
  __syncthreads();
  int n_newton = 0, pcg_total = 0;
  double e_carry = 0.0;
  bool have_e = false;
  double dmax_x = INFINITY, dmax_c = INFINITY;
  for (int nit = 0; nit < max_newton; ++nit) {
    const bool take_lag = fric && (nit == 0);  // (the first iteration stands at the state the step starts from)
    // ---- element pass (as fem_newton_kernel) + bounding spheres of the ball triangles + candidate lists ----
    for (int k = tid; k < 3 * VN; k += NT) vg[k] = 0.0;
    __syncthreads();
    for (int t = tid; t < T; t += NT) {  // (the tets' rows go straight into the LDS gradient: no (12,T) array through memory, no gather)
      int v[4];
      double Di[9], F[9], r[12], g[12];
      load_tet(m, t, v, Di);
      deformation_gradient(xs, v, Di, F);
      TetState s;
      tet_state(m, F, s);
      shape_rows(Di, r);
      element_gradient(s, r, dt2 * m.vol[t], g);
#pragma unroll
      for (int w4 = 0; w4 < 4; ++w4)
#pragma unroll
        for (int i = 0; i < 3; ++i) atomicAdd(&vg[v[w4] * 3 + i], g[w4 * 3 + i]);
    }
    for (int t = tid; t < nt; t += NT) {
      const int* tr = bd.tri + t * 3;
      double c3[3], rt = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) c3[i] = (xb[tr[0] * 3 + i] + xb[tr[1] * 3 + i] + xb[tr[2] * 3 + i]) * (1.0 / 3.0);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double r0 = xb[tr[k] * 3] - c3[0], r1 = xb[tr[k] * 3 + 1] - c3[1], r2 = xb[tr[k] * 3 + 2] - c3[2];
        rt = fmax(rt, sqrt(r0 * r0 + r1 * r1 + r2 * r2));
      }
      bts[t * 4] = c3[0]; bts[t * 4 + 1] = c3[1]; bts[t * 4 + 2] = c3[2]; bts[t * 4 + 3] = rt;
    }
    BALL_TICK(0);  // element pass, ball triangle spheres
    if (tid == 0) { n_pairs = 0; n_act = 0; }
    if (tid < 12) gb[tid] = 0.0;
    if (tid < 16) YY[tid] = 0.0;
    if (tid < 144) Bm[tid] = 0.0;
    // candidates at reach L (the cull's first barrier also stands behind the zeroing above); a ball triangle by its sphere
    BallCull cl = {cpv, cpt, cpe, cbv, cbt, cbe, &n_cpv, &n_cpt, &n_cpe, &n_cbv, &n_cbt, &n_cbe, &s_flags};
    ball_cull<NT>(bd, cl, xs, qs, xb, L, sh, tid, [&](int t, const double* lo, const double* hi) __attribute__((always_inline)) {
      const double rt = bts[t * 4 + 3];
      bool in = true;
#pragma unroll
      for (int i = 0; i < 3; ++i) in = in && bts[t * 4 + i] + rt >= lo[i] && bts[t * 4 + i] - rt <= hi[i];
      return in;
    });
    // pair list: the products of the candidate lists behind a cheap rejection, every pair closer than L.  Kinds 1 and 2 reject with
    // ball_pair_far; kind 0 keeps its own test against the triangle's sphere bts, which this kernel has at hand
    auto list_pair = [&](int kind, int i, int j) __attribute__((always_inline)) {
      BallPairEval pe;
      ball_pair_eval<false>(kind, i, j, xs, xb, bd, pe);  // (the distance alone is used)
      if (pe.d < L) {
        const int s = atomicAdd(&n_pairs, 1);
        if (s < kBallMaxPairs) plist[s] = ball_pair_code(kind, i, j);
      }
    };
    for (int k = tid; k < cl.npv * cl.nbt; k += NT) {
      const int v = cpv[k / cl.nbt], t = cbt[k - (k / cl.nbt) * cl.nbt];
      const double r0 = xs[v * 3] - bts[t * 4], r1 = xs[v * 3 + 1] - bts[t * 4 + 1], r2 = xs[v * 3 + 2] - bts[t * 4 + 2];
      const double lim = L + bts[t * 4 + 3];
      if (r0 * r0 + r1 * r1 + r2 * r2 < lim * lim) list_pair(0, v, t);
    }
    for (int k = tid; k < cl.nbv * cl.npt; k += NT) {
      const int bv = cbv[k / cl.npt], t = cpt[k - (k / cl.npt) * cl.npt];
      if (!ball_pair_far(1, bv, t, xs, xb, bd, L)) list_pair(1, bv, t);
    }
    for (int k = tid; k < cl.npe * cl.nbe; k += NT) {
      const int pe = cpe[k / cl.nbe], be_ = cbe[k - (k / cl.nbe) * cl.nbe];
      if (!ball_pair_far(2, pe, be_, xs, xb, bd, L)) list_pair(2, pe, be_);
    }
    __syncthreads();
    if (n_pairs > kBallMaxPairs) { if (tid == 0) { s_flags |= kBallFlagOverflow; n_pairs = kBallMaxPairs; } }
    __syncthreads();
    BALL_TICK(1);  // candidates, pair list
    // ---- nodal gradient, diagonal blocks (pad rows; pairs are added below), ground ----
    for (int v = tid; v < V; v += NT) {
      const double a3[3] = {vg[v * 3], vg[v * 3 + 1], vg[v * 3 + 2]};  // (the element pass's sums)
      const double mv = m.mass[v];
      const bool c = cons && cons[v];
      const double md = mv * (1.0 + (c ? m.strength : 0.0));
      double D[9] = {md, 0, 0, 0, md, 0, 0, 0, md};
      double gz = 0.0, cb = 0.0;
      const double w = bd.parea[v];
      if (bd.ground && w > 0.0) {
        double bb, b1, b2;
        barrier3((xs[v * 3 + 2] - bd.gh) / dhat, bb, b1, b2);
        if (!(xs[v * 3 + 2] - bd.gh > 0.0)) atomicOr(&s_flags, kFemFlagPenetration);
        gz = kk * w * b1 / dhat;
        cb = kk * w * b2 / (dhat * dhat);
        D[8] += cb;
        if (fric && take_lag && b1 < 0.0) {  // (inside the ground's barrier zone)
          const int sl = atomicAdd(&n_fric, 1);
          const double cq0[4] = {0.0, 0.0, 0.0, 0.0}, pco1[3] = {1.0, 0.0, 0.0};
          const int row1[3] = {v, -1, -1};
          if (sl < kBallMaxFric) ball_rec_store(frec + (size_t)sl * kBallRec, ball_contact_lambda(bd.kappa, w, b1, dhat), kUp, cq0, pco1, row1);
        }
      }
      cbp[v] = cb;
      if (blk) {  // elastic part: the step's lagged blocks (see blk above)
        const double* qb = blk + (size_t)v * 16;
        D[0] += qb[0]; D[1] += qb[1]; D[2] += qb[2]; D[3] += qb[1]; D[4] += qb[3]; D[5] += qb[4]; D[6] += qb[2]; D[7] += qb[4]; D[8] += qb[5];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) Dinv[(size_t)v * 9 + k] = D[k];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double gi = a3[i] + mv * (xs[v * 3 + i] - xt[v * 3 + i]);
        if (c) gi += m.strength * mv * (xs[v * 3 + i] - aim[v * 3 + i]);
        vg[v * 3 + i] = gi + (i == 2 ? gz : 0.0);
      }
    }
    if (bd.ground)
      for (int k = tid; k < nv; k += NT) {
        const double gap = xb[k * 3 + 2] - bd.gh;
        if (!(gap > 0.0)) atomicOr(&s_flags, kFemFlagPenetration);
        if (gap < dhat && gap > 0.0) {
          double bb, b1, b2;
          barrier3(gap / dhat, bb, b1, b2);
          const double f = kk * bd.area[k] * b1 / dhat, cb = kk * bd.area[k] * b2 / (dhat * dhat);
          if (fric && take_lag) {
            const int sl = atomicAdd(&n_fric, 1);
            const double pco0[3] = {0.0, 0.0, 0.0};
            const int row0[3] = {-1, -1, -1};
            if (sl < kBallMaxFric) ball_rec_store(frec + (size_t)sl * kBallRec, ball_contact_lambda(bd.kappa, bd.area[k], b1, dhat), kUp, bd.Y + k * 4, pco0, row0);
          }
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            atomicAdd(&gb[a * 3 + 2], f * bd.Y[k * 4 + a]);
#pragma unroll
            for (int c = 0; c < 4; ++c) atomicAdd(&YY[a * 4 + c], cb * bd.Y[k * 4 + a] * bd.Y[k * 4 + c]);
          }
        }
      }
    __syncthreads();
    BALL_TICK(2);  // gradient, elastic blocks, ground
    // ---- pairs at x: gradient, diagonal blocks, ball block, active records ----
    SUB_TICK0();
    {
      const int np = n_pairs;
      for (int k = tid; k < np; k += NT) {
        int kind, pi, tj;
        ball_pair_decode(plist[k], kind, pi, tj);
        BallPairEval pe;  // (LISTED: most of the listed edge pairs are outside d_hat and leave ahead of the mollifier)
        if (!ball_pair_eval<true>(kind, pi, tj, xs, xb, bd, pe)) continue;
        double bb, b1, b2;
        barrier3(pe.d / dhat, bb, b1, b2);
        const double s = kk * pe.w * b1 / dhat, wk = kk * pe.w * b2 / (dhat * dhat);
        if (pe.molg > 0.0) {
          const double f = kk * pe.molg * bb;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            atomicAdd(&vg[pe.prow[0] * 3 + i], -f * pe.ga[i]);
            atomicAdd(&vg[pe.prow[1] * 3 + i], f * pe.ga[i]);
#pragma unroll
            for (int a4 = 0; a4 < 4; ++a4) atomicAdd(&gb[a4 * 3 + i], f * pe.yd[a4] * pe.gbq[i]);
          }
        }
        // pad rows
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          if (pe.prow[r] < 0) continue;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            atomicAdd(&vg[pe.prow[r] * 3 + i], s * pe.pco[r] * pe.n[i]);
#pragma unroll
            for (int j = 0; j < 3; ++j) atomicAdd(&Dinv[(size_t)pe.prow[r] * 9 + i * 3 + j], wk * pe.pco[r] * pe.pco[r] * pe.n[i] * pe.n[j]);
          }
        }
        // ball rows
#pragma unroll
        for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            atomicAdd(&gb[a4 * 3 + i], s * pe.cq[a4] * pe.n[i]);
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
              for (int j = 0; j < 3; ++j) atomicAdd(&Bm[(a4 * 3 + i) * 12 + c4 * 3 + j], wk * pe.cq[a4] * pe.cq[c4] * pe.n[i] * pe.n[j]);
          }
        if (take_lag) {
          const int sf = atomicAdd(&n_fric, 1);
          if (sf < kBallMaxFric) ball_rec_store(frec + (size_t)sf * kBallRec, ball_contact_lambda(bd.kappa, pe.w, b1, dhat), pe.n, pe.cq, pe.pco, pe.prow);
        }
        const int sl = atomicAdd(&n_act, 1);
        if (sl < kBallMaxActive) ball_rec_store(arec + (size_t)sl * kBallRec, wk, pe.n, pe.cq, pe.pco, pe.prow);
      }
    }
    __syncthreads();
    if (n_act > kBallMaxActive) { if (tid == 0) { s_flags |= kBallFlagOverflow; n_act = kBallMaxActive; } }
    if (n_fric > kBallMaxFric) { if (tid == 0) { s_flags |= kBallFlagOverflow; n_fric = kBallMaxFric; } }
    SUB_TICK(0);
    if (fric) {  // friction of the lagged contacts at x: gradient, Hessians (kept for H.p), diagonal / ball blocks
      __syncthreads();
      const int nf = n_fric;
      // (records dealt to the waves round-robin: the ball rows of every record go to the SAME 12 + 144 LDS addresses, and lanes of one wave
      //  that add to one address are served one after the other - 60 records in wave 0 were 45 kcycles of this phase)
      for (int k = (tid & 63) * NWV + (tid >> 6); k < nf; k += NT) {
        const double* rc = frec + (size_t)k * kBallRec;
        const int* ri = ball_rec_rows(rc);
        double u[3], f0, fa, fb;
        fric_u(rc, xs, qs, u);
        const double yv = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        ball_fric_law(yv, f_eps, f0, fa, fb);
        const double cf = dt2 * f_mu * rc[0];
        const double iy = yv > 0.0 ? 1.0 / yv : 0.0;
        const double t3[3] = {u[0] * iy, u[1] * iy, u[2] * iy}, n3[3] = {rc[1], rc[2], rc[3]};
        double M[6];  // xx xy xz yy yz zz of cf [fa (I - n n^T) + (fb - fa) t t^T]
        {
          int kq = 0;
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) M[kq++] = cf * (fa * ((i == j ? 1.0 : 0.0) - n3[i] * n3[j]) + (fb - fa) * t3[i] * t3[j]);
        }
#pragma unroll
        for (int kq = 0; kq < 6; ++kq) fM[(size_t)k * 6 + kq] = M[kq];
        const double Mf[9] = {M[0], M[1], M[2], M[1], M[3], M[4], M[2], M[4], M[5]};
        const double g3[3] = {cf * fa * u[0], cf * fa * u[1], cf * fa * u[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          if (ri[r] < 0) continue;
          const double pc = rc[8 + r];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            atomicAdd(&vg[ri[r] * 3 + i], pc * g3[i]);
#pragma unroll
            for (int j = 0; j < 3; ++j) atomicAdd(&Dinv[(size_t)ri[r] * 9 + i * 3 + j], pc * pc * Mf[i * 3 + j]);
          }
        }
#pragma unroll
        for (int a4 = 0; a4 < 4; ++a4) {
          const double ca = rc[4 + a4];
          if (ca == 0.0) continue;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            atomicAdd(&gb[a4 * 3 + i], ca * g3[i]);
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4)
#pragma unroll
              for (int j = 0; j < 3; ++j) atomicAdd(&Bm[(a4 * 3 + i) * 12 + c4 * 3 + j], ca * rc[4 + c4] * Mf[i * 3 + j]);
          }
        }
      }
      __syncthreads();
    }
    SUB_TICK(1);
    // ---- ball rows: gradient, the block without the pairs (H.p) and with them (preconditioner, factored) ----
    if (tid < 144) {
      const int ra = tid / 12, ca = tid - ra * 12, a4 = ra / 3, i = ra - a4 * 3, c4 = ca / 3, j = ca - c4 * 3;
      double v = (i == j) ? bd.S[a4 * 4 + c4] : 0.0;
      if (a4 > 0 && c4 > 0) {  // 4 kappa vol dt^2 [delta_mn A A^T + c_n c_m^T], m = a4 - 1, n = c4 - 1
        const int mm = a4 - 1, nn = c4 - 1;
        double blk = qs[3 + nn * 3 + i] * qs[3 + mm * 3 + j];
        if (mm == nn) blk += qs[3 + i] * qs[3 + j] + qs[6 + i] * qs[6 + j] + qs[9 + i] * qs[9 + j];
        v += dt2 * 4.0 * bd.kv * blk;
      }
      if (i == 2 && j == 2) v += YY[a4 * 4 + c4];
      B0[tid] = v;
      Lc[tid] = v + Bm[tid];
    }
    if (tid < 12) {
      const int a4 = tid / 3, i = tid - a4 * 3;
      double g = 0.0;
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) g += bd.S[a4 * 4 + c4] * (qs[c4 * 3 + i] - qts[c4 * 3 + i]);
      if (a4 > 0) {
        const int mm = a4 - 1;
        double go = 0.0;
        for (int l = 0; l < 3; ++l) {
          const double r = qs[3 + mm * 3] * qs[3 + l * 3] + qs[4 + mm * 3] * qs[4 + l * 3] + qs[5 + mm * 3] * qs[5 + l * 3] - (mm == l ? 1.0 : 0.0);
          go += r * qs[3 + l * 3 + i];
        }
        g += dt2 * 4.0 * bd.kv * go;
      }
      vg[V * 3 + tid] = g + gb[tid];
    }
    __syncthreads();
    if (tid == 0) {  // Cholesky of the 12 x 12 block in place (lower triangle)
      for (int j = 0; j < 12; ++j) {
        double s = Lc[j * 12 + j];
        for (int k = 0; k < j; ++k) s -= Lc[j * 12 + k] * Lc[j * 12 + k];
        s = s > 0.0 ? sqrt(s) : sqrt(fmax(bd.S[0], 1e-300));  // (the block is SPD by construction: S (x) I is, the rest is PSD)
        Lc[j * 12 + j] = s;
        for (int i = j + 1; i < 12; ++i) {
          double t = Lc[i * 12 + j];
          for (int k = 0; k < j; ++k) t -= Lc[i * 12 + k] * Lc[j * 12 + k];
          Lc[i * 12 + j] = t / s;
        }
      }
    }
    __syncthreads();
    if (tid < 12) {  // column tid of the inverse: L L^T z = e_tid (twelve independent solves; applied by twelve dot products per PCG iteration)
      double yv[12];
      for (int i = 0; i < 12; ++i) {
        double sv = i == tid ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) sv -= Lc[i * 12 + k] * yv[k];
        yv[i] = sv / Lc[i * 12 + i];
      }
      for (int i = 11; i >= 0; --i) {
        double sv = yv[i];
        for (int k = i + 1; k < 12; ++k) sv -= Lc[k * 12 + i] * yv[k];
        yv[i] = sv / Lc[i * 12 + i];
      }
      for (int i = 0; i < 12; ++i) Bi[i * 12 + tid] = yv[i];
    }
    if (mode & 1) {  // terms only
      __syncthreads();
      const double E = energy(x, qs, xb);
      if (tid == 0 && e_out) e_out[b] = E;
      if (g_out)
        for (int k = tid; k < 3 * VN; k += NT) g_out[(size_t)b * 3 * VN + k] = vg[k];
      if (tid == 0 && step_info) step_info[(size_t)b * 4 + 2] = (double)s_flags;
      return;
    }
    SUB_TICK(2);
    // block part of the pad's preconditioner: block-tridiagonal LDL^T along the vertex chains of tacex_fem_set_chains (the columns of
    // vertices through the pad's thickness; a chain of one vertex = 3 x 3 block Jacobi) - S_0 = D_0, G_i = S_i^-1 E_i,
    // S_{i+1} = D_{i+1} - E_i^T G_i, the thread of a chain walks it (fem_newton_lds_kernel does the same); S^-1 | G as floats in LDS
    for (int ch = tid; ch < nch; ch += NT)
      chain_factor(m.ch_next ? m.ch_head[ch] : ch,
                   [&](int v, double (&Dv)[9]) __attribute__((always_inline)) {
#pragma unroll
                     for (int k = 0; k < 9; ++k) Dv[k] = Dinv[(size_t)v * 9 + k];
                   },
                   [&](int v, const double*& Ev) __attribute__((always_inline)) {  // (no blk table: every vertex a chain of its own)
                     if (!blk) return false;
                     Ev = blk + (size_t)v * 16 + 6;
                     return true;
                   }, cf, cnx);
    __syncthreads();  // (the chains have read their blocks: r may take over the tail of their slot)
    for (int k = tid; k < 3 * VN; k += NT) { rL[k] = (bd.kinematic && k >= 3 * V) ? 0.0 : -vg[k]; dL[k] = 0.0; }  // (a fixed body: zero residual rows stay zero through the PCG)
    __syncthreads();
    SUB_TICK(3);
    BALL_TICK(3);  // pairs, friction, ball blocks, factorisation, pad block inverses
    // ---- PCG: every vector in LDS (x, p, H.p = the accumulators of the tets' rows, z, r, d); the mesh constants, the blocks' tables and
    //      the pair records are what it reads from memory ----
    for (int k = tid; k < 3 * V; k += NT) acc[k] = 0.0;  // (xs holds x since the kernel's start / the last accepted step)
    __syncthreads();
    constexpr int VS = 1024 / NT;  // vertices per thread (V <= 697: ball_lds_ok)
    double md_r[VS], cb_r[VS];  // this thread's vertices: mass (+ constraint) diagonal and ground curvature, constant through the PCG loop
#pragma unroll
    for (int sl = 0; sl < VS; ++sl) {
      const int v = tid + sl * NT;
      md_r[sl] = v < V ? m.mass[v] * (1.0 + ((cons && cons[v]) ? m.strength : 0.0)) : 0.0;
      cb_r[sl] = v < V ? cbp[v] : 0.0;
    }
    double rz = precondition();
    for (int k = tid; k < 3 * V; k += NT) ps[k] = rsl[k];
    if (tid < 12) ps[V * 3 + tid] = zq[tid];
    const double rz0 = rz;
    int it = 0;
    __syncthreads();
    while (it < pcg_max_iter && rz0 > 0.0 && rz > pcg_tol_rate * rz0) {
      PCG_TICK0();
      for (int t = tid; t < T; t += NT) {
        int v[4];
        double Di[9], F[9], dF[9], dP[9], r[12];
        load_tet(m, t, v, Di);
        deformation_gradient(xs, v, Di, F);
        TetState s;
        tet_state(m, F, s);
        deformation_gradient(ps, v, Di, dF);
        apply_dP(m, s, dF, dP);
        shape_rows(Di, r);
        double rows[12];
        element_hp_rows(dP, r, dt2 * m.vol[t], rows);
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4)
#pragma unroll
          for (int i = 0; i < 3; ++i) atomicAdd(&acc[v[w4] * 3 + i], rows[w4 * 3 + i]);
      }
      __syncthreads();
      PCG_TICK(0);
#pragma unroll
      for (int sl = 0; sl < VS; ++sl) {
        const int v = tid + sl * NT;
        if (v < V) {
#pragma unroll
          for (int i = 0; i < 3; ++i) acc[v * 3 + i] += md_r[sl] * ps[v * 3 + i] + (i == 2 ? cb_r[sl] * ps[v * 3 + 2] : 0.0);  // acc IS H.p from here on
        }
      }
      if (tid < 12) {
        double sv = 0.0;
        for (int k = 0; k < 12; ++k) sv += B0[tid * 12 + k] * ps[V * 3 + k];
        Hpq[tid] = sv;
      }
      if (tid >= 64 && tid < 64 + NWV * 12) Hw[tid - 64] = 0.0;
      __syncthreads();
      PCG_TICK(6);
      // records are dealt to the waves round-robin (record k -> wave k % 8, lane k / 8) and each wave adds the ball rows into its own copy
      double* const hw = Hw + 12 * (tid >> 6);
      {
        const int na = n_act;
        for (int k = (tid & 63) * NWV + (tid >> 6); k < na; k += NT) {
          const double* rc = arec + (size_t)k * kBallRec;
          const int* ri = ball_rec_rows(rc);
          const double n0 = rc[1], n1 = rc[2], n2 = rc[3];
          double gp = 0.0;
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4) gp += rc[4 + a4] * (n0 * ps[(V + a4) * 3] + n1 * ps[(V + a4) * 3 + 1] + n2 * ps[(V + a4) * 3 + 2]);
#pragma unroll
          for (int r = 0; r < 3; ++r)
            if (ri[r] >= 0) gp += rc[8 + r] * (n0 * ps[ri[r] * 3] + n1 * ps[ri[r] * 3 + 1] + n2 * ps[ri[r] * 3 + 2]);
          const double f = rc[0] * gp;
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4) {
            atomicAdd(&hw[a4 * 3], f * rc[4 + a4] * n0);
            atomicAdd(&hw[a4 * 3 + 1], f * rc[4 + a4] * n1);
            atomicAdd(&hw[a4 * 3 + 2], f * rc[4 + a4] * n2);
          }
#pragma unroll
          for (int r = 0; r < 3; ++r)
            if (ri[r] >= 0) {
              atomicAdd(&acc[ri[r] * 3], f * rc[8 + r] * n0);
              atomicAdd(&acc[ri[r] * 3 + 1], f * rc[8 + r] * n1);
              atomicAdd(&acc[ri[r] * 3 + 2], f * rc[8 + r] * n2);
            }
        }
      }
      if (fric) {
        const int nf = n_fric;
        for (int k = (tid & 63) * NWV + (tid >> 6); k < nf; k += NT) {
          const double* rc = frec + (size_t)k * kBallRec;
          const int* ri = ball_rec_rows(rc);
          const double* M = fM + (size_t)k * 6;
          double w3[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4)
#pragma unroll
            for (int i = 0; i < 3; ++i) w3[i] += rc[4 + a4] * ps[(V + a4) * 3 + i];
#pragma unroll
          for (int r = 0; r < 3; ++r)
            if (ri[r] >= 0)
#pragma unroll
              for (int i = 0; i < 3; ++i) w3[i] += rc[8 + r] * ps[ri[r] * 3 + i];
          const double mw[3] = {M[0] * w3[0] + M[1] * w3[1] + M[2] * w3[2], M[1] * w3[0] + M[3] * w3[1] + M[4] * w3[2],
                                M[2] * w3[0] + M[4] * w3[1] + M[5] * w3[2]};
#pragma unroll
          for (int a4 = 0; a4 < 4; ++a4)
            if (rc[4 + a4] != 0.0)
#pragma unroll
              for (int i = 0; i < 3; ++i) atomicAdd(&hw[a4 * 3 + i], rc[4 + a4] * mw[i]);
#pragma unroll
          for (int r = 0; r < 3; ++r)
            if (ri[r] >= 0)
#pragma unroll
              for (int i = 0; i < 3; ++i) atomicAdd(&acc[ri[r] * 3 + i], rc[8 + r] * mw[i]);
        }
      }
      __syncthreads();
      PCG_TICK(1);
      double part = 0.0;
      for (int k = tid; k < 3 * V; k += NT) part += ps[k] * acc[k];
      if (tid < 12) {
#pragma unroll
        for (int w8 = 0; w8 < NWV; ++w8) Hpq[tid] += Hw[w8 * 12 + tid];
        if (bd.kinematic) Hpq[tid] = 0.0;  // a fixed body: its rows of the operator are eliminated (only thread tid reads Hpq[tid] below)
        part += ps[V * 3 + tid] * Hpq[tid];
      }
      const double pHp = bsum(part);
      if (!(pHp > 0.0)) {
        if (it == 0) {
          for (int k = tid; k < 3 * V; k += NT) dL[k] = rsl[k];
          if (tid < 12) dL[V * 3 + tid] = zq[tid];
        }
        break;
      }
      const double al = rz / pHp;
      for (int k = tid; k < 3 * V; k += NT) { dL[k] += al * ps[k]; rL[k] -= al * acc[k]; acc[k] = 0.0; }  // (acc: zero for the next sweep)
      if (tid < 12) { dL[V * 3 + tid] += al * ps[V * 3 + tid]; rL[V * 3 + tid] -= al * Hpq[tid]; }
      __syncthreads();
      PCG_TICK(2);
      const double rz_new = precondition();
      const double beta = rz_new / rz;
      for (int k = tid; k < 3 * V; k += NT) ps[k] = rsl[k] + beta * ps[k];
      if (tid < 12) ps[V * 3 + tid] = zq[tid] + beta * ps[V * 3 + tid];
      rz = rz_new;
      ++it;
      __syncthreads();
    }
    __syncthreads();
    pcg_total += it;
    BALL_TICK(4);  // PCG
    // ---- step bound ----
    if (tid < 12) rhs12[tid] = dL[V * 3 + tid];
    __syncthreads();
    ball_points(bd, rhs12, dxb, tid, NT);
    __syncthreads();
    double amax = 1.0, vmax = 0.0, dmx = 0.0, dmc = 0.0;
    for (int v = tid; v < V; v += NT) {
      const double d0 = dL[v * 3], d1 = dL[v * 3 + 1], d2 = dL[v * 3 + 2];
      dmx = fmax(dmx, fmax(fabs(d0), fmax(fabs(d1), fabs(d2))));
      if (bd.parea[v] > 0.0) {
        vmax = fmax(vmax, sqrt(d0 * d0 + d1 * d1 + d2 * d2));
        const double gap = xs[v * 3 + 2] - bd.gh;
        if (bd.ground && d2 < 0.0 && gap > 0.0) amax = fmin(amax, kCcdSlack * gap / -d2);
      }
    }
    for (int k = tid; k < nv; k += NT) {
      const double d0 = dxb[k * 3], d1 = dxb[k * 3 + 1], d2 = dxb[k * 3 + 2];
      vmax = fmax(vmax, sqrt(d0 * d0 + d1 * d1 + d2 * d2));
      const double gap = xb[k * 3 + 2] - bd.gh;
      if (bd.ground && d2 < 0.0 && gap > 0.0) amax = fmin(amax, kCcdSlack * gap / -d2);
    }
    if (tid < 3) dmx = fmax(dmx, fabs(dL[V * 3 + tid]));
    if (tid >= 3 && tid < 12) dmc = fabs(dL[V * 3 + tid]);
    vmax = block_sum_max(vmax, sh);
    dmx = block_sum_max(dmx, sh);
    dmc = block_sum_max(dmc, sh);
    if (vmax > 0.0) amax = fmin(amax, kCcdSlack * R / (2.0 * vmax));
    amax = -block_sum_max(-amax, sh);
    {
      double al = amax;
      const int np = n_pairs;
      for (int k = tid; k < np; k += NT) {
        int kind, pi, tj;
        ball_pair_decode(plist[k], kind, pi, tj);
        if (kind == 2) {
          const int* ea = bd.pedge + pi * 2;
          const int* eb = bd.bedge + tj * 2;
          double pa[6], pb[6], da[6], db[6];
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              pa[j * 3 + i] = xs[ea[j] * 3 + i]; da[j * 3 + i] = dL[ea[j] * 3 + i];
              pb[j * 3 + i] = xb[eb[j] * 3 + i]; db[j * 3 + i] = dxb[eb[j] * 3 + i];
            }
          double sa, tb, d, n[3];
          ee_closest(pa, pa + 3, pb, pb + 3, sa, tb, d, n);
          if (d < R) al = fmin(al, accd_ee(pa, pb, da, db, al));
          continue;
        }
        const int* tr = (kind == 0 ? bd.tri : bd.ptri) + tj * 3;
        double p3[3], trx[9], dp[3], dtr[9];
        const double* P = kind == 0 ? xs : xb;
        const double* dP_ = kind == 0 ? dL : dxb;
        const double* Tq = kind == 0 ? xb : xs;
        const double* dT = kind == 0 ? dxb : dL;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          p3[i] = P[pi * 3 + i]; dp[i] = dP_[pi * 3 + i];
#pragma unroll
          for (int j = 0; j < 3; ++j) { trx[j * 3 + i] = Tq[tr[j] * 3 + i]; dtr[j * 3 + i] = dT[tr[j] * 3 + i]; }
        }
        double be[3], d, n[3];
        pt_closest(p3, trx, trx + 3, trx + 6, be, d, n);
        if (d < R) al = fmin(al, accd_pt(p3, trx, dp, dtr, al));
      }
      amax = -block_sum_max(-al, sh);
    }
    dmax_x = dmx; dmax_c = dmc;
    // ---- backtracking line search (first E <= E0 wins; rescue halvings as in the other Newton kernels) ----
    BALL_TICK(5);  // step bound (ground, additive CCD)
    // E(x): the accepted candidate's energy of the previous iteration IS this iteration's (every pair inside d_hat is in both lists)
    const double E0 = have_e ? e_carry : energy(xs, qs, xb);
    double step = amax, E1 = E0;
    bool accepted = false;
    const int ls_cap = ls_max_iter > kLsRescueStream ? ls_max_iter : kLsRescueStream;
    for (int ls = 0; ls <= ls_cap; ++ls) {
      for (int k = tid; k < 3 * V; k += NT) ycl[k] = xs[k] + step * dL[k];  // (the candidate in the idle PCG direction's slot; dL still holds d)
      if (tid < 12) rhs12[tid] = qs[tid] + step * dL[V * 3 + tid];
      __syncthreads();
      ball_points(bd, rhs12, xbc, tid, NT);
      __syncthreads();
      const double Ec = energy(ycl, rhs12, xbc);
      if (Ec <= E0) { E1 = Ec; accepted = true; e_carry = Ec; have_e = true; break; }
      step *= 0.5;
      __syncthreads();
    }
    // REFINEMENT (mode bits 8-11 = bisections: tacex_fem_set_line_search_refine): a step the halving had to cut was cut by a pair ENTERING the barrier zone (10 GPa against a
    // 0.1 MPa gel: a few um inside cost more than the step gains, r06 section 15), and the accepted half usually leaves that pair just
    // OUTSIDE - where it has no curvature for the next iteration either, which is then cut again.  A few bisections between the accepted and
    // the last rejected step find a larger one that still decreases E and has the pair inside, active in the next Hessian.
    const int n_refine = (mode >> 8) & 15;
    if (accepted && step < amax && n_refine > 0) {
      double lo_s = step, hi_s = 2.0 * step;
      for (int rf = 0; rf < n_refine; ++rf) {
        const double mid = 0.5 * (lo_s + hi_s);
        __syncthreads();
        for (int k = tid; k < 3 * V; k += NT) ycl[k] = xs[k] + mid * dL[k];
        if (tid < 12) rhs12[tid] = qs[tid] + mid * dL[V * 3 + tid];
        __syncthreads();
        ball_points(bd, rhs12, xbc, tid, NT);
        __syncthreads();
        const double Ec = energy(ycl, rhs12, xbc);
        if (Ec <= E0) { lo_s = mid; E1 = Ec; e_carry = Ec; } else { hi_s = mid; }
      }
      // (the candidate buffers hold the LAST trial: rebuild them at the accepted step)
      step = lo_s;
      __syncthreads();
      for (int k = tid; k < 3 * V; k += NT) ycl[k] = xs[k] + step * dL[k];
      if (tid < 12) rhs12[tid] = qs[tid] + step * dL[V * 3 + tid];
      __syncthreads();
      ball_points(bd, rhs12, xbc, tid, NT);
      __syncthreads();
    }
    ++n_newton;
    BALL_TICK(6);  // line search
#ifdef TACEX_BALL_TRACE  // debug build: the late Newton iterations of the envs that need them (scripts/r06/ball_trace.py)
    if (tid == 0 && (nit >= 2 || it >= 20))
      printf("trace env %d newton %d: pcg %d amax %.3e step %.3e E0 %.12e dE %.3e dmx %.3e (tol %.1e) dmc %.3e (tol %.1e) pairs %d act %d fric %d\n", b, nit, it, amax, step,
             E0, E1 - E0, dmx, dx_tol, dmc, dc_tol, n_pairs, n_act, n_fric);
#endif
    if (accepted) {
      for (int k = tid; k < 3 * V; k += NT) { const double v_ = ycl[k]; x[k] = v_; xs[k] = v_; }
      for (int k = tid; k < 3 * nv; k += NT) xb[k] = xbc[k];
      __syncthreads();
      if (tid < 12) qs[tid] = rhs12[tid];
    } else if (!(dmx <= dx_tol && dmc <= dc_tol)) {
      if (tid == 0) s_flags |= kFemFlagLsFailed;
      __syncthreads();
      break;
    }
    __syncthreads();
    if (dmx <= dx_tol && dmc <= dc_tol) break;
  }
#ifdef TACEX_BALL_CLOCK
  if (tid == 0 && (b == 0 || b == (int)gridDim.x - 1))
    printf("ball clock env %d: newton %d pcg %d | kcycles: element %lld candidates %lld gradient+blocks %lld pairs+factor %lld PCG %lld stepbound %lld linesearch %lld | inside PCG: sweep %lld vertex %lld records %lld dot+update %lld restrict+chains %lld coarse %lld prolong+sum %lld | phase 3: pairs %lld friction %lld ball block %lld chains %lld\n", b,
           n_newton, pcg_total, bck[0] / 1000, bck[1] / 1000, bck[2] / 1000, bck[3] / 1000, bck[4] / 1000, bck[5] / 1000, bck[6] / 1000, pck[0] / 1000, pck[6] / 1000, pck[1] / 1000,
           pck[2] / 1000, pck[3] / 1000, pck[4] / 1000, pck[5] / 1000, sck[0] / 1000, sck[1] / 1000, sck[2] / 1000, sck[3] / 1000);
#endif
  if (tid < 12) q[tid] = qs[tid];
  if (tid == 0 && step_info) {
    double* si = step_info + (size_t)b * 4;
    si[0] = (double)n_newton; si[1] = fmax(dmax_x, dmax_c); si[2] = (double)s_flags; si[3] = (double)pcg_total;
  }
}

// predictor / velocity of the ball rows (the pad's go through fem_predict_kernel / fem_velocity_kernel)
__global__ __launch_bounds__(256) void fem_ball_predict_kernel(const double* __restrict__ q, const double* __restrict__ qv, double* __restrict__ qt,
                                                               double* __restrict__ qprev, int B, double dt, double g0, double g1, double g2) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B * 12) return;
  const int r = k % 12;
  const double g = r == 0 ? g0 : (r == 1 ? g1 : (r == 2 ? g2 : 0.0));  // gravity acts on the translation row p
  qprev[k] = q[k];
  qt[k] = q[k] + dt * qv[k] + dt * dt * g;
}
__global__ __launch_bounds__(256) void fem_ball_velocity_kernel(const double* __restrict__ q, const double* __restrict__ qprev, double* __restrict__ qv,
                                                                int B, double inv_dt) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < B * 12) qv[k] = (q[k] - qprev[k]) * inv_dt;
}

}  // namespace tacex
