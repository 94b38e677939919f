// FEM device layer: the streaming Newton kernel (K17b), one projected-Newton iteration per launch with its vectors in memory.
#pragma once
#include "fem_device.h"
#include "fem_terms.h"

namespace tacex {

// ---- K17b: one projected-Newton iteration per env, everything inside one workgroup -----------------------------
// (workspace per env: newton_ws_doubles, fem_layout.h)

template <bool MAT>
__global__ __launch_bounds__(512) void fem_newton_kernel(FemDev m, double* xg, const double* xtg, const uint8_t* consg,
                                                         const double* aimg, double* stats, double* wsg,
                                                         int pcg_max_iter, double pcg_tol_rate, int ls_max_iter, double* dxg, double dx_tol,
                                                         double* step_info, int accumulate, const double* xprevg, const double* dispg,
                                                         int fric_ipc, int lds_sweep, FemMat mat) {
  // step_info (nullable): the row of this env [Newton iterations, max |d|, flags, PCG iterations] - SET by the first launch of a time
  // step (accumulate = 0), added to / OR-ed by the later ones: tacex_fem_step runs this kernel once per Newton iteration, and
  // UipcSim.check_step() must see a penetrating vertex or a dead line search of ANY of them (the row used to be zeroed)
  __shared__ double sh[17];
  __shared__ double crc[3 * kFemMaxCoarse], cyc[3 * kFemMaxCoarse];
  // lds_sweep (round 6; atomic mode only, 9 V doubles of dynamic LDS): x, the PCG direction p and per-vertex H.p accumulators live in LDS - a
  // tet recomputes its state from x, gathers p from LDS and ADDS its rows with ds_add_f64, instead of reading a cached state (96 B) and
  // writing rows (96 B) through HBM and a CSR gather afterwards: what made this kernel 4x slower per iteration than the CU-resident one.
  // The deterministic switch keeps the fixed-order gather (lds_sweep = 0).
  extern __shared__ __attribute__((aligned(16))) double nws_lds[];
  const int b = blockIdx.x;
  if (dxg && dxg[b] <= dx_tol) {  // converged in an earlier launch of this time step (same protocol as the CU-resident kernel)
    if (threadIdx.x == 0) { stats[(size_t)b * 4 + 2] = 0.0; stats[(size_t)b * 4 + 3] = 0.0; }
    return;
  }
  const bool mat_bad = env_material<MAT>(m, mat, b);
  const int V = m.V, T = m.T;
  const size_t o = (size_t)b * V * 3;
  double* x = xg + o;
  const double* xt = xtg + o;
  const uint8_t* cons = consg ? consg + (size_t)b * V : nullptr;
  const double* aim = aimg ? aimg + o : nullptr;
  double* ws = wsg + (size_t)b * newton_ws_doubles(V, T);
  double* ge = ws;                       // (12,T) tet gradients, later diag-block scratch
  double* tc = ws + (size_t)12 * T;      // (12,T) F(9), a, b, c
  double* hv = ws + (size_t)24 * T;      // (12,T) per-tet H*p contributions
  double* vg = ws + (size_t)36 * T;      // g
  // lds_sweep = 2: the PCG's r, z, d and H.p live in LDS as well (21 V doubles: 120 KB at 715 vertices) - the direction is computed and
  // consumed (step bound, line search) inside this launch, so nothing of the loop has to pass through memory (the workspace slots stay
  // where they are: the layout is one)
  double* vr = lds_sweep == 2 ? nws_lds + 9 * V : vg + (size_t)3 * V;
  double* vz = lds_sweep == 2 ? nws_lds + 12 * V : vg + (size_t)6 * V;
  double* vp = lds_sweep ? nws_lds + 3 * V : vg + (size_t)9 * V;
  double* xs_l = nws_lds;                   // (V,3) x
  double* acc_l = nws_lds + 6 * V;          // (V,3) accumulators
  double* vd = lds_sweep == 2 ? nws_lds + 15 * V : vg + (size_t)12 * V;
  double* vHp = lds_sweep == 2 ? nws_lds + 18 * V : vg + (size_t)15 * V;
  double* xc = vg + (size_t)18 * V;      // line-search candidate
  double* Dinv = xc + (size_t)3 * V;     // (V,9)
  double* cdat = Dinv + (size_t)9 * V;   // (V,5) barrier of the vertex at x: dt^2 b'' | n (3) | gap d
  double* flag_ = cdat + (size_t)5 * V;  // (V,4) friction lag: normal force | normal - taken in the FIRST launch of a time step, kept for its others
  double* fhs = flag_ + (size_t)4 * V;   // (V,6) friction Hessian block of the vertex at x (dt^2-scaled, rounded to float like the CU-resident kernel's)
  const double dt2 = m.dt * m.dt;
  // IPC barrier against the env's indenter (the same terms as in the CU-resident kernel: gradient b' n, PSD curvature b'' n n^T in
  // H.p and the block-Jacobi blocks, conservative step bound before the line search) and, since round 5, Coulomb friction with the lag
  // taken at the start of the step (capped by the contact reaction, or IPC's previous-configuration lag: tacex_fem_set_friction_lag).
  // Vertex chains, the coarse correction, the contact-following start and the edge snap exist in the CU-resident kernel only - this
  // is the path of meshes with more vertices than its workgroup has threads.
  const double* ind = (m.indenters && m.area) ? m.indenters + (size_t)b * 8 : nullptr;
  bool mesh_bad;
  const IndMesh im = env_mesh<true>(m, b, ind, mesh_bad);
  const bool fric = ind && m.fric_mu > 0.0 && xprevg != nullptr && dispg != nullptr;
  const double* xn = fric ? xprevg + o : nullptr;
  double disp3[3] = {0, 0, 0};
  if (fric) { disp3[0] = dispg[b * 3]; disp3[1] = dispg[b * 3 + 1]; disp3[2] = dispg[b * 3 + 2]; }
  const double* fl = fric ? flag_ : nullptr;

  // ---- element pass: cache F and coefficients, tet gradients, diagonal 3x3 blocks (into hv as (4*9? no: 12 rows)) ----
  // the four 3x3 diagonal blocks of the element Hessian need 36 doubles per tet: use ge+tc? they are needed later,
  // so diagonal blocks are accumulated vertex-side from recomputed columns below (second loop) instead.
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int v[4];
    double Di[9], F[9], r[12], g[12];
    load_tet(m, t, v, Di);
    deformation_gradient(x, v, Di, F);
    TetState s;
    tet_state(m, F, s);
    shape_rows(Di, r);
    element_gradient(s, r, dt2 * m.vol[t], g);
#pragma unroll
    for (int k = 0; k < 12; ++k) ge[(size_t)k * T + t] = g[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) tc[(size_t)k * T + t] = F[k];
    tc[(size_t)9 * T + t] = s.a; tc[(size_t)10 * T + t] = s.b; tc[(size_t)11 * T + t] = s.c;
  }
  __syncthreads();
  // ---- nodal gradient + block-Jacobi preconditioner (vertex gather; diagonal blocks recomputed per incidence) ----
  int pen = 0;  // a contact vertex of this thread sits at or beyond its indenter's surface (kFemFlagPenetration)
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    double a3[3];
    gather_vertex(m, ge, v, a3);
    const double mv = m.mass[v];
    const bool c = cons && cons[v];
    const double md = mv * (1.0 + (c ? m.strength : 0.0));
    double D[9] = {md, 0, 0, 0, md, 0, 0, 0, md};
    double cg[3] = {0, 0, 0};
    {
      const double xv[3] = {x[v * 3], x[v * 3 + 1], x[v * 3 + 2]};
      const ContactEval ce = contact_eval(m, im, ind, ind ? m.area[v] : 0.0, xv);
      if (ce.penetrating) pen = 1;
      const double cb2 = ce.active ? dt2 * ce.b2 : 0.0;
      cdat[(size_t)v * 5] = cb2;
      cdat[(size_t)v * 5 + 1] = ce.n[0]; cdat[(size_t)v * 5 + 2] = ce.n[1]; cdat[(size_t)v * 5 + 3] = ce.n[2];
      cdat[(size_t)v * 5 + 4] = (ind && m.area[v] > 0.0 && !ce.penetrating) ? ce.d : 1e300;
      if (ce.active) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          cg[i] = dt2 * ce.b1 * ce.n[i];
#pragma unroll
          for (int k = 0; k < 3; ++k) D[i * 3 + k] += cb2 * ce.n[i] * ce.n[k];
        }
      }
    }
    for (int e = m.vt_off[v]; e < m.vt_off[v + 1]; ++e) {
      const int code = m.vt_idx[e];
      const int t = code >> 2, l = code & 3;
      double Di[9], r[12];
#pragma unroll
      for (int k = 0; k < 9; ++k) Di[k] = m.dminv[(size_t)k * T + t];
      shape_rows(Di, r);
      TetState s;
      cached_tet_state(tc, T, t, s);
      const double sc = dt2 * m.vol[t];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double dF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dP[9];
        dF[k * 3 + 0] = r[l * 3 + 0]; dF[k * 3 + 1] = r[l * 3 + 1]; dF[k * 3 + 2] = r[l * 3 + 2];
        apply_dP(m, s, dF, dP);
#pragma unroll
        for (int i = 0; i < 3; ++i)
          D[i * 3 + k] += sc * (dP[i * 3 + 0] * r[l * 3 + 0] + dP[i * 3 + 1] * r[l * 3 + 1] + dP[i * 3 + 2] * r[l * 3 + 2]);
      }
    }
    double fg[3] = {0, 0, 0};
    if (fric) {
      const double xv[3] = {x[v * 3], x[v * 3 + 1], x[v * 3 + 2]};
      if (!accumulate) {  // first launch of the time step: the lag (FrictionModel.update of the oracle; fem_newton_lds_kernel's lag_pending)
        double lam = 0.0, ln[3] = {cdat[(size_t)v * 5 + 1], cdat[(size_t)v * 5 + 2], cdat[(size_t)v * 5 + 3]};
        if (fric_ipc) {
          lam = friction_lag_ipc<true>(m, im, ind, m.area[v], disp3, xn + v * 3, ln);
        } else {
          const ContactEval ce = contact_eval(m, im, ind, m.area[v], xv);
          if (ce.active) {
            double go[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              go[i] = a3[i] + mv * (xv[i] - xt[v * 3 + i]);
              if (c) go[i] += m.strength * mv * (xv[i] - aim[v * 3 + i]);
            }
            lam = friction_lag_capped(ce, go, dt2);
            ln[0] = ce.n[0]; ln[1] = ce.n[1]; ln[2] = ce.n[2];
          }
        }
        const bool on = lam > 0.0;
        flag_[(size_t)v * 4] = on ? lam : 0.0;
        flag_[(size_t)v * 4 + 1] = on ? ln[0] : 0.0; flag_[(size_t)v * 4 + 2] = on ? ln[1] : 0.0; flag_[(size_t)v * 4 + 3] = on ? ln[2] : 0.0;
      }
      const double xn3[3] = {xn[v * 3], xn[v * 3 + 1], xn[v * 3 + 2]};
      const FricEval fe = friction_eval(m.fric_mu, m.fric_eps, flag_ + (size_t)v * 4, xv, xn3, disp3, true);
      double h[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) { h[k] = (double)(float)(dt2 * fe.h[k]); fhs[(size_t)v * 6 + k] = h[k]; }
#pragma unroll
      for (int i = 0; i < 3; ++i) fg[i] = dt2 * fe.g[i];
      D[0] += h[0]; D[1] += h[1]; D[2] += h[2]; D[3] += h[1]; D[4] += h[3]; D[5] += h[4]; D[6] += h[2]; D[7] += h[4]; D[8] += h[5];
    }
    double Di3[9];
    if (!inv3_spd(D, Di3)) {  // elastic block not SPD -> mass block (always SPD)
      const double im = 1.0 / md;
      Di3[0] = im; Di3[1] = 0; Di3[2] = 0; Di3[3] = 0; Di3[4] = im; Di3[5] = 0; Di3[6] = 0; Di3[7] = 0; Di3[8] = im;
    }
    // rounded to float like the blocks the CU-resident kernel keeps in LDS: the two kernels apply the SAME preconditioner
    const int up[9] = {0, 1, 2, 1, 4, 5, 2, 5, 8};
#pragma unroll
    for (int k = 0; k < 9; ++k) Dinv[(size_t)v * 9 + k] = (double)(float)Di3[up[k]];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double gi = a3[i] + mv * (x[v * 3 + i] - xt[v * 3 + i]) + cg[i] + fg[i];
      if (c) gi += m.strength * mv * (x[v * 3 + i] - aim[v * 3 + i]);
      vg[v * 3 + i] = gi;
      vr[v * 3 + i] = -gi;
      vd[v * 3 + i] = 0.0;
    }
  }
  const int any_pen = __syncthreads_or(pen);
  // z = Dinv r ; p = z ; rz
  double part = 0.0;
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double z = apply_block3_row(Dinv + (size_t)v * 9, vr + v * 3, i);
      vz[v * 3 + i] = z;
      part += vr[v * 3 + i] * z;
    }
  }
  // two-level preconditioner (round 6): block Jacobi + the additive coarse correction of tacex_fem_set_coarse_space - what the CU-resident
  // kernel applies minus its vertex chains; meshes beyond its reach (> 768 vertices, or the deterministic switch) no longer pay block
  // Jacobi's iteration counts.  The summation order is fixed: deterministic runs stay bit-identical.
  const bool two_level = m.nc > 0 && m.cn_off && m.ac_inv;
  if (two_level) {
    __syncthreads();
    part += coarse_correct(m, vr, vz, crc, cyc);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) vp[k] = vz[k];
  double rz = block_sum(part, sh);
  const double rz0 = rz;
  int it = 0;
  if (lds_sweep) {
    for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) { xs_l[k] = x[k]; acc_l[k] = 0.0; }
    __syncthreads();
  }
  while (it < pcg_max_iter && rz0 > 0.0 && rz > pcg_tol_rate * rz0) {  // (libuipc's test: on r.z itself, see fem_newton_lds_kernel)
    // ---- Hp = (M + s Mc + dt^2 K) p, matrix-free: per-tet dP[dF(p)] then vertex gather ----
    for (int t = threadIdx.x; lds_sweep && t < T; t += blockDim.x) {
      int v[4];
      double Di[9], F[9], dF[9], dP[9], r[12];
      load_tet(m, t, v, Di);
      deformation_gradient(xs_l, v, Di, F);
      TetState s;
      tet_state(m, F, s);
      deformation_gradient(vp, v, Di, dF);
      apply_dP(m, s, dF, dP);
      shape_rows(Di, r);
      double rows[12];
      element_hp_rows(dP, r, dt2 * m.vol[t], rows);
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int i = 0; i < 3; ++i) atomicAdd(&acc_l[v[w] * 3 + i], rows[w * 3 + i]);
    }
    for (int t = threadIdx.x; !lds_sweep && t < T; t += blockDim.x) {
      int v[4];
      double Di[9], dF[9], dP[9], r[12];
      load_tet(m, t, v, Di);
      deformation_gradient(vp, v, Di, dF);  // linear in p
      TetState s;
      cached_tet_state(tc, T, t, s);
      apply_dP(m, s, dF, dP);
      shape_rows(Di, r);
      double rows[12];
      element_hp_rows(dP, r, dt2 * m.vol[t], rows);
#pragma unroll
      for (int k = 0; k < 12; ++k) hv[(size_t)k * T + t] = rows[k];
    }
    __syncthreads();
    part = 0.0;
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
      double a3[3];
      if (lds_sweep) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { a3[i] = acc_l[v * 3 + i]; acc_l[v * 3 + i] = 0.0; }  // (zeroed for the next sweep by the thread that read it)
      } else {
        gather_vertex(m, hv, v, a3);
      }
      const double md = m.mass[v] * (1.0 + ((cons && cons[v]) ? m.strength : 0.0));
      const double cb2 = cdat[(size_t)v * 5];
      const double npq = cb2 * (cdat[(size_t)v * 5 + 1] * vp[v * 3] + cdat[(size_t)v * 5 + 2] * vp[v * 3 + 1] + cdat[(size_t)v * 5 + 3] * vp[v * 3 + 2]);
      double fp[3] = {0, 0, 0};
      if (fric) {
        const double* q = fhs + (size_t)v * 6;
        const double p0 = vp[v * 3], p1 = vp[v * 3 + 1], p2 = vp[v * 3 + 2];
        fp[0] = q[0] * p0 + q[1] * p1 + q[2] * p2; fp[1] = q[1] * p0 + q[3] * p1 + q[4] * p2; fp[2] = q[2] * p0 + q[4] * p1 + q[5] * p2;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double h = a3[i] + md * vp[v * 3 + i] + npq * cdat[(size_t)v * 5 + 1 + i] + fp[i];
        vHp[v * 3 + i] = h;
        part += vp[v * 3 + i] * h;
      }
    }
    const double pHp = block_sum(part, sh);
    if (!(pHp > 0.0)) {  // negative curvature: keep d (first iteration: preconditioned steepest descent)
      if (it == 0)
        for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) vd[k] = vz[k];
      break;
    }
    const double al = rz / pHp;
    part = 0.0;
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
      double rr[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        vd[v * 3 + i] += al * vp[v * 3 + i];
        rr[i] = vr[v * 3 + i] - al * vHp[v * 3 + i];
        vr[v * 3 + i] = rr[i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double z = apply_block3_row(Dinv + (size_t)v * 9, rr, i);
        vz[v * 3 + i] = z;
        part += rr[i] * z;
      }
    }
    if (two_level) {
      __syncthreads();
      part += coarse_correct(m, vr, vz, crc, cyc);
      __syncthreads();
    }
    const double rz_new = block_sum(part, sh);
    const double beta = rz_new / rz;
    for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) vp[k] = vz[k] + beta * vp[k];
    rz = rz_new;
    ++it;
    __syncthreads();
  }
  __syncthreads();
  // ---- backtracking line search on the incremental potential (accept the first E(x + step d) <= E(x)) ----
  const double E0 = env_energy(m, x, xt, cons, aim, sh, im, ind, fl, xn, disp3);  // (lag rows: written and read by the vertex's own thread)
  double step = 1.0, E1 = E0;
  if (ind) {  // conservative step bound (1-Lipschitz distance): no surface vertex may use more than kCcdSlack of its gap
    double amax = 1.0;
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
      const double gap = cdat[(size_t)v * 5 + 4];
      const double nd = sqrt(vd[v * 3] * vd[v * 3] + vd[v * 3 + 1] * vd[v * 3 + 1] + vd[v * 3 + 2] * vd[v * 3 + 2]);
      if (gap < 1e299 && nd > 0.0) amax = fmin(amax, kCcdSlack * gap / nd);
    }
    step = -block_sum_max(-amax, sh);
  }
  // max |d| of the unscaled Newton direction (the convergence test; also caps the search: no vertex starts further than the body is long,
  // the direction kept on negative curvature has no length scale - same rule as the CU-resident kernel)
  double dmax = 0.0;
  for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) dmax = fmax(dmax, fabs(vd[k]));
  dmax = block_sum_max(dmax, sh);
  if (dmax > m.step_cap) step = fmin(step, m.step_cap / dmax);
  bool accepted = false;
  const int ls_cap = ind ? (ls_max_iter > kLsRescueStream ? ls_max_iter : kLsRescueStream) : ls_max_iter;
  for (int ls = 0; ls <= ls_cap; ++ls) {
    for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) xc[k] = x[k] + step * vd[k];
    __syncthreads();
    const double Ec = env_energy(m, xc, xt, cons, aim, sh, im, ind, fl, xn, disp3);
    if (Ec <= E0) { E1 = Ec; accepted = true; break; }
    step *= 0.5;
  }
  if (accepted) {
    for (int k = threadIdx.x; k < 3 * V; k += blockDim.x) x[k] = xc[k];
  } else {
    step = 0.0;
  }
  if (threadIdx.x == 0) {
    // max |d| of the unscaled direction: <= dx_tol = converged (same rule as the CU-resident kernel).  A rejected search leaves x where it
    // was - every further launch of the step would repeat this iteration: the env is taken out of the step's remaining launches (0 = done),
    // its flag says why (the CU-resident kernel and the oracle's fem_step break out of their loops the same way)
    if (dxg) dxg[b] = (step_info && !accepted && !(dmax <= dx_tol)) ? 0.0 : dmax;  // (tacex_fem_step only: tacex_fem_newton_step's callers read max |d| itself)
    stats[(size_t)b * 4 + 0] = E0; stats[(size_t)b * 4 + 1] = E1; stats[(size_t)b * 4 + 2] = step; stats[(size_t)b * 4 + 3] = (double)it;
    if (step_info) {
      const int fl = (any_pen ? kFemFlagPenetration : 0) | ((!accepted && !(dmax <= dx_tol)) ? kFemFlagLsFailed : 0) |
                     (mesh_bad ? kFemFlagBadMesh : 0) | (mat_bad ? kFemFlagBadMaterial : 0);
      double* si = step_info + (size_t)b * 4;
      si[0] = (accumulate ? si[0] : 0.0) + 1.0;
      si[1] = dmax;
      si[2] = (double)((accumulate ? (int)si[2] : 0) | fl);
      si[3] = (accumulate ? si[3] : 0.0) + (double)it;
    }
  }
}

}  // namespace tacex
