// Gelpad FEM inner step for MI355X (gfx950), float64, batched over independent environments.
//
// What libuipc's world.advance() executes for the TacEx gelpad (tacex_uipc/sim/uipc_sim.py:250-252;
// StableNeoHookean + ElasticModuli.youngs_poisson, tacex_uipc/objects/uipc_object.py:442-470; soft position
// constraints, tacex_uipc/sim/uipc_attachments.py:139-142,364-428).  libuipc is an un-vendored submodule, so
// this follows the published model (Smith, de Goes, Kim 2018, eq. 14) - see oracle/fem_oracle.py, PARITY UNPINNED.
//
//   Psi(F) = mu/2 (Ic-3) + lam/2 (J-alpha)^2 - mu/2 log(Ic+1) - Psi(I)
//   P      = a F + c C,         a = mu (1 - 1/(Ic+1)),  c = lam (J - alpha),  C = cof F = [f1xf2, f2xf0, f0xf1]
//   dP[dF] = a dF + b (F:dF) F + lam (C:dF) C + c dC[dF],   b = 2 mu / (Ic+1)^2
//   E(x)   = 1/2 sum m |x-xt|^2 + dt^2 sum vol Psi(F) + 1/2 s sum_{constrained} m |x-aim|^2
//
// Design (bandwidth-bound, no MFMA): one tet per lane for element terms with element-minor SoA outputs
// (energy (B,T), grad (B,12,T), hess (B,144,T)) so every store is coalesced; nodal assembly is an atomics-free
// vertex gather over a CSR incidence list; reductions are wave shuffles + LDS; the Newton step runs as ONE
// workgroup per environment - matrix-free PCG (block-Jacobi preconditioned) and the backtracking line search
// stay inside a single launch with no host round trip.
//
// One translation unit.  The device code is one header per kernel family (DESIGN.md has the map); this file keeps the context, the
// LDS bookkeeping of the launches and the C API.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "fem_layout.h"
#include "tacex_hip.h"
#include "tacex_internal.h"

#include "fem_device.h"         // scene description, contact, friction, tet helpers, reductions, shared preconditioner steps
#include "fem_terms.h"          // element terms, energy, gradient
#include "fem_newton_stream.h"  // fem_newton_kernel
#include "fem_ball.h"           // fem_ball_newton_kernel: pad + affine body + ground
#include "fem_ball_contact_forces.h"  // fem_ball_contact_forces_kernel: the ball scene's contact forces and wrenches at a state
#include "fem_newton_lds.h"     // fem_newton_lds_kernel
#include "fem_assemble.h"       // fem_assemble_blocks_kernel
#include "fem_step_kernels.h"   // order, predict, velocity, reset, attachment, markers
#include "fem_contact_forces.h" // fem_contact_forces_kernel: contact forces and net wrench at a state

using namespace tacex;

struct tacex_fem_ctx {
  int device = 0;
  FemDev dev{};  // THE parameter block: the natural tet tables and everything the setters write
  // the same tets renumbered for fem_newton_lds_kernel and fem_assemble_blocks_kernel (see tacex_fem_create); tet_rec and tet_blk exist
  // in this numbering only (null in dev)
  struct {
    const int* tets = nullptr; const double* dminv = nullptr; const double* vol = nullptr; const int* vt_idx = nullptr;
    const double* tet_rec = nullptr; const double* tet_blk = nullptr;
  } nwt;
  FemMat mat{};      // the gel material library (tacex_fem_set_material_library); one copy: every launch hands it over
  // Friction slides relative to the indenter's displacement since the previous tacex_fem_step.  The previous positions (B,3) live
  // in the caller's workspace (no allocation in a compute call); the context remembers WHICH workspace and env count they were
  // written for, so another workspace or num_envs never reads stale data, and a new indenter TENSOR for the same contact (the
  // caller animating the indenter by passing fresh tensors) keeps them: only disabling contact or its first enable resets.
  const void* ind_prev_ws = nullptr;
  int ind_prev_B = 0;
  const double* rest = nullptr;  // (V,3) rest positions (tacex_fem_reset_envs)
  int last_resident = -1;       // which Newton kernel the last launch used: 1 CU-resident, 0 streaming, -1 none yet (tacex_fem_newton_resident)
  int last_threads = 0;         // block size of the last Newton launch (tacex_fem_newton_route), 0 = none yet
  int last_lds_mode = -1;       // its streaming-kernel LDS mode (2, 1, 0), -1 for the CU-resident and ball kernels
  int ls_refine = 4;            // bisections after a cut line search in fem_ball_newton_kernel (tacex_fem_set_line_search_refine)
  int fric_lag_mode = 0;        // 0: lag at the step's start state, capped by the contact reaction (round 4); 1: IPC's previous-configuration lag
  bool deterministic = false;   // window + CSR-gather sweeps (fixed summation order) instead of LDS atomics (tacex_fem_set_deterministic)
  bool follow_indenter = true;  // contact-following start of the Newton loop (tacex_fem_set_contact_following; fem_newton_lds_kernel)
  double* dx_dev = nullptr;  // optional (B,) last Newton update max|dx| per env: converged envs skip further iterations
  double dx_tol = 0.0;
  tacex::BallDev ball{};     // the env's free affine body + ground (tacex_fem_set_affine_body); nv == 0: none
  const void* ball_last_ws = nullptr;  // workspace / env count whose "q at the end of the previous step" rows are valid (kinematic bodies)
  int ball_last_B = 0;
  const void* ball_step_ws = nullptr;  // workspace / env count of the last tacex_fem_ball_step: its x_prev / q_prev rows are that step's start state
  int ball_step_B = 0;                 // (tacex_fem_ball_contact_forces takes its friction lag from them)
  // what tacex_fem_set_material_library needs to build a material's mass table (lumped_mass)
  std::vector<int> tets_host;    // (4,T) SoA, re-oriented
  std::vector<double> vol_host;  // (T)
  double fric_scene = 0.0;       // the ratio tacex_fem_set_friction gave (FemDev::fric_mu is the library's largest while a library is set)
  std::vector<void*> allocs;
};

// Tables a setter REPLACES (coarse space, chains, indenter mesh, vertex areas) are freed once nothing can read them any more:
// the setters are host-synchronous set-up calls, so they drain the device first (a caller who refreshed the
// preconditioner every step grew the device memory without bound).
// what the CU-resident Newton kernel and the block assembly get: dev with the tet tables in their numbering
static FemDev newton_dev(const tacex_fem_ctx* c) {
  FemDev d = c->dev;
  d.tets = c->nwt.tets; d.dminv = c->nwt.dminv; d.vol = c->nwt.vol; d.vt_idx = c->nwt.vt_idx;
  d.tet_rec = c->nwt.tet_rec; d.tet_blk = c->nwt.tet_blk;
  return d;
}

// The LDS bookkeeping of ONE kernel instantiation, per device: what a workgroup can get next to the kernel's static __shared__
// (dynamic_lds_limit) and what has been granted so far (ensure_dynamic_lds).  route<kernel>() is the only way to a kernel that takes
// dynamic LDS, so a kernel and its tables cannot be paired wrongly.
struct LdsTables { size_t avail[64] = {}, granted[64] = {}; };
template <typename K>
struct Route {
  K kern = nullptr;
  LdsTables* lds = nullptr;
  const void* id() const { return reinterpret_cast<const void*>(kern); }
};
template <auto KERN>
static Route<decltype(KERN)> route() {
  static LdsTables t;
  return {KERN, &t};
}

// Stable Neo-Hookean constants of a gel (Smith et al. 2018, eq. 14 with the rest-stable reparametrisation): the ONE place they are
// computed, so an env of a library material computes bit for bit what a scene created with that material computes
struct GelConstants { double mu, lam, alpha, psi_rest; };
static GelConstants gel_constants(double youngs, double poisson) {
  const double mu_l = youngs / (2.0 * (1.0 + poisson));
  const double lam_l = youngs * poisson / ((1.0 + poisson) * (1.0 - 2.0 * poisson));
  GelConstants g;
  g.mu = 4.0 / 3.0 * mu_l;
  g.lam = lam_l + 5.0 / 6.0 * mu_l;
  g.alpha = 1.0 + 0.75 * g.mu / g.lam;
  g.psi_rest = 0.5 * g.lam * (1.0 - g.alpha) * (1.0 - g.alpha) - 0.5 * g.mu * log(4.0);
  return g;
}

// lumped mass per vertex, added INTO mass (V, zeroed by the caller): a quarter of every incident tet's, tets in order (fixed summation order)
static void lumped_mass(double density, const std::vector<int>& tets_soa, const std::vector<double>& vol, int T, double* mass) {
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < 4; ++k) mass[tets_soa[(size_t)k * T + t]] += density * vol[t] / 4.0;
}

template <typename T>
static void fem_release(tacex_fem_ctx* c, const T*& ptr, bool* synced) {
  if (!ptr) return;
  if (!*synced) { (void)hipDeviceSynchronize(); *synced = true; }
  void* p = const_cast<void*>(static_cast<const void*>(ptr));
  for (size_t i = 0; i < c->allocs.size(); ++i)
    if (c->allocs[i] == p) { c->allocs.erase(c->allocs.begin() + (long)i); (void)hipFree(p); break; }
  ptr = nullptr;
}

template <typename T>
static int fem_upload(tacex_fem_ctx* c, const std::vector<T>& h, const T** out) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, h.size() * sizeof(T) + 16);
  if (e != hipSuccess) return fail_hip(e, "hipMalloc(fem table)");
  c->allocs.push_back(p);
  e = hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail_hip(e, "hipMemcpy(fem table)");
  *out = static_cast<const T*>(p);
  return 0;
}

// signed distance of every vertex to its env's indenter (the solver's own distance function): what a caller needs to keep the
// "approach by less than the gap" contract of tacex_fem_step without restating the indenter geometry
__global__ __launch_bounds__(256) void fem_contact_gaps_kernel(FemDev m, const double* xg, double* gaps) {
  const int b = blockIdx.x;
  const double* ind = m.indenters ? m.indenters + (size_t)b * 8 : nullptr;
  bool bad;
  const IndMesh im = env_mesh<true>(m, b, ind, bad);
  for (int v = threadIdx.x; v < m.V; v += blockDim.x) {
    const double* x = xg + ((size_t)b * m.V + v) * 3;
    const double x3[3] = {x[0], x[1], x[2]};
    const ContactEval c = contact_eval<true>(m, im, ind, 1.0, x3);
    gaps[(size_t)b * m.V + v] = c.d < 1e299 ? c.d : INFINITY;
  }
}

// unique edges (lower index first) of a triangle list, the area each stands for (a third of its triangles' rest areas: the edge areas sum
// to the surface area) and its squared rest length - oracle/abd_oracle.py surface_edges
static void surface_edges(const std::vector<int>& tri, const double* X, std::vector<int>& edges, std::vector<double>& earea, std::vector<double>& elen2) {
  std::map<std::pair<int, int>, double> acc;
  for (size_t t = 0; t + 2 < tri.size(); t += 3) {
    const double* a = X + (size_t)tri[t] * 3; const double* b = X + (size_t)tri[t + 1] * 3; const double* cc = X + (size_t)tri[t + 2] * 3;
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
    const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double ta = 0.5 * sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    for (int k = 0; k < 3; ++k) {
      const int u = tri[t + k], v = tri[t + (k + 1) % 3];
      acc[{u < v ? u : v, u < v ? v : u}] += ta / 3.0;
    }
  }
  edges.clear(); earea.clear(); elen2.clear();
  for (const auto& kv : acc) {
    const int u = kv.first.first, v = kv.first.second;
    edges.push_back(u); edges.push_back(v);
    earea.push_back(kv.second);
    double l2 = 0.0;
    for (int i = 0; i < 3; ++i) { const double dd = X[(size_t)v * 3 + i] - X[(size_t)u * 3 + i]; l2 += dd * dd; }
    elen2.push_back(l2);
  }
}

extern "C" {

int tacex_fem_create(int device_id, const tacex_fem_params* p, tacex_fem_ctx** out) {
  if (!p || !out || !p->rest_positions || !p->tets) { set_error("tacex_fem_create: null argument"); return 2; }
  const int V = p->num_verts, T = p->num_tets;
  if (V < 4 || T < 1) { set_error("tacex_fem_create: mesh too small (V=%d, T=%d)", V, T); return 2; }
  if (!(p->poisson > -1.0 && p->poisson < 0.5) || !(p->youngs > 0.0) || !(p->density > 0.0) || !(p->dt > 0.0)) {
    set_error("tacex_fem_create: need youngs > 0, -1 < poisson < 0.5, density > 0, dt > 0");
    return 2;
  }
  std::vector<int> tets((size_t)4 * T);
  std::vector<double> dminv((size_t)9 * T), vol(T), mass(V, 0.0);
  const double* X = p->rest_positions;
  for (int t = 0; t < T; ++t) {
    int v[4];
    for (int k = 0; k < 4; ++k) {
      v[k] = p->tets[t * 4 + k];
      if (v[k] < 0 || v[k] >= V) { set_error("tacex_fem_create: tet %d has vertex index %d out of range", t, v[k]); return 2; }
    }
    double Dm[9], det = 0.0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) Dm[i * 3 + k] = X[v[k + 1] * 3 + i] - X[v[0] * 3 + i];
      det = Dm[0] * (Dm[4] * Dm[8] - Dm[5] * Dm[7]) - Dm[1] * (Dm[3] * Dm[8] - Dm[5] * Dm[6]) + Dm[2] * (Dm[3] * Dm[7] - Dm[4] * Dm[6]);
      if (det > 0.0) break;
      int tmp = v[1]; v[1] = v[2]; v[2] = tmp;  // re-orient (same rule as the oracle)
    }
    if (!(det > 0.0)) { set_error("tacex_fem_create: tet %d is degenerate", t); return 2; }
    const double id = 1.0 / det;
    double inv[9] = {(Dm[4] * Dm[8] - Dm[5] * Dm[7]) * id, (Dm[2] * Dm[7] - Dm[1] * Dm[8]) * id, (Dm[1] * Dm[5] - Dm[2] * Dm[4]) * id,
                     (Dm[5] * Dm[6] - Dm[3] * Dm[8]) * id, (Dm[0] * Dm[8] - Dm[2] * Dm[6]) * id, (Dm[2] * Dm[3] - Dm[0] * Dm[5]) * id,
                     (Dm[3] * Dm[7] - Dm[4] * Dm[6]) * id, (Dm[1] * Dm[6] - Dm[0] * Dm[7]) * id, (Dm[0] * Dm[4] - Dm[1] * Dm[3]) * id};
    for (int k = 0; k < 9; ++k) dminv[(size_t)k * T + t] = inv[k];
    for (int k = 0; k < 4; ++k) tets[(size_t)k * T + t] = v[k];
    vol[t] = det / 6.0;
  }
  lumped_mass(p->density, tets, vol, T, mass.data());
  std::vector<int> off(V + 1, 0), idx((size_t)4 * T);
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < 4; ++k) off[tets[(size_t)k * T + t] + 1]++;
  for (int v = 0; v < V; ++v) off[v + 1] += off[v];
  {
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < 4; ++k) idx[cur[tets[(size_t)k * T + t]]++] = t * 4 + k;
  }
  hipError_t e = hipSetDevice(device_id);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  auto* c = new tacex_fem_ctx();
  c->device = device_id;
  c->tets_host = tets; c->vol_host = vol;
  FemDev& d = c->dev;
  d.V = V; d.T = T;
  {
    std::vector<double> rest(X, X + (size_t)3 * V);
    if (int rc0 = fem_upload(c, rest, &c->rest)) { tacex_fem_destroy(c); return rc0; }
  }
  int rc = fem_upload(c, tets, &d.tets) | fem_upload(c, dminv, &d.dminv) | fem_upload(c, vol, &d.vol) |
           fem_upload(c, mass, &d.mass) | fem_upload(c, off, &d.vt_off) | fem_upload(c, idx, &d.vt_idx);
  // Renumbered copy for the LDS Newton kernel.  Its per-window vertex gather waits, in every window, for the vertex with
  // the most incident tets IN THAT WINDOW; with a spatially coherent numbering all ~24 tets of a vertex sit in one or two
  // windows, so each of the 4 windows costs a full-valence gather (measured: 54 % of the kernel).  Dealing the tets out
  // round-robin spreads every vertex's tets evenly over the windows.
  {
    const int nwin = (T + kNwtChunk - 1) / kNwtChunk;
    std::vector<int> order;
    order.reserve(T);
    for (int w = 0; w < nwin; ++w)
      for (int t = w; t < T; t += nwin) order.push_back(t);
    std::vector<int> tets2((size_t)4 * T), off2(off), idx2((size_t)4 * T);
    std::vector<double> dminv2((size_t)9 * T), vol2(T);
    for (int n = 0; n < T; ++n) {
      const int t = order[n];
      for (int k = 0; k < 4; ++k) tets2[(size_t)k * T + n] = tets[(size_t)k * T + t];
      for (int k = 0; k < 9; ++k) dminv2[(size_t)k * T + n] = dminv[(size_t)k * T + t];
      vol2[n] = vol[t];
    }
    std::vector<int> cur(off.begin(), off.end() - 1);
    for (int n = 0; n < T; ++n)
      for (int k = 0; k < 4; ++k) idx2[cur[tets2[(size_t)k * T + n]]++] = n * 4 + k;
    std::vector<double> rec2((size_t)12 * T);
    for (int n = 0; n < T; ++n) {
      int ids[4];
      for (int k = 0; k < 4; ++k) ids[k] = tets2[(size_t)k * T + n];
      memcpy(&rec2[(size_t)n * 12], ids, sizeof(ids));  // 4 ints = the first two doubles of the record
      for (int k = 0; k < 9; ++k) rec2[(size_t)n * 12 + 2 + k] = dminv2[(size_t)k * T + n];
      rec2[(size_t)n * 12 + 11] = vol2[n];
    }
    const int nblk = (T + 63) / 64;
    std::vector<double> blk2((size_t)nblk * (kTetBlkBytes / 8), 0.0);
    for (int n = 0; n < T; ++n) {
      char* base = reinterpret_cast<char*>(blk2.data()) + (size_t)(n >> 6) * kTetBlkBytes;
      const int ln = n & 63;
      for (int k = 0; k < 9; ++k) memcpy(base + k * 512 + ln * 8, &dminv2[(size_t)k * T + n], 8);
      memcpy(base + 4608 + ln * 8, &vol2[n], 8);
      for (int k = 0; k < 4; ++k) memcpy(base + 5120 + k * 256 + ln * 4, &tets2[(size_t)k * T + n], 4);
    }
    rc |= fem_upload(c, blk2, &c->nwt.tet_blk) | fem_upload(c, tets2, &c->nwt.tets) | fem_upload(c, dminv2, &c->nwt.dminv) | fem_upload(c, vol2, &c->nwt.vol) |
          fem_upload(c, idx2, &c->nwt.vt_idx) | fem_upload(c, rec2, &c->nwt.tet_rec);
  }
  if (rc) { tacex_fem_destroy(c); return rc; }
  const GelConstants g = gel_constants(p->youngs, p->poisson);
  d.mu = g.mu; d.lam = g.lam; d.alpha = g.alpha; d.psi_rest = g.psi_rest;
  d.dt = p->dt;
  d.strength = p->constraint_strength_ratio;
  {
    double lo[3] = {X[0], X[1], X[2]}, hi[3] = {X[0], X[1], X[2]};
    for (int v = 1; v < V; ++v)
      for (int i = 0; i < 3; ++i) { lo[i] = fmin(lo[i], X[v * 3 + i]); hi[i] = fmax(hi[i], X[v * 3 + i]); }
    d.step_cap = sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
  }
  *out = c;
  return 0;
}

void tacex_fem_destroy(tacex_fem_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
}

size_t tacex_fem_workspace_bytes(const tacex_fem_ctx* c, int B) {
  if (!c || B <= 0) return 0;
  return StepLayout(c->dev.V, c->dev.T, B).total * sizeof(double);
}

int tacex_fem_element_terms(tacex_fem_ctx* c, const double* x, double* energy, double* grad, double* hess,
                            int project_psd, int B, void* stream) {
  if (!c || !x) { set_error("tacex_fem_element_terms: null argument"); return 2; }
  if (B <= 0) return 0;
  const bool mat = c->mat.n > 0;
  auto ke = (project_psd && hess) ? (mat ? fem_element_terms_kernel<true, true> : fem_element_terms_kernel<true, false>)
                                  : (mat ? fem_element_terms_kernel<false, true> : fem_element_terms_kernel<false, false>);
  hipLaunchKernelGGL(ke, dim3((c->dev.T + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, c->dev, x, energy, grad, hess, c->mat);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_element_terms_kernel");
}

int tacex_fem_energy(tacex_fem_ctx* c, const double* x, const double* xt, const uint8_t* cons, const double* aim,
                     double* E, void* ws, int B, void* stream) {
  (void)ws;
  if (!c || !x || !xt || !E) { set_error("tacex_fem_energy: null argument"); return 2; }
  if ((cons == nullptr) != (aim == nullptr)) { set_error("tacex_fem_energy: constrained_dev and aim_dev go together"); return 2; }
  if (B <= 0) return 0;
  hipLaunchKernelGGL(c->mat.n > 0 ? fem_energy_kernel<true> : fem_energy_kernel<false>, dim3(B), dim3(512), 0, (hipStream_t)stream, c->dev, x, xt, cons,
                     aim, E, c->mat);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_energy_kernel");
}

int tacex_fem_gradient(tacex_fem_ctx* c, const double* x, const double* xt, const uint8_t* cons, const double* aim,
                       double* g, void* ws, int B, void* stream) {
  if (!c || !x || !xt || !g || !ws) { set_error("tacex_fem_gradient: null argument"); return 2; }
  if ((cons == nullptr) != (aim == nullptr)) { set_error("tacex_fem_gradient: constrained_dev and aim_dev go together"); return 2; }
  if (B <= 0) return 0;
  hipLaunchKernelGGL(c->mat.n > 0 ? fem_gradient_kernel<true> : fem_gradient_kernel<false>, dim3(B), dim3(512), 0, (hipStream_t)stream, c->dev, x, xt,
                     cons, aim, g, static_cast<double*>(ws), c->mat);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_gradient_kernel");
}

int tacex_fem_set_contact(tacex_fem_ctx* c, const double* vertex_area_host, double d_hat, double stiffness, const double* indenters_dev) {
  if (!c) { set_error("tacex_fem_set_contact: null context"); return 2; }
  if (vertex_area_host) {
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    std::vector<double> a(vertex_area_host, vertex_area_host + c->dev.V);
    for (double v : a)
      if (!(v >= 0.0)) { set_error("tacex_fem_set_contact: vertex areas must be >= 0"); return 2; }
    const double* d = nullptr;
    if (int rc = fem_upload(c, a, &d)) return rc;
    bool synced = false;
    fem_release(c, c->dev.area, &synced);
    c->dev.area = d;
  }
  if (indenters_dev) {
    if (!c->dev.area) { set_error("tacex_fem_set_contact: vertex areas were never given"); return 2; }
    if (!(d_hat > 0.0) || !(stiffness > 0.0)) { set_error("tacex_fem_set_contact: need d_hat > 0 and stiffness > 0"); return 2; }
  }
  c->dev.dhat = d_hat;
  c->dev.kappa = stiffness;
  if (!indenters_dev || !c->dev.indenters) { c->ind_prev_ws = nullptr; c->ind_prev_B = 0; }  // contact off, or enabled for the first time:
                                                                                             // the next step sees no indenter motion
  c->dev.indenters = indenters_dev;
  return 0;
}

int tacex_fem_contact_gaps(tacex_fem_ctx* c, const double* x_dev, double* gaps_dev, int num_envs, void* stream) {
  if (!c || !x_dev || !gaps_dev) { set_error("tacex_fem_contact_gaps: null argument"); return 2; }
  if (num_envs <= 0) return 0;
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  hipLaunchKernelGGL(fem_contact_gaps_kernel, dim3(num_envs), dim3(256), 0, (hipStream_t)stream, c->dev, x_dev, gaps_dev);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_contact_gaps_kernel");
}

int tacex_fem_contact_forces(tacex_fem_ctx* c, const double* x_dev, const void* ws, const double* ref_points_dev, int with_friction,
                             double* wrench_dev, double* vertex_force_dev, int num_envs, void* stream) {
  if (!c || !x_dev || !wrench_dev) { set_error("tacex_fem_contact_forces: null argument"); return 2; }
  if (num_envs < 0) { set_error("tacex_fem_contact_forces: num_envs = %d", num_envs); return 2; }
  if (c->ball.nv > 0) {
    set_error("tacex_fem_contact_forces: not implemented for a scene with an affine body (tacex_fem_set_affine_body): its contacts are pairs, "
              "tacex_fem_ball_contact_forces reports them");
    return 2;
  }
  const int B = num_envs;
  const double *xprev = nullptr, *disp = nullptr, *ind_prev = nullptr;
  if (with_friction && c->dev.indenters) {  // (contact disabled: valid zeros, whatever else is set)
    if (c->fric_lag_mode != 1) {
      set_error("tacex_fem_contact_forces: friction is reported for IPC's lag only (tacex_fem_set_friction_lag mode 1): the reaction-capped "
                "lag depends on an iterate the step does not keep");
      return 2;
    }
    if (!ws) { set_error("tacex_fem_contact_forces: friction needs the step workspace (x_prev and the indenter displacement live there)"); return 2; }
    if (c->ind_prev_ws != ws || c->ind_prev_B != B) {
      set_error("tacex_fem_contact_forces: friction needs the workspace and num_envs of the context's last tacex_fem_step (num_envs %d, last step %d)",
                B, c->ind_prev_B);
      return 2;
    }
    const StepLayout lay(c->dev.V, c->dev.T, B);
    const double* base = static_cast<const double*>(ws);
    xprev = base + lay.x_prev; disp = base + lay.disp; ind_prev = base + lay.ind_prev;
  }
  if (B == 0) return 0;
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  hipLaunchKernelGGL(fem_contact_forces_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, c->dev, x_dev, xprev, disp, ind_prev, ref_points_dev,
                     wrench_dev, vertex_force_dev, c->mat);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_contact_forces_kernel");
}

int tacex_fem_set_deterministic(tacex_fem_ctx* c, int enable) {
  if (!c) { set_error("tacex_fem_set_deterministic: null context"); return 2; }
  c->deterministic = enable != 0;
  return 0;
}

int tacex_fem_set_contact_following(tacex_fem_ctx* c, int enable) {
  if (!c) { set_error("tacex_fem_set_contact_following: null context"); return 2; }
  c->follow_indenter = enable != 0;
  return 0;
}

int tacex_fem_set_friction(tacex_fem_ctx* c, double friction_ratio, double eps_velocity) {
  if (!c) { set_error("tacex_fem_set_friction: null context"); return 2; }
  if (!(friction_ratio >= 0.0) || (friction_ratio > 0.0 && !(eps_velocity > 0.0))) {
    set_error("tacex_fem_set_friction: need friction_ratio >= 0 and eps_velocity > 0");
    return 2;
  }
  c->fric_scene = friction_ratio;
  if (c->mat.n == 0) c->dev.fric_mu = friction_ratio;  // (with a material library: its largest ratio, set there)
  c->dev.fric_eps = eps_velocity * c->dev.dt;
  return 0;
}

int tacex_fem_set_line_search_refine(tacex_fem_ctx* c, int bisections) {
  if (!c || bisections < 0 || bisections > 15) { set_error("tacex_fem_set_line_search_refine: need a context and 0 <= bisections <= 15"); return 2; }
  c->ls_refine = bisections;
  return 0;
}

int tacex_fem_set_friction_lag(tacex_fem_ctx* c, int mode) {
  if (!c) { set_error("tacex_fem_set_friction_lag: null context"); return 2; }
  if (mode != 0 && mode != 1) { set_error("tacex_fem_set_friction_lag: mode must be 0 (reaction-capped lag at the step's start) or 1 (IPC: previous configuration)"); return 2; }
  c->fric_lag_mode = mode;
  return 0;
}

int tacex_fem_newton_resident(const tacex_fem_ctx* c) { return c ? c->last_resident : -1; }

int tacex_fem_newton_route(const tacex_fem_ctx* c, int* threads, int* lds_mode) {
  if (!c || !threads || !lds_mode) { set_error("tacex_fem_newton_route: null argument"); return 2; }
  *threads = c->last_threads;
  *lds_mode = c->last_lds_mode;
  return 0;
}

// One mesh's tables for the library: triangles in Morton order of their centroids (10 bits per axis over the mesh's bounding box),
// 16 consecutive ones form a cluster.  Appended to tri / bs / cl: a mesh's slice is the same whatever else the library holds.
static int pack_indenter_mesh(const char* who, int num_verts, const double* verts_host, int num_tris, const int32_t* tris_host,
                              std::vector<double>& tri, std::vector<double>& bs, std::vector<double>& cl) {
  if (num_verts < 3 || num_tris < 1 || !verts_host || !tris_host) { set_error("%s: bad arguments", who); return 2; }
  for (int k = 0; k < num_tris * 3; ++k)
    if (tris_host[k] < 0 || tris_host[k] >= num_verts) { set_error("%s: vertex index %d out of range", who, tris_host[k]); return 2; }
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int i = 0; i < num_verts; ++i)
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], verts_host[(size_t)i * 3 + k]); hi[k] = fmax(hi[k], verts_host[(size_t)i * 3 + k]); }
  std::vector<std::pair<uint32_t, int>> order(num_tris);
  for (int t = 0; t < num_tris; ++t) {
    uint32_t code = 0;
    for (int k = 0; k < 3; ++k) {
      double cen = 0.0;
      for (int j = 0; j < 3; ++j) cen += verts_host[(size_t)tris_host[(size_t)t * 3 + j] * 3 + k] / 3.0;
      const double ext = hi[k] - lo[k];
      uint32_t q = ext > 0.0 ? (uint32_t)fmin(1023.0, fmax(0.0, (cen - lo[k]) / ext * 1024.0)) : 0u;
      for (int bit = 0; bit < 10; ++bit) code |= ((q >> bit) & 1u) << (3 * bit + k);
    }
    order[t] = {code, t};
  }
  std::sort(order.begin(), order.end());
  const int ncl = (num_tris + kMeshCluster - 1) / kMeshCluster;
  const size_t tb = tri.size() / 9, cb = cl.size() / 4;  // this mesh's first triangle / cluster in the library
  tri.resize((tb + num_tris) * 9); bs.resize((tb + num_tris) * 4); cl.resize((cb + ncl) * 4);
  double* tr = tri.data() + tb * 9;
  double* bsp = bs.data() + tb * 4;
  double* clp = cl.data() + cb * 4;
  for (int s = 0; s < num_tris; ++s) {
    const int t = order[s].second;
    const double* v[3];
    for (int k = 0; k < 3; ++k) v[k] = verts_host + (size_t)tris_host[(size_t)t * 3 + k] * 3;
    double cen[3];
    for (int k = 0; k < 3; ++k) {
      tr[(size_t)s * 9 + k] = v[0][k];
      tr[(size_t)s * 9 + 3 + k] = v[1][k] - v[0][k];
      tr[(size_t)s * 9 + 6 + k] = v[2][k] - v[0][k];
      cen[k] = (v[0][k] + v[1][k] + v[2][k]) / 3.0;
      bsp[(size_t)s * 4 + k] = cen[k];
    }
    double r = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double d0 = v[j][0] - cen[0], d1 = v[j][1] - cen[1], d2 = v[j][2] - cen[2];
      r = fmax(r, sqrt(d0 * d0 + d1 * d1 + d2 * d2));
    }
    bsp[(size_t)s * 4 + 3] = r * (1.0 + 1e-12);
  }
  for (int q = 0; q < ncl; ++q) {
    const int s0 = q * kMeshCluster, s1 = std::min(num_tris, s0 + kMeshCluster);
    double cen[3] = {0, 0, 0};
    for (int s = s0; s < s1; ++s)
      for (int k = 0; k < 3; ++k) cen[k] += bsp[(size_t)s * 4 + k] / (s1 - s0);
    double r = 0.0;
    for (int s = s0; s < s1; ++s) {
      const double d0 = bsp[(size_t)s * 4] - cen[0], d1 = bsp[(size_t)s * 4 + 1] - cen[1], d2 = bsp[(size_t)s * 4 + 2] - cen[2];
      r = fmax(r, sqrt(d0 * d0 + d1 * d1 + d2 * d2) + bsp[(size_t)s * 4 + 3]);
    }
    for (int k = 0; k < 3; ++k) clp[(size_t)q * 4 + k] = cen[k];
    clp[(size_t)q * 4 + 3] = r * (1.0 + 1e-12);
  }
  return 0;
}

// replaces the library (num_meshes = 0: removes it); the per-env id array stays the caller's
static int set_indenter_library(tacex_fem_ctx* c, const char* who, int num_meshes, const int32_t* vert_counts, const double* verts_host,
                                const int32_t* tri_counts, const int32_t* tris_host) {
  if (num_meshes < 0 || (num_meshes > 0 && (!vert_counts || !verts_host || !tri_counts || !tris_host))) {
    set_error("%s: bad arguments", who);
    return 2;
  }
  std::vector<double> tri, bs, cl;
  std::vector<int> off((size_t)4 * num_meshes, 0);
  const double* vp = verts_host;
  const int32_t* tp = tris_host;
  for (int k = 0; k < num_meshes; ++k) {
    off[(size_t)4 * k] = (int)(tri.size() / 9);   // (first triangle | first cluster for now: offsets into im_lib below)
    off[(size_t)4 * k + 2] = (int)(cl.size() / 4);
    off[(size_t)4 * k + 3] = tri_counts[k];
    if (int rc = pack_indenter_mesh(who, vert_counts[k], vp, tri_counts[k], tp, tri, bs, cl)) {
      if (num_meshes > 1) {
        const std::string why = tacex_last_error();
        set_error("mesh %d: %s", k, why.c_str());
      }
      return rc;
    }
    if ((tri.size() + bs.size() + cl.size()) >= (size_t)1 << 31) { set_error("%s: library of more than 2^31 doubles", who); return 2; }
    vp += (size_t)vert_counts[k] * 3;
    tp += (size_t)tri_counts[k] * 3;
  }
  // im_lib = triangles | spheres | clusters, every region starting on a multiple of 4 doubles (the sphere tables are read as 32-byte vectors)
  const size_t nt = tri.size() / 9;
  const size_t bs0 = (tri.size() + 3) & ~(size_t)3, cl0 = bs0 + bs.size();
  std::vector<double> lib(cl0 + cl.size(), 0.0);
  std::copy(tri.begin(), tri.end(), lib.begin());
  std::copy(bs.begin(), bs.end(), lib.begin() + (long)bs0);
  std::copy(cl.begin(), cl.end(), lib.begin() + (long)cl0);
  for (int k = 0; k < num_meshes; ++k) {
    const size_t t0 = (size_t)off[(size_t)4 * k], c0 = (size_t)off[(size_t)4 * k + 2];
    off[(size_t)4 * k] = (int)(t0 * 9);
    off[(size_t)4 * k + 1] = (int)(bs0 + t0 * 4);
    off[(size_t)4 * k + 2] = (int)(cl0 + c0 * 4);
  }
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  FemDev& d = c->dev;
  {
    bool synced = false;
    fem_release(c, d.im_lib, &synced); fem_release(c, d.im_off, &synced);
    d.im_nt = d.im_nm = 0;
  }
  if (num_meshes > 0) {
    if (int rc = fem_upload(c, lib, &d.im_lib) | fem_upload(c, off, &d.im_off)) return rc;
    d.im_nt = (int)nt;
    d.im_nm = num_meshes;
  }
  return 0;
}

int tacex_fem_set_indenter_mesh(tacex_fem_ctx* c, int num_verts, const double* verts_host, int num_tris, const int32_t* tris_host) {
  if (!c) { set_error("tacex_fem_set_indenter_mesh: null context"); return 2; }
  // a library of one, shared by every env
  if (num_tris != 0 && (num_verts < 3 || num_tris < 1 || !verts_host || !tris_host)) { set_error("tacex_fem_set_indenter_mesh: bad arguments"); return 2; }
  const int32_t nv = num_verts, nt = num_tris;
  const int rc = set_indenter_library(c, "tacex_fem_set_indenter_mesh", num_tris == 0 ? 0 : 1, &nv, verts_host, &nt, tris_host);
  if (rc == 0) c->dev.im_ids = nullptr;
  return rc;
}

int tacex_fem_set_indenter_mesh_library(tacex_fem_ctx* c, int num_meshes, const int32_t* vert_counts, const double* verts_host,
                                        const int32_t* tri_counts, const int32_t* tris_host) {
  if (!c) { set_error("tacex_fem_set_indenter_mesh_library: null context"); return 2; }
  return set_indenter_library(c, "tacex_fem_set_indenter_mesh_library", num_meshes, vert_counts, verts_host, tri_counts, tris_host);
}

int tacex_fem_set_indenter_mesh_ids(tacex_fem_ctx* c, const int32_t* ids_dev) {
  if (!c) { set_error("tacex_fem_set_indenter_mesh_ids: null context"); return 2; }
  c->dev.im_ids = ids_dev;
  return 0;
}

// ---- gel material library -----------------------------------------------------------------------------------------------------------
int tacex_fem_set_material_library(tacex_fem_ctx* c, int num_materials, const double* youngs, const double* poisson, const double* density,
                                   const double* friction_ratio) {
  if (!c) { set_error("tacex_fem_set_material_library: null context"); return 2; }
  if (num_materials < 0 || (num_materials > 0 && (!youngs || !poisson || !density || !friction_ratio))) {
    set_error("tacex_fem_set_material_library: bad arguments (num_materials = %d)", num_materials);
    return 2;
  }
  if (num_materials > 0 && c->ball.nv > 0) {
    set_error("tacex_fem_set_material_library: not implemented for a scene with an affine body (tacex_fem_set_affine_body)");
    return 2;
  }
  const int V = c->dev.V, T = c->dev.T;
  const size_t stride = (size_t)kMatHead + V;
  std::vector<double> lib(stride * num_materials, 0.0);
  double fmax_ = 0.0;
  for (int k = 0; k < num_materials; ++k) {
    if (!(poisson[k] > -1.0 && poisson[k] < 0.5) || !(youngs[k] > 0.0) || !(density[k] > 0.0) || !(friction_ratio[k] >= 0.0)) {
      set_error("tacex_fem_set_material_library: material %d needs youngs > 0, -1 < poisson < 0.5, density > 0, friction_ratio >= 0", k);
      return 2;
    }
    double* rec = lib.data() + stride * k;
    const GelConstants g = gel_constants(youngs[k], poisson[k]);
    rec[0] = g.mu; rec[1] = g.lam; rec[2] = g.alpha; rec[3] = g.psi_rest;
    rec[4] = friction_ratio[k];
    lumped_mass(density[k], c->tets_host, c->vol_host, T, rec + kMatHead);
    fmax_ = fmax(fmax_, friction_ratio[k]);
  }
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  FemDev& d = c->dev;
  {
    // (the per-material coarse inverses belong to the library they were built for: they go with it)
    bool synced = false;
    fem_release(c, c->mat.lib, &synced); fem_release(c, c->mat.ac, &synced);
    c->mat.n = 0;
    d.fric_mu = c->fric_scene;
  }
  if (num_materials > 0) {
    if (int rc = fem_upload(c, lib, &c->mat.lib)) return rc;
    c->mat.n = num_materials;
    d.fric_mu = fmax_;  // sizes the friction state of the Newton kernels; an env's own ratio comes from its material
  }
  return 0;
}

int tacex_fem_set_material_ids(tacex_fem_ctx* c, const int32_t* ids_dev) {
  if (!c) { set_error("tacex_fem_set_material_ids: null context"); return 2; }
  c->mat.ids = ids_dev;
  return 0;
}

int tacex_fem_set_material_coarse_inverses(tacex_fem_ctx* c, int num_materials, const double* coarse_inverses_host) {
  if (!c) { set_error("tacex_fem_set_material_coarse_inverses: null context"); return 2; }
  FemDev& d = c->dev;
  if (num_materials != 0 && (num_materials != c->mat.n || !coarse_inverses_host || d.nc <= 0)) {
    set_error("tacex_fem_set_material_coarse_inverses: need one inverse per material of the library (%d), got %d, and a coarse space (nc = %d)", c->mat.n,
              num_materials, d.nc);
    return 2;
  }
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  bool synced = false;
  fem_release(c, c->mat.ac, &synced);
  if (num_materials == 0) return 0;
  std::vector<double> ai(coarse_inverses_host, coarse_inverses_host + (size_t)num_materials * 9 * d.nc * d.nc);
  return fem_upload(c, ai, &c->mat.ac);
}

int tacex_fem_set_chains(tacex_fem_ctx* c, int num_chains, const int32_t* chain_offsets_host, const int32_t* chain_vertices_host) {
  if (!c) { set_error("tacex_fem_set_chains: null context"); return 2; }
  FemDev& d = c->dev;
  auto drop_chains = [&]() {
    bool synced = false;
    (void)hipSetDevice(c->device);
    fem_release(c, d.ch_head, &synced); fem_release(c, d.ch_next, &synced); fem_release(c, d.ch_prev, &synced);
    d.nch = 0;
  };
  if (num_chains == 0) {  // every vertex its own chain: 3x3 block Jacobi
    drop_chains();
    return 0;
  }
  if (num_chains < 0 || !chain_offsets_host || !chain_vertices_host) { set_error("tacex_fem_set_chains: bad arguments"); return 2; }
  const int V = d.V;
  std::vector<int> nxt(V, -1), prv(V, -1), head;
  std::vector<char> member(V, 0);
  for (int ci = 0; ci < num_chains; ++ci) {
    const int a = chain_offsets_host[ci], b = chain_offsets_host[ci + 1];
    if (a < 0 || b < a) { set_error("tacex_fem_set_chains: offsets must ascend"); return 2; }
    for (int k = a; k < b; ++k) {
      const int v = chain_vertices_host[k];
      if (v < 0 || v >= V || member[v]) { set_error("tacex_fem_set_chains: vertex %d out of range or in two chains", v); return 2; }
      member[v] = 1;
      if (k > a) { nxt[chain_vertices_host[k - 1]] = v; prv[v] = chain_vertices_host[k - 1]; }
    }
    if (b > a) head.push_back(chain_vertices_host[a]);
  }
  for (int v = 0; v < V; ++v)
    if (!member[v]) head.push_back(v);  // the rest are chains of one vertex
  std::sort(head.begin(), head.end());
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  drop_chains();
  if (int rc = fem_upload(c, head, &d.ch_head) | fem_upload(c, nxt, &d.ch_next) | fem_upload(c, prv, &d.ch_prev)) return rc;
  d.nch = (int)head.size();
  return 0;
}

int tacex_fem_set_coarse_space(tacex_fem_ctx* c, int num_coarse, const int32_t* vertex_nodes_host, const double* vertex_weights_host,
                               const double* coarse_inverse_host) {
  if (!c) { set_error("tacex_fem_set_coarse_space: null context"); return 2; }
  auto drop_coarse = [&]() {
    bool synced = false;
    (void)hipSetDevice(c->device);
    FemDev& d0 = c->dev;
    fem_release(c, d0.cv_node, &synced); fem_release(c, d0.cv_w, &synced); fem_release(c, d0.cn_off, &synced);
    fem_release(c, d0.cn_vtx, &synced); fem_release(c, d0.cn_w, &synced); fem_release(c, d0.ac_inv, &synced);
    fem_release(c, c->mat.ac, &synced);  // (the per-material inverses were built for the space that goes: tacex_fem_set_material_coarse_inverses again)
    d0.nc = 0;
  };
  if (num_coarse == 0) {  // block Jacobi alone
    drop_coarse();
    return 0;
  }
  if (num_coarse < 1 || num_coarse > kFemMaxCoarse || !vertex_nodes_host || !vertex_weights_host || !coarse_inverse_host) {
    set_error("tacex_fem_set_coarse_space: need 1 <= num_coarse <= %d and non-null tables", kFemMaxCoarse);
    return 2;
  }
  const int V = c->dev.V, nc = num_coarse;
  std::vector<int> node(vertex_nodes_host, vertex_nodes_host + (size_t)V * 8);
  std::vector<double> w(vertex_weights_host, vertex_weights_host + (size_t)V * 8);
  for (size_t i = 0; i < node.size(); ++i)
    if (node[i] < 0 || node[i] >= nc || !(w[i] >= 0.0)) { set_error("tacex_fem_set_coarse_space: bad (node, weight) entry %zu", i); return 2; }
  // coarse node -> support (vertex, weight), zero weights dropped, vertices ascending (fixed summation order)
  std::vector<int> off(nc + 1, 0), vtx;
  std::vector<double> cw;
  for (int n = 0; n < nc; ++n) {
    for (int v = 0; v < V; ++v) {
      double ws = 0.0;
      for (int k = 0; k < 8; ++k)
        if (node[(size_t)v * 8 + k] == n) ws += w[(size_t)v * 8 + k];
      if (ws > 0.0) { vtx.push_back(v); cw.push_back(ws); }
    }
    off[n + 1] = (int)vtx.size();
  }
  std::vector<double> ai(coarse_inverse_host, coarse_inverse_host + (size_t)9 * nc * nc);
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  FemDev& d = c->dev;
  drop_coarse();
  if (int rc = fem_upload(c, node, &d.cv_node) | fem_upload(c, w, &d.cv_w) | fem_upload(c, off, &d.cn_off) | fem_upload(c, vtx, &d.cn_vtx) |
               fem_upload(c, cw, &d.cn_w) | fem_upload(c, ai, &d.ac_inv))
    return rc;
  d.nc = nc;
  return 0;
}

int tacex_fem_set_newton_early_exit(tacex_fem_ctx* c, double* dx_dev, double dx_tol) {
  if (!c) { set_error("tacex_fem_set_newton_early_exit: null context"); return 2; }
  c->dx_dev = dx_dev;
  c->dx_tol = dx_dev ? dx_tol : 0.0;
  return 0;
}

// elastic preconditioner blocks of all envs at x -> blk (B,V,16); dx_dev / dx_tol: envs already converged are skipped.  THE launch of
// fem_assemble_blocks_kernel: tacex_fem_ball_step comes here too (its blk region, no dx, tolerance 0)
static int launch_assemble(tacex_fem_ctx* c, const double* x, double* blk, int B, const double* dx_dev, double dx_tol, hipStream_t st, bool atom) {
  // TACEX_FEM_ASSEMBLE: 1 = tet-centric with LDS atomics, 0 = vertex-centric in a fixed order (A/B hook; default: follows the atomics switch)
  static const int asm_env = getenv("TACEX_FEM_ASSEMBLE") ? atoi(getenv("TACEX_FEM_ASSEMBLE")) : -1;
  const bool asm_atom = asm_env < 0 ? atom : (asm_env != 0 && !c->deterministic);
  const int V = c->dev.V;
  const size_t lds_a = ((size_t)3 * V + (asm_atom ? (size_t)15 * V : 0)) * sizeof(double);
  const bool mat = c->mat.n > 0;
  const auto ra = asm_atom ? (mat ? route<fem_assemble_blocks_kernel<true, true>>() : route<fem_assemble_blocks_kernel<true, false>>())
                           : (mat ? route<fem_assemble_blocks_kernel<false, true>>() : route<fem_assemble_blocks_kernel<false, false>>());
  hipError_t ea = ensure_dynamic_lds(ra.id(), lds_a, ra.lds->granted);
  if (ea != hipSuccess) return fail_hip(ea, "hipFuncSetAttribute(fem_assemble_blocks_kernel)");
  hipLaunchKernelGGL(ra.kern, dim3(B), dim3(512), lds_a, st, newton_dev(c), x, blk, dx_dev, dx_tol, c->mat);
  ea = hipGetLastError();
  return ea == hipSuccess ? 0 : fail_hip(ea, "fem_assemble_blocks_kernel");
}

// The twelve instantiations of fem_newton_lds_kernel: 256 and 768 threads exist in the atomic flavour with analytic indenters only
// (launch_newton picks nt accordingly), 512 threads in all four (mesh, atom) flavours; each with and without the material library.
using NewtonLdsRoute = Route<decltype(&fem_newton_lds_kernel<false, true, 512, false>)>;
static NewtonLdsRoute newton_lds_route(bool mesh, bool atom, int nt, bool mat) {
  auto pick = [&](auto with_mat) -> NewtonLdsRoute {
    constexpr bool MAT = decltype(with_mat)::value;
    if (nt == 256) return route<fem_newton_lds_kernel<false, true, 256, MAT>>();
    if (nt == 768) return route<fem_newton_lds_kernel<false, true, 768, MAT>>();
    if (mesh) return atom ? route<fem_newton_lds_kernel<true, true, 512, MAT>>() : route<fem_newton_lds_kernel<true, false, 512, MAT>>();
    return atom ? route<fem_newton_lds_kernel<false, true, 512, MAT>>() : route<fem_newton_lds_kernel<false, false, 512, MAT>>();
  };
  return mat ? pick(std::true_type{}) : pick(std::false_type{});
}

// one launch of the Newton kernel: up to max_newton iterations per env inside the CU-resident kernel, one iteration of the
// streaming fallback (mesh with more vertices than a workgroup has threads; TACEX_FEM_NEWTON_LDS=0)
static int launch_newton(tacex_fem_ctx* c, double* x, const double* xt, const uint8_t* cons, const double* aim, double* stats, void* ws,
                         int B, int pcg_max_iter, double pcg_tol_rate, int ls_max_iter, double* dx_dev, double dx_tol, int max_newton,
                         double* step_info, hipStream_t st, bool* resident, const double* xprev = nullptr, const double* disp = nullptr,
                         const int* env_order = nullptr, bool stream_accumulate = false) {
  static const int use_lds = getenv("TACEX_FEM_NEWTON_LDS") ? atoi(getenv("TACEX_FEM_NEWTON_LDS")) : 1;
  const bool fric = xprev && disp && c->dev.indenters && c->dev.fric_mu > 0.0;
  const bool mesh = c->dev.indenters && c->dev.im_nt > 0;  // the mesh-capable instantiation only when a mesh indenter exists
  static const int env_atomic = getenv("TACEX_FEM_ATOMIC") ? atoi(getenv("TACEX_FEM_ATOMIC")) : 1;  // A/B hook
  const bool atom = env_atomic != 0 && !c->deterministic;
  static const int fric_lag_at_start = getenv("TACEX_FEM_FRIC_LAG") ? atoi(getenv("TACEX_FEM_FRIC_LAG")) : 1;  // A/B hook: 0 = lag where this step's normal contact converged
  // threads per env: one per vertex, in steps of four waves (nwt_window_doubles); the wide variants are atomic-only and take analytic
  // indenters only (a mesh indenter or the deterministic switch on a mesh of more than 512 vertices: streaming kernel below)
  const int V = c->dev.V;
  // Meshes of <= 256 vertices run on 256 threads (round 6): ONE wave per SIMD with the whole 512-register file per lane (256 VGPRs + 74 AGPRs,
  // ScratchSize 0) against two waves per SIMD and 356 B/lane of scratch on 512 threads - measured on a 210-vertex / 720-tet pad, same
  // box, alternating: 0.248 / 0.249 against 0.294 / 0.290 ms per step of 512 envs (-15 %), 0.145 / 0.151 against 0.178 / 0.174 at 256
  // envs (profiles/r06_experiments.md section 3).  TACEX_FEM_NT256=0 keeps 512 threads (A/B).  The C4 pad (495 vertices) cannot run
  // it: a thread OWNS a vertex.
  static const int nt256 = getenv("TACEX_FEM_NT256") ? atoi(getenv("TACEX_FEM_NT256")) : 1;
  const int nt = (nt256 && V <= 256 && atom && !mesh) ? 256 : (V <= 512 ? 512 : 768);
  const size_t lds = nwt_lds_bytes(V, c->dev.T, fric, nt);
  hipError_t ea = hipSetDevice(c->device);  // (the LDS limits and opt-ins below are per device)
  if (ea != hipSuccess) return fail_hip(ea, "hipSetDevice");
  const bool mat = c->mat.n > 0;  // the material-library instantiations only when a library has been set
  NewtonLdsRoute rk;  // (kern == nullptr: the streaming kernel below)
  if (use_lds && V <= 768 && (nt <= 512 ? 4 * c->dev.T < 65535 : (atom && !mesh))) {
    rk = newton_lds_route(mesh, atom, nt, mat);
    // the env's state must fit next to the kernel's static __shared__; a pad that does not (e.g. 750 vertices on 768 threads) streams
    size_t limit = 0;
    ea = dynamic_lds_limit(rk.id(), rk.lds->avail, &limit);
    if (ea != hipSuccess) return fail_hip(ea, "hipFuncGetAttributes(fem_newton_lds_kernel)");
    if (lds > limit) rk = {};
  }
  if (rk.kern) {
    if (resident) *resident = true;
    c->last_resident = 1;
    c->last_threads = nt;
    c->last_lds_mode = -1;
    ea = ensure_dynamic_lds(rk.id(), lds, rk.lds->granted);
    if (ea != hipSuccess) return fail_hip(ea, "hipFuncSetAttribute(fem_newton_lds_kernel)");
    // elastic preconditioner blocks of all envs at the state this launch starts from -> workspace ((V,16) per env)
    if (int rc = launch_assemble(c, x, static_cast<double*>(ws), B, dx_dev, dx_tol, st, atom)) return rc;
    hipLaunchKernelGGL(rk.kern, dim3(B), dim3(nt), lds, st, newton_dev(c), x, xt, cons, aim, stats, pcg_max_iter,
                       pcg_tol_rate, ls_max_iter, dx_dev, dx_tol, max_newton, step_info, fric ? xprev : nullptr,
                       (xprev && disp && c->dev.indenters) ? disp : nullptr, env_order,
                       (c->follow_indenter ? 1 : 0) | ((fric_lag_at_start || c->fric_lag_mode == 1) ? 2 : 0) | (c->fric_lag_mode == 1 ? 4 : 0),
                       static_cast<double*>(ws), c->mat);  // env blocks of the workspace: (V,16) elastic preconditioner blocks per env
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail_hip(e, "fem_newton_lds_kernel");
  }
  if (resident) *resident = false;
  c->last_resident = 0;
  // x, p and the H.p accumulators in LDS when the summation order is free (atomic mode) and they fit next to the kernel's static
  // __shared__ (9 V doubles: ~2 200 vertices); all PCG vectors when 21 V doubles fit (~950 vertices); else global memory
  static const int stream_lds = getenv("TACEX_FEM_STREAM_LDS") ? atoi(getenv("TACEX_FEM_STREAM_LDS")) : 2;  // A/B hook: 0 none, 1 x / p / accumulators, 2 all PCG vectors
  size_t limit_s = 0;
  const auto rs = mat ? route<fem_newton_kernel<true>>() : route<fem_newton_kernel<false>>();
  ea = dynamic_lds_limit(rs.id(), rs.lds->avail, &limit_s);
  if (ea != hipSuccess) return fail_hip(ea, "hipFuncGetAttributes(fem_newton_kernel)");
  const bool lds_all = stream_lds != 1 && (size_t)21 * V * sizeof(double) <= limit_s;  // (TACEX_FEM_STREAM_LDS=1: x, p, accumulators only)
  const size_t lds_s = (size_t)(lds_all ? 21 : 9) * V * sizeof(double);
  const bool lds_sweep = stream_lds != 0 && atom && lds_s <= limit_s;
  if (lds_sweep) {
    const hipError_t es = ensure_dynamic_lds(rs.id(), lds_s, rs.lds->granted);
    if (es != hipSuccess) return fail_hip(es, "hipFuncSetAttribute(fem_newton_kernel)");
  }
  c->last_threads = 512;
  c->last_lds_mode = lds_sweep ? (lds_all ? 2 : 1) : 0;
  hipLaunchKernelGGL(rs.kern, dim3(B), dim3(512), lds_sweep ? lds_s : 0, st, c->dev, x, xt, cons, aim, stats, static_cast<double*>(ws), pcg_max_iter,
                     pcg_tol_rate, ls_max_iter, dx_dev, dx_tol, step_info, stream_accumulate ? 1 : 0, fric ? xprev : nullptr, fric ? disp : nullptr,
                     c->fric_lag_mode == 1 ? 1 : 0, lds_sweep ? (lds_all ? 2 : 1) : 0, c->mat);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_newton_kernel");
}

int tacex_fem_newton_step(tacex_fem_ctx* c, double* x, const double* xt, const uint8_t* cons, const double* aim,
                          double* stats, void* ws, int B, int pcg_max_iter, double pcg_tol_rate, int ls_max_iter,
                          void* stream) {
  if (!c || !x || !xt || !stats || !ws) { set_error("tacex_fem_newton_step: null argument"); return 2; }
  if ((cons == nullptr) != (aim == nullptr)) { set_error("tacex_fem_newton_step: constrained_dev and aim_dev go together"); return 2; }
  if (pcg_max_iter < 1 || ls_max_iter < 0 || !(pcg_tol_rate > 0.0)) { set_error("tacex_fem_newton_step: bad solver parameters"); return 2; }
  if (B <= 0) return 0;
  return launch_newton(c, x, xt, cons, aim, stats, ws, B, pcg_max_iter, pcg_tol_rate, ls_max_iter, c->dx_dev, c->dx_tol, 1, nullptr,
                       (hipStream_t)stream, nullptr);
}

int tacex_fem_step(tacex_fem_ctx* c, double* x, double* v, double* xt, const uint8_t* cons, const double* aim, double* stats,
                   double* step_info, void* ws, int B, const double gravity[3], int max_newton, double velocity_tol, int pcg_max_iter,
                   double pcg_tol_rate, int ls_max_iter, void* stream) {
  if (!c || !x || !v || !xt || !stats || !step_info || !ws || !gravity) { set_error("tacex_fem_step: null argument"); return 2; }
  if ((cons == nullptr) != (aim == nullptr)) { set_error("tacex_fem_step: constrained_dev and aim_dev go together"); return 2; }
  if (max_newton < 1 || pcg_max_iter < 1 || ls_max_iter < 0 || !(pcg_tol_rate > 0.0) || !(velocity_tol >= 0.0)) {
    set_error("tacex_fem_step: bad solver parameters");
    return 2;
  }
  if (B <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int V = c->dev.V;
  const size_t n3 = (size_t)B * V * 3;
  const StepLayout lay(V, c->dev.T, B);
  double* const base = static_cast<double*>(ws);
  double* xprev = base + lay.x_prev;
  double* dx = base + lay.dx;      // (B,) max |d| per env: the device-side convergence state of this time step
  double* disp = base + lay.disp;  // (B,3) indenter displacement since the previous step | (B,3) indenter position of the previous step
  double* ind_prev = base + lay.ind_prev;
  const double* ind = c->dev.indenters;
  const double dt = c->dev.dt, tol = velocity_tol * dt;
  hipLaunchKernelGGL(fem_predict_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, x, v, xt, xprev, dx, n3, B, dt, gravity[0],
                     gravity[1], gravity[2], ind, ind_prev, disp, (ind && c->ind_prev_ws == ws && c->ind_prev_B == B) ? 1 : 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "fem_predict_kernel");
  // heaviest envs first (see fem_newton_lds_kernel): worth it once a CU gets more than one env; TACEX_FEM_ORDER=0 = index order (A/B)
  static const int use_order = getenv("TACEX_FEM_ORDER") ? atoi(getenv("TACEX_FEM_ORDER")) : 1;
  int* env_order = nullptr;
  if (use_order && B > 1) {
    env_order = reinterpret_cast<int*>(base + lay.env_order);
    hipLaunchKernelGGL(fem_env_order_kernel, dim3(1), dim3(1024), 0, st, step_info, B, env_order);
    e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "fem_env_order_kernel");
  }
  bool resident = false;
  if (int rc = launch_newton(c, x, xt, cons, aim, stats, ws, B, pcg_max_iter, pcg_tol_rate, ls_max_iter, dx, tol, max_newton, step_info, st,
                             &resident, xprev, disp, env_order))
    return rc;
  if (!resident) {
    // streaming fallback: one launch per Newton iteration on a FIXED schedule; converged envs return at once (dx protocol), so the
    // launches past convergence cost microseconds and nothing is read back.  The first launch (above) SET the env's step_info row,
    // these add their iteration / PCG counts and OR their flags into it (penetration, dead line search: check_step() sees them).
    for (int it = 1; it < max_newton; ++it)
      if (int rc = launch_newton(c, x, xt, cons, aim, stats, ws, B, pcg_max_iter, pcg_tol_rate, ls_max_iter, dx, tol, 1, step_info, st, nullptr,
                                 xprev, disp, nullptr, true))  // (xprev / disp: the friction terms of the later iterations; the lag stays the first launch's)
        return rc;
  }
  hipLaunchKernelGGL(fem_velocity_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, x, xprev, v, n3, 1.0 / dt, ind, ind_prev, B);
  if (ind) { c->ind_prev_ws = ws; c->ind_prev_B = B; }
  e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_velocity_kernel");
}

// ---- the reference's UIPC scene: free affine-body ball + ground (fem_ball.h) ---------------------------------------------------------
int tacex_fem_set_affine_body(tacex_fem_ctx* c, int num_verts, const double* verts_host, int num_tris, const int32_t* tris_host, double density,
                              double kappa, const double* pad_vertex_area_host, int num_pad_tris, const int32_t* pad_tris_host, double d_hat,
                              double stiffness, double ground_height, int enable_ground, int kinematic) {
  if (!c) { set_error("tacex_fem_set_affine_body: null context"); return 2; }
  if (num_verts != 0 && c->mat.n > 0) {
    set_error("tacex_fem_set_affine_body: not implemented for a scene with a material library (tacex_fem_set_material_library)");
    return 2;
  }
  bool synced = false;
  BallDev& bd = c->ball;
  fem_release(c, bd.Y, &synced); fem_release(c, bd.tri, &synced); fem_release(c, bd.area, &synced);
  fem_release(c, bd.ptri, &synced); fem_release(c, bd.psv, &synced); fem_release(c, bd.parea, &synced);
  fem_release(c, bd.pedge, &synced); fem_release(c, bd.pearea, &synced); fem_release(c, bd.pelen2, &synced);
  fem_release(c, bd.bedge, &synced); fem_release(c, bd.bearea, &synced); fem_release(c, bd.belen2, &synced);
  bd = BallDev{};
  c->ball_last_ws = nullptr; c->ball_last_B = 0;
  c->ball_step_ws = nullptr; c->ball_step_B = 0;
  if (num_verts == 0) return 0;  // remove the body
  if (!verts_host || !tris_host || !pad_vertex_area_host || !pad_tris_host || num_verts < 4 || num_tris < 4 || num_pad_tris < 1) {
    set_error("tacex_fem_set_affine_body: null / too small mesh argument");
    return 2;
  }
  if (num_verts >= 32768 || num_tris >= 32768 || num_pad_tris >= 32768 || c->dev.V >= 32768) {
    set_error("tacex_fem_set_affine_body: the pair list packs indices into 15 bits (meshes of < 32768 vertices / triangles)");
    return 2;
  }
  if (!(density > 0.0) || !(kappa > 0.0) || !(d_hat > 0.0) || !(stiffness > 0.0)) { set_error("tacex_fem_set_affine_body: bad material / contact parameters"); return 2; }
  const int V = c->dev.V;
  std::vector<double> Y((size_t)num_verts * 4), area(num_verts, 0.0), parea(pad_vertex_area_host, pad_vertex_area_host + V);
  std::vector<int> tri(tris_host, tris_host + (size_t)num_tris * 3), ptri(pad_tris_host, pad_tris_host + (size_t)num_pad_tris * 3), psv;
  for (int t : tri) if (t < 0 || t >= num_verts) { set_error("tacex_fem_set_affine_body: triangle index out of range"); return 2; }
  for (int t : ptri) if (t < 0 || t >= V) { set_error("tacex_fem_set_affine_body: pad triangle index out of range"); return 2; }
  for (int k = 0; k < num_verts; ++k) { Y[k * 4] = 1.0; for (int i = 0; i < 3; ++i) Y[k * 4 + 1 + i] = verts_host[k * 3 + i]; }
  // moments of the closed surface (signed tetrahedra against the origin), vertex areas - oracle/abd_oracle.py AffineBody
  double S[16] = {}, vol = 0.0;
  for (int t = 0; t < num_tris; ++t) {
    const double* a = verts_host + (size_t)tri[t * 3] * 3; const double* b = verts_host + (size_t)tri[t * 3 + 1] * 3; const double* cc = verts_host + (size_t)tri[t * 3 + 2] * 3;
    const double bc[3] = {b[1] * cc[2] - b[2] * cc[1], b[2] * cc[0] - b[0] * cc[2], b[0] * cc[1] - b[1] * cc[0]};
    const double v6 = (a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2]) / 6.0;
    vol += v6;
    S[0] += v6;
    const double sm[3] = {a[0] + b[0] + cc[0], a[1] + b[1] + cc[1], a[2] + b[2] + cc[2]};
    for (int i = 0; i < 3; ++i) {
      S[1 + i] += v6 * sm[i] / 4.0;
      for (int j = 0; j < 3; ++j) S[(1 + i) * 4 + 1 + j] += v6 / 20.0 * (a[i] * a[j] + b[i] * b[j] + cc[i] * cc[j] + sm[i] * sm[j]);
    }
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
    const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double ta = 0.5 * sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    for (int k = 0; k < 3; ++k) area[tri[t * 3 + k]] += ta / 3.0;
  }
  if (!(vol > 0.0)) { set_error("tacex_fem_set_affine_body: the surface triangles must be oriented outward (enclosed volume %g)", vol); return 2; }
  for (int i = 1; i < 4; ++i) S[i * 4] = S[i];
  for (int k = 0; k < 16; ++k) bd.S[k] = density * S[k];
  for (int v = 0; v < V; ++v) if (parea[v] > 0.0) psv.push_back(v);
  bd.nv = num_verts; bd.nt = num_tris; bd.npt = num_pad_tris; bd.nsv = (int)psv.size();
  bd.kv = kappa * vol; bd.gh = ground_height; bd.dhat = d_hat; bd.kappa = stiffness; bd.ground = enable_ground ? 1 : 0; bd.kinematic = kinematic ? 1 : 0;
  if (int rc = fem_upload(c, Y, &bd.Y)) return rc;
  if (int rc = fem_upload(c, tri, &bd.tri)) return rc;
  if (int rc = fem_upload(c, area, &bd.area)) return rc;
  if (int rc = fem_upload(c, ptri, &bd.ptri)) return rc;
  if (int rc = fem_upload(c, psv, &bd.psv)) return rc;
  if (int rc = fem_upload(c, parea, &bd.parea)) return rc;
  // edge-edge pairs: the unique edges of both surfaces (oracle/abd_oracle.py surface_edges); the pad's rest positions come back from the device
  {
    std::vector<double> rest((size_t)3 * V);
    hipError_t e = hipMemcpy(rest.data(), c->rest, rest.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(e, "hipMemcpy(pad rest positions)");
    std::vector<int> pe, be;
    std::vector<double> pa, pl, ba, bl;
    surface_edges(ptri, rest.data(), pe, pa, pl);
    surface_edges(tri, verts_host, be, ba, bl);
    if (pe.size() / 2 >= 32768 || be.size() / 2 >= 32768) { set_error("tacex_fem_set_affine_body: more than 32767 surface edges"); return 2; }
    bd.npe = (int)(pe.size() / 2); bd.nbe = (int)(be.size() / 2); bd.ee = 1;
    if (int rc = fem_upload(c, pe, &bd.pedge)) return rc;
    if (int rc = fem_upload(c, pa, &bd.pearea)) return rc;
    if (int rc = fem_upload(c, pl, &bd.pelen2)) return rc;
    if (int rc = fem_upload(c, be, &bd.bedge)) return rc;
    if (int rc = fem_upload(c, ba, &bd.bearea)) return rc;
    if (int rc = fem_upload(c, bl, &bd.belen2)) return rc;
  }
  return 0;
}

int tacex_fem_set_edge_edge(tacex_fem_ctx* c, int enable) {
  if (!c || c->ball.nv == 0) { set_error("tacex_fem_set_edge_edge: no affine body set"); return 2; }
  c->ball.ee = enable ? 1 : 0;
  return 0;
}

static BallLayout ball_layout(const tacex_fem_ctx* c, int B) { return BallLayout(c->dev.V, c->dev.T, c->ball.nv, c->ball.nt, B); }

size_t tacex_fem_ball_workspace_bytes(const tacex_fem_ctx* c, int B) {
  if (!c || B <= 0 || c->ball.nv == 0) return 0;
  return ball_layout(c, B).total * sizeof(double);
}

int tacex_fem_ball_moments(const tacex_fem_ctx* c, double moments_out[16], double* kappa_vol_out) {
  if (!c || c->ball.nv == 0 || !moments_out) { set_error("tacex_fem_ball_moments: no affine body set"); return 2; }
  for (int k = 0; k < 16; ++k) moments_out[k] = c->ball.S[k];
  if (kappa_vol_out) *kappa_vol_out = c->ball.kv;
  return 0;
}

// threads per env of fem_ball_newton_kernel: 512 (two waves per SIMD at 256 VGPRs: 358 of them spilled) or 256 (one wave per SIMD with the whole
// register file); TACEX_BALL_NT picks (A/B, profiles/r06_experiments.md section 13)
static int ball_threads() {
  static const int nt = getenv("TACEX_BALL_NT") ? atoi(getenv("TACEX_BALL_NT")) : 512;
  return nt == 256 ? 256 : 512;
}

// The ball kernel has no smaller LDS mode: a pad whose state does not fit next to the kernel's static __shared__ (18.8 KB at 512 threads:
// up to 696 vertices; 697 at 256 threads) is refused with this message before anything is launched.
static int ball_lds_ok(tacex_fem_ctx* c, const char* who) {
  const size_t lds = ball_lds_bytes(c->dev.V);
  const auto rb = ball_threads() == 256 ? route<fem_ball_newton_kernel<256>>() : route<fem_ball_newton_kernel<512>>();
  hipError_t e = hipSetDevice(c->device);
  size_t limit = 0;
  if (e == hipSuccess) e = dynamic_lds_limit(rb.id(), rb.lds->avail, &limit);
  if (e != hipSuccess) return fail_hip(e, "hipFuncGetAttributes(fem_ball_newton_kernel)");
  if (lds > limit) {
    set_error("%s: pad of %d vertices (x, p, accumulators and chain factors of one env must fit a CU's 160 KB of LDS: %zu B next to the kernel's "
              "%zu B of static LDS)", who, c->dev.V, lds, (size_t)160 * 1024 - limit);
    return 2;
  }
  e = ensure_dynamic_lds(rb.id(), lds, rb.lds->granted);
  return e == hipSuccess ? 0 : fail_hip(e, "hipFuncSetAttribute(fem_ball_newton_kernel)");
}

static int ball_args_ok(tacex_fem_ctx* c, const void* x, const void* q, const void* ws, const uint8_t* cons, const double* aim, const char* who) {
  if (!c || !x || !q || !ws) { set_error("%s: null argument", who); return 2; }
  if (c->ball.nv == 0) { set_error("%s: no affine body (tacex_fem_set_affine_body)", who); return 2; }
  if ((size_t)9 * c->dev.V > (size_t)12 * c->dev.T) { set_error("%s: mesh with more than 4/3 vertices per tet (the lagged blocks share a per-tet array)", who); return 2; }
  if ((cons == nullptr) != (aim == nullptr)) { set_error("%s: constrained_dev and aim_dev go together", who); return 2; }
  return 0;
}

int tacex_fem_ball_terms(tacex_fem_ctx* c, const double* x, const double* xt, const double* q, const double* qt, const uint8_t* cons, const double* aim,
                         const double* x_prev, const double* q_prev, double* energy, double* grad, double* step_info, void* ws, int B, void* stream) {
  if (int rc = ball_args_ok(c, x, q, ws, cons, aim, "tacex_fem_ball_terms")) return rc;
  if (!xt || !qt) { set_error("tacex_fem_ball_terms: null argument"); return 2; }
  if (B <= 0) return 0;
  if (int rc = ball_lds_ok(c, "tacex_fem_ball_terms")) return rc;
  auto kern = ball_threads() == 256 ? fem_ball_newton_kernel<256> : fem_ball_newton_kernel<512>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(ball_threads()), ball_lds_bytes(c->dev.V), (hipStream_t)stream, c->dev, c->ball, const_cast<double*>(x), xt,
                     const_cast<double*>(q), qt, cons, aim, static_cast<double*>(ws), 1, 1.0, 0, 1, 0.0, 0.0, step_info, 1, energy, grad,
                     (x_prev && q_prev) ? x_prev : nullptr, (x_prev && q_prev) ? q_prev : nullptr, static_cast<const int*>(nullptr),
                     static_cast<const double*>(nullptr));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_ball_newton_kernel(terms)");
}

// the (B,12) rows "q at the end of the previous step" of a ball workspace (see tacex_fem_ball_step)
static double* ball_qlast(const tacex_fem_ctx* c, void* ws, int B) { return static_cast<double*>(ws) + ball_layout(c, B).q_last; }

int tacex_fem_ball_step(tacex_fem_ctx* c, double* x, double* v, double* q, double* qv, const uint8_t* cons, const double* aim, double* step_info,
                        void* ws, int B, const double gravity[3], int max_newton, double velocity_tol, double transrate_tol, int pcg_max_iter,
                        double pcg_tol_rate, int ls_max_iter, void* stream) {
  if (int rc = ball_args_ok(c, x, q, ws, cons, aim, "tacex_fem_ball_step")) return rc;
  if (!v || !qv || !step_info || !gravity) { set_error("tacex_fem_ball_step: null argument"); return 2; }
  if (max_newton < 1 || pcg_max_iter < 1 || ls_max_iter < 0 || !(pcg_tol_rate > 0.0) || !(velocity_tol >= 0.0) || !(transrate_tol >= 0.0)) {
    set_error("tacex_fem_ball_step: bad solver parameters");
    return 2;
  }
  if (B <= 0) return 0;
  if (int rc = ball_lds_ok(c, "tacex_fem_ball_step")) return rc;  // (before the predictors: a refused step leaves x, v, q and qv as they were)
  c->last_threads = ball_threads();
  c->last_lds_mode = -1;
  static const int ball_coarse_off = getenv("TACEX_BALL_COARSE") ? (atoi(getenv("TACEX_BALL_COARSE")) == 0) : 0;  // A/B hook: block Jacobi alone on the pad rows
  hipStream_t st = (hipStream_t)stream;
  const int V = c->dev.V;
  const size_t n3 = (size_t)B * V * 3;
  const BallLayout lay = ball_layout(c, B);
  double* const base = static_cast<double*>(ws);
  double* xprev = base + lay.x_prev;
  double* qprev = base + lay.q_prev;
  double* xt = base + lay.xt;
  double* qt = base + lay.qt;
  // A KINEMATIC body is moved by the caller between steps: friction then slides relative to where the body stood at the END of the previous
  // step (kept here; the first step with this workspace sees no body motion), like the analytic indenters' displacement in tacex_fem_step
  double* qlast = base + lay.q_last;
  const bool have_last = c->ball.kinematic && c->ball_last_ws == ws && c->ball_last_B == B;
  const double dt = c->dev.dt;
  hipLaunchKernelGGL(fem_predict_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, x, v, xt, xprev, static_cast<double*>(nullptr), n3, B, dt,
                     gravity[0], gravity[1], gravity[2], static_cast<const double*>(nullptr), static_cast<double*>(nullptr), static_cast<double*>(nullptr), 0);
  hipLaunchKernelGGL(fem_ball_predict_kernel, dim3((unsigned)((B * 12 + 255) / 256)), dim3(256), 0, st, q, qv, qt, qprev, B, dt, gravity[0], gravity[1],
                     gravity[2]);
  int* env_order = nullptr;
  static const int use_order = getenv("TACEX_FEM_ORDER") ? atoi(getenv("TACEX_FEM_ORDER")) : 1;
  if (use_order && B > 256) {  // (step_info still holds the previous step's counts; a first step sorts zeros = index order)
    env_order = reinterpret_cast<int*>(base + lay.env_order);
    hipLaunchKernelGGL(fem_env_order_kernel, dim3(1), dim3(1024), 0, st, step_info, B, env_order);
  }
  // elastic preconditioner blocks D | E of every env at the state the step starts from (what fem_newton_lds_kernel's launch does too)
  double* blk = base + lay.blk;
  if (int rc = launch_assemble(c, x, blk, B, nullptr, 0.0, st, !c->deterministic)) return rc;  // (the device is current: ball_lds_ok)
  auto kern = ball_threads() == 256 ? fem_ball_newton_kernel<256> : fem_ball_newton_kernel<512>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(ball_threads()), ball_lds_bytes(c->dev.V), st, c->dev, c->ball, x, xt, q, qt, cons, aim, static_cast<double*>(ws), pcg_max_iter,
                     pcg_tol_rate, ls_max_iter, max_newton, velocity_tol * dt, transrate_tol * dt, step_info, (ball_coarse_off ? 2 : 0) | ((c->ls_refine & 15) << 8),
                     static_cast<double*>(nullptr), static_cast<double*>(nullptr), static_cast<const double*>(xprev),
                     static_cast<const double*>(have_last ? qlast : qprev), static_cast<const int*>(env_order), static_cast<const double*>(blk));
  hipLaunchKernelGGL(fem_velocity_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, x, xprev, v, n3, 1.0 / dt, static_cast<const double*>(nullptr),
                     static_cast<double*>(nullptr), B);
  hipLaunchKernelGGL(fem_ball_velocity_kernel, dim3((unsigned)((B * 12 + 255) / 256)), dim3(256), 0, st, q, qprev, qv, B, 1.0 / dt);
  if (c->ball.kinematic) {
    // the pose this step's friction slid the body rows from is kept for tacex_fem_ball_contact_forces in the q~ rows, which nothing reads
    // once the Newton kernel has ended (a kinematic body has no inertia term to predict for): no workspace region of its own
    (void)hipMemcpyAsync(qt, have_last ? qlast : qprev, (size_t)B * 12 * sizeof(double), hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(qlast, q, (size_t)B * 12 * sizeof(double), hipMemcpyDeviceToDevice, st);
    c->ball_last_ws = ws; c->ball_last_B = B;
  }
  c->ball_step_ws = ws; c->ball_step_B = B;
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "tacex_fem_ball_step");
}

int tacex_fem_ball_contact_forces(tacex_fem_ctx* c, const double* x_dev, const double* q_dev, const void* ws, const double* x_prev_dev,
                                  const double* q_prev_dev, const double* ref_points_dev, int with_friction, double* record_dev,
                                  double* vertex_force_dev, int num_envs, void* stream) {
  if (!c || !x_dev || !q_dev || !record_dev) { set_error("tacex_fem_ball_contact_forces: null argument"); return 2; }
  if (c->ball.nv == 0) { set_error("tacex_fem_ball_contact_forces: no affine body (tacex_fem_set_affine_body); tacex_fem_contact_forces covers prescribed indenters"); return 2; }
  if (num_envs < 0) { set_error("tacex_fem_ball_contact_forces: num_envs = %d", num_envs); return 2; }
  if ((x_prev_dev == nullptr) != (q_prev_dev == nullptr)) { set_error("tacex_fem_ball_contact_forces: x_prev_dev and q_prev_dev go together"); return 2; }
  const int B = num_envs;
  const double *xprev = nullptr, *qlag = nullptr, *qref = nullptr;
  if (with_friction && c->dev.fric_mu > 0.0) {  // (friction ratio 0: valid zeros, whatever else is set)
    if (x_prev_dev) {
      xprev = x_prev_dev; qlag = q_prev_dev; qref = q_prev_dev;
    } else {
      if (!ws || c->ball_step_ws != ws || c->ball_step_B != B) {
        set_error("tacex_fem_ball_contact_forces: friction needs x_prev_dev / q_prev_dev or the workspace and num_envs of the context's last "
                  "tacex_fem_ball_step (num_envs %d, last step %d)", B, c->ball_step_B);
        return 2;
      }
      const BallLayout lay = ball_layout(c, B);
      const double* base = static_cast<const double*>(ws);
      xprev = base + lay.x_prev; qlag = base + lay.q_prev;
      // the step's own rule for the body rows: a free body slides from where the step started; a kinematic one from where it stood at
      // the end of the step BEFORE the last one (what that step's friction measured the body's motion from: tacex_fem_ball_step leaves
      // it in the q~ rows; its first step with a workspace leaves q_prev there: no body motion)
      qref = c->ball.kinematic ? base + lay.qt : qlag;
    }
  }
  if (B == 0) return 0;
  const size_t lds = ball_force_lds_bytes(c->dev.V, c->ball.nv, vertex_force_dev != nullptr);
  if (lds > (size_t)40 * 1024) {
    set_error("tacex_fem_ball_contact_forces: body of %d vertices, pad of %d (the body's surface points%s are kept in 40 KB of LDS: %zu B)", c->ball.nv,
              c->dev.V, vertex_force_dev ? " and the per-vertex forces" : "", lds);
    return 2;
  }
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  hipLaunchKernelGGL(fem_ball_contact_forces_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, c->ball, c->dev.V, c->dev.fric_mu, c->dev.fric_eps,
                     x_dev, q_dev, xprev, qlag, qref, ref_points_dev, record_dev, vertex_force_dev);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_ball_contact_forces_kernel");
}

int tacex_fem_reset_envs(tacex_fem_ctx* c, const int32_t* env_ids, int num_reset, const double* positions, double* x, double* v,
                         double* step_info, void* ws, int B, void* stream) {
  if (!c || !x || !v) { set_error("tacex_fem_reset_envs: null argument"); return 2; }
  if (B <= 0 || num_reset == 0) return 0;
  if (num_reset < 0 || (!env_ids && num_reset != B)) { set_error("tacex_fem_reset_envs: without env_ids, num_reset must equal num_envs"); return 2; }
  const int V = c->dev.V;
  // the previous indenter positions live in the workspace the last tacex_fem_step ran with (see tacex_fem_step): another workspace or
  // env count means the next step has no previous positions at all
  double* ind_prev = nullptr;
  if (ws && c->dev.indenters && c->ind_prev_ws == ws && c->ind_prev_B == B)
    ind_prev = static_cast<double*>(ws) + StepLayout(V, c->dev.T, B).ind_prev;
  hipLaunchKernelGGL(fem_reset_envs_kernel, dim3(num_reset), dim3(256), 0, (hipStream_t)stream, env_ids, positions, c->rest, x, v, step_info,
                     ind_prev, V, B);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_reset_envs_kernel");
}

int tacex_fem_ball_reset_envs(tacex_fem_ctx* c, const int32_t* env_ids, int num_reset, const double* q0, double* q, double* qv, void* ws, int B,
                              void* stream) {
  if (!c || !q0 || !q || !qv) { set_error("tacex_fem_ball_reset_envs: null argument"); return 2; }
  if (c->ball.nv == 0) { set_error("tacex_fem_ball_reset_envs: no affine body (tacex_fem_set_affine_body)"); return 2; }
  if (B <= 0 || num_reset == 0) return 0;
  if (num_reset < 0 || (!env_ids && num_reset != B)) { set_error("tacex_fem_ball_reset_envs: without env_ids, num_reset must equal num_envs"); return 2; }
  // q and qv are (B,4,3): the pad's reset kernel with V = 4 and q0 as the rest positions
  hipLaunchKernelGGL(fem_reset_envs_kernel, dim3(num_reset), dim3(256), 0, (hipStream_t)stream, env_ids, static_cast<const double*>(nullptr), q0, q, qv,
                     static_cast<double*>(nullptr), static_cast<double*>(nullptr), 4, B);
  // a kinematic body's friction reference: the next step measures the body's motion from q0, not from where it stood before the reset
  // (the rows of the other envs stay valid)
  if (c->ball.kinematic && ws && c->ball_last_ws == ws && c->ball_last_B == B)
    hipLaunchKernelGGL(fem_reset_envs_kernel, dim3(num_reset), dim3(256), 0, (hipStream_t)stream, env_ids, static_cast<const double*>(nullptr), q0,
                       ball_qlast(c, ws, B), qv, static_cast<double*>(nullptr), static_cast<double*>(nullptr), 4, B);  // (qv: zeroed again)
  // the env's friction reference of tacex_fem_ball_contact_forces: none until it steps (the rows of the other envs stay valid)
  if (ws && c->ball_step_ws == ws && c->ball_step_B == B)
    hipLaunchKernelGGL(fem_ball_clear_friction_ref_kernel, dim3(num_reset), dim3(64), 0, (hipStream_t)stream, env_ids,
                       static_cast<double*>(ws) + ball_layout(c, B).q_prev, B);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_reset_envs_kernel(ball)");
}

int tacex_fem_set_attachment_targets(const float* body_pos, const float* body_quat, const float* offsets, const int32_t* idx,
                                     double* aim, uint8_t* constrained, double* aim_compact, int B, int A, int V, void* stream) {
  if (!body_pos || !body_quat || !offsets || !idx || !aim || !constrained) { set_error("tacex_fem_set_attachment_targets: null argument"); return 2; }
  if (B <= 0 || A <= 0) return 0;
  hipLaunchKernelGGL(fem_attachment_aim_kernel, dim3((A + 127) / 128, B), dim3(128), 0, (hipStream_t)stream, body_pos, body_quat,
                     offsets, idx, aim, constrained, aim_compact, A, V);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_attachment_aim_kernel");
}

int tacex_fem_marker_uv(const double* pos, const int32_t* tri, const double* wgt, double fx, double fy, double cx,
                        double cy, double* uv, int B, int Vs, int M, void* stream) {
  if (!pos || !tri || !wgt || !uv) { set_error("tacex_fem_marker_uv: null argument"); return 2; }
  if (B <= 0 || M <= 0) return 0;
  hipLaunchKernelGGL(fem_marker_uv_kernel, dim3((M + 127) / 128, B), dim3(128), 0, (hipStream_t)stream, pos, tri, wgt, fx, fy,
                     cx, cy, uv, Vs, M);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_marker_uv_kernel");
}

int tacex_fem_marker_flow(const double* x, const int64_t* surf_ids, const double* cam_pos, const double* cam_rot_inv, const int32_t* tri,
                          const double* wgt, double fx, double fy, double cx, double cy, const double* init_uv, const int64_t* select,
                          double normalize_div, double* curr_uv, double* flow, float* flow_f32, int B, int V, int M, int K, void* stream) {
  if (!x || !surf_ids || !cam_pos || !cam_rot_inv || !tri || !wgt || !init_uv || !select || (!flow && !flow_f32)) {
    set_error("tacex_fem_marker_flow: null argument");
    return 2;
  }
  if (B <= 0 || M <= 0 || K <= 0) return 0;
  if ((size_t)M * 2 * sizeof(double) > 64 * 1024) { set_error("tacex_fem_marker_flow: %d markers (the env's projections are staged in 64 KB of LDS)", M); return 2; }
  hipLaunchKernelGGL(fem_marker_flow_kernel, dim3(B), dim3(256), (size_t)M * 2 * sizeof(double), (hipStream_t)stream, x,
                     reinterpret_cast<const long long*>(surf_ids), cam_pos, cam_rot_inv, tri, wgt, fx, fy, cx, cy, init_uv,
                     reinterpret_cast<const long long*>(select), normalize_div, curr_uv, flow, flow_f32, V, M, K);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_marker_flow_kernel");
}

int tacex_fem_marker_flow_library(const double* x, const int64_t* surf_ids, const double* cam_pos, const double* cam_rot_inv,
                                  const double* ref_surf_cam, const int32_t* lib_tri, const double* lib_wgt, const int32_t* lib_count,
                                  int P, int Mmax, const int32_t* pattern_ids, uint32_t* draws, uint64_t seed, double fx, double fy, double cx,
                                  double cy, double lose_prob, double sigma, int img_h, int img_w, double normalize_div, double* curr_uv,
                                  double* flow, float* flow_f32, int32_t* num_tracked, int B, int V, int Vs, int K, void* stream) {
  if (!x || !surf_ids || !cam_pos || !cam_rot_inv || !ref_surf_cam || !lib_tri || !lib_wgt || !lib_count || !pattern_ids || !draws ||
      (!flow && !flow_f32)) {
    set_error("tacex_fem_marker_flow_library: null argument");
    return 2;
  }
  if (P < 1) { set_error("tacex_fem_marker_flow_library: %d patterns (a library holds at least one)", P); return 2; }
  if (Mmax < 1 || Mmax > 1024) {
    set_error("tacex_fem_marker_flow_library: %d markers per pattern (1 to 1024: one env's markers are staged in LDS)", Mmax);
    return 2;
  }
  if (!(lose_prob >= 0.0 && lose_prob <= 1.0)) { set_error("tacex_fem_marker_flow_library: lose-tracking probability %g outside [0, 1]", lose_prob); return 2; }
  if (!(sigma >= 0.0)) { set_error("tacex_fem_marker_flow_library: negative noise sigma %g", sigma); return 2; }
  if (B <= 0 || K <= 0) return 0;
  if (V <= 0 || Vs <= 0) { set_error("tacex_fem_marker_flow_library: %d vertices, %d surface vertices", V, Vs); return 2; }
  hipLaunchKernelGGL(fem_marker_flow_library_kernel, dim3(B), dim3(256), (size_t)Mmax * 40, (hipStream_t)stream, x,
                     reinterpret_cast<const long long*>(surf_ids), cam_pos, cam_rot_inv, ref_surf_cam, lib_tri, lib_wgt, lib_count, P, Mmax,
                     pattern_ids, draws, (unsigned int)(seed & 0xffffffffull), (unsigned int)(seed >> 32), fx, fy, cx, cy, lose_prob, sigma,
                     (double)img_h, (double)img_w, normalize_div, curr_uv, flow, flow_f32, num_tracked, V, Vs, K);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "fem_marker_flow_library_kernel");
}

int tacex_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) { set_error("tacex_philox4x32: null argument"); return 2; }
  philox4x32_10(ctr, key, out);  // the function fem_marker_flow_library_kernel calls, compiled for the host
  return 0;
}

}  // extern "C"
