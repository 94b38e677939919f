// FEM device layer, shared part: the scene description every kernel takes (FemDev, FemMat), contact and friction of one vertex, the tet
// helpers, block reductions, the 3x3 / chain / coarse-space steps of the preconditioners and the step_info flags.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fem_layout.h"

namespace tacex {

struct FemDev {
  int V, T;
  const int* tets;        // (4,T) SoA
  const double* dminv;    // (9,T) SoA, row-major 3x3 per tet
  const double* vol;      // (T)
  const double* tet_rec;  // (T,12) AoS copy of one tet: vertex ids (4 ints in the first two doubles) | dminv (9) | vol - for loops that visit
                          // tets in VERTEX order (every lane another tet): six 16-byte loads per tet instead of 14 scattered ones; nullable
  const double* tet_blk;  // wave-blocked SoA copy for loops that visit tets in TET order (the sweeps of fem_newton_lds_kernel): per block of
                          // 64 tets [9][64] dminv | [64] vol | [4][64] vertex ids (int32) = kTetBlkBytes; every component of lane l sits at
                          // block base + immediate + 8 l, so ONE 32-bit offset register addresses all 14 loads (the SoA arrays above
                          // need 14 per-lane 64-bit addresses, which the Newton kernel spilled and re-read from scratch one by one)
  const double* mass;     // (V)
  const int* vt_off;      // (V+1) CSR vertex -> incident (tet*4 + local)
  const int* vt_idx;
  double mu, lam, alpha, psi_rest, dt, strength;
  double step_cap;  // bounding-box diagonal of the rest mesh: no line search starts with a vertex moving further (fem_newton_lds_kernel)
  // IPC contact of the gelpad surface against one analytic indenter per env (first slice)
  const double* area;       // (V) contact weight of a vertex = a third of the area of its surface triangles (0: interior); nullable
  const double* indenters;  // (B,8) [kind, cx, cy, cz, radius, nx, ny, nz]: kind 0 none, 1 sphere, 2 half-space; nullable
  double dhat, kappa;       // barrier activation distance [m], stiffness [J/m^2]
  double fric_mu, fric_eps; // Coulomb friction ratio (0: off) and stick tolerance eps_velocity * dt [m] (tacex_fem_set_friction)
  // coarse space of the two-level preconditioner (tacex_fem_set_coarse_space); nc = 0: block Jacobi alone
  int nc;                   // coarse nodes (<= kFemMaxCoarse)
  const int* cv_node;       // (V,8) coarse nodes of a vertex (trilinear hats of a coarse grid over the mesh)
  const double* cv_w;       // (V,8) their weights
  const int* cn_off;        // (nc+1) CSR coarse node -> (vertex, weight) of its support
  const int* cn_vtx;
  const double* cn_w;
  const double* ac_inv;     // (3 nc, 3 nc) inverse of P^T A_0 P, A_0 = rest-state operator incl. the constraint masses
  // rigid triangle-mesh indenters (kind 4): a LIBRARY of meshes, one chosen per env (tacex_fem_set_indenter_mesh_library / _ids;
  // tacex_fem_set_indenter_mesh = a library of one).  Per mesh: (nt,9) triangles a | b - a | c - a in the mesh frame, (nt,4) their
  // bounding spheres (centroid, radius), (ceil(nt / 16),4) the bounding sphere of every cluster of 16 consecutive triangles (Morton
  // order of the mesh's own triangles; no cluster straddles two meshes).  (These five fields take the bytes of the one-mesh fields
  // they replaced: the kernel argument layout - and the code of the MESH = false Newton kernels - stays what it was.)
  int im_nt;                // triangles of all meshes (0: no library)
  int im_nm;                // meshes
  const double* im_lib;     // every mesh's three tables in one allocation, each region 32-byte aligned
  const int* im_off;        // (nm,4) offsets into im_lib in doubles: triangles | spheres | clusters, then the triangle count
  const int* im_ids;        // (B) mesh id of every env (tacex_fem_set_indenter_mesh_ids, read at every step); nullptr: mesh 0 everywhere
  // vertex chains of the block-tridiagonal part of the preconditioner (tacex_fem_set_chains); nullptr: every vertex its own chain
  int nch;                  // chains, singletons included (<= V)
  const int* ch_head;       // (nch) first vertex of every chain
  const int* ch_next;       // (V) successor in the chain, -1 at its end
  const int* ch_prev;       // (V) predecessor, -1 at its head
};
// Gel MATERIAL LIBRARY (tacex_fem_set_material_library / _ids): K materials, one chosen per env.  Per material a record of kMatHead + V
// doubles: mu | lam | alpha | psi_rest | friction ratio | 3 pad | the (V) mass table of its density.  A kernel launched with MAT = true
// resolves its env's record once at entry (env_material) and overwrites mu, lam, alpha, psi_rest, fric_mu, mass and ac_inv of ITS copy
// of FemDev with it; with no library (n = 0) the MAT = false instantiations run and the argument is not read.  It is the LAST argument
// of every kernel that takes it and FemDev is what it was: no older argument moves, and the MAT = false kernels keep their code.
struct FemMat {
  int n;                // materials (0: no library)
  const double* lib;    // (n, kMatHead + V)
  const int* ids;       // (B) material id of every env (tacex_fem_set_material_ids, read at every step); nullptr: material 0 everywhere
  const double* ac;     // (n, 3 nc, 3 nc) coarse inverse per material (tacex_fem_set_material_coarse_inverses); nullptr: FemDev::ac_inv for all
};
constexpr int kMatHead = 8;
constexpr int kFemMaxCoarse = 64;

// ---- IPC barrier of one surface vertex against the env's analytic indenter ------------------------------------------
// Li et al. 2020 (IPC) eq. 6 in the dimensionless gap s = d / dhat:  b(s) = -(s - 1)^2 ln s  for 0 < s < 1, 0 beyond.
// Potential term of a vertex with weight w: dt^2 kappa w b(d / dhat); d = signed distance to the indenter surface
// (sphere: |x - c| - R, half-space: n . (x - c), capsule: distance to the axis segment - R), n = grad d.  A gap <= 0 is a penetration: infinite energy (the
// line search never accepts it; the conservative step bound below keeps the Newton direction out of it).
typedef double v4d __attribute__((ext_vector_type(4)));
struct ContactEval {
  bool active;      // 0 < d < dhat
  bool penetrating; // d <= 0
  double d, n[3];
  double e, b1, b2; // energy, dE/dd, d2E/dd2 (already times kappa w, NOT times dt^2)
};
// The env's mesh of the library, resolved ONCE per workgroup at kernel entry (wave-uniform: SGPRs).  nt = 0 - no mesh set, an env
// whose row is not kind 4, or a mesh id outside [0, im_nm), which is never dereferenced - makes a kind-4 row "no indenter"; `bad`
// reports the last case for a kind-4 row (kFemFlagBadMesh).  MESH = false: nothing is read.
struct IndMesh {
  int nt;
  const double* tri;  // (nt,9) this mesh's tables in FemDev::im_lib
  const double* bs;   // (nt,4)
  const double* cl;   // (ceil(nt / 16),4)
};
template <bool MESH>
__device__ __forceinline__ IndMesh env_mesh(const FemDev& m, int b, const double* ind, bool& bad) {
  IndMesh r{0, nullptr, nullptr, nullptr};
  bad = false;
  if (!MESH || !ind || m.im_nm <= 0) return r;
  const int id = m.im_ids ? __builtin_amdgcn_readfirstlane(m.im_ids[b]) : 0;
  if (id < 0 || id >= m.im_nm) {
    bad = (int)ind[0] == 4;
    return r;
  }
  const int* e = m.im_off + 4 * id;
  r.tri = m.im_lib + (unsigned)__builtin_amdgcn_readfirstlane(e[0]);
  r.bs = m.im_lib + (unsigned)__builtin_amdgcn_readfirstlane(e[1]);
  r.cl = m.im_lib + (unsigned)__builtin_amdgcn_readfirstlane(e[2]);
  r.nt = __builtin_amdgcn_readfirstlane(e[3]);
  return r;
}

// The env's material of the library, resolved ONCE per workgroup at kernel entry like env_mesh: every FEM kernel takes its env from
// the block index (fem_newton_lds_kernel through env_order), so no wave straddles two envs and the id, the five constants and the
// two table addresses are wave-uniform (readfirstlane: SGPRs, scalar loads).  REPLACES the material fields of the kernel's own copy
// of the scene description; everything downstream keeps reading `m.mu`, `m.mass[v]`, `m.ac_inv`, `m.fric_mu`.  An id outside
// [0, mat.n) is never dereferenced: the env takes material 0 and `bad` reports it (kFemFlagBadMaterial).  MAT = false: `m` is not
// touched - those instantiations are, statement for statement, the kernels from before the library.
__device__ __forceinline__ double uniform_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
template <bool MAT>
__device__ __forceinline__ bool env_material(FemDev& m, const FemMat& mat, int b) {
  bool bad = false;
  if constexpr (MAT) {
    if (mat.n > 0) {
      int id = mat.ids ? __builtin_amdgcn_readfirstlane(mat.ids[b]) : 0;
      if (id < 0 || id >= mat.n) { bad = true; id = 0; }
      const double* rec = mat.lib + (size_t)id * (size_t)(kMatHead + m.V);
      m.mu = uniform_f64(rec[0]); m.lam = uniform_f64(rec[1]); m.alpha = uniform_f64(rec[2]); m.psi_rest = uniform_f64(rec[3]);
      m.fric_mu = uniform_f64(rec[4]);
      m.mass = rec + kMatHead;
      if (mat.ac) m.ac_inv = mat.ac + (size_t)id * (size_t)(9 * m.nc * m.nc);
    }
  }
  return bad;
}

// Unsigned distance of p (mesh frame) to the nearest triangle of the indenter mesh and the unit vector from the closest point to p.
// Two-level culling with bounding spheres: clusters of kMeshCluster triangles (Morton order of the centroids, built on the host), then
// the triangles of a cluster; a sphere farther than the best distance so far is skipped.  The sphere tables are fetched FOUR at a time
// (a loop with one dependent L2 round trip per triangle took 45 ms per step for 320 triangles).  `cut2`: the search radius squared -
// energy evaluations only need triangles within d_hat (+ offset); with nothing inside the result is sqrt(cut2), n = 0.  Closest point
// by Ericson (Real-Time Collision Detection 5.1.5), regions in the book's order; of two triangles at exactly the same distance the
// first visited wins (they share the closest point unless p lies on the medial axis).
constexpr int kMeshCluster = 16;
struct MeshDist { double d, n0, n1, n2; };
__device__ __noinline__ MeshDist mesh_distance(int nt, const double* __restrict__ tris, const double* __restrict__ bsph,
                                               const double* __restrict__ clus, double p0, double p1, double p2, double cut2) {
  const double p[3] = {p0, p1, p2};
  double best2 = cut2, best = sqrt(cut2), bq[3] = {0, 0, 0};
  auto beyond = [&](const v4d& sp) {  // the sphere (centre, radius) lies farther than the best distance so far
    const double c0 = p[0] - sp.x, c1 = p[1] - sp.y, c2 = p[2] - sp.z;
    const double lim = sp.w + best;
    return c0 * c0 + c1 * c1 + c2 * c2 >= lim * lim;
  };
  auto triangle = [&](int t) {
    const double* tr = tris + (size_t)t * 9;
    const double a[3] = {tr[0], tr[1], tr[2]}, ab[3] = {tr[3], tr[4], tr[5]}, ac[3] = {tr[6], tr[7], tr[8]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2], d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
    const double bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]};
    const double d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2], d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    const double cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
    const double d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2], d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double s = 0.0, u = 0.0;  // closest point = a + s ab + u ac
    if (d1 <= 0.0 && d2 <= 0.0) { s = 0.0; u = 0.0; }
    else if (d3 >= 0.0 && d4 <= d3) { s = 1.0; u = 0.0; }
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { s = d1 / (d1 - d3); u = 0.0; }
    else if (d6 >= 0.0 && d5 <= d6) { s = 0.0; u = 1.0; }
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { s = 0.0; u = d2 / (d2 - d6); }
    else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) { u = (d4 - d3) / ((d4 - d3) + (d5 - d6)); s = 1.0 - u; }
    else { const double den = 1.0 / (va + vb + vc); s = vb * den; u = vc * den; }
    const double q[3] = {a[0] + s * ab[0] + u * ac[0], a[1] + s * ab[1] + u * ac[1], a[2] + s * ab[2] + u * ac[2]};
    const double r0 = p[0] - q[0], r1 = p[1] - q[1], r2 = p[2] - q[2];
    const double dd = r0 * r0 + r1 * r1 + r2 * r2;
    if (dd < best2) { best2 = dd; best = sqrt(dd); bq[0] = r0; bq[1] = r1; bq[2] = r2; }
  };
  const v4d* cl4 = reinterpret_cast<const v4d*>(clus);
  const v4d* bs4 = reinterpret_cast<const v4d*>(bsph);
  const int ncl = (nt + kMeshCluster - 1) / kMeshCluster;
  auto cluster = [&](int q) {
    const int t0 = q * kMeshCluster, t1 = min(nt, t0 + kMeshCluster);
    for (int tb = t0; tb < t1; tb += 4) {
      v4d ts[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ts[j] = bs4[min(tb + j, nt - 1)];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (tb + j < t1 && !beyond(ts[j])) triangle(tb + j);
    }
  };
  // pass 1: the cluster whose sphere comes nearest is searched first - its best distance culls nearly all of pass 2 (walking the
  // clusters in table order the bound only tightens as fast as the order happens to approach p)
  int first = -1;
  {
    double lo = 1e300;
    for (int c0 = 0; c0 < ncl; c0 += 4) {
      v4d cs[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) cs[k] = cl4[min(c0 + k, ncl - 1)];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double c0x = p[0] - cs[k].x, c1x = p[1] - cs[k].y, c2x = p[2] - cs[k].z;
        const double lb = sqrt(c0x * c0x + c1x * c1x + c2x * c2x) - cs[k].w;
        if (c0 + k < ncl && lb < lo) { lo = lb; first = c0 + k; }
      }
    }
    if (first >= 0 && lo < best) cluster(first);
  }
  for (int c0 = 0; c0 < ncl; c0 += 4) {
    v4d cs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cs[k] = cl4[min(c0 + k, ncl - 1)];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < ncl && c0 + k != first && !beyond(cs[k])) cluster(c0 + k);
  }
  MeshDist r;
  r.d = best;
  const double ir = best > 0.0 && best2 < cut2 ? 1.0 / best : 0.0;
  r.n0 = bq[0] * ir; r.n1 = bq[1] * ir; r.n2 = bq[2] * ir;
  return r;
}

// MESH = false compiles the triangle-mesh indenter (kind 4: a function call in the middle of a 256-register kernel) out: the Newton
// kernel is instantiated both ways and the mesh-capable one is launched only when a mesh has been set.
template <bool MESH = true>
__device__ __forceinline__ ContactEval contact_eval(const FemDev& m, const IndMesh& im, const double* ind, double w, const double x[3],
                                                    bool need_distance = true) {
  ContactEval c;
  c.active = false; c.penetrating = false; c.d = 1e300; c.e = 0.0; c.b1 = 0.0; c.b2 = 0.0; c.n[0] = c.n[1] = c.n[2] = 0.0;
  if (!ind || !(w > 0.0)) return c;
  const int kind = (int)ind[0];
  if (kind == 1) {
    const double r0 = x[0] - ind[1], r1 = x[1] - ind[2], r2 = x[2] - ind[3];
    const double rho = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    c.d = rho - ind[4];
    const double ir = rho > 0.0 ? 1.0 / rho : 0.0;
    c.n[0] = r0 * ir; c.n[1] = r1 * ir; c.n[2] = r2 * ir;
  } else if (kind == 2) {
    c.n[0] = ind[5]; c.n[1] = ind[6]; c.n[2] = ind[7];
    c.d = c.n[0] * (x[0] - ind[1]) + c.n[1] * (x[1] - ind[2]) + c.n[2] * (x[2] - ind[3]);
  } else if (kind == 3) {
    // capsule (cylinder with hemispherical caps, e.g. a lying pin or a finger): centre c, radius R, the vector (nx, ny, nz) is
    // HALF the axis (direction and half length); the closest axis point is c + clamp(p . a / |a|^2, -1, 1) a
    const double p0 = x[0] - ind[1], p1 = x[1] - ind[2], p2 = x[2] - ind[3];
    const double a0 = ind[5], a1 = ind[6], a2 = ind[7];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2;
    double t = aa > 0.0 ? (p0 * a0 + p1 * a1 + p2 * a2) / aa : 0.0;
    t = t < -1.0 ? -1.0 : (t > 1.0 ? 1.0 : t);
    const double r0 = p0 - t * a0, r1 = p1 - t * a1, r2 = p2 - t * a2;
    const double rho = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    c.d = rho - ind[4];
    const double ir = rho > 0.0 ? 1.0 / rho : 0.0;
    c.n[0] = r0 * ir; c.n[1] = r1 * ir; c.n[2] = r2 * ir;
  } else if (MESH && kind == 4 && im.nt > 0) {
    // rigid triangle mesh (the env's mesh of the library, env_mesh) at position c with rotation vector (nx, ny, nz), inflated by R: UNSIGNED
    // distance to the nearest triangle - R (the step bound keeps a vertex from crossing the surface; a vertex that starts
    // inside the mesh is not detected)
    const double r0 = ind[5], r1 = ind[6], r2 = ind[7];
    const double th2 = r0 * r0 + r1 * r1 + r2 * r2, th = sqrt(th2);
    const double ka = th < 1e-12 ? 1.0 : sin(th) / th, kb = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / th2;
    // R = I + ka K + kb K^2, K = [r]x
    const double R[9] = {1.0 - kb * (r1 * r1 + r2 * r2), -ka * r2 + kb * r0 * r1, ka * r1 + kb * r0 * r2,
                         ka * r2 + kb * r0 * r1, 1.0 - kb * (r0 * r0 + r2 * r2), -ka * r0 + kb * r1 * r2,
                         -ka * r1 + kb * r0 * r2, ka * r0 + kb * r1 * r2, 1.0 - kb * (r0 * r0 + r1 * r1)};
    const double g0 = x[0] - ind[1], g1 = x[1] - ind[2], g2 = x[2] - ind[3];
    const double pl[3] = {R[0] * g0 + R[3] * g1 + R[6] * g2, R[1] * g0 + R[4] * g1 + R[7] * g2, R[2] * g0 + R[5] * g1 + R[8] * g2};  // R^T (x - c)
    // need_distance = false (energy evaluations): anything at or beyond d_hat is as good as infinitely far
    const double reach = m.dhat + ind[4];
    const MeshDist md = mesh_distance(im.nt, im.tri, im.bs, im.cl, pl[0], pl[1], pl[2], need_distance ? 1e300 : reach * reach * (1.0 + 1e-12));
    const double nl[3] = {md.n0, md.n1, md.n2};
    c.d = md.d - ind[4];
    c.n[0] = R[0] * nl[0] + R[1] * nl[1] + R[2] * nl[2];
    c.n[1] = R[3] * nl[0] + R[4] * nl[1] + R[5] * nl[2];
    c.n[2] = R[6] * nl[0] + R[7] * nl[1] + R[8] * nl[2];
  } else {
    return c;
  }
  if (c.d <= 0.0) { c.penetrating = true; c.e = INFINITY; return c; }
  if (c.d >= m.dhat) return c;
  c.active = true;
  const double sg = c.d / m.dhat, ln = log(sg), q = sg - 1.0, kw = m.kappa * w;
  c.e = -kw * q * q * ln;
  c.b1 = kw * (-2.0 * q * ln - q * q / sg) / m.dhat;
  c.b2 = kw * (-2.0 * ln - 4.0 * q / sg + q * q / (sg * sg)) / (m.dhat * m.dhat);
  return c;
}
// ---- lagged Coulomb friction of one surface vertex (IPC, Li et al. 2020 eq. 18-20; US:103-124 enable_friction / friction ratio /
// eps_velocity).  Normal force lam = -dB/dd and contact normal n are LAGGED (frozen), which makes the potential a smooth function of
// x.  WHERE the lag is taken: the state the step starts from (the default since round 4, `lag_at_start` in fem_newton_lds_kernel) - IPC's
// lag "from the previous time step".  After the indenter has moved, that state sits deep in the 10 GPa barrier, where -dB/dd is orders of
// magnitude above the elastic forces of the soft pad (Newton directions of metres, PCG at its cap: why rounds 3-4 ran the loop in TWO
// PHASES - normal contact alone until converged, then the lag from that state and a friction phase); but the lag takes the SMALLER of
// -dB/dd and the contact REACTION (g_other . n) / dt^2, and at the start state - the previous step's equilibrium - that reaction is the
// previous step's normal force.  With the cap the start-of-step lag is well behaved, and the step saves the iteration the second phase
// cost (a pressing step is one Newton iteration instead of two).  TACEX_FEM_FRIC_LAG=0 keeps the two-phase loop for the A/B.
// u = (I - n n^T)(x - x_n - disp) is the tangential sliding relative to the indenter (x_n = positions the step
// started from, disp = the indenter's own displacement since the previous step).  Potential mu lam f0(|u|), f0(y) = -y^3 / (3 eps^2) + y^2 / eps + eps / 3 below the stick
// tolerance eps, y beyond; gradient mu lam (f1 / y) u; Hessian mu lam [(f1 / y)(T - t t^T) + f1' t t^T] (both coefficients >= 0).
struct FricVertex {  // what a vertex keeps in LDS for the step: lam, n (4 doubles)
  double lam, n[3];
};
struct FricEval {
  double e;       // mu lam f0(y)              (NOT times dt^2)
  double g[3];    // gradient
  double h[6];    // Hessian, symmetric: xx xy xz yy yz zz
};
__device__ __forceinline__ FricEval friction_eval(double mu, double eps, const double* fv /* lam, n */, const double x[3], const double xn[3],
                                                  const double disp[3], bool with_hessian) {
  FricEval f;
  f.e = 0.0; f.g[0] = f.g[1] = f.g[2] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) f.h[k] = 0.0;
  const double lam = fv[0];
  if (!(lam > 0.0)) return f;
  const double n0 = fv[1], n1 = fv[2], n2 = fv[3];
  const double r0 = x[0] - xn[0] - disp[0], r1 = x[1] - xn[1] - disp[1], r2 = x[2] - xn[2] - disp[2];
  const double rn = r0 * n0 + r1 * n1 + r2 * n2;
  const double u0 = r0 - rn * n0, u1 = r1 - rn * n1, u2 = r2 - rn * n2;
  const double y = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
  const bool stick = y < eps;
  const double a = stick ? 2.0 / eps - y / (eps * eps) : 1.0 / y;   // f1 / y
  const double c = mu * lam;
  f.e = c * (stick ? -y * y * y / (3.0 * eps * eps) + y * y / eps + eps / 3.0 : y);
  f.g[0] = c * a * u0; f.g[1] = c * a * u1; f.g[2] = c * a * u2;
  if (with_hessian) {
    const double bq = stick ? 2.0 / eps - 2.0 * y / (eps * eps) : 0.0;  // f1'
    const double iy = y > 0.0 ? 1.0 / y : 0.0;
    const double t0 = u0 * iy, t1 = u1 * iy, t2 = u2 * iy;
    const double ca = c * a, cb = c * (bq - a);  // a (T - t t^T) + bq t t^T = a T + (bq - a) t t^T
    f.h[0] = ca * (1.0 - n0 * n0) + cb * t0 * t0; f.h[1] = ca * (-n0 * n1) + cb * t0 * t1; f.h[2] = ca * (-n0 * n2) + cb * t0 * t2;
    f.h[3] = ca * (1.0 - n1 * n1) + cb * t1 * t1; f.h[4] = ca * (-n1 * n2) + cb * t1 * t2; f.h[5] = ca * (1.0 - n2 * n2) + cb * t2 * t2;
  }
  return f;
}
constexpr double kCcdSlack = 0.9;  // fraction of the conservative (1-Lipschitz) step bound d / |dx| a Newton step may use

// ---- small dense helpers (row-major 3x3 in double[9]) ---------------------------------------------------
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

struct TetState {
  double F[9], C[9];
  double a, b, c;   // coefficients above
  double Ic, J;
};

// the same through the AoS record (see FemDev::tet_rec); also returns the volume
__device__ __forceinline__ void load_tet_rec(const FemDev& m, int t, int v[4], double Di[9], double& vol) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v2d* q = reinterpret_cast<const v2d*>(m.tet_rec + (size_t)t * 12);
  const v2d q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5];
  v[0] = __double2loint(q0.x); v[1] = __double2hiint(q0.x); v[2] = __double2loint(q0.y); v[3] = __double2hiint(q0.y);
  Di[0] = q1.x; Di[1] = q1.y; Di[2] = q2.x; Di[3] = q2.y; Di[4] = q3.x; Di[5] = q3.y; Di[6] = q4.x; Di[7] = q4.y; Di[8] = q5.x;
  vol = q5.y;
}

// table read at (uniform base) + (32-bit byte offset): selects the scalar-base form of the load (global_load v, v_off, s[base:base+1]), so
// a loop keeps ONE 32-bit offset alive instead of a 64-bit per-lane address per table - the Newton kernel carried ~25 such addresses
// across its PCG loop, spilled them, and read them back from scratch (which misses the L2: 512 envs x 300 KB) one dependent wait at a time
template <typename T>
__device__ __forceinline__ T ldg_off(const void* base, unsigned byte_off) {
  return *reinterpret_cast<const T*>(static_cast<const char*>(base) + byte_off);
}

// a value the optimiser must treat as unknown: address arithmetic built on it is recomputed where it is used (a few integer
// operations) instead of being hoisted out of the enclosing loops and kept live - or spilled - across them
__device__ __forceinline__ unsigned opaque_u32(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}

// The thread index rebuilt from nothing but the wave's index (a scalar register) and the lane counter: inside the Newton kernel the
// register allocator spilled threadIdx.x itself - and the LDS addresses derived from it - and re-read them from scratch fourteen
// times per PCG iteration.  volatile: every call site gets its own two-instruction copy, nothing is carried between phases.
__device__ __forceinline__ int fresh_tid(int wave_index) {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return wave_index * 64 + l;
}

constexpr unsigned kTetBlkBytes = 9 * 512 + 512 + 4 * 256;  // 6144
// one tet through the wave-blocked table (see FemDev::tet_blk): coalesced like the SoA arrays, one offset register
__device__ __forceinline__ void load_tet_blk(const FemDev& m, int t, int v[4], double Di[9], double& vol) {
  const unsigned ln = (unsigned)t & 63u;
  const unsigned ob = ((unsigned)t >> 6) * kTetBlkBytes;
  const char* base = reinterpret_cast<const char*>(m.tet_blk);
  const unsigned o8 = ob + ln * 8u, o4 = ob + 5120u + ln * 4u;
#pragma unroll
  for (int k = 0; k < 9; ++k) Di[k] = *reinterpret_cast<const double*>(base + (o8 + (unsigned)k * 512u));
  vol = *reinterpret_cast<const double*>(base + (o8 + 4608u));
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const int*>(base + (o4 + (unsigned)k * 256u));
}

__device__ __forceinline__ void load_tet(const FemDev& m, int t, int v[4], double Di[9]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = m.tets[k * m.T + t];
#pragma unroll
  for (int k = 0; k < 9; ++k) Di[k] = m.dminv[k * m.T + t];
}

// F = Ds * DmInv with Ds columns (x1-x0, x2-x0, x3-x0); x points at one env's (V,3) array
__device__ __forceinline__ void deformation_gradient(const double* x, const int v[4], const double Di[9], double F[9]) {
  double Ds[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < 3; ++i) Ds[i * 3 + k] = x[v[k + 1] * 3 + i] - x[v[0] * 3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int mm = 0; mm < 3; ++mm)
      F[i * 3 + mm] = Ds[i * 3 + 0] * Di[0 * 3 + mm] + Ds[i * 3 + 1] * Di[1 * 3 + mm] + Ds[i * 3 + 2] * Di[2 * 3 + mm];
}

__device__ __forceinline__ void tet_state(const FemDev& m, const double F[9], TetState& s) {
  double f0[3] = {F[0], F[3], F[6]}, f1[3] = {F[1], F[4], F[7]}, f2[3] = {F[2], F[5], F[8]};
  double c0[3], c1[3], c2[3];
  cross3(f1, f2, c0);
  cross3(f2, f0, c1);
  cross3(f0, f1, c2);
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.C[i * 3 + 0] = c0[i]; s.C[i * 3 + 1] = c1[i]; s.C[i * 3 + 2] = c2[i]; }
  double Ic = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) { s.F[k] = F[k]; Ic += F[k] * F[k]; }
  s.Ic = Ic;
  s.J = f0[0] * c0[0] + f0[1] * c0[1] + f0[2] * c0[2];
  s.a = m.mu * (1.0 - 1.0 / (Ic + 1.0));
  s.b = 2.0 * m.mu / ((Ic + 1.0) * (Ic + 1.0));
  s.c = m.lam * (s.J - m.alpha);
}

__device__ __forceinline__ double psi_of(const FemDev& m, const TetState& s) {
  const double dj = s.J - m.alpha;
  return 0.5 * m.mu * (s.Ic - 3.0) + 0.5 * m.lam * dj * dj - 0.5 * m.mu * log(s.Ic + 1.0) - m.psi_rest;
}

// dP = (9x9 Hessian of Psi) applied to dF
__device__ __forceinline__ void apply_dP(const FemDev& m, const TetState& s, const double dF[9], double dP[9]) {
  double FdF = 0.0, CdF = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) { FdF += s.F[k] * dF[k]; CdF += s.C[k] * dF[k]; }
  const double* F = s.F;
  double f0[3] = {F[0], F[3], F[6]}, f1[3] = {F[1], F[4], F[7]}, f2[3] = {F[2], F[5], F[8]};
  double d0[3] = {dF[0], dF[3], dF[6]}, d1[3] = {dF[1], dF[4], dF[7]}, d2[3] = {dF[2], dF[5], dF[8]};
  double t1[3], t2[3], e0[3], e1[3], e2[3];
  cross3(d1, f2, t1); cross3(f1, d2, t2);
#pragma unroll
  for (int i = 0; i < 3; ++i) e0[i] = t1[i] + t2[i];
  cross3(d2, f0, t1); cross3(f2, d0, t2);
#pragma unroll
  for (int i = 0; i < 3; ++i) e1[i] = t1[i] + t2[i];
  cross3(d0, f1, t1); cross3(f0, d1, t2);
#pragma unroll
  for (int i = 0; i < 3; ++i) e2[i] = t1[i] + t2[i];
  const double bb = s.b * FdF, ll = m.lam * CdF;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    dP[i * 3 + 0] = s.a * dF[i * 3 + 0] + bb * F[i * 3 + 0] + ll * s.C[i * 3 + 0] + s.c * e0[i];
    dP[i * 3 + 1] = s.a * dF[i * 3 + 1] + bb * F[i * 3 + 1] + ll * s.C[i * 3 + 1] + s.c * e1[i];
    dP[i * 3 + 2] = s.a * dF[i * 3 + 2] + bb * F[i * 3 + 2] + ll * s.C[i * 3 + 2] + s.c * e2[i];
  }
}

// rows r_v (v = 0..3) with dF[k][m] / dx[v][k] = r_v[m]:  r_{1..3} = rows of DmInv, r_0 = -(r_1 + r_2 + r_3)
__device__ __forceinline__ void shape_rows(const double Di[9], double r[12]) {
#pragma unroll
  for (int mm = 0; mm < 3; ++mm) {
    r[3 + mm] = Di[0 * 3 + mm]; r[6 + mm] = Di[1 * 3 + mm]; r[9 + mm] = Di[2 * 3 + mm];
    r[mm] = -(Di[0 * 3 + mm] + Di[1 * 3 + mm] + Di[2 * 3 + mm]);
  }
}

// element gradient (12) = scale * P : dF/dx
__device__ __forceinline__ void element_gradient(const TetState& s, const double r[12], double scale, double g[12]) {
  double P[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) P[k] = s.a * s.F[k] + s.c * s.C[k];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int i = 0; i < 3; ++i)
      g[v * 3 + i] = scale * (P[i * 3 + 0] * r[v * 3 + 0] + P[i * 3 + 1] * r[v * 3 + 1] + P[i * 3 + 2] * r[v * 3 + 2]);
}

// ---- block-wide sum (wave shuffle + LDS), result broadcast to all threads ------------------------------------
__device__ __forceinline__ double block_sum(double v, double* sh /* >= 17 doubles */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();  // protect sh from the previous use
  if ((threadIdx.x & 63) == 0) sh[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += sh[w];
    sh[16] = s;
  }
  __syncthreads();
  return sh[16];
}

// block-wide maximum, same scheme
__device__ __forceinline__ double block_sum_max(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sh[0];
    for (int w = 1; w < nw; ++w) s = fmax(s, sh[w]);
    sh[16] = s;
  }
  __syncthreads();
  return sh[16];
}
constexpr int kLsRescueStream = 32;  // rescue halvings of the line search next to a barrier (kLsRescue of the CU-resident kernel)

__device__ __forceinline__ bool inv3_spd(const double A[9], double Ai[9]) {
  // Cholesky test + inverse via adjugate
  if (!(A[0] > 0.0)) return false;
  const double l10 = A[3] / sqrt(A[0]), l20 = A[6] / sqrt(A[0]);
  const double d1 = A[4] - l10 * l10;
  if (!(d1 > 0.0)) return false;
  const double l21 = (A[7] - l20 * l10) / sqrt(d1);
  const double d2 = A[8] - l20 * l20 - l21 * l21;
  if (!(d2 > 0.0)) return false;
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  const double id = 1.0 / det;
  Ai[0] = c00 * id; Ai[1] = (A[2] * A[7] - A[1] * A[8]) * id; Ai[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  Ai[3] = c01 * id; Ai[4] = (A[0] * A[8] - A[2] * A[6]) * id; Ai[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  Ai[6] = c02 * id; Ai[7] = (A[1] * A[6] - A[0] * A[7]) * id; Ai[8] = (A[0] * A[4] - A[1] * A[3]) * id;
  return true;
}

// ---- steps the Newton kernels share (fem_newton_kernel, fem_newton_lds_kernel, fem_ball_newton_kernel): ONE copy of each rule, so the
// kernels cannot drift apart in the preconditioner they apply or the friction lag they take ----

// row i of z = Dinv r, Dinv a row-major 3x3 block (block Jacobi)
__device__ __forceinline__ double apply_block3_row(const double* Dinv9, const double* r, int i) {
  return Dinv9[i * 3 + 0] * r[0] + Dinv9[i * 3 + 1] * r[1] + Dinv9[i * 3 + 2] * r[2];
}

// tet state of the streaming kernel's cache tc (12,T): F (9) | a | b | c as the element pass left them; the cofactor is rebuilt from F
// (Ic and J are not cached: apply_dP does not read them)
__device__ __forceinline__ void cached_tet_state(const double* tc, int T, int t, TetState& s) {
#pragma unroll
  for (int k = 0; k < 9; ++k) s.F[k] = tc[(size_t)k * T + t];
  {  // cofactor from F
    double f0[3] = {s.F[0], s.F[3], s.F[6]}, f1[3] = {s.F[1], s.F[4], s.F[7]}, f2[3] = {s.F[2], s.F[5], s.F[8]};
    double c0[3], c1[3], c2[3];
    cross3(f1, f2, c0); cross3(f2, f0, c1); cross3(f0, f1, c2);
#pragma unroll
    for (int i = 0; i < 3; ++i) { s.C[i * 3 + 0] = c0[i]; s.C[i * 3 + 1] = c1[i]; s.C[i * 3 + 2] = c2[i]; }
  }
  s.a = tc[(size_t)9 * T + t]; s.b = tc[(size_t)10 * T + t]; s.c = tc[(size_t)11 * T + t];
}

// the tet's 12 rows of H.p: rows[w * 3 + i] = sc * (dP r_w^T)[i], dP = apply_dP of dF(p), r = shape_rows, sc = dt^2 vol
__device__ __forceinline__ void element_hp_rows(const double dP[9], const double r[12], double sc, double rows[12]) {
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int i = 0; i < 3; ++i)
      rows[w * 3 + i] = sc * (dP[i * 3 + 0] * r[w * 3 + 0] + dP[i * 3 + 1] * r[w * 3 + 1] + dP[i * 3 + 2] * r[w * 3 + 2]);
}

// entry i of a coarse-space table.  OFF32: through ldg_off - the CU-resident kernel keeps one 32-bit offset per table alive instead of
// a 64-bit per-lane address (see ldg_off); the kernels whose vectors live in memory index the table as it is
template <bool OFF32, typename T>
__device__ __forceinline__ T coarse_table(const T* base, int i) {
  if constexpr (OFF32) return ldg_off<T>(base, (unsigned)i * (unsigned)sizeof(T));
  else return base[i];
}

// lanes per coarse NODE of the restriction: the largest power of two that divides a wave and leaves every node its own group
__device__ __forceinline__ int coarse_lanes_per_node(int NT, int nc) {
  int G = 1;
  while (2 * G <= NT / nc && 2 * G <= 64) G *= 2;
  return G;
}

// Restriction r_c = P^T r onto the coarse nodes: G lanes per coarse NODE, all three components (one (vertex, weight) fetch serves three
// sums); the partial sums of a node sit in ONE wave and are added by a butterfly of lane exchanges - no LDS round trip, no barrier, a
// fixed tree (deterministic).  Every lane of the wave takes part in the exchange.  rc is complete after the caller's next barrier.
template <bool OFF32>
__device__ __forceinline__ void restrict_to_coarse(const FemDev& m, const double* r, double* rc, int G, int tid) {
  const int node = tid / G, j = tid - node * G;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (node < m.nc) {
    const int e1 = coarse_table<OFF32>(m.cn_off, node + 1);
    for (int e = coarse_table<OFF32>(m.cn_off, node) + j; e < e1; e += G) {
      const int v0 = coarse_table<OFF32>(m.cn_vtx, e);
      const double w0 = coarse_table<OFF32>(m.cn_w, e);
      a0 += w0 * r[v0 * 3]; a1 += w0 * r[v0 * 3 + 1]; a2 += w0 * r[v0 * 3 + 2];
    }
  }
  for (int o2 = G >> 1; o2 > 0; o2 >>= 1) { a0 += __shfl_xor(a0, o2, 64); a1 += __shfl_xor(a1, o2, 64); a2 += __shfl_xor(a2, o2, 64); }
  if (node < m.nc && j == 0) { rc[node * 3] = a0; rc[node * 3 + 1] = a1; rc[node * 3 + 2] = a2; }
}

// Block-tridiagonal LDL^T along ONE vertex chain (tacex_fem_set_chains; a chain of one vertex = 3x3 block Jacobi), walked by the chain's
// thread from its head:  S_0 = D_0,  G_i = S_i^-1 E_i,  S_{i+1} = D_{i+1} - E_i^T G_i.  S^-1 (6, upper triangle) and G (9) go to
// cf (V,15) as FLOATS: z = L^-T S^-1 L^-1 r is symmetric positive definite for any G as long as the S^-1 are, so the rounding costs
// preconditioner quality only.  load_D(v, D[9]): the full diagonal block of vertex v; block_E(v, E): points E at the row-major block
// A(v, next(v)) and returns false where the scene has none (the ball kernel without its blk table: the chain falls apart into 3x3 blocks).
template <typename LoadD, typename BlockE>
__device__ __forceinline__ void chain_factor(int head, LoadD&& load_D, BlockE&& block_E, float* cf, const unsigned short* cnx) {
  int v = head;
  double S[9];
  load_D(v, S);
  while (true) {
    double Si[9];
    if (!inv3_spd(S, Si)) {  // cannot happen in exact arithmetic (PSD-projected element Hessians + mass); keep the operator SPD
      const double dm = fmax(S[0], fmax(S[4], S[8]));
      const double im = 1.0 / (dm > 0.0 ? dm : 1.0);
      Si[0] = im; Si[1] = 0; Si[2] = 0; Si[3] = 0; Si[4] = im; Si[5] = 0; Si[6] = 0; Si[7] = 0; Si[8] = im;
    }
    float* f = cf + v * 15;
    f[0] = (float)Si[0]; f[1] = (float)Si[1]; f[2] = (float)Si[2]; f[3] = (float)Si[4]; f[4] = (float)Si[5]; f[5] = (float)Si[8];
    const int n = cnx[v] == 0xffff ? -1 : (int)cnx[v];
    const double* Ev = nullptr;
    if (n < 0 || !block_E(v, Ev)) {
#pragma unroll
      for (int k = 0; k < 9; ++k) f[6 + k] = 0.0f;
      if (n < 0) break;
      load_D(n, S);
      v = n;
      continue;
    }
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) G[i * 3 + k] = Si[i * 3 + 0] * Ev[k] + Si[i * 3 + 1] * Ev[3 + k] + Si[i * 3 + 2] * Ev[6 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[6 + k] = (float)G[k];
    double Dn[9];  // S_next = D_next - E^T G
    load_D(n, Dn);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) S[i * 3 + k] = Dn[i * 3 + k] - (Ev[i] * G[k] + Ev[3 + i] * G[3 + k] + Ev[6 + i] * G[6 + k]);
    v = n;
  }
}

// Chain solve z = L^-T S^-1 L^-1 r with the factors of chain_factor, by the chain's thread: down the chain y_i = r_i - G_{i-1}^T y_{i-1},
// back up z_i = S_i^-1 y_i - G_i z_{i+1}; y travels in `out`.  IN_PLACE (in == out, the ball kernel): the head's y is r where it lies, so
// only the successors are written on the way down; with two arrays every y is.
template <bool IN_PLACE>
__device__ __forceinline__ void chain_solve(int head, const double* in, double* out, const float* cf, const unsigned short* cnx,
                                            const unsigned short* cpv) {
  int v = head, last = head;
  double y[3] = {in[v * 3], in[v * 3 + 1], in[v * 3 + 2]};
  while (true) {
    if constexpr (!IN_PLACE) { out[v * 3] = y[0]; out[v * 3 + 1] = y[1]; out[v * 3 + 2] = y[2]; }
    last = v;
    const int n = cnx[v] == 0xffff ? -1 : (int)cnx[v];
    if (n < 0) break;
    const float* g = cf + v * 15 + 6;
    const double y0 = y[0], y1 = y[1], y2 = y[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = in[n * 3 + k] - ((double)g[k] * y0 + (double)g[3 + k] * y1 + (double)g[6 + k] * y2);
    if constexpr (IN_PLACE) { out[n * 3] = y[0]; out[n * 3 + 1] = y[1]; out[n * 3 + 2] = y[2]; }
    v = n;
  }
  v = last;
  double zn[3] = {0, 0, 0};
  while (true) {
    const float* f = cf + v * 15;
    const double y0 = out[v * 3], y1 = out[v * 3 + 1], y2 = out[v * 3 + 2];
    double zz[3];
    zz[0] = (double)f[0] * y0 + (double)f[1] * y1 + (double)f[2] * y2;
    zz[1] = (double)f[1] * y0 + (double)f[3] * y1 + (double)f[4] * y2;
    zz[2] = (double)f[2] * y0 + (double)f[4] * y1 + (double)f[5] * y2;
#pragma unroll
    for (int i = 0; i < 3; ++i) zz[i] -= (double)f[6 + i * 3] * zn[0] + (double)f[7 + i * 3] * zn[1] + (double)f[8 + i * 3] * zn[2];
    out[v * 3] = zz[0]; out[v * 3 + 1] = zz[1]; out[v * 3 + 2] = zz[2];
    zn[0] = zz[0]; zn[1] = zz[1]; zn[2] = zz[2];
    const int pv = cpv[v] == 0xffff ? -1 : (int)cpv[v];
    if (pv < 0) break;
    v = pv;
  }
}

// Friction lag of one surface vertex (see friction_eval), the two rules of tacex_fem_set_friction_lag; each returns the normal force.
// IPC's lag to the letter (Li et al. 2020, section 5.4: lam^n, T^n "from the previous time step"): the barrier force and the normal (-> ln)
// of the PREVIOUS configuration - the position the step starts from (xn_v) against the indenter where it stood then (its row moved back
// by the displacement since the previous step).  That configuration is the previous step's equilibrium, so this IS the previous normal
// force; no cap, nothing of the current iterate enters (mode 1).
template <bool MESH>
__device__ __forceinline__ double friction_lag_ipc(const FemDev& m, const IndMesh& im, const double* ind, double wv, const double disp[3],
                                                   const double* xn_v, double ln[3]) {
  double indp[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) indp[k] = ind[k];
  indp[1] -= disp[0]; indp[2] -= disp[1]; indp[3] -= disp[2];
  const double xn3[3] = {xn_v[0], xn_v[1], xn_v[2]};
  const ContactEval cp = contact_eval<MESH>(m, im, indp, wv, xn3);
  ln[0] = cp.n[0]; ln[1] = cp.n[1]; ln[2] = cp.n[2];
  return (cp.active && !cp.penetrating) ? -cp.b1 : 0.0;
}
// The lag at the current state (mode 0), for a vertex whose barrier `ce` is active: the barrier force capped by the contact REACTION
// (go . n) / dt^2, go = the gradient without the contact terms (inertia + elasticity + constraints) - why: fem_newton_lds_kernel,
// FRICTION LAG.  The normal is ce.n.
__device__ __forceinline__ double friction_lag_capped(const ContactEval& ce, const double go[3], double dt2) {
  const double react = (go[0] * ce.n[0] + go[1] * ce.n[1] + go[2] * ce.n[2]) / dt2;
  return fmin(-ce.b1, fmax(react, 0.0));
}

// Additive coarse correction of the two-level preconditioner for kernels whose vectors live in memory (fem_newton_kernel, fem_ball_newton_kernel):
// z += P A_c^-1 P^T r over the (V,3) rows of one env (tacex_fem_set_coarse_space: trilinear hats of a coarse grid, A_c the rest-state
// operator's Galerkin product).  Every thread of the workgroup calls it; rc / yc: 3 * kFemMaxCoarse doubles of LDS each.  Returns this
// thread's share of r . (P A_c^-1 P^T r) (add it to the partial sum of r . z before the block reduction).  Fixed summation order.
__device__ __forceinline__ double coarse_correct(const FemDev& m, const double* r, double* z, double* rc, double* yc) {
  const int nc3 = 3 * m.nc, NT = (int)blockDim.x, tid = (int)threadIdx.x;
  restrict_to_coarse<false>(m, r, rc, coarse_lanes_per_node(NT, m.nc), tid);
  __syncthreads();
  double part = 0.0;
  if (tid < nc3) {
    double sv = 0.0;
    for (int k = 0; k < nc3; ++k) sv += m.ac_inv[(size_t)tid * nc3 + k] * rc[k];
    yc[tid] = sv;
    part = rc[tid] * sv;
  }
  __syncthreads();
  for (int v = tid; v < m.V; v += NT) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int nd = m.cv_node[v * 8 + k];
      const double w = m.cv_w[v * 8 + k];
      z[v * 3] += w * yc[nd * 3]; z[v * 3 + 1] += w * yc[nd * 3 + 1]; z[v * 3 + 2] += w * yc[nd * 3 + 2];
    }
  }
  return part;
}

// flags of step_info[., 2]
constexpr int kFemFlagPenetration = 1;  // a contact vertex was at or beyond the indenter surface when the iteration started
constexpr int kFemFlagLsFailed = 2;     // a line search found no decrease even after the rescue halvings
constexpr int kFemFlagCoarseOff = 4;    // informational: the coarse correction was switched off for the rest of the step (see kCoarseTrust)
constexpr int kFemFlagPsdSafe = 8;      // informational: the PCG met negative curvature and the env solved iterations of the step in PSD-safe mode
// (16: fem_ball.h's pair-list overflow)
constexpr int kFemFlagBadMesh = 32;     // the env's kind-4 row named a mesh id outside the library: no indenter this step (env_mesh)
constexpr int kFemFlagBadMaterial = 64; // the env's material id lay outside the library: it stepped with material 0 (env_material)

}  // namespace tacex
