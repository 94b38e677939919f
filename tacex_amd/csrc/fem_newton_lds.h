// FEM device layer: the CU-resident Newton kernel (K17c) and its LDS sizes.
#pragma once
#include "fem_device.h"

namespace tacex {

// ---- K17c: the same Newton iteration with the env's state resident on the CU ------------------------------------
// fem_newton_kernel above streams ~700 KB per env and PCG iteration through HBM / L2 (cached tet state, per-tet H*p rows,
// seven nodal vectors): 81 us per PCG iteration for 512 envs, bandwidth-bound.  Here
//   * thread v OWNS vertex v (V <= 512): x, r, z, p, d, H*p and the 3x3 preconditioner block live in registers;
//   * only what tets gather at random - x and p - sits in LDS (2 x 12 KB at 495 vertices);
//   * the tet state (F, cofactor, coefficients) is RECOMPUTED from the LDS x every iteration (~80 f64 FMAs) instead of
//     being re-read (96 B per tet);
//   * per-tet rows travel to their vertices through a 48 KB LDS window of 512 tets at a time; each vertex walks its CSR
//     incidence list (sorted by tet) once per iteration, so the result is deterministic (the order differs from the
//     streaming kernel's only by the tet renumbering of tacex_fem_create).
// Mesh constants (tets, DmInv, vol, CSR) are the only global reads inside the PCG loop and are shared by all envs (L2).
constexpr int kNwtThreads = 512;
constexpr int kNwtChunk = 512;  // tets per LDS exchange window (1024 = 2 per thread measured slower: 90 spilled VGPRs)
constexpr int kNwtTpw = kNwtChunk / kNwtThreads;
// MESHES OF MORE THAN 512 VERTICES run the same kernel with 768 threads (thread v still owns vertex v; 3 waves per SIMD instead of 2,
// i.e. 168 registers per lane instead of 256: more of the per-thread state goes to scratch, which is what such an env pays for
// staying on one CU - the streaming kernel's alternative is a trip through HBM per PCG iteration).  Only the atomic flavour exists
// there: without the exchange window and the incidence list in LDS (12 x NT doubles + 4 T shorts) a 593-vertex / 2 003-tet mesh with
// friction fits the CU's 160 KB.  The region between p and the reduction rows then only has to hold what the kernel parks in it: the
// 15 V doubles of D | E blocks the chain factorisation exchanges (p + region), the preconditioner's r | r_c | y_c | z.  What bounds the
// vertex count is the LDS, not the threads: 268 bytes per vertex with friction (about 600 vertices), 212 without (about 745) - a
// 1 024-thread variant would never be launched and is not instantiated.
__host__ __device__ constexpr int nwt_window_doubles(int V, int NT) {
  // (wide variants: p + this region carry the (V,15) D | E blocks the chain threads exchange for the factorisation - 12 V doubles - and,
  //  between sweeps, the preconditioner's r | r_c | y_c | z.  Shrinking it to the latter was tried in round 5: the factorisation then
  //  overwrites the reduction rows and the friction lag - a 550-vertex pad stopped yielding to its indenter.)
  return NT <= kNwtThreads ? 12 * kNwtChunk : (12 * V > 6 * V + 6 * kFemMaxCoarse ? 12 * V : 6 * V + 6 * kFemMaxCoarse);
}
// dynamic LDS of fem_newton_lds_kernel<., ., NT>: x, p | window | sums | [friction lag] | diagonal mass term (doubles) || chain factors |
// [friction Hessian blocks] (floats) || [incidence codes] | chain links | chain heads per thread | [CSR offsets] (u16)
static size_t nwt_lds_bytes(int V, int T, bool fric, int NT) {
  const bool big = NT > kNwtThreads;
  return ((((size_t)7 * V + (size_t)nwt_window_doubles(V, NT) + 2 * (NT / 64) + 2 + (fric ? (size_t)4 * V : 0)) * sizeof(double) +
           ((size_t)15 * V + (fric ? (size_t)6 * V : 0)) * sizeof(float) +
           ((big ? 0 : (size_t)4 * T + V + 1) + 2 * (size_t)V + NT) * sizeof(unsigned short)) + 15) & ~(size_t)15;
}

// block-wide sum with ONE barrier: wave partials go to one of two alternating LDS rows and every thread adds them in the
// same fixed order (the row written two calls ago cannot still be read: a barrier lies in between)
template <int NT>
__device__ __forceinline__ double block_sum1(double v, double* sh2 /* 2 x NT / 64 doubles */, int& phase) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  double* row = sh2 + (NT / 64) * (phase & 1);
  ++phase;
  if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += row[w];
  return s;
}

// The mesh constants of the NEXT window of a sweep of fem_newton_lds_kernel (each thread owns kNwtTpw tets of a window of NT): fetched
// while the current window is computed - the only global reads of a sweep.  One copy for the atomic and the window flavour.
template <int NT>
struct TetWindow {
  int vn[kNwtTpw][4];
  double Din[kNwtTpw][9], voln[kNwtTpw];
  __device__ __forceinline__ void fetch_first(const FemDev& m, int T, int tid) {  // window 0 (zeros past the last tet)
#pragma unroll
    for (int u = 0; u < kNwtTpw; ++u) {
      const int t = u * NT + tid;
      voln[u] = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) vn[u][k] = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) Din[u][k] = 0.0;
      if (t < T) load_tet_blk(m, t, vn[u], Din[u], voln[u]);
    }
  }
  // window j out (v, Di, vol), window j + 1 in
  __device__ __forceinline__ void take_and_fetch(const FemDev& m, int T, int j, int tid, int (&v)[kNwtTpw][4], double (&Di)[kNwtTpw][9],
                                                 double (&vol)[kNwtTpw]) {
#pragma unroll
    for (int u = 0; u < kNwtTpw; ++u) {
      vol[u] = voln[u];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[u][k] = vn[u][k];
#pragma unroll
      for (int k = 0; k < 9; ++k) Di[u][k] = Din[u][k];
      const int tn = (j + 1) * NT + u * NT + tid;
      if (tn < T) load_tet_blk(m, tn, vn[u], Din[u], voln[u]);
    }
  }
};

template <bool MESH, int NT>
__device__ __forceinline__ double env_energy_lds(const FemDev& m, const double* xl, const double x3[3], const double* xt,
                                                 bool own, bool c, const double* aim, double* sh, int& phase,
                                                 const IndMesh& im, const double* ind = nullptr, double wv = 0.0, const double* fv = nullptr,
                                                 const double* xn = nullptr, const double* disp = nullptr, const double* e_tets = nullptr) {
  // e_tets: this thread's share of the elastic energy, already summed over the same tets in the same order by the gradient sweep of the
  // Newton iteration (same x): the line search's E(x) then costs no tet sweep of its own - and is the same bits as with one
  double e = e_tets ? *e_tets : 0.0;
  const double dt2 = m.dt * m.dt;
  for (int t = threadIdx.x; t < (e_tets ? 0 : m.T); t += blockDim.x) {
    int v[4];
    double Di[9], F[9];
    double vol_t;
    load_tet_blk(m, t, v, Di, vol_t);
    deformation_gradient(xl, v, Di, F);
    TetState s;
    tet_state(m, F, s);
    e += dt2 * vol_t * psi_of(m, s);
  }
  if (own) {
    const int v = threadIdx.x;
    const double mv = m.mass[v];
    double q = 0.0, qc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double d = x3[i] - xt[v * 3 + i];
      q += d * d;
      if (c) { const double cc = x3[i] - aim[v * 3 + i]; qc += cc * cc; }
    }
    e += 0.5 * mv * q + 0.5 * m.strength * mv * qc;
    if (ind) e += dt2 * contact_eval<MESH>(m, im, ind, wv, x3, false).e;
    if (fv) {
      const double xn3[3] = {xn[v * 3], xn[v * 3 + 1], xn[v * 3 + 2]};
      e += dt2 * friction_eval(m.fric_mu, m.fric_eps, fv + v * 4, x3, xn3, disp, false).e;
    }
  }
  return block_sum1<NT>(e, sh, phase);
}

// block-wide minimum, same one-barrier scheme as block_sum1
template <int NT>
__device__ __forceinline__ double block_min1(double v, double* sh2, int& phase) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  double* row = sh2 + (NT / 64) * (phase & 1);
  ++phase;
  if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = row[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) s = fmin(s, row[w]);
  return s;
}

// Backtracking beyond the configured cap: when the capped search (LineSearch.max_iter, US:96-101) finds no decrease the step is
// halved further, down to 2^-kLsRescue - a Newton direction computed BEFORE a vertex enters the barrier zone knows nothing of
// the barrier it runs into (soft gel, 10 GPa contact resistance: the admissible step can be 1e-3 of the CCD bound), and an env
// whose search failed would otherwise repeat the same failing iteration until the iteration cap.
constexpr int kLsRescue = 32;
// PSD-SAFE MODE.  The Stable Neo-Hookean Hessian is applied matrix-free and unprojected: aI + b f f^T + lam c c^T + c_J d2J/dF2, whose last
// term is indefinite (eigenvalues +-sigma_k).  On the gelpad - a thin pad held on its whole back face - the sum stays positive definite
// along the directions the PCG visits; a slender body bent by its indenter (simple_axle held at its ends) has compressed elements with
// negative curvature, the PCG breaks off on its first direction, and with a coarse correction in M^-1 that direction is a soft global
// mode hundreds of metres long: the Newton loop crawls into inverted states (replayed in the oracle: 40 iterations, then 6 mm of
// "dent" on a 3 mm rod).  IPC projects every element Hessian onto the PSD cone; here an env that MEETS negative curvature (p^T H p <= 0)
// switches, for that Newton iteration (which starts over), to a Hessian in which |c_J| is clamped to a / sqrt(2 Ic) per element: the spectral norm of
// d2J/dF2 is below sqrt(2 Ic) (its eigenvalues are +-sigma_k and those of the scaling block, bounded by the sum of two singular
// values), so a I + c_J d2J/dF2 stays positive semi-definite and with it the element Hessian.  The gradient is untouched - the
// iteration becomes a quasi-Newton one on the same minimiser - and envs that never meet negative curvature never pay.
// The PCG stops on the M^-1 norm of the residual, and M^-1 contains the coarse operator of the REST state - without the barrier and
// friction stiffness of the current contacts.  Where the coarse space holds nearly free modes (a slender body held at its ends:
// simple_axle) those modes map the contact forces in b to a huge b^T M^-1 b, the relative test passes after a handful of iterations
// with the 2-norm of the residual ABOVE that of b (measured at exit: 3.7 x |b| in the median there; on the gelpad, whose back face
// is held, <= 0.004 x |b| with the test on the norm of rounds 1-4 and a few per cent with libuipc's test on r.z), and the Newton loop crawls on such directions until a line search fails.  Safeguard: if the
// residual's 2-norm at exit is above kCoarseTrust x |b| - no reduction at all -, the env drops the coarse correction for the rest of the time step (chains /
// block Jacobi alone: the test is then in a norm that sees the contact blocks) and the iteration starts over.
constexpr double kCoarseTrust = 1.0;

// One launch = up to `max_newton` Newton iterations of every env (tacex_fem_step: the whole Newton loop of world.advance(),
// US:250-252, without a host round trip; tacex_fem_newton_step: max_newton = 1).  An env leaves the loop when the Newton
// direction of an iteration moves no vertex by more than dx_tol (velocity_tol * dt, US:62-66) - the criterion looks at the UNSCALED
// direction (IPC's test on the search direction): a CCD- or search-shortened update says nothing about convergence.
// ATOM: per-tet rows are ADDED into per-vertex LDS accumulators with ds_add_f64 instead of travelling through the 48 KB exchange
// window and a CSR gather: 2 barriers per sweep instead of 8, no gather phase, and the atomics of one tet batch overlap the f64
// arithmetic of the next (no barrier between batches: wave skew no longer costs).  The price is the summation ORDER of a vertex's
// ~24 contributions, which then depends on the timing of the waves: results agree to round-off (1e-16 relative per add), not
// bit for bit from run to run.  `tacex_fem_set_deterministic(ctx, 1)` selects the window path (ATOM = false).
template <bool MESH, bool ATOM, int NT, bool MAT>
__global__ __launch_bounds__(NT) void fem_newton_lds_kernel(FemDev m, double* xg, const double* xtg,
                                                                     const uint8_t* consg, const double* aimg, double* stats,
                                                                     int pcg_max_iter, double pcg_tol_rate, int ls_max_iter,
                                                                     double* dxg, double dx_tol, int max_newton, double* step_info,
                                                                     const double* xprevg, const double* dispg, const int* env_order,
                                                                     int follow, double* lagg, FemMat mat) {
  extern __shared__ __attribute__((aligned(16))) double nlds[];
  constexpr int CH = NT;  // tets per pass of a sweep (one per thread) = tets per exchange window
  constexpr bool BIG = NT > kNwtThreads;  // meshes of more than 512 vertices: see nwt_lds_bytes
  static_assert(!BIG || ATOM, "the wide variants exist in the atomic flavour only");
  const int V = m.V, T = m.T;
  const int wave_s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int tid = fresh_tid(wave_s);
  double* xs = nlds;            // (V,3) current x
  double* ps = xs + 3 * V;      // (V,3) PCG direction p, later the line-search candidate
  double* hv = ps + 3 * V;      // (12, CH) per-tet rows of the current window | accumulators, exchange arrays (nwt_window_doubles)
  double* sh = hv + nwt_window_doubles(V, NT);  // 2 x NT / 64 wave partials of block_sum1 (+2 pad)
  // friction (tacex_fem_step with a friction ratio): (V,4) lagged normal force and normal, (V,6) Hessian blocks (floats)
  // (this is still the SCENE's friction switch - with a material library the largest ratio of the library, what the host sized the
  // allocation with: the LDS layout is one for all envs; whether THIS env has friction follows its own material: `fric` below)
  const bool fric_lds = m.indenters && m.area && m.fric_mu > 0.0 && xprevg != nullptr && dispg != nullptr;  // (xprevg is only handed over with friction)
  double* fl = sh + 2 * (NT / 64) + 2;
  double* mdl = fl + (fric_lds ? 4 * V : 0);  // (V) diagonal mass term m_v (1 + s c_v): read back per PCG iteration (per-thread constants
                                              // carried in registers across the tet arithmetic went to scratch)
  float* cf = reinterpret_cast<float*>(mdl + V);  // (V,15) chain factors: S^-1 (6, upper triangle) | G (9)
  float* fh = cf + 15 * V;
  unsigned short* csr = reinterpret_cast<unsigned short*>(fh + (fric_lds ? 6 * V : 0));  // (4T) incidence codes tet * 4 + local, vertex-major
  unsigned short* cnx = csr + (BIG ? 0 : 4 * T);  // (V) chain successor | (V) predecessor, 0xffff = none
  unsigned short* cpv = cnx + V;
  unsigned short* chd = cpv + V;      // (NT) head vertex of the chain thread t factors and solves, 0xffff = none
  unsigned short* vto = chd + NT;  // (V+1) CSR offsets of the incidence codes (4 T < 65535); like csr not there in the wide variants
  int phase = 0;  // block_sum1 row toggle
  // env_order: envs sorted by the solver work of their PREVIOUS time step, heaviest first (fem_env_order_kernel).  One env
  // occupies one CU for its whole Newton loop and a shard brings several envs per CU, so the launch ends with whatever the
  // last-started envs need: started in index order, the heavy envs of a scene may all come last.  Workgroups are dispatched
  // in blockIdx order, so this is longest-processing-time-first list scheduling with last step's cost as the estimate.
  const int b = env_order ? env_order[blockIdx.x] : (int)blockIdx.x;
  if (dxg && dxg[b] <= dx_tol) {  // this env's last update was below the Newton tolerance (uipc_sim.py:62-66): nothing to do
    if (threadIdx.x == 0) { stats[(size_t)b * 4 + 2] = 0.0; stats[(size_t)b * 4 + 3] = 0.0; }
    return;
  }
  const bool mat_bad = env_material<MAT>(m, mat, b);  // (looked up with the env b, not with blockIdx.x: env_order)
  const size_t o = (size_t)b * V * 3;
  double* x = xg + o;
  const double* xt = xtg + o;
  const double* aim = aimg ? aimg + o : nullptr;
  const bool own = tid < V;
  const bool c = own && consg && consg[(size_t)b * V + tid];
  const double dt2 = m.dt * m.dt;
  const int nchunk = (T + CH - 1) / CH;
  const double mv = own ? m.mass[tid] : 0.0;
  const double md = mv * (1.0 + (c ? m.strength : 0.0));
  // contact: this vertex's weight and the env's indenter (nullptr: contact off)
  const double* ind = (m.indenters && m.area) ? m.indenters + (size_t)b * 8 : nullptr;
  const double wv = (ind && own) ? m.area[tid] : 0.0;
  bool mesh_bad;
  const IndMesh im = env_mesh<MESH>(m, b, ind, mesh_bad);
  // friction needs the positions the step started from: tacex_fem_step only
  const bool fric = ind && m.fric_mu > 0.0 && xprevg != nullptr && dispg != nullptr;
  const double* xn = fric ? xprevg + o : nullptr;
  double disp3[3] = {0, 0, 0};
  if (ind && dispg) { disp3[0] = dispg[b * 3]; disp3[1] = dispg[b * 3 + 1]; disp3[2] = dispg[b * 3 + 2]; }

  double x3[3] = {0, 0, 0};
  if (own) {
#pragma unroll
    for (int i = 0; i < 3; ++i) x3[i] = x[tid * 3 + i];
    // CONTACT-FOLLOWING START of the Newton loop (tacex_fem_step, `follow`): a surface vertex the indenter RETREATS from (its surface
    // moves away along the vertex's contact normal: disp . n < 0) and that sat inside the barrier zone before the move starts the
    // iteration displaced by that normal component, x += (disp . n) n - back at the gap it had.  Only the initial guess changes; the
    // minimiser of the step's incremental potential is what it was.  Without it a retreating indenter leaves its contact vertices
    // outside the zone, the first Newton direction springs the dent back by a millimetre into a barrier that is a hard wall for this
    // soft gel, the line search cuts the step to 1e-3 and the contact set is rediscovered a ring of vertices per iteration: 4-5 Newton
    // iterations of ~25 PCG iterations per env and step (stragglers: 17-32 iterations, 1 000-1 800 PCG iterations on ONE CU, and the
    // launch waits for them) against 2 iterations of 2 while the indenter presses.  Where the indenter APPROACHES (disp . n >= 0)
    // nothing is moved: the shrunken gap raises the barrier force and that start already converges in two iterations (following
    // there was measured: the over-displaced surface has to come back up into the barrier and line searches fail).
    if ((follow & 1) && ind && wv > 0.0 && (disp3[0] != 0.0 || disp3[1] != 0.0 || disp3[2] != 0.0)) {
      const ContactEval c0 = contact_eval<MESH>(m, im, ind, wv, x3);
      const double dn = disp3[0] * c0.n[0] + disp3[1] * c0.n[1] + disp3[2] * c0.n[2];
      if (dn < 0.0 && !c0.penetrating && c0.d < 1e299) {
        const double xm[3] = {x3[0] + dn * c0.n[0], x3[1] + dn * c0.n[1], x3[2] + dn * c0.n[2]};
        const ContactEval cf = contact_eval<MESH>(m, im, ind, wv, xm);
        if (cf.active && !cf.penetrating) { x3[0] = xm[0]; x3[1] = xm[1]; x3[2] = xm[2]; }
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) xs[tid * 3 + i] = x3[i];
  }
  if constexpr (!BIG)
    for (int k = tid; k < 4 * T; k += NT) csr[k] = (unsigned short)m.vt_idx[k];
  if (own) {
    cnx[tid] = (unsigned short)(m.ch_next ? m.ch_next[tid] : -1);
    cpv[tid] = (unsigned short)(m.ch_prev ? m.ch_prev[tid] : -1);
  }
  const int nch = m.ch_next ? m.nch : V;
  // the chain a thread factors and solves: chains are dealt from the TOP thread down, so that their solves overlap the coarse
  // solve, which keeps the low threads busy.  The head vertex is looked up in LDS where it is needed (chain_head).
  {
    const int my_chain = NT - 1 - tid;
    chd[tid] = (unsigned short)(my_chain < nch ? (m.ch_next ? m.ch_head[my_chain] : my_chain) : 0xffff);
    if constexpr (!BIG)
      for (int k = tid; k <= V; k += NT) vto[k] = (unsigned short)m.vt_off[k];
    if (own) mdl[tid] = md;
  }
  auto chain_head = [&](int t) -> int { const int h = chd[t]; return h == 0xffff ? -1 : h; };
  __syncthreads();

#ifdef TACEX_FEM_CLOCK  // debug build: cycles (s_memtime) of the sections of a PCG iteration, group TACEX_FEM_CLOCK of four -> stats
  double fclk[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double fnw[4] = {0, 0, 0, 0};  // group 3: phases of a Newton iteration [gradient, block assembly + factorisation, PCG, line search]
  long long ftk = 0;
#define FEM_TICK(k) do { const long long now_ = __builtin_readcyclecounter(); fclk[k] += (double)(now_ - ftk); ftk = now_; } while (0)
#define FEM_TICK0() do { ftk = __builtin_readcyclecounter(); } while (0)
#else
#define FEM_TICK(k) do { } while (0)
#define FEM_TICK0() do { } while (0)
#endif
  // one sweep over the tets in windows of CH = kNwtTpw x 512: `make(v, Di, vol, rows)` fills the 12 rows of a tet (each thread
  // owns kNwtTpw independent tets of the window), then vertex `tid` adds the rows of its incident tets inside the window
  // (CSR entries are sorted by tet, so a cursor suffices).  The mesh constants of the NEXT window are fetched while this
  // window is computed and gathered (they are the only global reads of the sweep).
  // pre_zeroed (ATOM only): the caller has zeroed the accumulators before a barrier of its own (saves the sweep's first barrier)
  auto sweep = [&](auto&& make, double acc[3], bool pre_zeroed = false) {
    if constexpr (ATOM) {
      const int tid_a = fresh_tid(wave_s);
      double* av = hv;  // (V,3) accumulators at the head of the (otherwise idle) window region
      if (!pre_zeroed && tid_a < V) { av[tid_a * 3] = 0.0; av[tid_a * 3 + 1] = 0.0; av[tid_a * 3 + 2] = 0.0; }
      TetWindow<NT> nx;
      nx.fetch_first(m, T, tid_a);
      if (!pre_zeroed) __syncthreads();  // accumulators zeroed (and every reader of the window region's previous content is past it)
      for (int j = 0; j < nchunk; ++j) {
        int v[kNwtTpw][4];
        double Di[kNwtTpw][9], vol[kNwtTpw];
        nx.take_and_fetch(m, T, j, tid_a, v, Di, vol);
#pragma unroll
        for (int u = 0; u < kNwtTpw; ++u) {
          if (j * CH + u * NT + tid_a < T) {
            double rows[12];
            make(v[u], Di[u], vol[u], rows);
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
              for (int i = 0; i < 3; ++i) atomicAdd(&av[v[u][w] * 3 + i], rows[w * 3 + i]);
          }
        }
      }
      __syncthreads();
      acc[0] = tid_a < V ? av[tid_a * 3] : 0.0; acc[1] = tid_a < V ? av[tid_a * 3 + 1] : 0.0; acc[2] = tid_a < V ? av[tid_a * 3 + 2] : 0.0;
      return;
    }
    const int tid_s = fresh_tid(wave_s);
    int e = tid_s < V ? (int)vto[tid_s] : 0;
    const int e_end = tid_s < V ? (int)vto[tid_s + 1] : 0;
    int code = e < e_end ? (int)csr[e] : 0x7fffffff;
    int code1 = e + 1 < e_end ? (int)csr[e + 1] : 0x7fffffff;
    acc[0] = acc[1] = acc[2] = 0.0;
    TetWindow<NT> nx;
    nx.fetch_first(m, T, tid_s);
    for (int j = 0; j < nchunk; ++j) {
      FEM_TICK0();
      int v[kNwtTpw][4];
      double Di[kNwtTpw][9], vol[kNwtTpw];
      nx.take_and_fetch(m, T, j, tid_s, v, Di, vol);
#pragma unroll
      for (int u = 0; u < kNwtTpw; ++u) {
        const int tl = u * NT + tid;
        if (j * CH + tl < T) {
          double rows[12];
          make(v[u], Di[u], vol[u], rows);
#pragma unroll
          for (int k = 0; k < 12; ++k) hv[k * CH + tl] = rows[k];
        }
      }
      FEM_TICK(8);
      __syncthreads();
      FEM_TICK(9);
      const int tend4 = (j + 1) * CH * 4;
      // `code` / `code1` always hold entries e and e + 1 (INT_MAX past the list).  Two entries of the window are gathered per
      // round trip where there are two - their six rows are in flight together and are added in entry order - so a vertex
      // pays one LDS latency per PAIR of incident tets (a vertex has ~4 per window)
      while (code1 < tend4) {
        const int l0 = code & 3, t0 = (code >> 2) - j * CH, l1 = code1 & 3, t1 = (code1 >> 2) - j * CH;
        e += 2;
        const int n0 = e < e_end ? (int)csr[e] : 0x7fffffff;
        const int n1 = e + 1 < e_end ? (int)csr[e + 1] : 0x7fffffff;
        const double h00 = hv[(l0 * 3 + 0) * CH + t0], h01 = hv[(l0 * 3 + 1) * CH + t0], h02 = hv[(l0 * 3 + 2) * CH + t0];
        const double h10 = hv[(l1 * 3 + 0) * CH + t1], h11 = hv[(l1 * 3 + 1) * CH + t1], h12 = hv[(l1 * 3 + 2) * CH + t1];
        acc[0] += h00; acc[1] += h01; acc[2] += h02;
        acc[0] += h10; acc[1] += h11; acc[2] += h12;
        code = n0; code1 = n1;
      }
      if (code < tend4) {
        const int l = code & 3, tl = (code >> 2) - j * CH;
        ++e;
        acc[0] += hv[(l * 3 + 0) * CH + tl];
        acc[1] += hv[(l * 3 + 1) * CH + tl];
        acc[2] += hv[(l * 3 + 2) * CH + tl];
        code = code1;
        code1 = e + 1 < e_end ? (int)csr[e + 1] : 0x7fffffff;
      }
      FEM_TICK(10);
      if (j + 1 < nchunk) __syncthreads();
      FEM_TICK(11);  // the window is rewritten; after the last one the caller's next barrier suffices
    }
  };

  int n_newton = 0, flags = 0;
  bool done = false;
  double pcg_total = 0.0, dmax_last = INFINITY;
  // warm start of the next iteration's PCG: the part of this iteration's Newton direction the CCD filter / the line search cut off
  // (the direction is parked in the env's workspace block, behind the (V,16) preconditioner blocks: it is written once and read at most
  //  once per Newton iteration - as three more live f64 registers across the PCG loop it was part of what the allocator sent to scratch)
  double* const dprev_g = lagg + (size_t)gridDim.x * 16 * V + ((size_t)b * V + (own ? tid : 0)) * 3;
  double frac_prev = 0.0;  // (1 - accepted step) of the previous iteration, 0 when it was taken in full or rejected
  // FRICTION LAG AT THE START OF THE STEP (`follow` bit 1, the default): normal force and normal are taken in the FIRST iteration, at the
  // state the step starts from - IPC's lag "from the previous time step" (Li et al. 2020, section 5.4): that state is the previous step's
  // equilibrium, whose contact reaction is the previous normal force - and friction acts from the first iteration on.  Bit clear: the lag is
  // taken where the normal-contact solve of THIS step converged, in an iteration of its own (rounds 3-4: one more Newton iteration per step
  // with contact - a pressing step is two iterations instead of one).
  const bool lag_at_start = (follow & 2) != 0;
  bool fric_phase = fric && lag_at_start;   // friction terms are on (see friction_eval)
  bool lag_pending = fric && lag_at_start;  // the friction lag is taken in this iteration (behind the gradient and the contact evaluation)
  bool use_coarse = m.nc > 0;  // (block-uniform) false once the safeguard of kCoarseTrust has fired
  bool psd_safe = false;       // (block-uniform) see kFemFlagPsdSafe
  for (int nit = 0; nit < max_newton; ++nit) {
  if (nit > 0) __syncthreads();  // xs carries the accepted candidate of the previous iteration
  bool snapped_once = false;     // the edge snap (below) restarts an iteration at most once
  // every iteration tries the exact Hessian first: near the minimiser it is what converges quadratically.  (Measured against keeping
  // the mode for the rest of the step - faster on the axle, 273 against 441 ms, but its last iterations converge linearly and stop on
  // the tolerance 50 um from the minimiser - and against keeping it until a full step is accepted: gelpad scene 3.08 against 2.91 ms.)
  psd_safe = false;
restart_iteration:
#ifdef TACEX_FEM_CLOCK
  long long fph = __builtin_readcyclecounter();
#define FEM_PHASE(k) do { const long long n_ = __builtin_readcyclecounter(); fnw[k] += (double)(n_ - fph); fph = n_; } while (0)
#else
#define FEM_PHASE(k) do { } while (0)
#endif
  // ---- nodal gradient ----
  double r3[3], d3[3] = {0, 0, 0};
  double go3[3] = {0, 0, 0};  // gradient WITHOUT the contact terms (inertia + elasticity + constraints): the reaction a contact balances
  double e_tets = 0.0;  // this thread's tets' elastic energy at x: by-product of the gradient sweep, E(x) of the line search below
  {
    double a3[3];
    sweep([&](const int* v, const double* Di, double vol, double* g) {
      double F[9], r[12];
      deformation_gradient(xs, v, Di, F);
      TetState s;
      tet_state(m, F, s);
      e_tets += dt2 * vol * psi_of(m, s);
      shape_rows(Di, r);
      element_gradient(s, r, dt2 * vol, g);
    }, a3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double gi = 0.0;
      if (own) {
        gi = a3[i] + mv * (x3[i] - xt[tid * 3 + i]);
        if (c) gi += m.strength * mv * (x3[i] - aim[tid * 3 + i]);
      }
      r3[i] = -gi;
      go3[i] = gi;
    }
  }
  // barrier of this vertex at x: gradient b1 n, curvature b2 n n^T (the b1 * hess(d) part is negative semi-definite for a
  // convex indenter and dropped: the usual PSD projection of IPC)
  const ContactEval ce = contact_eval<MESH>(m, im, ind, wv, x3);
  if (ce.penetrating) flags |= kFemFlagPenetration;  // (per thread; or-reduced into step_info at the end)
  if (ce.active) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r3[i] -= dt2 * ce.b1 * ce.n[i];
  }
  const double cb2 = ce.active ? dt2 * ce.b2 : 0.0;
  // FRICTION LAG (normal force lam, normal n per vertex), taken once per step at the state the normal-contact solve converged to:
  // lam = min(-dB/dd, reaction), reaction = (g_other . n) / dt^2 = the normal force that balances inertia + elasticity + constraints
  // at this vertex.  In force balance the two agree (that IS the balance); but the Newton loop stops on its step-size tolerance
  // (velocity_tol * dt = 0.5 mm, US:62-66), where a contact vertex may still sit at 0.98 d_hat - and there the 10 GPa barrier pushes
  // with 87 N on a pad whose whole reaction is below 1 N.  Lagging THAT force made the first friction iteration's direction 0.66 m
  // long and the env spend 34 Newton / 1 900 PCG iterations on one CU while the launch waited (scene step 11, env 442; replayed
  // through the oracle in tests/studies/fem_straggler_replay.py: 38 / 2 280 -> 5 / 21 with the cap).
  if (lag_pending) {  // (block-uniform; every thread writes and later reads its own four doubles: no barrier)
    lag_pending = false;
    double lam = 0.0;
    if (own) {
      double ln[3] = {ce.n[0], ce.n[1], ce.n[2]};
      if (follow & 4) lam = friction_lag_ipc<MESH>(m, im, ind, wv, disp3, xn + tid * 3, ln);  // (tacex_fem_set_friction_lag, mode 1)
      else if (ce.active) lam = friction_lag_capped(ce, go3, dt2);
      const bool on = lam > 0.0;
      fl[tid * 4] = on ? lam : 0.0;
      fl[tid * 4 + 1] = on ? ln[0] : 0.0; fl[tid * 4 + 2] = on ? ln[1] : 0.0; fl[tid * 4 + 3] = on ? ln[2] : 0.0;
    }
    if (!__syncthreads_or(lam > 0.0)) {  // no vertex carries a normal force: nothing for friction to act on
      if (!lag_at_start) { done = true; break; }  // (two-phase mode: normal contact had converged, the step is done)
      fric_phase = false;                         // (lag at the start: this step runs without friction)
    }
  }
  // friction of this vertex at x: gradient into the residual, Hessian block into LDS (read back by H.p and the preconditioner)
  if (fric_phase && own) {
    const double xn3[3] = {xn[tid * 3], xn[tid * 3 + 1], xn[tid * 3 + 2]};
    const FricEval fe = friction_eval(m.fric_mu, m.fric_eps, fl + tid * 4, x3, xn3, disp3, true);
#pragma unroll
    for (int i = 0; i < 3; ++i) r3[i] -= dt2 * fe.g[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) fh[tid * 6 + k] = (float)(dt2 * fe.h[k]);
  }
  FEM_PHASE(0);
  // ---- block part of the preconditioner: block-tridiagonal LDL^T along vertex chains (tacex_fem_set_chains; a chain of one
  //      vertex = 3x3 block Jacobi).  Every vertex assembles its diagonal block D and the block E = A(v, next(v)) towards its
  //      chain successor (columns recomputed per incident tet), the blocks meet in LDS (the idle p / window region), and the
  //      thread of a chain walks it:  S_0 = D_0,  G_i = S_i^-1 E_i,  S_{i+1} = D_{i+1} - E_i^T G_i.  S^-1 (6) and G (9) stay in
  //      LDS as FLOATS: z = L^-T S^-1 L^-1 r is symmetric positive definite for any G as long as the S^-1 are, so the rounding
  //      costs preconditioner quality only (none measurable: profiles/r03_experiments.md section 9). ----
  //      The ELASTIC part of D and E is assembled in the FIRST iteration of a launch only and kept per env in the workspace (15
  //      doubles per vertex, SoA): between the Newton iterations of one time step the deformation gradients move by per cent, the
  //      blocks that change by orders of magnitude - barrier curvature, friction - are added fresh every iteration, and a
  //      preconditioner only has to stay SPD.  The assembly was 164 K of the 333 K cycles of an iteration in steady contact
  //      (section clock, profiles/r04_experiments.md), and every step with contact runs at least two iterations (normal contact,
  //      then friction).
  {
    double D[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // elastic part of D / E: assembled for ALL envs of the launch by fem_assemble_blocks_kernel ahead of this kernel, at the state the
    // launch starts from, (V,16) per env in the workspace (round 5; rounds 3-4 assembled it here in the first iteration of a launch -
    // 111 K of a pressing step's 268 K cycles, and the part of this kernel the register allocator spilled most for)
    if (own) {
      // one 128-byte record per vertex: D upper triangle (6) | E (9) | pad - ONE address (rebuilt here from a fresh thread id, never
      // carried across the PCG loop: fifteen hoisted [15][V] row addresses were 30 of the kernel's spilled registers)
      const double* q = lagg + ((size_t)b * V + (size_t)fresh_tid(wave_s)) * 16;
      D[0] = q[0]; D[1] = q[1]; D[2] = q[2]; D[4] = q[3]; D[5] = q[4]; D[8] = q[5];
      D[3] = D[1]; D[6] = D[2]; D[7] = D[5];
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = q[6 + k];
      // the blocks that are never lagged: mass + constraint, barrier curvature, friction
      D[0] += md; D[4] += md; D[8] += md;
    }
    // EDGE SNAP: one exact 1-D minimisation per surface vertex that is about to run into the barrier zone from outside (or sits in its
    // outermost sliver), along its contact normal - a nonlinear Gauss-Seidel sweep over the stiffest degrees of freedom, taken before
    // the Newton system of the iteration is set up.  The barrier is C2 with b'' -> 0 at d_hat: the Newton system is blind to it for
    // such a vertex, its direction sends the vertex a millimetre deep into a wall that stops it within microns, the line search cuts
    // the step OF THE WHOLE MESH to a per cent and the next iteration repeats it (the apex vertex of a retreating contact crossed the
    // zone edge back and forth for 13 iterations with max |d| 0.6-0.8 mm against a tolerance of 0.5 mm: 18 Newton / 530 PCG
    // iterations for that env, the launch waiting; with the snap 4 / 160 - tests/studies/fem_straggler_replay.py).  Along n the
    // vertex's energy is  phi(t) = -(g.n) t + 1/2 (n.D n) t^2 + dt^2 kappa A b((gap - t) / d_hat)  (g = contact-free gradient, D =
    // the block above): if the elastic 1-D Newton step t_el = g.n / n.D n reaches the zone, the vertex moves to where the barrier
    // balances the force it has to carry, e = sqrt(lam d_hat / (3 kappa A)) below d_hat (b' ~ -3 e^2 near the edge, lam = g.n / dt^2),
    // never further than t_el.  The iteration then restarts from the moved state (gradient, contact, blocks from the lag).
    if (ind && !snapped_once) {  // (block-uniform)
      double tmove = 0.0;
      if (own && wv > 0.0 && !ce.penetrating && ce.d < 1e299) {
        const double gn = go3[0] * ce.n[0] + go3[1] * ce.n[1] + go3[2] * ce.n[2];
        if (gn > 0.0) {
          double nDn = 0.0;
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) nDn += ce.n[i] * D[i * 3 + k] * ce.n[k];
          const double t_el = nDn > 0.0 ? gn / nDn : 0.0;
          const double e = fmin(fmax(sqrt(gn / dt2 * m.dhat / (3.0 * m.kappa * wv)), 1e-6), 1e-2);
          const double rest = ce.d - (1.0 - e) * m.dhat;  // distance to the balance depth
          if (rest > 0.0 && t_el > ce.d - m.dhat) tmove = fmin(t_el, rest);
        }
      }
      if (__syncthreads_or(tmove > 0.0)) {
        if (tmove > 0.0) {
#pragma unroll
          for (int i = 0; i < 3; ++i) { x3[i] -= tmove * ce.n[i]; xs[tid * 3 + i] = x3[i]; }
        }
        snapped_once = true;
        __syncthreads();
        goto restart_iteration;
      }
    }
    if (own) {
      if (fric_phase) {
        const float* h = fh + tid * 6;
        D[0] += h[0]; D[1] += h[1]; D[2] += h[2]; D[3] += h[1]; D[4] += h[3]; D[5] += h[4]; D[6] += h[2]; D[7] += h[4]; D[8] += h[5];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) D[i * 3 + k] += cb2 * ce.n[i] * ce.n[k];
    }
    double* xch = ps;  // (V,15) D (upper triangle) | E: p is idle until the PCG starts, the window once the gradient is gathered
    __syncthreads();   // every vertex has gathered the last window of the gradient sweep
    if (own) {
      double* q = xch + tid * 15;
      q[0] = D[0]; q[1] = D[1]; q[2] = D[2]; q[3] = D[4]; q[4] = D[5]; q[5] = D[8];
#pragma unroll
      for (int k = 0; k < 9; ++k) q[6 + k] = E[k];
    }
    __syncthreads();
    const int my_head = chain_head(tid);
    if (my_head >= 0)
      chain_factor(my_head,
                   [&](int v, double (&Dv)[9]) __attribute__((always_inline)) {
                     const double* q = xch + v * 15;
                     Dv[0] = q[0]; Dv[1] = q[1]; Dv[2] = q[2]; Dv[3] = q[1]; Dv[4] = q[3]; Dv[5] = q[4]; Dv[6] = q[2]; Dv[7] = q[4]; Dv[8] = q[5];
                   },
                   [&](int v, const double*& Ev) __attribute__((always_inline)) { Ev = xch + v * 15 + 6; return true; }, cf, cnx);
    __syncthreads();  // factors complete; the exchange region goes back to the PCG
  }
  // ---- preconditioner: z = D^-1 r (3x3 block Jacobi) + P A_c^-1 P^T r (additive coarse-grid correction) ----
  // Block Jacobi alone needs 120-330 PCG iterations on the thin, nearly incompressible pad: the error it cannot reach is
  // smooth over many elements.  The coarse space - trilinear hats of a small grid over the mesh, <= 64 nodes - carries those
  // modes; its operator is the Galerkin product with the REST-state matrix (constant per mesh and constraint set: factored on
  // the host once, profiles/r03_experiments.md section 4 shows it works as well as the current-state product).  Restriction is
  // a gather per coarse dof over its support, split over G threads with the partial sums added in a fixed order (deterministic,
  // no atomics); the sweep's LDS window is idle between two sweeps and carries r, the partial sums and the coarse vectors.
  const int nc3 = 3 * m.nc;
  // Gn lanes per coarse NODE for the restriction, H lanes per coarse dof for the coarse solve: powers of two that divide a wave, so
  // the partial sums of a node / dof sit in ONE wave and are added by a butterfly of lane exchanges - no LDS round trip, no barrier
  // (a fixed tree: deterministic)
  auto pow2_le = [](int v) { int p = 1; while (2 * p <= v && 2 * p <= 64) p *= 2; return p; };
  const int Gn = m.nc > 0 ? pow2_le(NT / m.nc) : 1;
  const int H = nc3 > 0 ? pow2_le(NT / nc3) : 1;
  const int Q = nc3 > 0 ? (nc3 + H - 1) / H : 0;
  auto apply_prec = [&](const double (&r)[3], double (&z)[3]) {
    double* rs = hv;                        // (V,3) residual
    double* rc = hv + 3 * V;                // (3 nc) restricted residual
    double* yc = rc + 3 * kFemMaxCoarse;    // (3 nc) coarse correction
    double* zs = yc + 3 * kFemMaxCoarse;    // (V,3) chain solve: y on the way down, z on the way back
    z[0] = z[1] = z[2] = 0.0;
    FEM_TICK(2);
    __syncthreads();  // every thread is done with the window of the last sweep
    const int tid_p = fresh_tid(wave_s);  // (fresh_tid: the LDS / table offsets below are rebuilt per application, never carried)
    const bool own_p = tid_p < V;
    if (own_p) {
#pragma unroll
      for (int i = 0; i < 3; ++i) rs[tid_p * 3 + i] = r[i];
    }
    __syncthreads();
    FEM_TICK(3);
    auto solve_my_chain = [&]() {  // rs -> zs, by the chain's thread
      const int my_head = chain_head(tid_p);
      if (my_head < 0) return;
      chain_solve<false>(my_head, rs, zs, cf, cnx, cpv);
    };
    if (nc3 == 0 || !use_coarse) {
      solve_my_chain();
      __syncthreads();
      if (own_p) {
#pragma unroll
        for (int i = 0; i < 3; ++i) z[i] = zs[tid_p * 3 + i];
      }
      return;
    }
    restrict_to_coarse<true>(m, rs, rc, Gn, tid_p);
    __syncthreads();
    FEM_TICK(5);
    {  // coarse solve y = A_c^-1 r_c: H lanes per row, each over a slice of its (contiguous) row.  The chain solves run beside it
       // on the threads it leaves idle (chains are dealt from the top).
      const int dof = tid_p / H, h = tid_p - dof * H;
      double acc = 0.0;
      if (dof < nc3) {
        const int q1 = min(nc3, (h + 1) * Q);
        const unsigned row = (unsigned)(dof * nc3) * 8u;  // (3 nc)^2 doubles <= 288 KB: 32-bit byte offsets
        for (int q = h * Q; q < q1; ++q) acc += ldg_off<double>(m.ac_inv, row + (unsigned)q * 8u) * rc[q];
      }
      for (int o = H >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      if (dof < nc3 && h == 0) yc[dof] = acc;
    }
    solve_my_chain();
    __syncthreads();
    FEM_TICK(6);
    if (own_p) {
#pragma unroll
      for (int i = 0; i < 3; ++i) z[i] = zs[tid_p * 3 + i];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int node = ldg_off<int>(m.cv_node, (unsigned)tid_p * 32u + (unsigned)k * 4u);
        const double w = ldg_off<double>(m.cv_w, (unsigned)tid_p * 64u + (unsigned)k * 8u);
#pragma unroll
        for (int i = 0; i < 3; ++i) z[i] += w * yc[node * 3 + i];
      }
    }
    FEM_TICK(7);
  };
  FEM_PHASE(1);
  // ---- PCG ----
  // Stops when the preconditioned residual has dropped to tol_rate times that of the right-hand side (r^T M^-1 r against
  // b^T M^-1 b; the same test as before for a zero start).  WARM START: when the previous iteration's step was cut short (CCD
  // bound, backtracking at the edge of the barrier zone - the release regime of a retreating indenter takes up to the iteration
  // cap of such steps), the new system differs from the old one only around the newly pinned vertices, and the unfinished part
  // (1 - step) d_prev is a far better start than zero: one extra H.d sweep buys most of the iterations.
  double z3[3], p3[3];
  double part = 0.0;
  apply_prec(r3, z3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p3[i] = z3[i];
    part += r3[i] * z3[i];
  }
  const double rz_b = block_sum1<NT>(part, sh, phase);
  double bb = 0.0;  // |b|^2, for the safeguard of kCoarseTrust
  if (use_coarse) bb = block_sum1<NT>(r3[0] * r3[0] + r3[1] * r3[1] + r3[2] * r3[2], sh, phase);
  double rz = rz_b;
  bool warm = frac_prev > 0.0 && rz_b > 0.0;
  const bool warm_used = warm;
  if (warm) {
#pragma unroll
    for (int i = 0; i < 3; ++i) d3[i] = own ? frac_prev * dprev_g[i] : 0.0;
  }
  int it = 0;
  bool neg_curv = false;
  // Stopping test as libuipc's linear_pcg runs it (src/backends/cuda/linear_system/linear_pcg.cu, LinearPCG::pcg: `abs(rz_new) <= global_tol_rate *
  // rz0`, global_tol_rate = linear_system/tol_rate, US:90): relative on r^T M^-1 r ITSELF, not on its square root - tol_rate 1e-3 is a factor 0.032
  // on the M^-1 norm of the residual.  (Rounds 1-4 tested the norm, tol_rate^2 on r.z: a thousand times stricter than the reference's own
  // solver and about twice the PCG iterations.)
  while (warm || (it < pcg_max_iter && rz_b > 0.0 && rz > pcg_tol_rate * rz_b)) {
    double q3[3] = {0, 0, 0};  // the vector H is applied to (d0 of the warm start, else p): lives in ps during the sweep
    const int tid = fresh_tid(wave_s);  // (shadows the kernel-wide copy: nothing derived from it crosses an iteration)
    FEM_TICK0();
    if (own) {
#pragma unroll
      for (int i = 0; i < 3; ++i) ps[tid * 3 + i] = warm ? d3[i] : p3[i];
      if constexpr (ATOM) { hv[tid * 3] = 0.0; hv[tid * 3 + 1] = 0.0; hv[tid * 3 + 2] = 0.0; }  // the sweep's accumulators (a block reduction's
                                                                                            // barrier lies behind the last reader of the region)
    }
    __syncthreads();
    // Hq = (M + s Mc + dt^2 K) q, matrix-free: per-tet dP[dF(q)] rows, gathered per vertex
    double a3[3];
    sweep([&](const int* v, const double* Di, double vol, double* rows) {
      double F[9], dF[9], dP[9], r[12];
      deformation_gradient(xs, v, Di, F);
      deformation_gradient(ps, v, Di, dF);  // linear in q
      TetState s;
      tet_state(m, F, s);
      if (psd_safe) {
        const double lim = s.a / sqrt(2.0 * fmax(s.Ic, 1e-300));
        s.c = fmin(fmax(s.c, -lim), lim);
      }
      apply_dP(m, s, dF, dP);
      shape_rows(Di, r);
      element_hp_rows(dP, r, dt2 * vol, rows);
    }, a3, ATOM);
    FEM_TICK(0);
    // (q is read back from LDS - the sweep leaves ps alone - rather than carried in registers across the tet arithmetic: the loop
    //  body holds ~250 live registers there, and every value carried across it went to scratch)
    double mdv = 0.0;
    if (own) {
#pragma unroll
      for (int i = 0; i < 3; ++i) q3[i] = ps[tid * 3 + i];
      mdv = mdl[tid];
    }
    double Hp3[3];
    part = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Hp3[i] = own ? a3[i] + mdv * q3[i] + cb2 * ce.n[i] * (ce.n[0] * q3[0] + ce.n[1] * q3[1] + ce.n[2] * q3[2]) : 0.0;
    }
    if (fric_phase && own) {
      const float* h = fh + tid * 6;
      Hp3[0] += h[0] * q3[0] + h[1] * q3[1] + h[2] * q3[2];
      Hp3[1] += h[1] * q3[0] + h[3] * q3[1] + h[4] * q3[2];
      Hp3[2] += h[2] * q3[0] + h[4] * q3[1] + h[5] * q3[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) part += q3[i] * Hp3[i];
    if (warm) {  // r = b - H d0, then the usual start from there (not counted as an iteration)
#pragma unroll
      for (int i = 0; i < 3; ++i) r3[i] -= Hp3[i];
      apply_prec(r3, z3);
      part = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        p3[i] = z3[i];
        part += r3[i] * z3[i];
      }
      rz = block_sum1<NT>(part, sh, phase);
      warm = false;
      continue;
    }
    const double pHp = block_sum1<NT>(part, sh, phase);
    FEM_TICK(1);
    if (!(pHp > 0.0)) {  // negative curvature (block-uniform)
      if (!psd_safe) {  // PSD-safe Hessian for this iteration, which starts over (same warm start)
        psd_safe = true;
        flags |= kFemFlagPsdSafe;
        pcg_total += (double)it;  // (the work was done)
        __syncthreads();
        goto restart_iteration;
      }
      if (it == 0 && frac_prev > 0.0) {  // a warm start alone is no descent direction: once more from a zero start
        frac_prev = 0.0;
        __syncthreads();
        goto restart_iteration;
      }
      // keep d (first iteration from a zero start: preconditioned steepest descent)
      if (it == 0) { d3[0] = z3[0]; d3[1] = z3[1]; d3[2] = z3[2]; }
      neg_curv = true;
      break;
    }
    const double al = rz / pHp;
    part = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      d3[i] += al * p3[i];
      r3[i] -= al * Hp3[i];
    }
    apply_prec(r3, z3);
#pragma unroll
    for (int i = 0; i < 3; ++i) part += r3[i] * z3[i];
    const double rz_new = block_sum1<NT>(part, sh, phase);
    const double beta = rz_new / rz;
#pragma unroll
    for (int i = 0; i < 3; ++i) p3[i] = z3[i] + beta * p3[i];
    rz = rz_new;
    ++it;
  }
  if (use_coarse && !neg_curv) {  // (block-uniform)
    const double rr = block_sum1<NT>(r3[0] * r3[0] + r3[1] * r3[1] + r3[2] * r3[2], sh, phase);
    if (rr > kCoarseTrust * kCoarseTrust * bb) {
      use_coarse = false;
      flags |= kFemFlagCoarseOff;
      pcg_total += (double)it;  // (the work was done)
      __syncthreads();
      goto restart_iteration;
    }
  }
  FEM_PHASE(2);
  // ---- backtracking line search on the incremental potential (accept the first E(x + step d) <= E(x)) ----
  const double E0 = env_energy_lds<MESH, NT>(m, xs, x3, xt, own, c, aim, sh, phase, im, ind, wv, fric_phase ? fl : nullptr, xn, disp3, &e_tets);
  double step = 1.0, E1 = E0;
  if (ind) {
    // CCD step filter for analytic indenters: a signed distance field is 1-Lipschitz, so a vertex at gap d moving by
    // step |dx| keeps a positive gap while step < d / |dx|; the largest step every surface vertex allows, with slack
    double amax = 1.0;
    if (wv > 0.0 && !ce.penetrating && ce.d < 1e299) {
      const double nd = sqrt(d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2]);
      if (nd > 0.0) amax = fmin(1.0, kCcdSlack * ce.d / nd);
    }
    step = block_min1<NT>(amax, sh, phase);
  }
  // max |d| of the UNSCALED Newton direction (what the convergence test looks at)
  const double dmax = -block_min1<NT>(own ? -fmax(fabs(d3[0]), fmax(fabs(d3[1]), fabs(d3[2]))) : 0.0, sh, phase);
  // no search starts with a vertex moving further than the body is long: a steepest-descent direction kept on negative curvature has
  // no length scale (M^-1 b with a soft coarse mode: 600 m on the 26 mm axle, out of reach of the 2^-40 the backtracking can do)
  if (dmax > m.step_cap) step = fmin(step, m.step_cap / dmax);
  const double step0 = step;  // after the CCD filter
  bool accepted = false;
  double xc3[3] = {0, 0, 0};
  const int ls_cap = ls_max_iter > kLsRescue ? ls_max_iter : kLsRescue;
  for (int ls = 0; ls <= ls_cap; ++ls) {
    __syncthreads();  // every tet is done reading ps (PCG sweep or the previous candidate)
    if (own) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { xc3[i] = x3[i] + step * d3[i]; ps[tid * 3 + i] = xc3[i]; }
    }
    __syncthreads();
    const double Ec = env_energy_lds<MESH, NT>(m, ps, xc3, xt, own, c, aim, sh, phase, im, ind, wv, fric_phase ? fl : nullptr, xn, disp3);
    if (Ec <= E0) { E1 = Ec; accepted = true; break; }
    step *= 0.5;
  }
  if (accepted) {
    if (own) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { x3[i] = xc3[i]; xs[tid * 3 + i] = xc3[i]; }
    }
  } else {
    step = 0.0;
    // (no decrease to be had at a point whose Newton step is below the tolerance: converged; a direction that came from a warm start
    //  has no descent guarantee: that iteration is repeated from a zero start, see below)
    if (!(dmax <= dx_tol) && !warm_used) flags |= kFemFlagLsFailed;
  }
  // A rejected search leaves x where it was and cuts the warm start: the next iteration would be bit-identical to this one, and
  // the one after, up to max_newton - each a full assembly, a PCG solve and up to 33 energy sweeps on a CU other envs wait for.
  // The env stops here with the flag set (block-uniform: `accepted` and `dmax` are block reductions).
  const bool ls_dead = !accepted && !(dmax <= dx_tol);
  FEM_PHASE(3);
  ++n_newton;
  pcg_total += (double)it;
  dmax_last = dmax;
  frac_prev = (accepted && step < 1.0) ? 1.0 - step : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (own) dprev_g[i] = d3[i];
  if (tid == 0) {
    stats[(size_t)b * 4 + 0] = E0; stats[(size_t)b * 4 + 1] = E1; stats[(size_t)b * 4 + 2] = step; stats[(size_t)b * 4 + 3] = (double)it;
#ifdef TACEX_FEM_CLOCK
    for (int k = 0; k < 4; ++k) stats[(size_t)b * 4 + k] = (TACEX_FEM_CLOCK) == 3 ? fnw[k] : fclk[4 * ((TACEX_FEM_CLOCK) % 3) + k];
#endif
  }
  // IPC's test (Li et al. 2020, Algorithm 1: the infinity norm of the SEARCH DIRECTION over dt against the velocity tolerance): the
  // unscaled Newton direction, whatever the CCD bound and the line search then made of the step - a shortened UPDATE says nothing
  // about convergence, a short DIRECTION does.  (Rounds 2-3 also demanded a full-length accepted step: at the edge of
  // the barrier zone that never happens and every retreat step ran to the iteration cap with directions 5x below the tolerance.)
  if (ls_dead) {
    if (warm_used) continue;  // (frac_prev is 0 now: the next iteration solves the same system from a zero start)
    break;
  }
  const bool converged = dmax <= dx_tol;
  if (converged) {  // wave-uniform: every quantity above is a block reduction
    if (fric && !fric_phase && !lag_at_start) {
      // (two-phase mode) normal contact is balanced: freeze the friction lag (normal force, normal) at this state and go on, unless
      // no vertex of the env is in contact
      fric_phase = true;
      bool touching = false;
      if (own) {
        const ContactEval cf = contact_eval<MESH>(m, im, ind, wv, x3);
        touching = cf.active;
        fl[tid * 4] = 0.0; fl[tid * 4 + 1] = 0.0; fl[tid * 4 + 2] = 0.0; fl[tid * 4 + 3] = 0.0;
      }
      // the lag itself needs the contact-free gradient at this state: the next iteration computes it first (lag_pending)
      if (__syncthreads_or(touching)) { frac_prev = 0.0; lag_pending = true; continue; }
    }
    done = true;
    break;
  }
  }  // Newton loop
  if (own) {
#pragma unroll
    for (int i = 0; i < 3; ++i) x[tid * 3 + i] = x3[i];
  }
  // what the next launch (tacex_fem_newton_step called in a loop) reads to skip this env: the direction's max |d| once the env
  // has converged (<= dx_tol), a value above the tolerance while it has not (a shortened update must not count as convergence)
  if (dxg && tid == 0) dxg[b] = dmax_last;
  if (step_info) {
    // (__syncthreads_or returns a truth value, not the OR of the bits: one reduction per flag)
    const int any = (__syncthreads_or(flags & kFemFlagPenetration) ? kFemFlagPenetration : 0) |
                    (__syncthreads_or(flags & kFemFlagLsFailed) ? kFemFlagLsFailed : 0) |
                    (flags & (kFemFlagCoarseOff | kFemFlagPsdSafe)) | (mesh_bad ? kFemFlagBadMesh : 0) |
                    (mat_bad ? kFemFlagBadMaterial : 0);  // (these are block-uniform)
    if (tid == 0) {
      step_info[(size_t)b * 4 + 0] = (double)n_newton; step_info[(size_t)b * 4 + 1] = dmax_last;
      step_info[(size_t)b * 4 + 2] = (double)any; step_info[(size_t)b * 4 + 3] = pcg_total;
    }
  }
}

}  // namespace tacex
