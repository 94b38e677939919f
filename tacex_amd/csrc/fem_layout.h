// Where everything sits in the caller's FEM workspaces: the per-env block sizes the kernels index with, and the regions behind the B env
// blocks that only the host hands out.  Plain C++17 with no HIP include (tests/fem_layout_check.cpp builds it with a host compiler);
// every offset and total is computed HERE and nowhere else, so a region cannot be added to a size and forgotten in an address.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define TACEX_LAYOUT_HD __host__ __device__
#else
#define TACEX_LAYOUT_HD
#endif

namespace tacex {

constexpr int kBallMaxPairs = 4096;   // listed candidate pairs per env and Newton iteration
constexpr int kBallMaxActive = 1024;  // pairs inside d_hat at the iteration's state
constexpr int kBallRec = 14;          // doubles per active record
constexpr int kBallMaxFric = 1024;    // lagged friction contacts per env and time step (pairs + ground)

// workspace per env of the pad kernels (doubles): ge 12T | tet cache 12T (F 9, a, b, c) | hv 12T | g,r,z,p,d,Hp,xc 7*3V | Dinv 9V | contact 5V |
// friction lag 4V | friction blocks 6V
TACEX_LAYOUT_HD inline size_t newton_ws_doubles(int V, int T) { return (size_t)36 * T + (size_t)45 * V; }  // (+ 10 V: friction lag | Hessian blocks)

// workspace of one env of the ball scene (doubles): ground curvature V | xb 3nv | xbc 3nv | dxb 3nv | ball triangle spheres 4nt | pair list (ints)
//   kBallMaxPairs / 2 | active records | friction records + their Hessians.  (Everything per-vertex lives in LDS.)
TACEX_LAYOUT_HD inline size_t ball_ws_doubles(int V, int T, int nv, int nt) {
  (void)T;
  return (size_t)V + (size_t)9 * nv + (size_t)4 * nt + kBallMaxPairs / 2 + (size_t)kBallMaxActive * kBallRec +
         (size_t)kBallMaxFric * (kBallRec + 6);  // lagged friction records + their Hessians at the iteration's state
}

// tacex_fem_step's workspace, offsets in doubles from its base:
// env blocks | x_prev (B,V,3) | max |d| (B) | indenter displacement (B,3) | previous indenter position (B,3) | 1 | env launch order (B int32)
struct StepLayout {
  size_t x_prev, dx, disp, ind_prev, env_order, total;
  StepLayout(int V, int T, int B) {
    const size_t b = (size_t)B;
    x_prev = b * newton_ws_doubles(V, T);
    dx = x_prev + b * 3 * V;
    disp = dx + b;
    ind_prev = disp + 3 * b;
    env_order = ind_prev + 3 * b + 1;
    total = env_order + (b + 1) / 2 + 7;  // (the int32 order rounded up to doubles, and slack)
  }
};

// tacex_fem_ball_step's workspace, offsets in doubles from its base:
// env blocks | x_prev (B,V,3) | q_prev (B,12) | x~ (B,V,3) | q~ (B,12) | q at the end of the previous step (B,12) | 1 | env launch order (B int32)
// | 1 | elastic preconditioner blocks (B,V,16)
struct BallLayout {
  size_t x_prev, q_prev, xt, qt, q_last, env_order, blk, total;
  BallLayout(int V, int T, int nv, int nt, int B) {
    const size_t b = (size_t)B;
    x_prev = b * ball_ws_doubles(V, T, nv, nt);
    q_prev = x_prev + b * 3 * V;
    xt = q_prev + 12 * b;
    qt = xt + b * 3 * V;
    q_last = qt + 12 * b;
    env_order = q_last + 12 * b + 1;
    blk = env_order + (b + 1) / 2 + 1;
    total = blk + b * 16 * V + 8;
  }
};

}  // namespace tacex
