// FEM device layer: geometry and contact rules of the ball scene (gelpad + one affine body + ground), ONE copy of each rule for the two
// kernels that stand on them - fem_ball_newton_kernel (fem_ball.h: the step) and fem_ball_contact_forces_kernel
// (fem_ball_contact_forces.h: the force report).  Here: the scene's tables (BallDev), closest points, mollifier, barrier and additive
// CCD; the pair code of the lists; one pair evaluated at a state (ball_pair_eval) and its cheap rejection (ball_pair_far); the candidate
// cull (ball_cull); the 14-double contact record; the smoothed Coulomb law; a contact's normal force.
#pragma once
#include "fem_device.h"

namespace tacex {

struct BallDev {
  int nv = 0, nt = 0, npt = 0, nsv = 0;
  const double* Y = nullptr;      // (nv,4) [1, X]
  const int* tri = nullptr;       // (nt,3)
  const double* area = nullptr;   // (nv) vertex areas
  const int* ptri = nullptr;      // (npt,3) pad surface triangles
  const int* psv = nullptr;       // (nsv) pad surface vertices
  const double* parea = nullptr;  // (V) pad vertex areas (0: interior)
  double S[16] = {};              // 4 x 4 moment matrix
  double kv = 0.0, gh = 0.0, dhat = 0.0, kappa = 0.0;
  // edge-edge pairs: pad surface edges x ball edges (unique edges of the two triangle lists), the area each edge stands for (a third of its
  // triangles' rest areas) and its squared rest length (the mollifier's threshold); ee = 0 switches the pair kind off
  int npe = 0, nbe = 0, ee = 0;
  const int* pedge = nullptr;      // (npe,2)
  const double* pearea = nullptr;  // (npe)
  const double* pelen2 = nullptr;  // (npe)
  const int* bedge = nullptr;      // (nbe,2)
  const double* bearea = nullptr;  // (nbe)
  const double* belen2 = nullptr;  // (nbe)
  int ground = 0;
  int kinematic = 0;  // AffineBodyConstitutionCfg.kinematic (uipc_object.py:70-73, 463-466: `is_fixed`): the body's rows are not unknowns - the
                      // caller moves q between steps, the pad sees it through the pairs (both ways) and their friction
};

constexpr int kBallMaxCand = 512;     // candidate pad vertices / pad triangles / ball vertices per env
constexpr double kBallReach = 2.0;    // additive CCD on pairs closer than kBallReach * d_hat
constexpr double kBallKeep = 0.1;     // ... which may keep this fraction of their gap
constexpr int kBallFlagOverflow = 16; // step_info flag: a candidate / pair list overflowed (the scene is outside what this slice handles)

// (kBallMaxPairs, kBallMaxActive, kBallRec, kBallMaxFric and the env's workspace block, ball_ws_doubles: fem_layout.h)

// closest point of triangle (a, b, c) to p: barycentric coordinates, distance, unit vector from the closest point to p
// (Ericson 5.1.5, regions in the book's order - oracle/abd_oracle.py point_triangle)
__device__ __forceinline__ void pt_closest(const double p[3], const double a[3], const double b[3], const double c[3], double beta[3], double& d,
                                           double n[3]) {
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const double d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2], d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
  const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const double d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2], d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
  const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const double d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2], d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  double s, u;
  if (d1 <= 0.0 && d2 <= 0.0) { s = 0.0; u = 0.0; }
  else if (d3 >= 0.0 && d4 <= d3) { s = 1.0; u = 0.0; }
  else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { s = d1 / (d1 - d3); u = 0.0; }
  else if (d6 >= 0.0 && d5 <= d6) { s = 0.0; u = 1.0; }
  else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { s = 0.0; u = d2 / (d2 - d6); }
  else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) { u = (d4 - d3) / ((d4 - d3) + (d5 - d6)); s = 1.0 - u; }
  else { const double den = 1.0 / (va + vb + vc); s = vb * den; u = vc * den; }
  beta[0] = 1.0 - s - u; beta[1] = s; beta[2] = u;
  const double r0 = ap[0] - s * ab[0] - u * ac[0], r1 = ap[1] - s * ab[1] - u * ac[1], r2 = ap[2] - s * ab[2] - u * ac[2];
  d = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
  const double id = d > 0.0 ? 1.0 / d : 0.0;
  n[0] = r0 * id; n[1] = r1 * id; n[2] = r2 * id;
}

// additive CCD of one point-triangle pair (oracle/abd_oracle.py accd_point_triangle): largest t <= t_max keeping >= keep * d(0)
__device__ double accd_pt(const double p[3], const double tr[9], const double dp_in[3], const double dtr_in[9], double t_max) {
  double dp[3], dtr[9], mean[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) mean[i] = (dp_in[i] + dtr_in[i] + dtr_in[3 + i] + dtr_in[6 + i]) * 0.25;
#pragma unroll
  for (int i = 0; i < 3; ++i) { dp[i] = dp_in[i] - mean[i]; dtr[i] = dtr_in[i] - mean[i]; dtr[3 + i] = dtr_in[3 + i] - mean[i]; dtr[6 + i] = dtr_in[6 + i] - mean[i]; }
  double lt = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) lt = fmax(lt, sqrt(dtr[3 * k] * dtr[3 * k] + dtr[3 * k + 1] * dtr[3 * k + 1] + dtr[3 * k + 2] * dtr[3 * k + 2]));
  const double l = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]) + lt;
  if (!(l > 0.0)) return t_max;
  auto dist = [&](double t) {
    double q[3], a[3], b[3], c[3], be[3], d, n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { q[i] = p[i] + t * dp[i]; a[i] = tr[i] + t * dtr[i]; b[i] = tr[3 + i] + t * dtr[3 + i]; c[i] = tr[6 + i] + t * dtr[6 + i]; }
    pt_closest(q, a, b, c, be, d, n);
    return d;
  };
  const double d0 = dist(0.0), g = kBallKeep * d0;
  double t = 0.0, tl = (1.0 - kBallKeep) * d0 / l;
  for (int it = 0; it < 64; ++it) {
    const double d = dist(t + tl);
    if (t > 0.0 && d < g) break;
    t += tl;
    if (t >= t_max) return t_max;
    tl = kCcdSlack * d / l;
  }
  return t;
}

// closest points of segments a0-a1 and b0-b1 (Ericson 5.1.9 - oracle/abd_oracle.py segment_segment): parameters, distance, unit vector from
// the point on b to the point on a; the distance's gradient is (1-s) n, s n on a's end points and -(1-t) n, -t n on b's
__device__ __forceinline__ void ee_closest(const double a0[3], const double a1[3], const double b0[3], const double b1[3], double& s, double& t, double& d,
                                           double n[3]) {
  const double d1[3] = {a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]}, d2[3] = {b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]};
  const double r[3] = {a0[0] - b0[0], a0[1] - b0[1], a0[2] - b0[2]};
  const double a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
  const double f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2], c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
  const double bq = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
  const double den = a * e - bq * bq;
  s = den > 0.0 ? fmin(fmax((bq * f - c * e) / den, 0.0), 1.0) : 0.0;
  t = (bq * s + f) / e;
  if (t < 0.0) { t = 0.0; s = fmin(fmax(-c / a, 0.0), 1.0); }
  else if (t > 1.0) { t = 1.0; s = fmin(fmax((bq - c) / a, 0.0), 1.0); }
  const double w0 = r[0] + s * d1[0] - t * d2[0], w1 = r[1] + s * d1[1] - t * d2[1], w2 = r[2] + s * d1[2] - t * d2[2];
  d = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double id = d > 0.0 ? 1.0 / d : 0.0;
  n[0] = w0 * id; n[1] = w1 * id; n[2] = w2 * id;
}

// IPC's mollifier of nearly parallel edge pairs in c = |e_a x e_b|^2 (Li et al. 2020 eq. 24 - oracle edge_mollifier): m, dm/dc; u = e_a x e_b
__device__ __forceinline__ void ee_mollifier(const double a0[3], const double a1[3], const double b0[3], const double b1[3], double eps, double& mol, double& dm,
                                             double e1[3], double e2[3], double u[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { e1[i] = a1[i] - a0[i]; e2[i] = b1[i] - b0[i]; }
  u[0] = e1[1] * e2[2] - e1[2] * e2[1]; u[1] = e1[2] * e2[0] - e1[0] * e2[2]; u[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const double r = (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) / eps;
  if (r < 1.0) { mol = (2.0 - r) * r; dm = 2.0 * (1.0 - r) / eps; }
  else { mol = 1.0; dm = 0.0; }
}

// additive CCD of one edge-edge pair (oracle accd_edge_edge); ea, eb, dea, deb: the two end points of each edge, row-major (2,3)
__device__ double accd_ee(const double ea[6], const double eb[6], const double dea_in[6], const double deb_in[6], double t_max) {
  double da[6], db[6], mean[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) mean[i] = (dea_in[i] + dea_in[3 + i] + deb_in[i] + deb_in[3 + i]) * 0.25;
#pragma unroll
  for (int i = 0; i < 3; ++i) { da[i] = dea_in[i] - mean[i]; da[3 + i] = dea_in[3 + i] - mean[i]; db[i] = deb_in[i] - mean[i]; db[3 + i] = deb_in[3 + i] - mean[i]; }
  const double la = fmax(sqrt(da[0] * da[0] + da[1] * da[1] + da[2] * da[2]), sqrt(da[3] * da[3] + da[4] * da[4] + da[5] * da[5]));
  const double lb = fmax(sqrt(db[0] * db[0] + db[1] * db[1] + db[2] * db[2]), sqrt(db[3] * db[3] + db[4] * db[4] + db[5] * db[5]));
  const double l = la + lb;
  if (!(l > 0.0)) return t_max;
  auto dist = [&](double t) {
    double a0[3], a1[3], b0[3], b1[3], s, u, d, n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { a0[i] = ea[i] + t * da[i]; a1[i] = ea[3 + i] + t * da[3 + i]; b0[i] = eb[i] + t * db[i]; b1[i] = eb[3 + i] + t * db[3 + i]; }
    ee_closest(a0, a1, b0, b1, s, u, d, n);
    return d;
  };
  const double d0 = dist(0.0), g = kBallKeep * d0;
  double t = 0.0, tl = (1.0 - kBallKeep) * d0 / l;
  for (int it = 0; it < 64; ++it) {
    const double d = dist(t + tl);
    if (t > 0.0 && d < g) break;
    t += tl;
    if (t >= t_max) return t_max;
    tl = kCcdSlack * d / l;
  }
  return t;
}

__device__ __forceinline__ void barrier3(double s, double& b, double& b1, double& b2) {  // b(s), b'(s), b''(s) of the dimensionless barrier
  if (!(s > 0.0)) { b = INFINITY; b1 = 0.0; b2 = 0.0; return; }
  if (s >= 1.0) { b = 0.0; b1 = 0.0; b2 = 0.0; return; }
  const double ln = log(s), q = s - 1.0;
  b = -q * q * ln;
  b1 = -2.0 * q * ln - q * q / s;
  b2 = -2.0 * ln - 4.0 * q / s + q * q / (s * s);
}

// normal force of a contact of weight w (newtons, >= 0): -d/dd of kappa w b(d / d_hat), b1 = b'(d / d_hat)
__device__ __forceinline__ double ball_contact_lambda(double kappa, double w, double b1, double dhat) { return -kappa * w * b1 / dhat; }

// surface points of the body: out (nv,3) = Y qq, qq = (p, c_1, c_2, c_3)
__device__ __forceinline__ void ball_points(const BallDev& bd, const double* qq, double* out, int tid, int NT) {
  for (int k = tid; k < bd.nv; k += NT) {
    const double y0 = bd.Y[k * 4], y1 = bd.Y[k * 4 + 1], y2 = bd.Y[k * 4 + 2], y3 = bd.Y[k * 4 + 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[k * 3 + i] = y0 * qq[i] + y1 * qq[3 + i] + y2 * qq[6 + i] + y3 * qq[9 + i];
  }
}

// ---- pairs -----------------------------------------------------------------------------------------------------------
// kind 0: pad surface vertex i x ball triangle j | 1: ball vertex i x pad surface triangle j | 2: pad surface edge i x ball edge j.
// A list entry is kind << 30 | i << 15 | j (indices < 32768).
__device__ __forceinline__ int ball_pair_code(int kind, int i, int j) { return (int)(((unsigned)kind << 30) | ((unsigned)i << 15) | (unsigned)j); }
__device__ __forceinline__ void ball_pair_decode(int code, int& kind, int& i, int& j) {
  const unsigned c = (unsigned)code;
  kind = (int)(c >> 30); i = (int)((c >> 15) & 0x7fff); j = (int)(c & 0x7fff);
}

// One pair at a state (xs: the env's pad vertices, xb: the body's surface points Y q): its distance is d, the gradient of d over the state
// rows is pco[r] n on the pad rows prow[r] (-1: unused) and cq[a] n on the body's four rows.
struct BallPairEval {
  double d, w, n[3];    // distance, weight (the mollifier included), unit normal
  double cq[4], pco[3];
  int prow[3];
  double cp[3];         // the pad-side closest point
  double molg;          // w0 m'(c) of a mollified edge-edge pair (0: none); grad c = -ga / +ga on prow[0] / prow[1], yd[a] gbq on the body rows
  double ga[3], gbq[3], yd[4];
};

// Returns whether the pair is active (d < d_hat, weight > 0).  A caller reads what it needs and the rest is dropped once this is inlined:
// the energy takes d and w, the lists d alone.  LISTED: the caller walks a list that reaches well past d_hat (the step's: 2.8 d_hat, most
// of its edge pairs inactive) - an edge pair at d >= d_hat skips the mollifier and the coefficients and comes back with d, n and w = 0.
// Spelling (profiles/ball_pairs_isa.md): the skip is a block, not a return from the middle, and every field is worked out in a local
// of its own and handed over once at the end - either of the other two spellings costs the step kernel registers and scratch.
template <bool LISTED>
__device__ __forceinline__ bool ball_pair_eval(int kind, int i, int j, const double* xs, const double* xb, const BallDev& bd, BallPairEval& e) {
  double d, w, n[3], cq[4] = {0.0, 0.0, 0.0, 0.0}, pco[3] = {0.0, 0.0, 0.0}, cp[3] = {0.0, 0.0, 0.0};
  double molg = 0.0, ga[3] = {0.0, 0.0, 0.0}, gbq[3] = {0.0, 0.0, 0.0}, yd[4] = {0.0, 0.0, 0.0, 0.0};
  int prow[3] = {-1, -1, -1};
  if (kind == 2) {
    const int* ea = bd.pedge + i * 2;
    const int* eb = bd.bedge + j * 2;
    double a0[3], a1[3], b0[3], b1[3], sa, tb, mol, dm, e1[3], e2[3], u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a0[k] = xs[ea[0] * 3 + k]; a1[k] = xs[ea[1] * 3 + k]; b0[k] = xb[eb[0] * 3 + k]; b1[k] = xb[eb[1] * 3 + k]; }
    ee_closest(a0, a1, b0, b1, sa, tb, d, n);
    w = 0.0;
    if (!LISTED || d < bd.dhat) {
      ee_mollifier(a0, a1, b0, b1, 1e-3 * bd.pelen2[i] * bd.belen2[j], mol, dm, e1, e2, u);
      const double w0 = 0.5 * (bd.pearea[i] + bd.bearea[j]);
      w = w0 * mol;
#pragma unroll
      for (int a4 = 0; a4 < 4; ++a4) {
        cq[a4] = -((1.0 - tb) * bd.Y[eb[0] * 4 + a4] + tb * bd.Y[eb[1] * 4 + a4]);
        yd[a4] = bd.Y[eb[1] * 4 + a4] - bd.Y[eb[0] * 4 + a4];
      }
      prow[0] = ea[0]; prow[1] = ea[1]; prow[2] = -1;
      pco[0] = 1.0 - sa; pco[1] = sa; pco[2] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) cp[k] = (1.0 - sa) * a0[k] + sa * a1[k];
      if (dm > 0.0) {  // grad c = 2 (e2 x u) on a1 (minus on a0), 2 (u x e1) on b1 (minus on b0)
        molg = w0 * dm;
        ga[0] = 2.0 * (e2[1] * u[2] - e2[2] * u[1]); ga[1] = 2.0 * (e2[2] * u[0] - e2[0] * u[2]); ga[2] = 2.0 * (e2[0] * u[1] - e2[1] * u[0]);
        gbq[0] = 2.0 * (u[1] * e1[2] - u[2] * e1[1]); gbq[1] = 2.0 * (u[2] * e1[0] - u[0] * e1[2]); gbq[2] = 2.0 * (u[0] * e1[1] - u[1] * e1[0]);
      }
    }
  } else {
    const int* tr = (kind == 0 ? bd.tri : bd.ptri) + j * 3;
    const int t0 = tr[0], t1 = tr[1], t2 = tr[2];
    double p3[3], a[3], bq[3], c[3], be[3];
    if (kind == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { p3[k] = xs[i * 3 + k]; a[k] = xb[t0 * 3 + k]; bq[k] = xb[t1 * 3 + k]; c[k] = xb[t2 * 3 + k]; }
      w = bd.parea[i];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { p3[k] = xb[i * 3 + k]; a[k] = xs[t0 * 3 + k]; bq[k] = xs[t1 * 3 + k]; c[k] = xs[t2 * 3 + k]; }
      w = bd.area[i];
    }
    pt_closest(p3, a, bq, c, be, d, n);
    if (kind == 0) {
#pragma unroll
      for (int a4 = 0; a4 < 4; ++a4) cq[a4] = -(be[0] * bd.Y[t0 * 4 + a4] + be[1] * bd.Y[t1 * 4 + a4] + be[2] * bd.Y[t2 * 4 + a4]);
      prow[0] = i; prow[1] = -1; prow[2] = -1;
      pco[0] = 1.0; pco[1] = 0.0; pco[2] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) cp[k] = p3[k];
    } else {
#pragma unroll
      for (int a4 = 0; a4 < 4; ++a4) cq[a4] = bd.Y[i * 4 + a4];
      prow[0] = t0; prow[1] = t1; prow[2] = t2;
      pco[0] = -be[0]; pco[1] = -be[1]; pco[2] = -be[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) cp[k] = be[0] * a[k] + be[1] * bq[k] + be[2] * c[k];
    }
  }
  e.d = d; e.w = w; e.molg = molg;
#pragma unroll
  for (int k = 0; k < 3; ++k) { e.n[k] = n[k]; e.pco[k] = pco[k]; e.prow[k] = prow[k]; e.cp[k] = cp[k]; e.ga[k] = ga[k]; e.gbq[k] = gbq[k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) { e.cq[k] = cq[k]; e.yd[k] = yd[k]; }
  return d < bd.dhat && w > 0.0;
}

// cheap rejection ahead of ball_pair_eval: true when the pair cannot be closer than L (spheres about a triangle's first corner / the edges' mid points)
__device__ __forceinline__ bool ball_pair_far(int kind, int i, int j, const double* xs, const double* xb, const BallDev& bd, double L) {
  if (kind == 2) {
    const int* ea = bd.pedge + i * 2;
    const int* eb = bd.bedge + j * 2;
    double r2 = 0.0, ha = 0.0, hb = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a0 = xs[ea[0] * 3 + k], a1 = xs[ea[1] * 3 + k], b0 = xb[eb[0] * 3 + k], b1 = xb[eb[1] * 3 + k];
      const double mi = 0.5 * ((a0 + a1) - (b0 + b1)), hai = 0.5 * (a1 - a0), hbi = 0.5 * (b1 - b0);
      r2 += mi * mi; ha += hai * hai; hb += hbi * hbi;
    }
    const double lim = L + sqrt(ha) + sqrt(hb);
    return r2 >= lim * lim;
  }
  const double* P = kind == 0 ? xs : xb;  // the point's array; the triangle lives in the other
  const double* Q = kind == 0 ? xb : xs;
  const int* tr = (kind == 0 ? bd.tri : bd.ptri) + j * 3;
  double r2 = 0.0, e2 = 0.0, f2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = Q[tr[0] * 3 + k], r = P[i * 3 + k] - a, e = Q[tr[1] * 3 + k] - a, f = Q[tr[2] * 3 + k] - a;
    r2 += r * r; e2 += e * e; f2 += f * f;
  }
  const double lim = L + sqrt(fmax(e2, f2));
  return r2 >= lim * lim;
}

// ---- candidate cull --------------------------------------------------------------------------------------------------
// The six candidate lists of an env and their counters.  Each kernel declares them as its own __shared__ arrays (capacity kBallMaxCand,
// indices < 32768) and names them here; n: the lists' lengths after ball_cull, clamped to the capacity.
struct BallCull {
  unsigned short *cpv, *cpt, *cpe;  // candidate pad vertices / triangles / edges
  unsigned short *cbv, *cbt, *cbe;  // candidate ball vertices / triangles / edges
  int *n_cpv, *n_cpt, *n_cpe, *n_cbv, *n_cbt, *n_cbe;
  int *flags;                       // |= kBallFlagOverflow when a list overflowed
  int npv, npt, npe, nbv, nbt, nbe;
};

__device__ __forceinline__ void ball_cull_push(int* n, unsigned short* list, int item) {
  const int s = atomicAdd(n, 1);
  if (s < kBallMaxCand) list[s] = (unsigned short)item;
}

// Candidates at the state (xs pad vertices, p the body's translation row, xb its surface points) and reach L: the pad's surface vertices /
// triangles / edges within L of the ball's bounding sphere about p, then the ball's side - what lies within L of the bounding box of the
// pad's candidates (a ball of 320 triangles / 480 edges / 162 vertices touches the pad with a few dozen of each: the pair tests shrink
// accordingly).  tri_in(t, lo, hi): whether ball triangle t reaches into the box - the caller's own test.  Slots are handed out with LDS
// atomics: the order of a list varies between runs.  Block-wide (barriers inside); sh: >= 17 doubles.
template <int NT, typename TriIn>
__device__ __forceinline__ void ball_cull(const BallDev& bd, BallCull& c, const double* xs, const double* p, const double* xb, double L, double* sh, int tid,
                                          TriIn&& tri_in) {
  if (tid == 0) { *c.n_cpv = 0; *c.n_cpt = 0; *c.n_cpe = 0; *c.n_cbv = 0; *c.n_cbt = 0; *c.n_cbe = 0; }
  double rb = 0.0;  // bounding radius of the ball about p
  for (int k = tid; k < bd.nv; k += NT) {
    const double r0 = xb[k * 3] - p[0], r1 = xb[k * 3 + 1] - p[1], r2 = xb[k * 3 + 2] - p[2];
    rb = fmax(rb, sqrt(r0 * r0 + r1 * r1 + r2 * r2));
  }
  rb = block_sum_max(rb, sh);
  for (int k = tid; k < bd.nsv; k += NT) {
    const int v = bd.psv[k];
    const double r0 = xs[v * 3] - p[0], r1 = xs[v * 3 + 1] - p[1], r2 = xs[v * 3 + 2] - p[2];
    const double lim = rb + L;
    if (r0 * r0 + r1 * r1 + r2 * r2 < lim * lim) ball_cull_push(c.n_cpv, c.cpv, v);
  }
  for (int k = tid; k < bd.npt; k += NT) {
    const int* tr = bd.ptri + k * 3;
    double c3[3], rt = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) c3[i] = (xs[tr[0] * 3 + i] + xs[tr[1] * 3 + i] + xs[tr[2] * 3 + i]) * (1.0 / 3.0);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double r0 = xs[tr[j] * 3] - c3[0], r1 = xs[tr[j] * 3 + 1] - c3[1], r2 = xs[tr[j] * 3 + 2] - c3[2];
      rt = fmax(rt, sqrt(r0 * r0 + r1 * r1 + r2 * r2));
    }
    const double r0 = c3[0] - p[0], r1 = c3[1] - p[1], r2 = c3[2] - p[2];
    const double lim = rb + L + rt;
    if (r0 * r0 + r1 * r1 + r2 * r2 < lim * lim) ball_cull_push(c.n_cpt, c.cpt, k);
  }
  if (bd.ee)
    for (int k = tid; k < bd.npe; k += NT) {
      const int* ed = bd.pedge + k * 2;
      double r2 = 0.0, h2 = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double mi = 0.5 * (xs[ed[0] * 3 + i] + xs[ed[1] * 3 + i]) - p[i], hi = 0.5 * (xs[ed[1] * 3 + i] - xs[ed[0] * 3 + i]);
        r2 += mi * mi; h2 += hi * hi;
      }
      const double lim = rb + L + sqrt(h2);
      if (r2 < lim * lim) ball_cull_push(c.n_cpe, c.cpe, k);
    }
  __syncthreads();
  if (*c.n_cpv > kBallMaxCand || *c.n_cpt > kBallMaxCand || *c.n_cpe > kBallMaxCand) { if (tid == 0) *c.flags |= kBallFlagOverflow; }
  c.npv = min(*c.n_cpv, kBallMaxCand); c.npt = min(*c.n_cpt, kBallMaxCand); c.npe = min(*c.n_cpe, kBallMaxCand);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  auto grow = [&](int v) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { lo[i] = fmin(lo[i], xs[v * 3 + i]); hi[i] = fmax(hi[i], xs[v * 3 + i]); }
  };
  for (int k = tid; k < c.npv; k += NT) grow(c.cpv[k]);
  for (int k = tid; k < c.npt; k += NT) { const int* tr = bd.ptri + c.cpt[k] * 3; grow(tr[0]); grow(tr[1]); grow(tr[2]); }
  for (int k = tid; k < c.npe; k += NT) { const int* ed = bd.pedge + c.cpe[k] * 2; grow(ed[0]); grow(ed[1]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { lo[i] = -block_sum_max(-lo[i], sh) - L; hi[i] = block_sum_max(hi[i], sh) + L; }
  for (int k = tid; k < bd.nv; k += NT) {
    const double p0 = xb[k * 3], p1 = xb[k * 3 + 1], p2 = xb[k * 3 + 2];
    if (p0 >= lo[0] && p0 <= hi[0] && p1 >= lo[1] && p1 <= hi[1] && p2 >= lo[2] && p2 <= hi[2]) ball_cull_push(c.n_cbv, c.cbv, k);
  }
  for (int t = tid; t < bd.nt; t += NT)
    if (tri_in(t, lo, hi)) ball_cull_push(c.n_cbt, c.cbt, t);
  if (bd.ee)
    for (int k = tid; k < bd.nbe; k += NT) {
      const int* eb = bd.bedge + k * 2;
      bool in = true;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double a = xb[eb[0] * 3 + i], b2 = xb[eb[1] * 3 + i];
        in = in && fmax(a, b2) >= lo[i] && fmin(a, b2) <= hi[i];
      }
      if (in) ball_cull_push(c.n_cbe, c.cbe, k);
    }
  __syncthreads();
  if (*c.n_cbv > kBallMaxCand || *c.n_cbt > kBallMaxCand || *c.n_cbe > kBallMaxCand) { if (tid == 0) *c.flags |= kBallFlagOverflow; }
  c.nbv = min(*c.n_cbv, kBallMaxCand); c.nbt = min(*c.n_cbt, kBallMaxCand); c.nbe = min(*c.n_cbe, kBallMaxCand);
}

// ---- the contact record (kBallRec = 14 doubles: active pairs of an iteration, lagged friction contacts of a step) ------------------
// head (the pair's curvature / the contact's normal force) | n (3) | body coefficients cq (4) | pad coefficients pco (3) | pad rows (3
// ints in the last three doubles' first 12 bytes; -1: unused)
__device__ __forceinline__ void ball_rec_store(double* rc, double head, const double n[3], const double cq[4], const double pco[3], const int prow[3]) {
  rc[0] = head; rc[1] = n[0]; rc[2] = n[1]; rc[3] = n[2];
  rc[4] = cq[0]; rc[5] = cq[1]; rc[6] = cq[2]; rc[7] = cq[3];
  rc[8] = pco[0]; rc[9] = pco[1]; rc[10] = pco[2];
  int* ri = reinterpret_cast<int*>(rc + 11);
  ri[0] = prow[0]; ri[1] = prow[1]; ri[2] = prow[2];
}
__device__ __forceinline__ const int* ball_rec_rows(const double* rc) { return reinterpret_cast<const int*>(rc + 11); }

// ---- smoothed Coulomb law of a lagged contact (IPC, Li et al. 2020 eq. 18-20; fem_device.h, friction_eval, has the prose) -----------
// tangential part of a relative displacement against the contact's normal
__device__ __forceinline__ void ball_tangential(const double rel[3], const double n[3], double u[3]) {
  const double rn = rel[0] * n[0] + rel[1] * n[1] + rel[2] * n[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = rel[i] - rn * n[i];
}
// at sliding y, stick tolerance eps: f0(y) (potential per mu lam), fa = f1(y) / y (gradient: fa u), fb = f1'(y) (Hessian: fa T + (fb - fa) t t^T)
__device__ __forceinline__ void ball_fric_law(double y, double eps, double& f0, double& fa, double& fb) {
  const bool stick = y < eps;
  f0 = stick ? -y * y * y / (3.0 * eps * eps) + y * y / eps + eps / 3.0 : y;
  fa = stick ? 2.0 / eps - y / (eps * eps) : 1.0 / y;
  fb = stick ? 2.0 / eps - 2.0 * y / (eps * eps) : 0.0;
}

}  // namespace tacex
