// Height-map SOURCE for arbitrary rigid indenters (second slice): pinhole depth image of a triangle mesh per
// env - what the IsaacLab TiledCamera hands GelSightSensor._get_height_map (GS:229-263, 581-593: "distance_to_image_plane"
// depth in metres, inf where the camera sees nothing inside its clipping range).  One shared mesh (object frame), one rigid pose
// per env (unit quaternion wxyz + translation into the camera frame: x right, y down, z along the optical axis).
//
// Workgroup = (env, 64 x 32 pixel tile) with the tile's z-buffer in LDS; every thread walks the triangles t = tid, tid + 256, ...:
// transform, project, clip the bounding box to the tile, and for the covered pixel centres (j + 0.5, i + 0.5) interpolate 1/z
// (affine in screen space for a pinhole) and atomicMin the depth (positive floats order like their bit patterns).  No back-face
// culling (the nearest surface wins whatever its orientation), fragments outside [near, far] are dropped per pixel (clipping),
// triangles with a vertex at or behind the camera plane are dropped whole.  Arithmetic is plain float32 with FMA contraction
// off (this file is compiled with -ffp-contract=off, tacex_amd/_build.py) and IEEE division - see oracle/mesh_depth_oracle.py, which repeats them in the same order: the two agree bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "tacex_hip.h"
#include "tacex_internal.h"
#include "wave_ops.h"

namespace tacex {

constexpr int kRasterTileW = 64, kRasterTileH = 32;

struct RasterArgs {
  const float* verts;   // (V,3)
  const int* tris;      // (T,3)
  const float* pos;     // (B,3) translation into the camera frame
  const float* quat;    // (B,4) wxyz rotation into the camera frame (normalised here, in double)
  float* depth;         // (B,H,W)
  int V, T, B, H, W;
  float fx, fy, cx, cy, near_m, far_m;
  int tiles_x, tiles_y;
  float bs[4];          // bounding sphere of the mesh in the object frame (centre, radius); radius < 0: unknown
};

// rotation and translation of env `env` into the camera frame: the quaternion normalised in double, the matrix rounded once to float32
// (what the NumPy restatement does)
struct RasterPose {
  float r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2;
};
__device__ __forceinline__ RasterPose raster_pose(const RasterArgs& a, int env) {
  double qw = a.quat[4 * env], qx = a.quat[4 * env + 1], qy = a.quat[4 * env + 2], qz = a.quat[4 * env + 3];
  const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  RasterPose P;
  P.r00 = (float)(1.0 - 2.0 * (qy * qy + qz * qz)); P.r01 = (float)(2.0 * (qx * qy - qz * qw)); P.r02 = (float)(2.0 * (qx * qz + qy * qw));
  P.r10 = (float)(2.0 * (qx * qy + qz * qw)); P.r11 = (float)(1.0 - 2.0 * (qx * qx + qz * qz)); P.r12 = (float)(2.0 * (qy * qz - qx * qw));
  P.r20 = (float)(2.0 * (qx * qz - qy * qw)); P.r21 = (float)(2.0 * (qy * qz + qx * qw)); P.r22 = (float)(1.0 - 2.0 * (qx * qx + qy * qy));
  P.t0 = a.pos[3 * env]; P.t1 = a.pos[3 * env + 1]; P.t2 = a.pos[3 * env + 2];
  return P;
}

// Tiles the mesh cannot touch skip the triangle loop (a contact covers a few percent of the image): conservative screen
// bounds of the mesh's bounding sphere bs (centre, radius; radius < 0: unknown) - x, y in [c -+ r] over z in [c.z - r, c.z + r] -
// against the tile [x0, x1) x [y0, y1).  Exactness is not at stake: a skipped tile holds no fragment.
__device__ __forceinline__ bool raster_tile_empty(const RasterArgs& a, const RasterPose& P, const float bs[4], int x0, int x1, int y0, int y1) {
  bool tile_empty = false;
  if (bs[3] >= 0.0f) {
    const float r = bs[3];
    const float bx = ((P.r00 * bs[0] + P.r01 * bs[1]) + P.r02 * bs[2]) + P.t0;
    const float by = ((P.r10 * bs[0] + P.r11 * bs[1]) + P.r12 * bs[2]) + P.t1;
    const float bz = ((P.r20 * bs[0] + P.r21 * bs[1]) + P.r22 * bs[2]) + P.t2;
    const float zn = bz - r, zf = bz + r;
    if (zf < a.near_m || zn > a.far_m) {
      tile_empty = true;
    } else if (zn > 1e-4f) {
      const float m = 1.001f;  // slack for the rounding of the bounds themselves
      const float ulo = fminf(a.fx * (bx - r * m) / zn, a.fx * (bx - r * m) / zf) + a.cx - 1.0f;
      const float uhi = fmaxf(a.fx * (bx + r * m) / zn, a.fx * (bx + r * m) / zf) + a.cx + 1.0f;
      const float vlo = fminf(a.fy * (by - r * m) / zn, a.fy * (by - r * m) / zf) + a.cy - 1.0f;
      const float vhi = fmaxf(a.fy * (by + r * m) / zn, a.fy * (by + r * m) / zf) + a.cy + 1.0f;
      tile_empty = uhi < (float)x0 || ulo > (float)x1 || vhi < (float)y0 || vlo > (float)y1;
    }
  }
  return tile_empty;
}

// triangle t of a.tris (indices into a.verts) into the tile's z-buffer (LDS, atomicMin of the depth's bit pattern)
__device__ __forceinline__ void raster_triangle(const RasterArgs& a, const RasterPose& P, int t, int x0, int x1, int y0, int y1, unsigned* zbuf) {
  float sx[3], sy[3], iz[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int vi = a.tris[3 * t + k];
    const float vx = a.verts[3 * vi], vy = a.verts[3 * vi + 1], vz = a.verts[3 * vi + 2];
    const float px = ((P.r00 * vx + P.r01 * vy) + P.r02 * vz) + P.t0;
    const float py = ((P.r10 * vx + P.r11 * vy) + P.r12 * vz) + P.t1;
    const float pz = ((P.r20 * vx + P.r21 * vy) + P.r22 * vz) + P.t2;
    ok = ok && pz > 1e-6f;
    iz[k] = 1.0f / pz;
    sx[k] = (a.fx * px) * iz[k] + a.cx;
    sy[k] = (a.fy * py) * iz[k] + a.cy;
  }
  if (!ok) return;
  const float minx = fminf(fminf(sx[0], sx[1]), sx[2]), maxx = fmaxf(fmaxf(sx[0], sx[1]), sx[2]);
  const float miny = fminf(fminf(sy[0], sy[1]), sy[2]), maxy = fmaxf(fmaxf(sy[0], sy[1]), sy[2]);
  // pixel centres j + 0.5 inside [minx, maxx]: j from ceil(minx - 0.5) to floor(maxx - 0.5)
  const int jx0 = max(x0, (int)ceilf(minx - 0.5f)), jx1 = min(x1 - 1, (int)floorf(maxx - 0.5f));
  const int iy0 = max(y0, (int)ceilf(miny - 0.5f)), iy1 = min(y1 - 1, (int)floorf(maxy - 0.5f));
  if (jx0 > jx1 || iy0 > iy1) return;
  const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
  if (area == 0.0f) return;
  const float inv_area = 1.0f / area;
  for (int i = iy0; i <= iy1; ++i) {
    const float py = (float)i + 0.5f;
    for (int j = jx0; j <= jx1; ++j) {
      const float px = (float)j + 0.5f;
      // edge functions (twice the signed sub-triangle areas); inside when all share the sign of `area` (zero counts as inside)
      const float e0 = (sx[2] - sx[1]) * (py - sy[1]) - (sy[2] - sy[1]) * (px - sx[1]);
      const float e1 = (sx[0] - sx[2]) * (py - sy[2]) - (sy[0] - sy[2]) * (px - sx[2]);
      const float e2 = (sx[1] - sx[0]) * (py - sy[0]) - (sy[1] - sy[0]) * (px - sx[0]);
      const bool in = area > 0.0f ? (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) : (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
      if (!in) continue;
      const float l0 = e0 * inv_area, l1 = e1 * inv_area, l2 = e2 * inv_area;
      const float invz = (l0 * iz[0] + l1 * iz[1]) + l2 * iz[2];
      const float z = 1.0f / invz;
      if (!(z >= a.near_m && z <= a.far_m)) continue;  // clipping range of the camera (also drops NaN)
      atomicMin(&zbuf[(i - y0) * kRasterTileW + (j - x0)], __float_as_uint(z));
    }
  }
}

__global__ __launch_bounds__(256) void mesh_depth_kernel(RasterArgs a) {
  __shared__ unsigned zbuf[kRasterTileW * kRasterTileH];
  const int per_env = a.tiles_x * a.tiles_y;
  const int env = blockIdx.x / per_env, tile = blockIdx.x - env * per_env;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * kRasterTileW, y0 = ty * kRasterTileH;
  const int x1 = min(x0 + kRasterTileW, a.W), y1 = min(y0 + kRasterTileH, a.H);  // exclusive
  for (int i = threadIdx.x; i < kRasterTileW * kRasterTileH; i += blockDim.x) zbuf[i] = 0x7f800000u;  // +inf
  __syncthreads();
  const RasterPose P = raster_pose(a, env);
  const bool tile_empty = raster_tile_empty(a, P, a.bs, x0, x1, y0, y1);
  for (int t = tile_empty ? a.T : threadIdx.x; t < a.T; t += blockDim.x) raster_triangle(a, P, t, x0, x1, y0, y1, zbuf);
  __syncthreads();
  for (int i = threadIdx.x; i < kRasterTileW * kRasterTileH; i += blockDim.x) {
    const int yy = y0 + i / kRasterTileW, xx = x0 + i % kRasterTileW;
    if (yy < y1 && xx < x1) a.depth[((size_t)env * a.H + yy) * a.W + xx] = __uint_as_float(zbuf[i]);
  }
}

// ---- The same image from a mesh LIBRARY: every env renders its own mesh (tacex_depth_from_mesh_library) -------------------------------
// The library is the concatenation of the meshes' vertex and triangle tables (triangles index the concatenated vertices); env b renders
// triangles [first, first + count) of mesh ids[b] with raster_pose / raster_tile_empty / raster_triangle - mesh_depth_kernel's
// operations, so every env's image is bit-equal to tacex_depth_from_mesh on its mesh alone (the nearest fragment is a minimum: the
// order and grouping of the triangles do not matter).
// Load balance: envs differ in triangle count, and one workgroup walking a long mesh would hold its CU while short meshes' workgroups
// are long done.  So a workgroup takes at most kLibChunk triangles of its env's mesh (4 per thread): the (env, tile) pairs are split
// into chunks and a workgroup's length is bounded whatever the mix.  Chunk 0 of every (env, tile) stores the whole tile (like
// mesh_depth_kernel: +inf where nothing was drawn); a second launch, ordered behind it on the stream, runs the further chunks of the
// longer meshes and merges them with a global atomicMin on the depth bits of the pixels they drew.  A library whose meshes all fit
// one chunk takes the first launch only.
constexpr int kLibChunk = 1024;

struct RasterLibArgs {
  RasterArgs r;          // verts / tris: the library; bs unused
  const int* mesh_tris;  // (K,2) first triangle | triangles
  const float* mesh_bs;  // (K,4) bounding sphere of every mesh (object frame; radius < 0: unknown); nullable
  const int* ids;        // (B) mesh of every env; nullable: mesh 0
  int K;
  int chunk0;            // first chunk of this launch (0 or 1)
  int nchunk;            // chunks per (env, tile) in this launch
};

template <bool MERGE>
__global__ __launch_bounds__(256) void mesh_library_depth_kernel(RasterLibArgs L) {
  __shared__ unsigned zbuf[kRasterTileW * kRasterTileH];
  const RasterArgs& a = L.r;
  const int per_env = a.tiles_x * a.tiles_y;
  const int chunk = L.chunk0 + (int)(blockIdx.x % (unsigned)L.nchunk);
  const int et = (int)(blockIdx.x / (unsigned)L.nchunk);
  const int env = et / per_env, tile = et - env * per_env;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * kRasterTileW, y0 = ty * kRasterTileH;
  const int x1 = min(x0 + kRasterTileW, a.W), y1 = min(y0 + kRasterTileH, a.H);  // exclusive
  const int id = L.ids ? L.ids[env] : 0;
  const bool valid = id >= 0 && id < L.K;  // an id outside the library renders nothing (never dereferenced)
  const int first = valid ? L.mesh_tris[2 * id] : 0, count = valid ? L.mesh_tris[2 * id + 1] : 0;
  const int t0 = chunk * kLibChunk;
  if (MERGE && t0 >= count) return;  // (workgroup-uniform)
  const RasterPose P = raster_pose(a, env);
  float bs[4] = {0.0f, 0.0f, 0.0f, -1.0f};
  if (valid && L.mesh_bs) { bs[0] = L.mesh_bs[4 * id]; bs[1] = L.mesh_bs[4 * id + 1]; bs[2] = L.mesh_bs[4 * id + 2]; bs[3] = L.mesh_bs[4 * id + 3]; }
  const bool tile_empty = t0 >= count || raster_tile_empty(a, P, bs, x0, x1, y0, y1);
  if (MERGE && tile_empty) return;
  for (int i = threadIdx.x; i < kRasterTileW * kRasterTileH; i += blockDim.x) zbuf[i] = 0x7f800000u;  // +inf
  __syncthreads();
  const int t1 = min(count, t0 + kLibChunk);
  for (int t = tile_empty ? t1 : t0 + (int)threadIdx.x; t < t1; t += blockDim.x) raster_triangle(a, P, first + t, x0, x1, y0, y1, zbuf);
  __syncthreads();
  for (int i = threadIdx.x; i < kRasterTileW * kRasterTileH; i += blockDim.x) {
    const int yy = y0 + i / kRasterTileW, xx = x0 + i % kRasterTileW;
    if (yy < y1 && xx < x1) {
      float* d = a.depth + ((size_t)env * a.H + yy) * a.W + xx;
      if (!MERGE) *d = __uint_as_float(zbuf[i]);
      else if (zbuf[i] != 0x7f800000u) atomicMin(reinterpret_cast<unsigned*>(d), zbuf[i]);
    }
  }
}


// ---- Camera depth of the FEM gel pad itself: per-env DEFORMED vertices (UipcSim.x), one camera pose per env ----------------------------
// The vertices come straight out of the FEM state x (B,V,3) float64 through surf_ids, go into the camera frame in float64 exactly as
// VisionTactileSensorUIPC.transform_world_to_camera_frame does (p_c[i] = (Rinv[i][0] d0 + Rinv[i][1] d1) + Rinv[i][2] d2, d = x - cam_pos,
// no FMA in this file) and are rounded ONCE to float32.  From that float32 camera-frame point on every operation is mesh_depth_kernel's,
// in its order (projection, pixel centres, edge functions with zero inside, 1/z interpolation, IEEE division, [near, far] per fragment,
// triangles with a vertex at pz <= 1e-6 dropped whole, no culling): oracle/mesh_depth_oracle.py with an identity pose reproduces the
// image bit for bit from the camera-frame float32 vertices.
//
// Workgroup = (env, 64 x 32 tile), 256 threads.
//  1. Staging: the env's Vs vertices are projected once per workgroup into LDS as (sx, sy, 1/z, front) - up to kDeformStageMax
//     vertices (32 KB of dynamic LDS; above that nothing is staged and every triangle projects its three vertices itself with the same
//     function, so the image is the same).  The same loop reduces the screen-space box of the FRONT vertices over the workgroup: a tile
//     whose pixel centres that box does not reach holds no fragment (every rendered triangle has front vertices only and its pixels lie
//     inside its own vertex box) and skips the rest.  The contact face covers most of the frame; the skip matters for envs whose pad
//     is partly or wholly out of view.
//  2. Triangle setup, 256 triangles per round: each thread sets up one, clips its pixel box to the tile and appends the survivors to
//     a list in LDS (one wave-uniform broadcast read per list entry later on).
//  3. Raster: every thread OWNS 8 pixels of the tile (one column, every 4th row) and walks the list, keeping its z-buffer in registers.
//     No atomics: the nearest fragment is a minimum, which does not depend on the order the fragments arrive in, and each (triangle,
//     pixel) pair is computed with exactly mesh_depth_kernel's expressions - so the image is the same as a per-triangle scatter with an
//     atomicMin into LDS would give, without its load imbalance (the pad has ~160 large triangles: a handful per tile, one lane each).
//     Depths are compared as bit patterns like that atomicMin (positive floats order like their bits).
constexpr int kDeformStageMax = 2048;  // vertices staged in LDS (16 B each: 32 KB)
constexpr int kDeformBlock = 256;
constexpr int kDeformRows = kRasterTileH * kRasterTileW / kDeformBlock;  // pixels per thread (8)
static_assert(kRasterTileW == 64 && kDeformBlock / 64 * kDeformRows == kRasterTileH, "a wave owns whole 64-pixel tile rows");

//
// Vertex SOURCE: where the float64 world point of rendered vertex `sv` of env `env` comes from is the kernel's template parameter - the
// one thing the two entry points differ in.  Everything from the world point on (camera frame, rounding, projection, staging, tile skip,
// setup rounds, raster) is the one copy below.
//  - FemSurfaceVerts (tacex_depth_from_deformed_mesh): x[env][surf_ids[sv]], the FEM state.
//  - AffineBodyVerts (tacex_depth_from_affine_body): the affine body's state q (B,4,3) = (p, c1, c2, c3), c_k the columns of A, read in
//    place (UipcSim.q), applied to the rest vertex X (nv,3), one table for all envs: per component w = ((p + X0 c1) + X1 c2) + X2 c3 in
//    float64, separate multiplies and adds (no FMA in this file).  The 12 unknowns are the same for the whole workgroup.
// A source may also say that a tile can hold no fragment (`out_of_tile`, workgroup-uniform): its vertices are then not staged for that tile.
// The pad's never does (its vertices are the bound); the body's tests the in-range slab of its bounding sphere.
struct DeformArgs {
  const int* tris;        // (T,3) indices into the Vs rendered vertices
  const double* cam_pos;  // (B,3)
  const double* rot_inv;  // (B,3,3) world -> camera rotation (row-major)
  float* depth;           // (B,H,W)
  int Vs, T, B, H, W;
  float fx, fy, cx, cy, near_m, far_m;
  int tiles_x, tiles_y, staged;
};

struct FemSurfaceVerts {
  const double* x;      // (B,V,3) world positions
  const int* surf_ids;  // (Vs,) vertex ids into x
  int V;
  struct Env {
    const double* xb;
    const int* surf_ids;
    __device__ __forceinline__ void world(int sv, double w[3]) const {
      const size_t vi = (size_t)surf_ids[sv] * 3;
      w[0] = xb[vi]; w[1] = xb[vi + 1]; w[2] = xb[vi + 2];
    }
    // (no bound on the pad's vertices cheaper than projecting them)
    __device__ __forceinline__ bool out_of_tile(const DeformArgs&, const double*, const double*, int, int, int, int, float*) const { return false; }
  };
  __device__ __forceinline__ Env env(int e) const { return Env{x + (size_t)e * V * 3, surf_ids}; }
};

struct AffineBodyVerts {
  const double* X;  // (Vs,3) rest vertices, body frame
  const double* q;  // (B,4,3) p | c1 | c2 | c3
  struct Env {
    const double* X;
    const double* q;  // this env's 12 unknowns
    __device__ __forceinline__ void world(int sv, double w[3]) const {
      const double X0 = X[3 * sv], X1 = X[3 * sv + 1], X2 = X[3 * sv + 2];
#pragma unroll
      for (int i = 0; i < 3; ++i) w[i] = ((q[i] + X0 * q[3 + i]) + X1 * q[6 + i]) + X2 * q[9 + i];
    }
    // Workgroup-uniform: true when the tile [x0, x1) x [y0, y1) can hold no fragment of the body.  The staging loop - which forms the
    // float64 world point of every vertex once per TILE, 40 tiles per 320 x 240 env - is skipped then (measured,
    // profiles/ball_depth_bench.md).  Conservative float32 bound: |A X| <= |A|_2 |X| with |A|_2^2 = the largest eigenvalue of A^T A <= its
    // largest absolute row sum (Gershgorin; A^T A is close to I for the stiff body), so the body - vertices and triangles - lies in the
    // sphere of radius r = |A|_2 max|X| about its origin c = R (p - cam_pos) in the camera frame (R a rotation).  A fragment also has
    // near <= z <= far: it lies in the slab of the sphere between zlo = max(c.z - r, near) and zhi = min(c.z + r, far), whose points are
    // within rho = sqrt(r^2 - dist^2) of the sphere's axis (dist: from c.z to the slab, 0 inside it) - for the ball pressed into the pad
    // the small cap in front of the far plane, not the ball's silhouette.  The slab's screen bounds are taken like the bounding sphere's
    // in raster_tile_empty, with its slack (0.1 % of the radius, one pixel) for the rounding of the bound.
    // `red`: kDeformBlock / 64 floats of LDS.
    __device__ __forceinline__ bool out_of_tile(const DeformArgs& a, const double* cp, const double* R, int x0, int x1, int y0, int y1,
                                                float* red) const {
      float r2 = 0.0f;
      for (int v = threadIdx.x; v < a.Vs; v += kDeformBlock) {
        const float X0 = (float)X[3 * v], X1 = (float)X[3 * v + 1], X2 = (float)X[3 * v + 2];
        r2 = fmaxf(r2, (X0 * X0 + X1 * X1) + X2 * X2);
      }
      r2 = wave_max(r2);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r2;
      __syncthreads();
      for (int w = 0; w < kDeformBlock / 64; ++w) r2 = fmaxf(r2, red[w]);
      __syncthreads();  // (the caller reuses `red`)
      float c[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) c[i] = (float)q[3 + i];  // c[3 k + i]: component i of column k of A
      float g[3][3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) g[j][k] = fabsf((c[3 * j] * c[3 * k] + c[3 * j + 1] * c[3 * k + 1]) + c[3 * j + 2] * c[3 * k + 2]);
      const float a2 = fmaxf(fmaxf((g[0][0] + g[0][1]) + g[0][2], (g[1][0] + g[1][1]) + g[1][2]), (g[2][0] + g[2][1]) + g[2][2]);
      const double d0 = q[0] - cp[0], d1 = q[1] - cp[1], d2 = q[2] - cp[2];
      const float bx = (float)((R[0] * d0 + R[1] * d1) + R[2] * d2), by = (float)((R[3] * d0 + R[4] * d1) + R[5] * d2);
      const float bz = (float)((R[6] * d0 + R[7] * d1) + R[8] * d2);
      const float m = 1.001f, r = (sqrtf(r2) * sqrtf(a2)) * m;
      if (bz + r < a.near_m || bz - r > a.far_m) return true;
      const float zlo = fmaxf(bz - r, a.near_m), zhi = fminf(bz + r, a.far_m);
      if (!(zlo > 1e-4f)) return false;
      const float dist = bz > zhi ? bz - zhi : (bz < zlo ? zlo - bz : 0.0f);
      const float rho = sqrtf(fmaxf(r * r - dist * dist, 0.0f)) * m;
      const float ulo = fminf(a.fx * (bx - rho) / zlo, a.fx * (bx - rho) / zhi) + a.cx - 1.0f;
      const float uhi = fmaxf(a.fx * (bx + rho) / zlo, a.fx * (bx + rho) / zhi) + a.cx + 1.0f;
      const float vlo = fminf(a.fy * (by - rho) / zlo, a.fy * (by - rho) / zhi) + a.cy - 1.0f;
      const float vhi = fmaxf(a.fy * (by + rho) / zlo, a.fy * (by + rho) / zhi) + a.cy + 1.0f;
      return uhi < (float)x0 || ulo > (float)x1 || vhi < (float)y0 || vlo > (float)y1;
    }
  };
  __device__ __forceinline__ Env env(int e) const { return Env{X, q + (size_t)e * 12}; }
};

struct TriSetup {  // one list entry (64 B): what the per-pixel test of mesh_depth_kernel reads
  float sx[3], sy[3], iz[3], area, inv_area;
  int jx0, jx1, iy0, iy1, pad;
};

// (sx, sy, 1/z, front) of rendered vertex `sv` of the env - mesh_depth_kernel's projection of the float32 camera-frame point
template <class VertsEnv>
__device__ __forceinline__ float4 project_deformed(const DeformArgs& a, const VertsEnv& verts, const double* cp, const double* R, int sv) {
  double w[3];
  verts.world(sv, w);
  const double d0 = w[0] - cp[0], d1 = w[1] - cp[1], d2 = w[2] - cp[2];
  const float px = (float)((R[0] * d0 + R[1] * d1) + R[2] * d2);
  const float py = (float)((R[3] * d0 + R[4] * d1) + R[5] * d2);
  const float pz = (float)((R[6] * d0 + R[7] * d1) + R[8] * d2);
  const float iz = 1.0f / pz;
  return make_float4((a.fx * px) * iz + a.cx, (a.fy * py) * iz + a.cy, iz, pz > 1e-6f ? 1.0f : 0.0f);
}

// ---- Contact traction of the pad's face as an image (tacex_traction_image_from_deformed_mesh) -----------------------------------------
// fem_traction_image_kernel is deformed_mesh_depth_kernel<FemSurfaceVerts> with a per-vertex quantity carried through it: the body below
// is the one copy of both (TRACTION is a compile-time switch; the depth kernels compile to what they were without it).
//  - Vertex traction [Pa], camera frame, of rendered vertex sv with v = surf_ids[sv]: tw[i] = f[env][v][i] / area[v] (float64 division),
//    tc[i] = (Rinv[i][0] tw[0] + Rinv[i][1] tw[1]) + Rinv[i][2] tw[2] in float64, rounded ONCE to float32; zero where area[v] <= 0.
//    Up to kTractionStageMax vertices are computed once per workgroup into LDS (12 B each, behind the projections); above that they are
//    computed per winner with the same function, so the image is the same.
//  - Fragments are the depth kernel's.  The WINNER of a pixel is the fragment with the smallest (bits of z, triangle index t in tris):
//    the list in LDS is filled through an atomicAdd, so fragments arrive in an order that differs from run to run, and at a pixel centre on
//    an edge two triangles share both give a fragment, often with the same z.  The key (z bits, t) lives in registers next to each other.
//  - After the walk the winner's l_k, 1/z_k and z are formed AGAIN with the expressions of the walk (same bits) and the traction is
//    interpolated perspective-correctly: w_k = (l_k * iz[k]) * z, t[i] = (w0 t0[i] + w1 t1[i]) + w2 t2[i].  A pixel without a fragment
//    gets 0, 0, 0.  Plain stores, no float atomics.
constexpr int kTractionStageMax = 1536;  // vertices whose traction is staged in LDS: 1536 * (16 + 12) B = 42 KB, with the 16 KB triangle
                                         // list under the 64 KB a launch gets without hipFuncSetAttribute (2048 * 28 B would not be)
struct TractionArgs {
  const double* force;  // (B,V,3) world frame [N]
  const double* area;   // (V,) [m^2]
  float* traction;      // (B,H,W,3) camera frame [Pa]
  int tstaged;
};
struct NoTraction {};

struct float3s { float x, y, z; };  // (12 B: float3 of the HIP headers is 12 B too, but carries operators this file does not use)

__device__ __forceinline__ float3s vertex_traction(const double* fb, const double* area, const int* surf_ids, const double* R, int sv) {
  const int v = surf_ids[sv];
  const double ar = area[v];
  float3s t{0.0f, 0.0f, 0.0f};
  if (ar > 0.0) {
    const double w0 = fb[(size_t)v * 3] / ar, w1 = fb[(size_t)v * 3 + 1] / ar, w2 = fb[(size_t)v * 3 + 2] / ar;
    t.x = (float)((R[0] * w0 + R[1] * w1) + R[2] * w2);
    t.y = (float)((R[3] * w0 + R[4] * w1) + R[5] * w2);
    t.z = (float)((R[6] * w0 + R[7] * w1) + R[8] * w2);
  }
  return t;
}

template <class Verts, bool TRACTION, class Extra>
__device__ __forceinline__ void deformed_raster(const DeformArgs& a, const Verts& src, const Extra& tr) {
  extern __shared__ float4 stage[];  // (min(Vs, kDeformStageMax),) when a.staged [| (Vs,) float3s tractions when tr.tstaged]
  __shared__ TriSetup list[kDeformBlock];
  __shared__ float box[4][kDeformBlock / 64];
  __shared__ int count;
  const int per_env = a.tiles_x * a.tiles_y;
  const int env = blockIdx.x / per_env, tile = blockIdx.x - env * per_env;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * kRasterTileW, y0 = ty * kRasterTileH;
  const int x1 = min(x0 + kRasterTileW, a.W), y1 = min(y0 + kRasterTileH, a.H);  // exclusive
  const typename Verts::Env verts = src.env(env);
  const double* cp = a.cam_pos + (size_t)env * 3;
  const double* R = a.rot_inv + (size_t)env * 9;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // a source that can bound its vertices cheaply says so here: nothing is staged then, the vertex box below stays empty and the tile is
  // stored as +inf by the one store at the end
  const bool out = verts.out_of_tile(a, cp, R, x0, x1, y0, y1, box[0]);

  float minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
  for (int v = out ? a.Vs : tid; v < a.Vs; v += kDeformBlock) {
    const float4 p = project_deformed(a, verts, cp, R, v);
    if (a.staged) stage[v] = p;
    if (p.w != 0.0f) { minx = fminf(minx, p.x); maxx = fmaxf(maxx, p.x); miny = fminf(miny, p.y); maxy = fmaxf(maxy, p.y); }
  }
  minx = wave_min(minx); maxx = wave_max(maxx); miny = wave_min(miny); maxy = wave_max(maxy);
  if (lane == 0) { box[0][wave] = minx; box[1][wave] = maxx; box[2][wave] = miny; box[3][wave] = maxy; }
  if (tid == 0) count = 0;
  __syncthreads();
  for (int w = 0; w < kDeformBlock / 64; ++w) {
    minx = fminf(minx, box[0][w]); maxx = fmaxf(maxx, box[1][w]); miny = fminf(miny, box[2][w]); maxy = fmaxf(maxy, box[3][w]);
  }
  // pixel centres j + 0.5 the box reaches: ceil(minx - 0.5) ... floor(maxx - 0.5), as for one triangle (no front vertex: empty box)
  const bool tile_empty = !(floorf(maxx - 0.5f) >= (float)x0 && ceilf(minx - 0.5f) <= (float)(x1 - 1) &&
                            floorf(maxy - 0.5f) >= (float)y0 && ceilf(miny - 0.5f) <= (float)(y1 - 1));

  const double* fb = nullptr;  // this env's vertex forces
  float3s* tstage = nullptr;
  if constexpr (TRACTION) {
    fb = tr.force + (size_t)env * src.V * 3;
    tstage = reinterpret_cast<float3s*>(stage + (a.staged ? a.Vs : 0));
    // (visible to the interpolation at the end: every setup round below has a barrier)
    if (tr.tstaged && !tile_empty)
      for (int v = tid; v < a.Vs; v += kDeformBlock) tstage[v] = vertex_traction(fb, tr.area, src.surf_ids, R, v);
  }

  unsigned zb[kDeformRows];
  int tw[TRACTION ? kDeformRows : 1];  // the winner's triangle, -1: no fragment
#pragma unroll
  for (int k = 0; k < kDeformRows; ++k) zb[k] = 0x7f800000u;  // +inf
  if constexpr (TRACTION) {
#pragma unroll
    for (int k = 0; k < kDeformRows; ++k) tw[k] = -1;
  }
  const int col = lane, row0 = wave;  // this thread's pixels: (y0 + row0 + 4k, x0 + col)
  const float pxc = (float)(x0 + col) + 0.5f;
  for (int base = tile_empty ? a.T : 0; base < a.T; base += kDeformBlock) {
    const int t = base + tid;
    if (t < a.T) {
      float sx[3], sy[3], iz[3];
      bool ok = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int sv = a.tris[3 * t + k];
        const float4 p = a.staged ? stage[sv] : project_deformed(a, verts, cp, R, sv);
        sx[k] = p.x; sy[k] = p.y; iz[k] = p.z;
        ok = ok && p.w != 0.0f;
      }
      if (ok) {
        const float mnx = fminf(fminf(sx[0], sx[1]), sx[2]), mxx = fmaxf(fmaxf(sx[0], sx[1]), sx[2]);
        const float mny = fminf(fminf(sy[0], sy[1]), sy[2]), mxy = fmaxf(fmaxf(sy[0], sy[1]), sy[2]);
        const int jx0 = max(x0, (int)ceilf(mnx - 0.5f)), jx1 = min(x1 - 1, (int)floorf(mxx - 0.5f));
        const int iy0 = max(y0, (int)ceilf(mny - 0.5f)), iy1 = min(y1 - 1, (int)floorf(mxy - 0.5f));
        const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
        if (jx0 <= jx1 && iy0 <= iy1 && area != 0.0f) {
          TriSetup& e = list[atomicAdd(&count, 1)];
#pragma unroll
          for (int k = 0; k < 3; ++k) { e.sx[k] = sx[k]; e.sy[k] = sy[k]; e.iz[k] = iz[k]; }
          e.area = area; e.inv_area = 1.0f / area;
          e.jx0 = jx0; e.jx1 = jx1; e.iy0 = iy0; e.iy1 = iy1;
          if constexpr (TRACTION) e.pad = t;
        }
      }
    }
    __syncthreads();
    const int n = count;
    for (int l = 0; l < n; ++l) {
      const TriSetup& e = list[l];
      if (x0 + col < e.jx0 || x0 + col > e.jx1) continue;
#pragma unroll
      for (int k = 0; k < kDeformRows; ++k) {
        const int i = y0 + row0 + 4 * k;
        if (i < e.iy0 || i > e.iy1) continue;
        const float py = (float)i + 0.5f, px = pxc;
        const float e0 = (e.sx[2] - e.sx[1]) * (py - e.sy[1]) - (e.sy[2] - e.sy[1]) * (px - e.sx[1]);
        const float e1 = (e.sx[0] - e.sx[2]) * (py - e.sy[2]) - (e.sy[0] - e.sy[2]) * (px - e.sx[2]);
        const float e2 = (e.sx[1] - e.sx[0]) * (py - e.sy[0]) - (e.sy[1] - e.sy[0]) * (px - e.sx[0]);
        const bool in = e.area > 0.0f ? (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) : (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
        if (!in) continue;
        const float l0 = e0 * e.inv_area, l1 = e1 * e.inv_area, l2 = e2 * e.inv_area;
        const float invz = (l0 * e.iz[0] + l1 * e.iz[1]) + l2 * e.iz[2];
        const float z = 1.0f / invz;
        if (!(z >= a.near_m && z <= a.far_m)) continue;  // clipping range (also drops NaN)
        if constexpr (TRACTION) {
          const unsigned zu = __float_as_uint(z);
          // (a finite z: zu < +inf's bits, so the first fragment always wins against tw = -1)
          if (zu < zb[k] || (zu == zb[k] && e.pad < tw[k])) { zb[k] = zu; tw[k] = e.pad; }
        } else {
          zb[k] = min(zb[k], __float_as_uint(z));
        }
      }
    }
    __syncthreads();
    if (tid == 0) count = 0;
    __syncthreads();
  }
  if constexpr (TRACTION) {
    if (x0 + col < x1) {
#pragma unroll
      for (int k = 0; k < kDeformRows; ++k) {
        const int i = y0 + row0 + 4 * k;
        if (i >= y1) continue;
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        if (tw[k] >= 0) {
          float sx[3], sy[3], iz[3];
          float3s tv[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int sv = a.tris[3 * tw[k] + c];
            const float4 p = a.staged ? stage[sv] : project_deformed(a, verts, cp, R, sv);
            sx[c] = p.x; sy[c] = p.y; iz[c] = p.z;
            tv[c] = tr.tstaged ? tstage[sv] : vertex_traction(fb, tr.area, src.surf_ids, R, sv);
          }
          // the walk's expressions for this triangle and pixel: the same l_k and z, bit for bit
          const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
          const float inv_area = 1.0f / area;
          const float py = (float)i + 0.5f, px = pxc;
          const float e0 = (sx[2] - sx[1]) * (py - sy[1]) - (sy[2] - sy[1]) * (px - sx[1]);
          const float e1 = (sx[0] - sx[2]) * (py - sy[2]) - (sy[0] - sy[2]) * (px - sx[2]);
          const float e2 = (sx[1] - sx[0]) * (py - sy[0]) - (sy[1] - sy[0]) * (px - sx[0]);
          const float l0 = e0 * inv_area, l1 = e1 * inv_area, l2 = e2 * inv_area;
          const float invz = (l0 * iz[0] + l1 * iz[1]) + l2 * iz[2];
          const float z = 1.0f / invz;
          const float w0 = (l0 * iz[0]) * z, w1 = (l1 * iz[1]) * z, w2 = (l2 * iz[2]) * z;
          o0 = (w0 * tv[0].x + w1 * tv[1].x) + w2 * tv[2].x;
          o1 = (w0 * tv[0].y + w1 * tv[1].y) + w2 * tv[2].y;
          o2 = (w0 * tv[0].z + w1 * tv[1].z) + w2 * tv[2].z;
        }
        const size_t px_id = ((size_t)env * a.H + i) * a.W + x0 + col;
        float* o = tr.traction + px_id * 3;
        o[0] = o0; o[1] = o1; o[2] = o2;
        if (a.depth) a.depth[px_id] = __uint_as_float(zb[k]);
      }
    }
  } else {
    if (x0 + col < x1) {
#pragma unroll
      for (int k = 0; k < kDeformRows; ++k) {
        const int i = y0 + row0 + 4 * k;
        if (i < y1) a.depth[((size_t)env * a.H + i) * a.W + x0 + col] = __uint_as_float(zb[k]);
      }
    }
  }
}

template <class Verts>
__global__ __launch_bounds__(kDeformBlock) void deformed_mesh_depth_kernel(DeformArgs a, Verts src) {
  deformed_raster<Verts, false>(a, src, NoTraction{});
}

__global__ __launch_bounds__(kDeformBlock) void fem_traction_image_kernel(DeformArgs a, FemSurfaceVerts src, TractionArgs tr) {
  deformed_raster<FemSurfaceVerts, true>(a, src, tr);
}

// tiles, staging and the launch of either instantiation (a: everything but tiles_x / tiles_y / staged filled in)
template <class Verts>
static int launch_deformed_mesh_depth(DeformArgs a, Verts src, hipStream_t stream) {
  a.tiles_x = (a.W + kRasterTileW - 1) / kRasterTileW; a.tiles_y = (a.H + kRasterTileH - 1) / kRasterTileH;
  if ((size_t)a.B * a.tiles_x * a.tiles_y >= (size_t)1 << 31) { set_error("deformed_mesh_depth_kernel: grid too large"); return 2; }
  a.staged = a.Vs <= kDeformStageMax;
  const size_t lds = a.staged ? (size_t)a.Vs * sizeof(float4) : 0;
  hipLaunchKernelGGL(deformed_mesh_depth_kernel<Verts>, dim3((unsigned)(a.B * a.tiles_x * a.tiles_y)), dim3(kDeformBlock), lds, stream, a, src);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("deformed_mesh_depth_kernel: %s", hipGetErrorString(e)); return 1; }
  return 0;
}

}  // namespace tacex

extern "C" int tacex_depth_from_mesh(const float* verts_dev, const int32_t* tris_dev, int num_verts, int num_tris,
                                     const float* pos_dev, const float* quat_dev, float fx, float fy, float cx, float cy, float near_clip_m,
                                     float far_clip_m, const float* bounding_sphere, float* depth_m_dev, int num_envs, int height,
                                     int width, void* stream) {
  using namespace tacex;
  if (!verts_dev || !tris_dev || !pos_dev || !quat_dev || !depth_m_dev) { set_error("tacex_depth_from_mesh: null buffer"); return 2; }
  if (num_verts <= 0 || num_tris <= 0 || height <= 0 || width <= 0) { set_error("tacex_depth_from_mesh: empty mesh or image"); return 2; }
  if (!(near_clip_m >= 0.0f) || !(far_clip_m > near_clip_m)) { set_error("tacex_depth_from_mesh: clipping range (%g, %g)", near_clip_m, far_clip_m); return 2; }
  if (num_envs <= 0) return 0;
  RasterArgs a{};
  a.verts = verts_dev; a.tris = tris_dev; a.pos = pos_dev; a.quat = quat_dev; a.depth = depth_m_dev;
  a.V = num_verts; a.T = num_tris; a.B = num_envs; a.H = height; a.W = width;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.near_m = near_clip_m; a.far_m = far_clip_m;
  if (bounding_sphere) { a.bs[0] = bounding_sphere[0]; a.bs[1] = bounding_sphere[1]; a.bs[2] = bounding_sphere[2]; a.bs[3] = bounding_sphere[3]; }
  else a.bs[3] = -1.0f;
  a.tiles_x = (width + kRasterTileW - 1) / kRasterTileW; a.tiles_y = (height + kRasterTileH - 1) / kRasterTileH;
  hipLaunchKernelGGL(mesh_depth_kernel, dim3((unsigned)(num_envs * a.tiles_x * a.tiles_y)), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("mesh_depth_kernel: %s", hipGetErrorString(e)); return 1; }
  return 0;
}


extern "C" int tacex_depth_from_deformed_mesh(const double* x_dev, int num_verts, const int32_t* surf_ids_dev, int num_surf_verts,
                                              const int32_t* tris_dev, int num_tris, const double* cam_pos_dev, const double* cam_rot_inv_dev,
                                              float fx, float fy, float cx, float cy, float near_clip_m, float far_clip_m, float* depth_m_dev,
                                              int num_envs, int height, int width, void* stream) {
  using namespace tacex;
  if (!x_dev || !surf_ids_dev || !tris_dev || !cam_pos_dev || !cam_rot_inv_dev || !depth_m_dev) {
    set_error("tacex_depth_from_deformed_mesh: null buffer"); return 2;
  }
  if (num_verts <= 0 || num_surf_verts <= 0 || num_surf_verts > num_verts || num_tris <= 0 || num_envs <= 0 || height <= 0 || width <= 0) {
    set_error("tacex_depth_from_deformed_mesh: bad counts (verts %d, surface verts %d, tris %d, envs %d, image %dx%d)", num_verts,
              num_surf_verts, num_tris, num_envs, width, height);
    return 2;
  }
  if (!(near_clip_m >= 0.0f) || !(far_clip_m > near_clip_m)) {
    set_error("tacex_depth_from_deformed_mesh: clipping range (%g, %g)", near_clip_m, far_clip_m); return 2;
  }
  DeformArgs a{};
  a.tris = tris_dev; a.cam_pos = cam_pos_dev; a.rot_inv = cam_rot_inv_dev; a.depth = depth_m_dev;
  a.Vs = num_surf_verts; a.T = num_tris; a.B = num_envs; a.H = height; a.W = width;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.near_m = near_clip_m; a.far_m = far_clip_m;
  return launch_deformed_mesh_depth(a, FemSurfaceVerts{x_dev, surf_ids_dev, num_verts}, (hipStream_t)stream);
}


extern "C" int tacex_traction_image_from_deformed_mesh(const double* x_dev, int num_verts, const int32_t* surf_ids_dev, int num_surf_verts,
                                                       const int32_t* tris_dev, int num_tris, const double* vertex_force_dev,
                                                       const double* vertex_area_dev, const double* cam_pos_dev,
                                                       const double* cam_rot_inv_dev, float fx, float fy, float cx, float cy,
                                                       float near_clip_m, float far_clip_m, float* traction_dev, float* depth_m_dev,
                                                       int num_envs, int height, int width, void* stream) {
  using namespace tacex;
  if (!x_dev || !surf_ids_dev || !tris_dev || !vertex_force_dev || !vertex_area_dev || !cam_pos_dev || !cam_rot_inv_dev || !traction_dev) {
    set_error("tacex_traction_image_from_deformed_mesh: null buffer"); return 2;
  }
  if (num_verts <= 0 || num_surf_verts <= 0 || num_surf_verts > num_verts || num_tris <= 0 || num_envs <= 0 || height <= 0 || width <= 0) {
    set_error("tacex_traction_image_from_deformed_mesh: bad counts (verts %d, surface verts %d, tris %d, envs %d, image %dx%d)", num_verts,
              num_surf_verts, num_tris, num_envs, width, height);
    return 2;
  }
  if (!(near_clip_m >= 0.0f) || !(far_clip_m > near_clip_m)) {
    set_error("tacex_traction_image_from_deformed_mesh: clipping range (%g, %g)", near_clip_m, far_clip_m); return 2;
  }
  DeformArgs a{};
  a.tris = tris_dev; a.cam_pos = cam_pos_dev; a.rot_inv = cam_rot_inv_dev; a.depth = depth_m_dev;
  a.Vs = num_surf_verts; a.T = num_tris; a.B = num_envs; a.H = height; a.W = width;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.near_m = near_clip_m; a.far_m = far_clip_m;
  a.tiles_x = (a.W + kRasterTileW - 1) / kRasterTileW; a.tiles_y = (a.H + kRasterTileH - 1) / kRasterTileH;
  if ((size_t)a.B * a.tiles_x * a.tiles_y >= (size_t)1 << 31) { set_error("fem_traction_image_kernel: grid too large"); return 2; }
  a.staged = a.Vs <= kDeformStageMax;
  TractionArgs tr{vertex_force_dev, vertex_area_dev, traction_dev, a.Vs <= kTractionStageMax};
  const size_t lds = (a.staged ? (size_t)a.Vs * sizeof(float4) : 0) + (tr.tstaged ? (size_t)a.Vs * sizeof(float3s) : 0);
  hipLaunchKernelGGL(fem_traction_image_kernel, dim3((unsigned)(a.B * a.tiles_x * a.tiles_y)), dim3(kDeformBlock), lds, (hipStream_t)stream, a,
                     FemSurfaceVerts{x_dev, surf_ids_dev, num_verts}, tr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("fem_traction_image_kernel: %s", hipGetErrorString(e)); return 1; }
  return 0;
}


extern "C" int tacex_depth_from_affine_body(const double* rest_verts_dev, int num_verts, const int32_t* tris_dev, int num_tris,
                                            const double* q_dev, const double* cam_pos_dev, const double* cam_rot_inv_dev, float fx, float fy,
                                            float cx, float cy, float near_clip_m, float far_clip_m, float* depth_m_dev, int num_envs,
                                            int height, int width, void* stream) {
  using namespace tacex;
  if (!rest_verts_dev || !tris_dev || !q_dev || !cam_pos_dev || !cam_rot_inv_dev || !depth_m_dev) {
    set_error("tacex_depth_from_affine_body: null buffer"); return 2;
  }
  if (num_verts <= 0 || num_tris <= 0 || num_envs <= 0 || height <= 0 || width <= 0) {
    set_error("tacex_depth_from_affine_body: bad counts (verts %d, tris %d, envs %d, image %dx%d)", num_verts, num_tris, num_envs, width,
              height);
    return 2;
  }
  if (!(near_clip_m >= 0.0f) || !(far_clip_m > near_clip_m)) {
    set_error("tacex_depth_from_affine_body: clipping range (%g, %g)", near_clip_m, far_clip_m); return 2;
  }
  DeformArgs a{};
  a.tris = tris_dev; a.cam_pos = cam_pos_dev; a.rot_inv = cam_rot_inv_dev; a.depth = depth_m_dev;
  a.Vs = num_verts; a.T = num_tris; a.B = num_envs; a.H = height; a.W = width;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.near_m = near_clip_m; a.far_m = far_clip_m;
  return launch_deformed_mesh_depth(a, AffineBodyVerts{rest_verts_dev, q_dev}, (hipStream_t)stream);
}


extern "C" int tacex_depth_from_mesh_library(const float* verts_dev, const int32_t* tris_dev, const int32_t* mesh_tris_dev,
                                             const float* mesh_spheres_dev, int num_meshes, int max_mesh_tris, const int32_t* mesh_ids_dev,
                                             const float* pos_dev, const float* quat_dev, float fx, float fy, float cx, float cy,
                                             float near_clip_m, float far_clip_m, float* depth_m_dev, int num_envs, int height, int width,
                                             void* stream) {
  using namespace tacex;
  if (!verts_dev || !tris_dev || !mesh_tris_dev || !pos_dev || !quat_dev || !depth_m_dev) {
    set_error("tacex_depth_from_mesh_library: null buffer"); return 2;
  }
  if (num_meshes <= 0 || max_mesh_tris <= 0 || height <= 0 || width <= 0) {
    set_error("tacex_depth_from_mesh_library: empty library or image (meshes %d, max triangles %d, image %dx%d)", num_meshes, max_mesh_tris,
              width, height);
    return 2;
  }
  if (!(near_clip_m >= 0.0f) || !(far_clip_m > near_clip_m)) {
    set_error("tacex_depth_from_mesh_library: clipping range (%g, %g)", near_clip_m, far_clip_m); return 2;
  }
  if (num_envs <= 0) return 0;
  RasterLibArgs L{};
  RasterArgs& a = L.r;
  a.verts = verts_dev; a.tris = tris_dev; a.pos = pos_dev; a.quat = quat_dev; a.depth = depth_m_dev;
  a.B = num_envs; a.H = height; a.W = width;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.near_m = near_clip_m; a.far_m = far_clip_m;
  a.bs[3] = -1.0f;
  a.tiles_x = (width + kRasterTileW - 1) / kRasterTileW; a.tiles_y = (height + kRasterTileH - 1) / kRasterTileH;
  L.mesh_tris = mesh_tris_dev; L.mesh_bs = mesh_spheres_dev; L.ids = mesh_ids_dev; L.K = num_meshes;
  const int chunks = (max_mesh_tris + kLibChunk - 1) / kLibChunk;
  const size_t pairs = (size_t)num_envs * a.tiles_x * a.tiles_y;
  if (pairs * (size_t)std::max(chunks - 1, 1) >= (size_t)1 << 31) { set_error("tacex_depth_from_mesh_library: grid too large"); return 2; }
  L.chunk0 = 0; L.nchunk = 1;
  hipLaunchKernelGGL(mesh_library_depth_kernel<false>, dim3((unsigned)pairs), dim3(256), 0, (hipStream_t)stream, L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("mesh_library_depth_kernel: %s", hipGetErrorString(e)); return 1; }
  if (chunks > 1) {
    L.chunk0 = 1; L.nchunk = chunks - 1;
    hipLaunchKernelGGL(mesh_library_depth_kernel<true>, dim3((unsigned)(pairs * L.nchunk)), dim3(256), 0, (hipStream_t)stream, L);
    e = hipGetLastError();
    if (e != hipSuccess) { set_error("mesh_library_depth_kernel: %s", hipGetErrorString(e)); return 1; }
  }
  return 0;
}
