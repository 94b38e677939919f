// Stand-alone check of tacex_amd/csrc/fem_layout.h (built and run by test_fem_workspace_layout.py with a host compiler): every region
// offset and total of the two FEM workspaces equals the expression the host layer used before the layouts got a header of their own
// (written out below as literals), the regions are in order, do not overlap and end within the total, and they are aligned.
#include <stdio.h>

#include "fem_layout.h"

static int failures = 0;
#define CHECK(cond)                                                                                             \
  do {                                                                                                          \
    if (!(cond)) { ++failures; printf("FAIL %s:%d (V=%d T=%d B=%d nv=%d nt=%d): %s\n", __FILE__, __LINE__, V, T, B, nv, nt, #cond); } \
  } while (0)

struct Region { const char* name; size_t begin_bytes, length_bytes, align; };

// in order, no overlap, aligned, the last one ends within total_bytes
static void check_regions(const Region* r, int n, size_t total_bytes, int V, int T, int B, int nv, int nt) {
  for (int i = 0; i < n; ++i) {
    CHECK(r[i].begin_bytes % r[i].align == 0);
    CHECK(r[i].length_bytes > 0);
    if (i + 1 < n) CHECK(r[i].begin_bytes + r[i].length_bytes <= r[i + 1].begin_bytes);
  }
  CHECK(r[n - 1].begin_bytes + r[n - 1].length_bytes <= total_bytes);
}

int main() {
  const int Vs[] = {4, 495, 2232}, Ts[] = {1, 1920}, Bs[] = {1, 2, 3, 512};
  const int bodies[][2] = {{4, 4}, {42, 80}};
  int cases = 0;
  for (int V : Vs)
    for (int T : Ts)
      for (int B : Bs) {
        const size_t b = (size_t)B, v = (size_t)V, t = (size_t)T, D = sizeof(double);
        {
          const int nv = 0, nt = 0;
          CHECK(tacex::newton_ws_doubles(V, T) == 36 * t + 45 * v);
          const tacex::StepLayout L(V, T, B);
          const size_t N = b * (36 * t + 45 * v);
          CHECK(L.x_prev == N);
          CHECK(L.dx == N + b * v * 3);
          CHECK(L.disp == N + b * v * 3 + b);
          CHECK(L.ind_prev == N + b * v * 3 + b + 3 * b);
          CHECK(L.env_order == N + b * v * 3 + b + 3 * b + 3 * b + 1);
          CHECK(L.total == N + b * 3 * v + 7 * b + 8 + (b + 1) / 2);
          const Region r[] = {{"x_prev", L.x_prev * D, 3 * b * v * D, 8}, {"dx", L.dx * D, b * D, 8},
                              {"disp", L.disp * D, 3 * b * D, 8},         {"ind_prev", L.ind_prev * D, 3 * b * D, 8},
                              {"env_order", L.env_order * D, b * sizeof(int), 4}};
          check_regions(r, 5, L.total * D, V, T, B, nv, nt);
          ++cases;
        }
        for (const auto& body : bodies) {
          const int nv = body[0], nt = body[1];
          const size_t per_env = v + 9 * (size_t)nv + 4 * (size_t)nt + 4096 / 2 + (size_t)1024 * 14 + (size_t)1024 * (14 + 6);
          CHECK(tacex::ball_ws_doubles(V, T, nv, nt) == per_env);
          const tacex::BallLayout L(V, T, nv, nt, B);
          const size_t N = b * per_env, n3 = b * v * 3;
          CHECK(L.x_prev == N);
          CHECK(L.q_prev == N + n3);
          CHECK(L.xt == N + n3 + b * 12);
          CHECK(L.qt == N + n3 + b * 12 + n3);
          CHECK(L.q_last == N + 2 * n3 + b * 24);
          CHECK(L.env_order == N + 2 * n3 + b * 24 + b * 12 + 1);
          CHECK(L.blk == N + 2 * n3 + b * 24 + b * 12 + (b + 1) / 2 + 2);
          CHECK(L.total == N + b * 6 * v + b * 36 + 8 + (b + 1) / 2 + 2 + b * 16 * v);
          const Region r[] = {{"x_prev", L.x_prev * D, 3 * b * v * D, 8}, {"q_prev", L.q_prev * D, 12 * b * D, 8},
                              {"xt", L.xt * D, 3 * b * v * D, 8},         {"qt", L.qt * D, 12 * b * D, 8},
                              {"q_last", L.q_last * D, 12 * b * D, 8},    {"env_order", L.env_order * D, b * sizeof(int), 4},
                              {"blk", L.blk * D, 16 * b * v * D, 8}};
          check_regions(r, 7, L.total * D, V, T, B, nv, nt);
          ++cases;
        }
      }
  printf("%d layouts checked, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
