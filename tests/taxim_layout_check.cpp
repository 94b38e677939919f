// Stand-alone check of tacex_amd/csrc/taxim_layout.h (built and run by test_taxim_workspace_layout.py with a host compiler): every region
// offset and total of the Taxim render workspace and of the shadow branch's regions behind it equals the expression the host layer used
// before the layouts got a header of their own (written out below as literals); the regions are in order, do not overlap, are 256-byte
// aligned and end at the total; a chunk's regions stay in front of the whole batch's contact rows; the observation scratch bound.
// With arguments "H W B [H W B ...]" the same checks run on those frames and frame counts instead of the built-in set.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "taxim_layout.h"

static int failures = 0;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    if (!(cond)) { ++failures; printf("FAIL %s:%d (H=%d W=%d B=%d n=%d): %s\n", __FILE__, __LINE__, H, W, B, n, #cond); } \
  } while (0)

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Region { const char* name; size_t begin, length; };

// in order, no overlap, 256-byte aligned, the last one ends at total
static void check_regions(const Region* r, int count, size_t total, int H, int W, int B) {
  const int n = 0;
  for (int i = 0; i < count; ++i) {
    CHECK(r[i].begin % 256 == 0);
    CHECK(r[i].length > 0);
    if (i + 1 < count) CHECK(r[i].begin + r[i].length <= r[i + 1].begin);
  }
  CHECK(align_up(r[count - 1].begin + r[count - 1].length, 256) == total);
}

int main(int argc, char** argv) {
  const int sizes[][2] = {{16, 16}, {17, 20}, {240, 320}, {480, 640}}, Bs[] = {1, 2, 63, 64, 65, 512, 2048};
  const int obs[][2] = {{32, 32}, {8, 64}, {64, 8}};
  struct Frames { int H, W, B; };
  std::vector<Frames> set;
  if (argc > 1) {
    if ((argc - 1) % 3) { printf("usage: %s [H W B]...\n", argv[0]); return 2; }
    for (int i = 1; i + 2 < argc; i += 3) set.push_back({atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2])});
  } else {
    for (const auto& hw : sizes)
      for (int B : Bs) set.push_back({hw[0], hw[1], B});
  }
  int cases = 0;
  for (const Frames& fr : set) {
      const int H = fr.H, W = fr.W, B = fr.B;
      int n = 0;
      const size_t px = (size_t)B * H * W;
      const size_t img = align_up((size_t)B * H * W * sizeof(float), 256), vec = align_up((size_t)B * sizeof(float), 256);
      {
        const tacex::PassLayout L(H, W, B);
        CHECK(L.z[0] == 0);
        CHECK(L.z[1] == img);
        CHECK(L.tmp == 2 * img);
        CHECK(L.shift_a == 3 * img);
        CHECK(L.shift_b == 3 * img + vec);
        CHECK(L.pdepth == 3 * img + 2 * vec);
        CHECK(L.rows == 3 * img + 3 * vec);
        CHECK(L.total == 3 * img + 3 * vec + align_up((size_t)B * 4 * sizeof(int), 256));
        const Region r[] = {{"z0", L.z[0], px * 4},       {"z1", L.z[1], px * 4},         {"tmp", L.tmp, px * 4},
                            {"shift_a", L.shift_a, (size_t)B * 4}, {"shift_b", L.shift_b, (size_t)B * 4}, {"pdepth", L.pdepth, (size_t)B * 4},
                            {"rows", L.rows, (size_t)B * 16}};
        check_regions(r, 7, L.total, H, W, B);
        // a pass walked in chunks of n frames lays the chunk out on the same base: all of it in front of the whole batch's rows
        for (int m : Bs) {
          if (m > B) continue;
          n = m;
          const tacex::PassLayout C(H, W, n);
          CHECK(C.z[0] + (size_t)n * H * W * 4 <= C.z[1]);
          CHECK(C.pdepth + (size_t)n * 4 <= C.rows);
          CHECK(C.rows <= L.rows);
        }
        n = 0;
        ++cases;
      }
      {
        const tacex::ShadowLayout S(H, W, B);
        CHECK(S.z == 0);
        CHECK(S.mask == img);
        CHECK(S.gdir == 2 * img);
        CHECK(S.raw == 3 * img);
        CHECK(S.shadow == 6 * img);
        CHECK(S.tmp == 9 * img);
        CHECK(S.total == 12 * img);
        const Region r[] = {{"z", S.z, px * 4},         {"mask", S.mask, px},         {"gdir", S.gdir, px * 4},
                            {"raw", S.raw, 3 * px * 4}, {"shadow", S.shadow, 3 * px * 4}, {"tmp", S.tmp, 3 * px * 4}};
        for (int i = 0; i + 1 < 6; ++i) CHECK(r[i].begin + r[i].length <= r[i + 1].begin);
        for (const Region& g : r) CHECK(g.begin % 256 == 0);
        CHECK(S.tmp + 3 * img == S.total);
        CHECK(tacex::PassLayout(H, W, B).total % 256 == 0);  // the shadow regions start where the pass layout ends
        ++cases;
      }
      for (const auto& o : obs) {
        const int oh = o[0], ow = o[1];
        const size_t want = (size_t)B * (size_t)(H * ow > oh * W ? H * ow : oh * W) * 3;
        CHECK(tacex::obs_resize_floats(H, W, oh, ow, B) == want);
        CHECK(tacex::obs_scratch_floats(H, W, oh, ow, B) == want + (size_t)B * oh * ow * 3);
        ++cases;
      }
      // the max takes each side somewhere in the set
      CHECK(H * 64 > 8 * W && 64 * W > H * 8);
  }
  printf("%d layouts checked, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
