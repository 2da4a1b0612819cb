// Stand-alone host program for the scene table of csrc/ragged.h: the host fill's accept / reject decisions, the entries
// past B, and the unrolled lookup against the binary search.  Every offsets array is an exactly sized heap array, so a read
// past it is an out-of-bounds access that a sanitizer build reports (g++ -fsanitize=address,undefined); without sanitizers
// the program still verifies the decisions.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../pq3d_amd/csrc/ragged.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static std::vector<int64_t> offsets_of(const std::vector<long long>& lens) {
  std::vector<int64_t> off(lens.size() + 1, 0);
  for (size_t b = 0; b < lens.size(); ++b) off[b + 1] = off[b] + lens[b];
  return off;
}

template <int MAXB> static bool fills(const std::vector<int64_t>& off, int B, long long max_scene, long long max_total) {
  SceneTable<MAXB> t;
  const std::string e = scene_table_fill(t, off.empty() ? nullptr : off.data(), B, max_scene, max_total, "who");
  EXPECT(e.empty() || e.rfind("who: ", 0) == 0);       // the error text starts with the entry point's name
  if (e.empty()) {
    EXPECT(t.B == B);
    for (int b = 0; b <= MAXB; ++b) EXPECT(t.off[b] == off[b < B ? b : B]);     // entries past B repeat off[B]
  }
  return e.empty();
}

template <int MAXB> static void fill_cases() {
  const long long big = 1LL << 40;
  const std::vector<long long> ones(MAXB, 1);
  EXPECT(!fills<MAXB>(offsets_of({3}), 0, big, big));
  EXPECT(fills<MAXB>(offsets_of(ones), MAXB, big, big));
  EXPECT(fills<MAXB>(offsets_of({3}), 1, big, big));
  EXPECT(!fills<MAXB>(offsets_of(std::vector<long long>(MAXB + 1, 1)), MAXB + 1, big, big));
  EXPECT(!fills<MAXB>({}, 1, big, big));                                          // null offsets
  EXPECT(!fills<MAXB>({1, 4}, 1, big, big) && !fills<MAXB>({-1, 4}, 1, big, big));   // offsets[0] != 0
  EXPECT(fills<MAXB>(offsets_of({2, 5, 1}), 3, big, big));
  EXPECT(!fills<MAXB>(offsets_of({0, 5, 1}), 3, big, big) && !fills<MAXB>(offsets_of({2, 0, 1}), 3, big, big) &&
         !fills<MAXB>(offsets_of({2, 5, 0}), 3, big, big));                       // an empty scene: first, middle, last
  EXPECT(!fills<MAXB>({0, 5, 3}, 2, big, big) && !fills<MAXB>({0, INT64_MIN}, 1, big, big));   // descending offsets
  EXPECT(fills<MAXB>(offsets_of({2, 7, 7}), 3, 7, big) && !fills<MAXB>(offsets_of({2, 8, 7}), 3, 7, big));
  EXPECT(!fills<MAXB>({0, INT64_MAX}, 1, big, big));
  EXPECT(fills<MAXB>(offsets_of({2, 7, 7}), 3, big, 16) && !fills<MAXB>(offsets_of({2, 7, 8}), 3, big, 16));
}

template <int MAXB> static void lookup_cases(const std::vector<long long>& lens) {
  const int B = (int)lens.size();
  const std::vector<int64_t> off = offsets_of(lens);
  SceneTable<MAXB> t;
  EXPECT(scene_table_fill(t, off.data(), B, 1LL << 40, 1LL << 40, "who").empty());
  for (int b = 0; b < B; ++b) {
    if (b > 0) EXPECT(t.scene(off[b] - 1) == b - 1);
    EXPECT(t.scene(off[b]) == b);
    EXPECT(t.scene(off[b + 1] - 1) == b);
  }
  std::vector<int> scene(off[B], -1);       // every row: the unrolled lookup and the binary search agree
  for (int64_t i = 0; i < off[B]; ++i) {
    const int b = t.scene(i);
    EXPECT(b == scene_of(off.data(), B, (long)i) && b >= 0 && b < B && off[b] <= i && i < off[b + 1]);
    scene[i] = b;
  }
  // the same compare-and-sum over a table of another type (the first block of every scene)
  int blk0[MAXB + 1];
  for (int b = 0; b <= MAXB; ++b) blk0[b] = (int)t.off[b] * 2;
  for (int k = 0; k < blk0[B]; ++k) EXPECT(ragged_find(blk0, B, k) == scene[k / 2]);
}

int main() {
  fill_cases<8>();
  fill_cases<64>();
  lookup_cases<8>({5});
  lookup_cases<8>({1, 1, 1});
  lookup_cases<8>({3, 1, 70, 1, 1, 9, 2, 1});
  lookup_cases<64>({1, 1, 4, 1});
  std::vector<long long> lens(64);
  for (int b = 0; b < 64; ++b) lens[b] = 1 + b * 37 % 70;
  lookup_cases<64>(lens);
  lookup_cases<64>(std::vector<long long>(64, 1));
  EXPECT(grid_cap(0, 256) == 1 && grid_cap(1, 256) == 1 && grid_cap(257, 256) == 2 && grid_cap(1L << 40, 256) == 2048);
  std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
