// Stand-alone host program for the range checks of csrc/instance_targets.hip (instance_targets_check.h): every accepted value
// indexes an exactly sized heap table, so a wrong check is an out-of-bounds access that a sanitizer build reports
// (g++ -fsanitize=address,undefined); without sanitizers the program still verifies the accept / reject decisions.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pq3d_amd/csrc/instance_targets_check.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

int main() {
  const int cap = 4096;
  const int64_t big = int64_t(1) << 62;
  const int64_t probes[] = {INT64_MIN, -big, -big - 1, -4097, -4096, -3, -2, -1, 0, 1, 7, 4094, 4095, 4096, 4097, 65535, 65536,
                            (int64_t(1) << 31) - 1, int64_t(1) << 31, (int64_t(1) << 32) - 1, int64_t(1) << 32, big - 1, big, INT64_MAX};
  std::vector<int> first(cap + 1, 0);
  for (int64_t id : probes) {
    const int slot = pq_it_slot(id, cap);
    EXPECT((slot >= 0) == (id >= -1 && id < cap));
    if (slot >= 0) { EXPECT(slot == id + 1); first[slot] += 1; }
  }
  EXPECT(first[0] == 1 && first[1] == 1 && first[cap] == 1);
  for (int64_t limit : {int64_t(1), int64_t(8), int64_t(130), int64_t(1) << 24}) {
    std::vector<unsigned char> seen(limit, 0);
    for (int64_t seg : probes) {
      EXPECT(pq_it_seg_ok(seg, limit) == (seg >= 0 && seg < limit));
      if (pq_it_seg_ok(seg, limit)) seen[seg] = 1;
    }
    EXPECT(seen[0] == 1);
  }
  for (int64_t rows : {int64_t(0), int64_t(1), int64_t(3), int64_t(4096)})
    for (int64_t cols : {int64_t(0), int64_t(1), int64_t(130), int64_t(5000)}) {
      std::vector<unsigned char> table(rows * cols, 0);
      for (int64_t r : probes)
        for (int64_t c : probes) {
          const int64_t cell = pq_it_cell(r, c, rows, cols);
          EXPECT((cell >= 0) == (r >= 0 && r < rows && c >= 0 && c < cols));
          if (cell >= 0) { EXPECT(cell == r * cols + c); table[cell] = 1; }
        }
    }
  // the largest table the kernels form: rows, cols < 2^31 never overflow the product
  EXPECT(pq_it_cell((int64_t(1) << 31) - 2, (int64_t(1) << 31) - 2, (int64_t(1) << 31) - 1, (int64_t(1) << 31) - 1) ==
         ((int64_t(1) << 31) - 2) * ((int64_t(1) << 31) - 1) + ((int64_t(1) << 31) - 2));
  std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
