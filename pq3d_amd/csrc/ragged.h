// Helpers of the kernels that work on a batch of ragged scenes (segment.hip, instseg*.hip, scene_prep.hip,
// instance_targets.hip, scene_augment.hip): the by-value scene table with its lookup and its host fill, the binary search over
// a device offsets array, the block-wide exclusive scan, the capped grid size.  The first part is plain C++ shared with a
// stand-alone host program (tests/ragged_check_main.cpp), so that it runs on the CPU under sanitizers; the second part is
// device code.
#pragma once
#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
#define PQ_RG_HD __host__ __device__ __forceinline__
#define PQ_RG_UNROLL _Pragma("unroll")
#else
#define PQ_RG_HD inline
#define PQ_RG_UNROLL
#endif

// The number of entries first[1 .. N - 2] (of the leading B) that are <= i: for an ascending table of first rows (first[0] = 0)
// the scene b < B with first[b] <= i < first[b + 1].  Unrolled compare-and-sum, every index a compile-time constant: the
// table is a by-value kernel argument and stays in scalar registers.  A per-lane dynamic index (a search loop) sends the whole
// struct to private memory instead.
template <typename T, int N, typename I> PQ_RG_HD int ragged_find(const T (&first)[N], int B, I i) {
  int b = 0;
  PQ_RG_UNROLL
  for (int k = 1; k < N - 1; ++k) b += (k < B && i >= first[k]) ? 1 : 0;
  return b;
}

// Rows of scene b < B of a concatenated array: [off[b], off[b + 1]); entries past B repeat off[B] (= all rows).
template <int MAXB> struct SceneTable {
  int B;
  long long off[MAXB + 1];
  PQ_RG_HD int scene(long long i) const { return ragged_find(off, B, i); }     // 0 <= i < off[B]
};

// Fills t from the caller's host array of B + 1 offsets.  Returns "" or the argument error, which starts with `who` (the
// entry point's name): 1 <= B <= MAXB, offsets[0] = 0, every scene 1 .. max_scene rows, at most max_total rows in all.
template <int MAXB>
inline std::string scene_table_fill(SceneTable<MAXB>& t, const int64_t* offsets, int B, long long max_scene, long long max_total,
                                    const char* who) {
  const std::string w(who);
  if (!offsets || B < 1 || B > MAXB) return w + ": 1 <= B <= " + std::to_string(MAXB) + " scenes, offsets a host array";
  if (offsets[0] != 0) return w + ": offsets[0] must be 0";
  for (int b = 0; b < B; ++b) {          // (offsets[b] >= 0 here, so the difference of an accepted pair cannot overflow)
    if (offsets[b + 1] <= offsets[b]) return w + ": every scene needs at least one point";
    if (offsets[b + 1] - offsets[b] > max_scene) return w + ": at most " + std::to_string(max_scene) + " points per scene";
  }
  if (offsets[B] > max_total) return w + ": at most " + std::to_string(max_total) + " points per call";
  t.B = B;
  for (int b = 0; b <= MAXB; ++b) t.off[b] = offsets[b < B ? b : B];
  return std::string();
}

// largest b in [0, B) with off[b] <= i (i < off[B]): the scene of row i, for an offsets array in device memory (any B)
PQ_RG_HD int scene_of(const int64_t* __restrict__ off, int B, long i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// blocks of `per` items for n items, between 1 and 2048 (grid-stride kernels)
inline unsigned grid_cap(long n, long per) {
  long g = (n + per - 1) / per;
  if (g > 2048) g = 2048;
  return (unsigned)(g < 1 ? 1 : g);
}

#if defined(__HIPCC__)
// scene_table_fill inside an entry point that returns an error code
#define PQ_SCENE_TABLE(t, offsets, B, max_scene, max_total, who)                                      \
  do {                                                                                                \
    const std::string e_ = scene_table_fill(t, offsets, B, max_scene, max_total, who);                \
    PQ_CHECK_ARG(e_.empty(), e_.c_str());                                                             \
  } while (0)

PQ_DEV float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

template <typename T> PQ_DEV T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// Exclusive prefix sum of one value per thread over the block; `total` = the block's sum, in every thread.
//   * the block has a multiple of 64 threads, at most 1024, and EVERY thread calls (two barriers inside);
//   * lds: SCAN_LDS values of LDS, used by nothing else between the first thread's entry and the last thread's return;
//   * it may be called again on the same lds right away: the barrier in front of the store orders it behind every read of
//     the call before, so the caller adds no barrier between calls.
constexpr int SCAN_LDS = 16;
template <typename T> PQ_DEV T block_excl_scan(T v, T* lds, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const T inc = wave_incl_scan(v);
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  // every wave scans the <= 16 wave sums itself (lane l holds wave l's): one LDS read and shuffles, no third barrier
  T s = lane < nw ? lds[lane] : T(0);
#pragma unroll
  for (int d = 1; d < SCAN_LDS; d <<= 1) {
    const T u = __shfl_up(s, d, 64);
    if (lane >= d) s += u;
  }
  total = __shfl(s, nw - 1, 64);
  return __shfl(s, wave, 64) - __shfl(inc, 63, 64) + inc - v;
}
#endif
