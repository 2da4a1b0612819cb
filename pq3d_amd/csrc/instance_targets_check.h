// Range checks of the instance-target kernels (csrc/instance_targets.hip): plain integer arithmetic shared by the kernels
// and by a stand-alone host program (tests/instance_targets_check_main.cpp), so that it can be run on the CPU under
// sanitizers.  No value of a point2instance / point2segment array is used as an index before one of these has accepted it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PQ_IT_HD __host__ __device__ inline
#else
#define PQ_IT_HD inline
#endif

// slot of an instance id in a scene's table of cap + 1 slots (slot 0: id -1), or -1 for an id outside [-1, cap)
PQ_IT_HD int pq_it_slot(int64_t id, int cap) { return (id < -1 || id >= (int64_t)cap) ? -1 : (int)(id + 1); }

// a segment id is usable iff 0 <= seg < limit
PQ_IT_HD bool pq_it_seg_ok(int64_t seg, int64_t limit) { return seg >= 0 && seg < limit; }

// cell of a row-major [rows, cols] table, or -1 when (r, c) is outside it; the product cannot overflow for rows, cols < 2^31
PQ_IT_HD int64_t pq_it_cell(int64_t r, int64_t c, int64_t rows, int64_t cols) {
  return (r < 0 || r >= rows || c < 0 || c >= cols) ? -1 : r * cols + c;
}
