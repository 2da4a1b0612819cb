// Batched exact linear sum assignment (the Hungarian step of HungarianMatcher, matcher.py:184) on the device: G independent
// problems in one launch, one 64-lane wave per matrix.  Each result is exactly scipy.optimize.linear_sum_assignment on the
// block widened to float64: the shortest-augmenting-path solver of scipy's rectangular_lsap.cpp (Crouse), step for step:
//   - n_cols < n_rows: solve the transpose (rows = the shorter side);
//   - NaN or -inf anywhere in the block: "invalid numeric entries" (PQ3D_LSAP_INVALID);
//   - rows are augmented in order; each Dijkstra starts with remaining[it] = nc - 1 - it, and removing position `index`
//     moves the last element into it (remaining[index] = remaining[--num_remaining]);
//   - reduced cost r = ((minVal + c[i][j]) - u[i]) - v[j] in fp64, in that order (no contraction: built -ffp-contract=off);
//   - duals u[i] += minVal - spc[col4row[i]] (SR rows but curRow), u[curRow] += minVal, v[j] -= minVal - spc[j] (SC);
//   - a least shortest-path cost of +inf: "infeasible" (PQ3D_LSAP_INFEASIBLE).
// The one sequential choice, scipy's scan `spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)` over `remaining`,
// is the minimum of a total order on (spc, unassigned, position): with m the least spc, an unassigned column with spc == m
// at the LARGEST position wins, else the column with spc == m at the SMALLEST position.  Each lane takes positions
// lane, lane + 64, ... of `remaining`, and a butterfly of shuffles (fp64 value, flag, position) gives every lane the same
// winner.  All state lives in LDS (u, v, spc in fp64; path, row4col, col4row, remaining; SC / SR flags), the cost block is
// staged there (in the solved orientation, fp32) when it fits the 64 KB budget and read from global memory otherwise.
// Integer outputs only: bit-identical run to run.  Every loop is bounded (a Dijkstra step removes one column).
#include "common.h"

namespace {

constexpr int LSAP_LDS_BUDGET = 65536;

struct LsapLayout {
  int u, v, spc, cost, path, r4c, rem, c4r, sc, sr, bytes;
};

// NR = min(R, Cmax) rows and NC = max(R, Cmax) columns bound every matrix of the launch in its solved orientation
__host__ __device__ inline LsapLayout lsap_layout(int R, int Cmax, bool stage) {
  const int NR = R < Cmax ? R : Cmax, NC = R < Cmax ? Cmax : R;
  LsapLayout l;
  int o = 0;
  l.u = o; o += 8 * NR;
  l.v = o; o += 8 * NC;
  l.spc = o; o += 8 * NC;
  l.cost = o; o += stage ? 4 * R * Cmax : 0;
  l.path = o; o += 4 * NC;
  l.r4c = o; o += 4 * NC;
  l.rem = o; o += 4 * NC;
  l.c4r = o; o += 4 * NR;
  l.sc = o; o += NC;
  l.sr = o; o += NR;
  l.bytes = (o + 15) & ~15;
  return l;
}

// strict total order of the Dijkstra step's candidates: smaller spc; then unassigned first; then, among unassigned, the
// larger position, among assigned, the smaller position
PQ_DEV bool lsap_before(double a, int ua, int pa, double b, int ub, int pb) {
  if (a != b) return a < b;
  if (ua != ub) return ua > ub;
  return ua ? pa > pb : pa < pb;
}

__global__ __launch_bounds__(64) void lsap_kernel(const float* __restrict__ cost, int R, int Cmax, long ld,
                                                  const int* __restrict__ n_rows, const int* __restrict__ n_cols,
                                                  int* __restrict__ row_idx, int* __restrict__ col_idx,
                                                  int* __restrict__ n_match, int* __restrict__ err, int stage) {
  extern __shared__ __align__(16) unsigned char lsap_smem[];
  const LsapLayout ly = lsap_layout(R, Cmax, stage != 0);
  double* u = (double*)(lsap_smem + ly.u);
  double* v = (double*)(lsap_smem + ly.v);
  double* spc = (double*)(lsap_smem + ly.spc);
  float* sc = (float*)(lsap_smem + ly.cost);
  int* path = (int*)(lsap_smem + ly.path);
  int* r4c = (int*)(lsap_smem + ly.r4c);
  int* rem = (int*)(lsap_smem + ly.rem);
  int* c4r = (int*)(lsap_smem + ly.c4r);
  unsigned char* SC = lsap_smem + ly.sc;
  unsigned char* SR = lsap_smem + ly.sr;

  const int g = blockIdx.x, lane = threadIdx.x;
  const int M = R < Cmax ? R : Cmax;
  int* rowo = row_idx + (long)g * M;
  int* colo = col_idx + (long)g * M;
  const float* base = cost + (long)g * R * ld;
  const int nr0 = n_rows ? n_rows[g] : R, nc0 = n_cols ? n_cols[g] : Cmax;
  int code = 0, nm = 0;
  if (nr0 < 0 || nr0 > R || nc0 < 0 || nc0 > Cmax) code = PQ3D_LSAP_BAD_SIZE;
  if (code == 0 && nr0 > 0 && nc0 > 0) {
    const bool tr = nc0 < nr0;
    const int nr = tr ? nc0 : nr0, nc = tr ? nr0 : nc0;
    // scan (and stage) the block: rows of the original matrix, coalesced along its columns
    int bad = 0;
    for (int r = 0; r < nr0; ++r)
      for (int c = lane; c < nc0; c += 64) {
        const float x = base[(long)r * ld + c];
        bad |= (x != x) | (x == -INFINITY);
        if (stage) sc[tr ? c * nc + r : r * nc + c] = x;
      }
    if (__ballot(bad)) code = PQ3D_LSAP_INVALID;
    auto cst = [&](int i, int j) -> float {
      return stage ? sc[i * nc + j] : (tr ? base[(long)j * ld + i] : base[(long)i * ld + j]);
    };
    for (int j = lane; j < nc; j += 64) { v[j] = 0.0; r4c[j] = -1; }
    for (int i = lane; i < nr; i += 64) { u[i] = 0.0; c4r[i] = -1; }
    __syncthreads();
    for (int cur = 0; cur < nr && code == 0; ++cur) {
      for (int j = lane; j < nc; j += 64) { rem[j] = nc - 1 - j; SC[j] = 0; spc[j] = INFINITY; }
      for (int i = lane; i < nr; i += 64) SR[i] = 0;
      __syncthreads();
      int i = cur, num = nc, sink = -1;
      double minVal = 0.0;
      while (sink < 0) {   // each pass removes one of the `num` remaining columns; num == 0 ends as infeasible below
        if (lane == 0) SR[i] = 1;
        const double ui = u[i];
        double bv = INFINITY;
        int bu = 0, bp = 0x7fffffff;
        for (int it = lane; it < num; it += 64) {
          const int j = rem[it];
          const double r = ((minVal + (double)cst(i, j)) - ui) - v[j];
          double s = spc[j];
          if (r < s) { path[j] = i; spc[j] = r; s = r; }
          const int un = r4c[j] < 0;
          if (lsap_before(s, un, it, bv, bu, bp)) { bv = s; bu = un; bp = it; }
        }
        for (int d = 32; d > 0; d >>= 1) {
          const double ov = __shfl_xor(bv, d);
          const int ou = __shfl_xor(bu, d), op = __shfl_xor(bp, d);
          if (lsap_before(ov, ou, op, bv, bu, bp)) { bv = ov; bu = ou; bp = op; }
        }
        minVal = bv;
        if (bp == 0x7fffffff || minVal == INFINITY) { code = PQ3D_LSAP_INFEASIBLE; break; }
        const int j = rem[bp];
        const int rj = r4c[j];
        if (rj < 0) sink = j; else i = rj;
        __syncthreads();   // every lane has read rem[bp] before it is overwritten
        if (lane == 0) { SC[j] = 1; rem[bp] = rem[num - 1]; }
        --num;
        __syncthreads();
      }
      if (code) break;
      __syncthreads();
      for (int r = lane; r < nr; r += 64)
        if (SR[r] && r != cur) u[r] += minVal - spc[c4r[r]];
      if (lane == 0) u[cur] += minVal;
      for (int j = lane; j < nc; j += 64)
        if (SC[j]) v[j] -= minVal - spc[j];
      __syncthreads();
      if (lane == 0) {   // augment along path (at most one step per SR row)
        int j = sink;
        for (int k = 0; k <= nr; ++k) {
          const int r = path[j];
          r4c[j] = r;
          const int t = c4r[r];
          c4r[r] = j;
          j = t;
          if (r == cur) break;
        }
      }
      __syncthreads();
    }
    if (code == 0) {
      nm = nr;
      if (!tr) {
        for (int r = lane; r < nr; r += 64) { rowo[r] = r; colo[r] = c4r[r]; }
      } else {   // scipy's argsort of col4row: pairs in ascending query (= solved column) order
        int cnt = 0;
        for (int q0 = 0; q0 < nc; q0 += 64) {
          const int q = q0 + lane;
          const int t = q < nc ? r4c[q] : -1;
          const unsigned long long m = __ballot(t >= 0);
          if (t >= 0) {
            const int k = cnt + __popcll(m & ((1ull << lane) - 1ull));
            rowo[k] = q;
            colo[k] = t;
          }
          cnt += __popcll(m);
        }
      }
    }
  }
  for (int k = nm + lane; k < M; k += 64) { rowo[k] = 0; colo[k] = 0; }
  if (lane == 0) { n_match[g] = nm; err[g] = code; }
}

}  // namespace

extern "C" int pq3d_lsap_batched(const float* cost, int32_t G, int32_t R, int32_t Cmax, int64_t ld, const int32_t* n_rows,
                                 const int32_t* n_cols, int32_t* row_idx, int32_t* col_idx, int32_t* n_match, int32_t* err,
                                 void* stream) {
  PQ_DEVICE_GUARD(stream, row_idx);
  PQ_CHECK_ARG(G >= 0 && R >= 1 && Cmax >= 1 && R <= PQ3D_LSAP_MAX_DIM && Cmax <= PQ3D_LSAP_MAX_DIM && ld >= Cmax,
               "pq3d_lsap_batched: need G >= 0, 1 <= R, Cmax <= PQ3D_LSAP_MAX_DIM and ld >= Cmax");
  if (G == 0) return 0;
  PQ_CHECK_ARG(cost && row_idx && col_idx && n_match && err, "pq3d_lsap_batched: null pointer");
  const bool stage = lsap_layout(R, Cmax, true).bytes <= LSAP_LDS_BUDGET;
  const int bytes = lsap_layout(R, Cmax, stage).bytes;
  hipLaunchKernelGGL(lsap_kernel, dim3((unsigned)G), dim3(64), bytes, (hipStream_t)stream, cost, (int)R, (int)Cmax, (long)ld,
                     n_rows, n_cols, row_idx, col_idx, n_match, err, stage ? 1 : 0);
  PQ_LAUNCH_CHECK();
  return 0;
}
