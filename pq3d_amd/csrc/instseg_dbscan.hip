// DBSCAN splitting of instance queries (InstSegEval.dbscan with min_samples = 1, evaluator/instseg_eval.py:245-270) as gfx950
// kernels: per scene and kept query q, the voxels M_q = {v : m(v, q) > 0} split into the connected components of the graph
// "((dx*dx + dy*dy) + dz*dz) <= eps*eps" (fp64 on the fp32 coordinates, no contraction).  With min_samples = 1 every point is
// a core point, so DBSCAN's clusters are exactly these components.
//
// Grid: cells of side c = eps / sqrt(3) * (1 - 1e-6) per scene (origin = the scene's coordinate minimum).  Two voxels of one
// cell are within eps (a clique), and cells 3 or more apart along an axis are more than 2c > eps apart, so a voxel's
// neighbours lie in the +-2 stencil (62 cells in the half stencil).  The voxels are sorted by dense cell key with the
// segment-plan machinery (segment_plan.h), then the work runs on (query, occupied cell) NODES -- O(Q * cells) memory, no
// [V, Q] label array:
//   dbscan_bounds_kernel   per-scene coordinate minimum / maximum (integer atomics on order-preserving codes) and the
//                          non-finite flag (bit 8 of the instseg flag word);
//   dbscan_key_kernel      dense cell key per voxel;
//   dbscan_tile_kernel /   compact ids of the occupied cells in sorted order (per-tile start counts, then per tile its
//   dbscan_cells_kernel    offset + an in-tile scan): cell_first [NC + 1], cell of each voxel, voxel coordinates in sorted
//                          order (float4, w = voxel index);
//   dbscan_node_kernel     per (sorted voxel, 64-query block): the mask bit word (ballot of m > 0 over the kept queries) and
//                          per node the smallest voxel and the mask voxels' bounding box (integer atomics: order-free);
//   dbscan_union_kernel    one wave per node (q, c) over its 62 half-stencil neighbours (q, c'): skipped when c' holds no
//                          mask voxel of q, when the boxes are more than eps apart, or when both nodes already share a
//                          root; otherwise the pair test over the two cells' mask voxels (64 lanes at a time, the first hit
//                          ends it) and a lock-free union (atomicCAS hooks the larger root under the smaller; nothing waits
//                          on another workgroup);
//   dbscan_compress_kernel every node -> its root; the component's head = its smallest voxel (atomicMin);
//   dbscan_heads_kernel    per node its component head; the head bit of each component in a per-query voxel bitmap;
//   dbscan_prefix_kernel   per query the prefix popcounts of that bitmap -> components per (scene, query);
//   dbscan_colofs_kernel   column offsets per (scene, query) and per scene (colseg, read back once by the caller);
//   dbscan_columns_kernel  column j of scene b = (q, head) in (q, head) order: the rank of the head in the bitmap;
//   dbscan_colprob_kernel  the columns' class probabilities [sum_b Q'_b, C] (the ragged top-k's input, csrc/instseg.hip);
//   dbscan_table_kernel    the voxel-level 0/1 table [B * Vmax, K] of the selected columns and per-64-voxel partial sums
//                          of sigmoid(m) [v in column] and [v in column] in fp64 (fixed order; ranked by pq3d_instseg_rank).
// The partition is unique, so the columns do not depend on the order the unions ran in; every sum runs in a fixed order
// (no float atomics): results are bit-identical run to run.
#include "common.h"
#include "ragged.h"
#include "segment_plan.h"

namespace {

using namespace pq3d_plan;

constexpr int TILE = 1024;        // sorted voxels per compaction tile
constexpr int NODE_SPAN = 128;    // sorted voxels per wave of the node kernel
constexpr int VCHUNK = PQ3D_INSTSEG_SEG_CHUNK;   // voxels per partial-sum chunk of the table kernel
constexpr int GRID_WORDS = PQ3D_DBSCAN_GRID_WORDS;
constexpr int NONE = 0x7fffffff;  // minvox of a node without mask voxels

// order-preserving unsigned code of a float (larger float -> larger code)
PQ_DEV unsigned fenc(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PQ_DEV float fdec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// parent words are read and written at device scope (no stale per-CU cache lines while other workgroups hook)
PQ_DEV int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PQ_DEV void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x.  A parent is always a smaller id, so the walk ends.  Path halving stores only into non-roots (which never become
// roots again) and only ancestors, so it races benignly with the hooks.
PQ_DEV int uf_find(int* parent, int x) {
  while (true) {
    const int p = ld(parent + x);
    if (p == x) return x;
    const int g = ld(parent + p);
    if (g == p) return p;
    st(parent + x, g);
    x = g;
  }
}
// lock-free union: hook the larger root under the smaller.  A failed CAS means another thread changed that root's parent
// (progress of the grid as a whole); nothing waits for another workgroup.
PQ_DEV void uf_union(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    if (atomicCAS(parent + b, b, a) == b) return;
  }
}

// the adjacency test, exactly ((dx*dx + dy*dy) + dz*dz) <= eps2 in fp64 with every operation rounded on its own
PQ_DEV bool within(double ax, double ay, double az, double bx, double by, double bz, double eps2) {
  const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)) <= eps2;
}

// ---- bounds: grid (16, B); bounds[b*6 + d] = ~code(min), [b*6 + 3 + d] = code(max) (both maxima, so zero is the identity)
__global__ __launch_bounds__(256) void dbscan_bounds_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ voff,
                                                            unsigned* __restrict__ bounds, unsigned long long* __restrict__ stats) {
  __shared__ unsigned red[6][256];
  const int b = blockIdx.y, tid = threadIdx.x;
  unsigned acc[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  bool bad = false;
  for (long v = voff[b] + (long)blockIdx.x * 256 + tid; v < voff[b + 1]; v += (long)gridDim.x * 256) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float f = xyz[3 * v + d];
      if (!isfinite(f)) { bad = true; continue; }
      const unsigned e = fenc(f);
      acc[d] = max(acc[d], ~e);
      acc[3 + d] = max(acc[3 + d], e);
    }
  }
  if (bad) atomicOr(&stats[0], 8ull);
#pragma unroll
  for (int d = 0; d < 6; ++d) red[d][tid] = acc[d];
  for (int h = 128; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) {
#pragma unroll
      for (int d = 0; d < 6; ++d) red[d][tid] = max(red[d][tid], red[d][tid + h]);
    }
  }
  __syncthreads();
  if (tid < 6 && red[tid][0]) atomicMax(&bounds[b * 6 + tid], red[tid][0]);
}

// grid table of scene b (int64 words): {dense cell offset, nx, ny, nz, fp32 bits of the origin x, y, z, 0}
struct Grid {
  long off;
  int n[3];
  double lo[3];
};
PQ_DEV Grid grid_of(const int64_t* __restrict__ gtab, int b) {
  const int64_t* g = gtab + (long)b * GRID_WORDS;
  Grid r;
  r.off = g[0];
  r.n[0] = (int)g[1]; r.n[1] = (int)g[2]; r.n[2] = (int)g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) r.lo[d] = (double)__uint_as_float((unsigned)g[4 + d]);
  return r;
}

// ---- dense cell key per voxel: off_b + (ix * ny + iy) * nz + iz, i = floor((x - lo) / cell) clamped to the grid
__global__ __launch_bounds__(256) void dbscan_key_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ voff,
                                                         const int64_t* __restrict__ gtab, int B, long NV, double cell,
                                                         int64_t* __restrict__ key) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < NV; v += (long)gridDim.x * blockDim.x) {
    const int b = scene_of(voff, B, v);
    const Grid g = grid_of(gtab, b);
    long k = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double t = floor(__ddiv_rn(__dsub_rn((double)xyz[3 * v + d], g.lo[d]), cell));
      const int i = t < 0.0 ? 0 : (t >= (double)g.n[d] ? g.n[d] - 1 : (int)t);
      k = k * g.n[d] + i;
    }
    key[v] = g.off + k;
  }
}

// ---- compact cell ids.  Sorted position i starts a cell when its key differs from position i - 1's.
PQ_DEV bool cell_start(const int64_t* __restrict__ key, const int* __restrict__ perm, long i) {
  return i == 0 || key[perm[i]] != key[perm[i - 1]];
}
__global__ __launch_bounds__(256) void dbscan_tile_kernel(const int64_t* __restrict__ key, const int* __restrict__ perm, long NV,
                                                          int* __restrict__ tile_cnt) {
  __shared__ int red[4];
  const long t0 = (long)blockIdx.x * TILE, t1 = min(t0 + TILE, NV);
  int n = 0;
  for (long i = t0 + threadIdx.x; i < t1; i += 256) n += cell_start(key, perm, i) ? 1 : 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// one workgroup (1024 threads) per tile: its offset = the earlier tiles' counts, then an in-tile scan.  meta[0] = NC.
__global__ __launch_bounds__(1024) void dbscan_cells_kernel(const int64_t* __restrict__ key, const int* __restrict__ perm,
                                                            const float* __restrict__ xyz, long NV, const int* __restrict__ tile_cnt,
                                                            int* __restrict__ cell_first, int* __restrict__ cell_of_voxel,
                                                            float4* __restrict__ sxyz, int* __restrict__ meta) {
  __shared__ long sm[SCAN_LDS];
  const int t = blockIdx.x, tid = threadIdx.x;
  long pre = 0;
  for (int u = tid; u < t; u += 1024) pre += tile_cnt[u];
  long base;
  (void)block_excl_scan(pre, sm, base);
  const long i = (long)t * TILE + tid;
  const bool in = i < NV;
  const bool s = in && cell_start(key, perm, i);
  long tot;
  const long ex = block_excl_scan(s ? 1L : 0L, sm, tot);
  const long c = base + ex + (s ? 1 : 0) - 1;               // cells started at or before i, minus one
  if (in) {
    const int v = perm[i];
    if (s) cell_first[c] = (int)i;
    cell_of_voxel[v] = (int)c;
    sxyz[i] = make_float4(xyz[3L * v], xyz[3L * v + 1], xyz[3L * v + 2], __int_as_float(v));
  }
  if (t == (int)gridDim.x - 1 && tid == 0) {
    meta[0] = (int)(base + tot);
    cell_first[base + tot] = (int)NV;
  }
}

// ---- node init: parent = self, smallest voxel / component head = NONE
__global__ __launch_bounds__(256) void dbscan_init_kernel(long nnodes, int* __restrict__ parent, int* __restrict__ minvox,
                                                          int* __restrict__ cmin) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nnodes; n += (long)gridDim.x * blockDim.x) {
    parent[n] = (int)n;
    minvox[n] = NONE;
    cmin[n] = NONE;
  }
}

// ---- mask bits + node minima / boxes.  grid (ceil(NV / (4 NODE_SPAN)), W = ceil(Q / 64)); wave w walks NODE_SPAN sorted
// positions, lane = query qb*64 + lane.  bits[i * W + qb] = ballot of m > 0 over the block's kept queries.
__global__ __launch_bounds__(256) void dbscan_node_kernel(const float* __restrict__ masks, const int64_t* __restrict__ v2s,
                                                          const int64_t* __restrict__ voff, const int* __restrict__ qvalid,
                                                          const float4* __restrict__ sxyz, const int* __restrict__ cell_of_voxel,
                                                          int B, long S, int Q, long NV, long ncap, int W,
                                                          unsigned long long* __restrict__ bits, int* __restrict__ minvox,
                                                          unsigned* __restrict__ nbox) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qb = blockIdx.y, q = qb * 64 + lane;
  const long i0 = ((long)blockIdx.x * 4 + w) * NODE_SPAN, i1 = min(i0 + NODE_SPAN, NV);
  int cur = -1, mv = NONE;
  unsigned acc[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  auto flush = [&]() {
    if (cur >= 0 && mv != NONE) {
      const long n = (long)q * ncap + cur;
      atomicMin(&minvox[n], mv);
#pragma unroll
      for (int d = 0; d < 6; ++d) atomicMax(&nbox[n * 6 + d], acc[d]);
    }
    mv = NONE;
#pragma unroll
    for (int d = 0; d < 6; ++d) acc[d] = 0u;
  };
  for (long i = i0; i < i1; ++i) {
    const float4 p = sxyz[i];
    const int v = __float_as_int(p.w);
    const int c = cell_of_voxel[v];
    if (c != cur) { flush(); cur = c; }
    const int b = scene_of(voff, B, v);
    bool on = false;
    if (q < Q && (!qvalid || qvalid[(long)b * Q + q])) on = masks[((long)b * S + v2s[v]) * Q + q] > 0.f;
    const unsigned long long word = __ballot(on);
    if (lane == 0) bits[i * W + qb] = word;
    if (on) {
      if (v < mv) mv = v;
      const float xs[3] = {p.x, p.y, p.z};
#pragma unroll
      for (int d = 0; d < 3; ++d) { const unsigned e = fenc(xs[d]); acc[d] = max(acc[d], ~e); acc[3 + d] = max(acc[3 + d], e); }
    }
  }
  flush();
}

// ---- unions.  grid (ncap, ceil(Q / 4)); wave w: node (q = blockIdx.y*4 + w, c = blockIdx.x)
__global__ __launch_bounds__(256) void dbscan_union_kernel(const int* __restrict__ meta, const int* __restrict__ cell_first,
                                                           const int* __restrict__ seg_off, const int* __restrict__ perm,
                                                           const int64_t* __restrict__ key, const int* __restrict__ cell_of_voxel,
                                                           const int64_t* __restrict__ voff, const int64_t* __restrict__ gtab,
                                                           const float4* __restrict__ sxyz,
                                                           const unsigned long long* __restrict__ bits,
                                                           const int* __restrict__ minvox, const unsigned* __restrict__ nbox,
                                                           int B, int Q, long ncap, int W, double eps2, int* parent) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int c = blockIdx.x;
  if (q >= Q || c >= meta[0]) return;
  const long n = (long)q * ncap + c;
  if (minvox[n] == NONE) return;
  const int f1 = cell_first[c], e1 = cell_first[c + 1];
  const int v0 = __float_as_int(sxyz[f1].w);
  const int b = scene_of(voff, B, v0);
  const Grid g = grid_of(gtab, b);
  long loc = key[v0] - g.off;
  const int iz = (int)(loc % g.n[2]);
  loc /= g.n[2];
  const int iy = (int)(loc % g.n[1]);
  const int ix = (int)(loc / g.n[1]);
  double lo1[3], hi1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) { lo1[d] = (double)fdec(~nbox[n * 6 + d]); hi1[d] = (double)fdec(nbox[n * 6 + 3 + d]); }
  const int qw = q >> 6;
  const unsigned long long qbit = 1ull << (q & 63);
  for (int o = 0; o < 125; ++o) {
    const int dx = o / 25 - 2, dy = (o / 5) % 5 - 2, dz = o % 5 - 2;
    if (!(dx > 0 || (dx == 0 && (dy > 0 || (dy == 0 && dz > 0))))) continue;    // the half stencil: 62 cells
    const int jx = ix + dx, jy = iy + dy, jz = iz + dz;
    if (jx < 0 || jy < 0 || jz < 0 || jx >= g.n[0] || jy >= g.n[1] || jz >= g.n[2]) continue;
    const long dk = g.off + ((long)jx * g.n[1] + jy) * g.n[2] + jz;
    const int s0 = seg_off[dk];
    if (seg_off[dk + 1] == s0) continue;
    const int c2 = cell_of_voxel[perm[s0]];
    const long n2 = (long)q * ncap + c2;
    if (minvox[n2] == NONE) continue;
    // box gap per axis: a lower bound of every pair's |d| there, so its rounded sum of squares bounds the pair test below
    double gap[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double lo2 = (double)fdec(~nbox[n2 * 6 + d]), hi2 = (double)fdec(nbox[n2 * 6 + 3 + d]);
      const double a = __dsub_rn(lo2, hi1[d]), bb = __dsub_rn(lo1[d], hi2);
      gap[d] = fmax(fmax(a, bb), 0.0);          // (a nested select here crashed the gfx950 backend)
    }
    if (!within(gap[0], gap[1], gap[2], 0.0, 0.0, 0.0, eps2)) continue;
    if (uf_find(parent, (int)n) == uf_find(parent, (int)n2)) continue;
    const int e2 = cell_first[c2 + 1];
    bool hit = false;
    for (int jb = s0; jb < e2 && !hit; jb += 64) {
      const int j = jb + lane;
      const bool lj = j < e2 && (bits[(long)j * W + qw] & qbit);
      if (__ballot(lj) == 0ull) continue;
      float4 pj = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lj) pj = sxyz[j];
      for (int i = f1; i < e1; ++i) {
        if (!(bits[(long)i * W + qw] & qbit)) continue;
        const float4 pi = sxyz[i];
        const bool h = lj && within((double)pi.x, (double)pi.y, (double)pi.z, (double)pj.x, (double)pj.y, (double)pj.z, eps2);
        if (__ballot(h)) { hit = true; break; }
      }
    }
    if (hit && lane == 0) uf_union(parent, (int)n, (int)n2);
  }
}

// ---- every node with mask voxels -> its root; component head = the smallest voxel of its nodes
__global__ __launch_bounds__(256) void dbscan_compress_kernel(const int* __restrict__ meta, long ncap, long nnodes,
                                                              const int* __restrict__ minvox, int* parent, int* __restrict__ cmin) {
  const long nc = meta[0];
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nnodes; n += (long)gridDim.x * blockDim.x) {
    if (n % ncap >= nc || minvox[n] == NONE) continue;
    const int r = uf_find(parent, (int)n);
    atomicMin(&cmin[r], minvox[n]);
    st(parent + n, r);
  }
}

// ---- head per node; head bits hb[q * WV + v / 64] of the roots (v = head voxel)
__global__ __launch_bounds__(256) void dbscan_heads_kernel(const int* __restrict__ meta, long ncap, long nnodes, long WV,
                                                           const int* __restrict__ minvox, const int* __restrict__ parent,
                                                           const int* __restrict__ cmin, int* __restrict__ head,
                                                           unsigned long long* __restrict__ hb) {
  const long nc = meta[0];
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nnodes; n += (long)gridDim.x * blockDim.x) {
    if (n % ncap >= nc || minvox[n] == NONE) continue;
    const int r = parent[n];
    const int h = cmin[r];
    head[n] = h;
    if (r == n) atomicOr(&hb[(n / ncap) * WV + (h >> 6)], 1ull << (h & 63));
  }
}

// heads of query q at voxels below v
PQ_DEV long hrank(const unsigned long long* __restrict__ hb, const int* __restrict__ pre, long WV, int q, long v) {
  const long w = v >> 6;
  const unsigned long long m = (v & 63) ? (hb[(long)q * WV + w] & ((1ull << (v & 63)) - 1ull)) : 0ull;
  return (long)pre[(long)q * WV + w] + __popcll(m);
}

// ---- one workgroup (1024) per query: pre[q * WV + w] = heads in words [0, w); cnt[b * Q + q] = heads in scene b
__global__ __launch_bounds__(1024) void dbscan_prefix_kernel(const unsigned long long* __restrict__ hb, long WV,
                                                             const int64_t* __restrict__ voff, int B, int Q,
                                                             int* __restrict__ pre, int* __restrict__ cnt) {
  __shared__ long sm[SCAN_LDS];
  const int q = blockIdx.x, tid = threadIdx.x;
  long carry = 0;
  for (long w0 = 0; w0 < WV; w0 += 1024) {
    const long w = w0 + tid;
    const long c = w < WV ? __popcll(hb[(long)q * WV + w]) : 0;
    long tot;
    const long ex = block_excl_scan(c, sm, tot);
    if (w < WV) pre[(long)q * WV + w] = (int)(carry + ex);
    carry += tot;
  }
  __syncthreads();
  for (int b = tid; b < B; b += 1024)
    cnt[(long)b * Q + q] = (int)(hrank(hb, pre, WV, q, voff[b + 1]) - hrank(hb, pre, WV, q, voff[b]));
}

// ---- one workgroup: colq[b * Q + q] = first column of (b, q); colseg[b] = first column of scene b (colseg[B] = total)
__global__ __launch_bounds__(1024) void dbscan_colofs_kernel(const int* __restrict__ cnt, int B, int Q, int* __restrict__ colq,
                                                             int64_t* __restrict__ colseg) {
  __shared__ long sm[SCAN_LDS];
  long base = 0;
  for (int b = 0; b < B; ++b) {
    if (threadIdx.x == 0) colseg[b] = base;
    for (int q0 = 0; q0 < Q; q0 += 1024) {
      const int q = q0 + threadIdx.x;
      long tot;
      const long ex = block_excl_scan(q < Q ? (long)cnt[(long)b * Q + q] : 0L, sm, tot);
      if (q < Q) colq[(long)b * Q + q] = (int)(base + ex);
      base += tot;
    }
  }
  if (threadIdx.x == 0) colseg[B] = base;
}

// ---- columns in (q, head) order per scene: col[j] = {q, head voxel, scene, 0}
__global__ __launch_bounds__(256) void dbscan_columns_kernel(const int* __restrict__ meta, long ncap, long nnodes, long WV,
                                                             const int* __restrict__ minvox, const int* __restrict__ parent,
                                                             const int* __restrict__ head, const unsigned long long* __restrict__ hb,
                                                             const int* __restrict__ pre, const int* __restrict__ colq,
                                                             const int64_t* __restrict__ voff, int B, int Q, long ncol,
                                                             int4* __restrict__ col) {
  const long nc = meta[0];
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nnodes; n += (long)gridDim.x * blockDim.x) {
    if (n % ncap >= nc || minvox[n] == NONE || parent[n] != n) continue;
    const int q = (int)(n / ncap);
    const int h = head[n];
    const int b = scene_of(voff, B, h);
    const long j = colq[(long)b * Q + q] + hrank(hb, pre, WV, q, h) - hrank(hb, pre, WV, q, voff[b]);
    if (j >= 0 && j < ncol) col[j] = make_int4(q, h, b, 0);
  }
}

// ---- colprob[j * C + c] = prob[b_j, q_j * C + c]
__global__ __launch_bounds__(256) void dbscan_colprob_kernel(const float* __restrict__ prob, const int4* __restrict__ col, int Q,
                                                             int C, long ncol, float* __restrict__ colprob) {
  const long n = ncol * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long j = i / C;
    const int c = (int)(i - j * C);
    const int4 cj = col[j];
    colprob[i] = prob[((long)cj.z * Q + cj.x) * C + c];
  }
}

// ---- voxel table + score partials.  grid (ceil(Vmax / VCHUNK), ceil(K / 64), B); lane = selection k, waves stride over the
// chunk's voxels.  Selection k < kout[b] is column colseg[b] + sel[b, k]; padding selections give zeros.
__global__ __launch_bounds__(256) void dbscan_table_kernel(const float* __restrict__ masks, const int64_t* __restrict__ v2s,
                                                           const int64_t* __restrict__ voff, const int* __restrict__ cell_of_voxel,
                                                           const int* __restrict__ head, const int4* __restrict__ col,
                                                           const int64_t* __restrict__ colseg, const int* __restrict__ sel,
                                                           const int* __restrict__ kout, long S, int Q, int K, long Vmax, long ncap,
                                                           float* __restrict__ table, double2* __restrict__ part) {
  __shared__ double2 red[4][64];
  const int chunk = blockIdx.x, b = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.y * 64 + lane;
  const bool kv = k < K;
  const bool real = kv && k < kout[b];
  int q = 0, h = -1;
  if (real) {
    const int4 cj = col[colseg[b] + sel[(long)b * K + k]];
    q = cj.x;
    h = cj.y;
  }
  const long vb = voff[b], nvb = voff[b + 1] - vb;
  const long v0 = (long)chunk * VCHUNK, v1 = min(nvb, v0 + VCHUNK);
  double ss = 0.0, cc = 0.0;
  if (kv) {
    for (long v = v0 + w; v < v1; v += 4) {
      const long gv = vb + v;
      bool on = false;
      float m = 0.f;
      if (real) {
        m = masks[((long)b * S + v2s[gv]) * Q + q];
        on = m > 0.f && head[(long)q * ncap + cell_of_voxel[gv]] == h;
      }
      table[((long)b * Vmax + v) * K + k] = on ? 1.f : 0.f;
      if (on) { ss += (double)sigmoidf_(m); cc += 1.0; }
    }
  }
  red[w][lane] = make_double2(ss, cc);
  __syncthreads();
  if (w == 0 && kv) {
    double a = 0.0, c = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { a += red[i][lane].x; c += red[i][lane].y; }
    part[((long)b * gridDim.x + chunk) * K + k] = make_double2(a, c);
  }
}


// workspace sections, 256-byte aligned, in this order (pq3d_dbscan_ws_bytes)
struct DbWs {
  int *tile_cnt, *meta, *cell_first, *cell_of_voxel;
  float4* sxyz;
  unsigned long long* bits;
  int *parent, *minvox, *cmin, *head;
  unsigned* nbox;
  unsigned long long* hb;
  int *pre, *cnt, *colq;
  long bytes;
};
DbWs dbscan_ws(void* ws, long NV, long Q, long ncap, long B) {
  const long W = (Q + 63) / 64, WV = NV / 64 + 1, nn = Q * ncap, tiles = (NV + TILE - 1) / TILE;
  char* p = (char*)ws;
  long o = 0;
  auto a = [&](long bytes) { char* r = p ? p + o : nullptr; o += (bytes + 255) & ~255L; return (void*)r; };
  DbWs w;
  w.tile_cnt = (int*)a(tiles * 4); w.meta = (int*)a(16); w.cell_first = (int*)a((ncap + 2) * 4);
  w.cell_of_voxel = (int*)a(NV * 4); w.sxyz = (float4*)a(NV * 16); w.bits = (unsigned long long*)a(NV * W * 8);
  w.parent = (int*)a(nn * 4); w.minvox = (int*)a(nn * 4); w.cmin = (int*)a(nn * 4); w.head = (int*)a(nn * 4);
  w.nbox = (unsigned*)a(nn * 24); w.hb = (unsigned long long*)a(Q * WV * 8); w.pre = (int*)a(Q * WV * 4);
  w.cnt = (int*)a(B * Q * 4); w.colq = (int*)a(B * Q * 4);
  w.bytes = o;
  return w;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" int pq3d_dbscan_bounds(const float* xyz, const int64_t* voff, int32_t B, int64_t NV, uint32_t* bounds, int64_t* stats,
                                  void* stream) {
  PQ_DEVICE_GUARD(stream, bounds);
  PQ_CHECK_ARG(voff && bounds && stats && B >= 1 && B < 65536 && NV >= 0 && (xyz || NV == 0), "pq3d_dbscan_bounds: bad args");
  hipStream_t s = (hipStream_t)stream;
  ZeroList z;
  z.add(bounds, (long)B * 6);
  const int e = pq3d_zero_launch(z, s);
  if (e) return e;
  if (NV > 0)
    hipLaunchKernelGGL(dbscan_bounds_kernel, dim3(16u, (unsigned)B), dim3(256), 0, s, xyz, voff, (unsigned*)bounds,
                       (unsigned long long*)stats);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_dbscan_keys(const float* xyz, const int64_t* voff, const int64_t* gtab, int32_t B, int64_t NV, double cell,
                                int64_t* key, void* stream) {
  PQ_DEVICE_GUARD(stream, key);
  PQ_CHECK_ARG(xyz && voff && gtab && key && B >= 1 && NV >= 1 && cell > 0.0, "pq3d_dbscan_keys: bad args");
  hipLaunchKernelGGL(dbscan_key_kernel, dim3(grid_cap(NV, 256)), dim3(256), 0, (hipStream_t)stream, xyz, voff, gtab, (int)B,
                     (long)NV, cell, key);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t pq3d_dbscan_ws_bytes(int64_t NV, int32_t Q, int64_t ncap, int32_t B) {
  return dbscan_ws(nullptr, NV, Q, ncap, B).bytes;
}

extern "C" int pq3d_dbscan_components(const float* masks, const int64_t* v2s, const int64_t* voff, const int32_t* qvalid,
                                      const float* xyz, const int64_t* key, const int64_t* gtab, const void* plan,
                                      int64_t ndense, int32_t B, int64_t S, int32_t Q, int64_t NV, int64_t ncap, double eps,
                                      void* ws, int64_t ws_bytes, int64_t* colseg, void* stream) {
  PQ_DEVICE_GUARD(stream, ws);
  PQ_CHECK_ARG(masks && v2s && voff && xyz && key && gtab && plan && ws && colseg && B >= 1 && B < 65536 && S >= 1 && Q >= 1 &&
               NV >= 1 && ncap >= 1 && ncap <= NV && ndense >= ncap && eps > 0.0, "pq3d_dbscan_components: bad args");
  PQ_CHECK_ARG((int64_t)Q * ncap < (1LL << 31) - 1 && NV < (1LL << 31) - 65536 && (int64_t)Q * (NV / 64 + 1) < (1LL << 31) &&
               ndense < (1LL << 31) - 65536, "pq3d_dbscan_components: Q * cells, Q * NV / 64 and NV must fit 31 bits");
  const DbWs w = dbscan_ws(ws, NV, Q, ncap, B);
  PQ_CHECK_ARG(ws_bytes >= w.bytes && (((uintptr_t)ws) & 255) == 0,
               "pq3d_dbscan_components: workspace smaller than pq3d_dbscan_ws_bytes or not 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long W = (Q + 63) / 64, WV = NV / 64 + 1, nn = (long)Q * ncap, tiles = (NV + TILE - 1) / TILE;
  const PlanLayout L = plan_layout(NV, ndense);
  const int* P = (const int*)plan;
  ZeroList z;
  z.add(w.nbox, nn * 6);
  z.add(w.hb, (long)Q * WV * 2);
  const int e = pq3d_zero_launch(z, s);
  if (e) return e;
  hipLaunchKernelGGL(dbscan_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, s, key, P + L.perm, (long)NV, w.tile_cnt);
  hipLaunchKernelGGL(dbscan_cells_kernel, dim3((unsigned)tiles), dim3(1024), 0, s, key, P + L.perm, xyz, (long)NV,
                     (const int*)w.tile_cnt, w.cell_first, w.cell_of_voxel, w.sxyz, w.meta);
  hipLaunchKernelGGL(dbscan_init_kernel, dim3(grid_cap(nn, 256)), dim3(256), 0, s, nn, w.parent, w.minvox, w.cmin);
  hipLaunchKernelGGL(dbscan_node_kernel, dim3((unsigned)((NV + 4 * NODE_SPAN - 1) / (4 * NODE_SPAN)), (unsigned)W), dim3(256), 0, s,
                     masks, v2s, voff, (const int*)qvalid, (const float4*)w.sxyz, (const int*)w.cell_of_voxel, (int)B, (long)S,
                     (int)Q, (long)NV, (long)ncap, (int)W, w.bits, w.minvox, w.nbox);
  hipLaunchKernelGGL(dbscan_union_kernel, dim3((unsigned)ncap, (unsigned)((Q + 3) / 4)), dim3(256), 0, s, (const int*)w.meta,
                     (const int*)w.cell_first, P + L.seg_off, P + L.perm, key, (const int*)w.cell_of_voxel, voff, gtab,
                     (const float4*)w.sxyz, (const unsigned long long*)w.bits, (const int*)w.minvox, (const unsigned*)w.nbox,
                     (int)B, (int)Q, (long)ncap, (int)W, eps * eps, w.parent);
  hipLaunchKernelGGL(dbscan_compress_kernel, dim3(grid_cap(nn, 256)), dim3(256), 0, s, (const int*)w.meta, (long)ncap, nn,
                     (const int*)w.minvox, w.parent, w.cmin);
  hipLaunchKernelGGL(dbscan_heads_kernel, dim3(grid_cap(nn, 256)), dim3(256), 0, s, (const int*)w.meta, (long)ncap, nn, WV,
                     (const int*)w.minvox, (const int*)w.parent, (const int*)w.cmin, w.head, w.hb);
  hipLaunchKernelGGL(dbscan_prefix_kernel, dim3((unsigned)Q), dim3(1024), 0, s, (const unsigned long long*)w.hb, WV, voff, (int)B,
                     (int)Q, w.pre, w.cnt);
  hipLaunchKernelGGL(dbscan_colofs_kernel, dim3(1u), dim3(1024), 0, s, (const int*)w.cnt, (int)B, (int)Q, w.colq, colseg);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_dbscan_columns(const float* prob, const int64_t* voff, int32_t B, int32_t Q, int32_t C, int64_t NV,
                                   int64_t ncap, int64_t ncol, const void* ws, int32_t* col, float* colprob, void* stream) {
  PQ_DEVICE_GUARD(stream, col);
  PQ_CHECK_ARG(prob && voff && ws && col && colprob && B >= 1 && Q >= 1 && C >= 1 && NV >= 1 && ncap >= 1 && ncol >= 1 &&
               ncol * (int64_t)C < (1LL << 40), "pq3d_dbscan_columns: bad args");
  hipStream_t s = (hipStream_t)stream;
  const DbWs w = dbscan_ws((void*)ws, NV, Q, ncap, B);
  const long WV = NV / 64 + 1, nn = (long)Q * ncap;
  hipLaunchKernelGGL(dbscan_columns_kernel, dim3(grid_cap(nn, 256)), dim3(256), 0, s, (const int*)w.meta, (long)ncap, nn, WV,
                     (const int*)w.minvox, (const int*)w.parent, (const int*)w.head, (const unsigned long long*)w.hb,
                     (const int*)w.pre, (const int*)w.colq, voff, (int)B, (int)Q, (long)ncol, (int4*)col);
  hipLaunchKernelGGL(dbscan_colprob_kernel, dim3(grid_cap(ncol * C, 256)), dim3(256), 0, s, prob, (const int4*)col, (int)Q, (int)C,
                     (long)ncol, colprob);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_dbscan_table(const float* masks, const int64_t* v2s, const int64_t* voff, const void* ws, const int32_t* col,
                                 const int64_t* colseg, const int32_t* sel, const int32_t* kout, int32_t B, int64_t S, int32_t Q,
                                 int32_t K, int64_t NV, int64_t ncap, int64_t Vmax, float* table, void* part, int64_t part_bytes,
                                 void* stream) {
  PQ_DEVICE_GUARD(stream, table);
  PQ_CHECK_ARG(masks && v2s && voff && ws && col && colseg && sel && kout && table && part && B >= 1 && B < 65536 && S >= 1 &&
               Q >= 1 && K >= 1 && K <= PQ3D_INSTSEG_MAX_K && NV >= 1 && ncap >= 1 && Vmax >= 1, "pq3d_dbscan_table: bad args");
  const long nch = (Vmax + VCHUNK - 1) / VCHUNK;
  PQ_CHECK_ARG(nch < 65536L * 256 && part_bytes >= (int64_t)B * nch * K * 16 && (((uintptr_t)part) & 15) == 0,
               "pq3d_dbscan_table: partials smaller than B * ceil(Vmax / PQ3D_INSTSEG_SEG_CHUNK) * K * 16 bytes or misaligned");
  const DbWs w = dbscan_ws((void*)ws, NV, Q, ncap, B);
  hipLaunchKernelGGL(dbscan_table_kernel, dim3((unsigned)nch, (unsigned)((K + 63) / 64), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, masks, v2s, voff, (const int*)w.cell_of_voxel, (const int*)w.head, (const int4*)col,
                     colseg, (const int*)sel, (const int*)kout, (long)S, (int)Q, (int)K, (long)Vmax, (long)ncap, table,
                     (double2*)part);
  PQ_LAUNCH_CHECK();
  return 0;
}
