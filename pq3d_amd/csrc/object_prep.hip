// Grounding (stage-2) batches prepared on the device (the specification is tests/object_prep_ref.py): what the
// reference builds per sample on the host in data/datasets/sceneverse_base.py (_load_one_scan, get_scene,
// _obj_processing_post, match_gt_to_pred) and pads in its dataset wrapper.
//   bank     ob_count_kernel    one workgroup per (object row, chunk of OB_CHUNK points): how many points the row selects
//            ob_rowscan_kernel  one workgroup per row: exclusive scan of its chunk counts (block_excl_scan), the row's total
//            ob_emit_kernel     per (row, chunk) again: the selected points in ascending order into the row's CSR range
//            ob_box_kernel      one workgroup per kept object: fp32 min / max of its points, centre and size
//            Integer arithmetic only (no atomics): two runs give the same bits.
//   match    ob_match_kernel    one thread per GT box: box3d_iou in fp64 against every predicted box
//   sample   ob_sample_kernel   one workgroup per (item, slot), the hot path: draws num_points of the object's points by a
//            counter-based rule, gathers them and applies _obj_processing_post in fp64 with a fixed reduction tree
//   labels   ob_labels_kernel, ob_range_kernel, ob_rows_kernel: the 0-1 label rows, coord_min / coord_max, the gather of
//            offline per-object feature rows
// Every index that comes from the caller's data (scene_of_item, selected, targets) is range-checked before it indexes
// anything; a bad one sets a bit of the error word and the slot is written as padding.  Every loop bound is a kernel
// argument, a table entry the host wrote, or a constant.
#include "common.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int OB_CHUNK = PQ3D_OBJECT_CHUNK, OB_PER = OB_CHUNK / 256;        // points of a cell, consecutive points per thread
static_assert(PQ3D_OBJECT_MAX_SAMPLE == 8 * 512, "ob_sample_kernel: at most 8 pairs per thread");
constexpr int OB_ROUNDS = 4, OB_WALK_CAP = PQ3D_OBJECT_WALK_CAP;
static_assert(OB_PER == 4 && (PQ3D_OBJECT_MAX_POINTS + OB_CHUNK - 1) / OB_CHUNK <= 256 * 4, "ob_rowscan_kernel: four chunks per thread");

// the object rows of a set of scans (all device arrays, written by the host side of build_object_bank)
struct ObRows {
  const int64_t* pt_off;     // [S + 1] first point of every scan
  const int64_t* row_off;    // [S + 1] first row of every scan
  const int64_t* cell_off;   // [R + 1] first (row, chunk) cell of every row
  const int64_t* p2i;        // ids form: [P] instance id of every point
  const int64_t* ids;        // ids form: [R] the id row r selects
  const uint8_t* masks;      // masks form: the scans' [K_s, P_s] byte matrices, concatenated
  const int64_t* mask_off;   // masks form: [S + 1] first byte of every scan's matrix
  int S;
  long R, cells;
};

// The 4 selection bits of this thread's consecutive points in cell c; r = the row, p0 = the thread's first scan-local point.
PQ_DEV unsigned ob_flags(const ObRows& a, long c, long& r, long& p0) {
  r = scene_of(a.cell_off, (int)a.R, c);
  const int s = scene_of(a.row_off, a.S, r);
  const long P = a.pt_off[s + 1] - a.pt_off[s];
  p0 = (c - a.cell_off[r]) * OB_CHUNK + (long)threadIdx.x * OB_PER;
  unsigned f = 0;
  if (a.masks) {
    const uint8_t* m = a.masks + a.mask_off[s] + (r - a.row_off[s]) * P;
#pragma unroll
    for (int q = 0; q < OB_PER; ++q)
      if (p0 + q < P && m[p0 + q]) f |= 1u << q;
  } else {
    const int64_t id = a.ids[r];
    const int64_t* g = a.p2i + a.pt_off[s];
#pragma unroll
    for (int q = 0; q < OB_PER; ++q)
      if (p0 + q < P && g[p0 + q] == id) f |= 1u << q;
  }
  return f;
}

__global__ __launch_bounds__(256) void ob_count_kernel(ObRows a, int* __restrict__ cnt) {
  __shared__ int lds[SCAN_LDS];
  for (long c = blockIdx.x; c < a.cells; c += gridDim.x) {
    long r, p0;
    int total;
    block_excl_scan((int)__popc(ob_flags(a, c, r, p0)), lds, total);
    if (threadIdx.x == 0) cnt[c] = total;
  }
}

__global__ __launch_bounds__(256) void ob_rowscan_kernel(ObRows a, const int* __restrict__ cnt, int* __restrict__ cbase,
                                                         int* __restrict__ row_total) {
  __shared__ int lds[SCAN_LDS];
  for (long r = blockIdx.x; r < a.R; r += gridDim.x) {
    const long c0 = a.cell_off[r], nch = a.cell_off[r + 1] - c0;          // nch <= 1024 (host-checked scan size)
    int v[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long i = (long)threadIdx.x * 4 + q;
      v[q] = i < nch ? cnt[c0 + i] : 0;
      sum += v[q];
    }
    int total;
    int e = block_excl_scan(sum, lds, total);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long i = (long)threadIdx.x * 4 + q;
      if (i < nch) cbase[c0 + i] = e;
      e += v[q];
    }
    if (threadIdx.x == 0) row_total[r] = total;
  }
}

__global__ __launch_bounds__(256) void ob_emit_kernel(ObRows a, const int* __restrict__ cbase, const int64_t* __restrict__ row_entry,
                                                      long E, int* __restrict__ order) {
  __shared__ int lds[SCAN_LDS];
  for (long c = blockIdx.x; c < a.cells; c += gridDim.x) {
    long r, p0;
    const unsigned f = ob_flags(a, c, r, p0);
    int total;
    const int e = block_excl_scan((int)__popc(f), lds, total);
    long dst = row_entry[r] + cbase[c] + e;
#pragma unroll
    for (int q = 0; q < OB_PER; ++q)
      if ((f >> q) & 1u) {
        if (dst >= 0 && dst < E) order[dst] = (int)(p0 + q);
        ++dst;
      }
  }
}

// the concatenated scans and their objects' CSR (device arrays of an ObjectBank)
struct ObBank {
  const float* points;        // [P, 6]
  const int64_t* pt_off;      // [S + 1]
  const int32_t* obj_off;     // [S + 1] first object of every scan
  const int64_t* entry_off;   // [O + 1] first entry of every object
  const int32_t* order;       // [E] scan-local point indices, ascending within each object
  int S;
};

__global__ __launch_bounds__(256) void ob_box_kernel(ObBank bk, const int32_t* __restrict__ obj_scan, int O, float* __restrict__ center,
                                                     float* __restrict__ size) {
  __shared__ float red[4][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = blockIdx.x; o < O; o += gridDim.x) {
    const int s = obj_scan[o];
    const long e0 = bk.entry_off[o], e1 = bk.entry_off[o + 1];
    const float* pts = bk.points + bk.pt_off[s] * 6;
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (long e = e0 + threadIdx.x; e < e1; e += 256) {
      const float* p = pts + (long)bk.order[e] * 6;
#pragma unroll
      for (int k = 0; k < 3; ++k) { v[k] = fminf(v[k], p[k]); v[3 + k] = fmaxf(v[3 + k], p[k]); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = fminf(v[k], __shfl_xor(v[k], off, 64));
        v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], off, 64));
      }
    __syncthreads();                                     // (the reads of the object before)
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 6; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 3) {
      const int k = threadIdx.x;
      const float mn = fminf(fminf(red[0][k], red[1][k]), fminf(red[2][k], red[3][k]));
      const float mx = fmaxf(fmaxf(red[0][3 + k], red[1][3 + k]), fmaxf(red[2][3 + k], red[3][3 + k]));
      center[(long)o * 3 + k] = (mn + mx) / 2.f;
      size[(long)o * 3 + k] = mx - mn;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- match
PQ_DEV double ob_iou(const float* gc, const float* gs, const float* pc, const float* ps) {
  double d[3], v1 = 1.0, v2 = 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double g0 = (-(double)gs[k]) / 2.0 + (double)gc[k], g1 = (double)gs[k] / 2.0 + (double)gc[k];
    double p0 = (-(double)ps[k]) / 2.0 + (double)pc[k], p1 = (double)ps[k] / 2.0 + (double)pc[k];
    if (g1 < g0) { const double t = g0; g0 = g1; g1 = t; }
    if (p1 < p0) { const double t = p0; p0 = p1; p1 = t; }
    const double hi = p1 < g1 ? p1 : g1, lo = p0 > g0 ? p0 : g0, t = hi - lo;
    d[k] = t > 0.0 ? t : 0.0;
    v1 = k == 0 ? g1 - g0 : v1 * (g1 - g0);
    v2 = k == 0 ? p1 - p0 : v2 * (p1 - p0);
  }
  const double inter = d[0] * d[1] * d[2];
  return inter / (v1 + v2 - inter + 1e-8);
}

__global__ __launch_bounds__(256) void ob_match_kernel(const float* __restrict__ gc, const float* __restrict__ gs,
                                                       const float* __restrict__ pc, const float* __restrict__ ps, int G, int K,
                                                       int* __restrict__ matched, uint8_t* __restrict__ iou25,
                                                       uint8_t* __restrict__ iou50) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  double best = -1.0;
  int m = -1;
  for (int k = 0; k < K; ++k) {
    const double iou = ob_iou(gc + (long)g * 3, gs + (long)g * 3, pc + (long)k * 3, ps + (long)k * 3);
    if (iou > best) { best = iou; m = k; }
    iou25[(long)g * K + k] = iou >= 0.25 ? 1 : 0;
    iou50[(long)g * K + k] = iou >= 0.5 ? 1 : 0;
  }
  matched[g] = m;
}

// --------------------------------------------------------------------------------------------------------------- sample
struct ObKey {
  uint32_t k0, k1, rk[OB_ROUNDS];
};
PQ_DEV ObKey ob_key(uint64_t seed, uint32_t item, uint32_t slot) {
  ObKey k;
  k.k0 = drop_fin((uint32_t)seed ^ (item * 0x9E3779B1u));
  k.k1 = drop_fin(k.k0 + (uint32_t)(seed >> 32) + slot * 0x85EBCA6Bu + 0x27D4EB2Fu);
#pragma unroll
  for (int r = 0; r < OB_ROUNDS; ++r) k.rk[r] = drop_fin(k.k1 + (uint32_t)r * 0x9E3779B1u) ^ k.k0;
  return k;
}
PQ_DEV uint32_t ob_hash_j(const ObKey& k, uint32_t j) {
  uint32_t h = j ^ k.k0;
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h += k.k1; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}
PQ_DEV uint32_t ob_feistel(const ObKey& k, uint32_t x, int half) {
  const uint32_t mask = (1u << half) - 1u;
  uint32_t L = x >> half, R = x & mask;
#pragma unroll
  for (int r = 0; r < OB_ROUNDS; ++r) {
    const uint32_t t = L ^ (drop_fin(R ^ k.rk[r]) & mask);
    L = R;
    R = t;
  }
  return (L << half) | R;
}
// perm(j) of [0, n) (n >= 2): cycle-walking over the domain 4^half >= n, which is below 4 n.  A pass of a random permutation
// leaves [0, n) with probability < 3/4, so a walk longer than OB_WALK_CAP = 256 passes has probability < (3/4)^256 < 1e-31
// per draw (< 1e-24 for the 1e7 draws of a shipped batch).  Missing the cap sets `capped` and yields 0; it never spins.
PQ_DEV uint32_t ob_perm(const ObKey& k, uint32_t j, uint32_t n, int half, bool& capped) {
  uint32_t x = j;
  for (int it = 0; it < OB_WALK_CAP; ++it) {
    x = ob_feistel(k, x, half);
    if (x < n) return x;
  }
  capped = true;
  return 0;
}

PQ_DEV double ob_min(double a, double b) { return b < a ? b : a; }
PQ_DEV double ob_max(double a, double b) { return b > a ? b : a; }
PQ_DEV double ob_add(double a, double b) { return a + b; }

// lane = op(lane, partner) over offsets 32 .. 1: the fixed butterfly of the restatement's _tree
template <typename Op> PQ_DEV double ob_wave(double v, Op op) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  return v;
}

struct ObXyz { double x, y, z; };
// one gathered row: rotated xyz in fp64, (x R0k + y R1k) + z R2k
PQ_DEV ObXyz ob_point(const float (&row)[6], const double (&R)[9], bool rot) {
  const double x = row[0], y = row[1], z = row[2];
  ObXyz o = {x, y, z};
  if (rot) {
    o.x = (x * R[0] + y * R[3]) + z * R[6];
    o.y = (x * R[1] + y * R[4]) + z * R[7];
    o.z = (x * R[2] + y * R[5]) + z * R[8];
  }
  return o;
}

// A padded slot's feature block: n6 floats of zeros (16-byte stores when the block is aligned).
PQ_DEV void ob_zero_block(float* __restrict__ dst, long n6, bool vec) {
  if (vec) {
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (long i = threadIdx.x; i < n6 / 4; i += 256) d4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (long i = threadIdx.x; i < n6; i += 256) dst[i] = 0.f;
  }
}

// One workgroup per (item, slot).  Thread t owns the pairs of draws (2 p, 2 p + 1), p = t + 256 k, k < KP, and keeps their
// gathered rows in registers: one gather, no scratch memory, and a pair is 48 contiguous bytes of the output (three
// 16-byte stores).  KP = ceil(num_points / 512) is a template parameter (1, 2, 4, 8).
template <int KP>
__global__ __launch_bounds__(256) void ob_sample_kernel(ObBank bk, const int32_t* __restrict__ scene_of_item,
                                                        const int32_t* __restrict__ selected, int O_max, int np,
                                                        const int64_t* __restrict__ seed, const float* __restrict__ rotation,
                                                        float* __restrict__ fts, float* __restrict__ locs, float* __restrict__ boxes,
                                                        uint8_t* __restrict__ pad, int* __restrict__ err) {
  __shared__ double red[4][10];
  __shared__ int serr;
  const int bq = blockIdx.x, b = bq / O_max, q = bq - b * O_max, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool vec = (np & 1) == 0;                       // an even num_points keeps every slot's block 16-byte aligned
  float* out = fts + (long)bq * np * 6;
  // ---- the slot's object, every index checked (uniform over the workgroup)
  const int s = scene_of_item[b], o = selected[bq];
  int e = 0;
  long e0 = 0, n = 0, P = 0;
  if (s < 0 || s >= bk.S) e = 1;
  else if (o != -1) {
    const int n_obj = bk.obj_off[s + 1] - bk.obj_off[s];
    if (o < 0 || o >= n_obj) e = 2;
    else {
      const long g = (long)bk.obj_off[s] + o;
      e0 = bk.entry_off[g];
      n = bk.entry_off[g + 1] - e0;
      P = bk.pt_off[s + 1] - bk.pt_off[s];
      if (n < 1 || n > P || P > PQ3D_OBJECT_MAX_POINTS) e = 16;
    }
  }
  bool live = e == 0 && o != -1;
  // ---- the draws (positions in the object's ascending point list) and their rows
  float rw[KP][2][6];
  bool bad = false;
  if (live) {
    const ObKey key = ob_key((uint64_t)seed[0], (uint32_t)b, (uint32_t)q);
    const float* pts = bk.points + bk.pt_off[s] * 6;
    int half = 1;
    while ((1L << (2 * half)) < n) ++half;               // n <= 2^20: at most 10 steps
    int pt[KP][2];
#pragma unroll
    for (int k = 0; k < KP; ++k)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * (tid + 256 * k) + h;
        pt[k][h] = 0;
        if (j < np) {
          uint32_t i;
          if (n == 1) i = 0;
          else if (n >= np) i = ob_perm(key, (uint32_t)j, (uint32_t)n, half, bad);
          else i = (uint32_t)(((uint64_t)ob_hash_j(key, (uint32_t)j) * (uint64_t)n) >> 32);
          int v = i < (uint64_t)n ? bk.order[e0 + i] : -1;
          if (v < 0 || v >= P) { v = 0; e = 16; }
          pt[k][h] = v;
        }
      }
#pragma unroll
    for (int k = 0; k < KP; ++k)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float2* r2 = reinterpret_cast<const float2*>(pts + (long)pt[k][h] * 6);     // (rows are 24 bytes: 8-byte aligned)
        const float2 a = r2[0], c = r2[1], d = r2[2];
        rw[k][h][0] = a.x; rw[k][h][1] = a.y; rw[k][h][2] = c.x; rw[k][h][3] = c.y; rw[k][h][4] = d.x; rw[k][h][5] = d.y;
      }
  }
  if (bad) e |= 4;
  if (tid == 0) serr = 0;
  __syncthreads();
  if (e) atomicOr(&serr, e);
  __syncthreads();
  e = serr;
  if (e) {
    if (tid == 0) atomicOr(err, e);
    live = false;
  }
  if (!live) {
    ob_zero_block(out, (long)np * 6, vec);
    if (tid < 6) { locs[(long)bq * 6 + tid] = 0.f; boxes[(long)bq * 6 + tid] = 0.f; }
    if (tid == 0) pad[bq] = 0;
    return;
  }
  const bool rot = rotation != nullptr;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (rot)
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rotation[(long)b * 9 + k];
  // ---- mean, min, max over the sampled points: the thread folds its draws in the order (k, h)
  double sm[3] = {0.0, 0.0, 0.0}, mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int k = 0; k < KP; ++k)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (2 * (tid + 256 * k) + h < np) {
        const ObXyz p = ob_point(rw[k][h], R, rot);
        const double c[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) { sm[a] = sm[a] + c[a]; mn[a] = ob_min(mn[a], c[a]); mx[a] = ob_max(mx[a], c[a]); }
      }
#pragma unroll
  for (int k = 0; k < 3; ++k) { sm[k] = ob_wave(sm[k], ob_add); mn[k] = ob_wave(mn[k], ob_min); mx[k] = ob_wave(mx[k], ob_max); }
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) { red[wave][k] = sm[k]; red[wave][3 + k] = mn[k]; red[wave][6 + k] = mx[k]; }
  __syncthreads();
  double mean[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mean[k] = ob_add(ob_add(red[0][k], red[1][k]), ob_add(red[2][k], red[3][k])) / (double)np;
    mn[k] = ob_min(ob_min(red[0][3 + k], red[1][3 + k]), ob_min(red[2][3 + k], red[3][3 + k]));
    mx[k] = ob_max(ob_max(red[0][6 + k], red[1][6 + k]), ob_max(red[2][6 + k], red[3][6 + k]));
  }
  if (tid < 3) {
    const double sz = mx[tid] - mn[tid];
    locs[(long)bq * 6 + tid] = (float)mean[tid];
    locs[(long)bq * 6 + 3 + tid] = (float)sz;
    boxes[(long)bq * 6 + tid] = (float)((mn[tid] + mx[tid]) / 2.0);
    boxes[(long)bq * 6 + 3 + tid] = (float)sz;
  }
  if (tid == 0) pad[bq] = 1;
  // ---- the largest distance from the mean
  double d2 = -INFINITY;
#pragma unroll
  for (int k = 0; k < KP; ++k)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (2 * (tid + 256 * k) + h < np) {
        const ObXyz p = ob_point(rw[k][h], R, rot);
        const double cx = p.x - mean[0], cy = p.y - mean[1], cz = p.z - mean[2];
        d2 = ob_max(d2, (cx * cx + cy * cy) + cz * cz);
      }
  d2 = ob_wave(d2, ob_max);
  if (lane == 0) red[wave][9] = d2;
  __syncthreads();
  double dist = __dsqrt_rn(ob_max(ob_max(red[0][9], red[1][9]), ob_max(red[2][9], red[3][9])));
  dist = dist > 1e-6 ? dist : 1e-6;
  // ---- the feature rows: (xyz - mean) / dist | rgb, rounded to fp32 once
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int pr = tid + 256 * k;
    float f[12];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const ObXyz p = ob_point(rw[k][h], R, rot);
      f[6 * h + 0] = (float)((p.x - mean[0]) / dist);
      f[6 * h + 1] = (float)((p.y - mean[1]) / dist);
      f[6 * h + 2] = (float)((p.z - mean[2]) / dist);
      f[6 * h + 3] = rw[k][h][3]; f[6 * h + 4] = rw[k][h][4]; f[6 * h + 5] = rw[k][h][5];
    }
    if (vec) {
      if (2 * pr < np) {
        float4* o4 = reinterpret_cast<float4*>(out) + (long)pr * 3;
#pragma unroll
        for (int h = 0; h < 3; ++h) o4[h] = make_float4(f[4 * h], f[4 * h + 1], f[4 * h + 2], f[4 * h + 3]);
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (2 * pr + h < np)
#pragma unroll
          for (int a = 0; a < 6; ++a) out[(long)(2 * pr + h) * 6 + a] = f[6 * h + a];
    }
  }
}

__global__ void ob_zero_err_kernel(int* __restrict__ err) { err[0] = 0; }

// --------------------------------------------------------------------------------------------------------------- labels
struct ObMatch {
  const int32_t* matched;     // [sum G_s]
  const uint8_t *iou25, *iou50;   // the scans' [G_s, K_s] tables, concatenated
  const int32_t* gt_off;      // [S + 1] first GT object of every scan in `matched`
  const int64_t* tab_off;     // [S + 1] first cell of every scan's table
};

__global__ __launch_bounds__(256) void ob_labels_kernel(const int32_t* __restrict__ obj_off, int S, const int32_t* __restrict__ scene_of_item,
                                                        const int32_t* __restrict__ selected, const int32_t* __restrict__ targets, int B,
                                                        int O_max, int T_max, ObMatch mt, float* __restrict__ out,
                                                        int* __restrict__ err) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, N = (long)B * O_max;
  if (i >= N) return;
  const int b = (int)(i / O_max), s = scene_of_item[b], o = selected[i];
  float l0 = 0.f, l25 = 0.f, l50 = 0.f;
  int e = 0;
  if (s < 0 || s >= S) e = 1;
  else {
    const int n_sel = obj_off[s + 1] - obj_off[s];
    const int n_tgt = mt.matched ? mt.gt_off[s + 1] - mt.gt_off[s] : n_sel;
    const bool sel_ok = o >= 0 && o < n_sel;
    if (o != -1 && !sel_ok) e |= 2;
    for (int k = 0; k < T_max; ++k) {
      const int t = targets[(long)b * T_max + k];
      if (t == -1) continue;
      if (t < 0 || t >= n_tgt) { e |= 8; continue; }
      if (!sel_ok) continue;
      if (!mt.matched) {
        if (t == o) l0 = l25 = l50 = 1.f;
      } else {
        const long cell = mt.tab_off[s] + (long)t * n_sel + o;
        if (mt.matched[mt.gt_off[s] + t] == o) l0 = 1.f;
        if (mt.iou25[cell]) l25 = 1.f;
        if (mt.iou50[cell]) l50 = 1.f;
      }
    }
  }
  out[i] = l0; out[N + i] = l25; out[2 * N + i] = l50;
  if (e) atomicOr(err, e);
}

// coord_min / coord_max [B, 3]: min / max of obj_locs[:, :3] over the valid slots (zeros for an item without one)
__global__ __launch_bounds__(256) void ob_range_kernel(const float* __restrict__ locs, const uint8_t* __restrict__ pad, int B, int O_max,
                                                       float* __restrict__ cmin, float* __restrict__ cmax) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * 3) return;
  const int b = i / 3, k = i - b * 3;
  float mn = INFINITY, mx = -INFINITY;
  bool any = false;
  for (int q = 0; q < O_max; ++q)
    if (pad[(long)b * O_max + q]) {
      const float v = locs[((long)b * O_max + q) * 6 + k];
      mn = fminf(mn, v); mx = fmaxf(mx, v);
      any = true;
    }
  cmin[i] = any ? mn : 0.f;
  cmax[i] = any ? mx : 0.f;
}

// out[b, q, :] = table[obj_off[scene] + selected[b, q], :], zeros for a padded (or out-of-range) slot
__global__ __launch_bounds__(256) void ob_rows_kernel(const float* __restrict__ table, int D, const int32_t* __restrict__ obj_off, int S,
                                                      const int32_t* __restrict__ scene_of_item, const int32_t* __restrict__ selected,
                                                      long N, int O_max, float* __restrict__ out) {
  for (long i = blockIdx.x; i < N; i += gridDim.x) {
    const int b = (int)(i / O_max), s = scene_of_item[b], o = selected[i];
    const float* src = nullptr;
    if (s >= 0 && s < S && o >= 0 && o < obj_off[s + 1] - obj_off[s]) src = table + ((long)obj_off[s] + o) * D;
    for (int k = threadIdx.x; k < D; k += 256) out[i * D + k] = src ? src[k] : 0.f;
  }
}

}  // namespace

static ObRows ob_rows(const int64_t* pt_off, const int64_t* row_off, const int64_t* cell_off, const int64_t* p2i, const int64_t* ids,
                      const uint8_t* masks, const int64_t* mask_off, int32_t S, int64_t R, int64_t cells) {
  ObRows a;
  a.pt_off = pt_off; a.row_off = row_off; a.cell_off = cell_off; a.p2i = p2i; a.ids = ids; a.masks = masks; a.mask_off = mask_off;
  a.S = S; a.R = (long)R; a.cells = (long)cells;
  return a;
}
#define OB_CHECK_ROWS(who)                                                                                                  \
  PQ_CHECK_ARG(pt_off && row_off && cell_off && S >= 1 && R >= 1 && R <= 2147483647LL && cells >= R, who ": null pointer or empty set"); \
  PQ_CHECK_ARG((masks != nullptr) != (point2instance != nullptr), who ": pass point2instance + instance_ids or masks");       \
  PQ_CHECK_ARG(masks ? mask_off != nullptr : instance_ids != nullptr, who ": null pointer")

extern "C" int pq3d_object_count(const int64_t* pt_off, const int64_t* row_off, const int64_t* cell_off, const int64_t* point2instance,
                                 const int64_t* instance_ids, const uint8_t* masks, const int64_t* mask_off, int32_t S, int64_t R,
                                 int64_t cells, int32_t* cnt, int32_t* cbase, int32_t* row_total, void* stream) {
  PQ_DEVICE_GUARD(stream, pt_off);
  OB_CHECK_ROWS("pq3d_object_count");
  PQ_CHECK_ARG(cnt && cbase && row_total, "pq3d_object_count: null pointer");
  const ObRows a = ob_rows(pt_off, row_off, cell_off, point2instance, instance_ids, masks, mask_off, S, R, cells);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ob_count_kernel, dim3(grid_cap((long)cells, 1)), dim3(256), 0, s, a, cnt);
  hipLaunchKernelGGL(ob_rowscan_kernel, dim3(grid_cap((long)R, 1)), dim3(256), 0, s, a, (const int*)cnt, cbase, row_total);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_object_emit(const int64_t* pt_off, const int64_t* row_off, const int64_t* cell_off, const int64_t* point2instance,
                                const int64_t* instance_ids, const uint8_t* masks, const int64_t* mask_off, int32_t S, int64_t R,
                                int64_t cells, const int32_t* cbase, const int64_t* row_entry, int64_t E, int32_t* order, void* stream) {
  PQ_DEVICE_GUARD(stream, pt_off);
  OB_CHECK_ROWS("pq3d_object_emit");
  PQ_CHECK_ARG(cbase && row_entry && E >= 0 && (E == 0 || order), "pq3d_object_emit: null pointer");
  const ObRows a = ob_rows(pt_off, row_off, cell_off, point2instance, instance_ids, masks, mask_off, S, R, cells);
  hipLaunchKernelGGL(ob_emit_kernel, dim3(grid_cap((long)cells, 1)), dim3(256), 0, (hipStream_t)stream, a, cbase, row_entry, (long)E, order);
  PQ_LAUNCH_CHECK();
  return 0;
}

#define OB_BANK(bk, who)                                                                                                    \
  PQ_CHECK_ARG(points && pt_off && obj_off && entry_off && order && S >= 1, who ": null pointer or no scan");              \
  ObBank bk;                                                                                                                \
  bk.points = points; bk.pt_off = pt_off; bk.obj_off = obj_off; bk.entry_off = entry_off; bk.order = order; bk.S = S

extern "C" int pq3d_object_boxes(const float* points, const int64_t* pt_off, const int32_t* obj_off, const int64_t* entry_off,
                                 const int32_t* order, int32_t S, const int32_t* obj_scan, int32_t O, float* box_center, float* box_size,
                                 void* stream) {
  PQ_DEVICE_GUARD(stream, points);
  OB_BANK(bk, "pq3d_object_boxes");
  PQ_CHECK_ARG(obj_scan && box_center && box_size && O >= 1, "pq3d_object_boxes: null pointer or no object");
  hipLaunchKernelGGL(ob_box_kernel, dim3(grid_cap(O, 1)), dim3(256), 0, (hipStream_t)stream, bk, obj_scan, (int)O, box_center, box_size);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_match_boxes(const float* gt_center, const float* gt_size, const float* pred_center, const float* pred_size, int32_t G,
                                int32_t K, int32_t* matched, uint8_t* iou25, uint8_t* iou50, void* stream) {
  PQ_DEVICE_GUARD(stream, gt_center);
  PQ_CHECK_ARG(G >= 1 && K >= 0 && gt_center && gt_size && matched, "pq3d_match_boxes: G >= 1, K >= 0, no null pointer");
  PQ_CHECK_ARG(K == 0 || (pred_center && pred_size && iou25 && iou50), "pq3d_match_boxes: null pointer");
  hipLaunchKernelGGL(ob_match_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gt_center, gt_size, pred_center,
                     pred_size, (int)G, (int)K, matched, iou25, iou50);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_object_sample(const float* points, const int64_t* pt_off, const int32_t* obj_off, const int64_t* entry_off,
                                  const int32_t* order, int32_t S, const int32_t* scene_of_item, const int32_t* selected, int32_t B,
                                  int32_t O_max, int32_t num_points, const int64_t* seed, const float* rotation, float* obj_fts,
                                  float* obj_locs, float* obj_boxes, uint8_t* obj_pad_masks, int32_t* err, void* stream) {
  PQ_DEVICE_GUARD(stream, points);
  OB_BANK(bk, "pq3d_object_sample");
  PQ_CHECK_ARG(scene_of_item && selected && seed && obj_fts && obj_locs && obj_boxes && obj_pad_masks && err,
               "pq3d_object_sample: null pointer");
  PQ_CHECK_ARG(B >= 1 && O_max >= 1 && (long)B * O_max <= 2147483647L, "pq3d_object_sample: B >= 1, O_max >= 1, B * O_max < 2^31");
  PQ_CHECK_ARG(num_points >= 1 && num_points <= PQ3D_OBJECT_MAX_SAMPLE, "pq3d_object_sample: 1 <= num_points <= PQ3D_OBJECT_MAX_SAMPLE");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ob_zero_err_kernel, dim3(1), dim3(1), 0, s, err);
#define OB_SAMPLE(KP)                                                                                                        \
  hipLaunchKernelGGL(ob_sample_kernel<KP>, dim3((unsigned)(B * O_max)), dim3(256), 0, s, bk, scene_of_item, selected, (int)O_max, \
                     (int)num_points, seed, rotation, obj_fts, obj_locs, obj_boxes, obj_pad_masks, err)
  if (num_points <= 512) OB_SAMPLE(1);
  else if (num_points <= 1024) OB_SAMPLE(2);
  else if (num_points <= 2048) OB_SAMPLE(4);
  else OB_SAMPLE(8);
#undef OB_SAMPLE
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_ground_labels(const int32_t* obj_off, int32_t S, const int32_t* scene_of_item, const int32_t* selected,
                                  const int32_t* targets, int32_t B, int32_t O_max, int32_t T_max, const int32_t* matched,
                                  const uint8_t* iou25, const uint8_t* iou50, const int32_t* gt_off, const int64_t* tab_off, float* labels,
                                  int32_t* err, void* stream) {
  PQ_DEVICE_GUARD(stream, obj_off);
  PQ_CHECK_ARG(obj_off && scene_of_item && selected && targets && labels && err, "pq3d_ground_labels: null pointer");
  PQ_CHECK_ARG(S >= 1 && B >= 1 && O_max >= 1 && T_max >= 1 && (long)B * O_max <= 2147483647L,
               "pq3d_ground_labels: S, B, O_max, T_max >= 1, B * O_max < 2^31");
  PQ_CHECK_ARG(!matched || (iou25 && iou50 && gt_off && tab_off), "pq3d_ground_labels: the match tables go together");
  ObMatch mt;
  mt.matched = matched; mt.iou25 = iou25; mt.iou50 = iou50; mt.gt_off = gt_off; mt.tab_off = tab_off;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ob_zero_err_kernel, dim3(1), dim3(1), 0, s, err);
  hipLaunchKernelGGL(ob_labels_kernel, dim3((unsigned)(((long)B * O_max + 255) / 256)), dim3(256), 0, s, obj_off, (int)S, scene_of_item,
                     selected, targets, (int)B, (int)O_max, (int)T_max, mt, labels, err);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_object_range(const float* obj_locs, const uint8_t* obj_pad_masks, int32_t B, int32_t O_max, float* coord_min,
                                 float* coord_max, void* stream) {
  PQ_DEVICE_GUARD(stream, obj_locs);
  PQ_CHECK_ARG(obj_locs && obj_pad_masks && coord_min && coord_max && B >= 1 && O_max >= 1 && (long)B * 3 <= 2147483647L,
               "pq3d_object_range: null pointer or empty batch");
  hipLaunchKernelGGL(ob_range_kernel, dim3((unsigned)((B * 3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, obj_locs, obj_pad_masks,
                     (int)B, (int)O_max, coord_min, coord_max);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_object_rows(const float* table, int32_t D, const int32_t* obj_off, int32_t S, const int32_t* scene_of_item,
                                const int32_t* selected, int32_t B, int32_t O_max, float* out, void* stream) {
  PQ_DEVICE_GUARD(stream, table);
  PQ_CHECK_ARG(table && obj_off && scene_of_item && selected && out && D >= 1 && S >= 1 && B >= 1 && O_max >= 1,
               "pq3d_object_rows: null pointer or empty shape");
  const long N = (long)B * O_max;
  hipLaunchKernelGGL(ob_rows_kernel, dim3(grid_cap(N, 1)), dim3(256), 0, (hipStream_t)stream, table, (int)D, obj_off, (int)S, scene_of_item,
                     selected, N, (int)O_max, out);
  PQ_LAUNCH_CHECK();
  return 0;
}
