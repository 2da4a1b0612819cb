// Instance-segmentation training targets from per-point ids: what the reference builds per scene on the host
// (data/datasets/sceneverse_instseg.py extract_inst_info) and pads in instseg_wrapper.collate_fn, for a batch of ragged scenes:
//   1  it_first_kernel   per point: lowest point index of every instance id (atomicMin into a table of cap + 1 slots per scene),
//                        the scene's largest segment id, the range checks.
//   2  it_rank_kernel    one workgroup per scene: label of every present id (point2semantic at its first point), the class
//                        filter, rows = exclusive scan of "kept" in ascending id order; instance_ids, labels, n_inst.
//   3  it_cells_*_kernel per point: the mask cell (row of the point's instance, the point's segment).  Bytes are stored as 1
//                        (every writer stores the same value); the fp32 cells of the padded form are exchanged, and the thread
//                        that saw 0 bumps the row's integer count, so that t_sum is an exact count.
//   4  it_full_kernel    full_masks [G_b, P_b] bytes: a thread keeps the rows of 16 consecutive points in registers and writes
//                        one 16-byte store per mask row; nothing but stores depends on G.
// Atomics decide only who writes first, never a value.  Ids are range-checked (instance_targets_check.h) before they index
// anything; every table bound a kernel uses comes from the host (kernel arguments), never from the data.
#include "common.h"
#include "instance_targets_check.h"
#include "ragged.h"

#include <limits.h>

namespace {

constexpr int IT_CAP = PQ3D_INSTANCE_MAX_IDS, IT_SLOTS = IT_CAP + 1;     // slot 0: id -1, slot id + 1: id
constexpr int IT_NT = 1024, IT_PER = (IT_SLOTS + IT_NT - 1) / IT_NT;      // it_rank_kernel: consecutive slots per thread
constexpr int FM_PTS = 16, FM_ROWS = 8;                                   // it_full_kernel: points per thread, mask rows per block
static_assert(IT_CAP <= 32767, "prank holds a point's row as int16");

typedef SceneTable<PQ3D_INSTANCE_MAX_SCENES> ItScenes;

struct ItFilter {
  int n;
  long long v[PQ3D_INSTANCE_MAX_FILTER];
};

// per-scene shapes and bases of the list form (all from the host): segment_masks [rows, cols] at byte moff, full_masks
// [rows, P_b] at byte foff, prank at entry poff (a multiple of 16), it_full_kernel's blocks [blk0[b], blk0[b + 1])
struct ItMasks {
  long long rows[PQ3D_INSTANCE_MAX_SCENES], cols[PQ3D_INSTANCE_MAX_SCENES], moff[PQ3D_INSTANCE_MAX_SCENES],
      foff[PQ3D_INSTANCE_MAX_SCENES], poff[PQ3D_INSTANCE_MAX_SCENES];
  int blk0[PQ3D_INSTANCE_MAX_SCENES + 1];
};

__global__ __launch_bounds__(256) void it_init_kernel(int* __restrict__ first, long nfirst, int64_t* __restrict__ labels, long nlab,
                                                      int* __restrict__ n_inst, int* __restrict__ seg_len, int B,
                                                      int* __restrict__ err) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  for (long k = i; k < nfirst; k += step) first[k] = INT_MAX;
  for (long k = i; k < nlab; k += step) labels[k] = 0;
  if (i < B) { n_inst[i] = 0; seg_len[i] = 0; }
  if (i == 0) err[0] = 0;
}

__global__ __launch_bounds__(256) void it_first_kernel(const int64_t* __restrict__ p2i, const int64_t* __restrict__ p2s, ItScenes sc,
                                                       long P, long long seg_limit, int* __restrict__ first,
                                                       int* __restrict__ seg_len, int* __restrict__ err) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < P;
  int b = -1, top = 0, e = 0;
  if (live) {
    b = sc.scene(i);
    const int slot = pq_it_slot(p2i[i], IT_CAP);
    if (slot < 0) e |= 1;
    else {
      // the table only decreases, so a (possibly stale) value <= this index already settles it without an atomic
      const int local = (int)(i - sc.off[b]);
      int* f = first + (long)b * IT_SLOTS + slot;
      if (*f > local) atomicMin(f, local);
    }
    const int64_t seg = p2s[i];
    if (pq_it_seg_ok(seg, seg_limit)) top = (int)seg + 1;
    else e |= 2;
  }
  if (e) atomicOr(err, e);
  // the scene's segment count: one atomicMax per wave where the wave lies inside one scene (lane 0 holds the lowest point)
  const int b0 = __shfl(b, 0, 64);
  if (__all(!live || b == b0)) {
    int m = top;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(seg_len + b0, m);
  } else if (top > 0) {
    atomicMax(seg_len + b, top);
  }
}

__global__ __launch_bounds__(IT_NT) void it_rank_kernel(const int64_t* __restrict__ p2sem, ItScenes sc, ItFilter fl, int max_rows,
                                                        const int* __restrict__ first, int* __restrict__ rank,
                                                        int64_t* __restrict__ ids, int64_t* __restrict__ labels,
                                                        int* __restrict__ n_inst, int* __restrict__ err) {
  __shared__ int lds[SCAN_LDS];
  const int b = blockIdx.x, k0 = threadIdx.x * IT_PER;
  const long long n = sc.off[b + 1] - sc.off[b];
  bool keep[IT_PER];
  int64_t lab[IT_PER];
  int c = 0;
#pragma unroll
  for (int j = 0; j < IT_PER; ++j) {
    const int k = k0 + j;
    keep[j] = false;
    lab[j] = 0;
    if (k >= 1 && k < IT_SLOTS) {                         // (slot 0, id -1, is never an instance)
      const int f = first[(long)b * IT_SLOTS + k];
      if (f >= 0 && f < n) {                              // present (INT_MAX: no point carries the id)
        const int64_t l = p2sem[sc.off[b] + f];
        bool drop = false;
#pragma unroll
        for (int q = 0; q < PQ3D_INSTANCE_MAX_FILTER; ++q) drop |= q < fl.n && fl.v[q] == l;
        keep[j] = !drop;
        lab[j] = l;
      }
    }
    c += keep[j] ? 1 : 0;
  }
  int total;
  int r = block_excl_scan(c, lds, total);
#pragma unroll
  for (int j = 0; j < IT_PER; ++j) {
    const int k = k0 + j;
    if (k >= IT_SLOTS) break;
    int row = -1;
    if (keep[j]) {
      if (r < max_rows) {
        row = r;
        if (ids) ids[(long)b * max_rows + r] = k - 1;
        labels[(long)b * max_rows + r] = lab[j];
      }
      ++r;
    }
    rank[(long)b * IT_SLOTS + k] = row;
  }
  if (threadIdx.x == 0) {
    n_inst[b] = min(total, max_rows);
    if (total > max_rows) atomicOr(err, 4);
  }
}

// list form: segment_masks bytes and every point's row (prank, for it_full_kernel)
__global__ __launch_bounds__(256) void it_cells_kernel(const int64_t* __restrict__ p2i, const int64_t* __restrict__ p2s, ItScenes sc,
                                                       long P, const int* __restrict__ rank, ItMasks mk,
                                                       uint8_t* __restrict__ segmask, int16_t* __restrict__ prank) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int b = sc.scene(i);
  const int slot = pq_it_slot(p2i[i], IT_CAP);
  int r = slot < 0 ? -1 : rank[(long)b * IT_SLOTS + slot];
  if (r >= mk.rows[b]) r = -1;
  if (prank) prank[mk.poff[b] + (i - sc.off[b])] = (int16_t)r;
  const int64_t cell = pq_it_cell(r, p2s[i], mk.rows[b], mk.cols[b]);
  if (cell >= 0) segmask[mk.moff[b] + cell] = 1;
}

// padded form: T [B, Nt, Ns] fp32 cells and the rows' counts
__global__ __launch_bounds__(256) void it_cells_padded_kernel(const int64_t* __restrict__ p2i, const int64_t* __restrict__ p2s,
                                                              ItScenes sc, long P, const int* __restrict__ rank, int Ns, int Nt,
                                                              unsigned* __restrict__ T, int* __restrict__ cnt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int b = sc.scene(i);
  const int slot = pq_it_slot(p2i[i], IT_CAP);
  if (slot < 0) return;
  const int r = rank[(long)b * IT_SLOTS + slot];
  const int64_t cell = pq_it_cell(r, p2s[i], Nt, Ns);
  if (cell < 0) return;
  unsigned* c = T + (long)b * Nt * Ns + cell;
  // a cell only goes from 0 to 1.0f: one that already reads as set needs no exchange; a stale 0 only costs the exchange
  if (*c == 0u && atomicExch(c, 0x3f800000u) == 0u) atomicAdd(cnt + (long)b * Nt + r, 1);
}

__global__ __launch_bounds__(256) void it_count_kernel(const int* __restrict__ cnt, long n, float* __restrict__ t_sum) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) t_sum[i] = (float)cnt[i];
}

// full_masks: block (x, y) = 256 * FM_PTS consecutive points of one scene x FM_ROWS mask rows.  The 16 rows of a thread's
// points are read once (two 16-byte loads: prank is padded to 16 entries per scene); per mask row the thread stores 16
// bytes, consecutive lanes consecutive addresses.  A mask row starts at any byte (P_b is arbitrary), so the stores are
// unaligned 16-byte copies; the scene's last, partial chunk goes out as bytes.
__global__ __launch_bounds__(256) void it_full_kernel(ItScenes sc, ItMasks mk, const int16_t* __restrict__ prank,
                                                      uint8_t* __restrict__ out) {
  const int b = ragged_find(mk.blk0, sc.B, (int)blockIdx.x);
  const long long Pb = sc.off[b + 1] - sc.off[b], G = mk.rows[b];
  const long long p = ((long long)((int)blockIdx.x - mk.blk0[b]) * 256 + threadIdx.x) * FM_PTS;
  const long long g0 = (long long)blockIdx.y * FM_ROWS, g1 = min(g0 + FM_ROWS, G);
  if (p >= Pb || g0 >= G) return;
  const int n = (int)min((long long)FM_PTS, Pb - p);
  const uint4* src = reinterpret_cast<const uint4*>(prank + mk.poff[b] + p);
  const uint4 lo = src[0], hi = src[1];
  const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};          // two rows per word (0xffff: none)
  for (long long g = g0; g < g1; ++g) {
    const unsigned gg = (unsigned)g;
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      o[q] = ((w[2 * q] & 0xffffu) == gg ? 1u : 0u) | ((w[2 * q] >> 16) == gg ? 0x100u : 0u) |
             ((w[2 * q + 1] & 0xffffu) == gg ? 0x10000u : 0u) | ((w[2 * q + 1] >> 16) == gg ? 0x1000000u : 0u);
    uint8_t* dst = out + mk.foff[b] + g * Pb + p;
    if (n == FM_PTS) {
      __builtin_memcpy(dst, o, 16);
    } else {
#pragma unroll
      for (int j = 0; j < FM_PTS; ++j)
        if (j < n) dst[j] = (uint8_t)((o[j >> 2] >> (8 * (j & 3))) & 1u);
    }
  }
}

}  // namespace

// host: the scene table from an entry point's `offsets` and `B`, or its argument error
#define IT_TABLE(sc, who) PQ_SCENE_TABLE(sc, offsets, B, PQ3D_VOXELIZE_MAX_POINTS, PQ3D_VOXELIZE_MAX_POINTS, who)

extern "C" int pq3d_instance_tables(const int64_t* point2instance, const int64_t* point2semantic, const int64_t* point2segment,
                                    const int64_t* offsets, int32_t B, const int64_t* filter, int32_t n_filter, int64_t seg_limit,
                                    int32_t max_rows, int32_t* first, int32_t* rank, int64_t* instance_ids, int64_t* labels,
                                    int32_t* n_inst, int32_t* seg_len, int32_t* err, void* stream) {
  PQ_DEVICE_GUARD(stream, point2instance);
  PQ_CHECK_ARG(point2instance && point2semantic && point2segment && first && rank && labels && n_inst && seg_len && err,
               "pq3d_instance_tables: null pointer");
  ItScenes sc;
  IT_TABLE(sc, "pq3d_instance_tables");
  PQ_CHECK_ARG(n_filter >= 0 && n_filter <= PQ3D_INSTANCE_MAX_FILTER && (n_filter == 0 || filter),
               "pq3d_instance_tables: 0 <= n_filter <= PQ3D_INSTANCE_MAX_FILTER classes, filter a host array");
  PQ_CHECK_ARG(seg_limit >= 1 && seg_limit <= PQ3D_INSTANCE_MAX_SEGMENTS, "pq3d_instance_tables: 1 <= seg_limit <= PQ3D_INSTANCE_MAX_SEGMENTS");
  PQ_CHECK_ARG(max_rows >= 1 && max_rows <= PQ3D_INSTANCE_MAX_IDS, "pq3d_instance_tables: 1 <= max_rows <= PQ3D_INSTANCE_MAX_IDS");
  ItFilter fl;
  fl.n = n_filter;
  for (int q = 0; q < PQ3D_INSTANCE_MAX_FILTER; ++q) fl.v[q] = q < n_filter ? filter[q] : 0;
  const long P = (long)offsets[B];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(it_init_kernel, dim3(64), dim3(256), 0, s, first, (long)B * IT_SLOTS, labels, (long)B * max_rows, n_inst, seg_len,
                     (int)B, err);
  hipLaunchKernelGGL(it_first_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, point2instance, point2segment, sc, P,
                     (long long)seg_limit, first, seg_len, err);
  hipLaunchKernelGGL(it_rank_kernel, dim3(B), dim3(IT_NT), 0, s, point2semantic, sc, fl, (int)max_rows, (const int*)first, rank,
                     instance_ids, labels, n_inst, err);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instance_masks(const int64_t* point2instance, const int64_t* point2segment, const int64_t* offsets, int32_t B,
                                   const int32_t* rank, const int64_t* rows, const int64_t* cols, void* segment_masks, void* prank,
                                   void* full_masks, void* stream) {
  PQ_DEVICE_GUARD(stream, point2instance);
  PQ_CHECK_ARG(point2instance && point2segment && rank && rows && cols, "pq3d_instance_masks: null pointer");
  PQ_CHECK_ARG((prank != nullptr) == (full_masks != nullptr), "pq3d_instance_masks: full_masks and prank go together");
  ItScenes sc;
  IT_TABLE(sc, "pq3d_instance_masks");
  ItMasks mk = {};
  long long moff = 0, foff = 0, poff = 0, gmax = 0;
  int blk = 0;
  for (int b = 0; b < B; ++b) {
    PQ_CHECK_ARG(rows[b] >= 0 && rows[b] <= PQ3D_INSTANCE_MAX_IDS && cols[b] >= 0 && cols[b] <= PQ3D_INSTANCE_MAX_SEGMENTS,
                 "pq3d_instance_masks: rows in [0, PQ3D_INSTANCE_MAX_IDS], cols in [0, PQ3D_INSTANCE_MAX_SEGMENTS]");
    const long long Pb = offsets[b + 1] - offsets[b];
    mk.rows[b] = rows[b]; mk.cols[b] = cols[b]; mk.moff[b] = moff; mk.foff[b] = foff; mk.poff[b] = poff; mk.blk0[b] = blk;
    moff += rows[b] * cols[b];
    foff += rows[b] * Pb;
    poff += (Pb + FM_PTS - 1) / FM_PTS * FM_PTS;
    blk += (int)((Pb + 256 * FM_PTS - 1) / (256 * FM_PTS));
    gmax = rows[b] > gmax ? rows[b] : gmax;
  }
  for (int b = B; b <= PQ3D_INSTANCE_MAX_SCENES; ++b) mk.blk0[b] = blk;
  PQ_CHECK_ARG(moff == 0 || segment_masks, "pq3d_instance_masks: null pointer");
  const long P = (long)offsets[B];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(it_cells_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, point2instance, point2segment, sc, P, rank, mk,
                     (uint8_t*)segment_masks, (int16_t*)prank);
  if (full_masks && gmax > 0)
    hipLaunchKernelGGL(it_full_kernel, dim3((unsigned)blk, (unsigned)((gmax + FM_ROWS - 1) / FM_ROWS)), dim3(256), 0, s, sc, mk,
                       (const int16_t*)prank, (uint8_t*)full_masks);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instance_masks_padded(const int64_t* point2instance, const int64_t* point2segment, const int64_t* offsets,
                                          int32_t B, const int32_t* rank, int32_t Ns, int32_t Nt, float* T, int32_t* cnt, float* t_sum,
                                          void* stream) {
  PQ_DEVICE_GUARD(stream, point2instance);
  PQ_CHECK_ARG(point2instance && point2segment && rank && T && cnt && t_sum, "pq3d_instance_masks_padded: null pointer");
  ItScenes sc;
  IT_TABLE(sc, "pq3d_instance_masks_padded");
  PQ_CHECK_ARG(Ns >= 1 && Ns <= PQ3D_INSTANCE_MAX_SEGMENTS && Nt >= 1 && Nt <= PQ3D_INSTANCE_MAX_IDS,
               "pq3d_instance_masks_padded: 1 <= Ns <= PQ3D_INSTANCE_MAX_SEGMENTS, 1 <= Nt <= PQ3D_INSTANCE_MAX_IDS");
  const long P = (long)offsets[B], rows = (long)B * Nt;
  hipStream_t s = (hipStream_t)stream;
  PQ_CHECK_ARG(hipMemsetAsync(T, 0, (size_t)rows * Ns * sizeof(float), s) == hipSuccess &&
                   hipMemsetAsync(cnt, 0, (size_t)rows * sizeof(int32_t), s) == hipSuccess,
               "pq3d_instance_masks_padded: hipMemsetAsync failed");
  hipLaunchKernelGGL(it_cells_padded_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, point2instance, point2segment, sc, P,
                     rank, (int)Ns, (int)Nt, (unsigned*)T, cnt);
  hipLaunchKernelGGL(it_count_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const int*)cnt, rows, t_sum);
  PQ_LAUNCH_CHECK();
  return 0;
}
