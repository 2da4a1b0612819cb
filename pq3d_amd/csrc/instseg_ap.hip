// Overlap tables of instance-segmentation mask AP as gfx950 kernels: per scene, the point counts shared by every predicted
// mask column and every ground-truth instance, the void points of every column and the points of every instance.
//
// Reference: assign_instances_for_scan (common/eval_instseg.py), which recounts every (prediction, GT instance)
// intersection with numpy passes over all points of a scene, per prediction.  Here the counts of a batch of B ragged scenes
// (scene b's points are rows [poff[b], poff[b+1]) of the concatenated [NP, K] 0/1 mask bytes and [NP] GT ids) come from one
// pass over the mask bytes, in a fixed number of launches whatever B is:
//   ap_mark_kernel    per point: the id's label id / 1000 looked up in the valid-label rank table; a valid nonzero id gets
//                     the dense local key rank(label) * 1000 + id % 1000 (ascending in the id) and sets its bit in the
//                     scene's presence bit map; every other point (unlabeled, invalid label) is void (key -1); negative ids
//                     set an error bit;
//   ap_rank_kernel    one workgroup per scene: exclusive popcount prefix of the bit map words -> G_b, the scene's distinct
//                     valid ids (read back by the caller, with the error bits, to size the tables);
//   ap_keys_kernel    per point: its group goff[b] + rank of its id among the scene's ids, or the scene's void group
//                     goff[b] + G_b;
//   (the points are then grouped by pq3d_segment_plan: stable sort, segment offsets, <= 128-row pieces; segment_plan.h)
//   ap_count_kernel   one wave per piece: the byte rows of the piece's points (perm order) summed per column -- 4 columns per
//                     32-bit word when K % 4 == 0, as packed bytes (a piece has <= 128 rows, so no byte overflows) -- stored
//                     as the group's row of counts [NG, K] (a group of several pieces: integer atomics; exact, any order);
//   ap_gt_ids_kernel  the scene's ids in ascending order from the bit map;
//   ap_pack_kernel    per scene, into one int32 buffer read back once: gt_verts (group sizes), inter [K, G] (transposed),
//                     void [K] (the void group's row) and pred_verts [K] (the column's points: void + every group).
// Every count is an exact integer: results are bit-identical run to run.  Each mask byte is read once (ap_count_kernel).
#include "common.h"
#include "ragged.h"
#include "segment_plan.h"

namespace {

using namespace pq3d_plan;

constexpr int INST = PQ3D_AP_INST;

// ---- 1. local keys + presence bits --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ap_mark_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ poff, int B,
                                                      long NP, const int* __restrict__ lab_rank, int nlab, long W,
                                                      int* __restrict__ lkey, unsigned* __restrict__ bits,
                                                      unsigned long long* __restrict__ err_word) {
  unsigned long long err = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NP; i += (long)gridDim.x * blockDim.x) {
    const int64_t id = ids[i];
    int lk = -1;
    if (id < 0) {
      err |= 1;
    } else if (id != 0) {
      const int64_t lab = id / INST;
      const int r = lab < nlab ? lab_rank[lab] : -1;
      if (r >= 0) {
        lk = r * INST + (int)(id - lab * INST);
        unsigned* w = bits + (long)scene_of(poff, B, i) * W + (lk >> 5);
        const unsigned m = 1u << (lk & 31);
        // most points find their id's bit already set: skip the atomic then (an idempotent OR, so the race is harmless)
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(w, m);
      }
    }
    lkey[i] = lk;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) err |= __shfl_xor(err, d);
  if ((threadIdx.x & 63) == 0 && err) atomicOr(err_word, err);
}

// ---- 2. per scene: word prefix counts of the bit map, G_b ------------------------------------------------------------
__global__ __launch_bounds__(1024) void ap_rank_kernel(const unsigned* __restrict__ bits, long W, int* __restrict__ wpre,
                                                       int64_t* __restrict__ sizes) {
  __shared__ int sm[SCAN_LDS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long per = (W + 1023) / 1024;
  const long w0 = min(W, tid * per), w1 = min(W, w0 + per);
  const unsigned* bw = bits + (long)b * W;
  int n = 0;
  for (long w = w0; w < w1; ++w) n += __popc(bw[w]);
  int total;
  int run = block_excl_scan(n, sm, total);
  for (long w = w0; w < w1; ++w) {
    wpre[(long)b * W + w] = run;
    run += __popc(bw[w]);
  }
  if (tid == 0) sizes[b] = total;
}

// ---- 3. group of every point ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ap_keys_kernel(const int* __restrict__ lkey, const unsigned* __restrict__ bits,
                                                      const int* __restrict__ wpre, const int64_t* __restrict__ poff,
                                                      const int64_t* __restrict__ goff, int B, long NP, long W,
                                                      int64_t* __restrict__ key) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NP; i += (long)gridDim.x * blockDim.x) {
    const int b = scene_of(poff, B, i);
    const int lk = lkey[i];
    int64_t g;
    if (lk < 0) {
      g = goff[b + 1] - 1;                                  // the scene's void group
    } else {
      const long w = (long)b * W + (lk >> 5);
      g = goff[b] + wpre[w] + __popc(bits[w] & ((1u << (lk & 31)) - 1u));
    }
    key[i] = g;
  }
}

// ---- 4. segmented byte-row count --------------------------------------------------------------------------------------------
// Lanes of a wave: LPR = 1 << lpr_log2 lanes cover one row (VEC bytes each, KCH chunks per lane), 64 / LPR rows share one wave
// instruction; grid.y slices the columns.  Rows of a piece come from perm[] (64 at a time, one per lane, handed out with
// shuffles).  VEC = 4: a lane adds whole 32-bit words, i.e. 4 byte counters at once; the <= 128 rows of a piece keep every
// byte counter below 256, also after the sum over the lanes that shared an instruction.
template <int VEC> struct ByteVec;
template <> struct ByteVec<4> {
  static PQ_DEV unsigned ld(const uint8_t* p) { return __builtin_nontemporal_load((const unsigned*)p); }
};
template <> struct ByteVec<1> {
  static PQ_DEV unsigned ld(const uint8_t* p) { return __builtin_nontemporal_load(p); }
};

template <int VEC, int KCH>
__global__ __launch_bounds__(256) void ap_count_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ meta,
                                                       const int* __restrict__ perm, const int4* __restrict__ pieces,
                                                       int* __restrict__ out, long K, int lpr_log2) {
  constexpr int U = KCH >= 4 ? 2 : (KCH == 2 ? 4 : 8);     // row loads in flight per lane x KCH chunks = 8
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave >= meta[1]) return;
  const int4 pc = pieces[wave];
  const int lane = threadIdx.x & 63;
  const int LPR = 1 << lpr_log2, RPI = 64 >> lpr_log2;
  const int sub = lane >> lpr_log2, cl = lane & (LPR - 1);
  const long colw = (long)LPR * VEC;
  const long col0 = blockIdx.y * (colw * KCH) + cl * VEC;
  int rowv[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int r = pc.x + b * 64 + lane;
    rowv[b] = r < pc.y ? perm[r] : -1;
  }
  unsigned acc[KCH];
#pragma unroll
  for (int k = 0; k < KCH; ++k) acc[k] = 0u;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int nrows = min(64, pc.y - (pc.x + b * 64));
    if (nrows <= 0) break;
    for (int it0 = 0; it0 * RPI < nrows; it0 += U) {
      int rw[U];
      unsigned x[U][KCH];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = (it0 + u) * RPI + sub;
        rw[u] = __shfl(rowv[b], j & 63);
        if (j >= nrows) rw[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint8_t* p = masks + (long)(rw[u] < 0 ? 0 : rw[u]) * K + col0;
#pragma unroll
        for (int k = 0; k < KCH; ++k) x[u][k] = (rw[u] >= 0 && col0 + k * colw < K) ? ByteVec<VEC>::ld(p + k * colw) : 0u;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < KCH; ++k) acc[k] += x[u][k];
      }
    }
  }
  for (int m = LPR; m < 64; m <<= 1) {
#pragma unroll
    for (int k = 0; k < KCH; ++k) acc[k] += (unsigned)__shfl_xor((int)acc[k], m);
  }
  if (sub != 0) return;
  int* o = out + (long)pc.z * K;
#pragma unroll
  for (int k = 0; k < KCH; ++k) {
    const long c = col0 + k * colw;
    if (c >= K) continue;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int v = (int)((acc[k] >> (8 * e)) & 255u);
      if (pc.w < 0) o[c + e] = v;                           // the group's only piece
      else if (v) atomicAdd(&o[c + e], v);                  // integer sums: exact in any order
    }
  }
}

// ---- 5. the scene's ids in ascending order ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ap_gt_ids_kernel(const unsigned* __restrict__ bits, const int* __restrict__ wpre,
                                                        const int* __restrict__ labels, const int64_t* __restrict__ toff, long W,
                                                        int* __restrict__ packed) {
  const int b = blockIdx.y;
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  unsigned m = bits[(long)b * W + w];
  int r = wpre[(long)b * W + w];
  int* dst = packed + toff[b];
  while (m) {
    const int lk = (int)(w * 32) + __ffs(m) - 1;
    const int li = lk / INST;
    dst[r++] = labels[li] * INST + (lk - li * INST);
    m &= m - 1u;
  }
}

// ---- 6. per-scene tables: gt_verts [G], inter [K, G], void [K], pred_verts [K] after gt_ids [G] ---------------------------------
__global__ __launch_bounds__(256) void ap_pack_kernel(const int* __restrict__ out, const int* __restrict__ seg_off,
                                                      const int64_t* __restrict__ goff, const int64_t* __restrict__ toff, long K,
                                                      int* __restrict__ packed) {
  const int b = blockIdx.y;
  const long g0 = goff[b], G = goff[b + 1] - g0 - 1;
  int* dst = packed + toff[b] + G;
  const long n = G + K * G + K;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    if (e < G) {
      dst[e] = seg_off[g0 + e + 1] - seg_off[g0 + e];
    } else if (e < G + K * G) {
      const long k = (e - G) / G, g = (e - G) - k * G;
      dst[e] = out[(g0 + g) * K + k];
    } else {
      const long k = e - G - K * G;
      const int v = out[(g0 + G) * K + k];
      int s = v;
      for (long g = 0; g < G; ++g) s += out[(g0 + g) * K + k];
      dst[e] = v;
      dst[e + K] = s;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" int pq3d_ap_ids(const int64_t* ids, const int64_t* poff, int32_t B, int64_t NP, const int32_t* lab_rank,
                           int32_t nlab, int64_t W, int32_t* lkey, uint32_t* bits, int32_t* wpre, int64_t* sizes,
                           void* stream) {
  PQ_DEVICE_GUARD(stream, sizes);
  PQ_CHECK_ARG(poff && lab_rank && bits && wpre && sizes && B >= 1 && NP >= 0 && (NP == 0 || (ids && lkey)) && nlab >= 1 &&
               nlab <= PQ3D_AP_MAX_LABELS && W >= 1 && (int64_t)B * W < (1LL << 40), "pq3d_ap_ids: bad args");
  PQ_CHECK_ARG(W * 32 <= (int64_t)PQ3D_AP_MAX_LABELS * INST + 32, "pq3d_ap_ids: W larger than the label domain needs");
  PQ_CHECK_ARG(NP < (1LL << 31) - 65536, "pq3d_ap_ids: too many points for one call");
  hipStream_t s = (hipStream_t)stream;
  ZeroList z;
  z.add(bits, (long)B * W);
  z.add(sizes, 2 * (long)(B + 1));
  const int e = pq3d_zero_launch(z, s);
  if (e) return e;
  if (NP > 0)
    hipLaunchKernelGGL(ap_mark_kernel, dim3(grid_cap(NP, 256)), dim3(256), 0, s, ids, poff, (int)B, (long)NP, (const int*)lab_rank,
                       (int)nlab, (long)W, (int*)lkey, (unsigned*)bits, (unsigned long long*)(sizes + B));
  hipLaunchKernelGGL(ap_rank_kernel, dim3((unsigned)B), dim3(1024), 0, s, (const unsigned*)bits, (long)W, (int*)wpre, sizes);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_ap_keys(const int32_t* lkey, const uint32_t* bits, const int32_t* wpre, const int64_t* poff,
                            const int64_t* goff, int32_t B, int64_t NP, int64_t W, int64_t* key, void* stream) {
  PQ_DEVICE_GUARD(stream, goff);
  PQ_CHECK_ARG(bits && wpre && poff && goff && B >= 1 && NP >= 0 && W >= 1 && (NP == 0 || (lkey && key)),
               "pq3d_ap_keys: bad args");
  if (NP == 0) return 0;
  hipLaunchKernelGGL(ap_keys_kernel, dim3(grid_cap(NP, 256)), dim3(256), 0, (hipStream_t)stream, (const int*)lkey,
                     (const unsigned*)bits, (const int*)wpre, poff, goff, (int)B, (long)NP, (long)W, key);
  PQ_LAUNCH_CHECK();
  return 0;
}

template <int VEC, int KCH>
static void launch_count(const uint8_t* masks, const int* P, const PlanLayout& L, int* out, int64_t K, int lpr_log2, int ycols,
                         hipStream_t s) {
  const unsigned blocks = (unsigned)((L.max_pieces + 3) / 4);
  hipLaunchKernelGGL((ap_count_kernel<VEC, KCH>), dim3(blocks, (unsigned)ycols), dim3(256), 0, s, masks, P + L.meta, P + L.perm,
                     (const int4*)(P + L.pieces), out, (long)K, lpr_log2);
}

extern "C" int pq3d_ap_count(const uint8_t* masks, int64_t K, const void* plan, int64_t N, int64_t NG, int32_t* out,
                             void* stream) {
  PQ_DEVICE_GUARD(stream, out);
  PQ_CHECK_ARG(plan && out && NG >= 1 && N >= 0 && (masks || N == 0) && K >= 1 && K <= PQ3D_AP_MAX_K,
               "pq3d_ap_count: bad args (1 <= K <= PQ3D_AP_MAX_K)");
  PQ_CHECK_ARG(N < (1LL << 31) - 65536 && NG < (1LL << 31) - 65536 && NG * K < (1LL << 40), "pq3d_ap_count: too large");
  hipStream_t s = (hipStream_t)stream;
  ZeroList z;
  z.add(out, NG * K);
  const int e = pq3d_zero_launch(z, s);
  if (e) return e;
  const PlanLayout L = plan_layout(N, NG);
  const int* P = (const int*)plan;
  const int vec = (K % 4 == 0 && (((uintptr_t)masks) & 3) == 0) ? 4 : 1;
  const long chunks = K / vec + (K % vec != 0);
  int lg = 0;
  while ((1L << lg) < chunks && lg < 6) ++lg;
  const long per = (chunks + (1L << lg) - 1) >> lg;
  const int kch = per >= 3 ? 4 : (int)per;
  const long colw = (1L << lg) * vec * kch;
  const int ycols = (int)((K + colw - 1) / colw);
#define PQ_AP_COUNT(V, C) launch_count<V, C>(masks, P, L, out, K, lg, ycols, s)
  if (vec == 4) { if (kch == 1) PQ_AP_COUNT(4, 1); else if (kch == 2) PQ_AP_COUNT(4, 2); else PQ_AP_COUNT(4, 4); }
  else          { if (kch == 1) PQ_AP_COUNT(1, 1); else if (kch == 2) PQ_AP_COUNT(1, 2); else PQ_AP_COUNT(1, 4); }
#undef PQ_AP_COUNT
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_ap_pack(const int32_t* out, const void* plan, int64_t N, int64_t NG, const uint32_t* bits,
                            const int32_t* wpre, const int32_t* labels, const int64_t* goff, const int64_t* toff, int32_t B,
                            int64_t K, int64_t W, int64_t max_entries, int32_t* packed, void* stream) {
  PQ_DEVICE_GUARD(stream, packed);
  PQ_CHECK_ARG(out && plan && bits && wpre && labels && goff && toff && packed && B >= 1 && B < 65536 && K >= 1 &&
               K <= PQ3D_AP_MAX_K && W >= 1 && NG >= B && max_entries >= 0, "pq3d_ap_pack: bad args");
  hipStream_t s = (hipStream_t)stream;
  const PlanLayout L = plan_layout(N, NG);
  const int* P = (const int*)plan;
  hipLaunchKernelGGL(ap_gt_ids_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)B), dim3(256), 0, s, (const unsigned*)bits,
                     (const int*)wpre, (const int*)labels, toff, (long)W, (int*)packed);
  hipLaunchKernelGGL(ap_pack_kernel, dim3(grid_cap(max_entries, 256), (unsigned)B), dim3(256), 0, s, (const int*)out,
                     P + L.seg_off, goff, toff, (long)K, (int*)packed);
  PQ_LAUNCH_CHECK();
  return 0;
}
