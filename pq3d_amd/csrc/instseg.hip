// Instance-segmentation predictions of the mask head (per scene: top-k (query, class) pairs, mask scores, full-resolution
// masks by segment vote, boxes) as gfx950 kernels.
//
// Reference: InstSegEval.eval_instance_step with use_dbscan = False and filter_out_no_object_queries = False
// (evaluator/instseg_eval.py:85-149; get_mask_and_scores :283-304, get_full_res_mask :272-281, the predicted-box loop of
// record_preds :306-327), which copies everything to the host and loops over scenes and queries.
//
// One call over a batch of ragged scenes (scene b's voxels / points are rows [off[b], off[b+1]) of concatenated index maps)
// is a fixed number of launches whatever B is:
//   instseg_check_kernel   range checks of the three index maps (one flag word + the largest full-resolution segment id,
//                          read back once by the caller) and the voxels per segment (integer atomics);
//   instseg_compose_kernel per point: the composed row voxel2segment[voxel_to_full_maps[p]] + b * S of the [B*S, K] bit
//                          table and the batched full-resolution segment id segment_to_full_maps[p] + b * Sf;
//   instseg_prob_kernel    softmax over the C+1 classes, one wave per query row, last column dropped -> prob [B, Q*C];
//   instseg_filter_kernel  (filter_out_no_object_queries) per query row: 1 iff the argmax of the C+1 probabilities (ties:
//                          lower index) is not the no-object column C;
//   instseg_topk_kernel    one workgroup per scene: radix select of the K largest of the Q*C probabilities over their float
//                          bits (held in registers), LDS bitonic sort by (probability desc, flat index asc); the RAGGED form
//                          selects K_b = min(K, candidates) of scene b's own candidate range (per-scene offsets) and leaves
//                          out the rows of filtered queries (stored as bit pattern 0, below every kept candidate's bits + 1);
//   instseg_table_kernel   the [B*S, K] fp32 0/1 table [m > 0] (m = pred_masks[b][s][query_k]) and per-64-segment partial
//                          sums of n_s * sigmoid(m) * [m > 0] and n_s * [m > 0] (n_s = voxels of segment s): the voxel sums
//                          of the reference taken over segments; no [V, K] matrix;
//   instseg_rank_kernel    one workgroup per scene: final score = prob * sum / (count + 1e-6), LDS bitonic sort by
//                          (score desc, top-k rank asc);
//   (the vote sum[Sf-row, k] / count per full-resolution segment is pq3d_segment_reduce over the table, csrc/segment.hip)
//   instseg_expand_kernel  mask[p, j] = 2 * sum[key(p), order[j]] > count[key(p)] (exact: integer-valued fp32 sums) written
//                          as bytes in sorted column order, with per-256-point partial box sums (fp64) / minima / maxima;
//   instseg_box_kernel     per (scene, column): the partials in chunk order -> center, extent, valid;
//   instseg_gt_part_kernel the same partials over rows of 0/1 mask bytes [G', P] (the ground-truth boxes of
//                          record_preds :326-339), reduced by instseg_box_kernel.
// Every sum runs in a fixed order (no float atomics): results are bit-identical run to run.
#include "common.h"
#include "ragged.h"

namespace {

constexpr int SEG_CHUNK = PQ3D_INSTSEG_SEG_CHUNK;   // segments per table workgroup (one partial per chunk)
constexpr int PT_CHUNK = PQ3D_INSTSEG_PT_CHUNK;     // points per expand workgroup (one box partial per chunk)
constexpr int MAX_K = PQ3D_INSTSEG_MAX_K;

struct BoxPart {          // 64 bytes
  double s[3];            // coordinate sums
  float mn[3], mx[3];
  int n;                  // points
  int pad[3];
};
static_assert(sizeof(BoxPart) == PQ3D_INSTSEG_BOX_PART_BYTES, "box partial layout");

// ascending bitonic sort of keys[0, n) in LDS (n a power of two <= 1024, 1024 threads)
PQ_DEV void bitonic_sort_u64(unsigned long long* keys, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const int i = threadIdx.x;
      const int ixj = i ^ j;
      if (i < n && ixj > i) {
        const unsigned long long a = keys[i], c = keys[ixj];
        const bool up = (i & k) == 0;
        if ((a > c) == up) { keys[i] = c; keys[ixj] = a; }
      }
    }
  }
  __syncthreads();
}

PQ_DEV int pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// ---- 1. range checks + voxels per segment ------------------------------------------------------------------------------
// stats[0] |= 1: a voxel2segment id outside [0, S);  2: a voxel_to_full_maps id outside [0, V_b);  4: a negative
// segment_to_full_maps id.  stats[1] = max(segment_to_full_maps) + 1 over the batch.  nvox[b*S + s] += 1 per voxel.
__global__ __launch_bounds__(256) void instseg_check_kernel(const int64_t* __restrict__ v2s, const int64_t* __restrict__ v2f,
                                                            const int64_t* __restrict__ s2f, const int64_t* __restrict__ offs,
                                                            int B, long S, long NV, long NP, int* __restrict__ nvox,
                                                            unsigned long long* __restrict__ stats) {
  const int64_t* voff = offs;
  const int64_t* poff = offs + (B + 1);
  unsigned long long err = 0, mx = 0;
  const long n = NV > NP ? NV : NP;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (i < NV) {
      const int b = scene_of(voff, B, i);
      const int64_t s = v2s[i];
      if (s < 0 || s >= S) err |= 1;
      else atomicAdd(&nvox[(long)b * S + s], 1);
    }
    if (i < NP) {
      const int b = scene_of(poff, B, i);
      const int64_t v = v2f[i];
      if (v < 0 || v >= voff[b + 1] - voff[b]) err |= 2;
      const int64_t s2 = s2f[i];
      if (s2 < 0) err |= 4;
      else if ((unsigned long long)s2 + 1 > mx) mx = (unsigned long long)s2 + 1;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    err |= __shfl_xor(err, d);
    const unsigned long long o = __shfl_xor(mx, d);
    mx = o > mx ? o : mx;
  }
  __shared__ unsigned long long red[2][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = err; red[1][w] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < 4; ++i) { err |= red[0][i]; mx = red[1][i] > mx ? red[1][i] : mx; }
    // one flag word and one maximum for the whole grid: skip the atomics that would not change them (every block
    // contending for one address serialised the launch)
    if (err) atomicOr(&stats[0], err);
    if (mx > __hip_atomic_load(&stats[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&stats[1], mx);
  }
}

// ---- 2. composed indices -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void instseg_compose_kernel(const int64_t* __restrict__ v2s, const int64_t* __restrict__ v2f,
                                                              const int64_t* __restrict__ s2f, const int64_t* __restrict__ offs,
                                                              int B, long S, long Sf, long NP, int64_t* __restrict__ gather,
                                                              int64_t* __restrict__ key) {
  const int64_t* voff = offs;
  const int64_t* poff = offs + (B + 1);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NP; i += (long)gridDim.x * blockDim.x) {
    const int b = scene_of(poff, B, i);
    gather[i] = (int64_t)b * S + v2s[voff[b] + v2f[i]];
    key[i] = (int64_t)b * Sf + s2f[i];
  }
}

// ---- 3. softmax + top-K per scene ------------------------------------------------------------------------------------------
// 3a. prob[b, q*C + c] = softmax(logits[b, q, :])[c] for c < C (grid (ceil(Q / 4), B), one wave per query row)
__global__ __launch_bounds__(256) void instseg_prob_kernel(const float* __restrict__ logits, int Q, int C1,
                                                           float* __restrict__ prob) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
  if (q >= Q) return;
  const float* row = logits + ((long)b * Q + q) * C1;
  float m = -INFINITY;
  for (int c = lane; c < C1; c += 64) m = fmaxf(m, row[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C1; c += 64) s += expf(row[c] - m);
  s = wave_sum(s);
  const int C = C1 - 1;
  float* out = prob + ((long)b * Q + q) * C;
  for (int c = lane; c < C; c += 64) out[c] = expf(row[c] - m) / s;
}

// 3a'. valid[b*Q + q] = argmax_c softmax(logits[b, q, :])[c] != C over the C+1 probabilities (ties: lower index, as
// torch.argmax), with the same expression as instseg_prob_kernel (grid (ceil(Q / 4), B), one wave per query row)
__global__ __launch_bounds__(256) void instseg_filter_kernel(const float* __restrict__ logits, int Q, int C1,
                                                             int* __restrict__ valid) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
  if (q >= Q) return;
  const float* row = logits + ((long)b * Q + q) * C1;
  float m = -INFINITY;
  for (int c = lane; c < C1; c += 64) m = fmaxf(m, row[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C1; c += 64) s += expf(row[c] - m);
  s = wave_sum(s);
  float best = -INFINITY;
  int bi = C1;
  for (int c = lane; c < C1; c += 64) {
    const float p = expf(row[c] - m) / s;
    if (p > best || bi == C1) { best = p; bi = c; }       // ascending c per lane: strict > keeps the lower index
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const float ob = __shfl_xor(best, d);
    const int oi = __shfl_xor(bi, d);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) valid[(long)b * Q + q] = bi != C1 - 1 ? 1 : 0;
}

// sort key of a candidate: ascending key = descending probability, then ascending flat index (probabilities are >= 0, so
// their bit patterns order like the values)
PQ_DEV unsigned long long cand_key(unsigned u, int i) { return ((unsigned long long)(~u) << 32) | (unsigned)i; }

// 3b. one workgroup per scene over the n = Q*C probability bits: candidate i = tid + 1024 r lives in register r of thread tid
// (R > 0: n <= 1024 R, every pass runs on chip) or is re-read from the L2-resident prob array (R = 0, any n).
// RAGGED: scene b's candidates are prob[seg[b], seg[b+1]) (seg[b] a multiple of C, n = the largest range); a candidate of
// row r = (seg[b] + i) / C with qvalid[r] == 0 is left out.  Candidates are held as bits + 1 (0 = left out: below every
// kept one, so never selected while K_b <= kept); K_b = kall ? kept rows : min(K, kept candidates) (<= K), written to
// kout[b]; slots [K_b, K) of the outputs are padding (probability 0, query 0, class 0).
template <int R, bool RAGGED>
__global__ __launch_bounds__(1024) void instseg_topk_kernel(const float* __restrict__ prob, int n, int C, int K,
                                                            float* __restrict__ sel_prob, int* __restrict__ sel_query,
                                                            int* __restrict__ sel_class, const int64_t* __restrict__ seg,
                                                            const int* __restrict__ qvalid, int kall, int* __restrict__ kout) {
  __shared__ unsigned long long keys[MAX_K];
  __shared__ int hist[256];
  __shared__ int sm[SCAN_LDS];
  __shared__ int pick[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long base0 = RAGGED ? (long)seg[b] : (long)b * n;
  if constexpr (RAGGED) n = (int)(seg[b + 1] - seg[b]);
  const unsigned* U = (const unsigned*)prob + base0;
  int Kb = K;
  if constexpr (RAGGED) {
    const int rows = n / C;
    int kept = 0;
    for (int r0 = 0; r0 < rows; r0 += 1024) {
      const int r = r0 + tid;
      int tot;
      (void)block_excl_scan(r < rows && (!qvalid || qvalid[base0 / C + r]) ? 1 : 0, sm, tot);
      kept += tot;
    }
    const long kc = (long)kept * C;
    Kb = kall ? kept : (int)(kc < (long)K ? kc : (long)K);
    if (Kb > K) Kb = K;
    if (tid == 0) kout[b] = Kb;
  }
  // bits of candidate i (RAGGED: + 1, 0 when out of range or left out)
  auto load = [&](int i) -> unsigned {
    if constexpr (RAGGED) return i < n && (!qvalid || qvalid[base0 / C + i / C]) ? U[i] + 1u : 0u;
    else return i < n ? U[i] : 0u;
  };
  unsigned reg[R > 0 ? R : 1];
  if constexpr (R > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) reg[r] = load(tid + 1024 * r);
  }
  // f(i, u) for every candidate slot of this thread, in ascending tile order (the same trip count in every thread)
  auto for_each = [&](auto&& f) {
    if constexpr (R > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) f(tid + 1024 * r, reg[r]);
    } else {
      for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        f(i, load(i));
      }
    }
  };
  // radix select of the K-th largest bit pattern, 8 bits per pass from the top
  unsigned prefix = 0, pmask = 0;
  int need = Kb;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for_each([&](int i, unsigned u) {
      if (i < n && (u & pmask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);   // LDS integer atomics: order-free
    });
    __syncthreads();
    if (tid == 0) {
      int cum = 0, d = 255;
      for (; d > 0; --d) {
        if (cum + hist[d] >= need) break;
        cum += hist[d];
      }
      pick[0] = d;
      pick[1] = need - cum;
    }
    __syncthreads();
    prefix |= (unsigned)pick[0] << shift;
    pmask |= 255u << shift;
    need = pick[1];
    __syncthreads();
  }
  // the K survivors: every candidate above the threshold, and the `need` lowest flat indices equal to it
  const unsigned T = prefix;
  const int n_gt = Kb - need;
  int gt_carry = 0, eq_carry = 0;
  for_each([&](int i, unsigned u) {
    const int gt = i < n && u > T, eq = i < n && u == T;
    int tot;
    const int ex = block_excl_scan(gt | (eq << 16), sm, tot);   // <= 1024 per tile: both counts fit 16 bits
    if (gt) {
      const int slot = gt_carry + (ex & 0xffff);     // < n_gt by construction of T; the test only guards the LDS array
      if (slot < n_gt) keys[slot] = cand_key(u, i);
    }
    if (eq) {
      const int r = eq_carry + (ex >> 16);
      if (r < need) keys[n_gt + r] = cand_key(u, i);
    }
    gt_carry += tot & 0xffff;
    eq_carry += tot >> 16;
  });
  const int Kp = pow2_ceil(Kb);
  if (tid >= Kb && tid < Kp) keys[tid] = ~0ull;
  bitonic_sort_u64(keys, Kp);
  if (tid < Kb) {
    const unsigned long long k = keys[tid];
    const int i = (int)(k & 0xffffffffu);
    const int q = i / C;
    sel_prob[(long)b * K + tid] = __uint_as_float(~(unsigned)(k >> 32) - (RAGGED ? 1u : 0u));
    sel_query[(long)b * K + tid] = q;
    sel_class[(long)b * K + tid] = i - q * C;
  } else if (RAGGED && tid < K) {
    sel_prob[(long)b * K + tid] = 0.f;
    sel_query[(long)b * K + tid] = 0;
    sel_class[(long)b * K + tid] = 0;
  }
}
constexpr int TOPK_REGS = 48;    // register-resident candidates up to n = 49 152 (Q = 200 x C = 200 = 40 000)

// ---- 4. bit table + mask-score partial sums ---------------------------------------------------------------------------------
// grid (ceil(S / SEG_CHUNK), ceil(K / 64), B); lane = selection, waves stride over the chunk's segments
__global__ __launch_bounds__(256) void instseg_table_kernel(const float* __restrict__ masks, const int* __restrict__ nvox,
                                                            const int* __restrict__ sel_query, long S, int Q, int K,
                                                            float* __restrict__ table, double2* __restrict__ part) {
  __shared__ double2 red[4][64];
  const int chunk = blockIdx.x, b = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = blockIdx.y * 64 + lane;
  const bool kv = k < K;
  const int q = kv ? sel_query[(long)b * K + k] : 0;
  const long s0 = (long)chunk * SEG_CHUNK, s1 = min(S, s0 + SEG_CHUNK);
  double ss = 0.0, cc = 0.0;
  if (kv) {
#pragma unroll 4
    for (long s = s0 + w; s < s1; s += 4) {
      const long row = (long)b * S + s;
      const float m = masks[row * Q + q];
      const int nv = nvox[row];
      const bool on = m > 0.f;
      table[row * K + k] = on ? 1.f : 0.f;
      if (on) { ss += (double)nv * (double)sigmoidf_(m); cc += (double)nv; }
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

// ---- 5. final scores + sort per scene ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void instseg_rank_kernel(const double2* __restrict__ part, int nsc,
                                                            const float* __restrict__ sel_prob, const int* __restrict__ sel_class,
                                                            int K, float* __restrict__ scores, int64_t* __restrict__ classes,
                                                            int* __restrict__ order) {
  __shared__ unsigned long long keys[MAX_K];
  __shared__ float sc[MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Kp = pow2_ceil(K);
  if (tid < K) {
    double a = 0.0, c = 0.0;
#pragma unroll 4
    for (int i = 0; i < nsc; ++i) {
      const double2 p = part[((long)b * nsc + i) * K + tid];
      a += p.x;
      c += p.y;
    }
    // the reference's fp32 expression: (sigmoid * mask).sum(0) / (mask.sum(0) + 1e-6), times the class probability
    const float ms = (float)a / ((float)c + 1e-6f);
    const float s = sel_prob[(long)b * K + tid] * ms;
    sc[tid] = s;
    keys[tid] = cand_key(__float_as_uint(s), tid);
  } else if (tid < Kp) {
    keys[tid] = ~0ull;
  }
  bitonic_sort_u64(keys, Kp);
  if (tid < K) {
    const int r = (int)(keys[tid] & 0xffffffffu);
    scores[(long)b * K + tid] = sc[r];
    classes[(long)b * K + tid] = sel_class[(long)b * K + r];
    order[(long)b * K + tid] = r;
  }
}

// ---- 6. full-resolution masks + box partials ----------------------------------------------------------------------------------
// grid (point chunks, ceil(K / 64)); a chunk = PT_CHUNK points of one scene, wave w a quarter of them; lane = output
// column j (sorted order), reading the vote of top-k column order[j].  64 keys / coordinates are loaded per wave instruction and
// handed out with shuffles.
__global__ __launch_bounds__(256) void instseg_expand_kernel(const float* __restrict__ vsum, const float* __restrict__ vcount,
                                                             const int64_t* __restrict__ key, const float* __restrict__ coords,
                                                             const int64_t* __restrict__ offs, const int* __restrict__ order,
                                                             int B, int K, unsigned char* __restrict__ out,
                                                             BoxPart* __restrict__ part) {
  __shared__ double rs[4][3][64];
  __shared__ float rmn[4][3][64], rmx[4][3][64];
  __shared__ int rn[4][64];
  const int64_t* poff = offs + (B + 1);
  const int64_t* coff = offs + 2 * (B + 1);
  const long cid = blockIdx.x;
  const int b = scene_of(coff, B, cid);
  const long p0 = poff[b] + (cid - coff[b]) * PT_CHUNK;
  const long pend = min(p0 + PT_CHUNK, (long)poff[b + 1]);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = blockIdx.y * 64 + lane;
  const bool jv = j < K;
  const int r = jv ? order[(long)b * K + j] : 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  float mnx = INFINITY, mny = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxy = -INFINITY, mxz = -INFINITY;
  int cnt = 0;
  constexpr int PER_WAVE = PT_CHUNK / 4, DEPTH = 8;
  for (int sub = 0; sub < PER_WAVE / 64; ++sub) {
    const long pb = p0 + w * PER_WAVE + sub * 64;
    if (pb >= pend) break;
    const long pl = pb + lane;
    const bool pv = pl < pend;
    const int kl = pv ? (int)key[pl] : 0;
    const float xl = pv ? coords[3 * pl] : 0.f, yl = pv ? coords[3 * pl + 1] : 0.f, zl = pv ? coords[3 * pl + 2] : 0.f;
    const int np = (int)min((long)64, pend - pb);
    for (int t0 = 0; t0 < np; t0 += DEPTH) {
      // DEPTH vote loads in flight, then their thresholds / stores / box updates
      float sv[DEPTH], cv[DEPTH];
#pragma unroll
      for (int u = 0; u < DEPTH; ++u) {
        const int kp = __shfl(kl, (t0 + u) & 63);
        const bool ok = jv && t0 + u < np;
        sv[u] = ok ? vsum[(long)kp * K + r] : 0.f;
        cv[u] = ok ? vcount[kp] : 1.f;
      }
#pragma unroll
      for (int u = 0; u < DEPTH; ++u) {
        const int t = t0 + u;
        const float x = __shfl(xl, t & 63), y = __shfl(yl, t & 63), z = __shfl(zl, t & 63);
        if (jv && t < np) {
          const bool on = 2.f * sv[u] > cv[u];
          out[(pb + t) * K + j] = on ? 1 : 0;
          if (on) {
            sx += x; sy += y; sz += z;
            mnx = fminf(mnx, x); mny = fminf(mny, y); mnz = fminf(mnz, z);
            mxx = fmaxf(mxx, x); mxy = fmaxf(mxy, y); mxz = fmaxf(mxz, z);
            ++cnt;
          }
        }
      }
    }
  }
  rs[w][0][lane] = sx; rs[w][1][lane] = sy; rs[w][2][lane] = sz;
  rmn[w][0][lane] = mnx; rmn[w][1][lane] = mny; rmn[w][2][lane] = mnz;
  rmx[w][0][lane] = mxx; rmx[w][1][lane] = mxy; rmx[w][2][lane] = mxz;
  rn[w][lane] = cnt;
  __syncthreads();
  if (w == 0 && jv) {
    BoxPart o;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double s = 0.0;
      float mn = INFINITY, mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) { s += rs[i][d][lane]; mn = fminf(mn, rmn[i][d][lane]); mx = fmaxf(mx, rmx[i][d][lane]); }
      o.s[d] = s; o.mn[d] = mn; o.mx[d] = mx;
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) n += rn[i][lane];
    o.n = n;
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    part[cid * K + j] = o;
  }
}

// ---- 7. boxes from the partials: one workgroup per (column, scene); thread t takes chunks t, t+256, ... then a fixed-order
// tree over the threads (deterministic) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void instseg_box_kernel(const BoxPart* __restrict__ part, const int64_t* __restrict__ coff, int K,
                                                          float* __restrict__ boxes, unsigned char* __restrict__ valid) {
  __shared__ double rs[3][256];
  __shared__ float rmn[3][256], rmx[3][256];
  __shared__ int rn[256];
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int n = 0;
  for (long c = coff[b] + tid; c < coff[b + 1]; c += 256) {
    const BoxPart& p = part[c * K + j];
#pragma unroll
    for (int d = 0; d < 3; ++d) { s[d] += p.s[d]; mn[d] = fminf(mn[d], p.mn[d]); mx[d] = fmaxf(mx[d], p.mx[d]); }
    n += p.n;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) { rs[d][tid] = s[d]; rmn[d][tid] = mn[d]; rmx[d][tid] = mx[d]; }
  rn[tid] = n;
  for (int h = 128; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        rs[d][tid] += rs[d][tid + h];
        rmn[d][tid] = fminf(rmn[d][tid], rmn[d][tid + h]);
        rmx[d][tid] = fmaxf(rmx[d][tid], rmx[d][tid + h]);
      }
      rn[tid] += rn[tid + h];
    }
  }
  __syncthreads();
  if (tid < 3) {
    const int d = tid, nt = rn[0];
    float* o = boxes + ((long)b * K + j) * 6;
    o[d] = nt > 0 ? (float)(rs[d][0] / (double)nt) : 0.f;
    o[3 + d] = nt > 0 ? rmx[d][0] - rmn[d][0] : 0.f;
    if (d == 0) valid[(long)b * K + j] = nt > 0 ? 1 : 0;
  }
}

// ---- 8. boxes of 0/1 mask rows (the ground-truth boxes of InstSegEval.record_preds): row r = R mask bytes over the n_r points
// of its scene; chunk c of row r (GT_CHUNK points, coff[r] + c) -> one BoxPart with the same fixed-order fp64 sums as the
// expand kernel's, reduced by instseg_box_kernel (K = 1, one "scene" per row).  rinfo = {mask byte offset [R], first point
// [R], points [R], chunk offsets coff [R + 1]}.
constexpr int GT_CHUNK = PQ3D_INSTSEG_GT_CHUNK;
__global__ __launch_bounds__(256) void instseg_gt_part_kernel(const unsigned char* __restrict__ masks, const float* __restrict__ coords,
                                                              const int64_t* __restrict__ rinfo, int R, BoxPart* __restrict__ part) {
  __shared__ double rs[3][256];
  __shared__ float rmn[3][256], rmx[3][256];
  __shared__ int rn[256];
  const int64_t* moff = rinfo;
  const int64_t* pfirst = rinfo + R;
  const int64_t* npts = rinfo + 2 * R;
  const int64_t* coff = rinfo + 3 * R;
  const long cid = blockIdx.x;
  const int r = scene_of(coff, R, cid);
  const int tid = threadIdx.x;
  const long q0 = (cid - coff[r]) * GT_CHUNK, q1 = min(q0 + GT_CHUNK, (long)npts[r]);
  const unsigned char* m = masks + moff[r];
  const float* xyz = coords + 3 * pfirst[r];
  double s[3] = {0.0, 0.0, 0.0};
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int n = 0;
  for (long q = q0 + tid; q < q1; q += 256) {
    if (m[q]) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float v = xyz[3 * q + d];
        s[d] += v; mn[d] = fminf(mn[d], v); mx[d] = fmaxf(mx[d], v);
      }
      ++n;
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) { rs[d][tid] = s[d]; rmn[d][tid] = mn[d]; rmx[d][tid] = mx[d]; }
  rn[tid] = n;
  for (int h = 128; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        rs[d][tid] += rs[d][tid + h];
        rmn[d][tid] = fminf(rmn[d][tid], rmn[d][tid + h]);
        rmx[d][tid] = fmaxf(rmx[d][tid], rmx[d][tid + h]);
      }
      rn[tid] += rn[tid + h];
    }
  }
  __syncthreads();
  if (tid == 0) {
    BoxPart o;
#pragma unroll
    for (int d = 0; d < 3; ++d) { o.s[d] = rs[d][0]; o.mn[d] = rmn[d][0]; o.mx[d] = rmx[d][0]; }
    o.n = rn[0];
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    part[cid] = o;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" int pq3d_instseg_check(const int64_t* v2s, const int64_t* v2f, const int64_t* s2f, const int64_t* offs, int32_t B,
                                  int64_t S, int64_t NV, int64_t NP, int32_t* nvox, int64_t* stats, void* stream) {
  PQ_DEVICE_GUARD(stream, stats);
  PQ_CHECK_ARG(offs && nvox && stats && B >= 1 && S >= 1 && NV >= 0 && NP >= 0 && (v2s || NV == 0) &&
               (v2f || NP == 0) && (s2f || NP == 0), "pq3d_instseg_check: bad args");
  hipStream_t s = (hipStream_t)stream;
  ZeroList z;
  z.add(nvox, (long)B * S);
  z.add(stats, 4);
  const int e = pq3d_zero_launch(z, s);
  if (e) return e;
  const long n = NV > NP ? NV : NP;
  if (n > 0)
    hipLaunchKernelGGL(instseg_check_kernel, dim3(grid_cap(n, 256)), dim3(256), 0, s, v2s, v2f, s2f, offs, (int)B, (long)S,
                       (long)NV, (long)NP, nvox, (unsigned long long*)stats);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_compose(const int64_t* v2s, const int64_t* v2f, const int64_t* s2f, const int64_t* offs, int32_t B,
                                    int64_t S, int64_t Sf, int64_t NP, int64_t* gather, int64_t* key, void* stream) {
  PQ_DEVICE_GUARD(stream, gather);
  PQ_CHECK_ARG(offs && B >= 1 && S >= 1 && Sf >= 1 && NP >= 0 && (NP == 0 || (v2s && v2f && s2f && gather && key)),
               "pq3d_instseg_compose: bad args");
  if (NP == 0) return 0;
  hipLaunchKernelGGL(instseg_compose_kernel, dim3(grid_cap(NP, 256)), dim3(256), 0, (hipStream_t)stream, v2s, v2f, s2f, offs,
                     (int)B, (long)S, (long)Sf, (long)NP, gather, key);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_topk(const float* logits, int32_t B, int32_t Q, int32_t C1, int32_t K, float* prob, float* sel_prob,
                                 int32_t* sel_query, int32_t* sel_class, void* stream) {
  PQ_DEVICE_GUARD(stream, logits);
  PQ_CHECK_ARG(logits && prob && sel_prob && sel_query && sel_class && B >= 1 && Q >= 1 && C1 >= 2 && B < 65536,
               "pq3d_instseg_topk: bad args (B < 65536, Q >= 1, C1 >= 2)");
  const int64_t n = (int64_t)Q * (C1 - 1);
  PQ_CHECK_ARG(n < (1LL << 31) - 1024, "pq3d_instseg_topk: Q * C must fit 31 bits");
  PQ_CHECK_ARG(K >= 1 && K <= MAX_K && (int64_t)K <= n, "pq3d_instseg_topk: need 1 <= K <= min(1024, Q*C)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(instseg_prob_kernel, dim3((unsigned)((Q + 3) / 4), (unsigned)B), dim3(256), 0, s, logits, (int)Q, (int)C1, prob);
  if (n <= 1024L * TOPK_REGS)
    hipLaunchKernelGGL((instseg_topk_kernel<TOPK_REGS, false>), dim3((unsigned)B), dim3(1024), 0, s, (const float*)prob, (int)n,
                       (int)(C1 - 1), (int)K, sel_prob, (int*)sel_query, (int*)sel_class, (const int64_t*)nullptr,
                       (const int*)nullptr, 0, (int*)nullptr);
  else
    hipLaunchKernelGGL((instseg_topk_kernel<0, false>), dim3((unsigned)B), dim3(1024), 0, s, (const float*)prob, (int)n,
                       (int)(C1 - 1), (int)K, sel_prob, (int*)sel_query, (int*)sel_class, (const int64_t*)nullptr,
                       (const int*)nullptr, 0, (int*)nullptr);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_prob(const float* logits, int32_t B, int32_t Q, int32_t C1, float* prob, int32_t* qvalid,
                                 void* stream) {
  PQ_DEVICE_GUARD(stream, logits);
  PQ_CHECK_ARG(logits && prob && B >= 1 && Q >= 1 && C1 >= 2 && B < 65536, "pq3d_instseg_prob: bad args (B < 65536, Q >= 1, C1 >= 2)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(instseg_prob_kernel, dim3((unsigned)((Q + 3) / 4), (unsigned)B), dim3(256), 0, s, logits, (int)Q, (int)C1, prob);
  if (qvalid)
    hipLaunchKernelGGL(instseg_filter_kernel, dim3((unsigned)((Q + 3) / 4), (unsigned)B), dim3(256), 0, s, logits, (int)Q,
                       (int)C1, (int*)qvalid);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_topk_ragged(const float* prob, const int64_t* seg, const int32_t* qvalid, int32_t B, int32_t C,
                                        int32_t K, int32_t kall, int64_t max_n, float* sel_prob, int32_t* sel_query,
                                        int32_t* sel_class, int32_t* kout, void* stream) {
  PQ_DEVICE_GUARD(stream, seg);
  PQ_CHECK_ARG(prob && seg && sel_prob && sel_query && sel_class && kout && B >= 1 && B < 65536 && C >= 1 && K >= 1 &&
               K <= MAX_K && max_n >= 0, "pq3d_instseg_topk_ragged: bad args (B < 65536, C >= 1, 1 <= K <= 1024)");
  PQ_CHECK_ARG(max_n < (1LL << 31) - 1024, "pq3d_instseg_topk_ragged: candidates per scene must fit 31 bits");
  hipStream_t s = (hipStream_t)stream;
  if (max_n <= 1024L * TOPK_REGS)
    hipLaunchKernelGGL((instseg_topk_kernel<TOPK_REGS, true>), dim3((unsigned)B), dim3(1024), 0, s, prob, 0, (int)C, (int)K,
                       sel_prob, (int*)sel_query, (int*)sel_class, seg, (const int*)qvalid, (int)kall, (int*)kout);
  else
    hipLaunchKernelGGL((instseg_topk_kernel<0, true>), dim3((unsigned)B), dim3(1024), 0, s, prob, 0, (int)C, (int)K, sel_prob,
                       (int*)sel_query, (int*)sel_class, seg, (const int*)qvalid, (int)kall, (int*)kout);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_rank(const void* part, int64_t nsc, const float* sel_prob, const int32_t* sel_class, int32_t B,
                                 int32_t K, float* scores, int64_t* classes, int32_t* order, void* stream) {
  PQ_DEVICE_GUARD(stream, sel_prob);
  PQ_CHECK_ARG(part && sel_prob && sel_class && scores && classes && order && B >= 1 && B < 65536 && K >= 1 && K <= MAX_K &&
               nsc >= 0 && nsc < (1LL << 31), "pq3d_instseg_rank: bad args");
  hipLaunchKernelGGL(instseg_rank_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, (const double2*)part, (int)nsc,
                     sel_prob, (const int*)sel_class, (int)K, scores, classes, (int*)order);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_scores(const float* masks, const int32_t* nvox, const float* sel_prob, const int32_t* sel_query,
                                   const int32_t* sel_class, int32_t B, int64_t S, int32_t Q, int32_t K, float* table, void* ws,
                                   int64_t ws_bytes, float* scores, int64_t* classes, int32_t* order, void* stream) {
  PQ_DEVICE_GUARD(stream, masks);
  PQ_CHECK_ARG(masks && nvox && sel_prob && sel_query && sel_class && table && ws && scores && classes && order && B >= 1 &&
               S >= 1 && Q >= 1 && K >= 1 && K <= MAX_K, "pq3d_instseg_scores: bad args");
  const long nsc = (S + SEG_CHUNK - 1) / SEG_CHUNK;
  PQ_CHECK_ARG(ws_bytes >= (int64_t)B * nsc * K * 16, "pq3d_instseg_scores: workspace smaller than B * ceil(S / PQ3D_INSTSEG_SEG_CHUNK) * K * 16");
  PQ_CHECK_ARG((((uintptr_t)ws) & 15) == 0, "pq3d_instseg_scores: workspace must be 16-byte aligned");
  PQ_CHECK_ARG(nsc < 65536 * 256, "pq3d_instseg_scores: S too large");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(instseg_table_kernel, dim3((unsigned)nsc, (unsigned)((K + 63) / 64), (unsigned)B), dim3(256), 0, s, masks,
                     (const int*)nvox, (const int*)sel_query, (long)S, (int)Q, (int)K, table, (double2*)ws);
  hipLaunchKernelGGL(instseg_rank_kernel, dim3((unsigned)B), dim3(1024), 0, s, (const double2*)ws, (int)nsc, sel_prob,
                     (const int*)sel_class, (int)K, scores, classes, (int*)order);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_expand(const float* vsum, const float* vcount, const int64_t* key, const float* coords,
                                   const int64_t* offs, const int32_t* order, int32_t B, int64_t NP, int64_t n_chunks, int32_t K,
                                   uint8_t* masks, void* ws, int64_t ws_bytes, float* boxes, uint8_t* box_valid, void* stream) {
  PQ_DEVICE_GUARD(stream, boxes);
  PQ_CHECK_ARG(offs && order && boxes && box_valid && B >= 1 && NP >= 0 && n_chunks >= 0 && K >= 1 && K <= MAX_K &&
               (n_chunks == 0 || (vsum && vcount && key && coords && masks && ws)), "pq3d_instseg_expand: bad args");
  PQ_CHECK_ARG(n_chunks < (1LL << 31) && NP * (int64_t)K < (1LL << 62), "pq3d_instseg_expand: too many points");
  PQ_CHECK_ARG(n_chunks == 0 || (ws_bytes >= n_chunks * K * (int64_t)sizeof(BoxPart) && (((uintptr_t)ws) & 15) == 0),
               "pq3d_instseg_expand: workspace smaller than n_chunks * K * 64 bytes or not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (n_chunks > 0)
    hipLaunchKernelGGL(instseg_expand_kernel, dim3((unsigned)n_chunks, (unsigned)((K + 63) / 64)), dim3(256), 0, s, vsum, vcount,
                       key, coords, offs, (const int*)order, (int)B, (int)K, masks, (BoxPart*)ws);
  hipLaunchKernelGGL(instseg_box_kernel, dim3((unsigned)K, (unsigned)B), dim3(256), 0, s, (const BoxPart*)ws, offs + 2 * (B + 1),
                     (int)K, boxes, box_valid);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_instseg_gt_boxes(const uint8_t* masks, const float* coords, const int64_t* rinfo, int32_t R, int64_t n_chunks,
                                     void* ws, int64_t ws_bytes, float* boxes, uint8_t* box_valid, void* stream) {
  PQ_DEVICE_GUARD(stream, boxes);
  PQ_CHECK_ARG(rinfo && boxes && box_valid && R >= 1 && R < 65536 && n_chunks >= 0 &&
               (n_chunks == 0 || (masks && coords && ws)), "pq3d_instseg_gt_boxes: bad args (1 <= R < 65536)");
  PQ_CHECK_ARG(n_chunks < (1LL << 31), "pq3d_instseg_gt_boxes: too many points");
  PQ_CHECK_ARG(n_chunks == 0 || (ws_bytes >= n_chunks * (int64_t)sizeof(BoxPart) && (((uintptr_t)ws) & 15) == 0),
               "pq3d_instseg_gt_boxes: workspace smaller than n_chunks * 64 bytes or not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (n_chunks > 0)
    hipLaunchKernelGGL(instseg_gt_part_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, masks, coords, rinfo, (int)R,
                       (BoxPart*)ws);
  hipLaunchKernelGGL(instseg_box_kernel, dim3(1u, (unsigned)R), dim3(256), 0, s, (const BoxPart*)ws, rinfo + 3 * R, 1, boxes,
                     box_valid);
  PQ_LAUNCH_CHECK();
  return 0;
}
