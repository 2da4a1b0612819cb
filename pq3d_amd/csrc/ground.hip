// Stage-2 grounding loss and the refer evaluators' device part (the specification is tests/ground_eval_ref.py).
//   loss     bce_fwd_kernel     ONE workgroup of 1024 threads: clamp(x, min = -100) -> BCE-with-logits, summed in fp64 in a fixed
//                               order (thread-strided, 64-lane butterfly, 16 wave sums in a fixed tree), weight * mean + addend
//            bce_bwd_kernel     elementwise: g * weight / N * (sigmoid(x) - y), exactly 0 below the clamp
//   refer    refer_kernel       ONE workgroup, one wave per row: argmax, the hit bits of the prediction, the count table
//   f1       f1_cost_kernel     one workgroup per item: the slots sigmoid selects (block scan, slot order), the padded square
//                               -IoU matrix that evaluate_one_query hands to linear_sum_assignment
//            f1_count_kernel    one wave per item, after pq3d_lsap_batched: matched pairs of the selected rows at IoU 0.25 / 0.5
// No floating-point atomics and no cross-workgroup communication: two runs give the same bits.  Every index that comes from
// the caller's data (n_tgt, the assignment's rows and columns, tgt) is range-checked before it indexes anything.
#include "common.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace {

constexpr int BCE_THREADS = 1024, BCE_WAVES = BCE_THREADS / 64;

PQ_DEV double gr_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(BCE_THREADS) void bce_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long N,
                                                              float weight, const float* __restrict__ addend,
                                                              float* __restrict__ loss) {
  __shared__ double red[BCE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0;
  for (long i = tid; i < N; i += BCE_THREADS) {
    const float v = x[i];
    const float c = v < -100.f ? -100.f : v;              // (a NaN fails the comparison and stays)
    const float sp = log1pf(expf(-fabsf(c)));
    s = s + (((c > 0.f ? (double)c : 0.0) - (double)c * (double)y[i]) + (double)sp);
  }
  s = gr_wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double t[BCE_WAVES];
#pragma unroll
    for (int k = 0; k < BCE_WAVES; ++k) t[k] = red[k];
#pragma unroll
    for (int w = BCE_WAVES / 2; w > 0; w >>= 1)
#pragma unroll
      for (int k = 0; k < w; ++k) t[k] = t[k] + t[k + w];
    double r = (double)weight * (t[0] / (double)N);
    if (addend) r = r + (double)addend[0];
    loss[0] = (float)r;
  }
}

__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, long N, float weight,
                                                      const float* __restrict__ g, float* __restrict__ dx) {
  const double scale = (double)g[0] * (double)weight / (double)N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    const float v = x[i];
    float d = 0.f;
    if (!(v < -100.f)) d = (float)(scale * (1.0 / (1.0 + exp(-(double)v)) - (double)y[i]));
    dx[i] = d;
  }
}

// ---------------------------------------------------------------------------------------------------------------- refer
// a beats b: torch.argmax's order -- NaN is maximal, ties go to the smaller index
PQ_DEV bool gr_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ia < ib);
  return a > b || (a == b && ia < ib);
}

constexpr int RC_GROUPS = PQ3D_REFER_GROUPS, RC_COLS = 4;

__global__ __launch_bounds__(256) void refer_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                    const int64_t* __restrict__ tgt, const uint8_t* __restrict__ is_multiple,
                                                    const uint8_t* __restrict__ is_hard, const uint8_t* __restrict__ is_view_dep,
                                                    const uint8_t* __restrict__ item_mask, int B, int O, int* __restrict__ pred,
                                                    uint8_t* __restrict__ hits, int* __restrict__ counts) {
  __shared__ int red[4][RC_GROUPS * RC_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long BO = (long)B * O;
  int cnt[RC_GROUPS * RC_COLS];                           // lane 0's running table (every index a compile-time constant)
#pragma unroll
  for (int k = 0; k < RC_GROUPS * RC_COLS; ++k) cnt[k] = 0;
  for (int b = wave; b < B; b += 4) {
    const float* row = logits + (long)b * O;
    float bv = -INFINITY;
    int bi = 2147483647;                                  // (an empty lane loses to every real slot, -inf included)
    for (int j = lane; j < O; j += 64) {
      const float v = row[j];
      if (gr_better(v, j, bv, bi)) { bv = v; bi = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (gr_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {                                      // O >= 1: lane 0 holds slot 0, so 0 <= bi < O
      const long at = (long)b * O + bi;
      const bool h0 = tgt ? tgt[b] == (int64_t)bi : labels[at] != 0.f;
      const bool h25 = labels && labels[BO + at] != 0.f, h50 = labels && labels[2 * BO + at] != 0.f;
      const bool on = !item_mask || item_mask[b];
      pred[b] = bi;
      hits[b] = (uint8_t)((h0 ? 1 : 0) | (h25 ? 2 : 0) | (h50 ? 4 : 0) | (on ? 8 : 0));
      if (on) {
        const int add[RC_COLS] = {1, h0 ? 1 : 0, h25 ? 1 : 0, h50 ? 1 : 0};
        const uint8_t* fl[3] = {is_multiple, is_hard, is_view_dep};
#pragma unroll
        for (int c = 0; c < RC_COLS; ++c) cnt[c] += add[c];
#pragma unroll
        for (int f = 0; f < 3; ++f)
          if (fl[f]) {
            const bool set = fl[f][b] != 0;
#pragma unroll
            for (int c = 0; c < RC_COLS; ++c) {
              cnt[(1 + 2 * f) * RC_COLS + c] += set ? add[c] : 0;
              cnt[(2 + 2 * f) * RC_COLS + c] += set ? 0 : add[c];
            }
          }
      }
    }
  }
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < RC_GROUPS * RC_COLS; ++k) red[wave][k] = cnt[k];
  __syncthreads();
  if (threadIdx.x < RC_GROUPS * RC_COLS) {
    const int k = threadIdx.x;
    counts[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// ------------------------------------------------------------------------------------------------------------------- f1
// box3d_iou(construct_bbox_corners(pred), construct_bbox_corners(gt)) as evaluate_one_query meets it: the predicted box is an
// fp32 array (corners and volume in fp32), the target a list of Python floats (fp64); the rest is fp64, stored as fp32.
PQ_DEV float gr_iou(const float* __restrict__ p, const double* __restrict__ t) {
  double inter = 0.0, v2 = 0.0;
  float v1 = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ph = p[3 + k] / 2.f, pa = ph + p[k], pb = -ph + p[k];
    const float pmin = fminf(pa, pb), pmax = fmaxf(pa, pb);
    const double th = t[3 + k] / 2.0, ta = th + t[k], tb = -th + t[k];
    const double tmin = ta < tb ? ta : tb, tmax = ta < tb ? tb : ta;
    const double lo = (double)pmin > tmin ? (double)pmin : tmin, hi = (double)pmax < tmax ? (double)pmax : tmax;
    const double d = hi - lo > 0.0 ? hi - lo : 0.0;
    inter = k == 0 ? d : inter * d;
    v1 = k == 0 ? pmax - pmin : v1 * (pmax - pmin);
    v2 = k == 0 ? tmax - tmin : v2 * (tmax - tmin);
  }
  return (float)(inter / ((((double)v1 + v2) - inter) + 1e-8));
}

__global__ __launch_bounds__(256) void f1_cost_kernel(const float* __restrict__ logits, const float* __restrict__ obj_boxes,
                                                      const double* __restrict__ tgt_boxes, const int* __restrict__ n_tgt, int B, int O,
                                                      int T_max, int n, float* __restrict__ cost, int* __restrict__ sizes,
                                                      int* __restrict__ sel) {
  __shared__ int lds[SCAN_LDS];
  __shared__ int ssel[PQ3D_LSAP_MAX_DIM];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (long)b * O;
  // ---- the selected slots in slot order: thread t owns slots 4 t .. 4 t + 3 (O <= 1024)
  unsigned f = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = tid * 4 + q;
    if (j < O && sigmoidf_(row[j]) > 0.5f) f |= 1u << q;
  }
  int P;
  int e = block_excl_scan((int)__popc(f), lds, P);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if ((f >> q) & 1u) ssel[e++] = tid * 4 + q;           // e < P <= O <= 1024
  __syncthreads();
  int G = n_tgt[b], err = 0;
  if (G < 0 || G > T_max) { err = 1; G = 0; P = 0; }      // nothing is indexed through a bad count
  const int nb = P > G ? P : G;
  for (int j = tid; j < O; j += 256) sel[(long)b * O + j] = j < P ? ssel[j] : -1;
  if (tid == 0) {
    sizes[b] = P; sizes[B + b] = G; sizes[2 * B + b] = nb; sizes[3 * B + b] = err;
  }
  float* c = cost + (long)b * n * n;
  const float* ob = obj_boxes + (long)b * O * 6;
  const double* tb = tgt_boxes + (long)b * T_max * 6;
  for (int cell = tid; cell < nb * nb; cell += 256) {     // nb <= n <= 1024: no overflow
    const int i = cell / nb, j = cell - i * nb;
    float v = 0.f;
    if (i < P && j < G) v = -gr_iou(ob + (long)ssel[i] * 6, tb + (long)j * 6);
    c[(long)i * n + j] = v;
  }
}

__global__ __launch_bounds__(256) void f1_count_kernel(const float* __restrict__ cost, const int* __restrict__ row_idx,
                                                       const int* __restrict__ col_idx, const int* __restrict__ n_match,
                                                       const int* __restrict__ lsap_err, int B, int n, int* __restrict__ sizes,
                                                       int* __restrict__ out) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                     // (whole waves leave; no barrier below)
  const int P = sizes[b], G = sizes[B + b], nb = sizes[2 * B + b];
  int m = n_match[b], err = lsap_err[b] ? 2 : 0;
  if (m < 0 || m > n || (!err && m != nb)) { err |= 4; m = 0; }
  int t25 = 0, t50 = 0, bad = 0;
  for (int k = lane; k < m; k += 64) {
    const int r = row_idx[(long)b * n + k], c = col_idx[(long)b * n + k];
    if (r < 0 || r >= nb || c < 0 || c >= nb) { bad = 1; continue; }
    if (r < P) {
      const float iou = -cost[((long)b * n + r) * n + c];
      t25 += iou >= 0.25f ? 1 : 0;
      t50 += iou >= 0.5f ? 1 : 0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    t25 += __shfl_xor(t25, off, 64);
    t50 += __shfl_xor(t50, off, 64);
    bad |= __shfl_xor(bad, off, 64);
  }
  if (lane == 0) {
    if (bad) err |= 4;
    out[(long)b * 4 + 0] = t25; out[(long)b * 4 + 1] = t50; out[(long)b * 4 + 2] = P; out[(long)b * 4 + 3] = G;
    if (err) sizes[3 * B + b] |= err;                     // (this wave is the item's only writer)
  }
}

}  // namespace

extern "C" int pq3d_bce_logits_fwd(const float* x, const float* y, int64_t N, float weight, const float* addend, float* loss,
                                   void* stream) {
  PQ_DEVICE_GUARD(stream, x);
  PQ_CHECK_ARG(x && y && loss && N >= 1 && N <= PQ3D_BCE_MAX_N, "pq3d_bce_logits_fwd: null pointer or N outside [1, PQ3D_BCE_MAX_N]");
  hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(BCE_THREADS), 0, (hipStream_t)stream, x, y, (long)N, weight, addend, loss);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_bce_logits_bwd(const float* x, const float* y, int64_t N, float weight, const float* g, float* dx, void* stream) {
  PQ_DEVICE_GUARD(stream, x);
  PQ_CHECK_ARG(x && y && g && dx && N >= 1 && N <= PQ3D_BCE_MAX_N, "pq3d_bce_logits_bwd: null pointer or N outside [1, PQ3D_BCE_MAX_N]");
  hipLaunchKernelGGL(bce_bwd_kernel, dim3(grid_cap((long)N, 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)N, weight, g, dx);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_refer_counts(const float* logits, const float* labels, const int64_t* tgt, const uint8_t* is_multiple,
                                 const uint8_t* is_hard, const uint8_t* is_view_dependent, const uint8_t* item_mask, int32_t B,
                                 int32_t O, int32_t* pred, uint8_t* hits, int32_t* counts, void* stream) {
  PQ_DEVICE_GUARD(stream, logits);
  PQ_CHECK_ARG(logits && pred && hits && counts && (labels || tgt), "pq3d_refer_counts: null pointer (labels or tgt is needed)");
  PQ_CHECK_ARG(B >= 1 && O >= 1 && (long)B * O <= 2147483647L / 3, "pq3d_refer_counts: B >= 1, O >= 1, 3 * B * O < 2^31");
  hipLaunchKernelGGL(refer_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, tgt, is_multiple, is_hard,
                     is_view_dependent, item_mask, (int)B, (int)O, pred, hits, counts);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_ground_f1_cost(const float* logits, const float* obj_boxes, const double* tgt_boxes, const int32_t* n_tgt, int32_t B,
                                   int32_t O, int32_t T_max, float* cost, int32_t* sizes, int32_t* selected, void* stream) {
  PQ_DEVICE_GUARD(stream, logits);
  PQ_CHECK_ARG(logits && obj_boxes && tgt_boxes && n_tgt && cost && sizes && selected, "pq3d_ground_f1_cost: null pointer");
  PQ_CHECK_ARG(B >= 1 && O >= 1 && T_max >= 1 && O <= PQ3D_LSAP_MAX_DIM && T_max <= PQ3D_LSAP_MAX_DIM,
               "pq3d_ground_f1_cost: B >= 1, 1 <= O, T_max <= PQ3D_LSAP_MAX_DIM");
  const int n = O > T_max ? O : T_max;
  PQ_CHECK_ARG((long)B * n <= 2147483647L / n, "pq3d_ground_f1_cost: B * n * n < 2^31");
  hipLaunchKernelGGL(f1_cost_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, obj_boxes, tgt_boxes, n_tgt, (int)B,
                     (int)O, (int)T_max, n, cost, sizes, selected);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_ground_f1_count(const float* cost, const int32_t* row_idx, const int32_t* col_idx, const int32_t* n_match,
                                    const int32_t* lsap_err, int32_t B, int32_t n, int32_t* sizes, int32_t* out, void* stream) {
  PQ_DEVICE_GUARD(stream, cost);
  PQ_CHECK_ARG(cost && row_idx && col_idx && n_match && lsap_err && sizes && out, "pq3d_ground_f1_count: null pointer");
  PQ_CHECK_ARG(B >= 1 && n >= 1 && n <= PQ3D_LSAP_MAX_DIM, "pq3d_ground_f1_count: B >= 1, 1 <= n <= PQ3D_LSAP_MAX_DIM");
  hipLaunchKernelGGL(f1_count_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, cost, row_idx, col_idx, n_match,
                     lsap_err, (int)B, (int)n, sizes, out);
  PQ_LAUNCH_CHECK();
  return 0;
}
