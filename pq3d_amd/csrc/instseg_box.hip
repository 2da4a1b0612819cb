// Box matching of detection AP (eval_det_cls, common/eval_det.py) as one gfx950 kernel: for a batch of B ragged scenes, every
// detection's best same-class ground-truth box (ovmax / jmax) and whether it is a true positive at up to 4 IoU thresholds.
//
// Reference: eval_det_cls walks all detections of a class in descending score order; each looks at the same-class GT boxes
// of its own scene, takes the first maximum of calc_iou under a strict >, and is a TP iff ovmax > ovthresh and that GT box is
// not taken yet.  ovmax / jmax depend neither on the threshold nor on the taken flags, and the flags are per scene, so a
// detection is a TP at threshold t iff it is the first in score order among its scene's detections with the same jmax and
// ovmax > t.  That is what this kernel computes, one workgroup per scene, one detection per thread:
//   1. rank of every detection inside the scene by (-score, column) from the scores in LDS (no sorted input assumed);
//   2. the scene's GT rows staged once, BM_TILE at a time, as fp64 corners c -+ l / 2, volume (l0 * l1) * l2 and label; every
//      thread walks the staged rows in row order (uniform LDS addresses: broadcast reads) and keeps the first maximum;
//   3. winner per (GT row, threshold): integer minimum over ranks in an LDS table (atomicMin: the result does not depend on
//      the order); a detection is a TP where the winner's rank is its own.
// calc_iou on float64 copies of the fp32 boxes, in the reference's operation order, no contraction: IoU = 0 unless
// min(max_a, max_b) > max(min_a, min_b) strictly on all three axes; inter = (d0 * d1) * d2; inter / ((vol_a + vol_b) - inter).
// No floating-point atomics, no traffic between workgroups, no allocation: capturable, bit-identical run to run.
#include "common.h"

namespace {

constexpr int BM_THREADS = PQ3D_AP_MAX_K;                  // one detection per thread
constexpr int BM_TILE = 512;                               // GT rows staged at a time
// LDS: gmin / gmax [3][BM_TILE] + gvol [BM_TILE] fp64, glab [BM_TILE] int64, score [BM_THREADS] fp32, gok [BM_TILE] int32,
// then the winner table [max_g * T] int32
constexpr int BM_FIXED_BYTES = BM_TILE * (7 * 8 + 8) + BM_THREADS * 4 + BM_TILE * 4;
constexpr int BM_MAX_BYTES = BM_FIXED_BYTES + PQ3D_BOX_MAX_G * PQ3D_BOX_MAX_T * 4;
static_assert(BM_MAX_BYTES <= 160 * 1024, "box_match_kernel: LDS");

__global__ __launch_bounds__(BM_THREADS) void box_match_kernel(
    const float* __restrict__ pboxes, const int64_t* __restrict__ pclasses, const float* __restrict__ pscores,
    const uint8_t* __restrict__ pvalid, const int64_t* __restrict__ koff, long NK, const float* __restrict__ gboxes,
    const int64_t* __restrict__ glabels, const uint8_t* __restrict__ gvalid, const int64_t* __restrict__ goff, long NG,
    const double* __restrict__ thresholds, int T, int max_g, double* __restrict__ ovmax, int* __restrict__ jmax,
    uint8_t* __restrict__ flags, int* __restrict__ err) {
  extern __shared__ double bm_lds[];
  double* gmin = bm_lds;                                   // [3][BM_TILE]
  double* gmax = gmin + 3 * BM_TILE;                       // [3][BM_TILE]
  double* gvol = gmax + 3 * BM_TILE;                       // [BM_TILE]
  long long* glab = (long long*)(gvol + BM_TILE);          // [BM_TILE]
  float* score = (float*)(glab + BM_TILE);                 // [BM_THREADS]
  int* gok = (int*)(score + BM_THREADS);                   // [BM_TILE]
  int* win = gok + BM_TILE;                                // [G * T], G <= max_g

  const int b = blockIdx.x, tid = threadIdx.x;
  const long k0 = koff[b], k1 = koff[b + 1], g0 = goff[b], g1 = goff[b + 1];
  // nothing is indexed through a bad offset (uniform over the workgroup)
  if (k0 < 0 || k1 < k0 || k1 > NK || k1 - k0 > BM_THREADS || g0 < 0 || g1 < g0 || g1 > NG || g1 - g0 > max_g) {
    if (tid == 0) atomicOr(err, 8);
    return;
  }
  const int K = (int)(k1 - k0), G = (int)(g1 - g0);
  const double ninf = -__builtin_inf();
  int myerr = 0;

  // ---- this thread's detection
  const bool have = tid < K;
  bool ok = false;
  float sc = 0.f;
  long long cls = 0;
  double amin[3], amax[3], avol = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) amin[a] = amax[a] = 0.0;
  if (have && pvalid[k0 + tid]) {
    sc = pscores[k0 + tid];
    cls = pclasses[k0 + tid];
    const float* p = pboxes + (k0 + tid) * 6;
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float cf = p[a], lf = p[3 + a];
      fin = fin && __builtin_isfinite(cf) && __builtin_isfinite(lf);
      const double c = (double)cf, l = (double)lf;
      amax[a] = c + l / 2.0;
      amin[a] = c - l / 2.0;
      avol = a == 0 ? l : avol * l;
    }
    if (sc != sc) myerr |= 1;
    if (!fin) myerr |= 2;
    ok = myerr == 0;                                       // an offending detection is a false positive everywhere
  }
  score[tid] = ok ? sc : __builtin_nanf("");              // NaN: compares false below, so it takes no rank
  for (int i = tid; i < G * T; i += BM_THREADS) win[i] = 0x7fffffff;
  __syncthreads();

  // ---- 1. rank by (-score, column)
  int rank = 0;
  if (ok) {
    for (int j = 0; j < K; ++j) {
      const float s = score[j];
      rank += (s > sc || (s == sc && j < tid)) ? 1 : 0;
    }
  }

  // ---- 2. first maximum of the IoU over the scene's same-class GT rows
  double ov = ninf;
  int jm = -1;
  for (int t0 = 0; t0 < G; t0 += BM_TILE) {
    if (t0) __syncthreads();                               // the previous tile is consumed
    if (tid < BM_TILE) {
      const int g = t0 + tid;
      int okg = 0;
      if (g < G && gvalid[g0 + g]) {
        const float* q = gboxes + (g0 + g) * 6;
        bool fin = true;
        double vol = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float cf = q[a], lf = q[3 + a];
          fin = fin && __builtin_isfinite(cf) && __builtin_isfinite(lf);
          const double c = (double)cf, l = (double)lf;
          gmax[a * BM_TILE + tid] = c + l / 2.0;
          gmin[a * BM_TILE + tid] = c - l / 2.0;
          vol = a == 0 ? l : vol * l;
        }
        gvol[tid] = vol;
        glab[tid] = glabels[g0 + g];
        if (fin) okg = 1;
        else myerr |= 4;                                   // the row is left out of the matching
      }
      gok[tid] = okg;
    }
    __syncthreads();
    if (ok) {
      const int n = min(BM_TILE, G - t0);
      for (int j = 0; j < n; ++j) {
        if (!gok[j] || glab[j] != cls) continue;
        double d[3];
        bool pos = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double bmax = gmax[a * BM_TILE + j], bmin = gmin[a * BM_TILE + j];
          const double min_max = amax[a] < bmax ? amax[a] : bmax;
          const double max_min = amin[a] > bmin ? amin[a] : bmin;
          pos = pos && (min_max > max_min);
          d[a] = min_max - max_min;
        }
        double iou = 0.0;
        if (pos) {
          const double inter = (d[0] * d[1]) * d[2];
          iou = inter / ((avol + gvol[j]) - inter);
        }
        if (iou > ov) {
          ov = iou;
          jm = t0 + j;
        }
      }
    }
  }

  // ---- 3. the winner of every (GT row, threshold): the smallest rank among the detections above the threshold
  unsigned hit = 0;
  if (jm >= 0) {                                           // jm < G <= max_g: inside the table
    for (int t = 0; t < T; ++t) {
      if (ov > thresholds[t]) {
        hit |= 1u << t;
        atomicMin(&win[jm * T + t], rank);
      }
    }
  }
  __syncthreads();
  unsigned fl = 0;
  for (int t = 0; t < T; ++t)
    if (((hit >> t) & 1u) && win[jm * T + t] == rank) fl |= 1u << t;
  if (have) {
    ovmax[k0 + tid] = ov;
    jmax[k0 + tid] = jm;
    flags[k0 + tid] = (uint8_t)fl;
  }
  if (myerr) atomicOr(err, myerr);
}

}  // namespace

extern "C" int pq3d_box_match(const float* pboxes, const int64_t* pclasses, const float* pscores, const uint8_t* pvalid,
                              const int64_t* koff, int64_t NK, const float* gboxes, const int64_t* glabels, const uint8_t* gvalid,
                              const int64_t* goff, int64_t NG, const double* thresholds, int32_t T, int32_t B, int32_t max_g,
                              double* ovmax, int32_t* jmax, uint8_t* flags, int32_t* err, void* stream) {
  PQ_DEVICE_GUARD(stream, err);
  PQ_CHECK_ARG(koff && goff && thresholds && err && B >= 1 && NK >= 0 && NG >= 0, "pq3d_box_match: null pointer or B < 1");
  PQ_CHECK_ARG(NK == 0 || (pboxes && pclasses && pscores && pvalid && ovmax && jmax && flags), "pq3d_box_match: null prediction array");
  PQ_CHECK_ARG(NG == 0 || (gboxes && glabels && gvalid), "pq3d_box_match: null ground-truth array");
  PQ_CHECK_ARG(T >= 1 && T <= PQ3D_BOX_MAX_T && max_g >= 0 && max_g <= PQ3D_BOX_MAX_G,
               "pq3d_box_match: 1 <= T <= PQ3D_BOX_MAX_T, 0 <= max_g <= PQ3D_BOX_MAX_G");
  hipStream_t s = (hipStream_t)stream;
  ZeroList z;
  z.add(err, 1);
  const int e = pq3d_zero_launch(z, s);
  if (e) return e;
  const int lds = BM_FIXED_BYTES + (max_g > 0 ? max_g : 1) * T * 4;
  if (lds > 64 * 1024) {
    static std::atomic<unsigned> done{0};
    if (int e2 = pq3d_enable_big_lds(box_match_kernel, BM_MAX_BYTES, done)) {
      pq3d_set_error(hipGetErrorString((hipError_t)e2));
      return e2;
    }
  }
  hipLaunchKernelGGL(box_match_kernel, dim3((unsigned)B), dim3(BM_THREADS), (size_t)lds, s, pboxes, pclasses, pscores, pvalid, koff,
                     (long)NK, gboxes, glabels, gvalid, goff, (long)NG, thresholds, (int)T, (int)max_g, ovmax, jmax, flags, err);
  PQ_LAUNCH_CHECK();
  return 0;
}
