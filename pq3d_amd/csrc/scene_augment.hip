// Train-time augmentation of instance-segmentation scenes: what the reference's get_scene does per scene on the
// host (data/datasets/sceneverse_instseg.py: centre, random offset, axis flips, volumentations' Scale3d and three
// RotateAroundAxis3d, albumentations' RandomBrightnessContrast and RGBShift, A.Normalize, features = colour | xyz), for a
// batch of ragged scenes in two launches:
//   * aug_stats_kernel: per block of PQ3D_SCENE_AUGMENT_BLOCK points of one scene the fp64 sums and the fp32 minima / maxima
//     of the three axes, by a fixed tree (no floating-point atomics); it also zeroes the error word.
//   * aug_apply_kernel: every workgroup folds the partials of the scenes it touches in index order, derives mean, offset and
//     flip pivot once, then each thread takes 4 consecutive points with 16-byte loads and stores.
// Every arithmetic step of the rule is one fp32 operation in the order of include/pq3d_hip.h (the build has
// -ffp-contract=off and no fast-math); a stage that is off is skipped, not fed a neutral value.
// The scene tables (row offsets, first block of every scene) are host arrays: they travel by value as kernel arguments.
#include "common.h"
#include "ragged.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int AUG_NT = 256;
constexpr int AUG_BLOCK = PQ3D_SCENE_AUGMENT_BLOCK;
constexpr int AUG_ITEMS = AUG_BLOCK / AUG_NT;       // points per thread of the statistics kernel
constexpr int AUG_GROUP = 4;                        // consecutive points per thread of the apply kernel
constexpr int AUG_MAXB = PQ3D_VOXELIZE_MAX_SCENES;
static_assert(sizeof(pq3d_scene_augment_params) == PQ3D_SCENE_AUGMENT_K * sizeof(float), "parameter row");

struct AugScenes : SceneTable<AUG_MAXB> {     // off: points of scene b
  int blk0[AUG_MAXB + 1];          // first statistics block of scene b; blk0[B] = all blocks
};
struct AugColor { float mean255[3], rstd255[3]; };

// workspace: sums [nblk][3] fp64, then minima [nblk][3] and maxima [nblk][3] fp32
PQ_DEV const float* aug_ws_min(const void* ws, int nblk) { return (const float*)((const double*)ws + (long)nblk * 3); }

__global__ __launch_bounds__(AUG_NT) void aug_stats_kernel(const float* __restrict__ xyz, AugScenes sc, int train, void* ws,
                                                           int* __restrict__ err) {
  __shared__ double lsum[AUG_NT / 64][3];
  __shared__ float lmin[AUG_NT / 64][3], lmax[AUG_NT / 64][3];
  if (blockIdx.x == 0 && threadIdx.x == 0) err[0] = 0;
  if (!train) return;                                        // uniform
  const int nblk = sc.blk0[sc.B], blk = blockIdx.x;
  if (blk >= nblk) return;
  const int b = ragged_find(sc.blk0, sc.B, blk);
  const long p0 = sc.off[b] + (long)(blk - sc.blk0[b]) * AUG_BLOCK, p1 = sc.off[b + 1];
  double s[3] = {0.0, 0.0, 0.0};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int j = 0; j < AUG_ITEMS; ++j) {
    const long i = p0 + j * AUG_NT + threadIdx.x;
    if (i < p1) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = xyz[i * 3 + a];
        s[a] += (double)v; lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
      }
    }
  }
  // the fixed tree: butterfly over the wave, then the block's waves in order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s[a] += __shfl_xor(s[a], o, 64);
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
    }
    if (lane == 0) { lsum[wave][a] = s[a]; lmin[wave][a] = lo[a]; lmax[wave][a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    double t = lsum[0][a];
    float mn = lmin[0][a], mx = lmax[0][a];
    for (int w = 1; w < AUG_NT / 64; ++w) { t += lsum[w][a]; mn = fminf(mn, lmin[w][a]); mx = fmaxf(mx, lmax[w][a]); }
    float* fmn = (float*)((double*)ws + (long)nblk * 3);
    ((double*)ws)[(long)blk * 3 + a] = t;
    fmn[(long)blk * 3 + a] = mn;
    fmn[(long)nblk * 3 + (long)blk * 3 + a] = mx;
  }
}

// per scene, in LDS: the parameter row and what the statistics give (mean, offset, flip pivot per axis)
struct AugConst {
  pq3d_scene_augment_params p;
  float mean[3], off[3], cmax[3];
};

PQ_DEV float aug_clip(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }

// one point: x[3] coordinates and c[3] colours in, x[3] augmented coordinates and c[3] normalised colours out; returns error bits
PQ_DEV int aug_point(const AugConst& k, const AugColor& cc, float (&x)[3], float (&c)[3]) {
  int e = 0;
  const pq3d_scene_augment_params& p = k.p;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float v = x[a];
    if (!(fabsf(v) <= FLT_MAX)) e |= 1;
    if (p.on_centre != 0.f) v = v - k.mean[a];
    if (p.on_offset != 0.f) v = v + k.off[a];
    if (a < 2 && p.on_flip != 0.f && p.flip[a] != 0.f) v = k.cmax[a] - v;
    if (p.on_scale != 0.f) v = v * p.scale[a];
    x[a] = v;
  }
  if (p.on_rotate != 0.f) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float* R = p.rot + r * 9;
      const float y0 = (R[0] * x[0] + R[1] * x[1]) + R[2] * x[2];
      const float y1 = (R[3] * x[0] + R[4] * x[1]) + R[5] * x[2];
      const float y2 = (R[6] * x[0] + R[7] * x[1]) + R[8] * x[2];
      x[0] = y0; x[1] = y1; x[2] = y2;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float t = truncf(c[a]);
    if (!(t >= 0.f && t <= 255.f)) { e |= 2; t = t > 255.f ? 255.f : 0.f; }     // (NaN -> 0)
    if (p.on_colour != 0.f) {
      float v = t * p.alpha;
      v = v + p.beta255;
      t = truncf(aug_clip(v));
      t = truncf(aug_clip(t + p.shift[a]));
    }
    c[a] = (t - cc.mean255[a]) * cc.rstd255[a];
  }
  return e;
}

// VEC: the four arrays are 16-byte aligned; a thread's 4 points are then 3 + 3 16-byte loads and 3 + 6 16-byte stores
template <bool VEC>
__global__ __launch_bounds__(AUG_NT) void aug_apply_kernel(const float* xyz, const float* rgb, AugScenes sc,
                                                           const pq3d_scene_augment_params* __restrict__ prm, const void* ws,
                                                           AugColor cc, float* xyz_out, float* feat_out, int* __restrict__ err) {
  __shared__ AugConst kc[AUG_MAXB];
  __shared__ double fsum[AUG_MAXB][3];
  __shared__ float fmn[AUG_MAXB][3], fmx[AUG_MAXB][3];
  const long P = sc.off[sc.B];
  const long g0 = (long)blockIdx.x * (AUG_NT * AUG_GROUP);                 // first point of the workgroup (< P by the grid)
  const long g1 = g0 + AUG_NT * AUG_GROUP < P ? g0 + AUG_NT * AUG_GROUP : P;
  const int b_lo = sc.scene(g0), b_hi = sc.scene(g1 - 1), nsc = b_hi - b_lo + 1;
  const int tid = threadIdx.x;
  // the parameter rows of the workgroup's scenes (zeros = every stage off in evaluation)
  for (int t = tid; t < nsc * PQ3D_SCENE_AUGMENT_K; t += AUG_NT) {
    const int s = t / PQ3D_SCENE_AUGMENT_K, f = t - s * PQ3D_SCENE_AUGMENT_K;
    ((float*)&kc[b_lo + s].p)[f] = prm ? ((const float*)(prm + b_lo + s))[f] : 0.f;
  }
  if (prm) {
    // fold the partials of every scene the workgroup touches, in index order: thread = (scene, {sum, min, max}, axis)
    if (tid < nsc * 9) {
      const int s = tid / 9, r = tid - s * 9, kind = r / 3, a = r - kind * 3, b = b_lo + s;
      const int nblk = sc.blk0[sc.B], k0 = sc.blk0[b], k1 = sc.blk0[b + 1];
      if (kind == 0) {
        const double* q = (const double*)ws;
        double t = q[(long)k0 * 3 + a];
        for (int k = k0 + 1; k < k1; ++k) t += q[(long)k * 3 + a];
        fsum[b][a] = t;
      } else {
        const float* q = aug_ws_min(ws, nblk) + (kind == 2 ? (long)nblk * 3 : 0);
        float t = q[(long)k0 * 3 + a];
        for (int k = k0 + 1; k < k1; ++k) t = kind == 1 ? fminf(t, q[(long)k * 3 + a]) : fmaxf(t, q[(long)k * 3 + a]);
        (kind == 1 ? fmn : fmx)[b][a] = t;
      }
    }
  }
  __syncthreads();
  if (prm && tid < nsc * 3) {
    const int s = tid / 3, a = tid - s * 3, b = b_lo + s;
    AugConst& k = kc[b];
    const bool centre = k.p.on_centre != 0.f, offset = k.p.on_offset != 0.f;
    const float mean = (float)(fsum[b][a] / (double)(sc.off[b + 1] - sc.off[b]));
    const float lo = centre ? fmn[b][a] - mean : fmn[b][a], hi = centre ? fmx[b][a] - mean : fmx[b][a];
    const float off = ((hi - lo) * k.p.u[a] + lo) * 0.5f;
    k.mean[a] = mean; k.off[a] = off; k.cmax[a] = offset ? hi + off : hi;
  }
  __syncthreads();

  const long i0 = g0 + (long)tid * AUG_GROUP;
  if (i0 >= P) return;
  int e = 0;
  const int b0 = sc.scene(i0);
  if (VEC && i0 + AUG_GROUP <= P) {
    float4 xi[3], ci[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { xi[j] = ((const float4*)(xyz + i0 * 3))[j]; ci[j] = ((const float4*)(rgb + i0 * 3))[j]; }
    float* xf = (float*)xi;
    float* cf = (float*)ci;
    const int b3 = sc.scene(i0 + AUG_GROUP - 1);
    float4 fo[6];
    float* ff = (float*)fo;
#pragma unroll
    for (int j = 0; j < AUG_GROUP; ++j) {
      const int b = b3 == b0 ? b0 : sc.scene(i0 + j);            // a group that straddles scenes: every point its own
      float x[3] = {xf[j * 3], xf[j * 3 + 1], xf[j * 3 + 2]}, c[3] = {cf[j * 3], cf[j * 3 + 1], cf[j * 3 + 2]};
      e |= aug_point(kc[b], cc, x, c);
#pragma unroll
      for (int a = 0; a < 3; ++a) { xf[j * 3 + a] = x[a]; ff[j * 6 + a] = c[a]; ff[j * 6 + 3 + a] = x[a]; }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) ((float4*)(xyz_out + i0 * 3))[j] = xi[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) ((float4*)(feat_out + i0 * 6))[j] = fo[j];
  } else {
    for (long i = i0; i < i0 + AUG_GROUP && i < P; ++i) {        // the batch's tail, or unaligned arrays: point by point
      const int b = sc.scene(i);
      float x[3] = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]}, c[3] = {rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2]};
      e |= aug_point(kc[b], cc, x, c);
#pragma unroll
      for (int a = 0; a < 3; ++a) { xyz_out[i * 3 + a] = x[a]; feat_out[i * 6 + a] = c[a]; feat_out[i * 6 + 3 + a] = x[a]; }
    }
  }
  if (e) atomicOr(err, e);       // (integer OR: the word does not depend on the order)
}

// host: scene table from the caller's offsets; "" or an argument error text
std::string aug_table(const int64_t* offsets, int B, AugScenes& sc) {
  const std::string e = scene_table_fill(sc, offsets, B, PQ3D_VOXELIZE_MAX_POINTS, PQ3D_VOXELIZE_MAX_POINTS, "pq3d_scene_augment");
  if (!e.empty()) return e;
  int blk = 0;
  for (int b = 0; b <= AUG_MAXB; ++b) {
    sc.blk0[b] = blk;
    if (b < B) blk += (int)((sc.off[b + 1] - sc.off[b] + AUG_BLOCK - 1) / AUG_BLOCK);
  }
  return e;
}

long long aug_ws_bytes(const AugScenes& sc) { return (long long)sc.blk0[sc.B] * (3 * 8 + 6 * 4); }

}  // namespace

extern "C" int64_t pq3d_scene_augment_ws_bytes(const int64_t* offsets, int32_t B) {
  AugScenes sc;
  const std::string e = aug_table(offsets, B, sc);
  if (!e.empty()) { pq3d_set_error(e.c_str()); return -1; }
  return aug_ws_bytes(sc);
}

extern "C" int pq3d_scene_augment_stats(const float* coordinates, const int64_t* offsets, int32_t B, int32_t train, void* ws,
                                        int64_t ws_bytes, int32_t* err, void* stream) {
  PQ_DEVICE_GUARD(stream, coordinates);
  PQ_CHECK_ARG(coordinates && err, "pq3d_scene_augment_stats: null pointer");
  AugScenes sc;
  const std::string e = aug_table(offsets, B, sc);
  PQ_CHECK_ARG(e.empty(), e.c_str());
  if (train) {
    PQ_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= aug_ws_bytes(sc),
                 "pq3d_scene_augment_stats: workspace missing, unaligned or smaller than pq3d_scene_augment_ws_bytes");
  }
  hipLaunchKernelGGL(aug_stats_kernel, dim3(train ? (unsigned)sc.blk0[B] : 1u), dim3(AUG_NT), 0, (hipStream_t)stream, coordinates, sc,
                     (int)train, ws, err);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_scene_augment_apply(const float* coordinates, const float* colors, const int64_t* offsets, int32_t B,
                                        const float* params, const void* ws, int64_t ws_bytes, const float* color_consts,
                                        float* coordinates_out, float* features_out, int32_t* err, void* stream) {
  PQ_DEVICE_GUARD(stream, coordinates);
  PQ_CHECK_ARG(coordinates && colors && color_consts && coordinates_out && features_out && err, "pq3d_scene_augment_apply: null pointer");
  AugScenes sc;
  const std::string e = aug_table(offsets, B, sc);
  PQ_CHECK_ARG(e.empty(), e.c_str());
  if (params) {
    PQ_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= aug_ws_bytes(sc),
                 "pq3d_scene_augment_apply: workspace missing, unaligned or smaller than pq3d_scene_augment_ws_bytes");
    PQ_CHECK_ARG(((uintptr_t)params & 3) == 0, "pq3d_scene_augment_apply: params must be 4-byte aligned");
  }
  AugColor cc;
  for (int a = 0; a < 3; ++a) { cc.mean255[a] = color_consts[a]; cc.rstd255[a] = color_consts[3 + a]; }
  const long P = (long)sc.off[B];
  const unsigned grid = (unsigned)((P + AUG_NT * AUG_GROUP - 1) / (AUG_NT * AUG_GROUP));
  const bool vec = (((uintptr_t)coordinates | (uintptr_t)colors | (uintptr_t)coordinates_out | (uintptr_t)features_out) & 15) == 0;
  const pq3d_scene_augment_params* prm = (const pq3d_scene_augment_params*)params;
  if (vec)
    hipLaunchKernelGGL(aug_apply_kernel<true>, dim3(grid), dim3(AUG_NT), 0, (hipStream_t)stream, coordinates, colors, sc, prm, ws, cc,
                       coordinates_out, features_out, err);
  else
    hipLaunchKernelGGL(aug_apply_kernel<false>, dim3(grid), dim3(AUG_NT), 0, (hipStream_t)stream, coordinates, colors, sc, prm, ws, cc,
                       coordinates_out, features_out, err);
  PQ_LAUNCH_CHECK();
  return 0;
}
