// Training the PointNet++ set abstraction (pq3d_amd/pointnetpp.py: PointNetPP(trainable=True)).  Definition in
// include/pq3d_hip.h.  Rows are fp32, channels last, in pq3d_group_rows' order: row r = (b np + p) ns + s.
//   pq3d_bn_relu_maxpool   the last SharedMLP layer of a stage: pooled[g, c] = max_s relu(bn(z[g ns + s, c])) and the FIRST
//                          sample that attains it; the normalised rows are never written.  One thread per (group, channel),
//                          consecutive threads on consecutive channels: every load is a coalesced row segment.
//   pq3d_bn_pool_bwd_*     BatchNorm backward of that layer from the pooled gradient: bn_row.h's reduction and apply bodies with
//                          PoolGrad as the gradient source -- the same row blocks and lane order as pq3d_bn_bwd_*, so the pair equals
//                          the dense pair fed the scattered gradient bit for bit; no [G ns, C] gradient exists.
//   pq3d_group_rows_bwd    gradient of the grouping with respect to the point features.  One workgroup per cloud: a histogram of
//                          the np ns entries by source point (integer LDS atomics), an exclusive scan, then a STABLE placement --
//                          wave w walks all entries in order, 64 per step, and places those whose point is its own
//                          (point mod waves == w); lanes naming the same point are ranked by a ballot, so no two waves touch
//                          one cursor and every point's list is in increasing entry order.  Then one thread per (point, channel)
//                          adds its list front to back: no floating-point atomics, the same bits every run.
#include "bn_row.h"

namespace {

__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* __restrict__ z, long ldz, long G, int ns, int C,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ pooled, int32_t* __restrict__ arg) {
  const long total = G * C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long g = e / C;
    const int c = (int)(e - g * C);
    const float m = mean[c], rs = rstd[c], ga = gamma[c], be = beta[c];
    const float* zp = z + g * ns * ldz + c;
    float best = fmaxf(bn_affine(zp[0], m, rs, ga, be), 0.f);
    int at = 0;
    for (int s = 1; s < ns; ++s) {
      const float y = fmaxf(bn_affine(zp[(long)s * ldz], m, rs, ga, be), 0.f);
      if (y > best) { best = y; at = s; }      // strict: the first maximum stays (F.max_pool2d)
    }
    pooled[e] = best;
    arg[e] = at;
  }
}

constexpr int GB_THREADS = 256, GB_WAVES = GB_THREADS / 64;

// LDS: pos[N] int32 (histogram -> list start -> list end), list[E] uint16 (entry ids by point), tot[GB_THREADS] int32
__global__ __launch_bounds__(GB_THREADS) void group_rows_bwd_kernel(const float* __restrict__ drows, long ldr, int col_off,
                                                                    const int32_t* __restrict__ idx, float* __restrict__ dfeats,
                                                                    long ldf, int N, int C, int E) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
  int* pos = (int*)gb_smem;
  int* tot = pos + N;
  unsigned short* list = (unsigned short*)(tot + GB_THREADS);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* ix = idx + (long)b * E;
  for (int j = tid; j < N; j += GB_THREADS) pos[j] = 0;
  __syncthreads();
  for (int e = tid; e < E; e += GB_THREADS) {
    const int j = ix[e];
    if (j >= 0 && j < N) atomicAdd(&pos[j], 1);        // integer counts; an index outside the cloud names nobody
  }
  __syncthreads();
  // exclusive scan: thread t owns points [t per, (t + 1) per)
  const int per = (N + GB_THREADS - 1) / GB_THREADS, j0 = tid * per, j1 = min(j0 + per, N);
  int sum = 0;
  for (int j = j0; j < j1; ++j) sum += pos[j];
  tot[tid] = sum;
  __syncthreads();
  for (int o = 1; o < GB_THREADS; o <<= 1) {
    const int v = tid >= o ? tot[tid - o] : 0;
    __syncthreads();
    tot[tid] += v;
    __syncthreads();
  }
  int run = tot[tid] - sum;
  for (int j = j0; j < j1; ++j) {
    const int cnt = pos[j];
    pos[j] = run;
    run += cnt;
  }
  __syncthreads();
  // stable placement: this wave owns the points j with j % GB_WAVES == wave
  for (int e0 = 0; e0 < E; e0 += 64) {
    const int e = e0 + lane;
    const int j = e < E ? ix[e] : -1;
    const bool mine = j >= 0 && j < N && (j & (GB_WAVES - 1)) == wave;
    unsigned long long todo = __ballot(mine);
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int jl = __shfl(j, lead, 64);
      const bool same = mine && j == jl;
      const unsigned long long m = __ballot(same);
      const int base = pos[jl];
      if (same) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)e;
      if (lane == lead) pos[jl] = base + __popcll(m);
      __threadfence_block();                          // the next step of this wave reads the cursor it just moved
      todo &= ~m;
    }
  }
  __syncthreads();
  // pos[j] is now the END of point j's list, pos[j - 1] its start
  const float* src = drows + (long)b * E * ldr + col_off;
  float* dst = dfeats + (long)b * N * ldf;
  for (int w = tid; w < N * C; w += GB_THREADS) {
    const int j = w / C, c = w - j * C;
    float a = 0.f;
    for (int t = j ? pos[j - 1] : 0; t < pos[j]; ++t) a += src[(long)list[t] * ldr + c];
    dst[(long)j * ldf + c] = a;
  }
}

// GroupAll: sample s of the one group IS point s
__global__ __launch_bounds__(256) void group_all_bwd_kernel(const float* __restrict__ drows, long ldr, int col_off,
                                                            float* __restrict__ dfeats, long ldf, long rows, int C) {
  const long total = rows * C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / C;
    const int c = (int)(e - r * C);
    dfeats[r * ldf + c] = drows[r * ldr + col_off + c];
  }
}

}  // namespace

#define POOL_COMMON(name)                                                                                                   \
  PQ_CHECK_ARG(G >= 1 && ns >= 1 && C >= 1 && C <= 65535 * BN_CW && G <= (1LL << 40) / ns, name ": G >= 1, ns >= 1 and C >= 1 are required"); \
  PQ_CHECK_ARG(ldz >= C, name ": ldz >= C is required")

extern "C" int pq3d_bn_relu_maxpool(const float* z, int64_t ldz, int64_t G, int32_t ns, int32_t C, const float* mean,
                                    const float* rstd, const float* gamma, const float* beta, float* pooled, int32_t* arg,
                                    void* stream) {
  PQ_DEVICE_GUARD(stream, z);
  POOL_COMMON("pq3d_bn_relu_maxpool");
  PQ_CHECK_ARG(z && mean && rstd && gamma && beta && pooled && arg,
               "pq3d_bn_relu_maxpool: z, mean, rstd, gamma, beta, pooled and arg are required");
  hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(ew_grid((long)G * C)), dim3(256), 0, (hipStream_t)stream, z, (long)ldz, (long)G,
                     (int)ns, (int)C, mean, rstd, gamma, beta, pooled, arg);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_bn_pool_bwd_reduce(const float* gp, const float* pooled, const int32_t* arg, const float* z, int64_t ldz,
                                       int64_t G, int32_t ns, int32_t C, const float* mean, const float* rstd, float* dgamma,
                                       float* dbeta, float* part, void* stream) {
  PQ_DEVICE_GUARD(stream, gp);
  POOL_COMMON("pq3d_bn_pool_bwd_reduce");
  PQ_CHECK_ARG(gp && pooled && arg && z && mean && rstd && dgamma && dbeta && part,
               "pq3d_bn_pool_bwd_reduce: gp, pooled, arg, z, mean, rstd, dgamma, dbeta and part are required");
  const PoolGrad grad = {gp, pooled, arg, (int)ns, (int)C};
  bn_bwd_reduce_launch(grad, z, (long)ldz, (long)G * ns, (int)C, mean, rstd, dgamma, dbeta, part, (hipStream_t)stream);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_bn_pool_bwd_apply(const float* gp, const float* pooled, const int32_t* arg, const float* z, int64_t ldz,
                                      int64_t G, int32_t ns, int32_t C, const float* mean, const float* rstd, const float* gamma,
                                      const float* dgamma, const float* dbeta, float* dz, int64_t lddz, void* stream) {
  PQ_DEVICE_GUARD(stream, gp);
  POOL_COMMON("pq3d_bn_pool_bwd_apply");
  PQ_CHECK_ARG(gp && pooled && arg && z && mean && rstd && gamma && dgamma && dbeta && dz,
               "pq3d_bn_pool_bwd_apply: gp, pooled, arg, z, mean, rstd, gamma, dgamma, dbeta and dz are required");
  PQ_CHECK_ARG(lddz >= C, "pq3d_bn_pool_bwd_apply: lddz >= C is required");
  const PoolGrad grad = {gp, pooled, arg, (int)ns, (int)C};
  bn_bwd_apply_launch(grad, z, (long)ldz, (long)G * ns, (int)C, mean, rstd, gamma, dgamma, dbeta, dz, (long)lddz, (float*)nullptr, 0L,
                      0, (hipStream_t)stream);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_group_rows_bwd(const float* drows, int64_t ldr, int32_t col_off, const int32_t* idx, float* dfeats, int64_t ldf,
                                   int32_t B, int32_t N, int32_t C, int32_t np, int32_t ns, void* stream) {
  PQ_DEVICE_GUARD(stream, drows);
  PQ_CHECK_ARG(drows && dfeats && B >= 0 && N >= 1 && C >= 1 && np >= 1 && ns >= 1 && col_off >= 0,
               "pq3d_group_rows_bwd: drows and dfeats are required, B >= 0, N, C, np, ns >= 1, col_off >= 0");
  PQ_CHECK_ARG(ldr >= (int64_t)col_off + C && ldf >= C, "pq3d_group_rows_bwd: leading dimensions too small (ldr >= col_off + C, ldf >= C)");
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (!idx) {
    PQ_CHECK_ARG(np == 1 && ns == N, "pq3d_group_rows_bwd: without indices every point is a sample of one group (np == 1, ns == N)");
    const long rows = (long)B * N;
    hipLaunchKernelGGL(group_all_bwd_kernel, dim3(ew_grid(rows * C)), dim3(256), 0, s, drows, (long)ldr, (int)col_off, dfeats, (long)ldf,
                       rows, (int)C);
    PQ_LAUNCH_CHECK();
    return 0;
  }
  const int64_t E = (int64_t)np * ns;
  PQ_CHECK_ARG(N <= PQ3D_GROUP_BWD_MAX_POINTS && E <= PQ3D_GROUP_BWD_MAX_ENTRIES,
               "pq3d_group_rows_bwd: at most PQ3D_GROUP_BWD_MAX_POINTS points and PQ3D_GROUP_BWD_MAX_ENTRIES (np * ns) entries per cloud");
  PQ_CHECK_ARG((int64_t)N * C <= 0x7fffffffLL, "pq3d_group_rows_bwd: N * C too large");
  const size_t lds = ((size_t)N + GB_THREADS) * 4 + (size_t)E * 2;
  static std::atomic<unsigned> done{0};
  if (int e = pq3d_enable_big_lds(group_rows_bwd_kernel, 160 * 1024, done)) { pq3d_set_error(hipGetErrorString((hipError_t)e)); return e; }
  hipLaunchKernelGGL(group_rows_bwd_kernel, dim3((unsigned)B), dim3(GB_THREADS), lds, s, drows, (long)ldr, (int)col_off, idx, dfeats,
                     (long)ldf, (int)N, (int)C, (int)E);
  PQ_LAUNCH_CHECK();
  return 0;
}
