// The batch-statistics BatchNorm row arithmetic, written once: sparse_conv_bwd.hip (pq3d_bn_apply, pq3d_bn_bwd_*: a dense
// upstream gradient) and pointnet2_train.hip (pq3d_bn_relu_maxpool, pq3d_bn_pool_bwd_*: the gradient of a max over samples,
// never materialised) include these, so the pooled forms equal the dense ones bit for bit
// (tests/test_gpu_pointnetpp_train.py).  The order of every sum and product is part of that contract.
//   bn_affine           the normalised value of one element
//   DenseGrad/PoolGrad  where the backward takes g[r, c] from: dy (masked by the ReLU output y) or the pooled gradient
//   bn_bwd_*_kernel     column reductions: block (32 columns x 8 row lanes), grid (P row blocks, ceil(C / 32)).  Row block p owns
//                       rows [p rpb, (p + 1) rpb); thread (col, rl) walks rows rl, rl + 8, ... of it; the 8 row lanes are combined
//                       in lane order by thread rl = 0; the P partials are combined in block order by the finalize kernel.
#pragma once
#include "common.h"

namespace {

constexpr int BN_CW = 32, BN_RL = 8, BN_MAXP = 256;

__host__ __device__ inline long bn_blocks(long N) {
  long P = (N + 63) / 64;
  return P < 1 ? 1 : P > BN_MAXP ? BN_MAXP : P;
}

inline unsigned ew_grid(long total) {
  long gsz = (total + 255) / 256;
  return (unsigned)(gsz > 16384 ? 16384 : gsz < 1 ? 1 : gsz);
}

PQ_DEV float bn_affine(float z, float mean, float rstd, float gamma, float beta) { return (z - mean) * rstd * gamma + beta; }

// g[r, c] = dy[r, c], zeroed where the ReLU output y (optional) is not positive
struct DenseGrad {
  const float* dy; long lddy;
  const float* y; long ldy;
  PQ_DEV float operator()(long r, int c) const {
    float gv = dy[r * lddy + c];
    if (y && !(y[r * ldy + c] > 0.f)) gv = 0.f;
    return gv;
  }
};

// rows r = g ns + s of group g: g[r, c] = gp[g, c] where sample s attained the (positive) maximum, else 0
struct PoolGrad {
  const float* gp;
  const float* pooled;
  const int32_t* arg;
  int ns, C;
  PQ_DEV float operator()(long r, int c) const {
    const long g = r / ns, e = g * C + c;
    const int s = (int)(r - g * ns);
    return (arg[e] == s && pooled[e] > 0.f) ? gp[e] : 0.f;
  }
};

template <typename Grad>
__global__ __launch_bounds__(BN_CW * BN_RL) void bn_bwd_partial_kernel(const Grad grad, const float* __restrict__ z, long ldz, long N,
                                                                       int C, const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd, float* __restrict__ part) {
  __shared__ float sh[2][BN_RL][BN_CW];
  const int col = threadIdx.x & (BN_CW - 1), rl = threadIdx.x / BN_CW, c = blockIdx.y * BN_CW + col;
  const long P = gridDim.x, rpb = (N + P - 1) / P, r0 = (long)blockIdx.x * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
  float sg = 0.f, sgx = 0.f;
  if (c < C) {
    const float m = mean[c], rs = rstd[c];
    for (long r = r0 + rl; r < r1; r += BN_RL) {
      const float gv = grad(r, c);
      sg += gv;
      sgx += gv * ((z[r * ldz + c] - m) * rs);
    }
  }
  sh[0][rl][col] = sg; sh[1][rl][col] = sgx;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int j = 1; j < BN_RL; ++j) { sg += sh[0][j][col]; sgx += sh[1][j][col]; }
    float* p = part + ((long)blockIdx.x * C + c) * 2;
    p[0] = sg; p[1] = sgx;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ part, int P, int C, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float sg = 0.f, sgx = 0.f;
  for (int p = 0; p < P; ++p) {
    sg += part[((long)p * C + c) * 2];
    sgx += part[((long)p * C + c) * 2 + 1];
  }
  dbeta[c] = sg;
  dgamma[c] = sgx;
}

template <typename Grad>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const Grad grad, const float* __restrict__ z, long ldz, long N, int C,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                           const float* __restrict__ dbeta, float* __restrict__ dz, long lddz,
                                                           float* dres, long lddres, int dres_add) {
  const long total = N * C;
  const float inv_n = 1.f / (float)N;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / C;
    const int c = (int)(e - r * C);
    const float gv = grad(r, c);
    const float rs = rstd[c], xh = (z[r * ldz + c] - mean[c]) * rs;
    dz[r * lddz + c] = gamma[c] * rs * (gv - dbeta[c] * inv_n - xh * (dgamma[c] * inv_n));
    if (dres) {
      float* p = dres + r * lddres + c;
      *p = dres_add ? *p + gv : gv;
    }
  }
}

// the two launches of a backward reduction / the one of its apply, for either gradient source
template <typename Grad>
inline void bn_bwd_reduce_launch(const Grad& grad, const float* z, long ldz, long N, int C, const float* mean, const float* rstd,
                                 float* dgamma, float* dbeta, float* part, hipStream_t s) {
  const long P = bn_blocks(N);
  hipLaunchKernelGGL(bn_bwd_partial_kernel<Grad>, dim3((unsigned)P, (unsigned)((C + BN_CW - 1) / BN_CW)), dim3(BN_CW * BN_RL), 0, s,
                     grad, z, ldz, N, C, mean, rstd, part);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const float*)part, (int)P, C, dgamma,
                     dbeta);
}

template <typename Grad>
inline void bn_bwd_apply_launch(const Grad& grad, const float* z, long ldz, long N, int C, const float* mean, const float* rstd,
                                const float* gamma, const float* dgamma, const float* dbeta, float* dz, long lddz, float* dres,
                                long lddres, int dres_add, hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_apply_kernel<Grad>, dim3(ew_grid(N * C)), dim3(256), 0, s, grad, z, ldz, N, C, mean, rstd, gamma, dgamma,
                     dbeta, dz, lddz, dres, lddres, dres_add);
}

}  // namespace
