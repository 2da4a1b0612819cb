// Backward of the sparse 3-D convolutions and batch-statistics BatchNorm of the voxel backbone (pq3d_amd/sparse.py).
// Definition in include/pq3d_hip.h.  The input gradient is the forward kernel on the transposed map (sparse_conv.hip, wmode).
//   pq3d_sparse_conv_wgrad  dW[k, c, n] = sum_o x[nbr[o, k], c] dy[o, n].  A workgroup (4 waves) owns offset k, 32 input
//                           channels, 64 output channels and one chunk of consecutive 64-row tiles.  Per tile whose occupancy
//                           bit k is set: the 64 x rows are gathered by index and the 64 dy rows read directly, through
//                           registers (the fp32 -> bf16 conversion rides on the staging) into [channel][row] LDS images --
//                           the contraction runs over rows, so both MFMA fragments want 16 bytes of consecutive ROWS per
//                           lane.  Staging lane = row, so a wave's 64 lanes write 64 consecutive LDS words (no bank
//                           conflict) and read 32 bytes of 64 different rows.  The 2 x 4 sub-tiles of 16 x 16 are dealt two
//                           per wave; accumulators stay in registers over the chunk and every element is stored once: into
//                           dW when there is one chunk, else into slab s of the workspace, which wgrad_sum_kernel adds in
//                           chunk order.  No atomics; for a given number of chunks the bits are reproducible.
//                           ct = BF16 carries the fp32 x as TWO bf16 planes (hi = bf16(x), lo = bf16(x - hi); a second MFMA
//                           per step against the same dy fragment) and rounds only dy: an offset with one present pair is a
//                           ONE-term sum, and with both operands rounded (2^-8 relative each) such an element misses
//                           2^-8 |x| |dy| -- measured: 9 % of the elements of a one-row map -- with x exact it cannot.
//                           Sizing: the fine levels are a 32 x 32 .. 96 x 128 tile per offset over 10^4 - 10^5 rows (27 - 162
//                           workgroups without a row split: the split fills the chip); the coarse levels 27 x 8 x 4 = 864
//                           workgroups over ~10^3 rows (no split needed).
//   pq3d_bn_*               per-channel statistics / normalisation / their backward over the rows of a level: memory-bound
//                           column reductions in a fixed order (per-block partials, combined in block order) and elementwise
//                           passes; every row pointer has a leading dimension.
#include "bn_row.h"
#include "common.h"

namespace {

constexpr int WG_T = PQ3D_SPARSE_TILE, WG_CM = 32, WG_CN = 64, WG_THREADS = 256, WG_MAX_SPLITS = 4096;

template <typename CT>
__global__ __launch_bounds__(WG_THREADS) void sparse_wgrad_kernel(const pq3d_sparse_wgrad_desc d, const int S, const int ntn) {
  constexpr int EPL = Mma<CT>::EPL, KSTEP = Mma<CT>::KSTEP;
  constexpr int LDR = WG_T + 16 / (int)sizeof(CT);    // LDS row: 64 rows of the tile + 16 bytes
  __shared__ __attribute__((aligned(16))) CT Xs[WG_CM * LDR];
  __shared__ __attribute__((aligned(16))) CT Ys[WG_CN * LDR];
  constexpr bool SPLIT = sizeof(CT) == 2;             // bf16: x rides as two bf16 planes, x = hi + lo (see the top)
  __shared__ __attribute__((aligned(16))) CT Xl[SPLIT ? WG_CM * LDR : 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int K = d.K, Cin = d.Cin, Cout = d.Cout;
  const int k = blockIdx.y, s = blockIdx.z;
  const int ct_ = blockIdx.x / ntn, nt_ = blockIdx.x - ct_ * ntn;
  const int c0 = ct_ * WG_CM, n0 = nt_ * WG_CN;
  const long tiles = ((long)d.N_out + WG_T - 1) / WG_T, per = (tiles + S - 1) / S;
  const long t0 = (long)s * per, t1 = t0 + per < tiles ? t0 + per : tiles;
  const int msub = wave & 1, nsub = (wave >> 1) * 2;  // this wave's sub-tiles: channels 16 msub .., columns 16 (nsub + {0, 1}) ..
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (long t = t0; t < t1; ++t) {
    if (d.occ && k < 128 && !((d.occ[t * 4 + (k >> 5)] >> (k & 31)) & 1u)) continue;   // uniform: offset k absent from the tile
    const long o = t * WG_T + lane;
    int ix = -1;
    if (o < d.N_out) {
      ix = d.nbr[o * K + k];
      if (ix < 0 || ix >= d.N_in) ix = -1;
    }
    // ---- x rows (gathered) -> Xs[c][row]: wave w stages channels c0 + 8 w .. + 7 of the 64 rows
    {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
      const int c = c0 + wave * 8;
      if (ix >= 0 && c < Cin) load_elems<8>(d.x, PQ3D_F32, (long)ix * d.ldx + c, Cin - c, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const CT hi = Cvt<CT>::from(v[j]);
        Xs[(wave * 8 + j) * LDR + lane] = hi;
        if (SPLIT) Xl[(wave * 8 + j) * LDR + lane] = Cvt<CT>::from(v[j] - Cvt<CT>::to(hi));
      }
    }
    // ---- dy rows -> Ys[n][row]: wave w stages columns n0 + 16 w .. + 15 (zeros for a row whose offset k is absent)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
      const int nn = wave * 16 + h * 8, n = n0 + nn;
      if (ix >= 0 && n < Cout) load_elems<8>(d.dy, PQ3D_F32, o * d.ldy + n, Cout - n, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) Ys[(nn + j) * LDR + lane] = Cvt<CT>::from(v[j]);
    }
    __syncthreads();
#pragma unroll
    for (int st = 0; st < WG_T / KSTEP; ++st) {
      const u32x4 a = *(const u32x4*)&Xs[(msub * 16 + i) * LDR + st * KSTEP + g * EPL];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const u32x4 b = *(const u32x4*)&Ys[((nsub + q) * 16 + i) * LDR + st * KSTEP + g * EPL];
        Mma<CT>::mma(acc[q], a, b);
        if (SPLIT) {
          const u32x4 al = *(const u32x4*)&Xl[(msub * 16 + i) * LDR + st * KSTEP + g * EPL];
          Mma<CT>::mma(acc[q], al, b);
        }
      }
    }
    __syncthreads();
  }
  // ---- store: lane holds channels c0 + 16 msub + 4 g + r (r = 0..3) of column n0 + 16 (nsub + q) + i
  float* dst = S > 1 ? d.ws + (long)s * K * Cin * Cout : d.dW;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int n = n0 + (nsub + q) * 16 + i;
    if (n >= Cout) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + msub * 16 + 4 * g + r;
      if (c < Cin) dst[((long)k * Cin + c) * Cout + n] = acc[q][r];
    }
  }
}

// dW[e] = ws[0][e] + ws[1][e] + ... in chunk order
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dW, long E, int S) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long)gridDim.x * 256) {
    float a = ws[e];
    for (int s = 1; s < S; ++s) a += ws[(long)s * E + e];
    dW[e] = a;
  }
}

int wgrad_splits(long N_out, int Cin, int Cout, int K, int splits) {
  if (splits < 0 || splits > WG_MAX_SPLITS || N_out < 0 || Cin < 1 || Cout < 1 || K < 1) return -1;
  if (splits) return splits;
  const long tiles = (N_out + WG_T - 1) / WG_T;
  const long base = (long)K * ((Cin + WG_CM - 1) / WG_CM) * ((Cout + WG_CN - 1) / WG_CN);
  long S = (1024 + base - 1) / base;          // ~4 workgroups per CU over the launch
  const long cap = (tiles + 3) / 4;           // a chunk keeps at least 4 row tiles: its store is amortised
  if (S > cap) S = cap;
  if (S > 256) S = 256;
  return S < 1 ? 1 : (int)S;
}

// ---- batch-statistics BatchNorm -----------------------------------------------------------------------------------------
// The column-reduction layout, the element expression and the backward bodies are bn_row.h's (shared with pointnet2_train.hip).
PQ_DEV void chan(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  const float nt = n + nb, dl = mb - mean;
  mean += dl * (nb / nt);
  m2 += m2b + dl * dl * (n * nb / nt);
  n = nt;
}

__global__ __launch_bounds__(BN_CW * BN_RL) void bn_stats_partial_kernel(const float* __restrict__ z, long ldz, long N, int C,
                                                                         float* __restrict__ part) {
  __shared__ float sh[3][BN_RL][BN_CW];
  const int col = threadIdx.x & (BN_CW - 1), rl = threadIdx.x / BN_CW, c = blockIdx.y * BN_CW + col;
  const long P = gridDim.x, rpb = (N + P - 1) / P, r0 = (long)blockIdx.x * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
  float cnt = 0.f, s1 = 0.f, s2 = 0.f, shift = 0.f;
  if (c < C && r0 < r1) {
    shift = z[r0 * ldz + c];     // a value of the data: the sums below are of the size of the spread, not of the mean
    for (long r = r0 + rl; r < r1; r += BN_RL) {
      const float v = z[r * ldz + c] - shift;
      s1 += v;
      s2 += v * v;
      cnt += 1.f;
    }
  }
  float mean = 0.f, m2 = 0.f;
  if (cnt > 0.f) {
    const float dm = s1 / cnt;
    mean = shift + dm;
    m2 = fmaxf(s2 - s1 * dm, 0.f);
  }
  sh[0][rl][col] = cnt; sh[1][rl][col] = mean; sh[2][rl][col] = m2;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int j = 1; j < BN_RL; ++j) chan(cnt, mean, m2, sh[0][j][col], sh[1][j][col], sh[2][j][col]);
    float* p = part + ((long)blockIdx.x * C + c) * 3;
    p[0] = cnt; p[1] = mean; p[2] = m2;
  }
}

__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ part, int P, long N, int C, float eps,
                                                             float momentum, float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                             float* running_mean, float* running_var, int64_t* nbt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int p = 0; p < P; ++p) {
    const float* q = part + ((long)p * C + c) * 3;
    chan(n, mean, m2, q[0], q[1], q[2]);
  }
  const float var = m2 / (float)N;
  mean_o[c] = mean;
  rstd_o[c] = 1.f / sqrtf(var + eps);
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
  if (running_var) {
    const float unb = N > 1 ? m2 / (float)(N - 1) : var;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unb;
  }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, long ldz, long N, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ residual, long ldr, int act,
                                                       float* __restrict__ out, long ldo, int col_off) {
  const long total = N * C;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / C;
    const int c = (int)(e - r * C);
    float y = bn_affine(z[r * ldz + c], mean[c], rstd[c], gamma[c], beta[c]);
    if (residual) y += residual[r * ldr + c];
    if (act == PQ3D_ACT_RELU) y = fmaxf(y, 0.f);
    out[r * ldo + col_off + c] = y;
  }
}

}  // namespace

extern "C" int32_t pq3d_sparse_conv_wgrad_splits(int64_t N_out, int32_t Cin, int32_t Cout, int32_t K, int32_t splits) {
  return wgrad_splits((long)N_out, Cin, Cout, K, splits);
}

extern "C" int64_t pq3d_sparse_conv_wgrad_ws_bytes(int64_t N_out, int32_t Cin, int32_t Cout, int32_t K, int32_t splits) {
  const int S = wgrad_splits((long)N_out, Cin, Cout, K, splits);
  if (S < 0) return -1;
  return S > 1 ? (int64_t)S * K * Cin * Cout * 4 : 0;
}

extern "C" int pq3d_sparse_conv_wgrad(const pq3d_sparse_wgrad_desc* dp, void* stream) {
  PQ_CHECK_ARG(dp, "pq3d_sparse_conv_wgrad: null descriptor");
  const pq3d_sparse_wgrad_desc& d = *dp;
  PQ_DEVICE_GUARD(stream, d.dW);
  PQ_CHECK_ARG(d.N_out >= 0 && d.N_in >= 0 && d.Cin >= 1 && d.Cout >= 1 && d.K >= 1, "pq3d_sparse_conv_wgrad: bad sizes");
  PQ_CHECK_ARG(d.ct == PQ3D_F32 || d.ct == PQ3D_BF16, "pq3d_sparse_conv_wgrad: ct must be PQ3D_F32 or PQ3D_BF16");
  PQ_CHECK_ARG(d.ldx >= d.Cin && d.ldy >= d.Cout, "pq3d_sparse_conv_wgrad: leading dimensions too small (ldx >= Cin, ldy >= Cout)");
  PQ_CHECK_ARG(!d.occ || d.K <= 128, "pq3d_sparse_conv_wgrad: occupancy words cover K <= 128 offsets");
  PQ_CHECK_ARG(d.K <= 65535 && (int64_t)d.K * d.Cin * d.Cout <= (1LL << 40), "pq3d_sparse_conv_wgrad: K or K * Cin * Cout too large");
  const int S = wgrad_splits(d.N_out, d.Cin, d.Cout, d.K, d.splits);
  PQ_CHECK_ARG(S >= 1, "pq3d_sparse_conv_wgrad: splits must be 0 (chosen from the sizes) or 1 .. 4096");
  PQ_CHECK_ARG(d.dW && (d.N_out == 0 || (d.x && d.nbr && d.dy)), "pq3d_sparse_conv_wgrad: x, nbr, dy and dW are required");
  const int64_t need = S > 1 ? (int64_t)S * d.K * d.Cin * d.Cout * 4 : 0;
  PQ_CHECK_ARG(need == 0 || (d.ws && d.ws_bytes >= need),
               "pq3d_sparse_conv_wgrad: workspace too small (pq3d_sparse_conv_wgrad_ws_bytes gives the size)");
  PQ_CHECK_ARG((((uintptr_t)d.x | (uintptr_t)d.dy | (uintptr_t)d.dW) & 3) == 0 && (((uintptr_t)d.ws) & 15) == 0,
               "pq3d_sparse_conv_wgrad: misaligned pointer");
  const int ntc = (d.Cin + WG_CM - 1) / WG_CM, ntn = (d.Cout + WG_CN - 1) / WG_CN;
  const dim3 grid((unsigned)(ntc * ntn), (unsigned)d.K, (unsigned)S);
  hipStream_t s = (hipStream_t)stream;
  if (d.ct == PQ3D_BF16) hipLaunchKernelGGL((sparse_wgrad_kernel<bf16_t>), grid, dim3(WG_THREADS), 0, s, d, S, ntn);
  else hipLaunchKernelGGL((sparse_wgrad_kernel<float>), grid, dim3(WG_THREADS), 0, s, d, S, ntn);
  PQ_LAUNCH_CHECK();
  if (S > 1) {
    const long E = (long)d.K * d.Cin * d.Cout;
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3(ew_grid(E)), dim3(256), 0, s, (const float*)d.ws, d.dW, E, S);
    PQ_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int64_t pq3d_bn_ws_floats(int64_t N, int32_t C) {
  if (N < 0 || C < 1) return -1;
  return bn_blocks((long)N) * C * 3;
}

#define BN_COMMON(name)                                                                              \
  PQ_CHECK_ARG(N >= 1 && C >= 1 && C <= 65535 * BN_CW, name ": N >= 1 and 1 <= C are required");

extern "C" int pq3d_bn_stats(const float* z, int64_t ldz, int64_t N, int32_t C, float eps, float momentum, float* mean, float* rstd,
                             float* running_mean, float* running_var, int64_t* num_batches_tracked, float* part, void* stream) {
  PQ_DEVICE_GUARD(stream, z);
  BN_COMMON("pq3d_bn_stats");
  PQ_CHECK_ARG(z && mean && rstd && part && ldz >= C, "pq3d_bn_stats: z, mean, rstd and part are required, ldz >= C");
  hipStream_t s = (hipStream_t)stream;
  const long P = bn_blocks((long)N);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((unsigned)P, (unsigned)((C + BN_CW - 1) / BN_CW)), dim3(BN_CW * BN_RL), 0, s, z,
                     (long)ldz, (long)N, (int)C, part);
  PQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const float*)part, (int)P, (long)N,
                     (int)C, eps, momentum, mean, rstd, running_mean, running_var, num_batches_tracked);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_bn_apply(const float* z, int64_t ldz, int64_t N, int32_t C, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, const float* residual, int64_t ldr, int32_t act, float* out,
                             int64_t ldo, int32_t col_off, void* stream) {
  PQ_DEVICE_GUARD(stream, out);
  BN_COMMON("pq3d_bn_apply");
  PQ_CHECK_ARG(z && mean && rstd && gamma && beta && out, "pq3d_bn_apply: z, mean, rstd, gamma, beta and out are required");
  PQ_CHECK_ARG(act == PQ3D_ACT_NONE || act == PQ3D_ACT_RELU, "pq3d_bn_apply: act must be NONE or RELU");
  PQ_CHECK_ARG(ldz >= C && col_off >= 0 && ldo >= (int64_t)col_off + C && (!residual || ldr >= C),
               "pq3d_bn_apply: leading dimensions too small (ldz >= C, ldo >= col_off + C, ldr >= C)");
  hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_grid((long)N * C)), dim3(256), 0, (hipStream_t)stream, z, (long)ldz, (long)N, (int)C,
                     mean, rstd, gamma, beta, residual, (long)ldr, (int)act, out, (long)ldo, (int)col_off);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_bn_bwd_reduce(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* z, int64_t ldz, int64_t N,
                                  int32_t C, const float* mean, const float* rstd, float* dgamma, float* dbeta, float* part,
                                  void* stream) {
  PQ_DEVICE_GUARD(stream, dy);
  BN_COMMON("pq3d_bn_bwd_reduce");
  PQ_CHECK_ARG(dy && z && mean && rstd && dgamma && dbeta && part, "pq3d_bn_bwd_reduce: dy, z, mean, rstd, dgamma, dbeta and part are required");
  PQ_CHECK_ARG(lddy >= C && ldz >= C && (!y || ldy >= C), "pq3d_bn_bwd_reduce: leading dimensions too small");
  const DenseGrad grad = {dy, (long)lddy, y, (long)ldy};
  bn_bwd_reduce_launch(grad, z, (long)ldz, (long)N, (int)C, mean, rstd, dgamma, dbeta, part, (hipStream_t)stream);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_bn_bwd_apply(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* z, int64_t ldz, int64_t N,
                                 int32_t C, const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                                 const float* dbeta, float* dz, int64_t lddz, float* dres, int64_t lddres, int32_t dres_add,
                                 void* stream) {
  PQ_DEVICE_GUARD(stream, dy);
  BN_COMMON("pq3d_bn_bwd_apply");
  PQ_CHECK_ARG(dy && z && mean && rstd && gamma && dgamma && dbeta && dz,
               "pq3d_bn_bwd_apply: dy, z, mean, rstd, gamma, dgamma, dbeta and dz are required");
  PQ_CHECK_ARG(lddy >= C && ldz >= C && lddz >= C && (!y || ldy >= C) && (!dres || lddres >= C),
               "pq3d_bn_bwd_apply: leading dimensions too small");
  const DenseGrad grad = {dy, (long)lddy, y, (long)ldy};
  bn_bwd_apply_launch(grad, z, (long)ldz, (long)N, (int)C, mean, rstd, gamma, dgamma, dbeta, dz, (long)lddz, dres, (long)lddres,
                      (int)dres_add, (hipStream_t)stream);
  PQ_LAUNCH_CHECK();
  return 0;
}
