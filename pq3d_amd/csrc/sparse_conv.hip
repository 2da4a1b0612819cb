// Sparse 3-D convolution forward (and, by descriptor field wmode, input gradient) + kernel maps for the voxel backbone
// (pq3d_amd/sparse.py; reference: Res16UNet34C on MinkowskiEngine, modules/third_party/mask3d/res16unet.py).  The weight
// gradient and batch-statistics BatchNorm are in sparse_conv_bwd.hip.  Definition in include/pq3d_hip.h.
//   pq3d_sparse_conv_fwd  out[o] = act((sum_k x[nbr[o, k]] W[k]) * scale + shift + bias + residual[o]), output-stationary:
//                         a workgroup (4 waves) owns 64 output rows x 16 NTL output channels; wave w owns rows 16 w .. 16 w + 15.
//                         Per present offset k and per 32-channel chunk of Cin: the 64 neighbour rows are gathered by index
//                         through registers into an LDS tile in the compute type (the fp32 -> bf16 conversion rides on the
//                         staging, which is why the rows do not come in by LDS-DMA: a DMA load cannot convert; that register
//                         staging costs nothing against it is reasoned, not measured here), the [32, 16 NTL] slab of W[k] is staged transposed
//                         ([n][c]: the MFMA B fragment wants 16 bytes of consecutive c per lane), then KC / KSTEP MFMA steps.
//                         Accumulators stay in registers over all offsets; the epilogue stores every element once.  No atomics,
//                         and the summation order of an output element (offsets ascending, channels ascending) does not depend
//                         on the tiling the host picks: results are bitwise reproducible.
//                         Offsets whose occupancy bit is clear for the tile are skipped without touching memory.
//                         PACKED (Cin < 16): the contraction runs over q = k Cin + c, W viewed as [K Cin, Cout].  With
//                         ct = BF16 this path carries the fp32 input as TWO bf16 planes (hi = bf16(x), lo = bf16(x - hi); a
//                         second MFMA per step against the same W fragment): the stem reads raw data through three channels,
//                         a voxel with few neighbours sums a handful of terms, and bf16's unit roundoff is 2^-8 per operand --
//                         with both operands rounded such a sum can miss 2^-8 sum |x| |W| (measured: 1.03 x), with x exact it
//                         cannot.  The stem is < 1 % of the network's arithmetic.
//   pq3d_sparse_nbr       nbr[o, k] by binary search of the neighbour's key in the level's sorted keys; occupancy word per tile.
#include "common.h"

namespace {

constexpr int SC_T = PQ3D_SPARSE_TILE, SC_KC = 32, SC_THREADS = 256;

template <typename CT, int NTL, bool PACKED>
__global__ __launch_bounds__(SC_THREADS) void sparse_conv_kernel(const pq3d_sparse_conv_desc d) {
  constexpr int TN = 16 * NTL, EPL = Mma<CT>::EPL, KSTEP = Mma<CT>::KSTEP;
  constexpr int LDR = SC_KC + 16 / (int)sizeof(CT);   // LDS row: 32 elements + 16 bytes (keeps 16-byte alignment, shifts banks)
  __shared__ __attribute__((aligned(16))) CT As[SC_T * LDR];
  __shared__ __attribute__((aligned(16))) CT Bs[TN * LDR];
  __shared__ int idx_s[SC_T];
  constexpr bool SPLIT = PACKED && sizeof(CT) == 2;   // packed bf16: the input rides as two bf16 planes, x = hi + lo (see the top)
  __shared__ __attribute__((aligned(16))) CT Al[SPLIT ? SC_T * LDR : 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const long o0 = (long)blockIdx.x * SC_T;
  const int n0 = blockIdx.y * TN;
  const int K = d.K, Cin = d.Cin, Cout = d.Cout;
  f32x4 acc[NTL];
#pragma unroll
  for (int nt = 0; nt < NTL; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  unsigned occw[4] = {~0u, ~0u, ~0u, ~0u};
  if (!PACKED && d.occ) {
#pragma unroll
    for (int w = 0; w < 4; ++w) occw[w] = d.occ[(long)blockIdx.x * 4 + w];
  }
  const int ar = tid >> 2, ac = (tid & 3) * 8;          // A staging: this thread's row of the tile and its 8 channels of the chunk
  const long ao = o0 + ar;
  const int kloops = PACKED ? 1 : K;
  const int clen = PACKED ? K * Cin : Cin;              // length of the contraction one "offset" of the loop runs over
  for (int k = 0; k < kloops; ++k) {
    if (!PACKED) {
      const unsigned w = k < 32 ? occw[0] : k < 64 ? occw[1] : k < 96 ? occw[2] : occw[3];
      if (k < 128 && !((w >> (k & 31)) & 1u)) continue;   // uniform: nothing of this offset in the tile
      if (tid < SC_T) {
        const long o = o0 + tid;
        int ix = -1;
        if (o < d.N_out) {
          ix = d.nbr[o * K + k];
          if (ix < 0 || ix >= d.N_in) ix = -1;
        }
        idx_s[tid] = ix;
      }
      __syncthreads();
    }
    for (int c0 = 0; c0 < clen; c0 += SC_KC) {
      // ---- A: gathered rows -> As[row][c]
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
      if (PACKED) {
        if (ao < d.N_out) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int q = c0 + ac + j;
            if (q < clen) {
              const int kq = q / Cin, c = q - kq * Cin;
              const int ix = d.nbr[ao * K + kq];
              if (ix >= 0 && ix < d.N_in) v[j] = d.x[(long)ix * d.ldx + c];
            }
          }
        }
      } else {
        const int ix = idx_s[ar];
        if (ix >= 0 && c0 + ac < Cin) load_elems<8>(d.x, PQ3D_F32, (long)ix * d.ldx + c0 + ac, Cin - (c0 + ac), v);
      }
      if (sizeof(CT) == 2) {
        *(u32x4*)&As[ar * LDR + ac] = pack_frag<bf16_t>(v);
        if (SPLIT) {
          float lo[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) lo[j] = v[j] - bf2f(f2bf(v[j]));
          *(u32x4*)&Al[ar * LDR + ac] = pack_frag<bf16_t>(lo);
        }
      } else {
        *(float4*)((float*)As + ar * LDR + ac) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)((float*)As + ar * LDR + ac + 4) = make_float4(v[4], v[5], v[6], v[7]);
      }
      // ---- B: W[k][c0 .. c0 + 32)[n0 .. n0 + TN) -> Bs[n][c]
      if (!PACKED && d.wmode) {   // W stored [K, Cout, Cin] (the input gradient): the chunk is contiguous along c, no transpose
        const int kw = d.wmode == 2 ? K - 1 - k : k;
        for (int u = tid; u < TN * (SC_KC / 8); u += SC_THREADS) {
          const int nn = u / (SC_KC / 8), kk = (u - nn * (SC_KC / 8)) * 8;
          float w[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) w[j] = 0.f;
          if (n0 + nn < Cout && c0 + kk < Cin)
            load_elems<8>(d.W, d.dtW, ((long)kw * Cout + n0 + nn) * Cin + c0 + kk, Cin - (c0 + kk), w);
#pragma unroll
          for (int j = 0; j < 8; ++j) Bs[nn * LDR + kk + j] = Cvt<CT>::from(w[j]);
        }
      } else {
        for (int u = tid; u < SC_KC * (TN / 8); u += SC_THREADS) {
          const int kk = u / (TN / 8), nn = (u - kk * (TN / 8)) * 8;
          const int c = c0 + kk;
          float w[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) w[j] = 0.f;
          if (c < clen && n0 + nn < Cout)
            load_elems<8>(d.W, d.dtW, ((long)k * Cin + c) * Cout + n0 + nn, Cout - (n0 + nn), w);
#pragma unroll
          for (int j = 0; j < 8; ++j) Bs[(nn + j) * LDR + kk] = Cvt<CT>::from(w[j]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < SC_KC / KSTEP; ++s) {
        const u32x4 a = *(const u32x4*)&As[(wave * 16 + i) * LDR + s * KSTEP + g * EPL];
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
          const u32x4 b = *(const u32x4*)&Bs[(nt * 16 + i) * LDR + s * KSTEP + g * EPL];
          Mma<CT>::mma(acc[nt], a, b);
        }
        if (SPLIT) {
          const u32x4 al = *(const u32x4*)&Al[(wave * 16 + i) * LDR + s * KSTEP + g * EPL];
#pragma unroll
          for (int nt = 0; nt < NTL; ++nt) {
            const u32x4 b = *(const u32x4*)&Bs[(nt * 16 + i) * LDR + s * KSTEP + g * EPL];
            Mma<CT>::mma(acc[nt], al, b);
          }
        }
      }
      __syncthreads();
    }
  }
  // ---- epilogue: lane holds rows 16 wave + 4 g + r (r = 0..3) of column n0 + 16 nt + i
#pragma unroll
  for (int nt = 0; nt < NTL; ++nt) {
    const int n = n0 + nt * 16 + i;
    if (n >= Cout) continue;
    const float sc = d.scale ? d.scale[n] : 1.f, sh = d.shift ? d.shift[n] : 0.f, bi = d.bias ? d.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long o = o0 + wave * 16 + 4 * g + r;
      if (o >= d.N_out) continue;
      float y = acc[nt][r];
      if (d.scale) y *= sc;
      if (d.shift) y += sh;
      if (d.bias) y += bi;
      if (d.residual) y += d.residual[o * d.ldr + n];
      if (d.act == PQ3D_ACT_RELU) y = fmaxf(y, 0.f);
      d.out[o * d.ldo + d.col_off + n] = y;
    }
  }
}

template <typename CT, bool PACKED>
void sparse_conv_launch(const pq3d_sparse_conv_desc& d, int ntl, hipStream_t s) {
  const unsigned tiles = (unsigned)((d.N_out + SC_T - 1) / SC_T);
  const dim3 grid(tiles, (unsigned)((d.Cout + 16 * ntl - 1) / (16 * ntl)));
  switch (ntl) {
    case 2: hipLaunchKernelGGL((sparse_conv_kernel<CT, 2, PACKED>), grid, dim3(SC_THREADS), 0, s, d); break;
    case 4: hipLaunchKernelGGL((sparse_conv_kernel<CT, 4, PACKED>), grid, dim3(SC_THREADS), 0, s, d); break;
    case 6: hipLaunchKernelGGL((sparse_conv_kernel<CT, 6, PACKED>), grid, dim3(SC_THREADS), 0, s, d); break;
    default: hipLaunchKernelGGL((sparse_conv_kernel<CT, 8, PACKED>), grid, dim3(SC_THREADS), 0, s, d); break;
  }
}

// Output channels per workgroup (16 ntl).  Wide tiles gather every neighbour row once; on the coarse levels (a few row tiles
// against 27 x 256 x 256 weights) the launch is split over output channels instead so that it fills the chip.  The choice
// does not change any output bit.
int pick_ntl(long tiles, int Cout) {
  int ntl = Cout <= 32 ? 2 : Cout <= 64 ? 4 : Cout <= 96 ? 6 : 8;
  if (ntl == 8 && tiles * ((Cout + 127) / 128) < 512) ntl = 4;
  if (ntl == 4 && Cout > 32 && tiles * ((Cout + 63) / 64) < 256) ntl = 2;
  return ntl;
}

// ---- kernel map: one thread per (output row, offset) -------------------------------------------------------------------
__global__ __launch_bounds__(256) void sparse_nbr_kernel(const int64_t* __restrict__ keys, long n_in, const int32_t* __restrict__ q,
                                                         long n_out, const int32_t* __restrict__ offs, int K,
                                                         int32_t* __restrict__ nbr) {
  const long total = n_out * K;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long o = t / K;
    const int k = (int)(t - o * K);
    const long b = q[o * 4];
    const long x = (long)q[o * 4 + 1] + offs[k * 3] + (1L << 19), y = (long)q[o * 4 + 2] + offs[k * 3 + 1] + (1L << 19),
               z = (long)q[o * 4 + 3] + offs[k * 3 + 2] + (1L << 19);
    int hit = -1;
    if (x >= 0 && x < (1L << 20) && y >= 0 && y < (1L << 20) && z >= 0 && z < (1L << 20)) {
      const int64_t key = (b << 60) | (z << 40) | (y << 20) | x;
      long lo = 0, hi = n_in;   // lower bound
      while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < n_in && keys[lo] == key) hit = (int)lo;
    }
    nbr[t] = hit;
  }
}

// one wave per tile of 64 output rows: bit k of the tile's 128-bit word = some row has offset k present
__global__ __launch_bounds__(64) void sparse_occ_kernel(const int32_t* __restrict__ nbr, long n_out, int K, uint32_t* __restrict__ occ) {
  const int lane = threadIdx.x;
  const long o = (long)blockIdx.x * SC_T + lane;
  unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  for (int k = 0; k < K; ++k) {
    const bool p = o < n_out && nbr[o * K + k] >= 0;
    if (__ballot(p) != 0ull) {
      const unsigned bit = 1u << (k & 31);
      if (k < 32) w0 |= bit; else if (k < 64) w1 |= bit; else if (k < 96) w2 |= bit; else w3 |= bit;
    }
  }
  if (lane < 4) occ[(long)blockIdx.x * 4 + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
}

}  // namespace

extern "C" int pq3d_sparse_conv_fwd(const pq3d_sparse_conv_desc* dp, void* stream) {
  PQ_CHECK_ARG(dp, "pq3d_sparse_conv_fwd: null descriptor");
  const pq3d_sparse_conv_desc& d = *dp;
  PQ_DEVICE_GUARD(stream, d.out);
  PQ_CHECK_ARG(d.N_out >= 0 && d.N_in >= 0 && d.Cin >= 1 && d.Cout >= 1 && d.K >= 1, "pq3d_sparse_conv_fwd: bad sizes");
  PQ_CHECK_ARG(d.ct == PQ3D_F32 || d.ct == PQ3D_BF16, "pq3d_sparse_conv_fwd: ct must be PQ3D_F32 or PQ3D_BF16");
  PQ_CHECK_ARG(d.dtW == PQ3D_F32 || d.dtW == PQ3D_BF16, "pq3d_sparse_conv_fwd: bad weight dtype");
  PQ_CHECK_ARG(d.act == PQ3D_ACT_NONE || d.act == PQ3D_ACT_RELU, "pq3d_sparse_conv_fwd: act must be NONE or RELU");
  PQ_CHECK_ARG(d.ldx >= d.Cin && d.col_off >= 0 && d.ldo >= (int64_t)d.col_off + d.Cout && (!d.residual || d.ldr >= d.Cout),
               "pq3d_sparse_conv_fwd: leading dimensions too small (ldx >= Cin, ldo >= col_off + Cout, ldr >= Cout)");
  PQ_CHECK_ARG(!d.occ || d.K <= 128, "pq3d_sparse_conv_fwd: occupancy words cover K <= 128 offsets");
  PQ_CHECK_ARG((int64_t)d.K * d.Cin <= (1 << 24), "pq3d_sparse_conv_fwd: K * Cin too large");
  if (d.N_out == 0) return 0;
  PQ_CHECK_ARG(d.x && d.nbr && d.W && d.out, "pq3d_sparse_conv_fwd: x, nbr, W and out are required");
  PQ_CHECK_ARG((((uintptr_t)d.x | (uintptr_t)d.out | (uintptr_t)d.residual) & 3) == 0 && (((uintptr_t)d.W) & 1) == 0,
               "pq3d_sparse_conv_fwd: misaligned pointer");
  const long tiles = ((long)d.N_out + SC_T - 1) / SC_T;
  const bool packed = d.Cin < 16 && d.K > 1;
  PQ_CHECK_ARG(d.wmode >= 0 && d.wmode <= 2 && !(packed && d.wmode), "pq3d_sparse_conv_fwd: wmode must be 0, 1 or 2 (1, 2: Cin >= 16 or K = 1)");
  PQ_CHECK_ARG(d.ntl == 0 || d.ntl == 2 || d.ntl == 4 || d.ntl == 6 || d.ntl == 8, "pq3d_sparse_conv_fwd: ntl must be 0, 2, 4, 6 or 8");
  const int ntl = d.ntl ? d.ntl : pick_ntl(tiles, d.Cout);
  PQ_CHECK_ARG((d.Cout + 16 * ntl - 1) / (16 * ntl) <= 65535, "pq3d_sparse_conv_fwd: Cout too large");
  hipStream_t s = (hipStream_t)stream;
  if (d.ct == PQ3D_BF16) {
    if (packed) sparse_conv_launch<bf16_t, true>(d, ntl, s); else sparse_conv_launch<bf16_t, false>(d, ntl, s);
  } else {
    if (packed) sparse_conv_launch<float, true>(d, ntl, s); else sparse_conv_launch<float, false>(d, ntl, s);
  }
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_sparse_nbr(const int64_t* keys, int64_t n_in, const int32_t* q, int64_t n_out, const int32_t* offs, int32_t K,
                               int32_t* nbr, uint32_t* occ, void* stream) {
  PQ_DEVICE_GUARD(stream, nbr);
  PQ_CHECK_ARG(nbr && n_in >= 0 && n_out >= 0 && K >= 1, "pq3d_sparse_nbr: bad args");
  PQ_CHECK_ARG(n_in <= 0x7fffffffL && n_out <= 0x7fffffffL, "pq3d_sparse_nbr: rows are int32 indices");
  PQ_CHECK_ARG(!keys || (q && offs), "pq3d_sparse_nbr: a lookup needs q and offs");
  PQ_CHECK_ARG(!occ || K <= 128, "pq3d_sparse_nbr: occupancy words cover K <= 128 offsets");
  if (n_out == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (keys) {
    const long total = (long)n_out * K;
    long gsz = (total + 255) / 256;
    if (gsz > 65536) gsz = 65536;
    hipLaunchKernelGGL(sparse_nbr_kernel, dim3((unsigned)gsz), dim3(256), 0, s, keys, (long)n_in, q, (long)n_out, offs, (int)K, nbr);
    PQ_LAUNCH_CHECK();
  }
  if (occ) {
    hipLaunchKernelGGL(sparse_occ_kernel, dim3((unsigned)((n_out + SC_T - 1) / SC_T)), dim3(64), 0, s, nbr, (long)n_out, (int)K, occ);
    PQ_LAUNCH_CHECK();
  }
  return 0;
}
