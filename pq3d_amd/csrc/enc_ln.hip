// One launch for G independent nn.Sequential(Linear, LayerNorm) encoders of one (K, N) (ObjectEncoder.input_feat_proj of every scene
// memory AND CoordinateEncoder.feat_proj: N = 256 outputs, K <= 256 inputs, thousands of rows, a row count per group):
//     lin_g = x_g W_g^T + b_g          y_g = LN_g(lin_g)          (lin, mean, rstd kept for the backward pass)
// Until now a grouped GEMM wrote lin and an independent-branch LayerNorm launch read it straight back.  A workgroup that owns whole
// rows has the complete row when its tile's products finish, so the LayerNorm runs on the tile in LDS; lin leaves once, for the tape.
//
// Plan: persistent workgroups, at most one per CU, each with a contiguous range of 32-row tiles: the groups' ceil(rows[g] / 32)
// tiles laid end to end, every group's tiles starting at its row 0 (so a group's tile boundaries do not depend on its neighbours,
// and a short launch -- the position encoder's 281 tiles, 25 workgroups with a second round -- rides in a long one: 1049 tiles at
// config 2, 4-5 per workgroup).  A workgroup finds (group, first row) of a tile with a cursor over the groups' tile counts that
// only moves forward; mean / rstd are packed group after group.
// Every row here is streaming work (K = 256: 1 KB in, 2 KB out per row), so the compulsory traffic is the floor; what the two-launch
// path added on top was W: 256 KB per group, fetched from L2 and split into hi / lo bf16 planes once per ROW TILE (as much conversion
// work per tile as 8 tiles of x).  Here wave w keeps output columns [32 w, 32 w + 32) of W -- hi and lo MFMA fragments over the
// whole K, 16 registers per 32-wide k step, 128 at K = 256 -- in registers for the workgroup's life: W is fetched and split once
// per workgroup (again where its range crosses into the next group), and only x goes through LDS (34 KB of planes + the 33 KB
// fp32 output tile: one 8-wave workgroup per CU, 2 waves per SIMD, 256 registers each).  The next tile's x rows are in flight during
// the current tile's MFMAs and LayerNorm.  No workgroup ever waits for another.
//
// Arithmetic is the two launches' own: split-bf16 product (hi / lo planes of chain_common.h's split_hi_lo = gemm.hip's store_split; per
// 32-wide k step the terms lo*hi, hi*lo, hi*hi, k ascending, one accumulator per output: gemm.hip's mma_tile_x3), bias added to the
// accumulator, then add_ln_fwd_kernel<4, true>'s independent-branch row: lane l owns columns 4 l .. 4 l + 3, ln_row.h's statistics.
// tests/test_gpu_enc_ln.py compares lin, mean, rstd and y bit for bit with the two-launch path, tests/test_gpu_enc_ragged.py a
// launch over unequal groups with one launch per group.
#include <atomic>

#include "chain_common.h"

namespace {

constexpr int EN = 256;                 // output columns = LayerNorm width
constexpr int ECL = EN + 4;             // fp32 output tile [32][ECL]

template <int KS> constexpr size_t enc_lds() { return (size_t)2 * TM * (KS * 32 + 8) * 2 + (size_t)TM * ECL * 4; }

// KS: 32-wide k steps (K = 32 KS)
template <int KS>
__global__ __launch_bounds__(CT) void linear_ln_fwd_kernel(const pq3d_linear_ln_desc d, const int ntiles) {
  constexpr int K = KS * 32, LDA = K + 8, CPR = K / 8;        // 8-float chunks per row
  constexpr int NCH = (TM * CPR + CT - 1) / CT;               // chunks of a row tile per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char enc_smem[];
  bf16_t* const Ah = (bf16_t*)enc_smem;                       // [32][LDA] x 2 planes
  bf16_t* const Al = Ah + TM * LDA;
  float* const Ct = (float*)(Al + TM * LDA);                  // [32][ECL]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int wc = wave * 32;                                   // this wave's output columns
  // the groups' ceil(rows[g] / 32) tiles laid end to end (the host filled rows[] and counted them)
  const long total = ntiles;
  const int t0 = (int)(total * blockIdx.x / gridDim.x), t1 = (int)(total * (blockIdx.x + 1) / gridDim.x);
  if (t0 >= t1) return;
  // (uniform) a cursor over the groups: g holds tiles [tb, tb + tiles(rows[g])) and statistics rows from so on.  Tiles are visited
  // in ascending order, so a cursor only ever moves forward: at most `groups` steps in a workgroup's life
  struct Cur { int g, tb, R; long so; };
  auto seek = [&](Cur& c, int t) {
    while (t >= c.tb + (c.R + TM - 1) / TM) {
      c.tb += (c.R + TM - 1) / TM;
      c.so += c.R;
      c.R = d.rows[++c.g];
    }
  };
  Cur ci = {0, 0, d.rows[0], 0};      // of the tile whose rows are being fetched
  seek(ci, t0);
  Cur cc = ci;                        // of the tile being computed

  float av[NCH][8];
  auto issue = [&](int t) {           // the tile's x rows (rows past the group's end: clamped duplicates, never stored)
    seek(ci, t);
    const int R = ci.R, m0 = (t - ci.tb) * TM;
    const float* x = d.x[ci.g];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * CT;
      if (TM * CPR % CT == 0 || ch < TM * CPR) load8<false>(x, (long)min(m0 + ch / CPR, R - 1) * K + (ch % CPR) * 8, av[i]);
    }
  };
  issue(t0);
  u32x4 bh[2][KS], bl[2][KS];
  float bcol[2], gm[4], bt[4];
  int cur = -1;
  for (int t = t0; t < t1; ++t) {
    seek(cc, t);
    const int g = cc.g, R = cc.R, m0 = (t - cc.tb) * TM;
    if (g != cur) {                   // (uniform) this group's weight fragments, bias and LayerNorm parameters
      cur = g;
      const float* W = d.W[g];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          float v[8];
          load8<false>(W, (long)(wc + nb * 16 + li) * K + ks * 32 + lg * 8, v);
          split_hi_lo(v, bh[nb][ks], bl[nb][ks]);
        }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) bcol[nb] = d.bias[g] ? d.bias[g][wc + nb * 16 + li] : 0.f;
      load4<false>(d.gamma[g], lane * 4, gm);
      load4<false>(d.beta[g], lane * 4, bt);
    }
    // x planes of the tile (the previous tile's fragment reads ended before its output tile was written)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * CT;
      if (TM * CPR % CT == 0 || ch < TM * CPR) {
        const int o = (ch / CPR) * LDA + (ch % CPR) * 8;
        u32x4 hi, lo;
        split_hi_lo(av[i], hi, lo);
        *(u32x4*)&Ah[o] = hi;
        *(u32x4*)&Al[o] = lo;
      }
    }
    __syncthreads();                  // planes complete; the previous tile's LayerNorm reads of Ct are done
    if (t + 1 < t1) issue(t + 1);
    f32x4 acc[2][2];
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[rh][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4 ah[2], al[2];
#pragma unroll
      for (int rh = 0; rh < 2; ++rh) {
        const int oa = (rh * 16 + li) * LDA + ks * 32 + lg * 8;
        ah[rh] = *(const u32x4*)&Ah[oa];
        al[rh] = *(const u32x4*)&Al[oa];
      }
#pragma unroll
      for (int rh = 0; rh < 2; ++rh)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          Mma<bf16_t>::mma(acc[rh][nb], al[rh], bh[nb][ks]);
          Mma<bf16_t>::mma(acc[rh][nb], ah[rh], bl[nb][ks]);
          Mma<bf16_t>::mma(acc[rh][nb], ah[rh], bh[nb][ks]);
        }
    }
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ct[(rh * 16 + lg * 4 + r) * ECL + wc + nb * 16 + li] = (acc[rh][nb][r] + bcol[nb]) * 1.f;
    __syncthreads();
    // LayerNorm of the tile: wave w takes rows 4 w .. 4 w + 3 (add_ln_fwd_kernel<4, true>, independent branch, no residual)
    float* const ling = d.lin[g];
    float* const yg = d.y[g];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lr = wave * 4 + i;
      const long row = m0 + lr;
      if (row < R) {                  // (uniform per wave)
        const float4 l4 = *(const float4*)&Ct[lr * ECL + lane * 4];
        const long base = row * EN + lane * 4;
        *(float4*)(ling + base) = l4;
        const float ov[4] = {l4.x, l4.y, l4.z, l4.w};
        float v[4], out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 0.f + ov[j];
        const RowStats st = ln_row_stats(v, EN, d.eps, AllCols{});
#pragma unroll
        for (int j = 0; j < 4; ++j) { out[j] = 0.f; out[j] += 1.f * ((v[j] - st.mean) * st.rstd * gm[j] + bt[j]); }
        if (lane == 0) {
          d.mean[cc.so + row] = st.mean;
          d.rstd[cc.so + row] = st.rstd;
        }
        *(float4*)(yg + base) = make_float4(out[0], out[1], out[2], out[3]);
      }
    }
  }
}

int enc_cus() {   // CUs of the current device (one persistent workgroup each)
  static std::atomic<int> cus[32];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int n = cus[dev & 31].load(std::memory_order_relaxed);
  if (n <= 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
    cus[dev & 31].store(n, std::memory_order_relaxed);
  }
  return n;
}

template <int KS> int enc_launch(const pq3d_linear_ln_desc& d, int ntiles, hipStream_t s) {
  static std::atomic<unsigned> done{0};
  auto kern = linear_ln_fwd_kernel<KS>;
  if (int e = pq3d_enable_big_lds(kern, (int)enc_lds<KS>(), done)) { pq3d_set_error(hipGetErrorString((hipError_t)e)); return e; }
  const long total = ntiles;
  const long cus = enc_cus();
  hipLaunchKernelGGL(kern, dim3((unsigned)(total < cus ? total : cus)), dim3(CT), enc_lds<KS>(), s, d, ntiles);
  return 0;
}

}  // namespace

extern "C" int pq3d_linear_ln_fwd(const pq3d_linear_ln_desc* dp, void* stream) {
  PQ_DEVICE_GUARD(stream, dp ? dp->x[0] : nullptr);
  PQ_CHECK_ARG(dp != nullptr, "pq3d_linear_ln_fwd: null descriptor");
  pq3d_linear_ln_desc d = *dp;
  PQ_CHECK_ARG(d.N == EN && d.K >= 64 && d.K <= 256 && d.K % 64 == 0, "pq3d_linear_ln_fwd: N = 256, K in {64, 128, 192, 256}");
  PQ_CHECK_ARG(d.groups >= 1 && d.groups <= PQ3D_MAX_GROUPS, "pq3d_linear_ln_fwd: 1 <= groups <= PQ3D_MAX_GROUPS");
  bool ragged = false;
  for (int g = 0; g < PQ3D_MAX_GROUPS; ++g) ragged = ragged || d.rows[g] != 0;
  long tiles = 0;
  for (int g = 0; g < PQ3D_MAX_GROUPS; ++g) {
    if (g >= d.groups) { PQ_CHECK_ARG(d.rows[g] == 0, "pq3d_linear_ln_fwd: rows set past the last group"); continue; }
    if (!ragged) d.rows[g] = d.R;     // all zero: R rows in every group
    PQ_CHECK_ARG(d.rows[g] >= 1, ragged ? "pq3d_linear_ln_fwd: every group's rows >= 1 (or all zero)" : "pq3d_linear_ln_fwd: R >= 1");
    PQ_CHECK_ARG((long)d.rows[g] * EN < (1L << 31), "pq3d_linear_ln_fwd: too many rows");
    tiles += (d.rows[g] + TM - 1) / TM;
  }
  PQ_CHECK_ARG(tiles < (1L << 30), "pq3d_linear_ln_fwd: too many rows");
  const int nt = (int)tiles;          // (the kernel reads rows[], never R)
  PQ_CHECK_ARG(d.mean && d.rstd, "pq3d_linear_ln_fwd: null mean / rstd");
  for (int g = 0; g < d.groups; ++g) {
    PQ_CHECK_ARG(d.x[g] && d.W[g] && d.gamma[g] && d.beta[g] && d.lin[g] && d.y[g], "pq3d_linear_ln_fwd: null pointer");
    const void* al[] = {d.x[g], d.W[g], d.gamma[g], d.beta[g], d.lin[g], d.y[g]};
    for (const void* p : al) PQ_CHECK_ARG((((uintptr_t)p) & 15) == 0, "pq3d_linear_ln_fwd: operands must be 16-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  int e = 0;
  switch (d.K / 32) {
    case 2: e = enc_launch<2>(d, nt, s); break;
    case 4: e = enc_launch<4>(d, nt, s); break;
    case 6: e = enc_launch<6>(d, nt, s); break;
    default: e = enc_launch<8>(d, nt, s); break;
  }
  if (e) return e;
  PQ_LAUNCH_CHECK();
  return 0;
}
