// Body of gemm_wktt_kernel / gemm_wktt_kg_kernel (gemm_wktt.hip), included once per kernel between the kernel's braces: the
// kernel descriptor `d` (by value), the split factor `sk`, the template parameters TA, TB, HB2, KC, TT and the macro WKTT_K = the
// reduction length of this workgroup's group (d.K for the uniform kernel, whose code this text leaves exactly as it was).
  constexpr int TM = TT, TN = TT, LDT = TT + 8, CPK = TT / 8;   // [k][TT + 8] bf16 tiles of A and B; 8-element chunks per k row
  constexpr int MI = TT / 64, NJ = TT / 32;                     // 16x16 MFMA blocks per wave: 4 x 2 waves of (16 MI) x (16 NJ)
  extern __shared__ __attribute__((aligned(16))) unsigned char tt_smem[];
  bf16_t* const At = (bf16_t*)tt_smem;        // [KC][LDT]: A(k, m0 + col)
  bf16_t* const Bt = At + KC * LDT;           // [KC][LDT]: B(k, n0 + col)
  constexpr int NCH = KC * CPK / WT;          // 8-element chunks per operand per thread (4)
  const int split = blockIdx.z % sk, g = blockIdx.z / sk;
  const pq3d_kgroup& q = d.gp[min(g, PQ3D_MAX_GROUPS - 1)];
  const TA* A = (const TA*)q.A;
  const TB* B = (const TB*)q.B;
  const float* B2 = (const float*)q.B2;
  float* C = (float*)q.C;
  // the tiles one XCD receives are neighbours in the (m, n) plane (common.h tile_index_plane): in hardware order the n-tiles
  // of one m-tile sit gridDim.x ids apart -- on other XCDs, much later -- and every one of them fetches the g slab again
  // (caption LM head, dW [32128 x 512] over 512 rows: 8 n-tiles, 535-643 MB fetched per launch for 66 MB of g)
  const TileIdx ti = tile_index_plane(d.xcd_order);
  float* cs_out = ti.y == 0 ? q.colsum : nullptr;
  asm volatile("" ::"s"(d.M), "s"(d.N), "s"(d.K), "s"(d.lda), "s"(d.ldb), "s"(d.ldc), "s"(d.alpha), "s"(A), "s"(B), "s"(B2), "s"(C), "s"(cs_out));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int wm = (wave >> 1) * (16 * MI), wn = (wave & 1) * (16 * NJ);   // 4 x 2 waves
  const int m0 = ti.x * TM, n0 = ti.y * TN;
  const int nck = (WKTT_K + KC - 1) / KC, per = (nck + sk - 1) / sk;
  const int c0 = split * per, c1 = min(nck, c0 + per);
  if (c0 >= c1) return;
  f32x4 acc[MI][NJ], accb[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bool do_cs = cs_out != nullptr && wn == 0;
  Raw<TA, 8> ra[NCH];
  Raw<TB, 8> rb[NCH];
  Raw<float, 8> rb2[HB2 ? NCH : 1];
  bool ok[NCH];
  const float s2 = B2 ? 1.f : 0.f;
  auto issue = [&](int ck) {
    const int k0 = ck * KC;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + i * WT, k = k0 + c / CPK, x = (c % CPK) * 8;
      ok[i] = k < WKTT_K;
      const long ka = ok[i] ? k : 0;
      const long offa = ka * d.lda + min(m0 + x, d.M - 8), offb = ka * d.ldb + min(n0 + x, d.N - 8);
      ra[i].load(A + offa);
      rb[i].load(B + offb);
      if constexpr (HB2) rb2[i].load(B2 ? B2 + offb : (const float*)B + offb);
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + i * WT, o = (c / CPK) * LDT + (c % CPK) * 8;
      u32x4 pa, pb;
      if constexpr (sizeof(TA) == 2) pa = __builtin_bit_cast(u32x4, ra[i]);
      else { float v[8]; ra[i].to_float(v); pa = pack_frag<bf16_t>(v); }
      if constexpr (sizeof(TB) == 2 && !HB2) pb = __builtin_bit_cast(u32x4, rb[i]);
      else {
        float v[8];
        rb[i].to_float(v);
        if constexpr (HB2) {
          float w[8];
          rb2[i].to_float(w);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += s2 * w[j];
        }
        pb = pack_frag<bf16_t>(v);
      }
      if (!ok[i]) { pa = (u32x4){0, 0, 0, 0}; pb = (u32x4){0, 0, 0, 0}; }
      *(u32x4*)&At[o] = pa;
      *(u32x4*)&Bt[o] = pb;
    }
  };
  issue(c0);
  for (int ck = c0; ck < c1; ++ck) {
    if (ck > c0) __syncthreads();
    put();
    __syncthreads();
    const int nks = (min(KC, WKTT_K - ck * KC) + 31) >> 5;
    if (ck + 1 < c1) issue(ck + 1);
#pragma unroll
    for (int ks = 0; ks < KC / 32; ++ks) {
      if (ks < nks) {   // uniform
        u32x4 a[MI], bfr[NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i) a[i] = km_frag(At, LDT, wm + i * 16, ks, li, lg);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bfr[j] = km_frag(Bt, LDT, wn + j * 16, ks, li, lg);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) Mma<bf16_t>::mma(acc[i][j], a[i], bfr[j]);
        if (do_cs) {
          const u32x4 ones = (u32x4){0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
#pragma unroll
          for (int i = 0; i < MI; ++i) Mma<bf16_t>::mma(accb[i], a[i], ones);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = n0 + wn + j * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + i * 16 + lg * 4 + r;
        // (a plain read-modify-write for unsplit launches -- one writer per element -- was measured SLOWER than the L2 atomics:
        // 62 vs 59 us average at config 5: the returning loads stall the epilogue, the atomics are fire-and-forget)
        if (row < d.M && col < d.N) unsafeAtomicAdd(C + (long)row * d.ldc + col, acc[i][j][r] * d.alpha);
      }
    }
  if (do_cs && li == 0) {   // every column of accb holds the row sums of the A tile over k
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + i * 16 + lg * 4 + r;
        if (row < d.M) unsafeAtomicAdd(&cs_out[row], accb[i][r] * d.alpha);
      }
  }
