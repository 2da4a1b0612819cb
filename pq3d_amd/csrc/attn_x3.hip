// Split-bf16 cross-attention forward (compute mode 'bf16x3'): fp32-GRADE scores and value contraction on the bf16 matrix cores.
//
// Reference arithmetic: CrossAttentionLayer.forward_post (query_encoder.py:288-307) -> nn.MultiheadAttention with add_zero_attn
// (:268-270): softmax(q k^T / sqrt(d_h) [+ masks, + the zero key]) v in fp32.  The 'bf16' mode rounds K, V, Q, P and O to bf16
// (five sites of 0.8e-3 .. 1.5e-3 of the query scale each after 4 layers: profiles/rounding_sites_r05.txt), which is what keeps it
// at 3e-3 .. 7e-3 end to end.  Here every one of them is carried as a hi + lo bf16 pair:
//   * K and V arrive as two bf16 PLANES (hi = bf16(x), lo = bf16(x - hi): pq3d_gemm's PQ3D_ACT_PLANES epilogue) -- the bytes of an
//     fp32 tensor, but each plane is an MFMA operand as stored (no conversion in the loop, and the backward reads the hi plane
//     alone = exactly a 'bf16'-mode tensor);
//   * q (fp32) is split once into register fragments, P (fp32 registers) per 64-key block;
//   * S = K_lo q_hi + K_hi q_lo + K_hi q_hi and O += V_lo P_hi + V_hi P_lo + V_hi P_hi (small terms first): 3 MFMAs per product,
//     ~2^-17 relative per term; O leaves in fp32 (+ a bf16 copy for the backward's delta / weight gradient).
// Structure = attn_resident.hip's all-keys-resident forward: 8 compute waves (16 queries each) + 4 loader waves, the key/value
// slice parked in LDS, online softmax per wave.  Two planes double the LDS per key (289 B), so a workgroup holds 512 keys at a
// time (stage 1, then stage 2 over it; <= 1024 keys per key split as before: config 2 needs no split / combine launch).
// STAGING (profiles/NOTES_attn_x3_staging.md): a stage arrives in NP = 4 PIECES (128 keys; d_h = 64: 64), each behind a workgroup
// barrier of its own, so block 0 starts once a quarter of stage 1 is parked instead of all of it:
//   * the compute waves request piece 0 (one chunk of each plane per thread) as the first thing that goes to memory -- q rows,
//     key-padding bytes and mask words queue behind it -- park it, (A0), and run its blocks; then (Ap), blocks of piece p, ...
//   * the loader waves request pieces 1 .. 3 in the order of their use, pass (A0), and per piece: park it, request the next part
//     of stage 2 into the registers it has left (a quarter behind pieces 1 and 2 each, half behind piece 3: never more than the
//     128 registers stage 2 needs anyway), (Ap).  Once (A3) is passed pieces 0 .. 2 are consumed: three quarters of stage 2 are
//     parked over them while piece 3 is read; the last quarter and the mask words after (B), then (C).
//   * every wave of the workgroup executes the same barriers on every path (the count depends on the slice's block count alone,
//     which is uniform); a block that returns early returns from block() only.
// Loads use a uniform base per plane + a 32-bit byte offset (a scene's key/value rows span < 4 GB: checked by the launcher): with
// 64-bit per-lane addresses the up to 32 requests a loader thread keeps in flight did not fit 168 registers.
// Measured at config 2 (MI355X, same box, alternating runs): entry -> first barrier 6.5-7.0 us -> 3.0-3.4 us in workgroup 0, the
// launch 33.4 / 33.5 us -> 28.0 / 28.1 us.  Arithmetic, block order, grid and key splits are untouched: outputs are bit for bit
// what they were (tests/test_gpu_x3_staging.py).
// d_h = 64 (the head width of the reference's shipped decoders: hidden 768, 12 heads, configs/instseg_sceneverse.yaml:95,141) runs the
// same kernel with 256 keys per stage (both planes padded to 144-byte rows), two k steps per score tile and the K / V fragments
// fetched per tile instead of per block (168 registers per wave): shipped stage-1 / stage-2 decoder steps 14.7 / 15.4 ms in
// 'bf16x3' against 49.8 / 52.6 ms on the exact-f32 kernels the mode fell back to before, 13.6 / 13.7 ms in 'bf16'.
// New against the bf16 kernel: a 3-D self-mask as BIT WORDS (pq3d_mask_pack: row_open folded in) staged per 512-key stage, and up
// to 256 queries as two query halves in grid.x -- config 4's shape (200 queries, 4096 keys, self-mask) stays on this kernel.
#include <atomic>
#include <type_traits>

#include "attn_common.h"

namespace {

constexpr int XW = 8;             // compute waves = 16-query tiles
constexpr int XLW = 4;            // loader waves
// per head size: keys resident at a time (16 KB of one K plane), 64-key blocks per stage, LDS row strides.  d_h = 32: K rows unpadded
// (64 B: the 289 B per key that let 512 keys stay); d_h = 64: both planes padded to 72 elements (144 B rows: 16 lanes of a fragment
// read cover 16 distinct 4-bank groups; unpadded 128 B rows would be 8-way conflicts), 256 keys per stage.
template <int DH> struct X3 {
  static constexpr int XK = 16384 / DH;              // 512 / 256
  static constexpr int XNB = XK / KB;                // 8 / 4
  static constexpr int CPR = DH / 8;                 // 16-byte chunks per key row and plane
  static constexpr int NP = 4;                       // stage 1 arrives in NP pieces of PB 64-key blocks (128 / 64 keys)
  static constexpr int PB = XNB / NP;                // 2 / 1
  static constexpr int PCH = XK * CPR / NP;          // chunks of one plane per piece (512): one per compute thread (piece 0)
  static constexpr int LCP = PCH / (XLW * 64);       // ... per loader thread and piece (pieces 1 .. NP - 1) (2)
  static constexpr int XCH2 = XK * CPR / (XLW * 64); // ... per loader thread, stage 2 (8)
  // first stage-2 chunk a loader thread requests once piece p is parked: XCH2 / NP behind each piece but the last, the rest there
  static constexpr int s2lo(int p) { return p >= NP ? XCH2 : (p - 1) * XCH2 / NP; }
  static_assert(PCH == XW * 64 && LCP * XLW * 64 == PCH && PB * NP == XNB && XCH2 % NP == 0, "piece layout");
  static constexpr int MWR = 2 * XNB;                // mask words per query row and stage
  static constexpr int XMW = MWR + 1;                // + 1: conflict-free column reads
  static constexpr int MW1 = MWR * 128 / (XW * 64);  // mask words per compute thread (stage 1) / loader thread (stage 2)
  static constexpr int MW2 = MWR * 128 / (XLW * 64);
  static constexpr int LDK = DH == 32 ? 32 : AT<bf16_t, DH>::LDR;
  static constexpr int LDV = AT<bf16_t, DH>::LDR;
  static constexpr int KSD = DH / 32;                // k steps of a product over d_h
};

// probe builds only (-DPQ3D_X3_TIMELINE, tools/probes/x3_timeline.py): thread 0 of workgroup (0, 0, 0) stamps wall_clock64() into
// d.ws (unused without a key split): 0 entry, 1 first stage-1 requests issued, 2 first barrier passed, 3 last block of stage 1
// done, 4 barrier (C) passed, 5 last block done, 6 exit
#ifdef PQ3D_X3_TIMELINE
#define X3_TL(i) do { if (d.ws && KS == 1 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) ((long long*)d.ws)[i] = wall_clock64(); } while (0)
#else
#define X3_TL(i) do { } while (0)
#endif

PQ_DEV void x3_split(const float* v, u32x4& hi, u32x4& lo) {
  hi = pack_frag<bf16_t>(v);
  float w[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w[2 * j] = v[2 * j] - __uint_as_float(hi[j] << 16);
    w[2 * j + 1] = v[2 * j + 1] - __uint_as_float(hi[j] & 0xffff0000u);
  }
  lo = pack_frag<bf16_t>(w);
}

template <int DH, bool DROP, bool MASKB>
__global__ __launch_bounds__((XW + XLW) * 64) void attn_fwd_x3_kernel(const pq3d_attn_desc d, const int KS, const int per) {
  ATTN_KARG_PIN(d);
  typedef AT<bf16_t, DH> A;
  typedef X3<DH> X;
  constexpr int LDK = X::LDK, LDV = X::LDV, XK = X::XK, XNB = X::XNB, CPR = X::CPR, XCH2 = X::XCH2, XMW = X::XMW,
                MWR = X::MWR, KSD = X::KSD, NP = X::NP, PB = X::PB, PCH = X::PCH, LCP = X::LCP;
  extern __shared__ __attribute__((aligned(16))) unsigned char xsm[];
  bf16_t* const Kh = (bf16_t*)xsm;
  bf16_t* const Kl = Kh + XK * LDK;
  bf16_t* const Vh = Kl + XK * LDK;
  bf16_t* const Vl = Vh + XK * LDV;
  uint8_t* const kpm_s = (uint8_t*)(Vl + XK * LDV);          // [2 XK] key padding of the whole slice
  uint32_t* const msk_s = (uint32_t*)(kpm_s + 2 * XK);       // [128][XMW] mask bit words of the current stage (MASKB)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
  const WgXyz wg = attn_wg_xyz(KS);
  const int b = wg.b, h = wg.h, split = wg.x % KS, qh = wg.x / KS;
  const int nkb = (d.Lk + KB - 1) / KB;
  const int kb_lo = (int)((long)nkb * split / KS), kb_hi = (int)((long)nkb * (split + 1) / KS);
  const int nb = kb_hi - kb_lo, key_lo = kb_lo * KB, nk = nb * KB;
  const bool loader = wave >= XW;   // wave-uniform role
  const long koff = (long)b * d.k_sb + (long)h * d.k_sh, voff = (long)b * d.v_sb + (long)h * d.v_sh;
  const int q_base = qh * per, q_end = min(q_base + per, d.Lq);
  const int q0 = q_base + wave * 16, myq = q0 + li;
  const bool wave_active = !loader && q0 < q_end, qvalid = !loader && myq < q_end;
  const int bm = d.mask_bmod > 0 ? b % d.mask_bmod : b;
  const int nwords = (d.Lk + 31) / 32;
  X3_TL(0);

  // one 16-byte chunk of a key row in all four planes: global -> registers (rows past the slice / past Lk: clamped duplicates,
  // never parked / masked through kpm_s)
  // Addresses = a workgroup-uniform base per plane + a 32-bit byte offset (one register per K / V pair; the launcher checks that a
  // (scene, head)'s rows span < 4 GB): the staging below keeps up to 32 requests of a thread in flight.
  const char* const kbh = (const char*)((const bf16_t*)d.k + koff), * const kbl = (const char*)((const bf16_t*)d.k_lo + koff);
  const char* const vbh = (const char*)((const bf16_t*)d.v + voff), * const vbl = (const char*)((const bf16_t*)d.v_lo + voff);
  const uint32_t k_sl2 = (uint32_t)d.k_sl * 2u, v_sl2 = (uint32_t)d.v_sl * 2u;
  // Chunk c = c0 + t with c0 a constant multiple of CPR and t the thread's index among its role's threads: row c0 / CPR + t / CPR,
  // part t % CPR -- the thread's two terms are computed once, every chunk differs by a constant.
  auto gload = [&](int stage, int c0, int t, u32x4& kh, u32x4& kl, u32x4& vh, u32x4& vl) {
    const uint32_t gk = (uint32_t)min(key_lo + stage * XK + c0 / CPR + t / CPR, d.Lk - 1), part = (uint32_t)(t % CPR) * 16u;
    const uint32_t ko = gk * k_sl2 + part, vo = gk * v_sl2 + part;
    kh = *(const u32x4*)(kbh + ko);
    kl = *(const u32x4*)(kbl + ko);
    vh = *(const u32x4*)(vbh + vo);
    vl = *(const u32x4*)(vbl + vo);
  };
  auto park = [&](int c0, int t, const u32x4& kh, const u32x4& kl, const u32x4& vh, const u32x4& vl) {
    const int ko = (t / CPR) * LDK + (t % CPR) * 8, vo = (t / CPR) * LDV + (t % CPR) * 8;
    *(u32x4*)&Kh[ko + (c0 / CPR) * LDK] = kh;
    *(u32x4*)&Kl[ko + (c0 / CPR) * LDK] = kl;
    *(u32x4*)&Vh[vo + (c0 / CPR) * LDV] = vh;
    *(u32x4*)&Vl[vo + (c0 / CPR) * LDV] = vl;
  };
  // the stage's mask words of the workgroup's 128 query rows: word (q, w) = bits[bm, q_base + q, 2 (kb_lo + 8 stage) + w]
  const char* const mrow = MASKB ? (const char*)(d.mask_bits + (long)bm * d.Lq * nwords) : nullptr;   // uniform; <= 256 rows of nwords
  auto mask_words = [&](int stage, int t, int nthreads, uint32_t (&mw)[X::MW2], int n) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const int q = t / MWR + i * (nthreads / MWR), w = t % MWR;   // word t + i nthreads (nthreads: a multiple of MWR)
      const int gq = min(q_base + q, d.Lq - 1), gw = 2 * (kb_lo + XNB * stage) + w;
      // clamped, not branched around (one basic block); uniform base + 32-bit byte offset as in gload
      const uint32_t wv = *(const uint32_t*)(mrow + (uint32_t)(gq * nwords + min(gw, nwords - 1)) * 4u);
      mw[i] = gw < nwords ? wv : 0u;
    }
  };
  auto mask_park = [&](int t, int nthreads, const uint32_t (&mw)[X::MW2], int n) {
#pragma unroll
    for (int i = 0; i < n; ++i) {
      msk_s[(t / MWR) * XMW + (t % MWR) + i * (nthreads / MWR) * XMW] = mw[i];
    }
  };

  // ---- loader waves: a code path of their own behind a SCALAR branch (`wave` is read through readfirstlane), so that the 128
  // registers that hold the second half of the slice are not live across the compute waves' code; same barrier sequence
  if (loader) {
    const int t2 = tid - XW * 64;
    // two straight-line bodies behind one uniform branch (with / without a second stage): no register is carried through a join
    auto body = [&](auto with2) __attribute__((always_inline)) {
      constexpr bool W2 = decltype(with2)::value;   // W2: nb > XNB, every piece of stage 1 exists
      u32x4 kh1[NP - 1][LCP], kl1[NP - 1][LCP], vh1[NP - 1][LCP], vl1[NP - 1][LCP];
      u32x4 kh2[XCH2], kl2[XCH2], vh2[XCH2], vl2[XCH2];
      uint32_t mw2[X::MW2];
      // pieces 1 .. NP - 1 of stage 1, requested in the order of their use before anything else of this wave goes to memory
#pragma unroll
      for (int p = 1; p < NP; ++p)
        if (W2 || p * PB < nb) {
#pragma unroll
          for (int j = 0; j < LCP; ++j) gload(0, p * PCH + j * XLW * 64, t2, kh1[p - 1][j], kl1[p - 1][j], vh1[p - 1][j], vl1[p - 1][j]);
          __builtin_amdgcn_sched_barrier(0);   // requests return in the order they are issued: keep it the order of use
        }
      __syncthreads();   // (A0) piece 0 parked (by the compute waves)
#pragma unroll
      for (int p = 1; p < NP; ++p)
        if (W2 || p * PB < nb) {   // uniform over the workgroup
#pragma unroll
          for (int j = 0; j < LCP; ++j) park(p * PCH + j * XLW * 64, t2, kh1[p - 1][j], kl1[p - 1][j], vh1[p - 1][j], vl1[p - 1][j]);
          if constexpr (W2) {
            // stage 2 into the registers the piece has left: a quarter behind each piece but the last, the rest behind that one
            // (the scheduler must not lift these requests over the parks: both register sets would be live at once)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = X::s2lo(p); i < X::s2lo(p + 1); ++i) gload(1, i * XLW * 64, t2, kh2[i], kl2[i], vh2[i], vl2[i]);
            if constexpr (MASKB)
              if (p == 1) mask_words(1, t2, XLW * 64, mw2, X::MW2);   // while the fewest registers are live
          }
          __syncthreads();   // (Ap) piece p parked
        }
      if constexpr (W2) {
        // every wave has passed (A NP-1): pieces 0 .. NP - 2 of stage 1 are consumed, their part of stage 2 is parked over them
        // while the last piece is still being read; the rest, and the mask words, after (B)
        constexpr int S2A = (NP - 1) * XCH2 / NP;
        auto park2 = [&](int i) {
          if (i * XLW * 64 / CPR + t2 / CPR < nk - XK) park(i * XLW * 64, t2, kh2[i], kl2[i], vh2[i], vl2[i]);   // rows of the slice only
        };
#pragma unroll
        for (int i = 0; i < S2A; ++i) park2(i);
        __syncthreads();   // (B) every wave is done reading stage 1
#pragma unroll
        for (int i = S2A; i < XCH2; ++i) park2(i);
        if constexpr (MASKB) mask_park(t2, XLW * 64, mw2, X::MW2);
        __syncthreads();   // (C) stage 2 parked
      }
    };
    if (nb > XNB) body(std::true_type{});
    else body(std::false_type{});
    return;
  }
  // ---- compute waves: piece 0 (one chunk of each plane per thread) is requested first -- the q rows, the key-padding bytes and
  // the mask words queue behind it, not in front
  u32x4 qfh[KSD], qfl[KSD];
  {
    u32x4 kh0, kl0, vh0, vl0;
    gload(0, 0, tid, kh0, kl0, vh0, vl0);
    __builtin_amdgcn_sched_barrier(0);   // nothing is lifted in front of these four requests
    X3_TL(1);
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) {   // q row (fp32) -> hi / lo fragments: lane (i, g) holds k = 32 ks + 8 g .. + 7 of query i
      const long qo = (long)b * d.q_sb + (long)min(myq, d.Lq - 1) * d.q_sl + (long)h * d.q_sh + 32 * ks + 8 * lg;
      const float4 a0 = *(const float4*)((const float*)d.q + qo), a1 = *(const float4*)((const float*)d.q + qo + 4);
      const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      x3_split(v, qfh[ks], qfl[ks]);
      if (d.q_bf && split == 0 && qvalid) *(u32x4*)((bf16_t*)d.q_bf + qo) = qfh[ks];
    }
    uint8_t kp[2 * XK / (XW * 64)];
#pragma unroll
    for (int i = 0; i < 2 * XK / (XW * 64); ++i) {
      const int j = tid + i * XW * 64;
      kp[i] = (j < nk && key_lo + j < d.Lk) ? (d.kpm ? d.kpm[(long)b * d.Lk + key_lo + j] : 0) : 1;
    }
    uint32_t mw[X::MW2];
    if constexpr (MASKB) mask_words(0, tid, XW * 64, mw, X::MW1);
#pragma unroll
    for (int i = 0; i < 2 * XK / (XW * 64); ++i) kpm_s[tid + i * XW * 64] = kp[i];
    if constexpr (MASKB) mask_park(tid, XW * 64, mw, X::MW1);
    park(0, tid, kh0, kl0, vh0, vl0);
  }

  // online softmax in the base-2 domain (attn_resident.hip): x2 = s * (scale * log2 e), p = 2^(x2 - m2)
  const float sc2 = d.scale * 1.44269504088896341f;
  const bool zero0 = d.zero_attn && split == 0;   // the zero key (add_zero_attn) is the initial state of split 0 only
  float m = zero0 ? 0.f : -1e30f, l = (zero0 && lg == 0) ? 1.f : 0.f;
  f32x4 acc[A::MT];
#pragma unroll
  for (int mt = 0; mt < A::MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  DropState dst;
  uint32_t drow = 0;
  if constexpr (DROP) {
    dst = drop_init(d.drop, d.drop_bmod > 0 ? b / d.drop_bmod : 0, d.Lk);
    drow = (uint32_t)(((long)(d.drop_bmod > 0 ? b % d.drop_bmod : b) * d.H + h) * d.Lq + min(myq, d.Lq - 1));
  }
  const int qrow = (wave * 16 + li) * XMW;   // this lane's row of the staged mask words
  // t: block inside the resident stage, tg: block inside the key slice
  auto block = [&](int t, int tg) __attribute__((always_inline)) {
    uint32_t mwb[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) mwb[tt] = *(const uint32_t*)&kpm_s[tg * KB + tt * 16 + 4 * lg];
    uint32_t nib[4] = {0u, 0u, 0u, 0u};   // MASKB: the lane's 4 keys of tile tt as a nibble (bit r = key 16 tt + 4 lg + r masked)
    if constexpr (MASKB) {
      const uint32_t w0 = msk_s[qrow + 2 * t], w1 = msk_s[qrow + 2 * t + 1];
      nib[0] = (w0 >> (4 * lg)) & 0xFu; nib[1] = (w0 >> (16 + 4 * lg)) & 0xFu;
      nib[2] = (w1 >> (4 * lg)) & 0xFu; nib[3] = (w1 >> (16 + 4 * lg)) & 0xFu;
      // a block no query of the wave attends to contributes nothing
      bool dead = true;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const uint32_t k4 = ((mwb[tt] & 1u) | ((mwb[tt] >> 7) & 2u) | ((mwb[tt] >> 14) & 4u) | ((mwb[tt] >> 21) & 8u));
        nib[tt] |= k4;
        dead = dead && nib[tt] == 0xFu;
      }
      if (__all((int)dead)) return;
    } else {
      if (__all((mwb[0] & mwb[1] & mwb[2] & mwb[3]) == 0x01010101u)) return;   // fully padded block
    }
    const bf16_t* Kht = Kh + t * KB * LDK;
    const bf16_t* Klt = Kl + t * KB * LDK;
    const bf16_t* Vht = Vh + t * KB * LDV;
    const bf16_t* Vlt = Vl + t * KB * LDV;
    f32x4 sc[4];
    if constexpr (DH == 32) {
      u32x4 kfh[4], kfl[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        kfh[tt] = rfrag<bf16_t>(&Kht[(tt * 16 + li) * LDK], 0, lg);
        kfl[tt] = rfrag<bf16_t>(&Klt[(tt * 16 + li) * LDK], 0, lg);
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        sc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        Mma<bf16_t>::mma(sc[tt], kfl[tt], qfh[0]);
        Mma<bf16_t>::mma(sc[tt], kfh[tt], qfl[0]);
        Mma<bf16_t>::mma(sc[tt], kfh[tt], qfh[0]);
      }
    } else {   // two k steps over d_h: fragments of one key tile at a time (register budget: 168 per wave)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        sc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSD; ++ks) {
          const u32x4 kh_ = rfrag<bf16_t>(&Kht[(tt * 16 + li) * LDK], ks, lg), kl_ = rfrag<bf16_t>(&Klt[(tt * 16 + li) * LDK], ks, lg);
          Mma<bf16_t>::mma(sc[tt], kl_, qfh[ks]);
          Mma<bf16_t>::mma(sc[tt], kh_, qfl[ks]);
          Mma<bf16_t>::mma(sc[tt], kh_, qfh[ks]);
        }
      }
    }
    u32x4 vfh[DH == 32 ? A::MT : 1][2], vfl[DH == 32 ? A::MT : 1][2];
    if constexpr (DH == 32) {
#pragma unroll
      for (int mt = 0; mt < A::MT; ++mt)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          vfh[mt][u] = tfrag_tr(Vht, LDV, u * 32, mt * 16, li, lg);
          vfl[mt][u] = tfrag_tr(Vlt, LDV, u * 32, mt * 16, li, lg);
        }
    }
    if constexpr (MASKB) {
      if (!__all((nib[0] | nib[1] | nib[2] | nib[3]) == 0u)) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int r = 0; r < 4; ++r) sc[tt][r] = ((nib[tt] >> r) & 1u) ? -INFINITY : sc[tt][r];
      }
    } else {
      if (!__all((mwb[0] | mwb[1] | mwb[2] | mwb[3]) == 0u)) {   // padded keys in the block (the tail only): raw score -> -inf
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int r = 0; r < 4; ++r) sc[tt][r] = ((mwb[tt] >> (8 * r)) & 0xffu) ? -INFINITY : sc[tt][r];
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) mx = fmaxf(fmaxf(mx, fmaxf(sc[tt][0], sc[tt][1])), fmaxf(sc[tt][2], sc[tt][3]));
    mx = group_max(mx) * sc2;
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    float p[4][4];
    float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) p[tt][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[tt][r], sc2, -m_new));
      rs0 += p[tt][0] + p[tt][1];
      rs1 += p[tt][2] + p[tt][3];
    }
    l = l * alpha + (rs0 + rs1);   // per-lane partial (alpha is uniform over the query's 4 lanes)
    m = m_new;
    if constexpr (DROP) {   // the softmax denominator keeps every key; only the value contraction sees the mask
      const int k0 = key_lo + tg * KB;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const uint32_t cp = (uint32_t)(k0 + tt * 16 + 4 * lg) >> 1;
        const uint32_t w0 = drop_word(dst, drow, cp), w1 = drop_word(dst, drow, cp + 1);
        p[tt][0] = drop_keep_lo(dst, w0) ? p[tt][0] : 0.f;
        p[tt][1] = drop_keep_hi(dst, w0) ? p[tt][1] : 0.f;
        p[tt][2] = drop_keep_lo(dst, w1) ? p[tt][2] : 0.f;
        p[tt][3] = drop_keep_hi(dst, w1) ? p[tt][3] : 0.f;
      }
    }
    // P as hi + lo bf16 fragments (PackP's layout: k index = tile rows)
    u32x4 pfh[2], pfl[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int tt = 2 * u + hf;
        const uint32_t h0 = pack_bf2(p[tt][0], p[tt][1]), h1 = pack_bf2(p[tt][2], p[tt][3]);
        pfh[u][2 * hf] = h0;
        pfh[u][2 * hf + 1] = h1;
        pfl[u][2 * hf] = pack_bf2(p[tt][0] - __uint_as_float(h0 << 16), p[tt][1] - __uint_as_float(h0 & 0xffff0000u));
        pfl[u][2 * hf + 1] = pack_bf2(p[tt][2] - __uint_as_float(h1 << 16), p[tt][3] - __uint_as_float(h1 & 0xffff0000u));
      }
#pragma unroll
    for (int mt = 0; mt < A::MT; ++mt) {
      acc[mt] *= alpha;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if constexpr (DH == 32) {
          Mma<bf16_t>::mma(acc[mt], vfl[mt][u], pfh[u]);
          Mma<bf16_t>::mma(acc[mt], vfh[mt][u], pfl[u]);
          Mma<bf16_t>::mma(acc[mt], vfh[mt][u], pfh[u]);
        } else {   // value fragments of one 16-column tile at a time
          const u32x4 vh_ = tfrag_tr(Vht, LDV, u * 32, mt * 16, li, lg), vl_ = tfrag_tr(Vlt, LDV, u * 32, mt * 16, li, lg);
          Mma<bf16_t>::mma(acc[mt], vl_, pfh[u]);
          Mma<bf16_t>::mma(acc[mt], vh_, pfl[u]);
          Mma<bf16_t>::mma(acc[mt], vh_, pfh[u]);
        }
      }
    }
  };
#pragma unroll 1
  for (int p = 0; p < NP && (p == 0 || p * PB < nb); ++p) {   // uniform over the workgroup; (A0) always, as in the loader waves
    __syncthreads();   // (Ap) piece p parked
    if (p == 0) X3_TL(2);
    if (wave_active)
      for (int t = p * PB; t < min(nb, (p + 1) * PB); ++t) block(t, t);
  }
  X3_TL(3);
  if (nb > XNB) {   // uniform over the workgroup
    __syncthreads();   // (B)
    __syncthreads();   // (C) the loader waves have parked stage 2 over stage 1
    X3_TL(4);
    if (wave_active)
      for (int t = XNB; t < nb; ++t) block(t - XNB, t);
  }
  X3_TL(5);
  l = group_sum(l);
  if (!qvalid) return;
  constexpr float LN2 = 0.693147180559945309f;
  if (KS == 1) {
    const float inv = (DROP ? dst.scale : 1.f) / l;
    const long oo = (long)b * d.o_sb + (long)myq * d.o_sl + (long)h * d.o_sh + 4 * lg;
#pragma unroll
    for (int mt = 0; mt < A::MT; ++mt) {
      const float4 v = make_float4(acc[mt][0] * inv, acc[mt][1] * inv, acc[mt][2] * inv, acc[mt][3] * inv);
      *(float4*)((float*)d.o + oo + mt * 16) = v;
      if (d.o_bf) *(u32x2*)((bf16_t*)d.o_bf + oo + mt * 16) = (u32x2){pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
    }
    if (lg == 0) d.lse[((long)b * d.H + h) * d.Lq + myq] = m * LN2 + logf(l);
  } else {   // partial softmax state for attention.hip's combine kernel (same layout as the streaming forward)
    const long rows = (long)d.B * d.H * d.Lq, ridx = (((long)split * d.B + b) * d.H + h) * d.Lq + myq;
    float* po = d.ws + ridx * DH;
#pragma unroll
    for (int mt = 0; mt < A::MT; ++mt)
      *(float4*)(po + mt * 16 + 4 * lg) = make_float4(acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]);
    if (lg == 0) {
      d.ws[(long)KS * rows * DH + ridx] = m * LN2;   // natural-log domain, as the combine kernel expects
      d.ws[(long)KS * rows * (DH + 1) + ridx] = l;
    }
  }
  X3_TL(6);
}

template <int DH, bool DROP, bool MASKB> int launch_x3(const pq3d_attn_desc& d, hipStream_t s, int KS, int nqh, int per) {
  typedef X3<DH> X;
  const size_t lds = (size_t)X::XK * (2 * X::LDK * 2 + 2 * X::LDV * 2) + 2 * X::XK + (MASKB ? 128 * X::XMW * 4 : 0) + 16;
  static_assert((size_t)X::XK * (2 * X::LDK * 2 + 2 * X::LDV * 2) + 2 * X::XK + 128 * X::XMW * 4 + 16 <= 160 * 1024, "LDS");
  auto kern = attn_fwd_x3_kernel<DH, DROP, MASKB>;
  static std::atomic<unsigned> attr_done{0};   // > 64 KB of dynamic LDS: opt-in once per (kernel, device)
  if (int e = pq3d_enable_big_lds(kern, 160 * 1024, attr_done)) { pq3d_set_error(hipGetErrorString((hipError_t)e)); return e; }
  hipLaunchKernelGGL(kern, dim3(KS * nqh, d.H, d.B), dim3((XW + XLW) * 64), lds, s, d, KS, per);
  return 0;
}

}  // namespace

// pq3d_attn_fwd with k_lo set (attention.hip routes here; the caller launches the combine kernel for ksplit > 1)
int pq3d_attn_fwd_x3(const pq3d_attn_desc& d, hipStream_t s) {
  PQ_CHECK_ARG(d.dt == PQ3D_F32 && d.k_lo && d.v_lo, "pq3d_attn_fwd (split-bf16 planes): q / o must be fp32, k_lo and v_lo set");
  PQ_CHECK_ARG((d.dh == 32 || d.dh == 64) && !d.bias && d.Lq <= 256 && d.Lk >= 1,
               "pq3d_attn_fwd (split-bf16 planes): d_h = 32 / 64, <= 256 queries, no additive bias");
  PQ_CHECK_ARG(!d.mask || d.mask_bits, "pq3d_attn_fwd (split-bf16 planes): a 3-D mask must come as bit words (pq3d_mask_pack)");
  PQ_CHECK_ARG(!(d.mask && d.kpm), "pq3d_attn_fwd (split-bf16 planes): key padding and a 3-D mask are exclusive");
  PQ_CHECK_ARG(!((d.q_sl | d.q_sb | d.q_sh | d.o_sl | d.o_sb | d.o_sh) & 3) && !((d.k_sl | d.k_sb | d.k_sh | d.v_sl | d.v_sb | d.v_sh) & 7),
               "pq3d_attn_fwd (split-bf16 planes): strides must be multiples of 16 bytes");
  PQ_CHECK_ARG((long)d.Lk * d.k_sl < (1L << 31) - 64 && (long)d.Lk * d.v_sl < (1L << 31) - 64 && d.k_sl >= 0 && d.v_sl >= 0,
               "pq3d_attn_fwd (split-bf16 planes): the key / value rows of a scene must span less than 4 GB");
  PQ_CHECK_ARG(((((uintptr_t)d.k_lo) | ((uintptr_t)d.v_lo) | ((uintptr_t)d.q_bf) | ((uintptr_t)d.o_bf)) & 15) == 0,
               "pq3d_attn_fwd (split-bf16 planes): planes must be 16-byte aligned");
  const int KS = d.ksplit > 1 ? d.ksplit : 1, nkb = (d.Lk + KB - 1) / KB;
  const int xk = d.dh == 32 ? X3<32>::XK : X3<64>::XK;
  PQ_CHECK_ARG(((nkb + KS - 1) / KS) * KB <= 2 * xk, "pq3d_attn_fwd (split-bf16 planes): at most 1024 (d_h = 64: 512) keys per key split");
  const int nqh = (d.Lq + 127) / 128, per = (d.Lq + nqh - 1) / nqh;
  const bool dr = d.drop.p > 0.f && d.drop.seed, mb = d.mask != nullptr;
  if (d.dh == 32) {
    if (dr) return mb ? launch_x3<32, true, true>(d, s, KS, nqh, per) : launch_x3<32, true, false>(d, s, KS, nqh, per);
    return mb ? launch_x3<32, false, true>(d, s, KS, nqh, per) : launch_x3<32, false, false>(d, s, KS, nqh, per);
  }
  if (dr) return mb ? launch_x3<64, true, true>(d, s, KS, nqh, per) : launch_x3<64, true, false>(d, s, KS, nqh, per);
  return mb ? launch_x3<64, false, true>(d, s, KS, nqh, per) : launch_x3<64, false, false>(d, s, KS, nqh, per);
}
