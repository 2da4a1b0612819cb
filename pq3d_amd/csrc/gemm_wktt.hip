// Weight-gradient products of the query side, dW[N_out, K_in] += g^T (x [+ x2]) over R = B*N_q rows, with whole-K-chunk
// tiles: the TT layout (both operands k-major: A = g [R][N_out], B = x [R][K_in]) of pq3d_gemm for reductions of a few
// hundred rows.  The 64x64-tile pipeline kernel walks such a reduction in 64-row steps -- 800 rows = 13 dependent
// (load -> convert -> LDS -> barrier -> MFMA -> barrier) steps split over 2-4 workgroups: the five flush launches of a config-2
// backward took 112 us for 10.9 GFLOP.  Here a workgroup of 8 waves stages 256 reduction rows of both operands at once
// (all loads of the chunk in flight together, converted to bf16 once, [k][m] / [k][n] tiles read back with the transposing
// LDS read) and issues the chunk's MFMAs back to back; the next chunk's loads fly during them.  Split-K with atomics into
// the pre-zeroed gradient arena (its own split factor: one round of workgroups), fused bias gradient (column sums of g on
// the matrix pipe, as gemm_fast_kernel).  Single-bf16 operands (every backward product of the path), fp32 accumulate.
#include <atomic>
#include <cstdlib>

#include "gemm_common.h"

namespace {

constexpr int WT = 512;

// TT = tile edge (64 or 128: 128-wide tiles halve the operand re-reads from L2, which bound these products at 64 -- each
// g tile is re-read by every n tile and each x tile by every m tile), KC = reduction rows staged per chunk (256 / 128)
template <typename TA, typename TB, bool HB2, int KC, int TT>
__global__ __launch_bounds__(WT) void gemm_wktt_kernel(const pq3d_kdesc d, const int sk) {
#define WKTT_K d.K
#include "gemm_wktt_body.h"
#undef WKTT_K
}

// Groups with reduction lengths of their own (pq3d_gemm_desc.Kg: one [M, N] over different row counts, the encoders' weight
// gradients): every group's chunks are split over the launch's sk slices.  Its own kernel over the same body text, so that the
// uniform kernel above keeps its arguments and its code.
struct TtKg { int32_t K[PQ3D_MAX_GROUPS]; };
template <typename TA, typename TB, int KC, int TT>
__global__ __launch_bounds__(WT) void gemm_wktt_kg_kernel(const pq3d_kdesc d, const int sk, const TtKg kg) {
  constexpr bool HB2 = false;
  const int kg_K = kg.K[min((int)(blockIdx.z / sk), PQ3D_MAX_GROUPS - 1)];
#define WKTT_K kg_K
#include "gemm_wktt_body.h"
#undef WKTT_K
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <typename TA, typename TB, bool HB2, int KC, int TT>
int tt_launch_t(const pq3d_gemm_desc& d, const pq3d_kdesc& kd, hipStream_t s) {
  auto kern = gemm_wktt_kernel<TA, TB, HB2, KC, TT>;
  constexpr size_t lds = 2 * (size_t)KC * (TT + 8) * sizeof(bf16_t);
  static std::atomic<unsigned> done{0};
  if (int e = pq3d_enable_big_lds(kern, (int)lds, done)) return e;
  bool ragged = false;
  for (int g = 0; g < PQ3D_MAX_GROUPS; ++g) ragged = ragged || d.Kg[g] != 0;
  // split factor of this kernel: as many KC-row chunks side by side as keep the launch within one round of workgroups
  // (two ~70 KB workgroups per CU)
  const long tiles = (long)((d.M + TT - 1) / TT) * ((d.N + TT - 1) / TT) * d.groups;
  const int nck = (d.K + KC - 1) / KC;
  int sk = (int)(512 / (tiles > 0 ? tiles : 1));
  if (sk < 1) sk = 1;
  if (sk > nck) sk = nck;
  const dim3 grid((d.M + TT - 1) / TT, (d.N + TT - 1) / TT, d.groups * sk);
  pq3d_kdesc k2 = kd;
  const long kl = ((long)(nck + sk - 1) / sk) * KC;   // reduction rows of one workgroup
  k2.xcd_order = plane_xcd_order((int)grid.x, (int)grid.y, (long)TT * kl * (long)sizeof(TA), (long)TT * kl * (long)(sizeof(TB) + (HB2 ? 4 : 0)));
  if (ragged) {
    if constexpr (!HB2) {
      auto kern_kg = gemm_wktt_kg_kernel<TA, TB, KC, TT>;
      static std::atomic<unsigned> done_kg{0};
      if (int e = pq3d_enable_big_lds(kern_kg, (int)lds, done_kg)) return e;
      TtKg kg;
      for (int g = 0; g < PQ3D_MAX_GROUPS; ++g) kg.K[g] = d.Kg[g];
      hipLaunchKernelGGL(kern_kg, grid, dim3(WT), lds, s, k2, sk, kg);
      return 0;
    }
    return (int)hipErrorInvalidValue;   // (pq3d_gemm_wktt_try refuses B2 with Kg)
  }
  hipLaunchKernelGGL(kern, grid, dim3(WT), lds, s, k2, sk);
  return 0;
}
template <typename TA, typename TB, bool HB2>
int tt_launch(const pq3d_gemm_desc& d, const pq3d_kdesc& kd, hipStream_t s) {
  // 64 x 64 tiles, 256 reduction rows per chunk.  (128 x 128 tiles over 128-row chunks -- the same 70 KB of LDS, half the
  // operand re-reads from L2 -- were measured slower at config 2: flush launches 25-33 us against 15-25, one 178-VGPR
  // workgroup per CU and four times the atomics per tile; the instantiation is not built any more)
  return tt_launch_t<TA, TB, HB2, 256, 64>(d, kd, s);
}

}  // namespace

// Returns true when the whole-K weight-gradient kernel took the launch (*err = 0 or a hipError_t), false when the call is
// outside its domain.  The caller has zero-filled C (or accumulates on purpose).
bool pq3d_gemm_wktt_try(const pq3d_gemm_desc& d, const pq3d_kdesc& kd, hipStream_t s, int* err) {
  *err = 0;
  if (!(d.transA && d.transB) || d.ct != PQ3D_BF16 || d.batch != 1 || d.kconcat > 1 || d.splitk < 2 || d.dtC != PQ3D_F32) return false;
  if (d.M < 8 || d.N < 8 || d.M % 8 || d.N % 8 || d.lda % 8 || d.ldb % 8 || d.K < 1) return false;
  if (d.ldc != d.N) return false;
  // this kernel has no epilogue beyond alpha and the fused column sums: anything else belongs to the pipeline kernel
  if (d.act || d.act_grad || d.row_scale || d.row_fill_flag || d.mask_out || (d.drop.p > 0.f && d.drop.seed)) return false;
  for (int g = 0; g < d.groups; ++g)
    if (d.bias[g] || d.aux[g] || d.C2[g] || d.row_mask[g]) return false;
  // long reductions over bf16 x bf16 operands (the K/V projections' weight gradients) belong to the 128x128-tile kernel
  if (d.dtA == PQ3D_BF16 && d.dtB == PQ3D_BF16 && d.K >= 2048) return false;
  bool b2 = false;
  for (int g = 0; g < d.groups; ++g) {
    if (!d.A[g] || !d.B[g] || !d.C[g] || !al16(d.A[g]) || !al16(d.B[g]) || d.A2[g]) return false;
    if (d.B2[g] && d.Kg[0]) return false;   // per-group reduction lengths: no second B operand
    if (d.B2[g]) { b2 = true; if (!al16(d.B2[g]) || d.dtB2 != PQ3D_F32 || d.dtB != PQ3D_F32) return false; }
  }
  int e;
  const bool af = d.dtA == PQ3D_F32, bf = d.dtB == PQ3D_F32;
  if (b2) e = af ? tt_launch<float, float, true>(d, kd, s) : tt_launch<bf16_t, float, true>(d, kd, s);
  else if (af && bf) e = tt_launch<float, float, false>(d, kd, s);
  else if (af) e = tt_launch<float, bf16_t, false>(d, kd, s);
  else if (bf) e = tt_launch<bf16_t, float, false>(d, kd, s);
  else e = tt_launch<bf16_t, bf16_t, false>(d, kd, s);
  if (e) { pq3d_set_error(hipGetErrorString((hipError_t)e)); *err = e; }
  return true;
}
