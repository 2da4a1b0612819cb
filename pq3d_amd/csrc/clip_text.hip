// Device pieces of the CLIP text prompt encoder (pq3d_amd/clip_text.py; reference: modules/language/clip.py driving HF
// CLIPTextModelWithProjection, frozen -- forward only) that the GEMM / LayerNorm kernels do not cover:
//   pq3d_clip_embed       x[n, t] = token_embedding[ids[n, t]] + position_embedding[t]   (out-of-vocabulary ids are clamped)
//   pq3d_attn_causal_fwd  causal self-attention with an arbitrary per-key validity mask for T <= 77 tokens, d_h = 64, reading q, k, v
//                         from the packed output of one [3 d, d] projection; one workgroup per (prompt, head)
//   pq3d_l2norm_rows      F.normalize(p = 2) of every row
// The attention kernel follows the lessons recorded at the top of attn_small.hip: tiles are swept into LDS / registers with all
// loads in flight first, every thread carries independent accumulator chains, wave reductions are DPP / lane-swap moves.
#include "common.h"

namespace {

inline unsigned grid_of(long total, long cap = 4096) {
  long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}
inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// ---- token + position embedding: one thread per 4 channels --------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_embed_kernel(const void* __restrict__ tok, const void* __restrict__ pos,
                                                         const int64_t* __restrict__ ids, void* __restrict__ x, long rows, int T,
                                                         int d, long vocab, int dt_tab, int dt_out) {
  const int d4 = d >> 2;
  const long total = rows * d4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / d4;
    const int c = (int)(i - r * d4) * 4, t = (int)(r % T);
    long id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // clamped: no bounds fault on a bad token id
    float a[4], b[4];
    load_elems<4>(tok, dt_tab, id * d + c, 4, a);
    load_elems<4>(pos, dt_tab, (long)t * d + c, 4, b);
    if (dt_out == PQ3D_F32) {
      *(float4*)((float*)x + r * d + c) = make_float4(a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]);
    } else {
      *(u32x2*)((bf16_t*)x + r * d + c) = (u32x2){pack_bf2(a[0] + b[0], a[1] + b[1]), pack_bf2(a[2] + b[2], a[3] + b[3])};
    }
  }
}

// ---- causal self-attention, short sequences ---------------------------------------------------------------------------
// One workgroup (256 threads) per (prompt, head).  LDS: K [TR][64], V [TR][64] (TR = T rounded up to 4; fp32), the score /
// probability tile S [T][LS] and 1 / rowsum.
//   scores  : thread owns query row i (its 64 q values in registers, read once from global) and every NG-th key j <= i; the K
//             rows come from LDS as wave-wide broadcasts; two keys per step = two independent accumulator chains of packed FMAs.
//             Only the causal triangle is formed; validity is applied by the softmax.
//   softmax : one wave per row, two keys per lane; a row without a visible key gets p = 0 and 1 / rowsum = 0 (-> zeros out)
//   O = P V : lane owns channel c, the wave owns rows w, w + 4, ...; RB rows at a time share every V read (P rows are broadcast
//             float4 reads), and only keys up to the block's last row are visited.
constexpr int CA_DH = 64, CA_NT = 256, CA_RB = 4;
typedef float ca_f32x2 __attribute__((ext_vector_type(2)));

PQ_DEV float ca_dot(const float* krow, const float (&q)[CA_DH]) {   // krow: LDS, one address per wave (or two): broadcast
  ca_f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
  for (int x = 0; x < CA_DH; x += 4) {
    const float4 t = *(const float4*)&krow[x];
    a0 = __builtin_elementwise_fma((ca_f32x2){t.x, t.y}, (ca_f32x2){q[x], q[x + 1]}, a0);
    a1 = __builtin_elementwise_fma((ca_f32x2){t.z, t.w}, (ca_f32x2){q[x + 2], q[x + 3]}, a1);
  }
  const ca_f32x2 s = a0 + a1;
  return s.x + s.y;
}

__global__ __launch_bounds__(CA_NT) void attn_causal_fwd_kernel(const void* __restrict__ qkv, const uint8_t* __restrict__ valid,
                                                                void* __restrict__ out, int T, int H, int dt, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int TR = (T + 3) & ~3, LS = TR + 4;   // float4-readable probability rows, bank-shifted
  float* Ks = sm;                 // [TR][64]
  float* Vs = Ks + TR * CA_DH;    // [TR][64]
  float* S = Vs + TR * CA_DH;     // [T][LS]
  float* Li = S + T * LS;         // [T]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, n = blockIdx.y;
  const int dm = H * CA_DH;
  const long row0 = (long)n * T;          // first token row of this prompt
  const long ld = 3L * dm;                // elements per token in qkv
  const long qoff = (long)h * CA_DH, koff = dm + qoff, voff = 2L * dm + qoff;

  // ---- K and V into LDS: 16 chunks of 8 elements per token and operand, U chunks in flight per thread
  {
    constexpr int U = 4;
    const int nc = TR * 8;   // chunks per operand (tail rows are zero-filled)
    for (int base = tid; base < 2 * nc; base += CA_NT * U) {
      float v[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = min(base + u * CA_NT, 2 * nc - 1), op = e >= nc, cc = e - op * nc, t = cc >> 3, x = (cc & 7) * 8;
        load_elems<8>(qkv, dt, (row0 + min(t, T - 1)) * ld + (op ? voff : koff) + x, 8, v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = base + u * CA_NT;
        if (e < 2 * nc) {
          const int op = e >= nc, cc = e - op * nc, t = cc >> 3, x = (cc & 7) * 8;
          float* dst = (op ? Vs : Ks) + t * CA_DH + x;
          const bool in = t < T;
          *(float4*)dst = in ? make_float4(v[u][0], v[u][1], v[u][2], v[u][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
          *(float4*)(dst + 4) = in ? make_float4(v[u][4], v[u][5], v[u][6], v[u][7]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
  }
  // ---- this thread's query row (registers) and its two keys' validity bits (softmax phase: lane <-> key)
  const int TP = (T + 15) & ~15, NG = CA_NT / TP;   // T <= 77: TP <= 80, NG >= 3
  const int i = tid % TP, jg = tid / TP;
  float q[CA_DH];
  {
    const long qb = (row0 + min(i, T - 1)) * ld + qoff;
#pragma unroll
    for (int x = 0; x < CA_DH; x += 8) {
      float t8[8];
      load_elems<8>(qkv, dt, qb + x, 8, t8);
#pragma unroll
      for (int u = 0; u < 8; ++u) q[x + u] = t8[u];
    }
  }
  const bool v0 = lane < T && (!valid || valid[row0 + lane] != 0);
  const bool v1 = lane + 64 < T && (!valid || valid[row0 + lane + 64] != 0);
  __syncthreads();
  // ---- scores of the causal triangle
  if (i < T && jg < NG) {
    for (int j = jg; j <= i; j += 2 * NG) {
      const int j2 = j + NG;
      const float s0 = ca_dot(&Ks[j * CA_DH], q);
      const float s1 = ca_dot(&Ks[min(j2, T - 1) * CA_DH], q);
      S[i * LS + j] = s0 * scale;
      if (j2 <= i) S[i * LS + j2] = s1 * scale;
    }
  }
  __syncthreads();
  // ---- row softmax over the visible keys: one wave per row
  for (int r = wave; r < T; r += CA_NT / 64) {
    const bool w0 = v0 && lane <= r, w1 = v1 && lane + 64 <= r;
    const float a0 = w0 ? S[r * LS + lane] : -INFINITY, a1 = w1 ? S[r * LS + lane + 64] : -INFINITY;
    const float m = wave_max(fmaxf(a0, a1));
    const float e0 = w0 ? __expf(a0 - m) : 0.f, e1 = w1 ? __expf(a1 - m) : 0.f;
    const float l = wave_sum(e0 + e1);
    if (lane < LS) S[r * LS + lane] = e0;            // masked and padding columns: 0 (read times V by the float4 loop)
    if (lane + 64 < LS) S[r * LS + lane + 64] = e1;
    if (lane == 0) Li[r] = l > 0.f ? 1.f / l : 0.f;   // no visible key: zeros
  }
  __syncthreads();
  // ---- O = P V
  const int c = lane;
  for (int rb = wave; rb < T; rb += 4 * CA_RB) {     // rows rb, rb + 4, ..., rb + 4 (RB - 1)
    const int last = min(rb + 4 * (CA_RB - 1), T - 1);
    const int jend = (last + 4) & ~3;                // keys [0, last] rounded up to 4 (<= TR; P is 0 past each row's own index)
    ca_f32x2 ac0[CA_RB], ac1[CA_RB];
#pragma unroll
    for (int r = 0; r < CA_RB; ++r) { ac0[r] = (ca_f32x2){0.f, 0.f}; ac1[r] = (ca_f32x2){0.f, 0.f}; }
    for (int jj = 0; jj < jend; jj += 4) {
      float vv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) vv[u] = Vs[(jj + u) * CA_DH + c];
      float4 p[CA_RB];
#pragma unroll
      for (int r = 0; r < CA_RB; ++r) p[r] = *(const float4*)&S[min(rb + 4 * r, T - 1) * LS + jj];
#pragma unroll
      for (int r = 0; r < CA_RB; ++r) {
        ac0[r] = __builtin_elementwise_fma((ca_f32x2){p[r].x, p[r].y}, (ca_f32x2){vv[0], vv[1]}, ac0[r]);
        ac1[r] = __builtin_elementwise_fma((ca_f32x2){p[r].z, p[r].w}, (ca_f32x2){vv[2], vv[3]}, ac1[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < CA_RB; ++r) {
      const int row = rb + 4 * r;
      if (row < T) {
        const ca_f32x2 t = ac0[r] + ac1[r];
        store_elem(out, dt, (row0 + row) * dm + qoff + c, (t.x + t.y) * Li[row]);
      }
    }
  }
}

inline size_t attn_causal_lds(int T) {
  const int TR = (T + 3) & ~3, LS = TR + 4;
  return ((size_t)2 * TR * CA_DH + (size_t)T * LS + T) * sizeof(float);
}

// ---- row L2 normalisation: one wave per row ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const void* __restrict__ x, void* __restrict__ y, long R, int d, int dt_x,
                                                          int dt_y, float eps) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;   // whole waves leave together
  const long base = r * d;
  float ss = 0.f;
  for (int c0 = lane * 4; c0 < d; c0 += 256) {
    float v[4];
    load_elems<4>(x, dt_x, base + c0, d - c0, v);
    ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  const float inv = 1.f / fmaxf(sqrtf(wave_sum(ss)), eps);
  for (int c0 = lane * 4; c0 < d; c0 += 256) {
    float v[4];
    load_elems<4>(x, dt_x, base + c0, d - c0, v);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c0 + u < d) store_elem(y, dt_y, base + c0 + u, v[u] * inv);
  }
}

std::atomic<unsigned> g_causal_big_lds{0};

}  // namespace

extern "C" int pq3d_clip_embed(const void* tok, const void* pos, const int64_t* ids, void* x, int64_t n, int32_t T, int32_t d,
                               int64_t vocab, int32_t dt_tab, int32_t dt_out, void* stream) {
  PQ_DEVICE_GUARD(stream, x);
  PQ_CHECK_ARG(tok && pos && ids && x && n >= 0 && T >= 1 && d >= 4 && (d % 4) == 0 && vocab >= 1,
               "pq3d_clip_embed: bad args (d % 4 == 0, vocab >= 1)");
  PQ_CHECK_ARG((dt_tab == PQ3D_F32 || dt_tab == PQ3D_BF16) && (dt_out == PQ3D_F32 || dt_out == PQ3D_BF16), "pq3d_clip_embed: bad dtype");
  PQ_CHECK_ARG(al16(tok) && al16(pos) && al16(x), "pq3d_clip_embed: tables and output must be 16-byte aligned");
  if (n == 0) return 0;
  const long rows = (long)n * T;
  hipLaunchKernelGGL(clip_embed_kernel, dim3(grid_of(rows * (d / 4))), dim3(256), 0, (hipStream_t)stream, tok, pos, ids, x, rows,
                     (int)T, (int)d, (long)vocab, (int)dt_tab, (int)dt_out);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_attn_causal_fwd(const void* qkv, const uint8_t* valid, void* out, int32_t n, int32_t T, int32_t H, int32_t dt,
                                    float scale, void* stream) {
  PQ_DEVICE_GUARD(stream, qkv);
  PQ_CHECK_ARG(qkv && out && n >= 0 && H >= 1 && H <= 65535 && n <= 65535, "pq3d_attn_causal_fwd: bad args");
  PQ_CHECK_ARG(T >= 1 && T <= PQ3D_ATTN_CAUSAL_MAX_T, "pq3d_attn_causal_fwd: T must be in [1, 77] (K, V and the scores of one head live in LDS)");
  PQ_CHECK_ARG(dt == PQ3D_F32 || dt == PQ3D_BF16, "pq3d_attn_causal_fwd: bad dtype");
  PQ_CHECK_ARG(al16(qkv) && al16(out), "pq3d_attn_causal_fwd: qkv and out must be 16-byte aligned");
  if (n == 0) return 0;
  const size_t lds = attn_causal_lds(T);
  if (lds > 64 * 1024) {
    if (int e = pq3d_enable_big_lds(attn_causal_fwd_kernel, (int)lds, g_causal_big_lds)) {
      pq3d_set_error(hipGetErrorString((hipError_t)e));
      return e;
    }
  }
  hipLaunchKernelGGL(attn_causal_fwd_kernel, dim3(H, n), dim3(CA_NT), lds, (hipStream_t)stream, qkv, valid, out, (int)T, (int)H,
                     (int)dt, scale);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_l2norm_rows(const void* x, void* y, int64_t R, int32_t d, int32_t dt_x, int32_t dt_y, float eps, void* stream) {
  PQ_DEVICE_GUARD(stream, x);
  PQ_CHECK_ARG(x && y && R >= 0 && d >= 1 && eps > 0.f, "pq3d_l2norm_rows: bad args");
  PQ_CHECK_ARG((dt_x == PQ3D_F32 || dt_x == PQ3D_BF16) && (dt_y == PQ3D_F32 || dt_y == PQ3D_BF16), "pq3d_l2norm_rows: bad dtype");
  PQ_CHECK_ARG((R + 3) / 4 <= 0x7fffffffL, "pq3d_l2norm_rows: too many rows");
  if (R == 0) return 0;
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (long)R, (int)d,
                     (int)dt_x, (int)dt_y, eps);
  PQ_LAUNCH_CHECK();
  return 0;
}
