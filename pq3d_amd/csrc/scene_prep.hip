// Scene preparation for instance segmentation: what the reference's dataloader does per scene on the host with
// MinkowskiEngine and fpsample (data/datasets/sceneverse_instseg.py get_scene / sample_query), for a batch of ragged scenes:
//   * pq3d_voxelize: q = floor(x / voxel_size) with the correctly rounded fp32 division, equal (scene, q) grouped by an
//     open-addressing hash table in global memory (slot claimed with atomicCAS, representative = atomicMin of the point
//     index), voxels numbered by the exclusive prefix sum of "point i is its voxel's representative".  Which thread wins a
//     slot decides only WHERE a voxel sits in the table, never an output.
//   * pq3d_fps_scene: exact farthest point sampling of whole scenes (N up to 2^20), one workgroup per scene and no
//     communication between workgroups.  The cloud is streamed as {x, y, z, dist} rows from an L2-resident workspace,
//     sorted by a Morton key so that a tile of consecutive rows is spatially compact; per tile its owner lane keeps the
//     bounding box, the maximum dist and its arg-max in registers, and a step re-scans only the tiles the new sample can
//     change.
// The scene tables (row offsets) are host arrays: they travel to the kernels by value as kernel arguments.
#include "common.h"
#include "ragged.h"

#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------ voxelize
constexpr int VOX_BIAS = 1 << 19;                // sparse._pack: 20-bit fields
constexpr int VOX_QLIM = VOX_BIAS - 8;           // CoordPyramid's range: -2^19 + 8 <= q < 2^19 - 8
constexpr int VOX_ITEMS = PQ3D_VOXELIZE_BLOCK / 256;   // consecutive points per thread of the count / emit kernels
constexpr unsigned long long VOX_EMPTY = ~0ull;  // no packed key has bit 63 set (scene < 8)

typedef SceneTable<PQ3D_VOXELIZE_MAX_SCENES> VoxScenes;

// q = floor(x / vs): IEEE division (the build has no fast-math and -ffp-contract=off; x * (1 / vs) differs on lattice points).
// Returns 0 or the error bits: 1 non-finite, 2 outside [-VOX_QLIM, VOX_QLIM).
PQ_DEV int vox_quantize(const float* __restrict__ p, float vs, int (&q)[3]) {
  int err = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = floorf(__fdiv_rn(p[a], vs));
    if (!(fabsf(f) <= FLT_MAX)) err |= 1;                                  // NaN or +-inf
    else if (f < (float)-VOX_QLIM || f >= (float)VOX_QLIM) err |= 2;
    else q[a] = (int)f;
  }
  return err;
}

PQ_DEV unsigned long long vox_pack(int b, const int (&q)[3]) {
  return ((unsigned long long)b << 60) | ((unsigned long long)(q[2] + VOX_BIAS) << 40) |
         ((unsigned long long)(q[1] + VOX_BIAS) << 20) | (unsigned long long)(q[0] + VOX_BIAS);
}

PQ_DEV unsigned vox_hash(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return (unsigned)k;
}

__global__ void vox_init_kernel(unsigned long long* __restrict__ keys, int* __restrict__ rep, long cap, long long* __restrict__ meta,
                                int nmeta) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nmeta) meta[i] = 0;
  for (long k = i; k < cap; k += (long)gridDim.x * blockDim.x) { keys[k] = VOX_EMPTY; rep[k] = INT_MAX; }
}

__global__ __launch_bounds__(256) void vox_insert_kernel(const float* __restrict__ xyz, VoxScenes sc, long P, float vs,
                                                         unsigned long long* __restrict__ keys, int* __restrict__ rep,
                                                         unsigned mask, int* __restrict__ slot, int* __restrict__ err) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  int q[3];
  const int e = vox_quantize(xyz + i * 3, vs, q);
  if (e) { atomicOr(err, e); slot[i] = -1; return; }
  const unsigned long long key = vox_pack(sc.scene(i), q);
  unsigned h = vox_hash(key) & mask;
  int found = -1;
  // the table holds at most P <= (mask + 1) / 2 keys, so a free or matching slot exists; the probe count is bounded anyway
  for (unsigned probe = 0; probe <= mask; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[h], VOX_EMPTY, key);
    if (prev == VOX_EMPTY || prev == key) { found = (int)h; break; }
    h = (h + 1) & mask;
  }
  slot[i] = found;
  if (found >= 0) atomicMin(&rep[found], (int)i);
  else atomicOr(err, 4);
}

PQ_DEV bool vox_is_rep(const int* __restrict__ slot, const int* __restrict__ rep, long i) {
  const int s = slot[i];
  return s >= 0 && rep[s] == (int)i;
}

__global__ __launch_bounds__(256) void vox_count_kernel(const int* __restrict__ slot, const int* __restrict__ rep, long P,
                                                        int* __restrict__ bsum) {
  __shared__ int lds[SCAN_LDS];
  const long i0 = (long)blockIdx.x * PQ3D_VOXELIZE_BLOCK + (long)threadIdx.x * VOX_ITEMS;
  int c = 0;
#pragma unroll
  for (int j = 0; j < VOX_ITEMS; ++j)
    if (i0 + j < P) c += vox_is_rep(slot, rep, i0 + j) ? 1 : 0;
  int total;
  block_excl_scan(c, lds, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum[0 .. nblk) -> its exclusive prefix sums in place; meta[B] = the number of voxels
__global__ __launch_bounds__(1024) void vox_scan_kernel(int* __restrict__ bsum, int nblk, long long* __restrict__ meta, int B) {
  __shared__ int lds[SCAN_LDS];
  const int per = (nblk + 1023) / 1024, k0 = threadIdx.x * per, k1 = min(k0 + per, nblk);
  int c = 0;
  for (int k = k0; k < k1; ++k) c += bsum[k];
  int total;
  int run = block_excl_scan(c, lds, total);
  for (int k = k0; k < k1; ++k) { const int v = bsum[k]; bsum[k] = run; run += v; }
  if (threadIdx.x == 0) meta[B] = total;
}

__global__ __launch_bounds__(256) void vox_emit_kernel(const float* __restrict__ xyz, VoxScenes sc, long P, float vs,
                                                       const int* __restrict__ slot, const int* __restrict__ rep,
                                                       const int* __restrict__ bpre, int* __restrict__ pv,
                                                       int64_t* __restrict__ unique_map, int32_t* __restrict__ vcoord,
                                                       long long* __restrict__ meta) {
  __shared__ int lds[SCAN_LDS];
  const long i0 = (long)blockIdx.x * PQ3D_VOXELIZE_BLOCK + (long)threadIdx.x * VOX_ITEMS;
  bool f[VOX_ITEMS];
  int c = 0;
#pragma unroll
  for (int j = 0; j < VOX_ITEMS; ++j) {
    f[j] = i0 + j < P && vox_is_rep(slot, rep, i0 + j);
    c += f[j] ? 1 : 0;
  }
  int total;
  int vid = bpre[blockIdx.x] + block_excl_scan(c, lds, total);
#pragma unroll
  for (int j = 0; j < VOX_ITEMS; ++j) {
    const long i = i0 + j;
    if (i >= P) break;
    const int b = sc.scene(i);
    if (i == sc.off[b]) meta[b] = vid;      // the first point of a scene is the representative of the scene's first voxel
    if (f[j]) {
      int q[3] = {0, 0, 0};
      vox_quantize(xyz + i * 3, vs, q);
      pv[i] = vid;
      unique_map[vid] = i - sc.off[b];
      vcoord[(long)vid * 4 + 0] = b; vcoord[(long)vid * 4 + 1] = q[0]; vcoord[(long)vid * 4 + 2] = q[1];
      vcoord[(long)vid * 4 + 3] = q[2];
      ++vid;
    }
  }
}

__global__ __launch_bounds__(256) void vox_inverse_kernel(VoxScenes sc, long P, const int* __restrict__ slot,
                                                          const int* __restrict__ rep, const int* __restrict__ pv,
                                                          const long long* __restrict__ meta, int64_t* __restrict__ inverse_map) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int s = slot[i];
  inverse_map[i] = s < 0 ? -1 : (int64_t)pv[rep[s]] - meta[sc.scene(i)];
}

// ----------------------------------------------------------------------------------------------------------------- FPS
constexpr int FPS_NT = 1024, FPS_NW = FPS_NT / 64;
constexpr int FPS_MAX_TILES = 1024;      // one tile per thread of the scene's workgroup
constexpr int FPS_TILE_SMALL = 256, FPS_TILE_BIG = 1024;     // rows per tile: N <= 2^18 / N <= 2^20

struct FpsScenes : SceneTable<PQ3D_FPS_MAX_SCENES> {     // off: caller rows of scene b
  int T;                                       // rows per tile
  int row0[PQ3D_FPS_MAX_SCENES + 1];           // first workspace row of scene b (a multiple of T); row0[B] = all rows
};

PQ_DEV float fps_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
PQ_DEV float fps_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// per-scene bounding box -> bbox[b][6] = {min xyz, max xyz}
__global__ __launch_bounds__(FPS_NT) void fps_bbox_kernel(const float* __restrict__ pts, FpsScenes sc, float* __restrict__ bbox) {
  __shared__ float red[6][FPS_NW];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n = sc.off[b + 1] - sc.off[b];
  const float* p = pts + sc.off[b] * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long k = threadIdx.x; k < n; k += FPS_NT)
#pragma unroll
    for (int a = 0; a < 3; ++a) { const float v = p[k * 3 + a]; lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v); }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = fps_wave_min(lo[a]); hi[a] = fps_wave_max(hi[a]);
    if (lane == 0) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < FPS_NW; ++w) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    bbox[b * 6 + threadIdx.x] = v;
  }
}

PQ_DEV unsigned fps_spread3(unsigned v) {     // 10 bits -> every third bit
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// sort key of caller row i: scene, then the 30-bit Morton code of its position in the scene's bounding box.  The key only
// decides which rows share a tile (how much the pruning saves), never a result.
__global__ __launch_bounds__(256) void fps_key_kernel(const float* __restrict__ pts, FpsScenes sc, const float* __restrict__ bbox,
                                                      int64_t* __restrict__ keys) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= sc.off[sc.B]) return;
  const int b = sc.scene(i);
  unsigned code = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = bbox[b * 6 + a], ext = bbox[b * 6 + 3 + a] - lo;
    float t = ext > 0.f ? (pts[i * 3 + a] - lo) / ext * 1023.f : 0.f;
    t = fminf(fmaxf(t, 0.f), 1023.f);          // (NaN -> 0: fmaxf returns the other operand)
    code |= fps_spread3((unsigned)(int)t) << a;
  }
  keys[i] = ((int64_t)b << 32) | (int64_t)code;
}

// one workgroup per tile: rows of the workspace in sorted order {x, y, z, dist = +inf}, their caller indices, the tile's box.
// Rows past the scene's end are padding: dist = -1 (never an arg-max: real distances are >= 0), caller index INT_MAX.
__global__ __launch_bounds__(256) void fps_stage_kernel(const float* __restrict__ pts, FpsScenes sc, const int64_t* __restrict__ perm,
                                                        float4* __restrict__ ws, int* __restrict__ cidx,
                                                        float* __restrict__ tilebox) {
  __shared__ float red[6][4];
  const int T = sc.T, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row_t = (long)blockIdx.x * T;
  int b = 0;
  while (b + 1 < sc.B && row_t >= sc.row0[b + 1]) ++b;
  const long n = sc.off[b + 1] - sc.off[b];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = threadIdx.x; k < T; k += 256) {
    const long row = row_t + k, r = row - sc.row0[b];     // r: rank of the row inside its scene
    float4 v = make_float4(0.f, 0.f, 0.f, -1.f);
    int ci = INT_MAX;
    if (r < n) {
      const long src = perm[sc.off[b] + r] - sc.off[b];
      if (src >= 0 && src < n) {                           // (a permutation that leaves the scene gives a padding row)
        const float* p = pts + (sc.off[b] + src) * 3;
        v = make_float4(p[0], p[1], p[2], INFINITY);
        ci = (int)src;
        lo[0] = fminf(lo[0], v.x); lo[1] = fminf(lo[1], v.y); lo[2] = fminf(lo[2], v.z);
        hi[0] = fmaxf(hi[0], v.x); hi[1] = fmaxf(hi[1], v.y); hi[2] = fmaxf(hi[2], v.z);
      }
    }
    ws[row] = v;
    cidx[row] = ci;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = fps_wave_min(lo[a]); hi[a] = fps_wave_max(hi[a]);
    if (lane == 0) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < 4; ++w) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    tilebox[(long)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

// reductions over the 64 lanes of a wave / over each row of 16 lanes with DPP moves (common.h's wave_max): no LDS round trips
PQ_DEV int fps_dpp_i(int x, int which) { return __float_as_int(dpp_xor_f(__int_as_float(x), which)); }
PQ_DEV float fps_row_max(float v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v = fmaxf(v, dpp_xor_f(v, k));
  return v;
}
PQ_DEV int fps_row_min(int v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v = min(v, fps_dpp_i(v, k));
  return v;
}
PQ_DEV int fps_wave_min_i(int v) {
  v = fps_row_min(v);
  u32pair_s a = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  v = min((int)a[0], (int)a[1]);
  u32pair_s b = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  return min((int)b[0], (int)b[1]);
}

// The sampling loop of one scene.  Tile t belongs to lane t / 16 of wave t % 16 (neighbouring tiles, which a sample tends to
// touch together, go to different waves); the owner keeps the tile's box, its maximum dist, the arg-max and that point's
// xyz in registers.  Per step, per wave, with no barrier:
//   A  every lane tests its tile against the new sample c: lb = (gx*gx + gy*gy) + gz*gz with g = the per-axis gap between c
//      and the tile's box.  For a point p of the tile |p.x - c.x| >= gx exactly, fp32 subtraction, multiplication and
//      addition round monotonically, and lb is evaluated in the operation order of d, so lb <= d in fp32 for every point of
//      the tile.  lb >= the tile's current maximum dist therefore means min(dist, d) = dist for all its points: nothing in
//      the tile changes, its stored arg-max stays valid, and it is skipped.  A ballot lists the wave's other tiles.
//   B  the wave walks its listed tiles in units of 256 rows (4 per lane; the next unit's rows are requested before the
//      current one is reduced): dist = min(dist, d), the tile's new (max dist, smallest caller index) and that point's xyz
//      go to the owner lane.
//   C  arg-max over the wave's tiles, one LDS record per wave, ONE barrier, arg-max over the 16 records (ties: smallest
//      caller index) = the next sample and its xyz.  The records are double-buffered, so the barrier of step s + 1 is what
//      keeps step s + 2 from overwriting a record that a slow wave still reads.
// Nothing leaves the workgroup.
template <int T>
__global__ __launch_bounds__(FPS_NT) void fps_scene_kernel(const float* __restrict__ pts, FpsScenes sc, float4* __restrict__ ws_all,
                                                           const int* __restrict__ cidx_all, const float* __restrict__ tilebox,
                                                           int32_t* __restrict__ out, int M, int start,
                                                           int64_t* __restrict__ scanned_out) {
  constexpr int CH = T / 256;
  __shared__ float red_v[2][FPS_NW], red_x[2][FPS_NW], red_y[2][FPS_NW], red_z[2][FPS_NW];
  __shared__ int red_i[2][FPS_NW];
  __shared__ unsigned long long scanned_all;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = sc.off[b + 1] - sc.off[b];
  const int ntiles = min((int)((n + T - 1) / T), FPS_MAX_TILES);
  float4* ws = ws_all + sc.row0[b];
  const int* cidx = cidx_all + sc.row0[b];
  const int mine = lane * FPS_NW + wave;          // this lane's tile
  const bool has = mine < ntiles;
  float lox = 0.f, loy = 0.f, loz = 0.f, hix = 0.f, hiy = 0.f, hiz = 0.f;
  if (has) {
    const float* tb = tilebox + ((long)(sc.row0[b] / T) + mine) * 6;
    lox = tb[0]; loy = tb[1]; loz = tb[2]; hix = tb[3]; hiy = tb[4]; hiz = tb[5];
  }
  float my_max = has ? INFINITY : -2.f, my_x = 0.f, my_y = 0.f, my_z = 0.f;
  int my_arg = INT_MAX;
  if (tid == 0) scanned_all = 0ull;
  const float* p0 = pts + (sc.off[b] + start) * 3;
  float cx = p0[0], cy = p0[1], cz = p0[2];
  if (tid == 0) out[(long)b * M] = start;
  long scanned = 0;
  for (int s = 1; s < M; ++s) {
    const int pb = s & 1;
    bool rescan = false;
    if (has) {
      const float gx = fmaxf(fmaxf(lox - cx, cx - hix), 0.f), gy = fmaxf(fmaxf(loy - cy, cy - hiy), 0.f),
                  gz = fmaxf(fmaxf(loz - cz, cz - hiz), 0.f);
      rescan = (gx * gx + gy * gy) + gz * gz < my_max;
    }
    unsigned long long need = __ballot(rescan);
    scanned += __popcll(need);
    int own = -1, ch = 0;                         // current unit: chunk ch of the tile of lane `own`
    if (need) { own = __ffsll((long long)need) - 1; need &= need - 1; }
    float4 ra[4], rb[4];
    int ca[4], cb[4];
    if (own >= 0) {
      const int row0 = (own * FPS_NW + wave) * T + lane;
#pragma unroll
      for (int j = 0; j < 4; ++j) { ra[j] = ws[row0 + j * 64]; ca[j] = cidx[row0 + j * 64]; }
    }
    float best = -2.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bi = INT_MAX;
    while (own >= 0) {
      int own_n = own, ch_n = ch + 1;
      if (ch_n == CH) {
        ch_n = 0; own_n = -1;
        if (need) { own_n = __ffsll((long long)need) - 1; need &= need - 1; }
      }
      if (own_n >= 0) {
        const int rown = (own_n * FPS_NW + wave) * T + ch_n * 256 + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) { rb[j] = ws[rown + j * 64]; cb[j] = cidx[rown + j * 64]; }
      }
      const int row0 = (own * FPS_NW + wave) * T + ch * 256 + lane;
      if (ch == 0) { best = -2.f; bi = INT_MAX; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 r = ra[j];
        const int ci = ca[j];
        const float dx = r.x - cx, dy = r.y - cy, dz = r.z - cz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        const float nd = fminf(d, r.w);
        if (nd != r.w) ((float*)&ws[row0 + j * 64])[3] = nd;
        if (nd > best || (nd == best && ci < bi)) { best = nd; bi = ci; bx = r.x; by = r.y; bz = r.z; }
      }
      if (ch == CH - 1) {
        const float wv = wave_max(best);
        const int wi = fps_wave_min_i(best == wv ? bi : INT_MAX);
        const unsigned long long src_m = __ballot(best == wv && bi == wi);
        const int src = src_m ? __ffsll((long long)src_m) - 1 : 0;
        const float sx = __shfl(bx, src, 64), sy = __shfl(by, src, 64), sz = __shfl(bz, src, 64);
        if (lane == own) { my_max = wv; my_arg = wi; my_x = sx; my_y = sy; my_z = sz; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { ra[j] = rb[j]; ca[j] = cb[j]; }
      own = own_n; ch = ch_n;
    }
    {
      const float wv = wave_max(my_max);
      const int wi = fps_wave_min_i(my_max == wv ? my_arg : INT_MAX);
      const unsigned long long src_m = __ballot(my_max == wv && my_arg == wi);
      if (lane == (src_m ? __ffsll((long long)src_m) - 1 : 0)) {
        red_v[pb][wave] = wv; red_i[pb][wave] = wi; red_x[pb][wave] = my_x; red_y[pb][wave] = my_y; red_z[pb][wave] = my_z;
      }
    }
    __syncthreads();
    const int r = lane & (FPS_NW - 1);
    const float rv = red_v[pb][r], mv = fps_row_max(rv);
    const int ri = red_i[pb][r], mi = fps_row_min(rv == mv ? ri : INT_MAX);
    const int w = fps_row_min(rv == mv && ri == mi ? r : FPS_NW - 1) & (FPS_NW - 1);
    cx = red_x[pb][w]; cy = red_y[pb][w]; cz = red_z[pb][w];
    if (tid == 0) out[(long)b * M + s] = mi;
  }
  if (scanned_out) {
    __syncthreads();
    if (lane == 0) atomicAdd(&scanned_all, (unsigned long long)scanned);
    __syncthreads();
    if (tid == 0) scanned_out[b] = (int64_t)scanned_all;
  }
}

// host: scene table from the caller's offsets; "" or an argument error text
std::string fps_table(const int64_t* offsets, int B, FpsScenes& sc) {
  const std::string e = scene_table_fill(sc, offsets, B, PQ3D_FPS_MAX_POINTS, (long long)PQ3D_FPS_MAX_SCENES * PQ3D_FPS_MAX_POINTS,
                                         "pq3d_fps_scene");
  if (!e.empty()) return e;
  long long nmax = 0;
  for (int b = 0; b < B; ++b) nmax = sc.off[b + 1] - sc.off[b] > nmax ? sc.off[b + 1] - sc.off[b] : nmax;
  sc.T = nmax <= (long long)FPS_TILE_SMALL * FPS_MAX_TILES ? FPS_TILE_SMALL : FPS_TILE_BIG;
  long long rows = 0;
  for (int b = 0; b <= PQ3D_FPS_MAX_SCENES; ++b) {
    sc.row0[b] = (int)rows;
    if (b < B) rows += (sc.off[b + 1] - sc.off[b] + sc.T - 1) / sc.T * sc.T;
  }
  return e;
}

}  // namespace

extern "C" int pq3d_voxelize(const float* coordinates, const int64_t* offsets, int32_t B, float voxel_size, int64_t capacity,
                             void* keys, int32_t* rep, int32_t* slot, int32_t* pv, int32_t* bsum, int64_t* unique_map,
                             int64_t* inverse_map, int32_t* voxel_coordinates, int64_t* meta, void* stream) {
  PQ_DEVICE_GUARD(stream, coordinates);
  PQ_CHECK_ARG(coordinates && offsets && keys && rep && slot && pv && bsum && unique_map && inverse_map && voxel_coordinates && meta,
               "pq3d_voxelize: null pointer");
  PQ_CHECK_ARG(voxel_size > 0.f && voxel_size <= FLT_MAX, "pq3d_voxelize: voxel_size must be a finite number > 0");
  VoxScenes sc;      // (at most 8 scenes: the packed key has 3 scene bits)
  PQ_SCENE_TABLE(sc, offsets, B, PQ3D_VOXELIZE_MAX_POINTS, PQ3D_VOXELIZE_MAX_POINTS, "pq3d_voxelize");
  const long P = (long)sc.off[B];
  PQ_CHECK_ARG(capacity >= 2 * P && capacity <= (1ll << 31) && (capacity & (capacity - 1)) == 0,
               "pq3d_voxelize: capacity must be a power of two >= 2 P");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nblk = (unsigned)((P + PQ3D_VOXELIZE_BLOCK - 1) / PQ3D_VOXELIZE_BLOCK), nb256 = (unsigned)((P + 255) / 256);
  int* err = (int*)(meta + B + 1);
  hipLaunchKernelGGL(vox_init_kernel, dim3(1024), dim3(256), 0, s, (unsigned long long*)keys, rep, (long)capacity, (long long*)meta,
                     B + 2);
  hipLaunchKernelGGL(vox_insert_kernel, dim3(nb256), dim3(256), 0, s, coordinates, sc, P, voxel_size, (unsigned long long*)keys, rep,
                     (unsigned)(capacity - 1), slot, err);
  hipLaunchKernelGGL(vox_count_kernel, dim3(nblk), dim3(256), 0, s, slot, rep, P, bsum);
  hipLaunchKernelGGL(vox_scan_kernel, dim3(1), dim3(1024), 0, s, bsum, (int)nblk, (long long*)meta, B);
  hipLaunchKernelGGL(vox_emit_kernel, dim3(nblk), dim3(256), 0, s, coordinates, sc, P, voxel_size, slot, rep, bsum, pv, unique_map,
                     voxel_coordinates, (long long*)meta);
  hipLaunchKernelGGL(vox_inverse_kernel, dim3(nb256), dim3(256), 0, s, sc, P, slot, rep, pv, (const long long*)meta, inverse_map);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t pq3d_fps_scene_rows(const int64_t* offsets, int32_t B) {
  FpsScenes sc;
  const std::string e = fps_table(offsets, B, sc);
  if (!e.empty()) { pq3d_set_error(e.c_str()); return -1; }
  return sc.row0[B];
}

extern "C" int pq3d_fps_scene_keys(const float* points, const int64_t* offsets, int32_t B, float* bbox, int64_t* keys, void* stream) {
  PQ_DEVICE_GUARD(stream, points);
  PQ_CHECK_ARG(points && bbox && keys, "pq3d_fps_scene_keys: null pointer");
  FpsScenes sc;
  const std::string e = fps_table(offsets, B, sc);
  PQ_CHECK_ARG(e.empty(), e.c_str());
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fps_bbox_kernel, dim3(B), dim3(FPS_NT), 0, s, points, sc, bbox);
  hipLaunchKernelGGL(fps_key_kernel, dim3((unsigned)((sc.off[B] + 255) / 256)), dim3(256), 0, s, points, sc, (const float*)bbox, keys);
  PQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int pq3d_fps_scene(const float* points, const int64_t* offsets, int32_t B, const int64_t* perm, int32_t M,
                              int32_t start_idx, void* ws, int64_t ws_rows, int32_t* cidx, float* tilebox, int32_t* idx,
                              int64_t* scanned, void* stream) {
  PQ_DEVICE_GUARD(stream, points);
  PQ_CHECK_ARG(points && perm && ws && cidx && tilebox && idx, "pq3d_fps_scene: null pointer");
  FpsScenes sc;
  const std::string e = fps_table(offsets, B, sc);
  PQ_CHECK_ARG(e.empty(), e.c_str());
  PQ_CHECK_ARG(ws_rows >= sc.row0[B], "pq3d_fps_scene: workspace smaller than pq3d_fps_scene_rows");
  for (int b = 0; b < B; ++b) {
    const long long n = offsets[b + 1] - offsets[b];
    PQ_CHECK_ARG(M >= 1 && M <= n, "pq3d_fps_scene: need 1 <= M <= N of every scene");
    PQ_CHECK_ARG(start_idx >= 0 && start_idx < n, "pq3d_fps_scene: start_idx outside a scene");
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fps_stage_kernel, dim3((unsigned)(sc.row0[B] / sc.T)), dim3(256), 0, s, points, sc, perm, (float4*)ws, cidx,
                     tilebox);
  if (sc.T == FPS_TILE_SMALL)
    hipLaunchKernelGGL((fps_scene_kernel<FPS_TILE_SMALL>), dim3(B), dim3(FPS_NT), 0, s, points, sc, (float4*)ws, (const int*)cidx,
                       (const float*)tilebox, idx, M, start_idx, scanned);
  else
    hipLaunchKernelGGL((fps_scene_kernel<FPS_TILE_BIG>), dim3(B), dim3(FPS_NT), 0, s, points, sc, (float4*)ws, (const int*)cidx,
                       (const float*)tilebox, idx, M, start_idx, scanned);
  PQ_LAUNCH_CHECK();
  return 0;
}
