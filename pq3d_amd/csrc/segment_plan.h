// Layout of the segment-plan buffer that pq3d_segment_plan (segment.hip) builds, shared with the kernels of other files
// that walk a plan (instseg_ap.hip's byte-row count).  A plan over N rows and S segments holds, in int32 units:
//   meta[0] valid rows, meta[1] pieces, meta[2] long segments;
//   seg_off[S + 1] CSR offsets per segment into perm[N] (rows ordered by segment, ascending row inside a segment);
//   pieces[] int4 {first sorted position, end position, segment, partial slot (-1: the segment's only piece)}: a segment of
//   n rows is cut into max(1, ceil(n / SEG_P)) pieces.
#pragma once

namespace pq3d_plan {

constexpr int SEG_P = 128;        // rows per piece (two 64-row index blocks)
constexpr int SORT_ROUNDS = 8;    // a sort tile = 256 threads x 8 rounds
constexpr int SORT_TILE = 256 * SORT_ROUNDS;

// ---- plan buffer layout (int32 units; every section starts on a 64-byte boundary) -----------------------------------
struct PlanLayout {
  long meta, seg_off, perm, pieces, longs, keys_a, keys_b, perm_b, tile_hist, dig_tot, bsum, total;
  long n_tiles, max_pieces, max_long, max_slots;
};
inline long up16(long x) { return (x + 15) & ~15L; }
inline PlanLayout plan_layout(long N, long S) {
  PlanLayout L;
  L.n_tiles = (N + SORT_TILE - 1) / SORT_TILE;
  if (L.n_tiles < 1) L.n_tiles = 1;
  L.max_pieces = S + N / SEG_P + 1;           // sum over segments of max(1, ceil(n / P))
  L.max_long = N / (SEG_P + 1) + 1;           // segments with more than P voxels
  L.max_slots = N / SEG_P + L.max_long + 1;   // their pieces
  long o = 0;
  L.meta = o; o += 16;
  L.seg_off = o; o += up16(S + 1);
  L.perm = o; o += up16(N);
  L.pieces = o; o += up16(4 * L.max_pieces);
  L.longs = o; o += up16(2 * L.max_long);
  L.keys_a = o; o += up16(N);
  L.keys_b = o; o += up16(N);
  L.perm_b = o; o += up16(N);
  L.tile_hist = o; o += up16(256 * L.n_tiles);
  L.dig_tot = o; o += 256;
  L.bsum = o; o += up16(3 * ((S + 1023) / 1024 + 1));
  L.total = o;
  return L;
}

}  // namespace pq3d_plan
