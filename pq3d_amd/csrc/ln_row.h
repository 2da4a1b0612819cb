// The LayerNorm row arithmetic, written once: norm.hip's kernels (any d, a row in PL values per lane) and the one-launch chain
// kernels (d = 256, 4 values per lane) call these, so a row normalised inside a chain equals the same row of a separate
// pq3d_add_ln_fwd / pq3d_add_ln_bwd launch bit for bit (tests/test_gpu_chain.py).  One wave per row; fp32; the order of every
// sum and product is part of that contract -- a change here changes every site at once, and nowhere else.
// `valid(j)`: value j of this lane is a column of the row (norm.hip: colof(lane, j) < d; rows without tail columns: AllCols).
#pragma once
#include "common.h"

struct RowStats { float mean, rstd; };
struct AllCols { PQ_DEV bool operator()(int) const { return true; } };

// mean, then the centred variance; v is zero in the columns that are not valid
template <int PL, typename Valid>
PQ_DEV RowStats ln_row_stats(const float (&v)[PL], int d, float eps, Valid valid) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < PL; ++j) s += v[j];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < PL; ++j) {
    const float t = v[j] - mean;
    q += valid(j) ? t * t : 0.f;
  }
  const float var = wave_sum(q) / (float)d;
  return {mean, 1.f / sqrtf(var + eps)};
}

// One backward row of y = w LN(v): g = d v from the upstream gradient dyr; this lane's parameter-gradient partials accumulate
// in dg / db
template <int PL, typename Valid>
PQ_DEV void ln_bwd_row(const float (&v)[PL], const float (&dyr)[PL], const float (&gam)[PL], float w, float mean, float rstd, int d,
                       Valid valid, float (&g)[PL], float (&dg)[PL], float (&db)[PL]) {
  float xh[PL], dz[PL];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < PL; ++j) {
    float x = 0.f, z = 0.f;
    if (valid(j)) {
      const float du = w * dyr[j];
      x = (v[j] - mean) * rstd;
      dg[j] += du * x;
      db[j] += du;
      z = du * gam[j];
      s1 += z;
      s2 += z * x;
    }
    xh[j] = x;
    dz[j] = z;
  }
  s1 = wave_sum(s1) / (float)d;
  s2 = wave_sum(s2) / (float)d;
#pragma unroll
  for (int j = 0; j < PL; ++j) g[j] = rstd * (dz[j] - s1 - xh[j] * s2);
}

// A gradient row that arrives in up to three addends: s = (row 0 + row 1) + row 2; load(i, t) reads addend i
template <int PL, typename Load>
PQ_DEV void add3_rows(Load load, bool has2, bool has3, float (&s)[PL]) {
  load(0, s);
  if (has2) {
    float t[PL];
    load(1, t);
#pragma unroll
    for (int j = 0; j < PL; ++j) s[j] += t[j];
    if (has3) {
      load(2, t);
#pragma unroll
      for (int j = 0; j < PL; ++j) s[j] += t[j];
    }
  }
}

// Residual dropout of one branch's row (colof(j): the column of value j); returns the keep bits (bit j: value j survived)
template <int PL, typename ColOf>
PQ_DEV unsigned res_dropout_row(float (&ov)[PL], const DropState& ds, long row, ColOf colof) {
  unsigned keep = 0;
#pragma unroll
  for (int j = 0; j < PL; ++j) {
    const bool k = drop_keep(ds, (uint32_t)row, (uint32_t)colof(j));
    keep |= (unsigned)k << j;
    ov[j] = k ? ov[j] * ds.scale : 0.f;
  }
  return keep;
}
