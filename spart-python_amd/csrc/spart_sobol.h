// Variance-based (Sobol') sensitivity indices of the sensor columns (spart_sobol, include/spart_hip.h; the definition is
// tools/sobol_defined.py and every function here reproduces it bit for bit).
//
// Part 1: the per-entry arithmetic -- a design point, the shift, the 64-term tree, the finish formulas and the delete-one-block
// jackknife of one (band, parameter) -- as plain functions under SPART_NO_CONTRACT.  hipcc compiles them into the kernels of
// part 2 and g++ compiles them for tests/hostmath/sobol_host.cpp.  Array arguments come with strides.
//
// Part 2: three kernels.  A chunk is a run of consecutive BLOCKS (64 samples of one site), site-major: block b of the call is
// block g = b % G of site m = b / G, G = N / 64.  Block lb of a chunk owns the 64 (F + 2) table rows
//   lb 64 (F + 2) + k 64 + lane,   k = 0: A,  1: B,  2 + f: C^f,   lane = sample 64 g + lane of the design,
// so a forward call serves many small sites at once and a large site runs over several chunks.  The block sums of a site
// wait in the workspace slot m % nslot until its last block has been summed; c_j waits beside them.
#pragma once

#include "spart_refine.h"    // REFINE_MAXF, REFINE_ROWS; spart_math.h: SPART_HD, SPART_NO_CONTRACT, NPARAM

namespace spart {

constexpr int SOBOL_BLOCK = 64;                         // samples per block: one wave
constexpr int64_t SOBOL_MIN_N = 128, SOBOL_MAX_N = 1 << 20;
constexpr int SOBOL_ROWS = REFINE_ROWS;                 // rows of one forward call at most
constexpr int SOBOL_MAXQ = 4 + 3 * REFINE_MAXF;

// the Q = 4 + 3 F quantities of a block, in the workspace's order: sa, sb, saa, sbb, then u_f, t_f, e_f per f
SPART_HD int sobol_nq(int F) { return 4 + 3 * F; }
// blocks per chunk: whole blocks of 64 (F + 2) rows within SOBOL_ROWS
SPART_HD int sobol_chunk_blocks(int F) { return SOBOL_ROWS / (SOBOL_BLOCK * (F + 2)); }

// x = lo + u (hi - lo), the difference formed first
SPART_HD double sobol_point(double lo, double hi, double u) {
  SPART_NO_CONTRACT
  const double w = hi - lo;
  return lo + u * w;
}

// a = y - c
SPART_HD double sobol_shift(double y, double c) {
  SPART_NO_CONTRACT
  return y - c;
}

// d = (yC - c) - a
SPART_HD double sobol_delta(double yc, double c, double a) {
  SPART_NO_CONTRACT
  const double s = yc - c;
  return s - a;
}

SPART_HD double sobol_mul(double a, double b) {
  SPART_NO_CONTRACT
  return a * b;
}

// The fixed tree over 64 terms t[r S], in place: for s = 32, 16, 8, 4, 2, 1: t_r = t_r + t_{r+s} for r < s.  -> t_0
SPART_HD double sobol_tree64(double* t, int S) {
  SPART_NO_CONTRACT
  for (int s = SOBOL_BLOCK / 2; s >= 1; s >>= 1)
    for (int r = 0; r < s; ++r) t[r * S] = t[r * S] + t[(r + s) * S];
  return t[0];
}

// mu = (SA + SB) / (2 n), m2 = (SAA + SBB) / (2 n), var = m2 - mu mu
SPART_HD void sobol_moments(double SA, double SB, double SAA, double SBB, double n, double* mu, double* var) {
  SPART_NO_CONTRACT
  const double n2 = 2.0 * n;
  const double m = (SA + SB) / n2;
  const double m2 = (SAA + SBB) / n2;
  *mu = m;
  *var = m2 - m * m;
}

// S1 = (U / n - mu (D / n)) / var
SPART_HD double sobol_first(double U, double D, double mu, double var, double n) {
  SPART_NO_CONTRACT
  const double p = U / n;
  const double q = mu * (D / n);
  return (p - q) / var;
}

// ST = (T / (2 n)) / var
SPART_HD double sobol_total(double T, double var, double n) {
  SPART_NO_CONTRACT
  return (T / (2.0 * n)) / var;
}

// One (band, f) of one site from its block sums: quantity q of block g at bs[g SG + q SQ] (the caller has moved bs to the
// band).  Totals over g ascending from 0.0, the finish formulas, and -- with jack -- the two jackknife passes.
// out: mean, var, S1, ST, S1_se, ST_se (the last two untouched without jack).
SPART_HD void sobol_entry(const double* bs, int64_t SG, int64_t SQ, int G, int f, double N, double c, bool jack, double* out) {
  SPART_NO_CONTRACT
  const double* pa = bs;
  const double* pb = bs + SQ;
  const double* paa = bs + 2 * SQ;
  const double* pbb = bs + 3 * SQ;
  const double* pu = bs + (4 + 3 * f) * SQ;
  const double* pt = bs + (5 + 3 * f) * SQ;
  const double* pd = bs + (6 + 3 * f) * SQ;
  double SA = 0.0, SB = 0.0, SAA = 0.0, SBB = 0.0, U = 0.0, T = 0.0, D = 0.0;
  for (int g = 0; g < G; ++g) {
    const int64_t o = g * SG;
    SA = SA + pa[o];
    SB = SB + pb[o];
    SAA = SAA + paa[o];
    SBB = SBB + pbb[o];
    U = U + pu[o];
    T = T + pt[o];
    D = D + pd[o];
  }
  double mu, var;
  sobol_moments(SA, SB, SAA, SBB, N, &mu, &var);
  out[0] = c + mu;
  out[1] = var;
  out[2] = sobol_first(U, D, mu, var, N);
  out[3] = sobol_total(T, var, N);
  if (!jack) return;
  const double n1 = N - (double)SOBOL_BLOCK, Gd = (double)G;
  double s1 = 0.0, st = 0.0;
  for (int g = 0; g < G; ++g) {
    const int64_t o = g * SG;
    double m, v;
    sobol_moments(SA - pa[o], SB - pb[o], SAA - paa[o], SBB - pbb[o], n1, &m, &v);
    s1 = s1 + sobol_first(U - pu[o], D - pd[o], m, v, n1);
    st = st + sobol_total(T - pt[o], v, n1);
  }
  const double b1 = s1 / Gd, bt = st / Gd;
  double v1 = 0.0, vt = 0.0;
  for (int g = 0; g < G; ++g) {
    const int64_t o = g * SG;
    double m, v;
    sobol_moments(SA - pa[o], SB - pb[o], SAA - paa[o], SBB - pbb[o], n1, &m, &v);
    const double e1 = sobol_first(U - pu[o], D - pd[o], m, v, n1) - b1;
    const double et = sobol_total(T - pt[o], v, n1) - bt;
    v1 = v1 + e1 * e1;
    vt = vt + et * et;
  }
  out[4] = __builtin_sqrt((v1 * (Gd - 1.0)) / Gd);
  out[5] = __builtin_sqrt((vt * (Gd - 1.0)) / Gd);
}

#if defined(__HIPCC__)

struct SobolCfg {
  const double* base[NPARAM];            // the sites' fixed rows (each (M,))
  int32_t is_free[NPARAM];
  int32_t free_col[REFINE_MAXF];
  double lo[REFINE_MAXF], hi[REFINE_MAXF];
};

struct SobolOut {                        // spart_sobol_out
  double *mean, *var, *S1, *ST, *S1_se, *ST_se;
};

// The (27, R) table of a chunk of bc blocks from block b0 of the call, R = bc 64 (F + 2): thread = row.
__global__ __launch_bounds__(256) void k_sobol_rows(SobolCfg a, int F, int64_t b0, int bc, int G, const double* __restrict__ uA,
                                                    const double* __restrict__ uB, double* __restrict__ table) {
  SPART_NO_CONTRACT
  const int per = SOBOL_BLOCK * (F + 2);
  const int64_t R = (int64_t)bc * per;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= R) return;
  const int lb = (int)(row / per), rem = (int)(row % per), k = rem / SOBOL_BLOCK, lane = rem % SOBOL_BLOCK;
  const int64_t b = b0 + lb, m = b / G;
  const int64_t n = (b % G) * SOBOL_BLOCK + lane;
#pragma unroll
  for (int p = 0; p < NPARAM; ++p)
    if (!a.is_free[p]) table[p * R + row] = a.base[p][m];
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    const double u = (k == 1 || k == 2 + f) ? uB[n * F + f] : uA[n * F + f];
    table[a.free_col[f] * R + row] = sobol_point(a.lo[f], a.hi[f], u);
  }
}

// The tree of sobol_tree64 across the 64 lanes of a wave: lane r holds t_r; a step adds lane r + s to lane r (a double crosses
// lanes as its two 32-bit halves).  Lanes r >= s carry values nobody reads.  -> t_0 in lane 0
__device__ __forceinline__ double sobol_wave_tree(double v) {
  SPART_NO_CONTRACT
#pragma unroll
  for (int s = SOBOL_BLOCK / 2; s >= 1; s >>= 1) v = v + __shfl_down(v, (unsigned)s, SOBOL_BLOCK);
  return v;
}

// One wave per (block of the chunk, band): lane = sample.  ycol (R, nb) is the forward call's column.  The site's c_j is
// yA[0, j]: read from the column when the site's first block is in this chunk, from cbuf (slot, nb) otherwise; the wave of
// a site's first block leaves it there for the chunks after.  Block sums to bs ((slot, G, Q, nb)).
__global__ __launch_bounds__(256) void k_sobol_blocks(const double* __restrict__ ycol, int nb, int F, int64_t b0, int bc, int G,
                                                      int nslot, double* __restrict__ cbuf, double* __restrict__ bs) {
  SPART_NO_CONTRACT
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (int64_t)bc * nb) return;                      // (a whole wave)
  const int lb = (int)(w / nb), j = (int)(w % nb), Q = sobol_nq(F);
  const int64_t b = b0 + lb, m = b / G;
  const int g = (int)(b % G), slot = (int)(m % nslot);
  const int64_t per = (int64_t)SOBOL_BLOCK * (F + 2), step = (int64_t)SOBOL_BLOCK * nb;
  const int64_t first = m * G - b0;                       // the site's block 0 as a block of this chunk (< 0: an earlier chunk)
  const double c = first >= 0 ? ycol[first * per * nb + j] : cbuf[(int64_t)slot * nb + j];
  if (g == 0 && lane == 0) cbuf[(int64_t)slot * nb + j] = c;
  const double* y = ycol + ((int64_t)lb * per + lane) * nb + j;
  double* o = bs + (((int64_t)slot * G + g) * Q) * nb + j;
  const double a = sobol_shift(y[0], c), bb = sobol_shift(y[step], c);
  const double sa = sobol_wave_tree(a), sb = sobol_wave_tree(bb);
  const double saa = sobol_wave_tree(sobol_mul(a, a)), sbb = sobol_wave_tree(sobol_mul(bb, bb));
  if (lane == 0) {
    o[0] = sa;
    o[nb] = sb;
    o[2 * (int64_t)nb] = saa;
    o[3 * (int64_t)nb] = sbb;
  }
  for (int f = 0; f < F; ++f) {
    const double d = sobol_delta(y[(2 + f) * step], c, a);
    const double su = sobol_wave_tree(sobol_mul(bb, d)), st = sobol_wave_tree(sobol_mul(d, d)), se = sobol_wave_tree(d);
    if (lane == 0) {
      o[(int64_t)(4 + 3 * f) * nb] = su;
      o[(int64_t)(5 + 3 * f) * nb] = st;
      o[(int64_t)(6 + 3 * f) * nb] = se;
    }
  }
}

// The sites m0 ... m0 + gridDim.y - 1, whose last block has been summed: lane = (band, f).  out is the call's.
__global__ __launch_bounds__(64) void k_sobol_finish(const double* __restrict__ bs, const double* __restrict__ cbuf, int nb, int F,
                                                     int G, int nslot, int64_t m0, double N, SobolOut out) {
  SPART_NO_CONTRACT
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= nb * F) return;
  const int j = e / F, f = e % F, Q = sobol_nq(F);
  const int64_t m = m0 + blockIdx.y;
  const int slot = (int)(m % nslot);
  double r[6];
  sobol_entry(bs + ((int64_t)slot * G * Q) * nb + j, (int64_t)Q * nb, nb, G, f, N, cbuf[(int64_t)slot * nb + j],
              out.S1_se || out.ST_se, r);
  const int64_t at = (m * nb + j) * F + f;
  if (f == 0) {
    if (out.mean) out.mean[m * nb + j] = r[0];
    if (out.var) out.var[m * nb + j] = r[1];
  }
  if (out.S1) out.S1[at] = r[2];
  if (out.ST) out.ST[at] = r[3];
  if (out.S1_se) out.S1_se[at] = r[4];
  if (out.ST_se) out.ST_se[at] = r[5];
}

#endif  // __HIPCC__

}  // namespace spart
