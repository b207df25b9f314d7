// The vector-Jacobian product of the sensor columns by bounded central differences (spart_vjp, include/spart_hip.h; the
// definition is tools/vjp_defined.py and every function here reproduces it bit for bit).
//
// Part 1: the per-entry arithmetic -- the two steps of a free parameter, one band's term, the ordered sum of a tile and the
// final division -- as plain functions under SPART_NO_CONTRACT.  hipcc compiles them into the kernels of part 2 and g++
// compiles them for tests/hostmath/vjp_host.cpp.  Array arguments come with a stride.
//
// Part 2: two kernels around ONE forward call per chunk.  A chunk of Mc observations owns
//   table  (27, 2 F Mc) float64, row = k Mc + m, block k = 2 f: p_f^+, block k = 2 f + 1: p_f^-;
//   cols   three (2 F Mc, nb) float64 blocks, same row order (with the SRF band model only the one the call is about);
//   den    (Mc, F) float64: a_f - b_f.
#pragma once

#include "spart_refine.h"    // refine_clip, refine_fill_*, RefineCfg, REFINE_*; spart_math.h: SPART_HD, SPART_NO_CONTRACT, NPARAM

namespace spart {

constexpr int VJP_ROWS = REFINE_ROWS;        // rows of one forward call at most: observations go in chunks of VJP_ROWS / (2 F)
constexpr double VJP_REL_STEP = 1e-3, VJP_MAX_REL_STEP = 0.5;

// observations per chunk
SPART_HD int64_t vjp_chunk(int F) { return VJP_ROWS / (2 * F); }

// a = x + h, b = x - h, each put back on the bound it passes: central inside the box, one-sided on a bound (a NaN x stays one)
struct VjpStep {
  double a, b;
};
SPART_HD VjpStep vjp_step(double x, double h, double lo, double hi) {
  SPART_NO_CONTRACT
  VjpStep s;
  s.a = x + h;
  if (s.a > hi) s.a = hi;
  s.b = x - h;
  if (s.b < lo) s.b = lo;
  return s;
}

// One band's term g (Y+ - Y-).  A band of g == 0 is skipped whatever Y holds: its term is +0.0, and s + (+0.0) is s for every
// s the sum can hold (it starts at +0.0 and an IEEE sum never gives -0.0 from there), so adding it IS skipping the band.
SPART_HD double vjp_term(double g, double yp, double ym) {
  SPART_NO_CONTRACT
  if (g == 0.0) return 0.0;
  const double d = yp - ym;
  return g * d;
}

// s over jn terms, ascending
SPART_HD double vjp_tile_add(double s, int jn, const double* p, int S) {
  SPART_NO_CONTRACT
  for (int jj = 0; jj < jn; ++jj) s = s + p[jj * S];
  return s;
}

// grad = s / (a - b)
SPART_HD double vjp_finish(double s, double den) {
  SPART_NO_CONTRACT
  return s / den;
}

// One lane per (observation, f): the group is the largest power of two W with W F <= 64 (4 ... 64 observations).
SPART_HD int vjp_group(int F) {
  int W = 64;
  while (W * F > 64) W >>= 1;
  return W;
}
// The LDS tile of a group, the family's padded [k][o] layout: term (f, jj) of observation o at f FS + jj (W + 1) + o doubles.
// Banks (ds_write_b64: 16 consecutive lanes, dword address mod 32; ds_read_b64: 32 consecutive lanes, dword address mod 64).
// The staging stores of 16 consecutive lanes walk jj at one (f, o): 2 (W + 1) jj mod 32 are 16 distinct even banks because
// W + 1 is odd.  The adding lanes o + W q read f = q at one jj: FS = 16 (W + 1) is 16 mod 32 doubles, which would put q and
// q + 2 on one bank; padded to FS = W mod 32 the 32 lanes of a half wave read the 32 doubles q W + o = lane: no conflict.
SPART_HD int vjp_fstride(int W) { return 16 * (W + 1) + (W < 32 ? ((W - 16) & 31) : 0); }

#if defined(__HIPCC__)

static_assert(REFINE_JT == 16, "vjp_fstride: a tile of 16 bands");

inline size_t vjp_lds_bytes(int F, int W) { return (size_t)F * (size_t)vjp_fstride(W) * 8; }
// the family's rule (refine_group): halve the group while its LDS is over the budget
inline int vjp_group_lds(int F) {
  int W = vjp_group(F);
  while (W > REFINE_MIN_GROUP && vjp_lds_bytes(F, W) > (size_t)REFINE_LDS_BUDGET) W >>= 1;
  return W;
}

// The table and the denominators of the chunk from observation m0: thread = observation.  refine_fill_row / _fixed write
// `F + 1` blocks for their argument F: 2 F - 1 makes them the 2 F blocks here; block 2 f gets a_f from them, block 2 f + 1
// b_f after them.
__global__ __launch_bounds__(256) void k_vjp_init(RefineCfg a, int64_t m0, int Mc, int F, double* __restrict__ table,
                                                  double* __restrict__ den) {
  SPART_NO_CONTRACT
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= Mc) return;
  const int64_t R = (int64_t)2 * F * Mc;
  refine_fill_fixed(a, m0 + m, table + m, R, 2 * F - 1, Mc);
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    const double x = refine_clip(a.freebase[f][m0 + m], a.lo[f], a.hi[f]);
    const VjpStep s = vjp_step(x, a.h[f], a.lo[f], a.hi[f]);
    double* row = table + a.free_col[f] * R + m;
    refine_fill_row(row, 2 * F - 1, Mc, 2 * f, x, s.a);
    row[(int64_t)(2 * f + 1) * Mc] = s.b;
    den[(int64_t)m * F + f] = s.a - s.b;
  }
}

// the chunk's rows of the three column blocks and of the three output gradients (g[c] NULL: column c takes no part)
struct VjpCols {
  const double* y[3];
  const double* g[3];
};

// After the forward call.  Single-wave workgroups of W = vjp_group_lds(F) consecutive observations.  Per column c with g[c],
// c ascending, and per tile of REFINE_JT bands, ascending: lanes run along the bands -- slot (o, jj) loads g once and then, per
// f, Y+ and Y- (8-byte loads, 128 B of a row per 16 lanes, 64-bit offsets) and leaves vjp_term in LDS; then lane o + W f adds
// the tile of its (observation, f) in ascending order onto ONE register that it carries across tiles and columns.  Every
// s_f is therefore the defined sum: no atomics, nothing depends on W or on the order of waves.
__global__ __launch_bounds__(64) void k_vjp_reduce(VjpCols a, const double* __restrict__ den, int Mc, int F, int nb, int W,
                                                   double* __restrict__ grad) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char vjp_smem[];
  constexpr int JT = REFINE_JT;
  double* P = reinterpret_cast<double*>(vjp_smem);
  const int WP = W + 1, FS = vjp_fstride(W);
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * W;                         // first observation of the group
  const int nobs = Mc - g0 < W ? Mc - g0 : W;
  const int o = lane % W, f = lane / W;                  // the (observation, f) this lane adds
  const bool mine = o < nobs && f < F;
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!a.g[c]) continue;                               // (kernel-uniform)
    const double* g_g = a.g[c] + (int64_t)g0 * nb;
    for (int j0 = 0; j0 < nb; j0 += JT) {
      __syncthreads();
      for (int i = lane; i < W * JT; i += 64) {
        const int jj = i % JT, oo = i / JT, j = j0 + jj;
        const bool in = oo < nobs && j < nb;
        const int64_t at = (int64_t)oo * nb + j;
        const double g = in ? g_g[at] : 0.0;
        for (int ff = 0; ff < F; ++ff) {
          double t = 0.0;
          if (in) {
            const double* yp = a.y[c] + ((int64_t)(2 * ff) * Mc + g0) * nb;
            const double* ym = yp + (int64_t)Mc * nb;
            t = vjp_term(g, yp[at], ym[at]);
          }
          P[ff * FS + jj * WP + oo] = t;
        }
      }
      __syncthreads();
      if (mine) s = vjp_tile_add(s, nb - j0 < JT ? nb - j0 : JT, P + f * FS + o, WP);
    }
  }
  if (mine) {
    const int64_t e = (int64_t)(g0 + o) * F + f;
    grad[e] = vjp_finish(s, den[e]);
  }
}

#endif  // __HIPCC__

}  // namespace spart
