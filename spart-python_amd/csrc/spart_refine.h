// Bounded Levenberg-Marquardt refinement around the float64 column path (spart_refine, include/spart_hip.h; the definition
// is tools/refine_defined.py and every function here reproduces it bit for bit).
//
// Part 1: the per-observation arithmetic -- cost, normal equations, damped solve, bounds, uncertainty -- as plain
// functions of small arrays, under SPART_NO_CONTRACT.  hipcc compiles them into the kernels of part 2 and of the family and
// g++ compiles them for tests/hostmath/refine_host.cpp. Every array argument comes with a stride S (element k at p[k * S]): the kernels
// keep one column per lane in LDS, the host build passes 1.
//
// Index conventions.  Only the LOWER triangle of A is formed: entry (a, b), a >= b, at refine_tri(a, b) = a (a + 1) / 2 + b,
// is sum_j (w_j J_ja) J_jb.  The packed vector of an observation is those F (F + 1) / 2 sums, then g_0 .. g_{F-1}.
#pragma once

#include "spart_math.h"      // SPART_HD, SPART_NO_CONTRACT

namespace spart {

constexpr int REFINE_MAXF = 16;              // free parameters per call
constexpr int REFINE_MAX_ITER = 100;
constexpr int REFINE_ROWS = 1 << 19;         // rows of one forward call: observations go in chunks of REFINE_ROWS / (F + 1)
constexpr double REFINE_LAMBDA_MIN = 1e-12, REFINE_LAMBDA_MAX = 1e12;

SPART_HD int refine_tri(int a, int b) { return a * (a + 1) / 2 + b; }
SPART_HD int refine_ntri(int F) { return F * (F + 1) / 2; }

// t = v; if t < lo: t = lo; if t > hi: t = hi  (a NaN stays a NaN)
SPART_HD double refine_clip(double v, double lo, double hi) {
  double t = v;
  if (t < lo) t = lo;
  if (t > hi) t = hi;
  return t;
}

// s_f h_f: the finite-difference step of trial value t, forward unless that leaves the box
SPART_HD double refine_fd_step(double t, double h, double hi) {
  SPART_NO_CONTRACT
  return t + h <= hi ? h : -h;
}

// a weight that kills its observation: negative, NaN or infinite
SPART_HD bool refine_bad_weight(double w) { return !(w >= 0.0) || w == __builtin_inf(); }

// one band of the trial cost: c + (w d) d with d = y0 - obs; the caller skips bands of weight 0
SPART_HD double refine_cost_band(double c, double w, double y0, double obs) {
  SPART_NO_CONTRACT
  const double d = y0 - obs;
  return c + (w * d) * d;
}

SPART_HD double refine_residual(double y0, double obs) {
  SPART_NO_CONTRACT
  return y0 - obs;
}

// J_jf = (Y_fj - Y_0j) / (s_f h_f)
SPART_HD double refine_jacobian(double yf, double y0, double sh) {
  SPART_NO_CONTRACT
  return (yf - y0) / sh;
}

// one band of one sum of the normal equations: acc + (w a) b
SPART_HD double refine_mac(double acc, double w, double a, double b) {
  SPART_NO_CONTRACT
  return acc + (w * a) * b;
}

// one free parameter of the prior's part of the trial cost: c + (p e) e with e = t - mu; the caller skips parameters of weight 0
SPART_HD double refine_prior_cost(double c, double p, double t, double mu) {
  SPART_NO_CONTRACT
  const double e = t - mu;
  return c + (p * e) * e;
}

// one free parameter of the prior's part of g: acc + p e (e = refine_residual(t, mu)); its part of A_aa is the plain sum A_aa + p
SPART_HD double refine_prior_gain(double acc, double p, double e) {
  SPART_NO_CONTRACT
  return acc + p * e;
}

SPART_HD double refine_lambda(double lam, bool accept) {
  SPART_NO_CONTRACT
  if (accept) {
    const double l = lam / 10.0;
    return l > REFINE_LAMBDA_MIN ? l : REFINE_LAMBDA_MIN;
  }
  const double l = lam * 10.0;
  return l < REFINE_LAMBDA_MAX ? l : REFINE_LAMBDA_MAX;
}

// ---- the per-observation phases.  Every kernel of the family (spart_refine_views.h, _mix.h, _posterior.h, _tiles.h, _series.h,
// spart_sample.h) and every host test runs THESE loops; what differs between callers arrives as a stride, a range or a count.

// packed entry e < ntri(n) -> the pair a >= b
SPART_HD void refine_pair(int e, int* a, int* b) {
  int r = 0;
  while ((r + 1) * (r + 2) / 2 <= e) ++r;
  *a = r;
  *b = e - r * (r + 1) / 2;
}

// entry e of a packed vector (nt = ntri(n) sums of A, then g): A_ab, or g_a with b = -1
SPART_HD void refine_packed_pair(int e, int nt, int* a, int* b) {
  if (e < nt) {
    refine_pair(e, a, b);
  } else {
    *a = e - nt;
    *b = -1;
  }
}

// the trial cost over jn bands, ascending: a bad weight raises *bad, a band of weight 0 is skipped.  -> c
SPART_HD double refine_tile_cost(double c, bool* bad, int jn, const double* w, int SW, const double* y, int SY, const double* obs,
                                 int SO) {
  SPART_NO_CONTRACT
  for (int jj = 0; jj < jn; ++jj) {
    const double wj = w[jj * SW];
    if (refine_bad_weight(wj)) *bad = true;
    if (wj == 0.0) continue;
    c = refine_cost_band(c, wj, y[jj * SY], obs[jj * SO]);
  }
  return c;
}

// the prior's cost terms, unknowns ascending; t(f): the trial value of unknown f.  -> c
template <typename T>
SPART_HD double refine_prior_total_of(int n, double c, bool* bad, T&& t, const double* mu, const double* pw) {
  SPART_NO_CONTRACT
  for (int f = 0; f < n; ++f) {
    const double p = pw[f];
    if (refine_bad_weight(p)) *bad = true;
    if (p == 0.0) continue;
    c = refine_prior_cost(c, p, t(f), mu[f]);
  }
  return c;
}
SPART_HD double refine_prior_total(int n, double c, bool* bad, const double* t, const double* mu, const double* pw) {
  return refine_prior_total_of(n, c, bad, [t](int f) { return t[f]; }, mu, pw);
}

// The decision of one call on one observation.  it == 0: alive (1) or dead from the start (2, na = -1).  Later: a dead one
// (na < 0) stays as it is, code 0; otherwise accepted (1: ct < cost, one more in na) or rejected (3), and lambda moves.
struct RefineDecision {
  int code, na;
  double lam;
};
SPART_HD RefineDecision refine_decide(int it, double ct, bool bad, double cost, double lam, int na) {
  RefineDecision d = {0, na, lam};
  if (it == 0) {
    d.code = (ct < __builtin_inf() && !bad) ? 1 : 2;
    if (d.code == 2) d.na = -1;
  } else if (na >= 0) {
    d.code = ct < cost ? 1 : 3;
    d.lam = refine_lambda(lam, d.code == 1);
    if (d.code == 1) ++d.na;
  }
  return d;
}

// one packed sum over the bands jb .. je - 1 of a tile, ascending, bands of weight 0 skipped.  -> acc
SPART_HD double refine_tile_sum(double acc, int jb, int je, const double* w, int SW, const double* ja, int SA, const double* jc,
                                int SC) {
  SPART_NO_CONTRACT
  for (int jj = jb; jj < je; ++jj) {
    const double wj = w[jj * SW];
    if (wj == 0.0) continue;
    acc = refine_mac(acc, wj, ja[jj * SA], jc[jj * SC]);
  }
  return acc;
}

// the prior's part of the sums of an accepted point x: A_aa + p_a and, where the packed vector has its g (mu != NULL: the
// posterior's has none), g_a + p_a e_a
SPART_HD void refine_prior_augment(int n, double* A, int SA, const double* x, int SX, const double* mu, const double* pw) {
  SPART_NO_CONTRACT
  for (int a = 0; a < n; ++a) {
    const double p = pw[a];
    if (p == 0.0) continue;
    double* Aaa = A + refine_tri(a, a) * SA;
    *Aaa = *Aaa + p;
    if (!mu) continue;
    double* ga = A + (refine_ntri(n) + a) * SA;
    *ga = refine_prior_gain(*ga, p, refine_residual(x[a * SX], mu[a]));
  }
}

// In-place Cholesky of a packed lower triangle, textbook row order, sums over k ascending; false at a pivot !(s > 0)
SPART_HD bool refine_cholesky(int F, double* L, int S) {
  SPART_NO_CONTRACT
  for (int i = 0; i < F; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = L[refine_tri(i, j) * S];
      for (int k = 0; k < j; ++k) s = s - L[refine_tri(i, k) * S] * L[refine_tri(j, k) * S];
      if (i == j) {
        if (!(s > 0.0)) return false;
        L[refine_tri(i, i) * S] = __builtin_sqrt(s);
      } else {
        L[refine_tri(i, j) * S] = s / L[refine_tri(j, j) * S];
      }
    }
  }
  return true;
}

// The next trial: B = A + lam diag(D), D_a = A_aa if A_aa > 0 else 1; B delta = -g by Cholesky, forward and back
// substitution; a failed factorisation or a non-finite delta_f gives delta = 0; t = clip(x + delta).
// A: packed (triangle then g).  L (F (F + 1) / 2) and d (F) are scratch.  lo / hi are dense.
SPART_HD void refine_propose(int F, const double* A, int SA, double lam, const double* x, int SX, const double* lo, const double* hi,
                             double* L, int SL, double* d, int SD, double* t, int ST) {
  SPART_NO_CONTRACT
  const int nt = refine_ntri(F);
  for (int a = 0; a < F; ++a)
    for (int b = 0; b <= a; ++b) {
      double v = A[refine_tri(a, b) * SA];
      if (a == b) v = v + lam * (v > 0.0 ? v : 1.0);
      L[refine_tri(a, b) * SL] = v;
    }
  bool ok = refine_cholesky(F, L, SL);
  if (ok) {
    for (int i = 0; i < F; ++i) {
      double s = -A[(nt + i) * SA];
      for (int k = 0; k < i; ++k) s = s - L[refine_tri(i, k) * SL] * d[k * SD];
      d[i * SD] = s / L[refine_tri(i, i) * SL];
    }
    for (int i = F - 1; i >= 0; --i) {
      double s = d[i * SD];
      for (int k = i + 1; k < F; ++k) s = s - L[refine_tri(k, i) * SL] * d[k * SD];
      d[i * SD] = s / L[refine_tri(i, i) * SL];
    }
    for (int f = 0; f < F; ++f) {
      const double v = d[f * SD];
      if (!(v - v == 0.0)) ok = false;                       // NaN or +-inf
    }
  }
  for (int f = 0; f < F; ++f) {
    const double dl = ok ? d[f * SD] : 0.0;
    t[f * ST] = refine_clip(x[f * SX] + dl, lo[f], hi[f]);
  }
}

// std_f from the undamped A: A = L L^T; L z = e_f; var_f = sum_{k >= f} z_k^2 (k ascending); all NaN when the factorisation
// fails.  L (F (F + 1) / 2) and z (F) are scratch.
SPART_HD void refine_std(int F, const double* A, int SA, double* L, int SL, double* z, int SZ, double* out, int SO) {
  SPART_NO_CONTRACT
  const int nt = refine_ntri(F);
  for (int e = 0; e < nt; ++e) L[e * SL] = A[e * SA];
  if (!refine_cholesky(F, L, SL)) {
    for (int f = 0; f < F; ++f) out[f * SO] = __builtin_nan("");
    return;
  }
  for (int f = 0; f < F; ++f) {
    double var = 0.0;
    for (int k = f; k < F; ++k) {
      double s = k == f ? 1.0 : 0.0;
      for (int i = f; i < k; ++i) s = s - L[refine_tri(k, i) * SL] * z[i * SZ];
      const double zk = s / L[refine_tri(k, k) * SL];
      z[k * SZ] = zk;
      var = var + zk * zk;
    }
    out[f * SO] = __builtin_sqrt(var);
  }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: the kernels.  One chunk of Mc observations owns
//   table  (27, (F + 1) Mc) float64, row = f Mc + m: the parameter columns of the next forward call -- block f = 0 holds
//          the trial points, block f = 1 .. F the same points with free column f - 1 moved by its finite-difference step;
//   cols   ((F + 1) Mc, nb) float64: the forward call's chosen sensor column, same row order;
//   state  t (Mc, F) the trial that `table` holds, A (Mc, P) the packed normal equations of the last accepted point,
//          lam (Mc), na (Mc) accepted steps (-1: dead);  x and cost, the caller's outputs, ARE the accepted point and its cost.
// k_refine_views_init (spart_refine_views.h, at V = 1 and Fs = F) writes all of `table` once; k_refine_step only ever rewrites
// its F free rows.
//
// k_refine_step.  Single-wave workgroups of W consecutive observations (W = 8, or 4 where 8 do not fit REFINE_LDS_BUDGET:
// refine_group).  The rows of one block f of `cols` that belong to W consecutive observations are ONE contiguous run of
// W nb doubles, so a tile of REFINE_JT bands is staged through LDS with band-contiguous lanes and then read one column per
// lane.  Everything indexed by the run-time F lives in LDS at [k][o], row stride W + 1 doubles (lane o touches column o only;
// the odd stride spreads the band-contiguous staging stores over the banks): no register array is indexed by a run-time
// value, so nothing goes to scratch.  The prior (pmu / ppw, NULL without one) has no LDS rows: lane o reads its observation's
// at most 2 F doubles from global memory in the two per-observation phases that use them.
//   pass 1   lane o < W: the trial cost of observation o from block 0, bands ascending, then the prior's terms (f ascending),
//            then the decision;
//   pass 2   (only for accepted or newly dead observations) all F + 1 blocks: y, r_j, J_jf in place of Y_f, then the
//            P = F (F + 1) / 2 + F sums of an observation dealt to its 64 / W lanes, each one sequential in j; then lane
//            o < W adds the prior's p_a to A_aa and p_a e_a to g_a, so the state holds the augmented sums;
//   finish   lane o < W: lambda, then either the damped solve and the F (F + 1) new table entries, or (last call) std.
// The per-entry order is the definition's whatever W is, so the mapping is free of the result.
constexpr int REFINE_JT = 16;                // bands per LDS tile (128 B of a row)
constexpr int REFINE_LDS_BUDGET = 40960;     // dynamic LDS of one workgroup at most: three workgroups fit a CU's 160 KiB
// Measured (tools/refine_rate.py, F = 6, nb = 13): groups of 4 and 8 observations take the same time, 16 take 1.2x and 32 take
// 2x as long per iteration -- a group is one wave whose per-observation phases run on W lanes, and what hides their latency is
// the number of waves a CU holds, which the LDS of a group limits.  At F = 16 a group of 4 beats 8.
constexpr int REFINE_MIN_GROUP = 4, REFINE_MAX_GROUP = 8;

// The LDS of a step kernel of the family, one formula.  Doubles per observation column (+ one int flag): tile_rows tiles of
// JT bands, weights and obs / r, the packed sums and the Cholesky factor of n unknowns, x / step / trial, `extra` rows of the
// kernel's own.  k_refine_step: (F + 1, F, 0); k_refine_views_step: (F + 1, n, 0); k_refine_mix_step: (n, n, MIX_MAXV).
inline int refine_lds_rows(int tile_rows, int n, int extra) {
  return tile_rows * REFINE_JT + 2 * REFINE_JT + (refine_ntri(n) + n) + refine_ntri(n) + 3 * n + 1 + extra;
}
inline size_t refine_lds_bytes(int rows, int W) { return (size_t)rows * (size_t)(W + 1) * 8; }
// observations per workgroup
inline int refine_group(int rows) {
  int W = REFINE_MAX_GROUP;
  while (W > REFINE_MIN_GROUP && refine_lds_bytes(rows, W) > (size_t)REFINE_LDS_BUDGET) W >>= 1;
  return W;
}

struct RefineCfg {
  const double* base[NPARAM];            // the caller's start columns (each (M,))
  const double* freebase[REFINE_MAXF];   // base[free[f]]
  int32_t is_free[NPARAM];
  int32_t free_col[REFINE_MAXF];
  double lo[REFINE_MAXF], hi[REFINE_MAXF], h[REFINE_MAXF];
};

// device copy of the per-call constants, written by the init kernel: lo, hi, h (REFINE_MAXF doubles each)
constexpr int REFINE_CFG_DOUBLES = 3 * REFINE_MAXF;

// ---- what the kernels of the family share beside part 1 (the init kernel of spart_refine itself is k_refine_views_init at
// V = 1, Fs = F: spart_refine_views.h)

// One value of a parameter column in all F + 1 blocks of a table (blk doubles from block to block): block `hot` gets `moved`,
// every other one v; hot < 0: none, a fixed parameter
__device__ __forceinline__ void refine_fill_row(double* row, int F, int64_t blk, int hot, double v, double moved) {
  for (int fp = 0; fp <= F; ++fp) row[(int64_t)fp * blk] = fp == hot ? moved : v;
}

// the fixed parameters of table row i (R doubles per parameter) from the caller's columns at src
__device__ __forceinline__ void refine_fill_fixed(const RefineCfg& a, int64_t src, double* table_i, int64_t R, int F, int64_t blk) {
#pragma unroll
  for (int p = 0; p < NPARAM; ++p) {
    if (a.is_free[p]) continue;
    refine_fill_row(table_i + p * R, F, blk, -1, a.base[p][src], 0.0);
  }
}

// thread u < REFINE_MAXF of an init kernel: the device copy of lo / hi / h of name fn (none: fn < 0) as unknown u's, and
// free_col[u]
__device__ __forceinline__ void refine_cfg_copy(const RefineCfg& a, int u, int fn, double* cfg, int32_t* cfg_free) {
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f == fn) {
      cfg[u] = a.lo[f];
      cfg[REFINE_MAXF + u] = a.hi[f];
      cfg[2 * REFINE_MAXF + u] = a.h[f];
    }
    if (f == u) cfg_free[u] = a.free_col[f];
  }
}

// The weight and observation tile of bands j0 .. j0 + JT - 1 of a group's W observations, nobs of them there: lanes run along
// the bands (out of range: weight 0).  obs_g / wts_g: the group's rows of nj bands, `stride` doubles apart (wts_g NULL: weight
// 1; wper == 0: one shared row, band j at wts_g[widx(j)]).  -> wl / rl [jj][o], row stride WP
template <typename WIdx>
__device__ __forceinline__ void refine_stage_obs(int lane, int W, int WP, int nobs, int j0, int nj, int stride, const double* obs_g,
                                                 const double* wts_g, int wper, WIdx&& widx, double* wl, double* rl) {
  constexpr int JT = REFINE_JT;
  for (int i = lane; i < W * JT; i += 64) {
    const int jj = i % JT, o = i / JT, j = j0 + jj;
    double w = 0.0, ob = 0.0;
    if (o < nobs && j < nj) {
      w = wts_g ? wts_g[wper ? o * stride + j : widx(j)] : 1.0;
      ob = obs_g[o * stride + j];
    }
    wl[jj * WP + o] = w;
    rl[jj * WP + o] = ob;
  }
}

// accepted (flag 1): the new packed sums become the state; rejected (3): the state's sums come back.  sA_g: the group's rows
__device__ __forceinline__ void refine_exchange(int lane, int W, int WP, int P, int nobs, const int* flag, double* Al, double* sA_g) {
  for (int i = lane; i < P * W; i += 64) {
    const int e = i % P, o = i / P;
    if (o >= nobs) continue;
    const int fl = flag[o];
    if (fl == 1) sA_g[i] = Al[e * WP + o];
    else if (fl == 3) Al[e * WP + o] = sA_g[i];
  }
}

// the last call's outputs of an observation that is alive: n_accept and std (each NULL: not asked for) at the observation's
// own entry / row; A, L, d, t: its LDS columns
__device__ __forceinline__ void refine_last_out(int n, int na, int32_t* n_accept, double* sdev, const double* A, double* L, double* d,
                                                double* t, int WP) {
  if (n_accept) *n_accept = na;
  if (sdev) {
    refine_std(n, A, WP, L, WP, d, WP, t, WP);
    for (int f = 0; f < n; ++f) sdev[f] = t[f * WP];
  }
}

// outputs of the call, already moved to the chunk's first observation; cost0 / sdev / n_accept / y may be NULL
struct RefineOut {
  double *x, *cost, *cost0, *sdev;
  int32_t* n_accept;
  double* y;
};

// Once per iteration `it` (last: it == n_iter).  obs / wts are the chunk's rows ((Mc, nb); wts NULL, or (nb,) with
// wper == 0, or the chunk's rows with wper == 1).  pmu / ppw: both NULL (no prior), or the prior's mean and weight, (F,) with
// pper == 0 or the chunk's rows of (M, F) with pper == 1.
__global__ __launch_bounds__(64) void k_refine_step(const double* __restrict__ cols, const double* __restrict__ obs,
                                                    const double* __restrict__ wts, int wper, const double* __restrict__ cfg,
                                                    const int32_t* __restrict__ cfg_free, double* __restrict__ table, int Mc, int F,
                                                    int nb, int W, int it, int last, double* __restrict__ st,
                                                    double* __restrict__ sA, double* __restrict__ slam, int32_t* __restrict__ sna,
                                                    RefineOut out, const double* __restrict__ pmu,
                                                    const double* __restrict__ ppw, int pper) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char refine_smem[];
  constexpr int JT = REFINE_JT;
  const int WP = W + 1, nt = refine_ntri(F), P = nt + F, G = 64 / W;
  double* Yl = reinterpret_cast<double*>(refine_smem);   // [(f JT + jj)][o]: the Y_f tile, J_jf in place for f >= 1
  double* wl = Yl + (F + 1) * JT * WP;                   // [jj][o] weights (0: skip the band)
  double* rl = wl + JT * WP;                             // [jj][o] obs, then r
  double* Al = rl + JT * WP;                             // [e][o] packed sums
  double* Ll = Al + P * WP;                              // [e][o] Cholesky factor
  double* xl = Ll + nt * WP;                             // [f][o] accepted point
  double* dl = xl + F * WP;                              // [f][o] s_f h_f, then the solve's scratch
  double* tl = dl + F * WP;                              // [f][o] next trial / std
  int* flag = reinterpret_cast<int*>(tl + F * WP);       // [o] 0 idle, 1 accepted, 2 dead since this call, 3 rejected
  const double* lo = cfg;
  const double* hi = cfg + REFINE_MAXF;
  const double* hh = cfg + 2 * REFINE_MAXF;
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * W;                         // first observation of the group
  const int m = g0 + lane;                               // (lanes < W) this lane's observation
  const bool mine = lane < W && m < Mc;
  const int64_t R = (int64_t)(F + 1) * Mc;
  const double* obs_g = obs + (int64_t)g0 * nb;
  const double* wts_g = wts ? (wper ? wts + (int64_t)g0 * nb : wts) : nullptr;
  const bool prior = ppw != nullptr;                     // (kernel-uniform)
  const int64_t pm = pper && mine ? (int64_t)m * F : 0;  // (lanes < W) where this lane's prior starts

  auto stage_obs = [&](int j0) {
    refine_stage_obs(lane, W, WP, Mc - g0, j0, nb, nb, obs_g, wts_g, wper, [](int j) { return j; }, wl, rl);
  };

  // ---- pass 1: the trial cost from block 0
  double ct = 0.0;
  bool bad = false;
  for (int j0 = 0; j0 < nb; j0 += JT) {
    __syncthreads();
    stage_obs(j0);
    const double* y0 = cols + (int64_t)g0 * nb;
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      Yl[jj * WP + o] = (g0 + o < Mc && j < nb) ? y0[o * nb + j] : 0.0;
    }
    __syncthreads();
    if (mine) ct = refine_tile_cost(ct, &bad, JT, wl + lane, WP, Yl + lane, WP, rl + lane, WP);
  }
  if (prior && mine) ct = refine_prior_total(F, ct, &bad, st + (int64_t)m * F, pmu + pm, ppw + pm);
  // ---- the decision
  int code = 0, na = 0;
  double lam = 0.0;
  if (mine) {
    const RefineDecision d = refine_decide(it, ct, bad, it == 0 ? 0.0 : out.cost[m], slam[m], sna[m]);
    code = d.code, na = d.na, lam = d.lam;
    if (it == 0 && out.cost0) out.cost0[m] = ct;
    if (code == 2) {
      out.cost[m] = ct;
      if (out.n_accept) out.n_accept[m] = -1;
      if (out.sdev)
        for (int f = 0; f < F; ++f) out.sdev[(int64_t)m * F + f] = __builtin_nan("");
    }
    if (code == 1) out.cost[m] = ct;
    if (code != 0) {
      slam[m] = lam;
      sna[m] = na;
    }
    for (int f = 0; f < F; ++f) {
      const double tf = st[(int64_t)m * F + f];
      double xf = tf;
      if (code == 1) out.x[(int64_t)m * F + f] = tf;
      else xf = out.x[(int64_t)m * F + f];
      xl[f * WP + lane] = xf;
      dl[f * WP + lane] = refine_fd_step(tf, hh[f], hi[f]);
    }
  }
  if (lane < W) flag[lane] = code;
  const bool fresh = __builtin_amdgcn_ballot_w64(code == 1 || code == 2) != 0;     // (wave-uniform)
  __syncthreads();

  // ---- pass 2: y, r, J and the sums of the observations that moved
  if (fresh) {
    for (int i = lane; i < P * W; i += 64) Al[(i / W) * WP + i % W] = 0.0;
    for (int j0 = 0; j0 < nb; j0 += JT) {
      __syncthreads();
      stage_obs(j0);
      for (int i = lane; i < (F + 1) * W * JT; i += 64) {
        const int jj = i % JT, o = (i / JT) % W, f = i / (JT * W), j = j0 + jj;
        const int fl = flag[o];
        const bool in = g0 + o < Mc && j < nb && (fl == 1 || (fl == 2 && f == 0));
        const double* yf = cols + ((int64_t)f * Mc + g0) * nb;
        Yl[(f * JT + jj) * WP + o] = in ? yf[o * nb + j] : 0.0;
      }
      __syncthreads();
      // r_j (block 0's lanes) and J_jf (the others); Y_0 itself is only read here
      double* y_g = out.y ? out.y + (int64_t)g0 * nb : nullptr;
      for (int i = lane; i < (F + 1) * W * JT; i += 64) {
        const int jj = i % JT, o = (i / JT) % W, f = i / (JT * W), j = j0 + jj;
        const int fl = flag[o];
        if (!(g0 + o < Mc && j < nb) || (fl != 1 && fl != 2)) continue;
        const double y0 = Yl[jj * WP + o];
        if (f == 0) {
          if (y_g) y_g[o * nb + j] = y0;
          if (wl[jj * WP + o] != 0.0) rl[jj * WP + o] = refine_residual(y0, rl[jj * WP + o]);
        } else if (fl == 1) {
          Yl[(f * JT + jj) * WP + o] = refine_jacobian(Yl[(f * JT + jj) * WP + o], y0, dl[(f - 1) * WP + o]);
        }
      }
      __syncthreads();
      {
        const int o = lane % W, q = lane / W;
        if (flag[o] == 1) {
          const int jn = nb - j0 < JT ? nb - j0 : JT;
          for (int e = q; e < P; e += G) {
            int a, b;                                      // A_ab, or (b < 0) g_a against r
            refine_packed_pair(e, nt, &a, &b);
            const double* ja = Yl + ((a + 1) * JT) * WP + o;
            const double* jb = b >= 0 ? Yl + ((b + 1) * JT) * WP + o : rl + o;
            Al[e * WP + o] = refine_tile_sum(Al[e * WP + o], 0, jn, wl + o, WP, ja, WP, jb, WP);
          }
        }
      }
    }
    __syncthreads();
    if (prior) {
      if (mine && code == 1) refine_prior_augment(F, Al + lane, WP, xl + lane, WP, pmu + pm, ppw + pm);
      __syncthreads();
    }
  }
  refine_exchange(lane, W, WP, P, Mc - g0, flag, Al, sA + (int64_t)g0 * P);
  __syncthreads();

  // ---- finish: the next trial and its table rows, or the outputs of the last call
  if (mine && (code == 1 || code == 3)) {
    if (!last) {
      refine_propose(F, Al + lane, WP, lam, xl + lane, WP, lo, hi, Ll + lane, WP, dl + lane, WP, tl + lane, WP);
      for (int f = 0; f < F; ++f) {
        const double tf = tl[f * WP + lane];
        st[(int64_t)m * F + f] = tf;
        refine_fill_row(table + cfg_free[f] * R + m, F, Mc, f + 1, tf, tf + refine_fd_step(tf, hh[f], hi[f]));
      }
    } else {
      refine_last_out(F, na, out.n_accept ? out.n_accept + m : nullptr, out.sdev ? out.sdev + (int64_t)m * F : nullptr, Al + lane,
                      Ll + lane, dl + lane, tl + lane, WP);
    }
  }
}
#endif  // __HIPCC__

}  // namespace spart
