// What the optimal-estimation fit of spart_refine knows about a point and used to throw away: the Jacobian of the sensor
// column, the posterior covariance A^-1 = (J^T W J + S_a^-1)^-1, the averaging kernel A^-1 J^T W J and its trace
// (spart_refine_posterior, include/spart_hip.h; the definition is tools/refine_posterior_defined.py and every function here
// reproduces it bit for bit).
//
// Part 1: the per-observation arithmetic behind refine_cholesky, as plain strided functions under SPART_NO_CONTRACT like those
// of spart_refine.h (element k of an array at p[k * S]).  hipcc compiles them into the kernel of part 2 and g++ compiles them
// for tests/hostmath/refine_posterior_host.cpp.
//
// Index conventions are spart_refine.h's.  Z = L^-1 is lower triangular and packed like L: Z_kf, k >= f, at refine_tri(k, f).
// cov is symmetric and kept as its packed lower triangle; K, the data part J^T W J, is needed in full, K_ab at a F + b.
#pragma once

#include "spart_refine.h"

namespace spart {

// Z = L^-1, column f by refine_std's recurrence: z_k = ((k == f) - sum_{f <= i < k} L_ki z_i) / L_kk, i ascending
SPART_HD void refine_inverse_lower(int F, const double* L, int SL, double* Z, int SZ) {
  SPART_NO_CONTRACT
  for (int f = 0; f < F; ++f)
    for (int k = f; k < F; ++k) {
      double s = k == f ? 1.0 : 0.0;
      for (int i = f; i < k; ++i) s = s - L[refine_tri(k, i) * SL] * Z[refine_tri(i, f) * SZ];
      Z[refine_tri(k, f) * SZ] = s / L[refine_tri(k, k) * SL];
    }
}

// cov_ab = (Z^T Z)_ab for a >= b: v = 0; for k = a ... F-1: v = v + Z_ka Z_kb.  cov_ff is refine_std's var_f bit for bit.
SPART_HD double refine_cov(int F, const double* Z, int SZ, int a, int b) {
  SPART_NO_CONTRACT
  double v = 0.0;
  for (int k = a; k < F; ++k) v = v + Z[refine_tri(k, a) * SZ] * Z[refine_tri(k, b) * SZ];
  return v;
}

// entry (a, b) of a symmetric matrix kept as its packed lower triangle
SPART_HD double refine_sym(const double* P, int S, int a, int b) { return P[(a >= b ? refine_tri(a, b) : refine_tri(b, a)) * S]; }

// ak_ab = 0; for c = 0 ... F-1: ak_ab = ak_ab + cov_ac K_cb.  cov packed, K full
SPART_HD double refine_avk(int F, const double* cov, int SC, const double* K, int SK, int a, int b) {
  SPART_NO_CONTRACT
  double v = 0.0;
  for (int c = 0; c < F; ++c) v = v + refine_sym(cov, SC, a, c) * K[(c * F + b) * SK];
  return v;
}

// dfs = 0; for a ascending: dfs = dfs + ak_aa.  d: the F diagonal entries
SPART_HD double refine_trace(int F, const double* d, int S) {
  SPART_NO_CONTRACT
  double v = 0.0;
  for (int a = 0; a < F; ++a) v = v + d[a * S];
  return v;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: k_refine_posterior.  It runs behind k_refine_views_init at V = 1 (whose table holds the point and its F neighbours)
// and one forward call, on refine_impl's chunk layout: cols ((F + 1) Mc, nb), row = f Mc + m; t (Mc, F) the clipped point.
//
// The shape is k_refine_step's: single-wave workgroups of W consecutive observations, tiles of REFINE_JT bands staged through
// LDS with band-contiguous lanes, everything indexed by the run-time F in LDS at [k][o] with the odd row stride W + 1, sums and
// matrix entries of an observation dealt to its 64 / W lanes -- each entry is sequential in its own index, so the mapping
// cannot enter the result.
//   pass 1   lane o < W: cost (bands ascending, then the prior), nband, dead or alive;
//   pass 2   all F + 1 blocks per tile: y out, J_jf in place of Y_f and out to global memory -- the nb F doubles of an
//            observation are contiguous and a tile's jn F of them are one run, written by consecutive lanes --, then the
//            F (F + 1) / 2 sums of K;
//   finish   K mirrored to full; lane o < W: the prior's diagonal, Cholesky in place, Z; dealt: cov (packed), then cov out and
//            ak; lane o < W: std, dfs, status.
// LDS rows per observation column: the (F + 1) JT tile, weights and observations (2 JT), three triangles (A / L, Z, cov), the
// full K (F^2), the step, the diagonal of ak, a flag.  At F = 16 that is 1001 rows: a group of 4 takes 40 040 bytes, so three
// workgroups fit a CU's 160 KiB like k_refine_step's; F <= 10 leaves room for groups of 8 (refine_posterior_group).
constexpr int REFINE_POST_LDS_BUDGET = 40960;
constexpr int REFINE_POST_MIN_GROUP = 4, REFINE_POST_MAX_GROUP = 8;

inline int refine_posterior_lds_rows(int F) { return (F + 1) * REFINE_JT + 2 * REFINE_JT + 3 * refine_ntri(F) + F * F + 2 * F + 1; }
inline size_t refine_posterior_lds_bytes(int F, int W) { return (size_t)refine_posterior_lds_rows(F) * (size_t)(W + 1) * 8; }
inline int refine_posterior_group(int F) {
  int W = REFINE_POST_MAX_GROUP;
  while (W > REFINE_POST_MIN_GROUP && refine_posterior_lds_bytes(F, W) > (size_t)REFINE_POST_LDS_BUDGET) W >>= 1;
  return W;
}

// outputs of the call (spart_posterior_out without x, which the init kernel writes), moved to the chunk's first observation;
// each may be NULL
struct PosteriorOut {
  double *y, *jac, *cov, *ak, *sdev, *dfs, *cost;
  int32_t *nband, *status;
};

// obs may be NULL (the band loop of the cost then adds nothing); wts / pmu / ppw as k_refine_step's.  W is a template
// parameter (refine_posterior_group gives 4 or 8): the group's strides and divisions are then constants, which keeps the
// kernel's many uniform values -- nine output pointers among them -- within the scalar registers.
template <int W>
__global__ __launch_bounds__(64) void k_refine_posterior(const double* __restrict__ cols, const double* __restrict__ obs,
                                                         const double* __restrict__ wts, int wper, const double* __restrict__ cfg,
                                                         int Mc, int F, int nb, const double* __restrict__ st,
                                                         PosteriorOut out, const double* __restrict__ pmu,
                                                         const double* __restrict__ ppw, int pper) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char refine_post_smem[];
  constexpr int JT = REFINE_JT;
  constexpr int WP = W + 1, G = 64 / W;
  const int nt = refine_ntri(F), FF = F * F;
  double* Yl = reinterpret_cast<double*>(refine_post_smem);   // [(f JT + jj)][o]: the Y_f tile, J_jf in place for f >= 1
  double* wl = Yl + (F + 1) * JT * WP;                        // [jj][o] weights (0: skip the band)
  double* rl = wl + JT * WP;                                  // [jj][o] obs
  double* Al = rl + JT * WP;                                  // [e][o] packed K, then A, then L
  double* Zl = Al + nt * WP;                                  // [e][o] packed L^-1
  double* Cl = Zl + nt * WP;                                  // [e][o] packed cov
  double* Kl = Cl + nt * WP;                                  // [a F + b][o] full K
  double* dl = Kl + FF * WP;                                  // [f][o] s_f h_f
  double* gl = dl + F * WP;                                   // [a][o] ak_aa
  int* flag = reinterpret_cast<int*>(gl + F * WP);            // [o] 0 idle, 1 alive, 2 dead, 4 alive but A not positive definite
  const double* hi = cfg + REFINE_MAXF;
  const double* hh = cfg + 2 * REFINE_MAXF;
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * W;                              // first observation of the group
  const int m = g0 + lane;                                    // (lanes < W) this lane's observation
  const bool mine = lane < W && m < Mc;
  const bool prior = ppw != nullptr;                          // (kernel-uniform)
  const int64_t pm = pper && mine ? (int64_t)m * F : 0;       // (lanes < W) where this lane's prior starts
  const double nan = __builtin_nan("");

  // the weight tile of bands j0 .. j0 + JT - 1: lanes run along the bands (out of range: weight 0)
  auto stage_weights = [&](int j0) {
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      double w = 0.0;
      if (g0 + o < Mc && j < nb) w = wts ? (wper ? wts[((int64_t)g0 + o) * nb + j] : wts[j]) : 1.0;
      wl[jj * WP + o] = w;
    }
  };

  // ---- pass 1: the cost from block 0, the count of weighted bands
  double ct = 0.0;
  bool bad = false;
  int nw = 0;
  for (int j0 = 0; j0 < nb; j0 += JT) {
    __syncthreads();
    stage_weights(j0);
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      const bool in = g0 + o < Mc && j < nb;
      const int64_t at = ((int64_t)g0 + o) * nb + j;
      Yl[jj * WP + o] = in ? cols[at] : 0.0;
      rl[jj * WP + o] = in && obs ? obs[at] : 0.0;
    }
    __syncthreads();
    if (mine) {
      for (int jj = 0; jj < JT; ++jj) nw += wl[jj * WP + lane] != 0.0 ? 1 : 0;
      const double c = refine_tile_cost(ct, &bad, JT, wl + lane, WP, Yl + lane, WP, rl + lane, WP);
      if (obs) ct = c;                                          // (without obs the tile only raises `bad`)
    }
  }
  if (prior && mine) ct = refine_prior_total(F, ct, &bad, st + (int64_t)m * F, pmu + pm, ppw + pm);
  int code = 0;
  if (mine) {
    code = (ct < __builtin_inf() && !bad) ? 1 : 2;
    if (out.cost) out.cost[m] = ct;
    if (out.nband) out.nband[m] = nw;
    for (int f = 0; f < F; ++f) dl[f * WP + lane] = refine_fd_step(st[(int64_t)m * F + f], hh[f], hi[f]);
  }
  if (lane < W) flag[lane] = code;
  __syncthreads();

  // ---- pass 2: y, J (kept and written out) and the sums of K
  for (int i = lane; i < nt * W; i += 64) Al[(i / W) * WP + i % W] = 0.0;
  for (int j0 = 0; j0 < nb; j0 += JT) {
    const int jn = nb - j0 < JT ? nb - j0 : JT;
    __syncthreads();
    stage_weights(j0);
    for (int i = lane; i < (F + 1) * W * JT; i += 64) {
      const int jj = i % JT, o = (i / JT) % W, f = i / (JT * W), j = j0 + jj;
      const bool in = g0 + o < Mc && j < nb;
      const double* yf = cols + ((int64_t)f * Mc + g0) * nb;
      Yl[(f * JT + jj) * WP + o] = in ? yf[o * nb + j] : 0.0;
    }
    __syncthreads();
    double* y_g = out.y ? out.y + (int64_t)g0 * nb : nullptr;
    for (int i = lane; i < (F + 1) * W * JT; i += 64) {
      const int jj = i % JT, o = (i / JT) % W, f = i / (JT * W), j = j0 + jj;
      if (!(g0 + o < Mc && j < nb)) continue;
      const double y0 = Yl[jj * WP + o];
      if (f == 0) {
        if (y_g) y_g[o * nb + j] = y0;
      } else {
        Yl[(f * JT + jj) * WP + o] = flag[o] == 1 ? refine_jacobian(Yl[(f * JT + jj) * WP + o], y0, dl[(f - 1) * WP + o]) : nan;
      }
    }
    __syncthreads();
    if (out.jac) {
      // observation o's entries (j0 + jj, f), jj < jn, are the jn F consecutive doubles from ((g0 + o) nb + j0) F
      const int run = jn * F;
      for (int i = lane; i < W * run; i += 64) {
        const int o = i / run, e = i - o * run, jj = e / F, f = e - jj * F;
        if (g0 + o >= Mc) continue;
        out.jac[((int64_t)(g0 + o) * nb + j0) * F + e] = Yl[((f + 1) * JT + jj) * WP + o];
      }
    }
    {
      const int o = lane % W, q = lane / W;
      if (flag[o] == 1)
        for (int e = q; e < nt; e += G) {
          int a, b;
          refine_pair(e, &a, &b);
          const double* ja = Yl + ((a + 1) * JT) * WP + o;
          const double* jb = Yl + ((b + 1) * JT) * WP + o;
          Al[e * WP + o] = refine_tile_sum(Al[e * WP + o], 0, jn, wl + o, WP, ja, WP, jb, WP);
        }
    }
  }
  __syncthreads();

  // ---- finish
  const int o = lane % W, q = lane / W;                      // the dealt phases: lane (o, q) takes entries q, q + G, ...
  const bool there = g0 + o < Mc;
  if (there && flag[o] == 1)
    for (int e = q; e < FF; e += G) {
      const int a = e / F, b = e - a * F;
      Kl[e * WP + o] = refine_sym(Al + o, WP, a, b);
    }
  __syncthreads();
  if (mine && code == 1) {
    if (prior) refine_prior_augment(F, Al + lane, WP, nullptr, 0, nullptr, ppw + pm);     // (K has no g)
    if (refine_cholesky(F, Al + lane, WP)) refine_inverse_lower(F, Al + lane, WP, Zl + lane, WP);
    else flag[lane] = 4;
  }
  __syncthreads();
  const int fl = there ? flag[o] : 0;
  if (fl == 1)
    for (int e = q; e < nt; e += G) {
      int a, b;
      refine_pair(e, &a, &b);
      Cl[e * WP + o] = refine_cov(F, Zl + o, WP, a, b);
    }
  __syncthreads();
  if (fl != 0) {
    const int64_t mo = (int64_t)(g0 + o) * FF;
    for (int e = q; e < FF; e += G) {
      const int a = e / F, b = e - a * F;
      double c = nan, k = nan;
      if (fl == 1) {
        c = refine_sym(Cl + o, WP, a, b);
        k = refine_avk(F, Cl + o, WP, Kl + o, WP, a, b);
        if (a == b) gl[a * WP + o] = k;
      }
      if (out.cov) out.cov[mo + e] = c;
      if (out.ak) out.ak[mo + e] = k;
    }
  }
  __syncthreads();
  if (mine) {
    const int f1 = flag[lane];
    if (out.status) out.status[m] = f1 == 1 ? 0 : f1 == 4 ? 1 : -1;
    if (out.sdev)
      for (int f = 0; f < F; ++f)
        out.sdev[(int64_t)m * F + f] = f1 == 1 ? __builtin_sqrt(Cl[refine_tri(f, f) * WP + lane]) : nan;
    if (out.dfs) out.dfs[m] = f1 == 1 ? refine_trace(F, gl + lane, WP) : nan;
  }
}
#endif  // __HIPCC__

}  // namespace spart
