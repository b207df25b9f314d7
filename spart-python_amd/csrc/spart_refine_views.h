// Joint refinement over V views of a pixel (spart_refine_views, include/spart_hip.h; the definition is
// tools/refine_views_defined.py and every function here reproduces it bit for bit): spart_refine's fit with ONE unknown vector
// per pixel -- Fs shared parameters and Fl local ones per view, n = Fs + V Fl unknowns -- against V observations.  The
// per-entry arithmetic and the per-observation phases are csrc/spart_refine.h's, called with n where it says F; k_refine_step
// is not touched.
//
// Part 1: the index maps, SPART_HD so that g++ compiles them for tests/hostmath/refine_views_host.cpp.
// Index conventions.  free_cols lists the F = Fs + Fl free columns by NAME, the shared ones first; bounds and steps belong to
// a name.  Unknown a < Fs is shared name a; unknown Fs + v Fl + l is local name Fs + l in view v.  Virtual band u = v nb + j.
// Unknown a is ACTIVE in view v when it is shared or a local of v: J_ua exists only there, and a sum skips what is absent.
#pragma once

#include "spart_refine.h"

namespace spart {

constexpr int VIEWS_MAXV = 64;               // views per pixel

// the unknown that free column f takes its value from in view v
SPART_HD int views_unknown(int v, int f, int Fs, int Fl) { return f < Fs ? f : Fs + v * Fl + (f - Fs); }
// the index into free_cols of unknown a
SPART_HD int views_name(int a, int Fs, int Fl) { return a < Fs ? a : Fs + (a - Fs) % Fl; }
// the view of a local unknown, -1 for a shared one
SPART_HD int views_view(int a, int Fs, int Fl) { return a < Fs ? -1 : (a - Fs) / Fl; }

// The tile-to-view map.  A tile holds the virtual bands j0 + jj, jj in [*jb, *je); an unknown of view v (v < 0: shared, the
// range stays) is active in the bands v nb ... (v + 1) nb - 1 only, so the range shrinks to the part of the tile inside that
// view -- empty (*jb >= *je) when the tile has none of it, one or both ends inside the tile when the view straddles it.
SPART_HD void views_clip_range(int v, int nb, int j0, int* jb, int* je) {
  if (v < 0) return;
  const int b = v * nb - j0, e = (v + 1) * nb - j0;
  if (b > *jb) *jb = b;
  if (e < *je) *je = e;
}

// pixels of one chunk: V (F + 1) forward rows each, REFINE_ROWS rows per forward call, one pixel at least
SPART_HD int64_t views_chunk(int V, int F) {
  const int64_t c = REFINE_ROWS / ((int64_t)(F + 1) * V);
  return c > 1 ? c : 1;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: the kernels.  One chunk of Mc pixels owns what a chunk of spart_refine owns, with
//   table  (27, (F + 1) Mc V) float64, row = (f Mc + m) V + v: block f = 0 holds every view's trial row, block f = 1 .. F the
//          same rows with free column f - 1 moved by the step of the unknown it belongs to in that view;
//   cols   ((F + 1) Mc V, nb): the forward call's chosen column in that row order, so block f of pixel m is ONE contiguous
//          run of U = V nb doubles -- the pixel's virtual bands -- and the W pixels of a group are one run of W U;
//   state  t (Mc, n), A (Mc, ntri(n) + n), lam, na (Mc).
// k_refine_views_step is k_refine_step over the virtual bands: the same single-wave groups of W pixels, 16-band LDS tiles,
// [k][o] rows at stride W + 1 for everything indexed by a run-time F or n, the same three phases and per-entry order.  What
// differs: F + 1 blocks of Y but n unknowns (block f at virtual band u holds J of the unknown views_unknown(u / nb, f - 1));
// a packed sum runs over the part of the tile where both its unknowns are active (views_clip_range); (nb,) weights are
// indexed u % nb; and a new trial rewrites V (F + 1) table entries per shared column, F + 1 per local unknown.
// LDS is refine_lds_rows(F + 1, n, 0), and W follows the same budget rule (refine_group): n <= 16 and F <= 16 bound it by what
// k_refine_step takes at F = 16.

// Once per chunk (pixels m0 .. m0 + Mc - 1 of the call's M), one thread per table row of a block: i = m V + v.  `a` is
// spart_refine's RefineCfg with every base column (V, M) view-major and lo / hi / h per name; the device copy `cfg` gets them
// per UNKNOWN (lo, hi, h: REFINE_MAXF doubles each).  A shared unknown starts from view 0's entry: the other views' entries of
// a shared column are never read.  x / t are the chunk's own rows.  At V = 1, Fs = F this is the init kernel of spart_refine
// and spart_refine_posterior: table row f Mc + m, unknown f = free column f.
__global__ __launch_bounds__(256) void k_refine_views_init(RefineCfg a, int64_t M, int64_t m0, int Mc, int V, int F, int Fs,
                                                           double lambda0, double* __restrict__ table, double* __restrict__ x,
                                                           double* __restrict__ t, double* __restrict__ lam,
                                                           int32_t* __restrict__ na, double* __restrict__ cfg,
                                                           int32_t* __restrict__ cfg_free) {
  SPART_NO_CONTRACT
  const int Fl = F - Fs, n = Fs + V * Fl;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && (int)threadIdx.x < REFINE_MAXF) {
    const int u = threadIdx.x;
    refine_cfg_copy(a, u, u < n ? views_name(u, Fs, Fl) : -1, cfg, cfg_free);
  }
  if (i >= Mc * V) return;
  const int m = i / V, v = i % V;
  const int64_t blk = (int64_t)Mc * V, R = (int64_t)(F + 1) * blk;
  const int64_t src = (int64_t)v * M + m0 + m;
  refine_fill_fixed(a, src, table + i, R, F, blk);
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    const double tf = refine_clip(a.freebase[f][f < Fs ? m0 + m : src], a.lo[f], a.hi[f]);
    const double moved = tf + refine_fd_step(tf, a.h[f], a.hi[f]);
    if (f >= Fs || v == 0) {
      const int u = views_unknown(v, f, Fs, Fl);
      x[(int64_t)m * n + u] = tf;
      t[(int64_t)m * n + u] = tf;
    }
    refine_fill_row(table + a.free_col[f] * R + i, F, blk, f + 1, tf, moved);
  }
  if (v == 0) {
    lam[m] = lambda0;
    na[m] = 0;
  }
}

// The arguments of k_refine_views_step, ONE struct so that the kernel can read the members it needs once, late, from the
// kernarg segment where it needs them (LATE below) instead of holding all of them in SGPRs from its first instruction:
// k_refine_step's argument list plus the view maps needs more scalar registers than a wave has, and spills.
// obs / wts are the chunk's rows ((Mc, V, nb); wts NULL, or (nb,) with wper == 0, or the chunk's rows with wper == 1); out is
// RefineOut with x / sdev (M, n) and y (M, V, nb).  pmu / ppw: both NULL, or the prior's mean and weight, (n,) with pper == 0 or
// the chunk's rows of (M, n) with pper == 1.  cfg: lo, hi, h per unknown.  it: the iteration; last: it == n_iter.
struct ViewsStep {
  const double *cols, *obs, *wts, *cfg;
  const int32_t* cfg_free;
  double* table;
  int32_t Mc, V, F, Fs, nb, it, last, wper, pper;
  double *st, *sA, *slam;
  int32_t* sna;
  RefineOut out;
  const double *pmu, *ppw;
};

// Once per iteration.  W (4 or 8: refine_group) is a template parameter: the strides and the lane maps are constants.
// The phases are written out here, not called from spart_refine.h's part 1 and 2 as every other kernel of the family calls
// them: over those functions this kernel had fewer instructions and the same registers, and the whole call measured 0.9 %
// slower, outside the run-to-run spread (profiles/refine_phases_ab.txt).  A change to a phase there is made here as well.
template <int W>
__global__ __launch_bounds__(64) void k_refine_views_step(ViewsStep a) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char refine_views_smem[];
  // (the struct is the only argument, so the kernarg segment starts with it)
#if defined(__HIP_DEVICE_COMPILE__)
  const __attribute__((address_space(4))) ViewsStep* LATE =
      (const __attribute__((address_space(4))) ViewsStep*)__builtin_amdgcn_kernarg_segment_ptr();
#else
  const ViewsStep* LATE = &a;                            // (the host pass only parses the kernel)
#endif
  constexpr int JT = REFINE_JT, WP = W + 1, G = 64 / W;
  const int Mc = a.Mc, V = a.V, F = a.F, Fs = a.Fs, nb = a.nb, it = a.it, wper = a.wper;
  const int Fl = F - Fs, n = Fs + V * Fl, U = V * nb;    // unknowns and virtual bands of a pixel
  const int nt = refine_ntri(n), P = nt + n;
  double* wl = reinterpret_cast<double*>(refine_views_smem);   // [jj][o] weights (0: skip the band)
  double* rl = wl + JT * WP;                             // [jj][o] obs, then r
  int* flag = reinterpret_cast<int*>(rl + JT * WP);      // [o] 0 idle, 1 accepted, 2 dead since this call, 3 rejected
  double* xl = rl + JT * WP + WP;                        // [a][o] accepted point
  double* dl = xl + n * WP;                              // [a][o] s_a h_a, then the solve's scratch
  double* tl = dl + n * WP;                              // [a][o] next trial / std
  double* Al = tl + n * WP;                              // [e][o] packed sums
  double* Ll = Al + P * WP;                              // [e][o] Cholesky factor
  double* Yl = Ll + nt * WP;                             // [(f JT + jj)][o]: the Y_f tile, J in place for f >= 1
  const double* cols = a.cols;
  const double* hi = a.cfg + REFINE_MAXF;
  const double* hh = a.cfg + 2 * REFINE_MAXF;
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * W;                         // first pixel of the group
  const int m = g0 + lane;                               // (lanes < W) this lane's pixel
  const bool mine = lane < W && m < Mc;
  const double* obs_g = a.obs + (int64_t)g0 * U;
  const double* wts_g = a.wts ? (wper ? a.wts + (int64_t)g0 * U : a.wts) : nullptr;
  const bool prior = a.ppw != nullptr;                   // (kernel-uniform)
  const int64_t pm = a.pper && mine ? (int64_t)m * n : 0;      // (lanes < W) where this lane's prior starts
  double* const st = a.st;
  double *const out_x = a.out.x, *const out_cost = a.out.cost;

  // the weight and observation tile of virtual bands j0 .. j0 + JT - 1: lanes run along the bands (out of range: weight 0)
  auto stage_obs = [&](int j0) {
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      const bool in = g0 + o < Mc && j < U;
      double w = 0.0, ob = 0.0;
      if (in) {
        w = wts_g ? wts_g[wper ? (int64_t)o * U + j : j % nb] : 1.0;
        ob = obs_g[(int64_t)o * U + j];
      }
      wl[jj * WP + o] = w;
      rl[jj * WP + o] = ob;
    }
  };

  // ---- pass 1: the trial cost from block 0, virtual bands ascending
  double ct = 0.0;
  bool bad = false;
  for (int j0 = 0; j0 < U; j0 += JT) {
    __syncthreads();
    stage_obs(j0);
    const double* y0 = cols + (int64_t)g0 * U;
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      Yl[jj * WP + o] = (g0 + o < Mc && j < U) ? y0[(int64_t)o * U + j] : 0.0;
    }
    __syncthreads();
    if (mine)
      for (int jj = 0; jj < JT; ++jj) {
        const double w = wl[jj * WP + lane];
        if (refine_bad_weight(w)) bad = true;
        if (w == 0.0) continue;
        ct = refine_cost_band(ct, w, Yl[jj * WP + lane], rl[jj * WP + lane]);
      }
  }
  if (prior && mine) {
    const double *pmu = LATE->pmu, *ppw = LATE->ppw;
    for (int u = 0; u < n; ++u) {
      const double p = ppw[pm + u];
      if (refine_bad_weight(p)) bad = true;
      if (p == 0.0) continue;
      ct = refine_prior_cost(ct, p, st[(int64_t)m * n + u], pmu[pm + u]);
    }
  }
  // ---- the decision
  int code = 0, na = 0;
  double lam = 0.0;
  if (mine) {
    double* const slam = LATE->slam;
    int32_t* const sna = LATE->sna;
    na = sna[m];
    lam = slam[m];
    if (it == 0) {
      code = (ct < __builtin_inf() && !bad) ? 1 : 2;
      if (double* cost0 = LATE->out.cost0) cost0[m] = ct;
      if (code == 2) {
        na = -1;
        out_cost[m] = ct;
        if (int32_t* n_accept = LATE->out.n_accept) n_accept[m] = -1;
        if (double* sdev = LATE->out.sdev)
          for (int u = 0; u < n; ++u) sdev[(int64_t)m * n + u] = __builtin_nan("");
      }
    } else if (na >= 0) {
      code = ct < out_cost[m] ? 1 : 3;
      lam = refine_lambda(lam, code == 1);
      if (code == 1) ++na;
    }
    if (code == 1) out_cost[m] = ct;
    if (code != 0) {
      slam[m] = lam;
      sna[m] = na;
    }
    for (int u = 0; u < n; ++u) {
      const double tu = st[(int64_t)m * n + u];
      double xu = tu;
      if (code == 1) out_x[(int64_t)m * n + u] = tu;
      else xu = out_x[(int64_t)m * n + u];
      xl[u * WP + lane] = xu;
      dl[u * WP + lane] = refine_fd_step(tu, hh[u], hi[u]);
    }
  }
  if (lane < W) flag[lane] = code;
  const bool fresh = __builtin_amdgcn_ballot_w64(code == 1 || code == 2) != 0;     // (wave-uniform)
  __syncthreads();

  // ---- pass 2: y, r, J and the sums of the pixels that moved
  if (fresh) {
    for (int i = lane; i < P * W; i += 64) Al[(i / W) * WP + i % W] = 0.0;
    for (int j0 = 0; j0 < U; j0 += JT) {
      __syncthreads();
      stage_obs(j0);
      for (int i = lane; i < (F + 1) * W * JT; i += 64) {
        const int jj = i % JT, o = (i / JT) % W, f = i / (JT * W), j = j0 + jj;
        const int fl = flag[o];
        const bool in = g0 + o < Mc && j < U && (fl == 1 || (fl == 2 && f == 0));
        const double* yf = cols + ((int64_t)f * Mc + g0) * U;
        Yl[(f * JT + jj) * WP + o] = in ? yf[(int64_t)o * U + j] : 0.0;
      }
      __syncthreads();
      // r_u (block 0's lanes) and J (the others): block f at virtual band u is the column of views_unknown(u / nb, f - 1)
      double* y_g = LATE->out.y;
      if (y_g) y_g += (int64_t)g0 * U;
      for (int i = lane; i < (F + 1) * W * JT; i += 64) {
        const int jj = i % JT, o = (i / JT) % W, f = i / (JT * W), j = j0 + jj;
        const int fl = flag[o];
        if (!(g0 + o < Mc && j < U) || (fl != 1 && fl != 2)) continue;
        const double y0 = Yl[jj * WP + o];
        if (f == 0) {
          if (y_g) y_g[(int64_t)o * U + j] = y0;
          if (wl[jj * WP + o] != 0.0) rl[jj * WP + o] = refine_residual(y0, rl[jj * WP + o]);
        } else if (fl == 1) {
          const int u = views_unknown(j / nb, f - 1, Fs, Fl);
          Yl[(f * JT + jj) * WP + o] = refine_jacobian(Yl[(f * JT + jj) * WP + o], y0, dl[u * WP + o]);
        }
      }
      __syncthreads();
      {
        const int o = lane % W, q = lane / W;
        if (flag[o] == 1) {
          const int jn = U - j0 < JT ? U - j0 : JT;
          for (int e = q; e < P; e += G) {
            int ua = 0, ub = -1;                           // e < nt: A_ab of unknowns ua >= ub; else g_a against r
            if (e < nt) {
              while ((ua + 1) * (ua + 2) / 2 <= e) ++ua;
              ub = e - ua * (ua + 1) / 2;
            } else {
              ua = e - nt;
            }
            // the bands of this tile where the entry exists: both unknowns active
            int jb = 0, je = jn;
            views_clip_range(views_view(ua, Fs, Fl), nb, j0, &jb, &je);
            if (ub >= 0) views_clip_range(views_view(ub, Fs, Fl), nb, j0, &jb, &je);
            const double* ja = Yl + ((views_name(ua, Fs, Fl) + 1) * JT) * WP + o;
            const double* jc = ub >= 0 ? Yl + ((views_name(ub, Fs, Fl) + 1) * JT) * WP + o : rl + o;
            double acc = Al[e * WP + o];
            for (int jj = jb; jj < je; ++jj) {
              const double w = wl[jj * WP + o];
              if (w == 0.0) continue;
              acc = refine_mac(acc, w, ja[jj * WP], jc[jj * WP]);
            }
            Al[e * WP + o] = acc;
          }
        }
      }
    }
    __syncthreads();
    if (prior) {
      if (mine && code == 1) {
        const double *pmu = LATE->pmu, *ppw = LATE->ppw;
        for (int u = 0; u < n; ++u) {
          const double p = ppw[pm + u];
          if (p == 0.0) continue;
          double* Aaa = Al + refine_tri(u, u) * WP + lane;
          double* ga = Al + (nt + u) * WP + lane;
          *Aaa = *Aaa + p;
          *ga = refine_prior_gain(*ga, p, refine_residual(xl[u * WP + lane], pmu[pm + u]));
        }
      }
      __syncthreads();
    }
  }
  // accepted: the new sums become the state; rejected: the state's sums come back
  {
    double* sA_g = LATE->sA + (int64_t)g0 * P;
    for (int i = lane; i < P * W; i += 64) {
      const int e = i % P, o = i / P;
      if (g0 + o >= Mc) continue;
      const int fl = flag[o];
      if (fl == 1) sA_g[i] = Al[e * WP + o];
      else if (fl == 3) Al[e * WP + o] = sA_g[i];
    }
  }
  __syncthreads();

  // ---- finish: the next trial and its table rows, or the outputs of the last call
  if (mine && (code == 1 || code == 3)) {
    if (!LATE->last) {
      const double* lo = LATE->cfg;
      refine_propose(n, Al + lane, WP, lam, xl + lane, WP, lo, lo + REFINE_MAXF, Ll + lane, WP, dl + lane, WP, tl + lane, WP);
      const int32_t* cfg_free = LATE->cfg_free;
      const int64_t blk = (int64_t)Mc * V, R = (int64_t)(F + 1) * blk;
      double* const table_m = LATE->table + (int64_t)m * V;
      for (int u = 0; u < n; ++u) {
        const double tu = tl[u * WP + lane];
        const double moved = tu + refine_fd_step(tu, hh[u], hi[u]);
        st[(int64_t)m * n + u] = tu;
        const int f = views_name(u, Fs, Fl), vu = views_view(u, Fs, Fl);
        const int v0 = vu < 0 ? 0 : vu, v1 = vu < 0 ? V : vu + 1;     // a shared value goes into every view's rows
        double* row = table_m + cfg_free[f] * R;
        for (int v = v0; v < v1; ++v)
          for (int fp = 0; fp <= F; ++fp) row[(int64_t)fp * blk + v] = fp == f + 1 ? moved : tu;
      }
    } else {
      if (int32_t* n_accept = LATE->out.n_accept) n_accept[m] = na;
      if (double* sdev = LATE->out.sdev) {
        refine_std(n, Al + lane, WP, Ll + lane, WP, dl + lane, WP, tl + lane, WP);
        for (int u = 0; u < n; ++u) sdev[(int64_t)m * n + u] = tl[u * WP + lane];
      }
    }
  }
}
#endif  // __HIPCC__

}  // namespace spart
