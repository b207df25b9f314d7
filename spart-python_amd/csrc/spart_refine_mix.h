// A linear mixture of V canopies per pixel (spart_refine_mix, include/spart_hip.h; the definition is
// tools/refine_mix_defined.py and every function here reproduces it bit for bit): spart_refine's fit of ONE observed column
// per pixel with y_j = sum_v a_v Y_v[j], the fractions a_v given or fitted on the simplex.  The per-entry arithmetic is
// csrc/spart_refine.h's part 1, called with n where it says F; the forward table and its row order are spart_refine_views';
// no kernel of either header is touched.
//
// Part 1: the unknown maps, the fractions and the two new per-entry products, SPART_HD so that g++ compiles them for
// tests/hostmath/refine_mix_host.cpp.
// Index conventions.  free_cols lists the F = Fs + Fl free columns by NAME, the shared ones first; bounds and steps belong to a
// name.  The unknowns are, in this order: the Fs shared names; the ACTIVE locals, component v ascending and within a component l
// ascending (an inactive local stays at its component's base value and is no unknown); with fitted fractions q_0 ... q_{V-2}.
// nm counts the model unknowns, n = nm + (V - 1 if the fractions are fitted else 0).
#pragma once

#include "spart_refine_views.h"

namespace spart {

constexpr int MIX_MAXV = 8;                  // components per pixel
constexpr int MIX_SHARED = 0, MIX_LOCAL = 1, MIX_FRACTION = 2;

// The maps, one small table: name[a] the index into free_cols of model unknown a, comp[a] its component (-1: shared; for a
// fraction unknown name is -1 and comp is the v of q_v), unk[v][f] the unknown that free column f takes its value from in
// component v (-1: that local is inactive there).
struct MixMap {
  int8_t name[REFINE_MAXF], comp[REFINE_MAXF];
  int8_t unk[MIX_MAXV][REFINE_MAXF];
  int32_t nm, n;
};

// Builds the maps from the (V, Fl) activity mask (row-major 0 / 1; NULL: all active).  -> n, or -1 for a local name that is
// active in no component, or -2 for more than REFINE_MAXF unknowns (the table is then not complete)
SPART_HD int mix_build_map(int V, int Fs, int Fl, const int32_t* active, int fit_fractions, MixMap* m) {
  for (int a = 0; a < REFINE_MAXF; ++a) m->name[a] = m->comp[a] = -1;
  for (int v = 0; v < MIX_MAXV; ++v)
    for (int f = 0; f < REFINE_MAXF; ++f) m->unk[v][f] = -1;
  m->nm = m->n = 0;
  for (int l = 0; l < Fl; ++l) {
    bool any = false;
    for (int v = 0; v < V; ++v) any = any || !active || active[v * Fl + l] != 0;
    if (!any) return -1;
  }
  int n = 0;
  for (int f = 0; f < Fs; ++f, ++n) {
    if (n >= REFINE_MAXF) return -2;
    m->name[n] = (int8_t)f;
    for (int v = 0; v < V; ++v) m->unk[v][f] = (int8_t)n;
  }
  for (int v = 0; v < V; ++v)
    for (int l = 0; l < Fl; ++l) {
      if (active && active[v * Fl + l] == 0) continue;
      if (n >= REFINE_MAXF) return -2;
      m->name[n] = (int8_t)(Fs + l);
      m->comp[n] = (int8_t)v;
      m->unk[v][Fs + l] = (int8_t)n;
      ++n;
    }
  m->nm = n;
  if (fit_fractions)
    for (int v = 0; v < V - 1; ++v, ++n) {
      if (n >= REFINE_MAXF) return -2;
      m->comp[n] = (int8_t)v;
    }
  m->n = n;
  return n;
}

SPART_HD int mix_kind(int a, int Fs, int nm) { return a < Fs ? MIX_SHARED : a < nm ? MIX_LOCAL : MIX_FRACTION; }

// The fractions of a trial.  Fitted (q: the V - 1 fraction unknowns): s = 0; for v < V - 1 ascending a_v = q_v, s = s + a_v;
// a_{V-1} = 1 - s; -> FEASIBLE iff a_{V-1} >= 0 (a NaN is not).  a at stride S.
SPART_HD bool mix_fractions(int V, const double* q, int SQ, double* a, int S) {
  SPART_NO_CONTRACT
  double s = 0.0;
  for (int v = 0; v < V - 1; ++v) {
    const double av = q[v * SQ];
    a[v * S] = av;
    s = s + av;
  }
  const double last = 1.0 - s;
  a[(V - 1) * S] = last;
  return last >= 0.0;
}

// one term of the mixed column: a_0 Y for the first component, y + a_v Y after it
SPART_HD double mix_add(double y, double a, double Y, bool first) {
  SPART_NO_CONTRACT
  const double p = a * Y;
  return first ? p : y + p;
}

// one component's term of a model unknown's Jacobian entry: a_v ((Y_(v,f+1) - Y_(v,0)) / (s h)), alone for a local unknown and
// for v = 0 of a shared one, added to acc after it
SPART_HD double mix_jac_term(double acc, double a, double yf, double y0, double sh, bool first) {
  SPART_NO_CONTRACT
  const double p = a * refine_jacobian(yf, y0, sh);
  return first ? p : acc + p;
}

// the Jacobian entry of the fraction q_v: Y_(v,0) - Y_(V-1,0)
SPART_HD double mix_jac_fraction(double yv, double ylast) {
  SPART_NO_CONTRACT
  return yv - ylast;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: the kernels.  One chunk of Mc pixels owns what a chunk of spart_refine_views owns: the table (27, (F + 1) Mc V),
// row = (f Mc + m) V + v, and cols ((F + 1) Mc V, nb) in that row order, so that the family's chunk loop and forward call serve
// unchanged; block f of pixel m is one run of V nb doubles, component v at offset v nb.  state: t (Mc, n), A (Mc, ntri(n) + n),
// lam, na (Mc).  The fractions are entries nm ... n - 1 of t and x and touch no table entry.
// k_refine_mix_step is k_refine_step over the nb bands of the MIXED column: the same single-wave groups of W pixels, 16-band
// LDS tiles, [k][o] rows at stride W + 1, the same three phases and per-entry order.  What differs: a tile of y and of the n
// Jacobian columns is FOLDED from the pixel's (F + 1) V blocks, components ascending, every element by the one lane that owns it
// (lanes run along the bands, so a wave reads runs of 16 doubles); the n columns are dense over the bands, so the packed sums
// are k_refine_step's; an infeasible trial's cost becomes +inf between the cost and the decision; a new trial writes V (F + 1)
// table entries per shared unknown, F + 1 per active local and none for a fraction; frac and y_comp are outputs.

// LDS is refine_lds_rows(n, n, MIX_MAXV): the n Jacobian tiles (the first is the y tile of pass 1) and, of the kernel's own,
// the MIX_MAXV fractions; W follows refine_group.

// The arguments of k_refine_mix_init, ONE struct: the maps are indexed by run-time values, which the kernel does through the
// kernarg segment (LATE below) so that no copy of the struct is indexed in registers.  cfg: spart_refine's RefineCfg with every
// base column (V, M) component-major and lo / hi / h per name; frac: the caller's (M, V).
struct MixInit {
  RefineCfg cfg;
  MixMap map;
  int64_t M, m0;
  int32_t Mc, V, F, Fs, fit;
  double lambda0, frac_lo, frac_hi;
  const double* frac;
  double *table, *x, *t, *lam;
  int32_t* na;
  double* dcfg;
  int32_t* dcfg_free;
};

// Once per chunk (pixels m0 .. m0 + Mc - 1 of the call's M), one thread per table row of a block: i = m V + v.  The device
// copy `dcfg` gets lo, hi, h per UNKNOWN (a fraction: its box and h = 0).  A shared unknown starts from component 0's entry; an
// inactive local keeps its component's base value, unclipped, in every block.  x / t are the chunk's own rows.
__global__ __launch_bounds__(256) void k_refine_mix_init(MixInit a) {
  SPART_NO_CONTRACT
#if defined(__HIP_DEVICE_COMPILE__)
  const __attribute__((address_space(4))) MixInit* LATE =
      (const __attribute__((address_space(4))) MixInit*)__builtin_amdgcn_kernarg_segment_ptr();
#else
  const MixInit* LATE = &a;                              // (the host pass only parses the kernel)
#endif
  const int Mc = a.Mc, V = a.V, F = a.F, Fs = a.Fs;
  const int nm = a.map.nm, n = a.map.n;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && (int)threadIdx.x < REFINE_MAXF) {
    const int u = threadIdx.x, fn = u < nm ? (int)LATE->map.name[u] : -1;
#pragma unroll
    for (int f = 0; f < REFINE_MAXF; ++f) {
      if (f == fn) {
        a.dcfg[u] = a.cfg.lo[f];
        a.dcfg[REFINE_MAXF + u] = a.cfg.hi[f];
        a.dcfg[2 * REFINE_MAXF + u] = a.cfg.h[f];
      }
      if (f == u) a.dcfg_free[u] = a.cfg.free_col[f];
    }
    if (u >= nm && u < n) {
      a.dcfg[u] = a.frac_lo;
      a.dcfg[REFINE_MAXF + u] = a.frac_hi;
      a.dcfg[2 * REFINE_MAXF + u] = 0.0;
    }
  }
  if (i >= Mc * V) return;
  const int m = i / V, v = i % V;
  const int64_t blk = (int64_t)Mc * V, R = (int64_t)(F + 1) * blk;
  const int64_t src = (int64_t)v * a.M + a.m0 + m;
#pragma unroll
  for (int p = 0; p < NPARAM; ++p) {
    if (a.cfg.is_free[p]) continue;
    const double val = a.cfg.base[p][src];
    double* row = a.table + p * R + i;
    for (int fp = 0; fp <= F; ++fp) row[(int64_t)fp * blk] = val;
  }
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    const int u = LATE->map.unk[v][f];
    double* row = a.table + a.cfg.free_col[f] * R + i;
    if (u < 0) {                                         // inactive here: the base value in every block
      const double val = a.cfg.freebase[f][src];
      for (int fp = 0; fp <= F; ++fp) row[(int64_t)fp * blk] = val;
      continue;
    }
    const double tf = refine_clip(a.cfg.freebase[f][f < Fs ? a.m0 + m : src], a.cfg.lo[f], a.cfg.hi[f]);
    const double moved = tf + refine_fd_step(tf, a.cfg.h[f], a.cfg.hi[f]);
    if (f >= Fs || v == 0) {
      a.x[(int64_t)m * n + u] = tf;
      a.t[(int64_t)m * n + u] = tf;
    }
    for (int fp = 0; fp <= F; ++fp) row[(int64_t)fp * blk] = fp == f + 1 ? moved : tf;
  }
  if (a.fit && v < V - 1) {
    const double q = refine_clip(a.frac[(a.m0 + m) * V + v], a.frac_lo, a.frac_hi);
    a.x[(int64_t)m * n + nm + v] = q;
    a.t[(int64_t)m * n + nm + v] = q;
  }
  if (v == 0) {
    a.lam[m] = a.lambda0;
    a.na[m] = 0;
  }
}

// outputs of the call, already moved to the chunk's first pixel; cost0 / sdev / n_accept / y / frac / y_comp may be NULL
struct MixOut {
  double *x, *cost, *cost0, *sdev;
  int32_t* n_accept;
  double *y, *frac, *y_comp;
};

// The arguments of k_refine_mix_step, ONE struct read late from the kernarg segment where a member is needed (LATE below), as
// ViewsStep is: the argument list plus the maps needs more scalar registers than a wave has.  obs / wts are the chunk's rows
// ((Mc, nb); wts NULL, or (nb,) with wper == 0, or the chunk's rows with wper == 1); frac: the chunk's rows of the caller's
// (M, V), read only when the fractions are given (fit == 0); pmu / ppw: both NULL, or the prior's mean and weight, (n,) with
// pper == 0 or the chunk's rows of (M, n) with pper == 1.  cfg: lo, hi, h per unknown.  it: the iteration; last: it == n_iter.
struct MixStep {
  const double *cols, *obs, *wts, *cfg, *frac;
  const int32_t* cfg_free;
  double* table;
  int32_t Mc, V, F, Fs, nb, it, last, wper, pper, fit;
  double *st, *sA, *slam;
  int32_t* sna;
  MixOut out;
  const double *pmu, *ppw;
  MixMap map;
};

// Once per iteration.  W (4 or 8: refine_group) is a template parameter: the strides and the lane maps are constants.
// The phases are written out here and in k_refine_mix_init, not called from spart_refine.h as the rest of the family calls
// them: over those functions the two kernels had fewer instructions, and the whole call at V = 4, n = 16 measured 1.5 % slower,
// outside the run-to-run spread (profiles/refine_phases_ab.txt).  A change to a phase there is made here as well.
template <int W>
__global__ __launch_bounds__(64) void k_refine_mix_step(MixStep a) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char refine_mix_smem[];
  // (the struct is the only argument, so the kernarg segment starts with it)
#if defined(__HIP_DEVICE_COMPILE__)
  const __attribute__((address_space(4))) MixStep* LATE =
      (const __attribute__((address_space(4))) MixStep*)__builtin_amdgcn_kernarg_segment_ptr();
#else
  const MixStep* LATE = &a;                              // (the host pass only parses the kernel)
#endif
  constexpr int JT = REFINE_JT, WP = W + 1, G = 64 / W;
  const int Mc = a.Mc, V = a.V, nb = a.nb, wper = a.wper;
  const int nm = a.map.nm, n = a.map.n;
  const int nt = refine_ntri(n), P = nt + n;
  double* wl = reinterpret_cast<double*>(refine_mix_smem);     // [jj][o] weights (0: skip the band)
  double* rl = wl + JT * WP;                             // [jj][o] obs, then r
  int* flag = reinterpret_cast<int*>(rl + JT * WP);      // [o] 0 idle, 1 accepted, 2 dead since this call, 3 rejected
  double* fl = rl + JT * WP + WP;                        // [v][o] the trial's fractions
  double* xl = fl + MIX_MAXV * WP;                       // [a][o] accepted point
  double* dl = xl + n * WP;                              // [a][o] s_a h_a, then the solve's scratch
  double* tl = dl + n * WP;                              // [a][o] next trial / std
  double* Al = tl + n * WP;                              // [e][o] packed sums
  double* Ll = Al + P * WP;                              // [e][o] Cholesky factor
  double* Jl = Ll + nt * WP;                             // [(a JT + jj)][o]: the J tile; rows 0 .. JT - 1 hold y in pass 1
  const double* cols = a.cols;
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * W;                         // first pixel of the group
  const int m = g0 + lane;                               // (lanes < W) this lane's pixel
  const bool mine = lane < W && m < Mc;
  const int64_t U = (int64_t)V * nb;                     // doubles of one block of a pixel
  const int64_t BS = (int64_t)Mc * U;                    // doubles from block f to block f + 1
  const double* obs_g = a.obs + (int64_t)g0 * nb;
  const double* wts_g = a.wts ? (wper ? a.wts + (int64_t)g0 * nb : a.wts) : nullptr;
  const bool prior = a.ppw != nullptr;                   // (kernel-uniform)
  const int64_t pm = a.pper && mine ? (int64_t)m * n : 0;      // (lanes < W) where this lane's prior starts
  double* const st = a.st;

  // the weight and observation tile of bands j0 .. j0 + JT - 1: lanes run along the bands (out of range: weight 0)
  auto stage_obs = [&](int j0) {
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      const bool in = g0 + o < Mc && j < nb;
      double w = 0.0, ob = 0.0;
      if (in) {
        w = wts_g ? wts_g[wper ? (int64_t)o * nb + j : j] : 1.0;
        ob = obs_g[(int64_t)o * nb + j];
      }
      wl[jj * WP + o] = w;
      rl[jj * WP + o] = ob;
    }
  };

  // ---- the trial's fractions (lane o < W): fitted from t on the simplex, or the caller's as they are
  bool bad = false, feasible = true;
  if (mine) {
    if (a.fit) {
      feasible = mix_fractions(V, st + (int64_t)m * n + nm, 1, fl + lane, WP);
    } else {
      const double* fr = LATE->frac + (int64_t)m * V;
      for (int v = 0; v < V; ++v) {
        const double av = fr[v];
        if (refine_bad_weight(av)) bad = true;
        fl[v * WP + lane] = av;
      }
    }
  }
  // ---- pass 1: the mixed column of block 0 and the trial cost, bands ascending
  double ct = 0.0;
  for (int j0 = 0; j0 < nb; j0 += JT) {
    __syncthreads();
    stage_obs(j0);
    for (int i = lane; i < W * JT; i += 64) {
      const int jj = i % JT, o = i / JT, j = j0 + jj;
      double y = 0.0;
      if (g0 + o < Mc && j < nb) {
        const double* Y0 = cols + (int64_t)(g0 + o) * U + j;
        for (int v = 0; v < V; ++v) y = mix_add(y, fl[v * WP + o], Y0[(int64_t)v * nb], v == 0);
      }
      Jl[jj * WP + o] = y;
    }
    __syncthreads();
    if (mine)
      for (int jj = 0; jj < JT; ++jj) {
        const double w = wl[jj * WP + lane];
        if (refine_bad_weight(w)) bad = true;
        if (w == 0.0) continue;
        ct = refine_cost_band(ct, w, Jl[jj * WP + lane], rl[jj * WP + lane]);
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
  if (!feasible) ct = __builtin_inf();                   // the simplex rule: rejected, or a dead start
  // ---- the decision
  int code = 0, na = 0;
  double lam = 0.0;
  if (mine) {
    double* const slam = LATE->slam;
    int32_t* const sna = LATE->sna;
    double *const out_x = LATE->out.x, *const out_cost = LATE->out.cost;
    const double* hi = LATE->cfg + REFINE_MAXF;
    const double* hh = LATE->cfg + 2 * REFINE_MAXF;
    na = sna[m];
    lam = slam[m];
    if (LATE->it == 0) {
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
    if (code == 1 || code == 2)
      if (double* frac = LATE->out.frac)
        for (int v = 0; v < V; ++v) frac[(int64_t)m * V + v] = fl[v * WP + lane];
  }
  if (lane < W) flag[lane] = code;
  const bool fresh = __builtin_amdgcn_ballot_w64(code == 1 || code == 2) != 0;     // (wave-uniform)
  __syncthreads();

  // ---- pass 2: y, y_comp, r, J and the sums of the pixels that moved
  if (fresh) {
    for (int i = lane; i < P * W; i += 64) Al[(i / W) * WP + i % W] = 0.0;
    for (int j0 = 0; j0 < nb; j0 += JT) {
      __syncthreads();
      stage_obs(j0);
      __syncthreads();
      // row 0: the mixed column, the outputs and r_j; row 1 + u: J of unknown u.  Every element folds its components in
      // ascending order on the one lane that owns it
      double* y_g = LATE->out.y;
      double* yc_g = LATE->out.y_comp;
      for (int i = lane; i < (n + 1) * W * JT; i += 64) {
        const int jj = i % JT, o = (i / JT) % W, row = i / (JT * W), j = j0 + jj;
        const int fg = flag[o];
        if (!(g0 + o < Mc && j < nb) || (fg != 1 && fg != 2)) continue;
        const double* Y0 = cols + (int64_t)(g0 + o) * U + j;                       // Y_(v,f) at Y0[f BS + v nb]
        if (row == 0) {
          double y = 0.0;
          for (int v = 0; v < V; ++v) {
            const double yv = Y0[(int64_t)v * nb];
            y = mix_add(y, fl[v * WP + o], yv, v == 0);
            if (yc_g) yc_g[((int64_t)(g0 + o) * V + v) * nb + j] = yv;
          }
          if (y_g) y_g[(int64_t)(g0 + o) * nb + j] = y;
          if (wl[jj * WP + o] != 0.0) rl[jj * WP + o] = refine_residual(y, rl[jj * WP + o]);
        } else if (fg == 1) {
          const int u = row - 1;
          const int vu = LATE->map.comp[u];
          double acc = 0.0;
          if (u >= nm) {
            acc = mix_jac_fraction(Y0[(int64_t)vu * nb], Y0[(int64_t)(V - 1) * nb]);
          } else {
            const double* Yf = Y0 + (int64_t)(LATE->map.name[u] + 1) * BS;
            const double sh = dl[u * WP + o];
            const int v0 = vu < 0 ? 0 : vu, v1 = vu < 0 ? V : vu + 1;
            for (int v = v0; v < v1; ++v)
              acc = mix_jac_term(acc, fl[v * WP + o], Yf[(int64_t)v * nb], Y0[(int64_t)v * nb], sh, v == v0);
          }
          Jl[(u * JT + jj) * WP + o] = acc;
        }
      }
      __syncthreads();
      {
        const int o = lane % W, q = lane / W;
        if (flag[o] == 1) {
          const int jn = nb - j0 < JT ? nb - j0 : JT;
          for (int e = q; e < P; e += G) {
            int ua = 0, ub = -1;                           // e < nt: A_ab of unknowns ua >= ub; else g_a against r
            if (e < nt) {
              while ((ua + 1) * (ua + 2) / 2 <= e) ++ua;
              ub = e - ua * (ua + 1) / 2;
            } else {
              ua = e - nt;
            }
            const double* ja = Jl + (ua * JT) * WP + o;
            const double* jc = ub >= 0 ? Jl + (ub * JT) * WP + o : rl + o;
            double acc = Al[e * WP + o];
            for (int jj = 0; jj < jn; ++jj) {
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
      const int fg = flag[o];
      if (fg == 1) sA_g[i] = Al[e * WP + o];
      else if (fg == 3) Al[e * WP + o] = sA_g[i];
    }
  }
  __syncthreads();

  // ---- finish: the next trial and its table rows, or the outputs of the last call
  if (mine && (code == 1 || code == 3)) {
    if (!LATE->last) {
      const double* lo = LATE->cfg;
      const double* hi = lo + REFINE_MAXF;
      const double* hh = lo + 2 * REFINE_MAXF;
      refine_propose(n, Al + lane, WP, lam, xl + lane, WP, lo, hi, Ll + lane, WP, dl + lane, WP, tl + lane, WP);
      const int32_t* cfg_free = LATE->cfg_free;
      const int F = LATE->F;
      const int64_t blk = (int64_t)Mc * V, R = (int64_t)(F + 1) * blk;
      double* const table_m = LATE->table + (int64_t)m * V;
      for (int u = 0; u < n; ++u) {
        const double tu = tl[u * WP + lane];
        st[(int64_t)m * n + u] = tu;
        if (u >= nm) continue;                             // a fraction touches no table entry
        const double moved = tu + refine_fd_step(tu, hh[u], hi[u]);
        const int f = LATE->map.name[u], vu = LATE->map.comp[u];
        const int v0 = vu < 0 ? 0 : vu, v1 = vu < 0 ? V : vu + 1;     // a shared value goes into every component's rows
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
