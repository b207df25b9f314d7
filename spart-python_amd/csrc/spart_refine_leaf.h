// PROSPECT inversion of leaf spectra: bounded Levenberg-Marquardt fits of a few of the nine leaf parameters against measured
// reflectance and / or transmittance on the 2001-band grid (spart_refine_leaf, include/spart_hip.h; the definition is
// tools/refine_leaf_defined.py and part 1 reproduces it bit for bit given the same forward model).
//
// The fit is spart_refine's (csrc/spart_refine.h: accept rule, lambda, damped solve, bounds, std) with the leaf model as its
// forward model and the band sums written as 64 lane partials plus one fixed join, so that a wave can run along the bands.
//
// Part 1: the per-leaf arithmetic as plain functions, compiled by hipcc into k_refine_leaf and by g++ into
// tests/hostmath/refine_leaf_host.cpp, which runs the 64 lanes as a loop.
// Part 2: k_refine_leaf<F>, one wave per leaf, the whole fit in one launch, no spectra in memory and no workspace.
#pragma once

#include "spart_math.h"
#include "spart_refine.h"
#if defined(__HIPCC__)
#include "spart_kernels.h"   // load_tab
#endif

namespace spart {

constexpr int LEAF_NPAR = 9;                 // parameters of a leaf, spart_prospect_batch's order
constexpr int LEAF_MAXF = 9;                 // free parameters per call
constexpr int LEAF_NC = 9;                   // leaf constants of a row: C_CAB ... C_NM1, leaf_band's argument order
constexpr int LEAF_LANES = 64;               // partials per band sum
constexpr int LEAF_PASSES = (NWL + LEAF_LANES - 1) / LEAF_LANES;      // 32 passes over the bands; the last has 17 live lanes
static_assert(C_CAB == 0 && C_NM1 == LEAF_NC - 1, "a row's constants are ConstIdx 0 ... 8");
static_assert(LEAF_MAXF <= REFINE_MAXF, "the phases of spart_refine.h serve");

// ------------------------------------------------------------------------------------------------------------------------
// Part 1

// The leaf constants of one row of nine parameters, formed by the prelude's PRE_LEAF part itself
struct LeafRowIn {
  const double* p;
  SPART_HD double operator()(int i) const { return p[i]; }
};
struct LeafRowOut {
  double* lc;
  SPART_HD void c(int i, double v) {
    if (i < LEAF_NC) lc[i] = v;
  }
  SPART_HD void a(int, double) {}
  SPART_HD void l(int, double) {}
};
SPART_HD void leaf_row_constants(const double* p9, double* lc) {
  LeafRowOut out = {lc};
  sample_prelude_to<false>(LeafRowIn{p9}, 0.0, 0.0, PRE_LEAF, out);
}

// (refl, tran) of one band of one row
SPART_HD void leaf_row_band(const BandTab<double>& tb, const double* lc, double& refl, double& tran) {
  double absb, K;
  leaf_band<double>(tb, lc[0], lc[1], lc[2], lc[3], lc[4], lc[5], lc[6], lc[7], lc[8], refl, tran, absb, K);
}

// What one lane carries through a sweep: its partial of the trial cost, of the F (F + 1) / 2 sums of A and of the F sums of g
// (refine_tri's packed order), and whether it met a weight that kills the leaf
template <int F> struct LeafPartial {
  static constexpr int NT = F * (F + 1) / 2, P = NT + F;
  double c;
  double s[P];
  int bad;
};

template <int F> SPART_HD void leaf_partial_zero(LeafPartial<F>& a) {
  a.c = 0.0;
#pragma unroll
  for (int e = 0; e < LeafPartial<F>::P; ++e) a.s[e] = 0.0;
  a.bad = 0;
}

// The terms of one observation array at one band: A_ab + (w J_a) J_b for a >= b, g_a + (w J_a) r
template <int F> SPART_HD void leaf_partial_terms(LeafPartial<F>& a, bool use, double w, const double* J, int SJ, double r) {
  constexpr int NT = LeafPartial<F>::NT;
  if (!use) return;
  double j[F];
#pragma unroll
  for (int f = 0; f < F; ++f) j[f] = J[f * SJ];
#pragma unroll
  for (int p = 0; p < F; ++p) {
#pragma unroll
    for (int q = 0; q <= p; ++q) a.s[p * (p + 1) / 2 + q] = refine_mac(a.s[p * (p + 1) / 2 + q], w, j[p], j[q]);
    a.s[NT + p] = refine_mac(a.s[NT + p], w, j[p], r);
  }
}

// One band of one lane.  lc: the F + 1 rows' constants (row f at lc + f LEAF_NC; row 0 is the trial, row f >= 1 has free
// parameter f - 1 moved by sh[f - 1]).  has_r / has_t: the observation array is given; w: its weight at this band (1 without a
// weights array).  Per sum the reflectance term comes first, then the transmittance term; a term whose array is absent or
// whose weight is 0 is skipped (the observation may be NaN there).  tab_at(): the band's BandTab, asked for once per row, so
// that the kernel may load it again instead of holding its 22 registers through the leaf model (F = 9 has none to spare).  J: 2 F doubles of the lane's own, element k at J[k SJ].
template <int F, typename Tab>
SPART_HD void leaf_partial_band(LeafPartial<F>& a, Tab&& tab_at, const double* lc, const double* sh, bool has_r,
                                double wr, double obr, bool has_t, double wt, double obt, double* J, int SJ) {
  SPART_NO_CONTRACT
  if (has_r && refine_bad_weight(wr)) a.bad = 1;
  if (has_t && refine_bad_weight(wt)) a.bad = 1;
  const bool ur = has_r && wr != 0.0, ut = has_t && wt != 0.0;
  if (!(ur || ut)) return;
  double y0r, y0t;
  leaf_row_band(tab_at(), lc, y0r, y0t);
  if (ur) a.c = refine_cost_band(a.c, wr, y0r, obr);
  if (ut) a.c = refine_cost_band(a.c, wt, y0t, obt);
  // the rows one after the other (NOT unrolled: one copy of the leaf model, and its temporaries die before the sums)
#pragma unroll 1
  for (int f = 0; f < F; ++f) {
    double yr, yt;
    leaf_row_band(tab_at(), lc + (f + 1) * LEAF_NC, yr, yt);
    J[f * SJ] = refine_jacobian(yr, y0r, sh[f]);
    J[(F + f) * SJ] = refine_jacobian(yt, y0t, sh[f]);
  }
  // every sum takes its reflectance term, then its transmittance term: all the first ones, then all the second ones
  leaf_partial_terms<F>(a, ur, wr, J, SJ, refine_residual(y0r, obr));
  leaf_partial_terms<F>(a, ut, wt, J + F * SJ, SJ, refine_residual(y0t, obt));
}

// the join's one operation: p_l = p_l + p_(l + d)
SPART_HD double leaf_join_add(double mine, double peer) {
  SPART_NO_CONTRACT
  return mine + peer;
}

// The join over LEAF_LANES partials held as an array (the host's form; the kernel does the same tree with cross-lane moves):
// for d = 32, 16, ... 1: p_l = p_l + p_(l + d) for l < d.  The sums end in p[0].
template <int F> inline void leaf_join_lanes(LeafPartial<F>* p) {
  for (int d = LEAF_LANES / 2; d >= 1; d >>= 1)
    for (int l = 0; l < d; ++l) {
      p[l].c = leaf_join_add(p[l].c, p[l + d].c);
      for (int e = 0; e < LeafPartial<F>::P; ++e) p[l].s[e] = leaf_join_add(p[l].s[e], p[l + d].s[e]);
      p[l].bad |= p[l + d].bad;
    }
}

// ---- the per-leaf state machine.  Every array is dense; on the device they are the wave's LDS rows and one lane runs these.
struct LeafFit {
  double lam, cost, cost0;
  int na;                                    // accepted steps, -1: dead
};

// x = t = the clipped start
SPART_HD void leaf_fit_start(int F, const double* base9, const int32_t* free_cols, const double* lo, const double* hi, double lambda0,
                             double* x, double* t, LeafFit* s) {
  for (int f = 0; f < F; ++f) x[f] = t[f] = refine_clip(base9[free_cols[f]], lo[f], hi[f]);
  s->lam = lambda0;
  s->cost = __builtin_inf();
  s->cost0 = __builtin_nan("");
  s->na = 0;
}

// s_f h_f of the trial t
SPART_HD void leaf_fit_steps(int F, const double* t, const double* h, const double* hi, double* sh) {
  for (int f = 0; f < F; ++f) sh[f] = refine_fd_step(t[f], h[f], hi[f]);
}

// row f of an evaluation: p_0 = the leaf with its free parameters at t; p_f = p_0 with free parameter f - 1 moved by sh[f - 1]
SPART_HD void leaf_fit_row(int F, int f, const double* base9, const int32_t* free_cols, const double* t, const double* sh,
                           double* p9) {
  SPART_NO_CONTRACT
  for (int k = 0; k < LEAF_NPAR; ++k) p9[k] = base9[k];
  for (int ff = 0; ff < F; ++ff) p9[free_cols[ff]] = t[ff];
  if (f >= 1) p9[free_cols[f - 1]] = t[f - 1] + sh[f - 1];
}

// After the join of evaluation `it`: c the band part of the trial cost, bad the lanes' verdict, An the packed band sums of the
// trial (overwritten with the prior's part added when the trial is accepted).  mu / pw: the leaf's prior, both NULL without
// one.  Moves x, A and the state, and unless `last` writes the next trial into t.  -> refine_decide's code
SPART_HD int leaf_fit_update(int F, int it, bool last, LeafFit* s, double c, bool bad, double* An, double* A, double* x, double* t,
                             const double* lo, const double* hi, const double* mu, const double* pw, double* L, double* d) {
  double ct = c;
  if (pw) ct = refine_prior_total(F, ct, &bad, t, mu, pw);
  const RefineDecision dc = refine_decide(it, ct, bad, it == 0 ? 0.0 : s->cost, s->lam, s->na);
  if (it == 0) s->cost0 = ct;
  s->lam = dc.lam;
  s->na = dc.na;
  if (dc.code == 2) s->cost = ct;
  if (dc.code == 1) {
    s->cost = ct;
    for (int f = 0; f < F; ++f) x[f] = t[f];
    if (pw) refine_prior_augment(F, An, 1, x, 1, mu, pw);
    for (int e = 0; e < refine_ntri(F) + F; ++e) A[e] = An[e];
  }
  if (!last && (dc.code == 1 || dc.code == 3)) refine_propose(F, A, 1, s->lam, x, 1, lo, hi, L, 1, d, 1, t, 1);
  return dc.code;
}

// std of a finished fit from the undamped A of the last accepted point; a dead leaf's is NaN
SPART_HD void leaf_fit_std(int F, const LeafFit* s, const double* A, double* L, double* z, double* sdev) {
  if (s->na < 0) {
    for (int f = 0; f < F; ++f) sdev[f] = __builtin_nan("");
    return;
  }
  refine_std(F, A, 1, L, 1, z, 1, sdev, 1);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: k_refine_leaf<F>.  Single-wave workgroups; a workgroup takes leaves m = blockIdx.x, blockIdx.x + gridDim.x, ...
// Per evaluation: lane 0 writes the steps, lanes 0 ... F each form one row's nine constants into LDS (broadcast reads in the
// sweep), then ONE sweep of LEAF_PASSES passes in which lane l takes band 64 pass + l -- its BandTab, observations and weights
// arrive coalesced, the F + 1 rows go through leaf_band one after the other (the lane's Jacobian row waits in its own LDS
// column, stride 64: no bank conflict), and the cost, g and A terms are added to the lane's partials, which are registers
// because F is a template parameter (every index into them is a compile-time constant after unrolling).  The trial's sums
// are formed speculatively with its cost; lane 0 drops them on a reject and keeps the accepted point's joined sums in LDS.
// The join is the defined tree by cross-lane moves.  The small solve runs on wave-uniform data: lane 0 over LDS rows.
// Scalar registers.  The float64 literals of the leaf model nearly fill the scalar file by themselves (k_prospect<double>: 96
// SGPRs), and a sweep adds its exec masks.  So NOTHING else may live across a sweep in SGPRs: the arguments are read back from
// an LDS copy, flags and lane tests are formed again where they are used (leaf_lane, leaf_flag hide them from the
// optimiser, which would otherwise keep each as a 64-bit mask for the whole kernel), loop bounds come through
// v_readfirstlane.  With any of these left to the compiler it parks SGPRs in VGPR lanes around the sweep.
struct LeafFitArgs {
  const double* leaf[LEAF_NPAR];             // (M,) each
  int32_t free_col[LEAF_MAXF];
  int32_t n_iter, wper, pper;
  double lo[LEAF_MAXF], hi[LEAF_MAXF], h[LEAF_MAXF];
  double lambda0;
  const double *obs_r, *obs_t, *w_r, *w_t;   // (M, NWL) dense; weights (NWL,) with wper == 0; NULL: absent
  const double *pmu, *ppw;                   // (F,) or (M, F) with pper == 1; both NULL: no prior
  double *x, *cost, *cost0, *sdev;
  int32_t* n_accept;
  double *y_r, *y_t;
};
constexpr int LEAF_MAX_BLOCKS = 1 << 14;     // the grid at most: the wave-strided loop takes the rest

// `a` is the kernel's argument block, copied to LDS once: read from the kernel-argument segment its 26 pointers and 28
// constants would sit in SGPRs for the whole fit beside the float64 literals of the leaf model, which alone nearly fill the
// scalar file (k_prospect<double>: 96), and spill into VGPR lanes.
// (16-byte aligned and so a multiple of 16 bytes long, like every static LDS block of the family)
template <int F> struct alignas(16) LeafLds {
  static constexpr int NT = F * (F + 1) / 2, P = NT + F;
  // (the small rows first: their offsets fit the instructions' own offset fields, no register holds an LDS address for them)
  double lc[(F + 1) * LEAF_NC], base[LEAF_NPAR], rows[(F + 1) * LEAF_NPAR];
  double x[F], t[F], sh[F], A[P], An[P], L[NT], d[F], mu[F], pw[F], sdev[F];
  LeafFit fit;                               // (lane 0 keeps the leaf's state here, not in registers across a sweep)
  int64_t M;
  int stride, code;
  LeafFitArgs a;
  double J[2 * F * LEAF_LANES];              // [k][lane]: J_r of free parameter k < F, J_t at F + k
};

// threadIdx.x, and a flag, as values the optimiser cannot trace: every use forms its own compare, none is kept as a mask
__device__ __forceinline__ int leaf_lane() {
  int l = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  // (the lane number of a single-wave workgroup IS threadIdx.x; counted afresh, no register holds it between uses)
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
#endif
  return l;
}
__device__ __forceinline__ int leaf_flag(bool b) {
  int v = b ? 1 : 0;
  asm volatile("" : "+v"(v));
  return v;
}
// a value every lane holds alike (read from LDS) as a scalar
__device__ __forceinline__ int leaf_scalar(int v) { return __builtin_amdgcn_readfirstlane(v); }
// a pointer read back from the LDS copy of the arguments is a generic one: say that it points to global memory
#if defined(__HIP_DEVICE_COMPILE__)
template <typename T> using leaf_gp = T __attribute__((address_space(1)))*;
#else
template <typename T> using leaf_gp = T*;
#endif
template <typename T> __device__ __forceinline__ leaf_gp<T> leaf_global(T* p) { return (leaf_gp<T>)p; }

template <int F>
__global__ __launch_bounds__(64) void k_refine_leaf(const double* __restrict__ tab, const LeafFitArgs args, const int64_t M) {
  SPART_NO_CONTRACT
  constexpr int P = LeafLds<F>::P;
  __shared__ LeafLds<F> s;
  if (leaf_lane() == 0) {
    s.a = args;
    s.M = M;
    s.stride = gridDim.x;
  }
  stage_f64_tables();                                      // (ends with a barrier)
  // (M <= 2e9: a leaf's number fits 32 bits, and so does the sum below, which ends the loop before it could wrap)
  for (unsigned m = blockIdx.x; leaf_scalar((int64_t)m < s.M); m += (unsigned)leaf_scalar(s.stride)) {
    __syncthreads();                                       // the previous leaf's rows have been read by every lane
    if (leaf_lane() == 0) {
      for (int k = 0; k < LEAF_NPAR; ++k) s.base[k] = leaf_global(s.a.leaf[k])[m];
      if (s.a.ppw) {
        const int64_t pm = s.a.pper ? (int64_t)m * F : 0;
        for (int f = 0; f < F; ++f) {
          s.mu[f] = leaf_global(s.a.pmu)[pm + f];
          s.pw[f] = leaf_global(s.a.ppw)[pm + f];
        }
      }
      leaf_fit_start(F, s.base, s.a.free_col, s.a.lo, s.a.hi, s.a.lambda0, s.x, s.t, &s.fit);
    }
    for (int it = 0; it <= leaf_scalar(s.a.n_iter); ++it) {
      if (leaf_lane() == 0) leaf_fit_steps(F, s.t, s.a.h, s.a.hi, s.sh);
      __syncthreads();
      {
        const int lane = leaf_lane();
        if (lane <= F) {
          leaf_fit_row(F, lane, s.base, s.a.free_col, s.t, s.sh, s.rows + lane * LEAF_NPAR);
          leaf_row_constants(s.rows + lane * LEAF_NPAR, s.lc + lane * LEAF_NC);
        }
      }
      __syncthreads();
      // ---- the sweep
      LeafPartial<F> acc;
      leaf_partial_zero(acc);
      {
        const int lane = leaf_lane();
#pragma unroll 1
        for (int pass = 0; pass < LEAF_PASSES; ++pass) {
          // (nothing read from LDS is carried from pass to pass: the pointers and flags are formed again, which costs a few
          // ds_reads and frees their dozen VGPRs for the leaf model at F = 9)
          asm volatile("" ::: "memory");
          unsigned mp = m;                                 // (its 64-bit product with 2001 is formed here, not kept)
          asm volatile("" : "+s"(mp));
          const int i = pass * LEAF_LANES + lane;
          if (i < NWL) {
            auto tab_at = [&]() {
              asm volatile("" ::: "memory");               // (a load of its own per row: L1 hits, not 22 VGPRs held)
              return load_tab(tab, i);
            };
            const bool hr = s.a.obs_r != nullptr, ht = s.a.obs_t != nullptr;
            const int64_t row = (int64_t)mp * NWL + i, wrow = s.a.wper ? row : i;
            double wr = 0.0, obr = 0.0, wt = 0.0, obt = 0.0;
            if (hr) {
              wr = s.a.w_r ? leaf_global(s.a.w_r)[wrow] : 1.0;
              obr = leaf_global(s.a.obs_r)[row];
            }
            if (ht) {
              wt = s.a.w_t ? leaf_global(s.a.w_t)[wrow] : 1.0;
              obt = leaf_global(s.a.obs_t)[row];
            }
            leaf_partial_band<F>(acc, tab_at, s.lc, s.sh, hr, wr, obr, ht, wt, obt, s.J + lane, LEAF_LANES);
          }
        }
      }
      // ---- the join: p_l = p_l + p_(l + d), d = 32 ... 1 (lanes l >= d add what nobody reads)
#pragma unroll
      for (int d = LEAF_LANES / 2; d >= 1; d >>= 1) {
        acc.c = leaf_join_add(acc.c, __shfl_down(acc.c, d));
#pragma unroll
        for (int e = 0; e < P; ++e) acc.s[e] = leaf_join_add(acc.s[e], __shfl_down(acc.s[e], d));
      }
      const bool bad = __builtin_amdgcn_ballot_w64(acc.bad != 0) != 0;
      if (leaf_lane() == 0) {
#pragma unroll
        for (int e = 0; e < P; ++e) s.An[e] = acc.s[e];
        const bool last = it == s.a.n_iter;
        // (F as a value the optimiser cannot see through: the solve's loops stay loops.  Unrolled for F >= 8 they keep so many
        // LDS loads in flight that the register file overflows)
        int Fr = F;
        asm volatile("" : "+v"(Fr));
        if (s.a.ppw) s.code = leaf_fit_update(Fr, it, last, &s.fit, acc.c, bad, s.An, s.A, s.x, s.t, s.a.lo, s.a.hi, s.mu, s.pw, s.L, s.d);
        else s.code = leaf_fit_update(Fr, it, last, &s.fit, acc.c, bad, s.An, s.A, s.x, s.t, s.a.lo, s.a.hi, nullptr, nullptr, s.L, s.d);
      }
      __syncthreads();
      if (leaf_scalar(s.code) == 2) break;                 // dead from the start: nothing of it moves again
    }
    // ---- the outputs, and the closing pass for the spectra at x
    const bool want_y = leaf_scalar(s.a.y_r != nullptr || s.a.y_t != nullptr) != 0;
    if (leaf_lane() == 0) {
      for (int f = 0; f < F; ++f) leaf_global(s.a.x)[(int64_t)m * F + f] = s.x[f];
      leaf_global(s.a.cost)[m] = s.fit.cost;
      if (s.a.cost0) leaf_global(s.a.cost0)[m] = s.fit.cost0;
      if (s.a.n_accept) leaf_global(s.a.n_accept)[m] = s.fit.na;
      if (s.a.sdev) {
        int Fr = F;
        asm volatile("" : "+v"(Fr));
        leaf_fit_std(Fr, &s.fit, s.A, s.L, s.d, s.sdev);
        for (int f = 0; f < F; ++f) leaf_global(s.a.sdev)[(int64_t)m * F + f] = s.sdev[f];
      }
      if (want_y) {
        leaf_fit_row(F, 0, s.base, s.a.free_col, s.x, s.sh, s.rows);
        leaf_row_constants(s.rows, s.lc);
      }
    }
    if (want_y) {
      __syncthreads();
      const int lane = leaf_lane();
      const int gyr = leaf_flag(s.a.y_r != nullptr), gyt = leaf_flag(s.a.y_t != nullptr);
      const auto yr_m = leaf_global(s.a.y_r) + (gyr ? (int64_t)m * NWL : 0);
      const auto yt_m = leaf_global(s.a.y_t) + (gyt ? (int64_t)m * NWL : 0);
#pragma unroll 1
      for (int pass = 0; pass < LEAF_PASSES; ++pass) {
        const int i = pass * LEAF_LANES + lane;
        if (i < NWL) {
          const BandTab<double> tb = load_tab(tab, i);
          double yr, yt;
          leaf_row_band(tb, s.lc, yr, yt);
          if (gyr != 0) yr_m[i] = yr;
          if (gyt != 0) yt_m[i] = yt;
        }
      }
    }
  }
}
#endif  // __HIPCC__

}  // namespace spart
