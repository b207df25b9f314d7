// Refinement with parameters shared by a tile of pixels (spart_refine_tiles, include/spart_hip.h; the definition is
// tools/refine_tiles_defined.py and every function here reproduces it bit for bit): spart_refine's fit with Fs unknowns per
// TILE of contiguous pixels and Fl = F - Fs unknowns per pixel, one Levenberg-Marquardt decision per tile.  The per-entry
// arithmetic is csrc/spart_refine.h's part 1; k_refine_step is not touched.
//
// Part 1: the index maps, the per-pixel elimination pieces and the small per-tile solves, SPART_HD so that g++ compiles them
// for tests/hostmath/refine_tiles_host.cpp.  Strides as in spart_refine.h (element k at p[k * S]).
// Index conventions.  free_cols lists the F free columns by NAME, the shared ones first; bounds and steps belong to a name.
// Inside a pixel the unknowns are taken in SOLVE ORDER, every local first: q = b for local name Fs + b, q = Fl + a for shared
// name a.  The packed vector of a pixel (P = ntri(F) + F doubles) is spart_refine's A then g in that order, so with one pixel
// per tile the call is spart_refine with free_cols = local names then shared names.  The packed vector of a tile
// (Ps = ntri(Fs) + Fs) is the shared block S then gs.  The unknowns of a tile are every live pixel's locals, pixels ascending,
// then the shared ones; entries between locals of different pixels are structurally absent and skipped.
#pragma once

#include "spart_refine.h"

namespace spart {

constexpr int TILES_MAXG = 4096;             // pixels per tile

// name f -> solve index, and back
SPART_HD int tiles_sol(int f, int Fs, int Fl) { return f < Fs ? Fl + f : f - Fs; }
SPART_HD int tiles_name(int q, int Fs, int Fl) { return q < Fl ? Fs + q : q - Fl; }
// refine_pair under the name this header gave it before the family shared one (host code written against that name compiles)
SPART_HD void tiles_pair(int e, int* a, int* b) { refine_pair(e, a, b); }
// pixels of one chunk at most
SPART_HD int64_t tiles_chunk(int F) { return REFINE_ROWS / (int64_t)(F + 1); }

// refine_cholesky over the columns j < Fl only: the local block of L becomes R_m, the local part of a shared row W_m, the
// shared block stays; false at a pivot !(s > 0)
SPART_HD bool tiles_eliminate(int F, int Fl, double* L, int S) {
  SPART_NO_CONTRACT
  for (int i = 0; i < F; ++i) {
    const int jn = i + 1 < Fl ? i + 1 : Fl;
    for (int j = 0; j < jn; ++j) {
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

// R_m d_m = -g_m[local], k ascending; g and d may be the same array
SPART_HD void tiles_local_forward(int Fl, const double* L, int SL, const double* g, int SG, double* d, int SD) {
  SPART_NO_CONTRACT
  for (int j = 0; j < Fl; ++j) {
    double s = -g[j * SG];
    for (int k = 0; k < j; ++k) s = s - L[refine_tri(j, k) * SL] * d[k * SD];
    d[j * SD] = s / L[refine_tri(j, j) * SL];
  }
}

// the local back substitution: j from Fl - 1 down, k = j + 1 .. Fl - 1 first and the shared a ascending after; d in place
SPART_HD void tiles_local_back(int Fs, int Fl, const double* L, int SL, const double* ds, int SS, double* d, int SD) {
  SPART_NO_CONTRACT
  for (int j = Fl - 1; j >= 0; --j) {
    double s = d[j * SD];
    for (int k = j + 1; k < Fl; ++k) s = s - L[refine_tri(k, j) * SL] * d[k * SD];
    for (int a = 0; a < Fs; ++a) s = s - L[refine_tri(Fl + a, j) * SL] * ds[a * SS];
    d[j * SD] = s / L[refine_tri(j, j) * SL];
  }
}

// std of local j of a pixel: refine_std's recurrence over the pixel's locals >= j and then every shared unknown.
// L: the pixel's undamped R_m / W_m; Ls: the tile's undamped shared factor; z (F) is scratch.
SPART_HD double tiles_local_std(int Fs, int Fl, int j, const double* L, int SL, const double* Ls, int SS, double* z, int SZ) {
  SPART_NO_CONTRACT
  double var = 0.0;
  for (int k = j; k < Fl; ++k) {
    double s = k == j ? 1.0 : 0.0;
    for (int i = j; i < k; ++i) s = s - L[refine_tri(k, i) * SL] * z[i * SZ];
    const double zk = s / L[refine_tri(k, k) * SL];
    z[k * SZ] = zk;
    var = var + zk * zk;
  }
  for (int a = 0; a < Fs; ++a) {
    double s = 0.0;
    for (int i = j; i < Fl; ++i) s = s - L[refine_tri(Fl + a, i) * SL] * z[i * SZ];
    for (int i = 0; i < a; ++i) s = s - Ls[refine_tri(a, i) * SS] * z[(Fl + i) * SZ];
    const double zk = s / Ls[refine_tri(a, a) * SS];
    z[(Fl + a) * SZ] = zk;
    var = var + zk * zk;
  }
  return __builtin_sqrt(var);
}

// The ordered walk over a tile's live pixels, for packed shared entry e of Ps, takes per pixel
// acc - sum_k W_m[a, k] W_m[b, k] (e < ntri(Fs)) or acc - sum_k W_m[a, k] d_(m, k) (the right-hand side): both are
// acc - sum_k Lm[oa + k] Lm[ob + k] on the pixel's eliminated packed vector Lm (d in its g slots) with these two offsets.
SPART_HD void tiles_schur_offsets(int e, int F, int Fs, int Fl, int* oa, int* ob) {
  const int nts = refine_ntri(Fs);
  int a = e - nts, b = -1;
  if (e < nts) refine_pair(e, &a, &b);
  *oa = refine_tri(Fl + a, 0);
  *ob = b >= 0 ? refine_tri(Fl + b, 0) : refine_ntri(F);
}
SPART_HD double tiles_schur_pixel(double acc, int oa, int ob, int Fl, const double* Lm) {
  SPART_NO_CONTRACT
  for (int k = 0; k < Fl; ++k) acc = acc - Lm[oa + k] * Lm[ob + k];
  return acc;
}

// The shared factor from the Schur sums (in place, dense packed): for shared k < b: s = s - Ls[a, k] Ls[b, k]
SPART_HD bool tiles_shared_factor(int Fs, double* Ls) {
  SPART_NO_CONTRACT
  for (int a = 0; a < Fs; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = Ls[refine_tri(a, b)];
      for (int k = 0; k < b; ++k) s = s - Ls[refine_tri(a, k)] * Ls[refine_tri(b, k)];
      if (a == b) {
        if (!(s > 0.0)) return false;
        Ls[refine_tri(a, a)] = __builtin_sqrt(s);
      } else {
        Ls[refine_tri(a, b)] = s / Ls[refine_tri(b, b)];
      }
    }
  return true;
}

// The shared forward and back substitution on the walked right-hand side ds (in place); false at a non-finite delta
SPART_HD bool tiles_shared_solve(int Fs, const double* Ls, double* ds) {
  SPART_NO_CONTRACT
  for (int a = 0; a < Fs; ++a) {
    double s = ds[a];
    for (int k = 0; k < a; ++k) s = s - Ls[refine_tri(a, k)] * ds[k];
    ds[a] = s / Ls[refine_tri(a, a)];
  }
  for (int a = Fs - 1; a >= 0; --a) {
    double s = ds[a];
    for (int k = a + 1; k < Fs; ++k) s = s - Ls[refine_tri(k, a)] * ds[k];
    ds[a] = s / Ls[refine_tri(a, a)];
  }
  bool ok = true;
  for (int a = 0; a < Fs; ++a)
    if (!(ds[a] - ds[a] == 0.0)) ok = false;
  return ok;
}

// std of shared f: refine_std's recurrence over the shared unknowns >= f; z (Fs) is scratch
SPART_HD double tiles_shared_std(int Fs, int f, const double* Ls, double* z) {
  SPART_NO_CONTRACT
  double var = 0.0;
  for (int k = f; k < Fs; ++k) {
    double s = k == f ? 1.0 : 0.0;
    for (int i = f; i < k; ++i) s = s - Ls[refine_tri(k, i)] * z[i];
    const double zk = s / Ls[refine_tri(k, k)];
    z[k] = zk;
    var = var + zk * zk;
  }
  return __builtin_sqrt(var);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: the kernels.  One chunk of Mc pixels in Tc whole tiles owns spart_refine's table (27, (F + 1) Mc), row = f Mc + m,
// and cols ((F + 1) Mc, nb), and the state
//   per pixel  lt (Mc, Fl) the trial locals, ct (Mc) the trial cost, live (Mc) 1 / 0, Ap (Mc, P) the packed sums of the last
//              accepted point, Lp (Mc, P) their eliminated form (R_m, W_m, d_m in the g slots; afterwards delta_l there);
//   per tile   zt (Tc, Fs) the trial shared values, St (Tc, Ps) the shared sums of the last accepted point, Lt (Tc, Ps) the
//              shared factor and delta_s, lam, na (-1: dead), code (0 idle, 1 accepted, 2 dead since this call, 3 rejected),
//              flag (nonzero: a failed pivot or a non-finite delta somewhere in the tile -- an integer OR, free of order);
//   maps       tstart (Tc + 1) the tiles' first pixels within the chunk, ptile (Mc) the tile of a pixel.
// out.shared / out.local ARE the accepted point and out.cost its cost.  A rejected tile keeps Ap and St: they are only ever
// overwritten on acceptance, which is the restore the definition asks for.
// Per iteration, after the forward call: k_tiles_cost (per pixel), k_tiles_decide (per tile: the ordered cost sum, the
// decision, lambda), k_tiles_normal (one thread per packed entry of a pixel of an accepted tile), k_tiles_eliminate (groups
// of 8 pixels through LDS, one lane per pixel), k_tiles_schur (per tile, one lane per packed shared entry walks the tile's
// pixels in order; the loads of a step do not depend on the add chain), k_tiles_local (delta_l or, last, the std outputs),
// k_tiles_apply (clip and the next trial's table rows).  Every sum has the definition's order whatever the launch shape.
constexpr int TILES_GROUP = 8;               // pixels per workgroup of the LDS-staged per-pixel kernels
constexpr int TILES_SCHUR_THREADS = 192;     // >= ntri(16) + 16 = 152 packed shared entries
constexpr int TILES_WALK = 16;               // pixels k_tiles_schur stages per step of its walk: 16 * 152 * 8 B of LDS at F = 16

inline size_t tiles_lds_bytes(int F) { return (size_t)(refine_ntri(F) + 2 * F) * (TILES_GROUP + 1) * 8; }

struct TilesOut {                              // the call's outputs moved to the chunk's first tile / pixel; NULL: not asked for
  double *shared, *shared_std, *local, *local_std, *cost, *cost0;
  int32_t* n_accept;
  double* pixel_cost;
  int32_t* status;
  double* y;
};

struct TilesState {
  double *lt, *ct, *Ap, *Lp, *zt, *St, *Lt, *lam;
  int32_t *live, *na, *code, *flag, *tstart, *ptile;
};

// Once per chunk, one thread per pixel: the whole table, the clipped start as the accepted point and the first trial.  A
// shared column is read at the tile's first pixel only.
__global__ __launch_bounds__(256) void k_tiles_init(RefineCfg a, int64_t m0, int Mc, int F, int Fs, double lambda0, TilesState s,
                                                    double* __restrict__ table, TilesOut out, double* __restrict__ cfg,
                                                    int32_t* __restrict__ cfg_free) {
  SPART_NO_CONTRACT
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && (int)threadIdx.x < REFINE_MAXF) refine_cfg_copy(a, threadIdx.x, threadIdx.x, cfg, cfg_free);
  if (m >= Mc) return;
  const int Fl = F - Fs, t = s.ptile[m], first = s.tstart[t];
  const int64_t R = (int64_t)(F + 1) * Mc;
  refine_fill_fixed(a, m0 + m, table + m, R, F, Mc);
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    const double tf = refine_clip(a.freebase[f][m0 + (f < Fs ? first : m)], a.lo[f], a.hi[f]);
    const double moved = tf + refine_fd_step(tf, a.h[f], a.hi[f]);
    if (f >= Fs) {
      out.local[(int64_t)m * Fl + (f - Fs)] = tf;
      s.lt[(int64_t)m * Fl + (f - Fs)] = tf;
    } else if (m == first) {
      out.shared[(int64_t)t * Fs + f] = tf;
      s.zt[(int64_t)t * Fs + f] = tf;
    }
    refine_fill_row(table + a.free_col[f] * R + m, F, Mc, f + 1, tf, moved);
  }
  if (m == first) {
    s.lam[t] = lambda0;
    s.na[t] = 0;
  }
}

// The trial cost of every pixel from block 0 of cols: bands ascending, then the local prior, b ascending.  it == 0 decides the
// dead pixels and writes their outputs.  obs / wts / pmu / ppw are the chunk's rows (wts NULL, (nb,) or rows; prior NULL, (Fl,)
// or rows).
__global__ __launch_bounds__(256) void k_tiles_cost(const double* __restrict__ cols, const double* __restrict__ obs,
                                                    const double* __restrict__ wts, int wper, const double* __restrict__ pmu,
                                                    const double* __restrict__ ppw, int pper, int Mc, int Fl, int nb, int it,
                                                    TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= Mc) return;
  if (it > 0 && (!s.live[m] || s.na[s.ptile[m]] < 0)) return;
  const double* y0 = cols + (int64_t)m * nb;
  const double* ob = obs + (int64_t)m * nb;
  const double* wr = wts ? (wper ? wts + (int64_t)m * nb : wts) : nullptr;
  double c = 0.0;
  bool bad = false;
  for (int j = 0; j < nb; ++j) {                                    // (refine_tile_cost with weights that may be absent)
    const double w = wr ? wr[j] : 1.0;
    if (refine_bad_weight(w)) bad = true;
    if (w == 0.0) continue;
    c = refine_cost_band(c, w, y0[j], ob[j]);
  }
  if (ppw) {
    const int64_t pm = pper ? (int64_t)m * Fl : 0;
    c = refine_prior_total(Fl, c, &bad, s.lt + (int64_t)m * Fl, pmu + pm, ppw + pm);
  }
  s.ct[m] = c;
  if (it == 0) {
    const bool alive = c < __builtin_inf() && !bad;
    s.live[m] = alive ? 1 : 0;
    if (out.status) out.status[m] = alive ? 0 : -1;
    if (!alive) {
      if (out.pixel_cost) out.pixel_cost[m] = c;
      if (out.local_std)
        for (int b = 0; b < Fl; ++b) out.local_std[(int64_t)m * Fl + b] = __builtin_nan("");
      if (out.y)
        for (int j = 0; j < nb; ++j) out.y[(int64_t)m * nb + j] = y0[j];
    }
  }
}

// One single-wave workgroup per tile: C = 0; for live m ascending: C = C + c_m (64 pixels at a time through LDS, lane 0 adds);
// then the shared prior, a ascending; then the decision, lambda, n_accept.  smu / spw: NULL, (Fs,) or the chunk's (Tc, Fs).
__global__ __launch_bounds__(64) void k_tiles_decide(const double* __restrict__ smu, const double* __restrict__ spw, int sper,
                                                     int Fs, int it, int last, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  __shared__ double cv[64];
  __shared__ int lv[64];
  __shared__ int code_s;
  const int t = blockIdx.x, lane = threadIdx.x;
  int na = s.na[t];
  if (it > 0 && na < 0) {                                          // (block-uniform) a dead tile changes no more
    if (lane == 0) s.code[t] = 0;
    return;
  }
  const int b0 = s.tstart[t], b1 = s.tstart[t + 1];
  double C = 0.0;
  bool any = false;
  int nl = b0 + lane < b1 ? s.live[b0 + lane] : 0;                   // the next 64 pixels, loaded while lane 0 adds the current
  double nv = b0 + lane < b1 ? s.ct[b0 + lane] : 0.0;
  for (int p0 = b0; p0 < b1; p0 += 64) {
    lv[lane] = nl;
    cv[lane] = nv;
    __syncthreads();
    const int m = p0 + 64 + lane;
    nl = m < b1 ? s.live[m] : 0;
    nv = m < b1 ? s.ct[m] : 0.0;
    if (lane == 0) {
#pragma unroll 8
      for (int i = 0; i < 64; ++i) {                                 // (beyond the tile: lv = 0)
        const double c = C + cv[i];
        C = lv[i] ? c : C;
        any = any || lv[i];
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    bool bad = false;
    if (spw) {
      const int64_t pt = sper ? (int64_t)t * Fs : 0;
      C = refine_prior_total(Fs, C, &bad, s.zt + (int64_t)t * Fs, smu + pt, spw + pt);
    }
    int code;
    double lam = s.lam[t];
    if (it == 0) {
      code = (any && !bad && C < __builtin_inf()) ? 1 : 2;
      if (out.cost0) out.cost0[t] = C;
      if (code == 2) {
        na = -1;
        out.cost[t] = C;
        if (out.n_accept) out.n_accept[t] = -1;
        if (out.shared_std)
          for (int a = 0; a < Fs; ++a) out.shared_std[(int64_t)t * Fs + a] = __builtin_nan("");
      }
    } else {
      code = C < out.cost[t] ? 1 : 3;
      lam = refine_lambda(lam, code == 1);
      if (code == 1) ++na;
    }
    if (code == 1) {
      out.cost[t] = C;
      for (int a = 0; a < Fs; ++a) out.shared[(int64_t)t * Fs + a] = s.zt[(int64_t)t * Fs + a];
    }
    s.lam[t] = lam;
    s.na[t] = na;
    s.code[t] = code;
    s.flag[t] = 0;
    if (last && code != 2 && out.n_accept) out.n_accept[t] = na;
    code_s = code;
  }
  __syncthreads();
  if (code_s == 2 && out.status)
    for (int m = b0 + lane; m < b1; m += 64)
      if (s.live[m]) out.status[m] = 1;
}

// One thread per packed entry e of a pixel (index m P + e, so a wave stays within a few pixels): the pixel outputs of an
// accepted or newly dead tile, and for an accepted tile entry e of A_m / g_m in solve order, bands ascending, J formed on the
// fly, then the local prior's part.  cfg: lo, hi, h per NAME.
__global__ __launch_bounds__(256) void k_tiles_normal(const double* __restrict__ cols, const double* __restrict__ obs,
                                                      const double* __restrict__ wts, int wper, const double* __restrict__ pmu,
                                                      const double* __restrict__ ppw, int pper, const double* __restrict__ cfg,
                                                      int Mc, int F, int Fs, int nb, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Mc * P) return;
  const int m = (int)(idx / P), e = (int)(idx % P);
  const int t = s.ptile[m], code = s.code[t];
  if ((code != 1 && code != 2) || !s.live[m]) return;
  const double* y0 = cols + (int64_t)m * nb;
  if (out.y)
    for (int j = e; j < nb; j += P) out.y[(int64_t)m * nb + j] = y0[j];
  if (e == 0 && out.pixel_cost) out.pixel_cost[m] = s.ct[m];
  if (code == 2) {
    if (out.local_std)
      for (int b = e; b < Fl; b += P) out.local_std[(int64_t)m * Fl + b] = __builtin_nan("");
    return;
  }
  for (int b = e; b < Fl; b += P) out.local[(int64_t)m * Fl + b] = s.lt[(int64_t)m * Fl + b];
  int qa, qb = -1;                                                 // e < nt: A_ab; else g_a against r
  if (e < nt) refine_pair(e, &qa, &qb);
  else qa = e - nt;
  const int fa = tiles_name(qa, Fs, Fl), fb = qb >= 0 ? tiles_name(qb, Fs, Fl) : 0;
  const double* hi = cfg + REFINE_MAXF;
  const double* hh = cfg + 2 * REFINE_MAXF;
  const double ta = fa < Fs ? s.zt[(int64_t)t * Fs + fa] : s.lt[(int64_t)m * Fl + (fa - Fs)];
  const double tb = fb < Fs ? s.zt[(int64_t)t * Fs + fb] : s.lt[(int64_t)m * Fl + (fb - Fs)];
  const double sha = refine_fd_step(ta, hh[fa], hi[fa]), shb = refine_fd_step(tb, hh[fb], hi[fb]);
  const double* ya = cols + ((int64_t)(fa + 1) * Mc + m) * nb;
  const double* yb = cols + ((int64_t)(fb + 1) * Mc + m) * nb;
  const double* ob = obs + (int64_t)m * nb;
  const double* wr = wts ? (wper ? wts + (int64_t)m * nb : wts) : nullptr;
  double acc = 0.0;
  for (int j = 0; j < nb; ++j) {
    const double w = wr ? wr[j] : 1.0;
    if (w == 0.0) continue;
    const double y = y0[j];
    const double ja = refine_jacobian(ya[j], y, sha);
    const double jb = qb >= 0 ? refine_jacobian(yb[j], y, shb) : refine_residual(y, ob[j]);
    acc = refine_mac(acc, w, ja, jb);
  }
  if (ppw && qa < Fl && (qb == qa || qb < 0)) {
    const int64_t pm = pper ? (int64_t)m * Fl : 0;
    const double p = ppw[pm + qa];
    if (p != 0.0) acc = qb >= 0 ? acc + p : refine_prior_gain(acc, p, refine_residual(ta, pmu[pm + qa]));
  }
  s.Ap[idx] = acc;
}

// Groups of TILES_GROUP pixels, one wave: Ap staged through LDS at [e][o], lane o < 8 damps the local diagonal (not on the
// last call: the std comes from the undamped sums), eliminates and runs the local forward substitution into the g slots; the
// result goes to Lp.  A failed pivot raises the tile's flag.
__global__ __launch_bounds__(64) void k_tiles_eliminate(int Mc, int F, int Fs, int last, TilesState s) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char tiles_smem[];
  constexpr int W = TILES_GROUP, WP = W + 1;
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F;
  double* Ll = reinterpret_cast<double*>(tiles_smem);              // [e][o]
  const int lane = threadIdx.x, g0 = blockIdx.x * W, m = g0 + lane;
  const int n = Mc - g0 < W ? Mc - g0 : W;                         // pixels of this group
  const double* src = s.Ap + (int64_t)g0 * P;
  for (int i = lane; i < n * P; i += 64) Ll[(i % P) * WP + i / P] = src[i];
  __syncthreads();
  if (lane < n && s.live[m]) {
    const int t = s.ptile[m], code = s.code[t];
    if (code == 1 || code == 3) {
      double* L = Ll + lane;
      if (!last) {
        const double lam = s.lam[t];
        for (int j = 0; j < Fl; ++j) {
          const double v = L[refine_tri(j, j) * WP];
          L[refine_tri(j, j) * WP] = v + lam * (v > 0.0 ? v : 1.0);
        }
      }
      if (!tiles_eliminate(F, Fl, L, WP)) atomicOr(&s.flag[t], 1);
      else if (!last) tiles_local_forward(Fl, L, WP, L + nt * WP, WP, L + nt * WP, WP);
    }
  }
  __syncthreads();
  double* dst = s.Lp + (int64_t)g0 * P;
  for (int i = lane; i < n * P; i += 64) dst[i] = Ll[(i % P) * WP + i / P];
}

// One workgroup per tile, lane e < Ps on packed shared entry e.  The walk over the tile's pixels stages TILES_WALK pixels'
// packed vectors at a time in LDS -- pixel-major scratch, so a stage is one contiguous run loaded by all lanes -- and every lane
// then takes its entry of the live ones in order: no load of the add chain waits for global memory.  Accepted: S / gs from Ap,
// then the shared prior -> St.  Then the (damped) entry minus the Schur sums over Lp in the same order; lane 0 finishes the small
// factor and the shared solve (or, last, the shared std) in LDS -> Lt.
__global__ __launch_bounds__(TILES_SCHUR_THREADS) void k_tiles_schur(const double* __restrict__ smu, const double* __restrict__ spw,
                                                                     int sper, int F, int Fs, int last, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  constexpr int PMAX = REFINE_MAXF * (REFINE_MAXF + 1) / 2 + REFINE_MAXF;
  __shared__ double stage[TILES_WALK * PMAX];
  __shared__ int lvs[TILES_WALK];
  __shared__ double sh[PMAX];
  __shared__ double zs[REFINE_MAXF];
  const int t = blockIdx.x, e = threadIdx.x;
  const int code = s.code[t];
  if (code != 1 && code != 3) return;                              // (block-uniform)
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs;
  const int b0 = s.tstart[t], b1 = s.tstart[t + 1];
  int a = e - nts, b = -1;
  if (e < nts) refine_pair(e, &a, &b);
  // step(acc, the staged packed vector of a live pixel) for every live pixel of the tile in order (every lane takes part)
  auto walk = [&](const double* __restrict__ src, double acc, auto&& step) {
    for (int p0 = b0; p0 < b1; p0 += TILES_WALK) {
      const int n = b1 - p0 < TILES_WALK ? b1 - p0 : TILES_WALK;
      __syncthreads();
      const double* run = src + (int64_t)p0 * P;
      for (int i = e; i < n * P; i += TILES_SCHUR_THREADS) stage[i] = run[i];
      if (e < n) lvs[e] = s.live[p0 + e];
      __syncthreads();
      if (e < Ps)
        for (int i = 0; i < n; ++i)
          if (lvs[i]) acc = step(acc, stage + i * P);
    }
    return acc;
  };
  double acc = 0.0;
  if (code == 1) {                                                 // (block-uniform)
    const int at = b >= 0 ? refine_tri(Fl + a, Fl + b) : nt + Fl + a;
    acc = walk(s.Ap, 0.0, [&](double v, const double* Am) { return v + Am[at]; });
    if (e < Ps) {
      if (spw && (b == a || b < 0)) {
        const int64_t pt = sper ? (int64_t)t * Fs : 0;
        const double p = spw[pt + a];
        if (p != 0.0) acc = b >= 0 ? acc + p : refine_prior_gain(acc, p, refine_residual(out.shared[(int64_t)t * Fs + a], smu[pt + a]));
      }
      s.St[(int64_t)t * Ps + e] = acc;
    }
  } else if (e < Ps) {
    acc = s.St[(int64_t)t * Ps + e];
  }
  if (e < Ps) {
    if (b == a && !last) acc = acc + s.lam[t] * (acc > 0.0 ? acc : 1.0);
    if (b < 0) acc = -acc;
  }
  {
    int oa = 0, ob = 0;
    if (e < Ps) tiles_schur_offsets(e, F, Fs, Fl, &oa, &ob);
    const bool mine = b >= 0 || !last;                             // (the right-hand side is not needed for the std)
    acc = walk(s.Lp, acc, [&](double v, const double* Lm) { return mine ? tiles_schur_pixel(v, oa, ob, Fl, Lm) : v; });
  }
  if (e < Ps) sh[e] = acc;
  __syncthreads();
  if (e == 0) {
    bool ok = tiles_shared_factor(Fs, sh);
    if (ok && !last) ok = tiles_shared_solve(Fs, sh, sh + nts);
    if (!ok) s.flag[t] = s.flag[t] | 1;
    if (last && out.shared_std)
      for (int f = 0; f < Fs; ++f)
        out.shared_std[(int64_t)t * Fs + f] = s.flag[t] == 0 ? tiles_shared_std(Fs, f, sh, zs) : __builtin_nan("");
  }
  __syncthreads();
  if (e < Ps) s.Lt[(int64_t)t * Ps + e] = sh[e];
}

// Groups of TILES_GROUP pixels through LDS as in k_tiles_eliminate: delta_l by the local back substitution into Lp's g slots
// (a non-finite one raises the tile's flag), or on the last call local_std.
__global__ __launch_bounds__(64) void k_tiles_local(int Mc, int F, int Fs, int last, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char tiles_smem[];
  constexpr int W = TILES_GROUP, WP = W + 1;
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs;
  double* Ll = reinterpret_cast<double*>(tiles_smem);              // [e][o]
  double* zl = Ll + P * WP;                                        // [f][o]
  const int lane = threadIdx.x, g0 = blockIdx.x * W, m = g0 + lane;
  const int n = Mc - g0 < W ? Mc - g0 : W;
  double* rows = s.Lp + (int64_t)g0 * P;
  for (int i = lane; i < n * P; i += 64) Ll[(i % P) * WP + i / P] = rows[i];
  __syncthreads();
  if (lane < n && s.live[m]) {
    const int t = s.ptile[m], code = s.code[t];
    if (code == 1 || code == 3) {
      const double* L = Ll + lane;
      const double* Lt = s.Lt + (int64_t)t * Ps;
      if (!last) {
        double* d = Ll + nt * WP + lane;
        tiles_local_back(Fs, Fl, L, WP, Lt + nts, 1, d, WP);
        bool ok = true;
        for (int j = 0; j < Fl; ++j) {
          const double v = d[j * WP];
          if (!(v - v == 0.0)) ok = false;
        }
        if (!ok) atomicOr(&s.flag[t], 2);
      } else if (out.local_std) {
        const bool ok = s.flag[t] == 0;
        for (int j = 0; j < Fl; ++j)
          out.local_std[(int64_t)m * Fl + j] = ok ? tiles_local_std(Fs, Fl, j, L, WP, Lt, 1, zl + lane, WP) : __builtin_nan("");
      }
    }
  }
  if (last) return;                                                // (kernel-uniform)
  __syncthreads();
  for (int i = lane; i < n * Fl; i += 64) rows[(i / Fl) * P + nt + i % Fl] = Ll[(nt + i % Fl) * WP + i / Fl];
}

// One thread per pixel of a live tile: t = clip(x + delta), delta = 0 for the whole tile under a raised flag; the trial state
// and the F (F + 1) table entries of a live pixel.  The tile's first pixel writes zt, live or not.
__global__ __launch_bounds__(256) void k_tiles_apply(const double* __restrict__ cfg, const int32_t* __restrict__ cfg_free,
                                                     double* __restrict__ table, int Mc, int F, int Fs, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= Mc) return;
  const int t = s.ptile[m], code = s.code[t];
  if (code != 1 && code != 3) return;
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs;
  const bool ok = s.flag[t] == 0, alive = s.live[m] != 0, first = m == s.tstart[t];
  if (!alive && !first) return;
  const double* lo = cfg;
  const double* hi = cfg + REFINE_MAXF;
  const double* hh = cfg + 2 * REFINE_MAXF;
  const int64_t R = (int64_t)(F + 1) * Mc;
  for (int f = 0; f < F; ++f) {
    if (f >= Fs && !alive) break;
    const double x = f < Fs ? out.shared[(int64_t)t * Fs + f] : out.local[(int64_t)m * Fl + (f - Fs)];
    const double dl = !ok ? 0.0 : f < Fs ? s.Lt[(int64_t)t * Ps + nts + f] : s.Lp[(int64_t)m * P + nt + (f - Fs)];
    const double tf = refine_clip(x + dl, lo[f], hi[f]);
    if (f < Fs) {
      if (first) s.zt[(int64_t)t * Fs + f] = tf;
    } else {
      s.lt[(int64_t)m * Fl + (f - Fs)] = tf;
    }
    if (!alive) continue;
    refine_fill_row(table + cfg_free[f] * R + m, F, Mc, f + 1, tf, tf + refine_fd_step(tf, hh[f], hi[f]));
  }
}
#endif  // __HIPCC__

}  // namespace spart
