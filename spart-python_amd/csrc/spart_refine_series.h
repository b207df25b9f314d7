// Refinement of time series of a pixel with a smoothness prior (spart_refine_series, include/spart_hip.h; the definition is
// tools/refine_series_defined.py and every function here reproduces it bit for bit): spart_refine_tiles with the tile read as a
// SERIES of rows (dates), and a first-difference penalty kappa_(m,b) = gamma_b link[m] between local b of rows m and m + 1.  The
// damped system of a series is block-tridiagonal with a border.  k_tiles_init / _cost / _normal / _apply are launched as they are.
//
// Part 1: the link weights, the chain's part of the cost and of the sums, one row of the chain elimination, the substitution
// along the chain and the std recurrence, SPART_HD so that g++ compiles them for tests/hostmath/refine_series_host.cpp.
// Strides as in spart_refine.h (element k at p[k * S]).  A row's packed vector is tiles' (R_m, W_m, d_m in the g slots once
// eliminated); X_m (Fl x Fl, entry (i, j) at i Fl + j) is the factor of the block between local i of row m and local j of row
// m - 1, present iff some kappa_(m-1, .) != 0.  Unknown order: row 0's locals, row 1's locals, ..., then the shared.
#pragma once

#include "spart_refine_tiles.h"

namespace spart {

#if defined(__clang__)
#define SPART_NO_UNROLL _Pragma("clang loop unroll(disable)")
#else
#define SPART_NO_UNROLL
#endif
constexpr int SERIES_MAXT = 256;             // rows per series: the std recurrence is quadratic in the length

// a link entry that is read: negative, NaN or infinite kills the series
SPART_HD bool series_bad_link(double v) { return !(v >= 0.0) || v == __builtin_inf(); }
SPART_HD double series_kappa(double gamma, double link) {
  SPART_NO_CONTRACT
  return gamma * link;
}
// is the block between two consecutive rows there?  link: the entry of the earlier row
SPART_HD bool series_present(int Fl, const double* gamma, double link) {
  bool p = false;
  for (int b = 0; b < Fl; ++b)
    if (series_kappa(gamma[b], link) != 0.0) p = true;
  return p;
}
// one tie of the cost: C + (kappa e) e with e = t_next - t_this; the caller skips kappa == 0
SPART_HD double series_chain_cost(double C, double k, double tn, double tc) {
  SPART_NO_CONTRACT
  const double e = tn - tc;
  return C + (k * e) * e;
}
// the chain's part of A_m[bb] and g_(m,b): the predecessor's tie first (kp, ep = t_m - t_(m-1)), then the successor's
// (kn, en = t_(m+1) - t_m); a tie that is not there is passed as kappa = 0
SPART_HD void series_augment(double* A, double* g, double kp, double ep, double kn, double en) {
  SPART_NO_CONTRACT
  if (kp != 0.0) {
    *A = *A + kp;
    *g = *g + kp * ep;
  }
  if (kn != 0.0) {
    *A = *A + kn;
    *g = *g - kn * en;
  }
}

// One row of the elimination, refine_cholesky's text over the present entries.  L: the row's (damped) packed vector, in place;
// Lq: the previous row's eliminated one (read only when pres); linkq: link of the previous row.  X out (when pres).  solve:
// also the forward substitution into the g slots.  false at a pivot !(s > 0).
SPART_HD bool series_chain_step(int F, int Fl, double* L, int S, const double* Lq, int SQ, bool pres, const double* gamma,
                                double linkq, double* X, int SX, bool solve) {
  SPART_NO_CONTRACT
  const int nt = refine_ntri(F);
  if (pres)
    SPART_NO_UNROLL
    for (int i = 0; i < Fl; ++i)
      SPART_NO_UNROLL
      for (int j = 0; j < Fl; ++j) {
        double s = i == j ? -series_kappa(gamma[j], linkq) : 0.0;
        SPART_NO_UNROLL
        for (int k = 0; k < j; ++k) s = s - X[(i * Fl + k) * SX] * Lq[refine_tri(j, k) * SQ];
        X[(i * Fl + j) * SX] = s / Lq[refine_tri(j, j) * SQ];
      }
  SPART_NO_UNROLL
  for (int i = 0; i < F; ++i) {
    const int jn = i + 1 < Fl ? i + 1 : Fl;
    SPART_NO_UNROLL
    for (int j = 0; j < jn; ++j) {
      double s = L[refine_tri(i, j) * S];
      if (pres) {
        if (i < Fl)
          SPART_NO_UNROLL
          for (int k = 0; k < Fl; ++k) s = s - X[(i * Fl + k) * SX] * X[(j * Fl + k) * SX];
        else
          SPART_NO_UNROLL
          for (int k = 0; k < Fl; ++k) s = s - Lq[refine_tri(i, k) * SQ] * X[(j * Fl + k) * SX];
      }
      SPART_NO_UNROLL
      for (int k = 0; k < j; ++k) s = s - L[refine_tri(i, k) * S] * L[refine_tri(j, k) * S];
      if (i == j) {
        if (!(s > 0.0)) return false;
        L[refine_tri(i, i) * S] = __builtin_sqrt(s);
      } else {
        L[refine_tri(i, j) * S] = s / L[refine_tri(j, j) * S];
      }
    }
  }
  if (solve)
    SPART_NO_UNROLL
    for (int j = 0; j < Fl; ++j) {
      double s = -L[(nt + j) * S];
      if (pres)
        SPART_NO_UNROLL
        for (int k = 0; k < Fl; ++k) s = s - X[(j * Fl + k) * SX] * Lq[(nt + k) * SQ];
      SPART_NO_UNROLL
      for (int k = 0; k < j; ++k) s = s - L[refine_tri(j, k) * S] * L[(nt + k) * S];
      L[(nt + j) * S] = s / L[refine_tri(j, j) * S];
    }
  return true;
}

// tiles' Schur sums of one eliminated row into the series' accumulators acc (Ps): entry e minus sum_k W[a, k] W[b, k], and with
// rhs entry nts + a minus sum_k W[a, k] d_k
SPART_HD void series_schur_row(int F, int Fs, int Fl, const double* L, int S, double* acc, int SA, bool rhs) {
  SPART_NO_CONTRACT
  const int n = refine_ntri(Fs) + (rhs ? Fs : 0);
  SPART_NO_UNROLL
  for (int e = 0; e < n; ++e) {
    int oa, ob;
    tiles_schur_offsets(e, F, Fs, Fl, &oa, &ob);
    double v = acc[e * SA];
    SPART_NO_UNROLL
    for (int k = 0; k < Fl; ++k) v = v - L[(oa + k) * S] * L[(ob + k) * S];
    acc[e * SA] = v;
  }
}

// tiles_shared_factor / _solve / _std on a strided packed vector (Ls then ds at ntri(Fs))
SPART_HD bool series_shared_factor(int Fs, double* Ls, int S) {
  SPART_NO_CONTRACT
  for (int a = 0; a < Fs; ++a)
    for (int b = 0; b <= a; ++b) {
      double s = Ls[refine_tri(a, b) * S];
      for (int k = 0; k < b; ++k) s = s - Ls[refine_tri(a, k) * S] * Ls[refine_tri(b, k) * S];
      if (a == b) {
        if (!(s > 0.0)) return false;
        Ls[refine_tri(a, a) * S] = __builtin_sqrt(s);
      } else {
        Ls[refine_tri(a, b) * S] = s / Ls[refine_tri(b, b) * S];
      }
    }
  return true;
}
SPART_HD bool series_shared_solve(int Fs, const double* Ls, double* ds, int S) {
  SPART_NO_CONTRACT
  for (int a = 0; a < Fs; ++a) {
    double s = ds[a * S];
    for (int k = 0; k < a; ++k) s = s - Ls[refine_tri(a, k) * S] * ds[k * S];
    ds[a * S] = s / Ls[refine_tri(a, a) * S];
  }
  for (int a = Fs - 1; a >= 0; --a) {
    double s = ds[a * S];
    for (int k = a + 1; k < Fs; ++k) s = s - Ls[refine_tri(k, a) * S] * ds[k * S];
    ds[a * S] = s / Ls[refine_tri(a, a) * S];
  }
  bool ok = true;
  for (int a = 0; a < Fs; ++a)
    if (!(ds[a * S] - ds[a * S] == 0.0)) ok = false;
  return ok;
}
SPART_HD double series_shared_std(int Fs, int f, const double* Ls, int S, double* z, int SZ) {
  SPART_NO_CONTRACT
  double var = 0.0;
  for (int k = f; k < Fs; ++k) {
    double s = k == f ? 1.0 : 0.0;
    for (int i = f; i < k; ++i) s = s - Ls[refine_tri(k, i) * S] * z[i * SZ];
    const double zk = s / Ls[refine_tri(k, k) * S];
    z[k * SZ] = zk;
    var = var + zk * zk;
  }
  return __builtin_sqrt(var);
}

// The back substitution of one row, j from Fl - 1 down: k = j + 1 .. Fl - 1 of the row, then the next row's i through
// Xn[i, j] (Xn NULL: no present block), then the shared a ascending; d in place in the g slots.  dn: the next row's delta.
SPART_HD void series_chain_back(int F, int Fs, int Fl, double* L, int S, const double* Xn, int SX, const double* dn, int SD,
                                const double* ds, int SS) {
  SPART_NO_CONTRACT
  const int nt = refine_ntri(F);
  for (int j = Fl - 1; j >= 0; --j) {
    double s = L[(nt + j) * S];
    for (int k = j + 1; k < Fl; ++k) s = s - L[refine_tri(k, j) * S] * L[(nt + k) * S];
    if (Xn)
      for (int i = 0; i < Fl; ++i) s = s - Xn[(i * Fl + j) * SX] * dn[i * SD];
    for (int a = 0; a < Fs; ++a) s = s - L[refine_tri(Fl + a, j) * S] * ds[a * SS];
    L[(nt + j) * S] = s / L[refine_tri(j, j) * S];
  }
}

// std of local j of a row: refine_std's recurrence over the row's locals >= j, every later row's locals and the shared, from the
// undamped factors.  `rows`: this row and the later ones of its series; row r's packed vector at L + r RL, its X at X + r RX
// (r >= 1), link[r] its tie to row r + 1 (link NULL: 1).  The shared right-hand sides are accumulated row by row in zs.
// za, zb (Fl) and zs (Fs) are scratch.
SPART_HD double series_local_std(int F, int Fs, int Fl, int j, int rows, const double* L, int64_t RL, int SL, const double* X,
                                 int64_t RX, int SX, const double* gamma, const double* link, const double* Ls, int SS, double* za,
                                 double* zb, double* zs, int SZ) {
  SPART_NO_CONTRACT
  double var = 0.0;
  double *zc = za, *zp = zb;
  for (int a = 0; a < Fs; ++a) zs[a * SZ] = 0.0;
  for (int r = 0; r < rows; ++r) {
    const double* Lr = L + r * RL;
    const double* Xr = X + r * RX;
    const bool pres = r > 0 && series_present(Fl, gamma, link ? link[r - 1] : 1.0);
    const int k0 = r == 0 ? j : 0, i0 = r == 1 ? j : 0;
    for (int k = k0; k < Fl; ++k) {
      double s = r == 0 && k == j ? 1.0 : 0.0;
      if (pres)
        for (int i = i0; i < Fl; ++i) s = s - Xr[(k * Fl + i) * SX] * zp[i * SZ];
      for (int i = k0; i < k; ++i) s = s - Lr[refine_tri(k, i) * SL] * zc[i * SZ];
      const double zk = s / Lr[refine_tri(k, k) * SL];
      zc[k * SZ] = zk;
      var = var + zk * zk;
    }
    for (int a = 0; a < Fs; ++a) {
      double s = zs[a * SZ];
      for (int i = k0; i < Fl; ++i) s = s - Lr[refine_tri(Fl + a, i) * SL] * zc[i * SZ];
      zs[a * SZ] = s;
    }
    double* sw = zc;
    zc = zp;
    zp = sw;
  }
  for (int a = 0; a < Fs; ++a) {
    double s = zs[a * SZ];
    for (int i = 0; i < a; ++i) s = s - Ls[refine_tri(a, i) * SS] * zs[i * SZ];
    const double zk = s / Ls[refine_tri(a, a) * SS];
    zs[a * SZ] = zk;
    var = var + zk * zk;
  }
  return __builtin_sqrt(var);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------------
// Part 2: the kernels.  The chunk state is tiles' (TilesState, "tile" = series; every row of a live series is live) plus Xp
// (Mc, Fl Fl), the factors of the link blocks, and gamma (Fl) on the device.  Per iteration, after the forward call:
// k_tiles_cost, k_series_decide (one thread per series: the ordered cost with the chain term, the decision), k_tiles_normal,
// k_series_augment (one thread per local of a row of an accepted series), k_series_sums (one thread per packed shared entry of
// an accepted series: S, gs in row order), k_series_factor (one lane per series, groups of W series through LDS at [e][o]: the
// walk along the chain with the forward substitution and the Schur sums in row order), k_series_shared (one thread per series:
// the shared factor and solve or, last, shared_std), k_series_back (the same walk backwards: delta_l) or, last, k_series_std (one thread per row), then k_tiles_apply.  No sum
// crosses lanes, so every order is the definition's whatever the launch shape; the failure flag of a series has one writer.
constexpr int SERIES_STD_THREADS = 64;

inline int series_group(int F) { return F <= 8 ? 8 : 4; }
inline size_t series_factor_lds(int F, int Fs, int W) {
  const int Fl = F - Fs, P = refine_ntri(F) + F, Ps = refine_ntri(Fs) + Fs;
  return (size_t)(2 * P + Fl * Fl + Ps) * (W + 1) * 8 + W * 8 + 3 * W * 4 + (size_t)(Fl + W) * 8;
}
inline size_t series_back_lds(int F, int Fs, int W) {
  const int Fl = F - Fs, P = refine_ntri(F) + F;
  return (size_t)(P + Fl * Fl + Fl + Fs) * (W + 1) * 8 + 3 * W * 4;
}
inline size_t series_std_lds(int F, int Fs) { return (size_t)(2 * (F - Fs) + Fs) * SERIES_STD_THREADS * 8; }

// One thread per series: C = 0; for m ascending: C = C + c_m; the chain term, m then b ascending on the trial locals; the
// shared prior; then tiles' decision.  it == 0 decides the dead series: any bad row (k_tiles_cost's live = 0, or a bad link entry
// that is read), a bad shared prior weight, or C not < +inf; its bad rows get status -1 and the others 1.
__global__ __launch_bounds__(256) void k_series_decide(const double* __restrict__ smu, const double* __restrict__ spw, int sper,
                                                       int Tc, int Fs, int Fl, int it, int last, const double* __restrict__ gamma,
                                                       const double* __restrict__ link, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tc) return;
  int na = s.na[t];
  if (it > 0 && na < 0) {
    s.code[t] = 0;
    return;
  }
  const int b0 = s.tstart[t], b1 = s.tstart[t + 1];
  double C = 0.0;
  bool bad = false;
  for (int m = b0; m < b1; ++m) {
    C = C + s.ct[m];
    if (it == 0 && !s.live[m]) bad = true;
  }
  for (int m = b0; m + 1 < b1; ++m) {
    const double lk = link ? link[m] : 1.0;
    if (it == 0 && series_bad_link(lk)) bad = true;
    for (int b = 0; b < Fl; ++b) {
      const double k = series_kappa(gamma[b], lk);
      if (k != 0.0) C = series_chain_cost(C, k, s.lt[(int64_t)(m + 1) * Fl + b], s.lt[(int64_t)m * Fl + b]);
    }
  }
  if (spw) {
    const int64_t pt = sper ? (int64_t)t * Fs : 0;
    C = refine_prior_total(Fs, C, &bad, s.zt + (int64_t)t * Fs, smu + pt, spw + pt);
  }
  int code;
  double lam = s.lam[t];
  if (it == 0) {
    code = (!bad && C < __builtin_inf()) ? 1 : 2;
    if (out.cost0) out.cost0[t] = C;
    if (code == 2) {
      na = -1;
      out.cost[t] = C;
      if (out.n_accept) out.n_accept[t] = -1;
      if (out.shared_std)
        for (int a = 0; a < Fs; ++a) out.shared_std[(int64_t)t * Fs + a] = __builtin_nan("");
      if (out.status)
        for (int m = b0; m < b1; ++m) {
          const bool badrow = !s.live[m] || (m + 1 < b1 && link && series_bad_link(link[m]));
          out.status[m] = badrow ? -1 : 1;
        }
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
}

// Behind k_tiles_normal, one thread per local b of a row of an accepted series: the chain's part of A_m[bb] and g_(m,b) at the
// accepted locals (s.lt is the trial that was just accepted)
__global__ __launch_bounds__(256) void k_series_augment(int Mc, int F, int Fs, const double* __restrict__ gamma,
                                                        const double* __restrict__ link, TilesState s) {
  SPART_NO_CONTRACT
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Mc * Fl) return;
  const int m = (int)(idx / Fl), b = (int)(idx % Fl);
  const int t = s.ptile[m];
  if (s.code[t] != 1) return;
  const int b0 = s.tstart[t], b1 = s.tstart[t + 1];
  const double tm = s.lt[(int64_t)m * Fl + b];
  double kp = 0.0, ep = 0.0, kn = 0.0, en = 0.0;
  if (m > b0) {
    kp = series_kappa(gamma[b], link ? link[m - 1] : 1.0);
    ep = tm - s.lt[(int64_t)(m - 1) * Fl + b];
  }
  if (m + 1 < b1) {
    kn = series_kappa(gamma[b], link ? link[m] : 1.0);
    en = s.lt[(int64_t)(m + 1) * Fl + b] - tm;
  }
  double* Am = s.Ap + (int64_t)m * P;
  double A = Am[refine_tri(b, b)], g = Am[nt + b];
  series_augment(&A, &g, kp, ep, kn, en);
  Am[refine_tri(b, b)] = A;
  Am[nt + b] = g;
}

// One thread per packed shared entry e of an accepted series: S_ab = 0; for m ascending: S_ab = S_ab + A_m[a, b]; gs likewise;
// then the shared prior -> St.  The loads of a step do not depend on the add chain.
__global__ __launch_bounds__(256) void k_series_sums(const double* __restrict__ smu, const double* __restrict__ spw, int sper,
                                                     int Tc, int F, int Fs, TilesState s, TilesOut out) {
  SPART_NO_CONTRACT
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)Tc * Ps) return;
  const int t = (int)(idx / Ps), e = (int)(idx % Ps);
  if (s.code[t] != 1) return;
  int a = e - nts, b = -1;
  if (e < nts) refine_pair(e, &a, &b);
  const int at = b >= 0 ? refine_tri(Fl + a, Fl + b) : nt + Fl + a;
  const int b0 = s.tstart[t], b1 = s.tstart[t + 1];
  double acc = 0.0;
  for (int m = b0; m < b1; ++m) acc = acc + s.Ap[(int64_t)m * P + at];
  if (spw && (b == a || b < 0)) {
    const int64_t pt = sper ? (int64_t)t * Fs : 0;
    const double p = spw[pt + a];
    if (p != 0.0) acc = b >= 0 ? acc + p : refine_prior_gain(acc, p, refine_residual(out.shared[(int64_t)t * Fs + a], smu[pt + a]));
  }
  s.St[idx] = acc;
}

// Groups of W series, one wave, lane o < W on series t0 + o.  Step r of the walk stages row r of every series of the group that
// has one (Ap -> LDS at [e][o], by all lanes, the local diagonal damped on the way unless last); lane o runs series_chain_step
// against the previous row's eliminated vector kept in the other LDS buffer and adds the row's Schur sums to its accumulators,
// which start from the damped S and -gs; all lanes write the row to Lp and X to Xp.  After the walk the accumulators go to Lt and
// a failed pivot sets the series' flag; k_series_shared finishes them.
template <int W>
__global__ __launch_bounds__(64) void k_series_factor(int Tc, int F, int Fs, int last, const double* __restrict__ gamma,
                                                      const double* __restrict__ link, TilesState s, double* __restrict__ Xp) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char series_smem[];
  constexpr int WP = W + 1;
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs, FF = Fl * Fl;
  double* buf0 = reinterpret_cast<double*>(series_smem);           // [e][o]
  double* buf1 = buf0 + P * WP;
  double* Xl = buf1 + P * WP;                                       // [i Fl + j][o]
  double* acc = Xl + FF * WP;                                       // [e][o]
  double* lml = acc + Ps * WP;                                      // [o]: lambda, 0 on the last call
  int* sb0 = reinterpret_cast<int*>(lml + W);                       // first row, rows (0: not this call's), per series of the group
  int* sln = sb0 + W;
  int* sfl = sln + W;                                               // Fl per lane: the recurrence's loop state stays in vector registers
  double* gl = reinterpret_cast<double*>(sfl + W);                  // gamma (Fl), then the staged row's link to its predecessor [o]
  double* lql = gl + Fl;
  const int lane = threadIdx.x, t0 = blockIdx.x * W;
  const int n = Tc - t0 < W ? Tc - t0 : W;
  if (lane < W) {
    int b0 = 0, ln = 0;
    double lam = 0.0;
    sfl[lane] = Fl;
    for (int b = lane; b < Fl; b += W) gl[b] = gamma[b];
    if (lane < n) {
      const int code = s.code[t0 + lane];
      b0 = s.tstart[t0 + lane];
      if (code == 1 || code == 3) ln = s.tstart[t0 + lane + 1] - b0;
      if (!last) lam = s.lam[t0 + lane];
    }
    sb0[lane] = b0;
    sln[lane] = ln;
    lml[lane] = lam;
  }
  __syncthreads();
  int maxlen = 0;
  for (int o = 0; o < n; ++o) maxlen = sln[o] > maxlen ? sln[o] : maxlen;
  if (maxlen == 0) return;                                         // (block-uniform)
  for (int i = lane; i < n * Ps; i += 64) {
    const int o = i / Ps, e = i % Ps;
    if (sln[o] == 0) continue;
    double v = s.St[(int64_t)(t0 + o) * Ps + e];
    if (e < nts) {
      int a, b;
      refine_pair(e, &a, &b);
      if (a == b && !last) v = v + lml[o] * (v > 0.0 ? v : 1.0);
    } else {
      v = -v;
    }
    acc[e * WP + o] = v;
  }
  for (int r = 0; r < maxlen; ++r) {                                // (a failed series is marked by sfl = -1: no lane mask lives across the walk)
    double* cur = r & 1 ? buf1 : buf0;
    const double* prev = r & 1 ? buf0 : buf1;
    for (int i = lane; i < n * P; i += 64) {
      const int o = i / P, e = i % P;
      if (r >= sln[o]) continue;
      if (e == 0) lql[o] = r > 0 ? (link ? link[sb0[o] + r - 1] : 1.0) : 0.0;
      double v = s.Ap[(int64_t)(sb0[o] + r) * P + e];
      if (!last && e < nt) {
        int a, b;
        refine_pair(e, &a, &b);
        if (a == b && a < Fl) v = v + lml[o] * (v > 0.0 ? v : 1.0);
      }
      cur[e * WP + o] = v;
    }
    __syncthreads();
    if (lane < n && r < sln[lane] && sfl[lane] > 0) {
      const int fl = sfl[lane];
      const double lq = lql[lane];
      const bool pres = r > 0 && series_present(fl, gl, lq);
      if (series_chain_step(Fs + fl, fl, cur + lane, WP, prev + lane, WP, pres, gl, lq, Xl + lane, WP, !last))
        series_schur_row(Fs + fl, Fs, fl, cur + lane, WP, acc + lane, WP, !last);
      else
        sfl[lane] = -1;
    }
    __syncthreads();
    for (int i = lane; i < n * P; i += 64) {
      const int o = i / P, e = i % P;
      if (r < sln[o]) s.Lp[(int64_t)(sb0[o] + r) * P + e] = cur[e * WP + o];
    }
    if (r > 0)
      for (int i = lane; i < n * FF; i += 64) {
        const int o = i / FF, e = i % FF;
        if (r < sln[o]) Xp[(int64_t)(sb0[o] + r) * FF + e] = Xl[e * WP + o];
      }
  }
  if (lane < n && sln[lane] > 0) s.flag[t0 + lane] = sfl[lane] > 0 ? 0 : 1;
  for (int i = lane; i < n * Ps; i += 64) {                        // (each lane reads what it wrote or what no lane changed since the barrier)
    const int o = i / Ps, e = i % Ps;
    if (sln[o]) s.Lt[(int64_t)(t0 + o) * Ps + e] = acc[e * WP + o];
  }
}

// One thread per series behind k_series_factor: the shared factor from the walked Schur sums in Lt, in place, then the shared
// solve or, last, shared_std (its z in LDS at [a][thread]); a failure sets the series' flag
__global__ __launch_bounds__(SERIES_STD_THREADS) void k_series_shared(int Tc, int Fs, int last, TilesState s,
                                                                      double* __restrict__ shared_std) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char series_smem[];
  double* z = reinterpret_cast<double*>(series_smem) + threadIdx.x;
  const int t = blockIdx.x * SERIES_STD_THREADS + threadIdx.x;
  if (t >= Tc) return;
  const int code = s.code[t];
  if (code != 1 && code != 3) return;
  const int nts = refine_ntri(Fs);
  double* sh = s.Lt + (int64_t)t * (nts + Fs);
  bool ok = s.flag[t] == 0;
  if (ok) ok = series_shared_factor(Fs, sh, 1);
  if (ok && !last) ok = series_shared_solve(Fs, sh, sh + nts, 1);
  if (!ok) s.flag[t] = 1;
  if (last && shared_std)
    for (int f = 0; f < Fs; ++f)
      shared_std[(int64_t)t * Fs + f] = ok ? series_shared_std(Fs, f, sh, 1, z, SERIES_STD_THREADS) : __builtin_nan("");
}

// The walk backwards, same groups: step r stages row r of Lp and X of row r + 1; lane o runs series_chain_back with the next
// row's delta (kept in LDS) and delta_s, checks the row's delta and keeps it for the next step; all lanes write the g slots back.
template <int W>
__global__ __launch_bounds__(64) void k_series_back(int Tc, int F, int Fs, const double* __restrict__ gamma,
                                                    const double* __restrict__ link, TilesState s, const double* __restrict__ Xp) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char series_smem[];
  constexpr int WP = W + 1;
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs, FF = Fl * Fl;
  double* cur = reinterpret_cast<double*>(series_smem);            // [e][o]
  double* Xl = cur + P * WP;
  double* dn = Xl + FF * WP;                                        // [j][o]
  double* ds = dn + Fl * WP;                                        // [a][o]
  int* sb0 = reinterpret_cast<int*>(ds + Fs * WP);
  int* sln = sb0 + W;
  const int lane = threadIdx.x, t0 = blockIdx.x * W;
  const int n = Tc - t0 < W ? Tc - t0 : W;
  if (lane < W) {
    int b0 = 0, ln = 0;
    if (lane < n) {
      const int code = s.code[t0 + lane];
      b0 = s.tstart[t0 + lane];
      if ((code == 1 || code == 3) && s.flag[t0 + lane] == 0) ln = s.tstart[t0 + lane + 1] - b0;
    }
    sb0[lane] = b0;
    sln[lane] = ln;
  }
  __syncthreads();
  int maxlen = 0;
  for (int o = 0; o < n; ++o) maxlen = sln[o] > maxlen ? sln[o] : maxlen;
  if (maxlen == 0) return;                                         // (block-uniform)
  for (int i = lane; i < n * Fs; i += 64) {
    const int o = i / Fs, a = i % Fs;
    if (sln[o]) ds[a * WP + o] = s.Lt[(int64_t)(t0 + o) * Ps + nts + a];
  }
  const bool mine = lane < n && sln[lane] > 0;
  bool fin = true;
  for (int r = maxlen - 1; r >= 0; --r) {
    __syncthreads();
    for (int i = lane; i < n * P; i += 64) {
      const int o = i / P, e = i % P;
      if (r < sln[o]) cur[e * WP + o] = s.Lp[(int64_t)(sb0[o] + r) * P + e];
    }
    for (int i = lane; i < n * FF; i += 64) {
      const int o = i / FF, e = i % FF;
      if (r + 1 < sln[o]) Xl[e * WP + o] = Xp[(int64_t)(sb0[o] + r + 1) * FF + e];
    }
    __syncthreads();
    if (mine && r < sln[lane]) {
      double* L = cur + lane;
      const bool pres = r + 1 < sln[lane] && series_present(Fl, gamma, link ? link[sb0[lane] + r] : 1.0);
      series_chain_back(F, Fs, Fl, L, WP, pres ? Xl + lane : nullptr, WP, dn + lane, WP, ds + lane, WP);
      for (int j = 0; j < Fl; ++j) {
        const double v = L[(nt + j) * WP];
        if (!(v - v == 0.0)) fin = false;
        dn[j * WP + lane] = v;
      }
    }
    __syncthreads();
    for (int i = lane; i < n * Fl; i += 64) {
      const int o = i / Fl, j = i % Fl;
      if (r < sln[o]) s.Lp[(int64_t)(sb0[o] + r) * P + nt + j] = cur[(nt + j) * WP + o];
    }
  }
  if (mine && !fin) s.flag[t0 + lane] = 2;
}

// Last call, one thread per row of a live series: local_std by series_local_std on the undamped factors in Lp / Xp / Lt, the
// recurrence's z in LDS at [k][lane]; NaN for the whole series under a raised flag
__global__ __launch_bounds__(SERIES_STD_THREADS) void k_series_std(int Mc, int F, int Fs, const double* __restrict__ gamma,
                                                                   const double* __restrict__ link, TilesState s,
                                                                   const double* __restrict__ Xp, double* __restrict__ local_std) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char series_smem[];
  constexpr int NT = SERIES_STD_THREADS;
  const int Fl = F - Fs, P = refine_ntri(F) + F, Ps = refine_ntri(Fs) + Fs, FF = Fl * Fl;
  double* za = reinterpret_cast<double*>(series_smem) + threadIdx.x;
  double* zb = za + Fl * NT;
  double* zs = zb + Fl * NT;
  const int m = blockIdx.x * NT + threadIdx.x;
  if (m >= Mc) return;
  const int t = s.ptile[m], code = s.code[t];
  if (code != 1 && code != 3) return;
  const bool ok = s.flag[t] == 0;
  const int rows = s.tstart[t + 1] - m;
  for (int j = 0; j < Fl; ++j)
    local_std[(int64_t)m * Fl + j] =
        ok ? series_local_std(F, Fs, Fl, j, rows, s.Lp + (int64_t)m * P, P, 1, Xp + (int64_t)m * FF, FF, 1, gamma,
                              link ? link + m : nullptr, s.Lt + (int64_t)t * Ps, 1, za, zb, zs, NT)
           : __builtin_nan("");
}
#endif  // __HIPCC__

}  // namespace spart
