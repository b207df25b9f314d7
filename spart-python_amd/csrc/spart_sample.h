// Ensemble MCMC sampling of the posterior of a fit (spart_sample, include/spart_hip.h; the definition is
// tools/sample_defined.py and every function here reproduces it bit for bit, exp apart).
//
// Part 1: the per-walker arithmetic -- Philox4x32-10, u53, the start point, the stretch, the in-box test, zp, the accept rule,
// one kept-step sum and the finish -- as plain functions under SPART_NO_CONTRACT (the best rule is the one comparison
// c_k < best_cost, written where it is used).  hipcc compiles them into the
// kernels of part 2 and g++ compiles them for tests/hostmath/sample_host.cpp.  Array arguments come with strides.
//
// Part 2: three kernels.  A chunk of Mc observations runs ALL its steps before the next chunk starts.  With H = W / 2, a
// half-step h moves the walkers k = h H + kk of every observation: table row r = m H + kk, R = Mc H rows.
//   k_sample_init   once per chunk: the fixed columns of the (27, R) table, x0, the start ensemble, the zeroed state;
//   k_sample_table  per half-step: the F free columns of the table -- the proposal y, or x_k where y leaves the box (and at the
//                   start, s = step0, x_k itself) -- with zp, u2 and the in-box flag of every row.  Philox runs here;
//   k_sample_step   per half-step, after the forward call: cost, decision, state, best, and on a kept step the chain rows and
//                   the sums, on the last one the outputs.
// State per chunk (workspace): x (Mc, W, F), c (Mc, W), x0, S, best_x (Mc, F), Q (Mc, F (F + 1) / 2), best_cost (Mc),
// n_accept (Mc) int64, dead (Mc) int32.
#pragma once

#include "spart_refine.h"    // REFINE_MAXF, REFINE_ROWS, refine_clip, refine_cost_band, refine_prior_cost, refine_bad_weight

namespace spart {

constexpr int SAMPLE_ROWS = REFINE_ROWS;               // rows of one forward call at most
constexpr int SAMPLE_MAX_STEPS = 1 << 20;

SPART_HD bool sample_walkers_ok(int W, int F) { return (W == 8 || W == 16 || W == 32 || W == 64) && W >= 2 * F; }
// observations per chunk
SPART_HD int64_t sample_chunk(int W) { return SAMPLE_ROWS / (W / 2); }
// keep number (from 0) of relative step rel = s - step0 >= 1, or -1
SPART_HD int64_t sample_keep(int64_t rel, int64_t burn, int64_t thin) {
  return rel > burn && (rel - burn) % thin == 0 ? (rel - burn) / thin - 1 : -1;
}

struct SampleBlock {
  uint32_t w0, w1, w2, w3;
};

// Philox4x32-10 (Salmon et al. 2011), integer only
SPART_HD SampleBlock sample_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  return {c0, c1, c2, c3};
}

// the block of (seed, global observation g, absolute step s, walker k, draw d)
SPART_HD SampleBlock sample_block(uint64_t seed, uint64_t g, uint64_t s, int k, int d) {
  return sample_philox((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)s, ((uint32_t)k << 8) | (uint32_t)d, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

// ((a >> 5) 2^26 + (b >> 6)) 2^-53: exact, in [0, 1)
SPART_HD double sample_u53(uint32_t a, uint32_t b) {
  SPART_NO_CONTRACT
  const double v = (double)(a >> 5) * 67108864.0 + (double)(b >> 6);
  return v * 1.1102230246251565e-16;
}

// a radius that kills its observation: not finite and > 0
SPART_HD bool sample_bad_radius(double r) { return !(r > 0.0) || r == __builtin_inf(); }

// lo <= y <= hi (a NaN is outside)
SPART_HD bool sample_in_box(double y, double lo, double hi) { return lo <= y && y <= hi; }

// one coordinate of the start ensemble: a = max(lo, x0 - r), b = min(hi, x0 + r), a + u (b - a)
SPART_HD double sample_start(double x0, double r, double lo, double hi, double u) {
  SPART_NO_CONTRACT
  const double m = x0 - r, p = x0 + r;
  const double a = m != m ? m : (lo > m ? lo : m);        // (numpy's maximum / minimum: a NaN stays)
  const double b = p != p ? p : (hi < p ? hi : p);
  const double w = b - a;
  return a + u * w;
}

// the draws of walker k = h W/2 + kk in half-step h of step s: z = ((a - 1) u1 + 1)^2 / a, u2, the partner j
SPART_HD void sample_draws(uint64_t seed, uint64_t g, uint64_t s, int h, int W, int k, double a, double* z, double* u2, int* j) {
  SPART_NO_CONTRACT
  const int H = W / 2;
  const SampleBlock b0 = sample_block(seed, g, s, k, 0), b1 = sample_block(seed, g, s, k, 1);
  const double u1 = sample_u53(b0.w0, b0.w1);
  *j = (1 - h) * H + (int)(b0.w2 % (uint32_t)H);
  *u2 = sample_u53(b1.w0, b1.w1);
  const double t = (a - 1.0) * u1 + 1.0;
  *z = (t * t) / a;
}

// y_f = x_jf + z (x_kf - x_jf)
SPART_HD double sample_stretch(double xj, double xk, double z) {
  SPART_NO_CONTRACT
  const double d = xk - xj;
  return xj + z * d;
}

// 1 multiplied by z F - 1 times
SPART_HD double sample_zp(double z, int F) {
  SPART_NO_CONTRACT
  double zp = 1.0;
  for (int i = 1; i < F; ++i) zp = zp * z;
  return zp;
}

// accept iff inside and u2 < q, q = zp exp(-((c' - c) / (2 T))); a NaN never accepts
SPART_HD bool sample_accept(bool inside, double u2, double zp, double cnew, double cold, double two_tau) {
  SPART_NO_CONTRACT
  const double q = zp * Mx<double>::exp_poly(-((cnew - cold) / two_tau));
  return inside && u2 < q;
}

// One entry of the kept-step sums over the W walkers of an observation, ascending: e = x_k - x0;  b >= 0: acc + e_a e_b,
// b < 0: acc + e_a.  x: the ensemble, walker k coordinate f at x[k SK + f SF].
SPART_HD double sample_sum(double acc, const double* x, int64_t SK, int64_t SF, int W, int a, int b, double x0a, double x0b) {
  SPART_NO_CONTRACT
  for (int k = 0; k < W; ++k) {
    const double ea = x[k * SK + a * SF] - x0a;
    if (b < 0) {
      acc = acc + ea;
    } else {
      const double eb = x[k * SK + b * SF] - x0b;
      acc = acc + ea * eb;
    }
  }
  return acc;
}

// mean_f = x0_f + S_f / n
SPART_HD double sample_mean(double x0, double S, double n) {
  SPART_NO_CONTRACT
  return x0 + S / n;
}

// cov_ab = Q_ab / n - (S_a / n) (S_b / n)
SPART_HD double sample_cov(double Q, double Sa, double Sb, double n) {
  SPART_NO_CONTRACT
  const double p = (Sa / n) * (Sb / n);
  return Q / n - p;
}

// refine_pair under the name this header gave it before the family shared one (host code written against that name compiles)
SPART_HD void sample_pair(int e, int* a, int* b) { refine_pair(e, a, b); }

#if defined(__HIPCC__)

constexpr int SAMPLE_JT = 16;                 // bands per LDS tile (128 B of a row)
static_assert(SAMPLE_JT == REFINE_JT, "refine_stage_obs stages tiles of REFINE_JT bands");
constexpr int SAMPLE_MAXOPW = 16;            // observations per wave at most: 64 / (W / 2) with W = 8

struct SampleCfg {
  const double* base[NPARAM];            // the caller's start columns (each (M,))
  const double* freebase[REFINE_MAXF];   // base[free[f]]
  int32_t is_free[NPARAM];
  int32_t free_col[REFINE_MAXF];
  double lo[REFINE_MAXF], hi[REFINE_MAXF];
};

struct SampleOut {                       // spart_sample_out, moved to the chunk's first observation
  double *mean, *cov, *std, *best_x, *best_cost;
  int64_t* n_accept;
  int32_t* status;
  double *chain, *chain_cost, *last, *last_cost;
};

// the state of a chunk and the per-row hand-over from k_sample_table to k_sample_step; `out`: the chunk's output pointers, left
// in the workspace by k_sample_init (k_sample_step reads each one where it needs it: its arguments stay within the SGPRs)
struct SampleState {
  double *x, *c, *x0, *S, *Q, *bx, *bc;
  int64_t* na;
  int32_t* dead;
  double *zp, *u2;
  int32_t *inside, *free_col;
  SampleOut* out;
};

// true in every lane of a group of H consecutive lanes (H divides 64) when c holds in any of them
__device__ __forceinline__ bool sample_group_any(bool c, int lane, int H) {
  const unsigned long long b = __builtin_amdgcn_ballot_w64(c);
  const unsigned long long mask = H == 64 ? ~0ull : ((1ull << H) - 1ull) << ((lane / H) * H);
  return (b & mask) != 0;
}

// Once per chunk (observations m0 ... m0 + Mc - 1 of the call): thread = table row (m, kk).  Every thread writes its row's fixed
// columns and the walkers kk and kk + H of its observation; the lane kk == 0 writes the per-observation state.  An observation
// that is dead already (radius, init) walks from x0, so that its rows stay valid.
__global__ __launch_bounds__(256) void k_sample_init(SampleCfg a, int64_t m0, int Mc, int F, int W, uint64_t seed, uint64_t g0,
                                                     uint64_t s0, double rel_init, const double* __restrict__ radius,
                                                     const double* __restrict__ init, double* __restrict__ table, SampleState st, SampleOut out) {
  SPART_NO_CONTRACT
  const int H = W / 2, nt = refine_ntri(F);
  const int64_t R = (int64_t)Mc * H;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = row < R;
  const int m = valid ? (int)(row / H) : 0, kk = valid ? (int)(row % H) : 0;
  if (blockIdx.x == 0) {
#pragma unroll
    for (int f = 0; f < REFINE_MAXF; ++f)
      if ((int)threadIdx.x == f) st.free_col[f] = a.free_col[f];
    if (threadIdx.x == 0) *st.out = out;
  }
  if (valid) {
#pragma unroll
    for (int p = 0; p < NPARAM; ++p)
      if (!a.is_free[p]) table[p * R + row] = a.base[p][m0 + m];
  }
  // pass 1: is the observation dead already?
  bool bad = false;
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F || !valid) continue;
    const double r = radius ? radius[(m0 + m) * F + f] : rel_init * (a.hi[f] - a.lo[f]);
    if (sample_bad_radius(r)) bad = true;
    if (init)
      for (int t = 0; t < 2; ++t)
        if (!sample_in_box(init[((m0 + m) * W + kk + t * H) * F + f], a.lo[f], a.hi[f])) bad = true;
  }
  bad = sample_group_any(bad, threadIdx.x & 63, H);
  if (!valid) return;
  // pass 2: x0 and the two walkers
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    const double x0 = refine_clip(a.freebase[f][m0 + m], a.lo[f], a.hi[f]);
    const double r = radius ? radius[(m0 + m) * F + f] : rel_init * (a.hi[f] - a.lo[f]);
    for (int t = 0; t < 2; ++t) {
      const int k = kk + t * H;
      double v = x0;
      if (!bad) {
        if (init) {
          v = init[((m0 + m) * W + k) * F + f];
        } else {
          const SampleBlock b = sample_block(seed, g0 + (uint64_t)m, s0, k, f);
          v = sample_start(x0, r, a.lo[f], a.hi[f], sample_u53(b.w0, b.w1));
        }
      }
      st.x[((int64_t)m * W + k) * F + f] = v;
    }
    if (kk == 0) {
      st.x0[(int64_t)m * F + f] = x0;
      st.S[(int64_t)m * F + f] = 0.0;
      st.bx[(int64_t)m * F + f] = __builtin_nan("");
    }
  }
  for (int e = kk; e < nt; e += H) st.Q[(int64_t)m * nt + e] = 0.0;
  if (kk == 0) {
    st.bc[m] = __builtin_inf();
    st.na[m] = 0;
    st.dead[m] = bad ? 1 : 0;
  }
}

// Per half-step h of absolute step s: thread = table row.  start: the rows are the walkers themselves.
__global__ __launch_bounds__(256) void k_sample_table(SampleCfg a, int Mc, int F, int W, int h, int start, uint64_t seed, uint64_t g0,
                                                      uint64_t s, double stretch, double* __restrict__ table, SampleState st) {
  SPART_NO_CONTRACT
  const int H = W / 2;
  const int64_t R = (int64_t)Mc * H;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= R) return;
  const int m = (int)(row / H), k = h * H + (int)(row % H);
  const double* xm = st.x + (int64_t)m * W * F;
  const double* xk = xm + (int64_t)k * F;
  double z = 1.0, u2 = 0.0;
  int j = k;
  bool inside = true;
  if (!start) {
    sample_draws(seed, g0 + (uint64_t)m, s, h, W, k, stretch, &z, &u2, &j);
    const double* xj = xm + (int64_t)j * F;
#pragma unroll
    for (int f = 0; f < REFINE_MAXF; ++f) {
      if (f >= F) continue;
      if (!sample_in_box(sample_stretch(xj[f], xk[f], z), a.lo[f], a.hi[f])) inside = false;
    }
  }
  const double* xj = xm + (int64_t)j * F;
#pragma unroll
  for (int f = 0; f < REFINE_MAXF; ++f) {
    if (f >= F) continue;
    table[a.free_col[f] * R + row] = (start || !inside) ? xk[f] : sample_stretch(xj[f], xk[f], z);
  }
  st.zp[row] = sample_zp(z, F);
  st.u2[row] = u2;
  st.inside[row] = inside ? 1 : 0;
}

struct SampleStep {
  const double *cols, *obs, *wts, *pmu, *ppw, *table;     // obs / wts / pmu / ppw: the chunk's rows (or the shared row)
  int Mc, F, nb, W, h, start, last, wper, pper;
  int64_t keep, n_keep;                                    // keep number of this step (-1: not kept)
  double two_tau, n;                                       // 2 T; (double)(n_keep W)
  SampleState st;
};

// Per half-step, after the forward call of its table: single-wave workgroups, lane = table row, so the H walkers of an
// observation sit in adjacent lanes and a wave holds 64 / H whole observations.  The 64 rows of a wave are ONE contiguous run of
// 64 nb doubles of `cols`: a tile of SAMPLE_JT bands goes through LDS with band-contiguous lanes and is read one row per lane
// (row stride 65 doubles); the weights and the observed values of the wave's observations beside it.
//   cost      lane: its row's cost, bands ascending, then the prior's terms;
//   decision  lane: accept or not; an accepted walker's x and c become the state;
//   best      the group's smallest cost, lowest k first, against best_cost;
//   kept      (h == 1) the chain rows, and the F (F + 1) / 2 + F sums of an observation dealt to its H lanes, each sequential in k;
//   finish    (last, h == 1) the outputs, dealt the same way.
__global__ __launch_bounds__(64) void k_sample_step(SampleStep p) {
  SPART_NO_CONTRACT
  constexpr int JT = SAMPLE_JT, YP = 65, OP = SAMPLE_MAXOPW + 1;
  __shared__ double Yl[JT * YP];           // [jj][lane]
  __shared__ double wl[JT * OP];           // [jj][o] weights (0: skip the band)
  __shared__ double ol[JT * OP];           // [jj][o] obs
  const SampleState& st = p.st;
  const SampleOut* __restrict__ out = st.out;
  const int F = p.F, nb = p.nb, W = p.W, H = W / 2, nt = refine_ntri(F), OPW = 64 / H;
  const int lane = threadIdx.x;
  const int64_t R = (int64_t)p.Mc * H;
  const int64_t row0 = (int64_t)blockIdx.x * 64, row = row0 + lane;
  const bool valid = row < R;
  const int o = lane / H, kk = lane % H, k = p.h * H + kk;
  const int mf = (int)(row0 / H);                       // first observation of the wave
  const int m = valid ? mf + o : mf;
  const double* cols_g = p.cols + row0 * nb;
  const double* obs_g = p.obs + (int64_t)mf * nb;
  const double* wts_g = p.wts ? (p.wper ? p.wts + (int64_t)mf * nb : p.wts) : nullptr;

  // ---- cost
  double ct = 0.0;
  bool bad = false;
  for (int j0 = 0; j0 < nb; j0 += JT) {
    __syncthreads();
    refine_stage_obs(lane, OPW, OP, p.Mc - mf, j0, nb, nb, obs_g, wts_g, p.wper, [](int j) { return j; }, wl, ol);
    for (int i = lane; i < 64 * JT; i += 64) {
      const int jj = i % JT, rr = i / JT, j = j0 + jj;
      Yl[jj * YP + rr] = (row0 + rr < R && j < nb) ? cols_g[(int64_t)rr * nb + j] : 0.0;
    }
    __syncthreads();
    if (valid) ct = refine_tile_cost(ct, &bad, JT, wl + o, OP, Yl + lane, YP, ol + o, OP);
  }
  const int64_t xat = ((int64_t)m * W + k) * F;          // this lane's walker in the state
  if (p.ppw && valid) {
    const int64_t pm = p.pper ? (int64_t)m * F : 0;
    const double* table = p.table;
    const int32_t* free_col = st.free_col;
    ct = refine_prior_total_of(F, ct, &bad, [=](int f) { return table[free_col[f] * R + row]; }, p.pmu + pm, p.ppw + pm);
  }

  // ---- decision
  bool dead = false, acc = false;
  double ck = __builtin_nan("");
  if (p.start) {
    if (valid) st.c[(int64_t)m * W + k] = ct;
    ck = ct;
    if (p.h == 1) {                                      // every start cost is known: is the observation dead?
      bool d = false;
      if (valid) d = bad || st.dead[m] != 0 || !(ct - ct == 0.0) || !(st.c[(int64_t)m * W + kk] - st.c[(int64_t)m * W + kk] == 0.0);
      dead = sample_group_any(d, lane, H);
      if (valid && kk == 0) st.dead[m] = dead ? 1 : 0;
    }
  } else if (valid) {
    dead = st.dead[m] != 0;
    const double cold = st.c[(int64_t)m * W + k];
    acc = !dead && sample_accept(st.inside[row] != 0, st.u2[row], st.zp[row], ct, cold, p.two_tau);
    ck = acc ? ct : cold;
    if (acc) {
      st.c[(int64_t)m * W + k] = ct;
      for (int f = 0; f < F; ++f) st.x[xat + f] = p.table[st.free_col[f] * R + row];
    }
  }
  if (!p.start) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(acc);
    const unsigned long long mask = H == 64 ? ~0ull : ((1ull << H) - 1ull) << (o * H);
    if (valid && kk == 0) st.na[m] += (int64_t)__builtin_popcountll(b & mask);
  }

  // ---- best: the smallest cost of the half, the lowest k among equals
  {
    double bcst = (valid && ck == ck) ? ck : __builtin_inf();
    int bk = kk;
    for (int s = H / 2; s >= 1; s >>= 1) {
      const double oc = __shfl_xor(bcst, s, 64);
      const int ok = __shfl_xor(bk, s, 64);
      if (oc < bcst || (oc == bcst && ok < bk)) {
        bcst = oc;
        bk = ok;
      }
    }
    if (valid && bk == kk && bcst < st.bc[m]) {
      st.bc[m] = bcst;
      for (int f = 0; f < F; ++f) st.bx[(int64_t)m * F + f] = st.x[xat + f];
    }
  }

  // ---- the chain rows of a kept step and the final ensemble: every lane its own walker
  const double nan = __builtin_nan("");
  if (valid && p.keep >= 0) {
    const int64_t at = ((int64_t)m * p.n_keep + p.keep) * W + k;
    if (out->chain)
      for (int f = 0; f < F; ++f) out->chain[at * F + f] = dead ? nan : st.x[xat + f];
    if (out->chain_cost) out->chain_cost[at] = dead ? nan : ck;
  }
  if (valid && p.last) {
    if (out->last)
      for (int f = 0; f < F; ++f) out->last[xat + f] = dead ? nan : st.x[xat + f];
    if (out->last_cost) out->last_cost[(int64_t)m * W + k] = dead ? nan : ck;
  }
  if (p.h == 0 || (p.keep < 0 && !p.last)) return;         // (kernel-uniform)

  // ---- the sums of a kept step: entry e of the observation to lane e % H
  __syncthreads();
  if (valid && p.keep >= 0)
    for (int e = kk; e < nt + F; e += H) {
      int a, b = -1;
      if (e < nt) refine_pair(e, &a, &b);
      else a = e - nt;
      double* acc_at = e < nt ? st.Q + (int64_t)m * nt + e : st.S + (int64_t)m * F + a;
      *acc_at = sample_sum(*acc_at, st.x + (int64_t)m * W * F, F, 1, W, a, b, st.x0[(int64_t)m * F + a],
                           st.x0[(int64_t)m * F + (b < 0 ? a : b)]);
    }
  if (!p.last) return;

  // ---- finish
  __syncthreads();
  if (!valid) return;
  for (int e = kk; e < nt + F; e += H) {
    if (e < nt) {
      int a, b;
      refine_pair(e, &a, &b);
      const double v = dead ? nan : sample_cov(st.Q[(int64_t)m * nt + e], st.S[(int64_t)m * F + a], st.S[(int64_t)m * F + b], p.n);
      if (out->cov) {
        out->cov[((int64_t)m * F + a) * F + b] = v;
        out->cov[((int64_t)m * F + b) * F + a] = v;
      }
      if (a == b && out->std) out->std[(int64_t)m * F + a] = __builtin_sqrt(v);
    } else {
      const int f = e - nt;
      if (out->mean) out->mean[(int64_t)m * F + f] = dead ? nan : sample_mean(st.x0[(int64_t)m * F + f], st.S[(int64_t)m * F + f], p.n);
      if (out->best_x) out->best_x[(int64_t)m * F + f] = dead ? nan : st.bx[(int64_t)m * F + f];
    }
  }
  if (kk == 0) {
    if (out->best_cost) out->best_cost[m] = dead ? nan : st.bc[m];
    if (out->n_accept) out->n_accept[m] = dead ? -1 : st.na[m];
    if (out->status) out->status[m] = dead ? -1 : 0;
  }
}

#endif  // __HIPCC__

}  // namespace spart
