// TEST INFRASTRUCTURE ONLY (tests/test_sample_host.py): part 1 of csrc/spart_sample.h -- Philox, u53, the start point, the
// stretch, the in-box test, zp, the accept rule, the best rule, the sums and the finish -- and a whole run built from them the
// way the kernels build it (sph_init, then per half-step sph_table, the caller's forward model, sph_step), for a g++ build with
// -ffp-contract=off.  `S` spreads every element of the state (x, c, the sums), so that a wrong stride shows.  With
// -DSAMPLE_MAIN the file is a stand-alone program (heap buffers of exact size) for -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../spart-python_amd/csrc/spart_sample.h"

using namespace spart;

extern "C" {

struct SphState {          // element i of x, c, sum, Q at [i S]; the others dense
  int64_t S;
  double *x, *c, *sum, *Q; // (M, W, F), (M, W), (M, F), (M, F (F + 1) / 2)
  double *x0, *bx, *bc;    // (M, F), (M, F), (M,)
  int64_t* na;             // (M,)
  int32_t* dead;           // (M,)
  double *zp, *u2;         // (M H,)
  int32_t* inside;         // (M H,)
};

struct SphOut {            // spart_sample_out
  double *mean, *cov, *std, *best_x, *best_cost;
  int64_t* n_accept;
  int32_t* status;
  double *chain, *chain_cost, *last, *last_cost;
};

void sph_philox(const uint32_t* c, const uint32_t* k, uint32_t* out) {
  const SampleBlock b = sample_philox(c[0], c[1], c[2], c[3], k[0], k[1]);
  out[0] = b.w0, out[1] = b.w1, out[2] = b.w2, out[3] = b.w3;
}
double sph_u53(uint32_t a, uint32_t b) { return sample_u53(a, b); }
int sph_walkers_ok(int W, int F) { return sample_walkers_ok(W, F) ? 1 : 0; }
int64_t sph_chunk(int W) { return sample_chunk(W); }
int64_t sph_keep(int64_t rel, int64_t burn, int64_t thin) { return sample_keep(rel, burn, thin); }

// k_sample_init: basefree (M, F) the start rows' free columns; radius (M, F) or NULL; init (M, W, F) or NULL
void sph_init(int M, int F, int W, uint64_t seed, uint64_t g0, uint64_t s0, double rel_init, const double* basefree, const double* lo,
              const double* hi, const double* radius, const double* init, SphState* st) {
  const int nt = refine_ntri(F);
  const int64_t S = st->S;
  for (int m = 0; m < M; ++m) {
    bool bad = false;
    for (int f = 0; f < F; ++f) {
      const double r = radius ? radius[(int64_t)m * F + f] : rel_init * (hi[f] - lo[f]);
      if (sample_bad_radius(r)) bad = true;
      if (init)
        for (int k = 0; k < W; ++k)
          if (!sample_in_box(init[((int64_t)m * W + k) * F + f], lo[f], hi[f])) bad = true;
    }
    for (int f = 0; f < F; ++f) {
      const double x0 = refine_clip(basefree[(int64_t)m * F + f], lo[f], hi[f]);
      const double r = radius ? radius[(int64_t)m * F + f] : rel_init * (hi[f] - lo[f]);
      for (int k = 0; k < W; ++k) {
        double v = x0;
        if (!bad) {
          if (init) {
            v = init[((int64_t)m * W + k) * F + f];
          } else {
            const SampleBlock b = sample_block(seed, g0 + (uint64_t)m, s0, k, f);
            v = sample_start(x0, r, lo[f], hi[f], sample_u53(b.w0, b.w1));
          }
        }
        st->x[(((int64_t)m * W + k) * F + f) * S] = v;
      }
      st->x0[(int64_t)m * F + f] = x0;
      st->sum[((int64_t)m * F + f) * S] = 0.0;
      st->bx[(int64_t)m * F + f] = __builtin_nan("");
    }
    for (int e = 0; e < nt; ++e) st->Q[((int64_t)m * nt + e) * S] = 0.0;
    st->bc[m] = __builtin_inf();
    st->na[m] = 0;
    st->dead[m] = bad ? 1 : 0;
  }
}

// k_sample_table: the free columns of the M H rows of half-step h -> rows (M H, F)
void sph_table(int M, int F, int W, int h, int start, uint64_t seed, uint64_t g0, uint64_t s, double a, const double* lo,
               const double* hi, SphState* st, double* rows) {
  const int H = W / 2;
  const int64_t S = st->S;
  for (int64_t row = 0; row < (int64_t)M * H; ++row) {
    const int m = (int)(row / H), k = h * H + (int)(row % H);
    const double* xm = st->x + (int64_t)m * W * F * S;
    const double* xk = xm + (int64_t)k * F * S;
    double z = 1.0, u2 = 0.0;
    int j = k;
    bool inside = true;
    if (!start) {
      sample_draws(seed, g0 + (uint64_t)m, s, h, W, k, a, &z, &u2, &j);
      for (int f = 0; f < F; ++f)
        if (!sample_in_box(sample_stretch(xm[((int64_t)j * F + f) * S], xk[f * S], z), lo[f], hi[f])) inside = false;
    }
    for (int f = 0; f < F; ++f)
      rows[row * F + f] = (start || !inside) ? xk[f * S] : sample_stretch(xm[((int64_t)j * F + f) * S], xk[f * S], z);
    st->zp[row] = sample_zp(z, F);
    st->u2[row] = u2;
    st->inside[row] = inside ? 1 : 0;
  }
}

// k_sample_step: Y (M H, nb) the forward model of `rows` (M H, F)
void sph_step(int M, int F, int nb, int W, int h, int start, int last, int64_t keep, int64_t n_keep, double two_tau, double n,
              const double* Y, const double* rows, const double* obs, const double* wts, int wper, const double* pmu,
              const double* ppw, int pper, SphState* st, const SphOut* out) {
  const int H = W / 2, nt = refine_ntri(F);
  const int64_t S = st->S;
  const double nan = __builtin_nan("");
  for (int m = 0; m < M; ++m) {
    bool anybad = false;
    std::vector<double> ck(H);
    const bool was_dead = st->dead[m] != 0;
    int nacc = 0;
    for (int kk = 0; kk < H; ++kk) {
      const int64_t row = (int64_t)m * H + kk;
      const int k = h * H + kk;
      const double one = 1.0;                                  // (no weights: every band reads this one, stride 0)
      const double* w = wts ? wts + (wper ? (int64_t)m * nb : 0) : &one;
      double ct = refine_tile_cost(0.0, &anybad, nb, w, wts ? 1 : 0, Y + row * nb, 1, obs + (int64_t)m * nb, 1);
      if (ppw) {
        const int64_t pm = pper ? (int64_t)m * F : 0;
        ct = refine_prior_total(F, ct, &anybad, rows + row * F, pmu + pm, ppw + pm);
      }
      double* c_at = st->c + ((int64_t)m * W + k) * S;
      if (start) {
        *c_at = ct;
        ck[kk] = ct;
      } else {
        const bool acc = !was_dead && sample_accept(st->inside[row] != 0, st->u2[row], st->zp[row], ct, *c_at, two_tau);
        ck[kk] = acc ? ct : *c_at;
        if (acc) {
          *c_at = ct;
          for (int f = 0; f < F; ++f) st->x[(((int64_t)m * W + k) * F + f) * S] = rows[row * F + f];
          ++nacc;
        }
      }
    }
    bool dead = was_dead;
    if (start) {
      dead = false;
      if (h == 1) {
        dead = anybad || was_dead;
        for (int k = 0; k < W; ++k) {
          const double c = st->c[((int64_t)m * W + k) * S];
          if (!(c - c == 0.0)) dead = true;
        }
        st->dead[m] = dead ? 1 : 0;
      }
    } else {
      st->na[m] += nacc;
    }
    for (int kk = 0; kk < H; ++kk)                            // best: k ascending, strictly smaller
      if (ck[kk] < st->bc[m]) {
        st->bc[m] = ck[kk];
        for (int f = 0; f < F; ++f) st->bx[(int64_t)m * F + f] = st->x[(((int64_t)m * W + h * H + kk) * F + f) * S];
      }
    for (int kk = 0; kk < H; ++kk) {
      const int k = h * H + kk;
      const int64_t xat = ((int64_t)m * W + k) * F;
      if (keep >= 0) {
        const int64_t at = ((int64_t)m * n_keep + keep) * W + k;
        if (out->chain)
          for (int f = 0; f < F; ++f) out->chain[at * F + f] = dead ? nan : st->x[(xat + f) * S];
        if (out->chain_cost) out->chain_cost[at] = dead ? nan : ck[kk];
      }
      if (last) {
        if (out->last)
          for (int f = 0; f < F; ++f) out->last[xat + f] = dead ? nan : st->x[(xat + f) * S];
        if (out->last_cost) out->last_cost[(int64_t)m * W + k] = dead ? nan : ck[kk];
      }
    }
    if (h == 0 || (keep < 0 && !last)) continue;
    if (keep >= 0)
      for (int e = 0; e < nt + F; ++e) {
        int a, b = -1;
        if (e < nt) refine_pair(e, &a, &b);
        else a = e - nt;
        double* acc_at = e < nt ? st->Q + ((int64_t)m * nt + e) * S : st->sum + ((int64_t)m * F + a) * S;
        *acc_at = sample_sum(*acc_at, st->x + (int64_t)m * W * F * S, F * S, S, W, a, b, st->x0[(int64_t)m * F + a],
                             st->x0[(int64_t)m * F + (b < 0 ? a : b)]);
      }
    if (!last) continue;
    for (int e = 0; e < nt + F; ++e) {
      if (e < nt) {
        int a, b;
        refine_pair(e, &a, &b);
        const double v = dead ? nan : sample_cov(st->Q[((int64_t)m * nt + e) * S], st->sum[((int64_t)m * F + a) * S],
                                                 st->sum[((int64_t)m * F + b) * S], n);
        if (out->cov) out->cov[((int64_t)m * F + a) * F + b] = v, out->cov[((int64_t)m * F + b) * F + a] = v;
        if (a == b && out->std) out->std[(int64_t)m * F + a] = __builtin_sqrt(v);
      } else {
        const int f = e - nt;
        if (out->mean) out->mean[(int64_t)m * F + f] = dead ? nan : sample_mean(st->x0[(int64_t)m * F + f], st->sum[((int64_t)m * F + f) * S], n);
        if (out->best_x) out->best_x[(int64_t)m * F + f] = dead ? nan : st->bx[(int64_t)m * F + f];
      }
    }
    if (out->best_cost) out->best_cost[m] = dead ? nan : st->bc[m];
    if (out->n_accept) out->n_accept[m] = dead ? -1 : st->na[m];
    if (out->status) out->status[m] = dead ? -1 : 0;
  }
}

}  // extern "C"

#ifdef SAMPLE_MAIN
// every (F, W) of the test at two strides on heap buffers of exact size, with a linear forward model y = A x: the strided run
// must give the dense run's bits, some proposals must be accepted and some rejected, and a planted bad weight must kill its row
int main() {
  const int nb = 5, M = 3, n_steps = 12, burn = 4, thin = 2;
  const int64_t n_keep = (n_steps - burn) / thin;
  const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0};
  uint32_t w[4];
  sph_philox(c0, k0, w);
  if (w[0] != 0x6627e8d5u || w[3] != 0x9b00dbd8u || sph_u53(0, 0) != 0.0 || sph_u53(~0u, ~0u) != 1.0 - 1.1102230246251565e-16) {
    std::printf("philox WRONG\n");
    return 1;
  }
  for (int F : {1, 2, 6, 16})
    for (int W : {8, 16, 32, 64}) {
      if (W < 2 * F) continue;
      const int H = W / 2, nt = F * (F + 1) / 2;
      std::vector<double> out[2][9];
      std::vector<int64_t> na[2];
      std::vector<int32_t> status[2];
      for (int run = 0; run < 2; ++run) {
        const int64_t S = run ? 3 : 1;
        std::vector<double> lo(F, 0.0), hi(F, 1.0), basefree((size_t)M * F), A((size_t)nb * F), obs((size_t)M * nb), wts((size_t)M * nb, 400.0);
        for (int f = 0; f < F; ++f)
          for (int m = 0; m < M; ++m) basefree[(size_t)m * F + f] = 0.05 + 0.3 * m + 0.01 * f;      // (m = 0 near lo, m = 2 near hi)
        for (int j = 0; j < nb; ++j)
          for (int f = 0; f < F; ++f) A[(size_t)j * F + f] = ((j * 7 + f * 3) % 11) / 11.0 + (j % F == f ? 1.0 : 0.0);
        for (int m = 0; m < M; ++m)
          for (int j = 0; j < nb; ++j) {
            double y = 0.0;
            for (int f = 0; f < F; ++f) y += A[(size_t)j * F + f] * basefree[(size_t)m * F + f];
            obs[(size_t)m * nb + j] = y;
          }
        wts[(size_t)1 * nb + 2] = -1.0;                                                             // observation 1 is dead
        auto sized = [&](size_t n) { return std::vector<double>(n ? (n - 1) * S + 1 : 0); };
        std::vector<double> x = sized((size_t)M * W * F), c = sized((size_t)M * W), sum = sized((size_t)M * F), Q = sized((size_t)M * nt);
        std::vector<double> x0((size_t)M * F), bx((size_t)M * F), bc(M), zp((size_t)M * H), u2((size_t)M * H);
        std::vector<int64_t> nacc(M);
        std::vector<int32_t> dead(M), inside((size_t)M * H);
        SphState st = {S, x.data(), c.data(), sum.data(), Q.data(), x0.data(), bx.data(), bc.data(), nacc.data(), dead.data(),
                       zp.data(), u2.data(), inside.data()};
        const size_t sizes[9] = {(size_t)M * F, (size_t)M * F * F, (size_t)M * F, (size_t)M * F, (size_t)M,
                                 (size_t)M * n_keep * W * F, (size_t)M * n_keep * W, (size_t)M * W * F, (size_t)M * W};
        for (int i = 0; i < 9; ++i) out[run][i].assign(sizes[i], -7.0);
        na[run].assign(M, -7), status[run].assign(M, -7);
        SphOut o = {out[run][0].data(), out[run][1].data(), out[run][2].data(), out[run][3].data(), out[run][4].data(), na[run].data(),
                    status[run].data(), out[run][5].data(), out[run][6].data(), out[run][7].data(), out[run][8].data()};
        sph_init(M, F, W, 42, 7, 0, 0.02, basefree.data(), lo.data(), hi.data(), nullptr, nullptr, &st);
        std::vector<double> rows((size_t)M * H * F), Y((size_t)M * H * nb);
        for (int rel = 0; rel <= n_steps; ++rel)
          for (int h = 0; h < 2; ++h) {
            sph_table(M, F, W, h, rel == 0, 42, 7, (uint64_t)rel, 2.0, lo.data(), hi.data(), &st, rows.data());
            for (size_t r = 0; r < (size_t)M * H; ++r)
              for (int j = 0; j < nb; ++j) {
                double y = 0.0;
                for (int f = 0; f < F; ++f) y += A[(size_t)j * F + f] * rows[r * F + f];
                Y[r * nb + j] = y;
              }
            sph_step(M, F, nb, W, h, rel == 0, rel == n_steps, rel == 0 ? -1 : sph_keep(rel, burn, thin), n_keep, 2.0,
                     (double)(n_keep * W), Y.data(), rows.data(), obs.data(), wts.data(), 1, nullptr, nullptr, 0, &st, &o);
          }
      }
      bool ok = true;
      for (int i = 0; i < 9; ++i) ok = ok && std::memcmp(out[0][i].data(), out[1][i].data(), out[0][i].size() * 8) == 0;
      ok = ok && na[0] == na[1] && status[0] == status[1];
      ok = ok && status[0][0] == 0 && status[0][1] == -1 && status[0][2] == 0 && na[0][1] == -1;
      ok = ok && na[0][0] > 0 && na[0][0] < (int64_t)W * n_steps;
      ok = ok && out[0][0][(size_t)1 * F] != out[0][0][(size_t)1 * F] && out[0][2][0] > 0.0;
      std::printf("F %d W %d%s\n", F, W, ok ? " ok" : " WRONG");
      if (!ok) return 1;
    }
  return 0;
}
#endif
