// TEST INFRASTRUCTURE ONLY (tests/test_refine_prior_host.py): the prior's part of spart_refine's per-observation arithmetic
// (csrc/spart_refine.h: refine_prior_cost, refine_prior_gain) beside the step functions of refine_host.cpp, for a g++ build
// with -ffp-contract=off, one observation per call, every array dense.  With -DREFINE_PRIOR_MAIN the file is a stand-alone
// program: the whole loop with priors on a toy forward model, every buffer on the heap at its exact size, for a
// -fsanitize=address,undefined build that is run as a child process.
#include "refine_host.cpp"

extern "C" {

// the prior's terms of the trial cost of one observation, after the bands: f ascending, weight 0 skipped; *bad as rh_cost's
double rp_prior_cost(int F, double c, const double* t, const double* mu, const double* p, int32_t* bad) {
  bool b = false;
  c = refine_prior_total(F, c, &b, t, mu, p);
  *bad = b ? 1 : 0;
  return c;
}

// the prior's terms of the packed sums of one observation, after the band sums, in place: a ascending, weight 0 skipped
void rp_prior_normal(int F, const double* t, const double* mu, const double* p, double* packed) {
  refine_prior_augment(F, packed, 1, t, 1, mu, p);
}

}  // extern "C"

#if defined(REFINE_PRIOR_MAIN)
#include <cmath>
#include <cstdio>
#include <vector>

namespace {

constexpr int NP = 27;

struct Toy {
  int nb;
  std::vector<double> Wm;      // (27, nb)
  explicit Toy(int nb_) : nb(nb_), Wm((size_t)NP * nb_) {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (double& v : Wm) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      v = ((double)(s >> 11) / 9007199254740992.0 - 0.5) * 3.0;
    }
  }
  void operator()(const double* row, double* y) const {
    for (int j = 0; j < nb; ++j) {
      double a = 0.0;
      for (int p = 0; p < NP; ++p) a += row[p] * Wm[(size_t)p * nb + j];
      y[j] = std::tanh(0.05 * a);
    }
  }
};

struct Result {
  std::vector<double> x, sdev;
  double cost, cost0;
  int na;
};

// spart_refine's loop for one observation (include/spart_hip.h), from the step functions
Result loop(const Toy& fw, const double* base, int F, const int* free_cols, const double* lo, const double* hi, const double* obs,
            const double* w, const double* mu, const double* p, int n_iter) {
  const int nb = fw.nb, nt = refine_ntri(F);
  std::vector<double> x(F), t(F), h(F), sh(F), start(F), rows((size_t)(F + 1) * NP), Y((size_t)(F + 1) * nb), J((size_t)nb * F), r(nb),
      packed(nt + F, 0.0), fresh(nt + F), tn(F), sdev(F, std::nan(""));
  for (int f = 0; f < F; ++f) {
    start[f] = base[free_cols[f]];
    h[f] = 1e-3 * (hi[f] - lo[f]);
  }
  rh_clip(F, start.data(), lo, hi, x.data());
  t = x;
  double c = INFINITY, cost0 = std::nan(""), lam = 1e-2;
  int na = 0;
  bool dead = false;
  for (int it = 0; it <= n_iter && !dead; ++it) {
    rh_fd_step(F, t.data(), h.data(), hi, sh.data());
    for (int fp = 0; fp <= F; ++fp) {
      double* row = rows.data() + (size_t)fp * NP;
      for (int q = 0; q < NP; ++q) row[q] = base[q];
      for (int f = 0; f < F; ++f) row[free_cols[f]] = t[f] + (f + 1 == fp ? sh[f] : 0.0);
      fw(row, Y.data() + (size_t)fp * nb);
    }
    int32_t bad = 0, pbad = 0;
    double ct = rh_cost(nb, Y.data(), obs, w, &bad);
    if (p) ct = rp_prior_cost(F, ct, t.data(), mu, p, &pbad);
    if (it == 0) {
      cost0 = ct;
      if (!(ct < INFINITY) || bad || pbad) {
        dead = true;
        c = ct;
        na = -1;
        break;
      }
    }
    const bool acc = ct < c;
    if (acc) {
      x = t;
      c = ct;
      rh_jacobian(F, nb, Y.data(), obs, w, sh.data(), J.data(), r.data());
      rh_normal(F, nb, J.data(), r.data(), w, fresh.data());
      if (p) rp_prior_normal(F, t.data(), mu, p, fresh.data());
      packed = fresh;
    }
    if (it > 0) {
      const int32_t a = acc ? 1 : 0;
      rh_lambda(1, &lam, &a, &lam);
      na += a;
    }
    if (it < n_iter) {
      rh_propose(F, packed.data(), lam, x.data(), lo, hi, tn.data());
      t = tn;
    }
  }
  if (!dead) rh_std(F, packed.data(), sdev.data());
  return {x, sdev, c, cost0, na};
}

}  // namespace

int main() {
  const int nb = 13, F = 4, M = 10, n_iter = 12;
  const int free_cols[F] = {15, 0, 2, 1};
  const std::vector<double> lo(F, 0.0), hi = {2.0, 1.0, 1.0, 1.0};
  const Toy fw(nb);
  uint64_t s = 12345;
  auto uni = [&s] {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  };
  int failures = 0;
  for (int m = 0; m < M; ++m) {
    std::vector<double> base(NP), truth(NP), obs(nb), w(nb), mu(F), p(F);
    for (int q = 0; q < NP; ++q) truth[q] = base[q] = uni();
    for (int f = 0; f < F; ++f) {
      truth[free_cols[f]] = lo[f] + uni() * (hi[f] - lo[f]);
      mu[f] = truth[free_cols[f]] + 0.1 * (uni() - 0.5) * (hi[f] - lo[f]);
      const double sigma = 0.1 * (hi[f] - lo[f]);
      p[f] = uni() < 0.2 ? 0.0 : 1.0 / (sigma * sigma);
      if (p[f] == 0.0) mu[f] = std::nan("");
    }
    fw(truth.data(), obs.data());
    for (int j = 0; j < nb; ++j) w[j] = std::pow(10.0, 2.0 * uni() - 1.0);
    bool want_dead = false;
    if (m == 1) base[free_cols[0]] = 5.0;                       // a start outside the box
    if (m == 2) p[1] = -1.0, want_dead = true;                  // a negative prior weight
    if (m == 3) p[2] = 100.0, mu[2] = std::nan(""), want_dead = true;      // a NaN mean under a weight
    if (m == 4) {                                               // no band counts: the prior alone, x -> clip(mu)
      for (double& v : w) v = 0.0;
      for (int f = 0; f < F; ++f) p[f] = 100.0, mu[f] = f == 0 ? 3.0 : 0.25 * (f + 1);
    }
    const Result res = loop(fw, base.data(), F, free_cols, lo.data(), hi.data(), obs.data(), w.data(), m == 5 ? nullptr : mu.data(),
                            m == 5 ? nullptr : p.data(), n_iter);
    bool ok = want_dead ? (res.na == -1 && std::isnan(res.sdev[0])) : (res.na >= 0 && res.cost <= res.cost0);
    if (m == 4)
      for (int f = 0; f < F; ++f) {
        const double want = refine_clip(mu[f], lo[f], hi[f]);
        if (!(std::fabs(res.x[f] - want) <= 1e-6 * (hi[f] - lo[f]))) ok = false;
      }
    std::printf("obs %d: n_accept %d cost0 %.6e cost %.6e x0 %.6f std0 %.3e %s\n", m, res.na, res.cost0, res.cost, res.x[0], res.sdev[0],
                ok ? "ok" : "WRONG");
    failures += ok ? 0 : 1;
  }
  return failures ? 1 : 0;
}
#endif  // REFINE_PRIOR_MAIN
