// TEST INFRASTRUCTURE ONLY (tests/test_refine_posterior_host.py): the per-observation arithmetic of spart_refine_posterior
// (csrc/spart_refine_posterior.h, part 1) beside the step functions of refine_host.cpp, for a g++ build with
// -ffp-contract=off, one observation per call.  The caller's arrays are dense; the scratch the functions work in has stride S,
// the way the kernel's LDS columns have.  With -DREFINE_POSTERIOR_MAIN the file is a stand-alone program for a
// -fsanitize=address,undefined build that is run as a child process: every buffer on the heap at its exact size.
#include <vector>

#include "refine_host.cpp"
#include "../../spart-python_amd/csrc/spart_refine_posterior.h"

extern "C" {

// J (nb, F) row-major, w (nb,), p (F,) or NULL -> K (F, F) full, cov (F, F), ak (F, F), std (F,), dfs; returns the status
// (0 ok, 1 A not positive definite: cov, ak, std, dfs are then NaN).  What k_refine_posterior does after its pass 1.
int rq_posterior(int F, int nb, const double* J, const double* w, const double* p, int S, double* K, double* cov, double* ak,
                 double* sdev, double* dfs) {
  const int nt = refine_ntri(F);
  std::vector<double> A((size_t)nt * S), Z((size_t)nt * S), C((size_t)nt * S), Kf((size_t)F * F * S), g((size_t)F * S);
  for (int e = 0; e < nt; ++e) {
    int a, b;
    refine_pair(e, &a, &b);
    A[(size_t)e * S] = refine_tile_sum(0.0, 0, nb, w, 1, J + a, F, J + b, F);
  }
  for (int a = 0; a < F; ++a)
    for (int b = 0; b < F; ++b) K[a * F + b] = Kf[(size_t)(a * F + b) * S] = refine_sym(A.data(), S, a, b);
  if (p) refine_prior_augment(F, A.data(), S, nullptr, 0, nullptr, p);      // (K has no g)
  const double nan = __builtin_nan("");
  if (!refine_cholesky(F, A.data(), S)) {
    for (int e = 0; e < F * F; ++e) cov[e] = ak[e] = nan;
    for (int f = 0; f < F; ++f) sdev[f] = nan;
    *dfs = nan;
    return 1;
  }
  refine_inverse_lower(F, A.data(), S, Z.data(), S);
  for (int a = 0; a < F; ++a)
    for (int b = 0; b <= a; ++b) C[(size_t)refine_tri(a, b) * S] = refine_cov(F, Z.data(), S, a, b);
  for (int a = 0; a < F; ++a)
    for (int b = 0; b < F; ++b) {
      cov[a * F + b] = refine_sym(C.data(), S, a, b);
      ak[a * F + b] = refine_avk(F, C.data(), S, Kf.data(), S, a, b);
      if (a == b) g[(size_t)a * S] = ak[a * F + b];
    }
  for (int f = 0; f < F; ++f) sdev[f] = __builtin_sqrt(C[(size_t)refine_tri(f, f) * S]);
  *dfs = refine_trace(F, g.data(), S);
  return 0;
}

}  // extern "C"

#if defined(REFINE_POSTERIOR_MAIN)
#include <cmath>
#include <cstdio>

int main() {
  uint64_t s = 2024;
  auto uni = [&s] {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  };
  int failures = 0;
  for (int F : {1, 2, 6, 16})
    for (int S : {1, 5, 9})
      for (int kind = 0; kind < 3; ++kind) {      // 0 no prior, 1 a prior, 2 a zero column of J without a prior (singular)
        const int nb = 64;      // (well over F weighted bands: a well-conditioned K)
        std::vector<double> J((size_t)nb * F), w(nb), p(F), K((size_t)F * F), cov((size_t)F * F), ak((size_t)F * F), sd(F);
        for (double& v : J) v = uni() - 0.5;
        for (double& v : w) v = uni() < 0.2 ? 0.0 : 1.0 + uni();
        for (double& v : p) v = 0.5 + uni();
        if (kind == 2)
          for (int j = 0; j < nb; ++j) J[(size_t)j * F] = 0.0;
        double dfs = 0.0;
        const int st = rq_posterior(F, nb, J.data(), w.data(), kind == 1 ? p.data() : nullptr, S, K.data(), cov.data(), ak.data(),
                                    sd.data(), &dfs);
        bool ok = st == (kind == 2 ? 1 : 0);
        if (kind == 0) ok = ok && std::fabs(dfs - F) <= 1e-6;
        if (kind == 1) ok = ok && dfs > 0.0 && dfs < F;
        if (kind == 2) ok = ok && std::isnan(dfs) && std::isnan(cov[0]);
        std::printf("F %d S %d kind %d: status %d dfs %.12f %s\n", F, S, kind, st, dfs, ok ? "ok" : "WRONG");
        failures += ok ? 0 : 1;
      }
  return failures ? 1 : 0;
}
#endif  // REFINE_POSTERIOR_MAIN
