// TEST INFRASTRUCTURE ONLY (tests/test_vjp_host.py): part 1 of csrc/spart_vjp.h -- the two steps of a free parameter, one
// band's term, the ordered sum of a tile, the division -- and a batch built from them the way k_vjp_reduce builds it (groups
// of W observations, tiles of 16 bands staged in the [f FS + jj (W + 1) + o] layout on a heap buffer of exactly the kernel's
// LDS size, one accumulator per (observation, f) carried across tiles and columns), for a g++ build with -ffp-contract=off.
// With -DVJP_MAIN the file is a stand-alone program for -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../spart-python_amd/csrc/spart_vjp.h"

using namespace spart;

extern "C" {

int64_t vjh_chunk(int F) { return vjp_chunk(F); }
int vjh_group(int F) { return vjp_group(F); }
int vjh_fstride(int W) { return vjp_fstride(W); }
double vjh_max_rel_step() { return VJP_MAX_REL_STEP; }
double vjh_rel_step() { return VJP_REL_STEP; }

void vjh_step(double x, double h, double lo, double hi, double* a, double* b) {
  const VjpStep s = vjp_step(refine_clip(x, lo, hi), h, lo, hi);
  *a = s.a, *b = s.b;
}

// grad (M, F) from g[c] (M, nb) or NULL, Yp / Ym (3, F, M, nb) and den (M, F), in groups of W observations
void vjh_grad(int M, int F, int nb, const double* g0, const double* g1, const double* g2, const double* Yp, const double* Ym,
              const double* den, int W, double* grad) {
  const int JT = 16, WP = W + 1, FS = vjp_fstride(W);
  const double* g[3] = {g0, g1, g2};
  std::vector<double> P((size_t)F * FS), s((size_t)W * F);
  for (int m0 = 0; m0 < M; m0 += W) {
    const int nobs = M - m0 < W ? M - m0 : W;
    std::fill(s.begin(), s.end(), 0.0);
    for (int c = 0; c < 3; ++c) {
      if (!g[c]) continue;
      for (int j0 = 0; j0 < nb; j0 += JT) {
        for (int i = 0; i < W * JT; ++i) {
          const int jj = i % JT, o = i / JT, j = j0 + jj;
          const bool in = o < nobs && j < nb;
          for (int f = 0; f < F; ++f) {
            const size_t at = (((size_t)c * F + f) * M + m0 + o) * nb + j;
            P[(size_t)f * FS + jj * WP + o] = in ? vjp_term(g[c][(size_t)(m0 + o) * nb + j], Yp[at], Ym[at]) : 0.0;
          }
        }
        for (int o = 0; o < nobs; ++o)
          for (int f = 0; f < F; ++f)
            s[(size_t)o * F + f] = vjp_tile_add(s[(size_t)o * F + f], nb - j0 < JT ? nb - j0 : JT, P.data() + (size_t)f * FS + o, WP);
      }
    }
    for (int o = 0; o < nobs; ++o)
      for (int f = 0; f < F; ++f) grad[(size_t)(m0 + o) * F + f] = vjp_finish(s[(size_t)o * F + f], den[(size_t)(m0 + o) * F + f]);
  }
}

}  // extern "C"

#ifdef VJP_MAIN
// every F and nb of the test with M = W + 3 observations on heap buffers of exact size, zero g entries over NaN Y, one NULL
// column: the staged sum must give the bits of the plain skipping loop of the definition
static double lcg(uint64_t& s) {
  s = s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(s >> 11) / 9007199254740992.0;
}

int main() {
  for (int F : {1, 2, 6, 16})
    for (int nb : {1, 13, 17, 211}) {
      const int W = vjp_group(F), M = W + 3;
      uint64_t seed = 77u + F * 1000 + nb;
      const size_t ny = (size_t)3 * F * M * nb;
      std::vector<double> Yp(ny), Ym(ny), den((size_t)M * F), grad((size_t)M * F), want((size_t)M * F);
      std::vector<double> g[3];
      for (double& v : Yp) v = lcg(seed);
      for (double& v : Ym) v = lcg(seed);
      for (double& v : den) v = 1e-3 * (1.0 + lcg(seed));
      for (int c = 0; c < 3; ++c) {
        g[c].resize((size_t)M * nb);
        for (double& v : g[c]) v = lcg(seed) - 0.5;
      }
      int nzero = 0;
      for (size_t i = 0; i < g[0].size(); i += 3) {        // zeros over NaN
        g[0][i] = 0.0;
        for (int f = 0; f < F; ++f) Yp[(size_t)f * M * nb + i] = std::numeric_limits<double>::quiet_NaN();
        ++nzero;
      }
      vjh_grad(M, F, nb, g[0].data(), nullptr, g[2].data(), Yp.data(), Ym.data(), den.data(), W, grad.data());
      for (int m = 0; m < M; ++m)
        for (int f = 0; f < F; ++f) {
          double s = 0.0;
          for (int c = 0; c < 3; c += 2)
            for (int j = 0; j < nb; ++j) {
              const double gj = g[c][(size_t)m * nb + j];
              if (gj == 0.0) continue;
              const size_t at = (((size_t)c * F + f) * M + m) * nb + j;
              const double d = Yp[at] - Ym[at];
              s = s + gj * d;
            }
          want[(size_t)m * F + f] = s / den[(size_t)m * F + f];
        }
      bool ok = std::memcmp(grad.data(), want.data(), grad.size() * 8) == 0 && nzero > 0;
      for (double v : grad) ok = ok && v == v;
      double a, b;
      vjh_step(7.5, 0.25, 0.0, 7.0, &a, &b);
      ok = ok && a == 7.0 && b == 6.75;
      std::printf("F %d nb %d W %d%s\n", F, nb, W, ok ? " ok" : " WRONG");
      if (!ok) return 1;
    }
  return 0;
}
#endif
