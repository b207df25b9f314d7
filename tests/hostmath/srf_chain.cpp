// The SRF band sum of include/spart_hip.h as ONE float64 answer: per row s and band j
//     acc = 0;  for e in start[j] .. start[j + 1] - 1 (ascending):  acc = fma(q[e], X[s, ev[e]], acc);  out[s, j] = acc / Q[j]
// with correctly rounded std::fma (glibc) and one IEEE division.  NaN, infinities and Q = 0 follow IEEE: no special code.
// scale[s, j] = (sum_e |q[e]| |X[s, ev[e]]|) / |Q[j]|, the rounding scale of the chain (plain sum, used for bounds only).
// Test-only (tests/helpers/srf_exact.py); built with -ffp-contract=off so that nothing but std::fma is fused.
#include <cmath>
#include <cstdint>

extern "C" void srf_chain(int64_t B, int64_t ne, const double* X, const int32_t* start, const int32_t* ev, const double* q,
                          const double* Q, int32_t nb, double* out, double* scale) {
  for (int64_t s = 0; s < B; ++s) {
    const double* x = X + s * ne;
    for (int32_t j = 0; j < nb; ++j) {
      double acc = 0.0, sc = 0.0;
      for (int32_t e = start[j]; e < start[j + 1]; ++e) {
        acc = std::fma(q[e], x[ev[e]], acc);
        sc = sc + std::fabs(q[e]) * std::fabs(x[ev[e]]);
      }
      out[s * nb + j] = acc / Q[j];
      scale[s * nb + j] = sc / std::fabs(Q[j]);
    }
  }
}
