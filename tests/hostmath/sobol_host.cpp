// TEST INFRASTRUCTURE ONLY (tests/test_sobol_host.py): part 1 of csrc/spart_sobol.h -- the design point, the shift, the 64-term
// tree, the finish formulas and the jackknife of one (band, parameter) -- and one site built from them the way the kernels build
// it (block sums in the (g, q, band) layout, then one entry per (band, f)), for a g++ build with -ffp-contract=off.  `stride`
// spreads every element of the block sums and of the tree's scratch, so that a wrong stride shows.  With -DSOBOL_MAIN the file
// is a stand-alone program (heap buffers of exact size) for -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../spart-python_amd/csrc/spart_sobol.h"

using namespace spart;

extern "C" {

int sbh_block() { return SOBOL_BLOCK; }
int sbh_nq(int F) { return sobol_nq(F); }
int sbh_chunk_blocks(int F) { return sobol_chunk_blocks(F); }
double sbh_point(double lo, double hi, double u) { return sobol_point(lo, hi, u); }

// the tree over t[0 .. 63], dense in, through a scratch of the given stride
double sbh_tree(const double* t, int stride) {
  std::vector<double> s((size_t)(SOBOL_BLOCK - 1) * stride + 1);
  for (int r = 0; r < SOBOL_BLOCK; ++r) s[(size_t)r * stride] = t[r];
  return sobol_tree64(s.data(), stride);
}

// the block sums of one site: yA, yB (N, nb), yC (F, N, nb) -> bs, element (g, q, j) at ((g Q + q) nb + j) stride; c (nb,)
void sbh_blocks(int N, int F, int nb, const double* yA, const double* yB, const double* yC, int stride, double* bs, double* c) {
  const int G = N / SOBOL_BLOCK, Q = sobol_nq(F);
  std::vector<double> t((size_t)(SOBOL_BLOCK - 1) * stride + 1);
  for (int j = 0; j < nb; ++j) c[j] = yA[j];
  for (int g = 0; g < G; ++g)
    for (int j = 0; j < nb; ++j)
      for (int q = 0; q < Q; ++q) {
        for (int r = 0; r < SOBOL_BLOCK; ++r) {
          const size_t n = (size_t)g * SOBOL_BLOCK + r;
          const double a = sobol_shift(yA[n * nb + j], c[j]), b = sobol_shift(yB[n * nb + j], c[j]);
          double v;
          if (q < 4) {
            v = q == 0 ? a : q == 1 ? b : q == 2 ? sobol_mul(a, a) : sobol_mul(b, b);
          } else {
            const int f = (q - 4) / 3, k = (q - 4) % 3;
            const double d = sobol_delta(yC[((size_t)f * N + n) * nb + j], c[j], a);
            v = k == 0 ? sobol_mul(b, d) : k == 1 ? sobol_mul(d, d) : d;
          }
          t[(size_t)r * stride] = v;
        }
        bs[(((size_t)g * Q + q) * nb + j) * stride] = sobol_tree64(t.data(), stride);
      }
}

// one (band, f) from block sums in sbh_blocks' layout -> out[6]: mean, var, S1, ST, S1_se, ST_se
void sbh_entry(const double* bs, int stride, int G, int F, int nb, int j, int f, double c, int jack, double* out) {
  const int Q = sobol_nq(F);
  sobol_entry(bs + (size_t)j * stride, (int64_t)Q * nb * stride, (int64_t)nb * stride, G, f, (double)G * SOBOL_BLOCK, c, jack != 0, out);
}

// a whole site: mean, var (nb,), S1, ST, S1_se, ST_se (nb, F)
void sbh_site(int N, int F, int nb, const double* yA, const double* yB, const double* yC, int stride, double* mean, double* var,
              double* S1, double* ST, double* S1se, double* STse) {
  const int G = N / SOBOL_BLOCK, Q = sobol_nq(F);
  std::vector<double> bs(((size_t)G * Q * nb - 1) * stride + 1), c(nb);
  sbh_blocks(N, F, nb, yA, yB, yC, stride, bs.data(), c.data());
  for (int j = 0; j < nb; ++j)
    for (int f = 0; f < F; ++f) {
      double r[6];
      sbh_entry(bs.data(), stride, G, F, nb, j, f, c[j], 1, r);
      mean[j] = r[0], var[j] = r[1];
      S1[j * F + f] = r[2], ST[j * F + f] = r[3], S1se[j * F + f] = r[4], STse[j * F + f] = r[5];
    }
}

}  // extern "C"

#ifdef SOBOL_MAIN
// every F, G and stride of the test on heap buffers of exact size; the strided run must give the dense run's bits, a constant
// band must give var == 0 and NaN indices, and yB == yA must give zeros
static double lcg(uint64_t& s) {
  s = s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(s >> 11) / 9007199254740992.0;
}

int main() {
  const int nb = 3;
  for (int F : {1, 3, 16})
    for (int G : {2, 3, 64})
      for (int stride : {1, 5}) {
        const int N = G * SOBOL_BLOCK;
        uint64_t seed = 1234u + F * 100 + G;
        std::vector<double> yA((size_t)N * nb), yB((size_t)N * nb), yC((size_t)F * N * nb);
        for (double& v : yA) v = 100.0 + lcg(seed);
        for (double& v : yB) v = 100.0 + lcg(seed);
        for (size_t i = 0; i < yC.size(); ++i) yC[i] = 0.5 * (yA[i % yA.size()] + 100.0 + lcg(seed));
        for (int n = 0; n < N; ++n) {                      // band 2 is constant
          yA[(size_t)n * nb + 2] = yB[(size_t)n * nb + 2] = 7.0;
          for (int f = 0; f < F; ++f) yC[((size_t)f * N + n) * nb + 2] = 7.0;
        }
        std::vector<double> out[2][6];
        for (int k = 0; k < 2; ++k) {
          for (int i = 0; i < 6; ++i) out[k][i].assign(i < 2 ? nb : (size_t)nb * F, -1.0);
          sbh_site(N, F, nb, yA.data(), yB.data(), yC.data(), k ? stride : 1, out[k][0].data(), out[k][1].data(), out[k][2].data(),
                   out[k][3].data(), out[k][4].data(), out[k][5].data());
        }
        bool ok = true;
        for (int i = 0; i < 6; ++i)
          ok = ok && std::memcmp(out[0][i].data(), out[1][i].data(), out[0][i].size() * 8) == 0;
        ok = ok && out[1][1][2] == 0.0 && out[1][2][2 * F] != out[1][2][2 * F] && out[1][0][2] == 7.0;
        ok = ok && out[1][1][0] > 0.0 && out[1][4][0] > 0.0;
        // yB == yA (and C == A): exact zeros
        std::vector<double> yCa((size_t)F * N * nb);
        for (int f = 0; f < F; ++f) std::memcpy(&yCa[(size_t)f * N * nb], yA.data(), (size_t)N * nb * 8);
        sbh_site(N, F, nb, yA.data(), yA.data(), yCa.data(), stride, out[1][0].data(), out[1][1].data(), out[1][2].data(),
                 out[1][3].data(), out[1][4].data(), out[1][5].data());
        for (int i = 2; i < 6; ++i)
          for (int f = 0; f < 2 * F; ++f) ok = ok && out[1][i][f] == 0.0;
        std::printf("F %d G %d stride %d%s\n", F, G, stride, ok ? " ok" : " WRONG");
        if (!ok) return 1;
      }
  return 0;
}
#endif
