// TEST INFRASTRUCTURE ONLY (tests/test_refine_series_host.py): part 1 of csrc/spart_refine_series.h -- the link weights, the
// chain's part of the cost and of the sums, the chain elimination step, the substitution along the chain and the std recurrence
// -- and one series' step built from them the way the kernels build it (a walk along the rows that keeps the previous row's
// eliminated vector, Schur sums in row order), for a g++ build with -ffp-contract=off.  Every array dense (stride 1) unless a
// stride is passed; a series has at most 256 rows.  With -DREFINE_SERIES_MAIN the file is a stand-alone program (heap buffers
// of exact size) for -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../spart-python_amd/csrc/spart_refine_series.h"

using namespace spart;

extern "C" {

int rsh_max_rows() { return SERIES_MAXT; }
int rsh_bad_link(double v) { return series_bad_link(v) ? 1 : 0; }

// C of one series: the rows' costs, the chain term on the trial locals lt (G, Fl), the shared prior; bad: a bad link entry that
// is read or a bad shared prior weight.  link NULL: 1.
double rsh_series_cost(int G, const double* c, int Fl, const double* gamma, const double* link, const double* lt, int Fs,
                       const double* zt, const double* smu, const double* spw, int32_t* bad) {
  double C = 0.0;
  *bad = 0;
  for (int m = 0; m < G; ++m) C = C + c[m];
  for (int m = 0; m + 1 < G; ++m) {
    const double lk = link ? link[m] : 1.0;
    if (series_bad_link(lk)) *bad = 1;
    for (int b = 0; b < Fl; ++b) {
      const double k = series_kappa(gamma[b], lk);
      if (k != 0.0) C = series_chain_cost(C, k, lt[(m + 1) * Fl + b], lt[m * Fl + b]);
    }
  }
  bool b = false;
  if (spw) C = refine_prior_total(Fs, C, &b, zt, smu, spw);
  if (b) *bad = 1;
  return C;
}

// the chain's part of the packed sums Ap (G, P) at the accepted locals l (G, Fl), in place
void rsh_augment(int G, int F, int Fs, const double* gamma, const double* link, const double* l, double* Ap) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F;
  for (int m = 0; m < G; ++m)
    for (int b = 0; b < Fl; ++b) {
      double kp = 0.0, ep = 0.0, kn = 0.0, en = 0.0;
      if (m > 0) {
        kp = series_kappa(gamma[b], link ? link[m - 1] : 1.0);
        ep = l[m * Fl + b] - l[(m - 1) * Fl + b];
      }
      if (m + 1 < G) {
        kn = series_kappa(gamma[b], link ? link[m] : 1.0);
        en = l[(m + 1) * Fl + b] - l[m * Fl + b];
      }
      series_augment(&Ap[m * P + refine_tri(b, b)], &Ap[m * P + nt + b], kp, ep, kn, en);
    }
}

// The walk along the chain with stride SW in every working array: Lp (G, P) the eliminated rows, Xp (G, Fl Fl), sh (Ps) the
// shared factor with the walked right-hand side; false at a failed pivot
static bool series_factor(int G, const double* Ap, const double* St, int F, int Fs, double lam, bool damp, const double* gamma,
                          const double* link, int SW, std::vector<double>& Lp, std::vector<double>& Xp, std::vector<double>& sh) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs, FF = Fl * Fl;
  Lp.assign((size_t)G * P * SW, 0.0);
  Xp.assign((size_t)G * FF * SW, 0.0);
  sh.assign((size_t)Ps * SW + 1, 0.0);
  for (int e = 0; e < Ps; ++e) {
    double v = St[e];
    if (e < nts) {
      int a, b;
      refine_pair(e, &a, &b);
      if (a == b && damp) v = v + lam * (v > 0.0 ? v : 1.0);
    } else {
      v = -v;
    }
    sh[(size_t)e * SW] = v;
  }
  for (int m = 0; m < G; ++m) {
    double* L = Lp.data() + (size_t)m * P * SW;
    for (int e = 0; e < P; ++e) L[e * SW] = Ap[m * P + e];
    if (damp)
      for (int j = 0; j < Fl; ++j) {
        const double v = L[refine_tri(j, j) * SW];
        L[refine_tri(j, j) * SW] = v + lam * (v > 0.0 ? v : 1.0);
      }
    const double lq = m > 0 ? (link ? link[m - 1] : 1.0) : 0.0;
    const bool pres = m > 0 && series_present(Fl, gamma, lq);
    const double* Lq = m > 0 ? Lp.data() + (size_t)(m - 1) * P * SW : L;
    if (!series_chain_step(F, Fl, L, SW, Lq, SW, pres, gamma, lq, Xp.data() + (size_t)m * FF * SW, SW, damp)) return false;
    series_schur_row(F, Fs, Fl, L, SW, sh.data(), SW, damp);
  }
  return series_shared_factor(Fs, sh.data(), SW);
}

// the next trial of a series: z (Fs), l (G, Fl) the accepted point, lo / hi per name -> zt, lt.  Returns 1 when the step was
// taken, 0 when delta = 0
int rsh_series_propose(int G, const double* Ap, const double* St, int F, int Fs, double lam, const double* gamma, const double* link,
                       int SW, const double* z, const double* l, const double* lo, const double* hi, double* zt, double* lt) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), FF = Fl * Fl;
  std::vector<double> Lp, Xp, sh;
  bool ok = series_factor(G, Ap, St, F, Fs, lam, true, gamma, link, SW, Lp, Xp, sh);
  if (ok) ok = series_shared_solve(Fs, sh.data(), sh.data() + (size_t)nts * SW, SW);
  if (ok)
    for (int m = G - 1; m >= 0; --m) {
      double* L = Lp.data() + (size_t)m * P * SW;
      const bool pres = m + 1 < G && series_present(Fl, gamma, link ? link[m] : 1.0);
      const double* Xn = pres ? Xp.data() + (size_t)(m + 1) * FF * SW : nullptr;
      const double* dn = m + 1 < G ? Lp.data() + ((size_t)(m + 1) * P + nt) * SW : L;
      series_chain_back(F, Fs, Fl, L, SW, Xn, SW, dn, SW, sh.data() + (size_t)nts * SW, SW);
      for (int j = 0; j < Fl; ++j)
        if (!(L[(nt + j) * SW] - L[(nt + j) * SW] == 0.0)) ok = false;
    }
  for (int a = 0; a < Fs; ++a) zt[a] = refine_clip(z[a] + (ok ? sh[(size_t)(nts + a) * SW] : 0.0), lo[a], hi[a]);
  for (int m = 0; m < G; ++m)
    for (int j = 0; j < Fl; ++j)
      lt[m * Fl + j] = refine_clip(l[m * Fl + j] + (ok ? Lp[((size_t)m * P + nt + j) * SW] : 0.0), lo[Fs + j], hi[Fs + j]);
  return ok ? 1 : 0;
}

// every std of a series from the undamped sums (NaN at a failed factorisation)
void rsh_series_std(int G, const double* Ap, const double* St, int F, int Fs, const double* gamma, const double* link, int SW,
                    double* shared_std, double* local_std) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, FF = Fl * Fl;
  std::vector<double> Lp, Xp, sh, z((size_t)(2 * Fl + Fs) * SW + 1);
  const bool ok = series_factor(G, Ap, St, F, Fs, 0.0, false, gamma, link, SW, Lp, Xp, sh);
  for (int f = 0; f < Fs; ++f) shared_std[f] = ok ? series_shared_std(Fs, f, sh.data(), SW, z.data(), SW) : __builtin_nan("");
  for (int m = 0; m < G; ++m)
    for (int j = 0; j < Fl; ++j)
      local_std[m * Fl + j] =
          ok ? series_local_std(F, Fs, Fl, j, G - m, Lp.data() + (size_t)m * P * SW, (int64_t)P * SW, SW,
                                Xp.data() + (size_t)m * FF * SW, (int64_t)FF * SW, SW, gamma, link ? link + m : nullptr, sh.data(), SW,
                                z.data(), z.data() + (size_t)Fl * SW, z.data() + (size_t)2 * Fl * SW, SW)
             : __builtin_nan("");
}

}  // extern "C"

#if defined(REFINE_SERIES_MAIN)
// A diagonally dominant series for every shape, stride and link kind (NULL, varied, a zero in the middle), and a singular one:
// the step must be taken / refused and every output finite / NaN accordingly
int main() {
  const int shapes[][2] = {{0, 1}, {1, 2}, {2, 2}, {0, 16}, {15, 1}};
  const int lens[] = {1, 2, 3, 8, 9, 39, 67};
  int wrong = 0;
  for (const auto& sf : shapes)
    for (int G : lens)
      for (int kind = 0; kind < 3; ++kind)
        for (int SW : {1, 5}) {
          const int Fs = sf[0], Fl = sf[1], F = Fs + Fl, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs;
          std::vector<double> Ap((size_t)G * P), St((size_t)Ps > 0 ? Ps : 1), gamma(Fl), link(G), z(Fs > 0 ? Fs : 1), l((size_t)G * Fl),
              lo(F, -10.0), hi(F, 10.0), zt(Fs > 0 ? Fs : 1), lt((size_t)G * Fl), ss(Fs > 0 ? Fs : 1), ls((size_t)G * Fl);
          unsigned seed = 12345u + (unsigned)(G * 131 + F * 7 + kind);
          auto rnd = [&]() {
            seed = seed * 1664525u + 1013904223u;
            return (double)(seed >> 8) / 16777216.0 - 0.5;
          };
          for (int m = 0; m < G; ++m) {
            for (int i = 0; i < F; ++i)
              for (int j = 0; j <= i; ++j) Ap[(size_t)m * P + refine_tri(i, j)] = i == j ? 2.0 * F + rnd() : 0.5 * rnd();
            for (int i = 0; i < F; ++i) Ap[(size_t)m * P + nt + i] = rnd();
            for (int b = 0; b < Fl; ++b) l[(size_t)m * Fl + b] = rnd();
            link[m] = kind == 2 && m == G / 2 ? 0.0 : 0.5 + rnd() * rnd();
          }
          for (int b = 0; b < Fl; ++b) gamma[b] = b % 3 == 2 ? 0.0 : 1.0 + b;
          for (int e = 0; e < Ps; ++e) St[e] = 0.0;
          for (int a = 0; a < Fs; ++a) {
            St[refine_tri(a, a)] = 2.0 * F * G;
            z[a] = rnd();
          }
          const double* lk = kind == 0 ? nullptr : link.data();
          rsh_augment(G, F, Fs, gamma.data(), lk, l.data(), Ap.data());
          const int took = rsh_series_propose(G, Ap.data(), St.data(), F, Fs, 1e-2, gamma.data(), lk, SW, z.data(), l.data(), lo.data(),
                                              hi.data(), zt.data(), lt.data());
          rsh_series_std(G, Ap.data(), St.data(), F, Fs, gamma.data(), lk, SW, ss.data(), ls.data());
          bool fin = took == 1;
          for (double v : ls) fin = fin && v - v == 0.0 && v > 0.0;
          for (int a = 0; a < Fs; ++a) fin = fin && ss[a] - ss[a] == 0.0;
          // the singular twin: a zero row block without a tie cannot be factorised undamped
          Ap[(size_t)(G - 1) * P + refine_tri(0, 0)] = -1.0;
          rsh_series_std(G, Ap.data(), St.data(), F, Fs, gamma.data(), lk, SW, ss.data(), ls.data());
          const bool nan = ls[0] != ls[0];
          if (!fin || !nan) ++wrong;
          std::printf("Fs %d Fl %d G %d link %d stride %d %s\n", Fs, Fl, G, kind, SW, fin && nan ? "ok" : "WRONG");
        }
  return wrong ? 1 : 0;
}
#endif
