// TEST INFRASTRUCTURE ONLY (tests/test_refine_mix_host.py): the maps, the fractions and the per-entry products of
// spart_refine_mix (csrc/spart_refine_mix.h, part 1) and one pixel's whole fit built from them and from the per-entry functions
// of csrc/spart_refine.h the way k_refine_mix_step builds it -- 16-band tiles, every element of y and J folded over the
// components in ascending order -- for a g++ build with -ffp-contract=off.  Every array dense (stride 1).  The forward model is
// a cheap positive toy, rmh_forward, which the Python test hands to the definition too.  With -DRMH_MAIN the file is a
// stand-alone program that drives the same loop over a few shapes (the sanitizer build).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../spart-python_amd/csrc/spart_refine_mix.h"

using namespace spart;

extern "C" {

int rmh_max_v() { return MIX_MAXV; }

// kind[a], name[a], comp[a] of the n unknowns (16 entries each); unknown[v F + f]; -> n, -1 or -2 as mix_build_map
int rmh_maps(int V, int Fs, int Fl, const int32_t* active, int fit, int32_t* kind, int32_t* name, int32_t* comp, int32_t* unknown,
             int32_t* nm) {
  MixMap m;
  const int n = mix_build_map(V, Fs, Fl, active, fit, &m);
  *nm = m.nm;
  for (int a = 0; a < REFINE_MAXF; ++a) {
    kind[a] = mix_kind(a, Fs, m.nm);
    name[a] = m.name[a];
    comp[a] = m.comp[a];
  }
  for (int v = 0; v < V; ++v)
    for (int f = 0; f < Fs + Fl; ++f) unknown[v * (Fs + Fl) + f] = m.unk[v][f];
  return n;
}

// the toy forward model: rows (R, 27) -> out (R, nb), positive, smooth, a NaN parameter gives a NaN row
void rmh_forward(int64_t R, const double* rows, int nb, double* out) {
  for (int64_t r = 0; r < R; ++r)
    for (int j = 0; j < nb; ++j) {
      double z = 0.0;
      for (int p = 0; p < 27; ++p) z += 0.3 * std::sin(1.0 + 0.7 * p + 1.3 * j * p + 0.3 * j) * rows[r * 27 + p];
      out[r * nb + j] = 0.05 + 1.0 / (1.0 + std::exp(-z)) + 0.05 * std::sin(rows[r * 27] * (j + 1));
    }
}

// One pixel's fit.  base (V, 27); free_cols, lo, hi (F,); obs (nb,); w NULL or (nb,); frac (V,); mu, pw NULL or (n,).
// Outputs x, sdev (n,), cost, cost0, n_accept, y (nb,), frac_out (V,), y_comp (V, nb), infeasible: the trials that were.
void rmh_pixel(int V, int Fs, int Fl, const int32_t* active, int fit, double flo, double fhi, int nb, const double* base,
               const int32_t* free_cols, const double* lo, const double* hi, double rel_step, double lambda0, int n_iter,
               const double* obs, const double* w, const double* frac, const double* mu, const double* pw, double* x, double* sdev,
               double* cost, double* cost0, int32_t* n_accept, double* y, double* frac_out, double* y_comp, int32_t* infeasible) {
  constexpr int JT = 16;                   // REFINE_JT of the kernels; the sums do not depend on it
  const int F = Fs + Fl;
  MixMap map;
  const int n = mix_build_map(V, Fs, Fl, active, fit, &map), nm = map.nm;
  const int nt = refine_ntri(n), P = nt + n;
  double lo_n[REFINE_MAXF], hi_n[REFINE_MAXF], h_n[REFINE_MAXF], t[REFINE_MAXF], sh[REFINE_MAXF], tn[REFINE_MAXF];
  double packed[REFINE_MAXF * (REFINE_MAXF + 1) / 2 + REFINE_MAXF], acc[REFINE_MAXF * (REFINE_MAXF + 1) / 2 + REFINE_MAXF];
  double L[REFINE_MAXF * (REFINE_MAXF + 1) / 2], d[REFINE_MAXF], a[MIX_MAXV];
  std::vector<double> rows((size_t)V * (F + 1) * 27), Y((size_t)V * (F + 1) * nb), Jt((size_t)n * JT);
  double wl[JT], rl[JT];
  for (int u = 0; u < n; ++u) {
    if (u < nm) {
      const int f = map.name[u], v = map.comp[u] < 0 ? 0 : map.comp[u];
      lo_n[u] = lo[f], hi_n[u] = hi[f], h_n[u] = rel_step * (hi[f] - lo[f]);
      x[u] = refine_clip(base[v * 27 + free_cols[f]], lo[f], hi[f]);
    } else {
      lo_n[u] = flo, hi_n[u] = fhi, h_n[u] = 0.0;
      x[u] = refine_clip(frac[map.comp[u]], flo, fhi);
    }
    t[u] = x[u];
    sdev[u] = __builtin_nan("");
  }
  for (int e = 0; e < P; ++e) packed[e] = 0.0;
  double c = __builtin_inf(), lam = lambda0;
  int na = 0;
  *infeasible = 0;
  for (int it = 0; it <= n_iter; ++it) {
    for (int u = 0; u < n; ++u) sh[u] = refine_fd_step(t[u], h_n[u], hi_n[u]);
    for (int v = 0; v < V; ++v)
      for (int fp = 0; fp <= F; ++fp) {
        double* row = rows.data() + ((size_t)v * (F + 1) + fp) * 27;
        for (int p = 0; p < 27; ++p) row[p] = base[v * 27 + p];
        for (int f = 0; f < F; ++f) {
          const int u = map.unk[v][f];
          if (u >= 0) row[free_cols[f]] = fp == f + 1 ? t[u] + sh[u] : t[u];
        }
      }
    rmh_forward((int64_t)V * (F + 1), rows.data(), nb, Y.data());                   // Y_(v,f) at Y[(v (F + 1) + f) nb]
    bool bad = false, feasible = true;
    if (fit) {
      feasible = mix_fractions(V, t + nm, 1, a, 1);
    } else {
      for (int v = 0; v < V; ++v) {
        a[v] = frac[v];
        if (refine_bad_weight(a[v])) bad = true;
      }
    }
    if (!feasible) ++*infeasible;
    // pass 1: the mixed column and the trial cost
    std::vector<double> ym(nb);
    for (int j = 0; j < nb; ++j) {
      double yj = 0.0;
      for (int v = 0; v < V; ++v) yj = mix_add(yj, a[v], Y[((size_t)v * (F + 1)) * nb + j], v == 0);
      ym[j] = yj;
    }
    const double one = 1.0;                // (no weights: every band reads this one, stride 0)
    double ct = refine_tile_cost(0.0, &bad, nb, w ? w : &one, w ? 1 : 0, ym.data(), 1, obs, 1);
    if (pw) ct = refine_prior_total(n, ct, &bad, t, mu, pw);
    if (!feasible) ct = __builtin_inf();
    const RefineDecision dec = refine_decide(it, ct, bad, c, lam, na);
    const int code = dec.code;
    na = dec.na, lam = dec.lam;
    if (it == 0) *cost0 = ct;
    if (code == 2) c = ct;
    if (code == 1 || code == 2) {
      if (code == 1) {
        c = ct;
        for (int u = 0; u < n; ++u) x[u] = t[u];
      }
      for (int v = 0; v < V; ++v) {
        frac_out[v] = a[v];
        for (int j = 0; j < nb; ++j) y_comp[v * nb + j] = Y[((size_t)v * (F + 1)) * nb + j];
      }
      for (int j = 0; j < nb; ++j) y[j] = ym[j];
    }
    if (code == 2) break;
    if (code == 1) {
      // pass 2: tile by tile, r and J folded over the components, then the packed sums
      for (int e = 0; e < P; ++e) acc[e] = 0.0;
      for (int j0 = 0; j0 < nb; j0 += JT) {
        const int jn = nb - j0 < JT ? nb - j0 : JT;
        for (int jj = 0; jj < jn; ++jj) {
          const int j = j0 + jj;
          wl[jj] = w ? w[j] : 1.0;
          rl[jj] = wl[jj] != 0.0 ? refine_residual(ym[j], obs[j]) : 0.0;
          for (int u = 0; u < n; ++u) {
            const int vu = map.comp[u];
            double g = 0.0;
            if (u >= nm) {
              g = mix_jac_fraction(Y[((size_t)vu * (F + 1)) * nb + j], Y[((size_t)(V - 1) * (F + 1)) * nb + j]);
            } else {
              const int f = map.name[u], v0 = vu < 0 ? 0 : vu, v1 = vu < 0 ? V : vu + 1;
              for (int v = v0; v < v1; ++v)
                g = mix_jac_term(g, a[v], Y[((size_t)v * (F + 1) + f + 1) * nb + j], Y[((size_t)v * (F + 1)) * nb + j], sh[u], v == v0);
            }
            Jt[(size_t)u * JT + jj] = g;
          }
        }
        for (int e = 0; e < P; ++e) {
          int ua, ub;
          refine_packed_pair(e, nt, &ua, &ub);
          const double* ja = Jt.data() + (size_t)ua * JT;
          const double* jc = ub >= 0 ? Jt.data() + (size_t)ub * JT : rl;
          acc[e] = refine_tile_sum(acc[e], 0, jn, wl, 1, ja, 1, jc, 1);
        }
      }
      if (pw) refine_prior_augment(n, acc, 1, x, 1, mu, pw);
      for (int e = 0; e < P; ++e) packed[e] = acc[e];
    }
    if (it < n_iter) {
      refine_propose(n, packed, 1, lam, x, 1, lo_n, hi_n, L, 1, d, 1, tn, 1);
      for (int u = 0; u < n; ++u) t[u] = tn[u];
    }
  }
  *cost = c;
  *n_accept = na;
  if (na >= 0) refine_std(n, packed, 1, L, 1, d, 1, sdev, 1);
}

}  // extern "C"

#if defined(RMH_MAIN)
// the stand-alone driver: a few shapes on synthetic pixels; prints a checksum so that nothing is optimised away
int main() {
  struct Shape {
    int V, Fs, Fl, fit;
    int32_t active[MIX_MAXV * 3];
    bool masked;
  };
  const Shape shapes[] = {{1, 0, 3, 0, {}, false},       {1, 2, 1, 1, {}, false}, {2, 1, 2, 1, {1, 1, 0, 0}, true},
                          {3, 0, 1, 1, {1, 0, 1}, true}, {4, 1, 3, 1, {}, false}, {8, 1, 1, 1, {}, false},
                          {8, 9, 0, 1, {}, false},       {2, 2, 1, 0, {}, false}};
  const int32_t free_cols[16] = {15, 0, 2, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14};
  double sum = 0.0;
  int fits = 0;
  for (const Shape& s : shapes)
    for (int nb : {7, 21})
      for (int px = 0; px < 4; ++px) {
        const int F = s.Fs + s.Fl;
        MixMap map;
        const int n = mix_build_map(s.V, s.Fs, s.Fl, s.masked ? s.active : nullptr, s.fit, &map);
        if (n < 1 || n > REFINE_MAXF) return 2;
        std::vector<double> base((size_t)s.V * 27), truth((size_t)s.V * 27), lo(F, 0.0), hi(F, 1.0), obs(nb), w(nb), frac(s.V), mu(n, 0.5),
            pw(n, 0.25), Yt((size_t)s.V * nb);
        unsigned seed = 12345u + 77u * px + 1000u * s.V + 13u * nb;
        auto rnd = [&] { return (double)((seed = seed * 1664525u + 1013904223u) >> 8) / 16777216.0; };
        for (size_t i = 0; i < base.size(); ++i) truth[i] = rnd(), base[i] = truth[i];
        for (int v = 0; v < s.V; ++v) {
          frac[v] = 1.0 / s.V;
          for (int f = 0; f < F; ++f) base[v * 27 + free_cols[f]] = truth[v * 27 + free_cols[f]] + 0.2 * (rnd() - 0.5);
        }
        rmh_forward(s.V, truth.data(), nb, Yt.data());
        for (int j = 0; j < nb; ++j) {
          obs[j] = 0.0;
          for (int v = 0; v < s.V; ++v) obs[j] += Yt[(size_t)v * nb + j] / s.V;
          w[j] = j == 2 ? 0.0 : 0.5 + rnd();
        }
        if (px == 3 && s.fit && s.V > 1) frac[0] = 0.999, frac[1 % s.V] = 0.5;       // an infeasible start when V > 2
        std::vector<double> x(n), sd(n), y(nb), fo(s.V), yc((size_t)s.V * nb);
        double c, c0;
        int32_t na, inf;
        rmh_pixel(s.V, s.Fs, s.Fl, s.masked ? s.active : nullptr, s.fit, 0.0, 1.0, nb, base.data(), free_cols, lo.data(), hi.data(), 1e-3,
                  1e-2, 4, obs.data(), px % 2 ? w.data() : nullptr, frac.data(), px == 2 ? mu.data() : nullptr,
                  px == 2 ? pw.data() : nullptr, x.data(), sd.data(), &c, &c0, &na, y.data(), fo.data(), yc.data(), &inf);
        for (double v : x) sum += v;
        if (std::isfinite(c)) sum += c;
        ++fits;
      }
  std::printf("refine_mix_host: %d fits, checksum %.17g\n", fits, sum);
  return 0;
}
#endif
