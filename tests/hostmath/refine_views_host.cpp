// TEST INFRASTRUCTURE ONLY (tests/test_refine_views_host.py): the index maps of spart_refine_views (csrc/spart_refine_views.h,
// part 1) and one pixel's step built from them and from the per-entry functions of csrc/spart_refine.h the way
// k_refine_views_step builds it -- 16-band tiles over the virtual bands, every packed sum over the part of a tile where its
// unknowns are active -- for a g++ build with -ffp-contract=off.  Every array dense (stride 1).
#include <cstdint>

#include "../../spart-python_amd/csrc/spart_refine_views.h"

using namespace spart;

extern "C" {

int rvh_max_v() { return VIEWS_MAXV; }
int64_t rvh_chunk(int V, int F) { return views_chunk(V, F); }

// name[a], view[a] of the n unknowns; unknown[v F + f]
void rvh_maps(int V, int Fs, int Fl, int32_t* name, int32_t* view, int32_t* unknown) {
  const int n = Fs + V * Fl, F = Fs + Fl;
  for (int a = 0; a < n; ++a) {
    name[a] = views_name(a, Fs, Fl);
    view[a] = views_view(a, Fs, Fl);
  }
  for (int v = 0; v < V; ++v)
    for (int f = 0; f < F; ++f) unknown[v * F + f] = views_unknown(v, f, Fs, Fl);
}

// the clipped start and the per-unknown lo / hi / h: base (V, 27) of one pixel, free / lo / hi / h per name
void rvh_start(int V, int Fs, int Fl, const double* base, const int32_t* free_cols, const double* lo, const double* hi, const double* h,
               double* x, double* lo_n, double* hi_n, double* h_n) {
  for (int a = 0; a < Fs + V * Fl; ++a) {
    const int f = views_name(a, Fs, Fl), v = views_view(a, Fs, Fl);
    lo_n[a] = lo[f];
    hi_n[a] = hi[f];
    h_n[a] = h[f];
    x[a] = refine_clip(base[(v < 0 ? 0 : v) * 27 + free_cols[f]], lo[f], hi[f]);
  }
}

// the steps sh (n,) and the V (F + 1) rows of the trial t, as (V, F + 1, 27)
void rvh_rows(int V, int Fs, int Fl, const double* base, const int32_t* free_cols, const double* t, const double* h_n,
              const double* hi_n, double* sh, double* rows) {
  const int F = Fs + Fl;
  for (int a = 0; a < Fs + V * Fl; ++a) sh[a] = refine_fd_step(t[a], h_n[a], hi_n[a]);
  for (int v = 0; v < V; ++v)
    for (int fp = 0; fp <= F; ++fp) {
      double* row = rows + (v * (F + 1) + fp) * 27;
      for (int p = 0; p < 27; ++p) row[p] = base[v * 27 + p];
      for (int f = 0; f < F; ++f) {
        const int a = views_unknown(v, f, Fs, Fl);
        row[free_cols[f]] = fp == f + 1 ? t[a] + sh[a] : t[a];
      }
    }
}

// the trial cost over the virtual bands: Y (V, F + 1, nb), obs (V nb,), w NULL, (nb,) (wper = 0) or (V nb,) (wper = 1)
double rvh_cost(int V, int F, int nb, const double* Y, const double* obs, const double* w, int wper, int32_t* bad) {
  const double one = 1.0;                  // (no weights: every band reads this one, stride 0)
  double c = 0.0;
  bool b = false;
  for (int v = 0; v < V; ++v)              // view v's bands are the virtual bands v nb ... (v + 1) nb - 1
    c = refine_tile_cost(c, &b, nb, w ? (wper ? w + v * nb : w) : &one, w ? 1 : 0, Y + (v * (F + 1)) * nb, 1, obs + v * nb, 1);
  *bad = b ? 1 : 0;
  return c;
}

// the packed sums (ntri(n) + n) of one pixel, tile by tile
void rvh_sums(int V, int Fs, int Fl, int nb, const double* Y, const double* obs, const double* w, int wper, const double* sh,
              double* packed) {
  constexpr int JT = 16;                   // REFINE_JT of the kernels; the sums do not depend on it
  const int F = Fs + Fl, n = Fs + V * Fl, U = V * nb, nt = refine_ntri(n), P = nt + n;
  double Jt[(REFINE_MAXF + 1) * JT], wl[JT], rl[JT];
  for (int e = 0; e < P; ++e) packed[e] = 0.0;
  for (int j0 = 0; j0 < U; j0 += JT) {
    const int jn = U - j0 < JT ? U - j0 : JT;
    for (int jj = 0; jj < jn; ++jj) {
      const int u = j0 + jj, v = u / nb, j = u % nb;
      wl[jj] = w ? w[wper ? u : u % nb] : 1.0;
      const double y0 = Y[(v * (F + 1)) * nb + j];
      rl[jj] = wl[jj] != 0.0 ? refine_residual(y0, obs[u]) : 0.0;
      for (int f = 1; f <= F; ++f)
        Jt[f * JT + jj] = refine_jacobian(Y[(v * (F + 1) + f) * nb + j], y0, sh[views_unknown(v, f - 1, Fs, Fl)]);
    }
    for (int e = 0; e < P; ++e) {
      int a, b;
      refine_packed_pair(e, nt, &a, &b);
      int jb = 0, je = jn;
      views_clip_range(views_view(a, Fs, Fl), nb, j0, &jb, &je);
      if (b >= 0) views_clip_range(views_view(b, Fs, Fl), nb, j0, &jb, &je);
      const double* ja = Jt + (views_name(a, Fs, Fl) + 1) * JT;
      const double* jc = b >= 0 ? Jt + (views_name(b, Fs, Fl) + 1) * JT : rl;
      packed[e] = refine_tile_sum(packed[e], jb, je, wl, 1, ja, 1, jc, 1);
    }
  }
}

// the prior's terms: cost, then the additions to the accepted sums
double rvh_prior_cost(int n, double c, const double* t, const double* mu, const double* pw, int32_t* bad) {
  bool b = false;
  c = refine_prior_total(n, c, &b, t, mu, pw);
  if (b) *bad = 1;
  return c;
}

void rvh_prior_normal(int n, double* packed, const double* x, const double* mu, const double* pw) {
  refine_prior_augment(n, packed, 1, x, 1, mu, pw);
}

double rvh_lambda(double lam, int accept) { return refine_lambda(lam, accept != 0); }

void rvh_propose(int n, const double* packed, double lam, const double* x, const double* lo, const double* hi, double* t) {
  double L[REFINE_MAXF * (REFINE_MAXF + 1) / 2], d[REFINE_MAXF];
  refine_propose(n, packed, 1, lam, x, 1, lo, hi, L, 1, d, 1, t, 1);
}

void rvh_std(int n, const double* packed, double* out) {
  double L[REFINE_MAXF * (REFINE_MAXF + 1) / 2], z[REFINE_MAXF];
  refine_std(n, packed, 1, L, 1, z, 1, out, 1);
}

}  // extern "C"
