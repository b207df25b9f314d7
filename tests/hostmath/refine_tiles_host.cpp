// TEST INFRASTRUCTURE ONLY (tests/test_refine_tiles_host.py): part 1 of csrc/spart_refine_tiles.h -- the index maps, the
// per-pixel elimination pieces and the small per-tile solves -- and one tile's step built from them and from the per-entry
// functions of csrc/spart_refine.h the way the kernels build it (the per-pixel pieces, then the ordered walk over the tile's
// live pixels), for a g++ build with -ffp-contract=off.  Every array dense (stride 1); a tile has at most 4096 pixels.
#include <cstdint>
#include <vector>

#include "../../spart-python_amd/csrc/spart_refine_tiles.h"

using namespace spart;

extern "C" {

int rth_max_tile() { return TILES_MAXG; }
int64_t rth_chunk(int F) { return tiles_chunk(F); }

// sol[f] of the F names, name[q] of the F solve indices, and the pairs of the packed triangle
void rth_maps(int Fs, int Fl, int32_t* sol, int32_t* name, int32_t* pa, int32_t* pb) {
  const int F = Fs + Fl;
  for (int f = 0; f < F; ++f) {
    sol[f] = tiles_sol(f, Fs, Fl);
    name[f] = tiles_name(f, Fs, Fl);
  }
  for (int e = 0; e < refine_ntri(F); ++e) {
    int a, b;
    refine_pair(e, &a, &b);
    pa[e] = a, pb[e] = b;
  }
}

double rth_clip(double v, double lo, double hi) { return refine_clip(v, lo, hi); }
double rth_step(double t, double h, double hi) { return refine_fd_step(t, h, hi); }
double rth_lambda(double lam, int accept) { return refine_lambda(lam, accept != 0); }

// c_m: the band loop on Y0 (nb,), then the local prior loop (pmu / ppw NULL or (Fl,))
double rth_pixel_cost(int nb, int Fl, const double* Y0, const double* obs, const double* w, const double* lt, const double* pmu,
                      const double* ppw, int32_t* bad) {
  const double one = 1.0;                  // (no weights: every band reads this one, stride 0)
  bool b = false;
  double c = refine_tile_cost(0.0, &b, nb, w ? w : &one, w ? 1 : 0, Y0, 1, obs, 1);
  if (ppw) c = refine_prior_total(Fl, c, &b, lt, pmu, ppw);
  *bad = b ? 1 : 0;
  return c;
}

// the packed sums of one pixel in solve order, entry by entry as k_tiles_normal forms them: Y (F + 1, nb), sh per NAME, then
// the local prior's part at the accepted locals l
void rth_pixel_sums(int F, int Fs, int nb, const double* Y, const double* obs, const double* w, const double* sh, const double* l,
                    const double* pmu, const double* ppw, double* packed) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F;
  for (int e = 0; e < P; ++e) {
    int qa, qb = -1;
    if (e < nt) refine_pair(e, &qa, &qb);
    else qa = e - nt;
    const int fa = tiles_name(qa, Fs, Fl), fb = qb >= 0 ? tiles_name(qb, Fs, Fl) : 0;
    double acc = 0.0;
    for (int j = 0; j < nb; ++j) {
      const double wj = w ? w[j] : 1.0;
      if (wj == 0.0) continue;
      const double y = Y[j];
      const double ja = refine_jacobian(Y[(fa + 1) * nb + j], y, sh[fa]);
      const double jb = qb >= 0 ? refine_jacobian(Y[(fb + 1) * nb + j], y, sh[fb]) : refine_residual(y, obs[j]);
      acc = refine_mac(acc, wj, ja, jb);
    }
    if (ppw && qa < Fl && (qb == qa || qb < 0)) {
      const double p = ppw[qa];
      if (p != 0.0) acc = qb >= 0 ? acc + p : refine_prior_gain(acc, p, refine_residual(l[qa], pmu[qa]));
    }
    packed[e] = acc;
  }
}

// C: the ordered sum over the live pixels, then the shared prior loop
double rth_tile_cost(int G, const int32_t* live, const double* c, int Fs, const double* zt, const double* smu, const double* spw,
                     int32_t* bad, int32_t* any) {
  double C = 0.0;
  *bad = *any = 0;
  for (int m = 0; m < G; ++m)
    if (live[m]) {
      C = C + c[m];
      *any = 1;
    }
  bool b = false;
  if (spw) C = refine_prior_total(Fs, C, &b, zt, smu, spw);
  *bad = b ? 1 : 0;
  return C;
}

// S and gs of an accepted tile from its pixels' packed sums Ap (G, P), then the shared prior at the accepted z
void rth_tile_sums(int G, const int32_t* live, const double* Ap, int F, int Fs, const double* z, const double* smu, const double* spw,
                   double* St) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs);
  for (int e = 0; e < nts + Fs; ++e) {
    int a, b = -1;
    if (e < nts) refine_pair(e, &a, &b);
    else a = e - nts;
    const int at = b >= 0 ? refine_tri(Fl + a, Fl + b) : nt + Fl + a;
    double acc = 0.0;
    for (int m = 0; m < G; ++m)
      if (live[m]) acc = acc + Ap[m * P + at];
    if (spw && (b == a || b < 0) && spw[a] != 0.0)
      acc = b >= 0 ? acc + spw[a] : refine_prior_gain(acc, spw[a], refine_residual(z[a], smu[a]));
    St[e] = acc;
  }
}

// the eliminated form Lp (G, P) of the tile's pixels and the shared factor with the walked right-hand side (Ps); false at a
// failed pivot anywhere
static bool tile_factor(int G, const int32_t* live, const double* Ap, const double* St, int F, int Fs, double lam, bool damp,
                        std::vector<double>& Lp, double* sh) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs), Ps = nts + Fs;
  bool ok = true;
  Lp.assign(Ap, Ap + (size_t)G * P);
  for (int m = 0; m < G; ++m) {
    if (!live[m]) continue;
    double* L = Lp.data() + (size_t)m * P;
    if (damp)
      for (int j = 0; j < Fl; ++j) {
        const double v = L[refine_tri(j, j)];
        L[refine_tri(j, j)] = v + lam * (v > 0.0 ? v : 1.0);
      }
    if (!tiles_eliminate(F, Fl, L, 1)) ok = false;
    else if (damp) tiles_local_forward(Fl, L, 1, L + nt, 1, L + nt, 1);
  }
  for (int e = 0; e < Ps; ++e) {
    int a, b = -1;
    if (e < nts) refine_pair(e, &a, &b);
    else a = e - nts;
    double acc = St[e];
    if (b == a && damp) acc = acc + lam * (acc > 0.0 ? acc : 1.0);
    if (b < 0) acc = -acc;
    int oa, ob;
    tiles_schur_offsets(e, F, Fs, Fl, &oa, &ob);
    if (b >= 0 || damp)
      for (int m = 0; m < G; ++m)
        if (live[m]) acc = tiles_schur_pixel(acc, oa, ob, Fl, Lp.data() + (size_t)m * P);
    sh[e] = acc;
  }
  if (!tiles_shared_factor(Fs, sh)) ok = false;
  return ok;
}

// the next trial of a tile: z (Fs), l (G, Fl) the accepted point, lo / hi per name -> zt, lt
void rth_tile_propose(int G, const int32_t* live, const double* Ap, const double* St, int F, int Fs, double lam, const double* z,
                      const double* l, const double* lo, const double* hi, double* zt, double* lt) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F, nts = refine_ntri(Fs);
  std::vector<double> Lp;
  double sh[REFINE_MAXF * (REFINE_MAXF + 1) / 2 + REFINE_MAXF];
  bool ok = tile_factor(G, live, Ap, St, F, Fs, lam, true, Lp, sh);
  if (ok) ok = tiles_shared_solve(Fs, sh, sh + nts);
  if (ok)
    for (int m = 0; m < G; ++m) {
      if (!live[m]) continue;
      double* L = Lp.data() + (size_t)m * P;
      tiles_local_back(Fs, Fl, L, 1, sh + nts, 1, L + nt, 1);
      for (int j = 0; j < Fl; ++j)
        if (!(L[nt + j] - L[nt + j] == 0.0)) ok = false;
    }
  for (int a = 0; a < Fs; ++a) zt[a] = refine_clip(z[a] + (ok ? sh[nts + a] : 0.0), lo[a], hi[a]);
  for (int m = 0; m < G; ++m) {
    if (!live[m]) continue;
    for (int j = 0; j < Fl; ++j)
      lt[m * Fl + j] = refine_clip(l[m * Fl + j] + (ok ? Lp[(size_t)m * P + nt + j] : 0.0), lo[Fs + j], hi[Fs + j]);
  }
}

// every std of a tile from the undamped sums (NaN at a failed factorisation; the rows of dead pixels are left alone)
void rth_tile_std(int G, const int32_t* live, const double* Ap, const double* St, int F, int Fs, double* shared_std, double* local_std) {
  const int Fl = F - Fs, nt = refine_ntri(F), P = nt + F;
  std::vector<double> Lp;
  double sh[REFINE_MAXF * (REFINE_MAXF + 1) / 2 + REFINE_MAXF], z[REFINE_MAXF];
  const bool ok = tile_factor(G, live, Ap, St, F, Fs, 0.0, false, Lp, sh);
  for (int f = 0; f < Fs; ++f) shared_std[f] = ok ? tiles_shared_std(Fs, f, sh, z) : __builtin_nan("");
  for (int m = 0; m < G; ++m) {
    if (!live[m]) continue;
    for (int j = 0; j < Fl; ++j)
      local_std[m * Fl + j] = ok ? tiles_local_std(Fs, Fl, j, Lp.data() + (size_t)m * P, 1, sh, 1, z, 1) : __builtin_nan("");
  }
}

}  // extern "C"
