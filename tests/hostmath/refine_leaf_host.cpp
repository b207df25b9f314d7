// TEST INFRASTRUCTURE ONLY (tests/test_refine_leaf_host.py): a stand-alone g++ build (-ffp-contract=off) of part 1 of
// csrc/spart_refine_leaf.h.
//   refine_leaf_host spectra IN OUT    rows in, leaf_band<double> spectra out: the forward model of tools/refine_leaf_defined.py
//   refine_leaf_host fit IN OUT        the whole fit of every leaf, the 64 lanes of a wave run as a loop
// IN and OUT are raw little-endian files: int64 header words, then float64 arrays, in the order read below.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spart-python_amd/csrc/spart_refine_leaf.h"

using namespace spart;

static void die(const char* what) {
  std::fprintf(stderr, "refine_leaf_host: %s\n", what);
  std::exit(2);
}

struct Reader {
  FILE* f;
  int64_t word() {
    int64_t v;
    if (std::fread(&v, 8, 1, f) != 1) die("short input (header)");
    return v;
  }
  std::vector<double> block(size_t n) {
    std::vector<double> v(n);
    if (n && std::fread(v.data(), 8, n, f) != n) die("short input (array)");
    return v;
  }
};

static void put(FILE* f, const std::vector<double>& v) {
  if (!v.empty() && std::fwrite(v.data(), 8, v.size(), f) != v.size()) die("cannot write");
}

// the leaf rows of the device table block from the raw tables (nr, Kab, Kca, Kdm, Kw, Ks, Kant, cbc, prot), as
// spart_ctx_create derives them; the soil rows stay 0
static std::vector<double> leaf_tab(Reader& in) {
  const std::vector<double> raw = in.block((size_t)9 * NWL);
  std::vector<double> tab((size_t)NTAB * NWL, 0.0);
  const int rows[8] = {TAB_KAB, TAB_KCA, TAB_KDM, TAB_KW, TAB_KS, TAB_KANT, TAB_CBC, TAB_PROT};
  for (int i = 0; i < NWL; ++i) {
    for (int k = 0; k < 8; ++k) tab[(size_t)rows[k] * NWL + i] = raw[(size_t)(k + 1) * NWL + i];
    const double nr = raw[i], t12 = calculate_tav(90, nr);
    tab[(size_t)TAB_TALF * NWL + i] = calculate_tav(40, nr);
    tab[(size_t)TAB_T12 * NWL + i] = t12;
    tab[(size_t)TAB_T21 * NWL + i] = t12 / (nr * nr);
  }
  return tab;
}

static BandTab<double> tab_at(const std::vector<double>& tab, int i) {
  BandTab<double> t;
  std::memset(&t, 0, sizeof(t));
  t.kab = tab[(size_t)TAB_KAB * NWL + i];
  t.kca = tab[(size_t)TAB_KCA * NWL + i];
  t.kdm = tab[(size_t)TAB_KDM * NWL + i];
  t.kw = tab[(size_t)TAB_KW * NWL + i];
  t.ks = tab[(size_t)TAB_KS * NWL + i];
  t.kant = tab[(size_t)TAB_KANT * NWL + i];
  t.kcbc = tab[(size_t)TAB_CBC * NWL + i];
  t.kprot = tab[(size_t)TAB_PROT * NWL + i];
  t.talf = tab[(size_t)TAB_TALF * NWL + i];
  t.t12 = tab[(size_t)TAB_T12 * NWL + i];
  t.t21 = tab[(size_t)TAB_T21 * NWL + i];
  return t;
}

static int run_spectra(Reader& in, FILE* out) {
  const int64_t R = in.word();
  const std::vector<double> tab = leaf_tab(in), rows = in.block((size_t)R * LEAF_NPAR);
  std::vector<double> refl((size_t)R * NWL), tran((size_t)R * NWL);
  for (int64_t r = 0; r < R; ++r) {
    double lc[LEAF_NC];
    leaf_row_constants(rows.data() + r * LEAF_NPAR, lc);
    for (int i = 0; i < NWL; ++i) leaf_row_band(tab_at(tab, i), lc, refl[(size_t)r * NWL + i], tran[(size_t)r * NWL + i]);
  }
  put(out, refl);
  put(out, tran);
  return 0;
}

struct FitIn {
  int64_t M, n_iter, has_r, has_t, wmode_r, wmode_t, pmode;      // modes: 0 none, 1 one row for all, 2 one row per leaf
  std::vector<double> tab, leaf, lo, hi, h, obs_r, obs_t, w_r, w_t, pmu, ppw;
  std::vector<int32_t> free_col;
  double lambda0;
};
struct FitOut {
  std::vector<double> x, cost, cost0, sdev, na;
};

// one leaf, as k_refine_leaf<F> runs it
template <int F> static void fit_leaf(const FitIn& a, int64_t m, FitOut& o) {
  constexpr int NT = LeafPartial<F>::NT, P = LeafPartial<F>::P;
  double rows[(F + 1) * LEAF_NPAR], lc[(F + 1) * LEAF_NC], x[F], t[F], sh[F], A[P], An[P], L[NT], d[F], sdev[F];
  for (int e = 0; e < P; ++e) A[e] = 0.0;
  const double* base = a.leaf.data() + m * LEAF_NPAR;
  const double* or_m = a.has_r ? a.obs_r.data() + m * NWL : nullptr;
  const double* ot_m = a.has_t ? a.obs_t.data() + m * NWL : nullptr;
  const double* wr_m = a.wmode_r ? a.w_r.data() + (a.wmode_r == 2 ? m * NWL : 0) : nullptr;
  const double* wt_m = a.wmode_t ? a.w_t.data() + (a.wmode_t == 2 ? m * NWL : 0) : nullptr;
  const double* mu = a.pmode ? a.pmu.data() + (a.pmode == 2 ? m * F : 0) : nullptr;
  const double* pw = a.pmode ? a.ppw.data() + (a.pmode == 2 ? m * F : 0) : nullptr;
  LeafFit fit;
  leaf_fit_start(F, base, a.free_col.data(), a.lo.data(), a.hi.data(), a.lambda0, x, t, &fit);
  static LeafPartial<F> lanes[LEAF_LANES];
  double Jrow[2 * F];
  for (int it = 0; it <= (int)a.n_iter; ++it) {
    leaf_fit_steps(F, t, a.h.data(), a.hi.data(), sh);
    for (int f = 0; f <= F; ++f) {
      leaf_fit_row(F, f, base, a.free_col.data(), t, sh, rows + f * LEAF_NPAR);
      leaf_row_constants(rows + f * LEAF_NPAR, lc + f * LEAF_NC);
    }
    for (int l = 0; l < LEAF_LANES; ++l) {
      leaf_partial_zero(lanes[l]);
      for (int pass = 0; pass < LEAF_PASSES; ++pass) {
        const int i = pass * LEAF_LANES + l;
        if (i >= NWL) continue;
        double wr = 0.0, obr = 0.0, wt = 0.0, obt = 0.0;
        if (a.has_r) wr = wr_m ? wr_m[i] : 1.0, obr = or_m[i];
        if (a.has_t) wt = wt_m ? wt_m[i] : 1.0, obt = ot_m[i];
        leaf_partial_band<F>(lanes[l], [&]() { return tab_at(a.tab, i); }, lc, sh, a.has_r != 0, wr, obr, a.has_t != 0, wt, obt, Jrow, 1);
      }
    }
    leaf_join_lanes<F>(lanes);
    for (int e = 0; e < P; ++e) An[e] = lanes[0].s[e];
    const int code = leaf_fit_update(F, it, it == (int)a.n_iter, &fit, lanes[0].c, lanes[0].bad != 0, An, A, x, t, a.lo.data(),
                                     a.hi.data(), mu, pw, L, d);
    if (code == 2) break;
  }
  leaf_fit_std(F, &fit, A, L, d, sdev);
  for (int f = 0; f < F; ++f) o.x[m * F + f] = x[f], o.sdev[m * F + f] = sdev[f];
  o.cost[m] = fit.cost;
  o.cost0[m] = fit.cost0;
  o.na[m] = fit.na;
}

template <int F> static void fit_all(int Fr, const FitIn& a, FitOut& o) {
  if constexpr (F <= LEAF_MAXF) {
    if (Fr != F) return fit_all<F + 1>(Fr, a, o);
    for (int64_t m = 0; m < a.M; ++m) fit_leaf<F>(a, m, o);
  }
}

static int run_fit(Reader& in, FILE* out) {
  FitIn a;
  a.M = in.word();
  const int64_t F = in.word();
  a.n_iter = in.word(), a.has_r = in.word(), a.has_t = in.word(), a.wmode_r = in.word(), a.wmode_t = in.word(), a.pmode = in.word();
  if (a.M < 0 || F < 1 || F > LEAF_MAXF || a.n_iter < 0 || a.n_iter > REFINE_MAX_ITER) die("bad sizes");
  a.tab = leaf_tab(in);
  a.leaf = in.block((size_t)a.M * LEAF_NPAR);
  for (double c : in.block((size_t)F)) {
    if (!(c >= 0 && c < LEAF_NPAR)) die("bad free column");
    a.free_col.push_back((int32_t)c);
  }
  a.lo = in.block((size_t)F);
  a.hi = in.block((size_t)F);
  const std::vector<double> opt = in.block(2);                     // rel_step, lambda0
  a.lambda0 = opt[1];
  for (int f = 0; f < F; ++f) a.h.push_back(opt[0] * (a.hi[f] - a.lo[f]));
  auto rows = [&](int64_t mode, size_t width) { return in.block(mode == 0 ? 0 : mode == 1 ? width : (size_t)a.M * width); };
  a.obs_r = rows(a.has_r ? 2 : 0, NWL);
  a.obs_t = rows(a.has_t ? 2 : 0, NWL);
  a.w_r = rows(a.wmode_r, NWL);
  a.w_t = rows(a.wmode_t, NWL);
  a.pmu = rows(a.pmode, (size_t)F);
  a.ppw = rows(a.pmode, (size_t)F);
  FitOut o;
  o.x.resize((size_t)a.M * F), o.sdev.resize((size_t)a.M * F), o.cost.resize(a.M), o.cost0.resize(a.M), o.na.resize(a.M);
  fit_all<1>((int)F, a, o);
  put(out, o.x);
  put(out, o.cost);
  put(out, o.cost0);
  put(out, o.sdev);
  put(out, o.na);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) die("usage: refine_leaf_host spectra|fit IN OUT");
  FILE* fi = std::fopen(argv[2], "rb");
  FILE* fo = std::fopen(argv[3], "wb");
  if (!fi || !fo) die("cannot open a file");
  Reader in = {fi};
  int rc;
  if (!std::strcmp(argv[1], "spectra")) rc = run_spectra(in, fo);
  else if (!std::strcmp(argv[1], "fit")) rc = run_fit(in, fo);
  else die("unknown mode");
  std::fclose(fi);
  if (std::fclose(fo) != 0) die("cannot write");
  return rc;
}
