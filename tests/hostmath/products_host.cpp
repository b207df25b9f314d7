// TEST INFRASTRUCTURE ONLY (tests/test_products_host.py): canopy_flux and products_band of csrc/spart_products.h beside
// canopy_band of csrc/spart_math.h, for a g++ build with -ffp-contract=off: the rsd / rdd composed from the four flux terms
// against the ones the library's canopy solve returns, band by band.  With -DPRODUCTS_MAIN the file is a stand-alone program
// for a -fsanitize=address,undefined build that is run as a child process: every buffer on the heap at its exact size.
#include <vector>

#include "hostmath.cpp"
#include "../../spart-python_amd/csrc/spart_products.h"

extern "C" {

// P (B, 27) -> out (B, 2001, 8) = rsd, rdd of canopy_band; rsd, rdd, a_s, a_d of canopy_flux + products_band; Ea-free partial
// terms are the caller's business.  Slots 6, 7: rho_dd of canopy_flux and of canopy_core.
void ph_bands(int64_t B, const double* tab, const double* P, double* out) {
  for (int64_t s = 0; s < B; ++s) {
    double c[NCONST], a[NATM], li[NLINCL];
    sample_prelude<double, false>(P + s * NPARAM, 0.01, 0.01, PRE_LEAF | PRE_SOIL | PRE_CANOPY, c, a, li);
    CanopyPar<double> cp;
    cp.sob = c[C_SOB]; cp.sof = c[C_SOF]; cp.hbf = c[C_HBF]; cp.ks = c[C_KS]; cp.ko = c[C_KO]; cp.lai = c[C_LAI]; cp.lai2 = c[C_LAI2];
    cp.tss = c[C_TSS]; cp.too = c[C_TOO]; cp.Z = c[C_Z]; cp.hot = c[C_HOT]; cp.pso2w = c[C_PSO2W];
    for (int band = 0; band < NWL; ++band) {
      const BandTab<double> tb = tab_at<double>(tab, band);
      double refl, tran, absb, K;
      leaf_band<double>(tb, c[C_CAB], c[C_CCA], c[C_CDM], c[C_CW], c[C_CS], c[C_CANT], c[C_CBC], c[C_PROT], c[C_NM1], refl, tran,
                        absb, K);
      const double rdry = soil_dry<double>(tb, c[C_F1], c[C_F2], c[C_F3]);
      double fm[7] = {c[C_FM0], c[C_FM1], c[C_FM2], c[C_FM3], c[C_FM4], c[C_FM5], c[C_FM6]};
      double rwet;
      soil_band<double>(tb, rdry, c[C_WET], fm, c[C_FMSUM], c[C_FILM2L], rwet);
      double rso, rdo, rsd, rdd;
      canopy_band<double>(cp, refl, tran, absb, rwet, rso, rdo, rsd, rdd);
      const CanopyCore<double> core = canopy_core<double>(cp, refl, tran, absb);
      const CanopyFlux<double> fl = canopy_flux<double>(cp, refl, tran, absb);
      double* o = out + ((size_t)s * NWL + band) * 8;
      o[0] = rsd; o[1] = rdd;
      products_band<double>(cp, fl, rwet, o[2], o[3], o[4], o[5]);
      o[6] = fl.rho_dd; o[7] = core.rho_dd;
    }
  }
}

// fCover of the kernel's routine, (B,)
void ph_fcover(int64_t B, const double* P, double* out) {
  for (int64_t s = 0; s < B; ++s) out[s] = products_fcover(P[s * NPARAM + 15], P[s * NPARAM + 16], P[s * NPARAM + 17]);
}

}  // extern "C"

#if defined(PRODUCTS_MAIN)
#include <cmath>
#include <cstdio>

// flat synthetic tables (no file is read): enough to walk every line of the band chain with in-range values
int main() {
  std::vector<double> tab((size_t)NTAB * NWL);
  for (int i = 0; i < NWL; ++i) {
    const double x = (double)i / (NWL - 1);
    tab[TAB_KAB * NWL + i] = 0.05 * (1.0 - x); tab[TAB_KCA * NWL + i] = 0.02 * (1.0 - x); tab[TAB_KDM * NWL + i] = 5.0 + 20.0 * x;
    tab[TAB_KW * NWL + i] = 40.0 * x * x; tab[TAB_KS * NWL + i] = 0.1 * (1.0 - x); tab[TAB_KANT * NWL + i] = 0.01 * (1.0 - x);
    tab[TAB_CBC * NWL + i] = 10.0 * x; tab[TAB_PROT * NWL + i] = 10.0 * x;
    tab[TAB_TALF * NWL + i] = 0.95; tab[TAB_T12 * NWL + i] = 0.90; tab[TAB_T21 * NWL + i] = 0.45;
    tab[TAB_GSV0 * NWL + i] = 0.3 + 0.2 * x; tab[TAB_GSV1 * NWL + i] = 0.05 * x; tab[TAB_GSV2 * NWL + i] = -0.02 * x;
    tab[TAB_CBAC * NWL + i] = 0.85; tab[TAB_PW * NWL + i] = 0.45; tab[TAB_RW * NWL + i] = 0.03;
  }
  const double rows[4][4] = {{3.0, 40.0, 20.0, -0.35}, {1e-6, 0.0, 60.0, 0.5}, {8.0, 60.0, 5.0, -0.5}, {0.01, 30.0, 55.0, 0.0}};   // LAI, tts, SMp, LIDFa
  const int B = 4;
  std::vector<double> P((size_t)B * NPARAM), out((size_t)B * NWL * 8), fc(B);
  for (int s = 0; s < B; ++s) {
    const double d[NPARAM] = {40, 0.01, 0.02, 0, 10, 10, 1.5, 0, 0, 0.5, 0, 100, rows[s][2], 25, 0.015, rows[s][0], rows[s][3], -0.15, 0.05,
                              rows[s][1], 0, 0, 0.325, 0.35, 1.41, 1013.25, 100};
    for (int i = 0; i < NPARAM; ++i) P[(size_t)s * NPARAM + i] = d[i];
  }
  ph_bands(B, tab.data(), P.data(), out.data());
  ph_fcover(B, P.data(), fc.data());
  int failures = 0;
  for (int s = 0; s < B; ++s) {
    double worst = 0.0;
    bool finite = std::isfinite(fc[s]);
    for (int i = 0; i < NWL; ++i) {
      const double* o = out.data() + ((size_t)s * NWL + i) * 8;
      for (int q = 0; q < 8; ++q) finite = finite && std::isfinite(o[q]);
      for (int q = 0; q < 2; ++q) worst = std::fmax(worst, std::fabs(o[2 + q] - o[q]) / std::fmax(std::fabs(o[q]), 1e-2));
    }
    const bool ok = finite && worst < 1e-9;
    std::printf("row %d: worst rel diff %.3e fCover %.6e %s\n", s, worst, fc[s], ok ? "ok" : "WRONG");
    failures += ok ? 0 : 1;
  }
  return failures ? 1 : 0;
}
#endif  // PRODUCTS_MAIN
