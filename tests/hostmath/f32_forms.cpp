// TEST INFRASTRUCTURE ONLY (tests/test_f32_forms.py): the float32 forms of the band arithmetic in csrc/spart_math.h against
// their float64 forms, and the common-case sample loop's leaf / film terms against the general ones, on the CPU.
#include <cstdint>
#include <cstring>

#include "../../spart-python_amd/csrc/spart_math.h"

using namespace spart;

template <typename T> static BandTab<T> tab_at(const double* tab, int i) {
  BandTab<T> t;
  t.kab = (T)tab[TAB_KAB * NWL + i]; t.kca = (T)tab[TAB_KCA * NWL + i]; t.kdm = (T)tab[TAB_KDM * NWL + i];
  t.kw = (T)tab[TAB_KW * NWL + i]; t.ks = (T)tab[TAB_KS * NWL + i]; t.kant = (T)tab[TAB_KANT * NWL + i];
  t.kcbc = (T)tab[TAB_CBC * NWL + i]; t.kprot = (T)tab[TAB_PROT * NWL + i]; t.talf = (T)tab[TAB_TALF * NWL + i];
  t.t12 = (T)tab[TAB_T12 * NWL + i]; t.t21 = (T)tab[TAB_T21 * NWL + i]; t.g0 = (T)tab[TAB_GSV0 * NWL + i];
  t.g1 = (T)tab[TAB_GSV1 * NWL + i]; t.g2 = (T)tab[TAB_GSV2 * NWL + i]; t.cbac = (T)tab[TAB_CBAC * NWL + i];
  t.pw = (T)tab[TAB_PW * NWL + i]; t.rw = (T)tab[TAB_RW * NWL + i];
  return t;
}

extern "C" {

// soil (B, NWL, 2): the float32 wet-soil reflectance and the float64 one from the SAME float32 inputs (prelude constants and
// tables rounded to float32, then widened): the difference is the error of the float32 arithmetic alone
void f32_soil(int64_t B, const double* tab, const double* P, double* out) {
  for (int64_t s = 0; s < B; ++s) {
    float c[NCONST];
    double a[NATM], li[NLINCL];
    sample_prelude<float, true>(P + s * NPARAM, 0.01, 0.01, PRE_ALL, c, a, li);
    for (int i = 0; i < NWL; ++i) {
      const BandTab<float> tf = tab_at<float>(tab, i);
      BandTab<double> td;
      td.kw = tf.kw; td.cbac = tf.cbac; td.pw = tf.pw; td.rw = tf.rw;
      const float rdry = soil_dry<float>(tf, c[C_F1], c[C_F2], c[C_F3]);
      float fm[7];
      double fmd[7];
      for (int k = 0; k < 7; ++k) fmd[k] = fm[k] = c[C_FM0 + k];
      float rf;
      double rd;
      soil_band<float>(tf, rdry, c[C_WET], fm, c[C_FMSUM], c[C_FILM2L], rf);
      soil_band<double>(td, rdry, c[C_WET], fmd, c[C_FMSUM], c[C_FILM2L], rd);
      out[(s * NWL + i) * 2] = rf;
      out[(s * NWL + i) * 2 + 1] = rd;
    }
  }
}

// the common-case body's leaf and film terms against the general body's, for samples with cbc = prot = 0: returns the number
// of (sample, band) pairs whose refl / tran / absb / K or wet-soil reflectance differ in any bit (0 expected)
int64_t f32_common_body_mismatches(int64_t B, const double* tab, const double* P) {
  int64_t bad = 0;
  for (int64_t s = 0; s < B; ++s) {
    float c[NCONST];
    double a[NATM], li[NLINCL];
    sample_prelude<float, true>(P + s * NPARAM, 0.01, 0.01, PRE_ALL, c, a, li);
    for (int i = 0; i < NWL; ++i) {
      const BandTab<float> tb = tab_at<float>(tab, i);
      float g[4], f[4];
      leaf_band<float>(tb, c[C_CAB], c[C_CCA], c[C_CDM], c[C_CW], c[C_CS], c[C_CANT], c[C_CBC], c[C_PROT], c[C_NM1], g[0], g[1], g[2], g[3]);
      leaf_band<float, false>(tb, c[C_CAB], c[C_CCA], c[C_CDM], c[C_CW], c[C_CS], c[C_CANT], c[C_CBC], c[C_PROT], c[C_NM1], f[0], f[1], f[2],
                              f[3]);
      const float rdry = soil_dry<float>(tb, c[C_F1], c[C_F2], c[C_F3]);
      float fm[7] = {c[C_FM0], c[C_FM1], c[C_FM2], c[C_FM3], c[C_FM4], c[C_FM5], c[C_FM6]};
      float rg, rf;
      soil_band<float>(tb, rdry, c[C_WET], fm, c[C_FMSUM], c[C_FILM2L], rg);
      const float tw1 = soil_tw1<float>(tb, c[C_FILM2L]);
      soil_band_tw<float>(tb, rdry, c[C_WET], fm, c[C_FMSUM], tw1, rf);
      if (std::memcmp(g, f, sizeof(g)) != 0 || std::memcmp(&rg, &rf, sizeof(rg)) != 0) ++bad;
    }
  }
  return bad;
}

}  // extern "C"
