// TEST INFRASTRUCTURE ONLY (tests/test_diet3_forms.py): SAILH's J2 under the band kernel's per-stage vote (sail_j2_possible,
// csrc/spart_math.h) against a copy of the form it replaced, bit for bit, on the CPU.
#include <cmath>
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

// the same bits, or both NaN (the forms under test run the same operations on a NaN: no payload is asked for)
static bool same(float a, float b) { return std::memcmp(&a, &b, sizeof(a)) == 0 || (std::isnan(a) && std::isnan(b)); }

// the replaced form, kept here as the reference: J2 with its test issued for every band
static float old_sail_j2_d(float L, float tk, float e1, float kpm, float ikpm) {
  float d = kpm * L;
  float v = (1.0f - tk * e1) * ikpm;
  if (d < SailJ<float>::THRESH) v = L * SailJ<float>::poly(d);
  return v;
}

extern "C" {

// Every (sample, band) of P (B, 27) x 2001 bands.  flags[s]: bit 0 = the sample's C_KSL row is NaN, bit 1 = its C_KOL row
// is NaN.  out[0] cases, out[1] J2 values (either of the two) that differ between the old form and the new one under the
// vote's bit, out[2] cases on the Taylor side of either J2 by the OLD form's own test, out[3] cases whose bit lets the
// test be skipped, out[4] canopy_core_l results that differ with and without the bit
void diet3_compare(int64_t B, const double* tab, const double* P, const int32_t* flags, int64_t* out) {
  for (int i = 0; i < 5; ++i) out[i] = 0;
  for (int64_t s = 0; s < B; ++s) {
    float c[NCONST];
    double a[NATM], li[NLINCL];
    sample_prelude<float, true>(P + s * NPARAM, 0.01, 0.01, PRE_ALL, c, a, li);
    if (flags[s] & 1) c[C_KSL] = NAN;
    if (flags[s] & 2) c[C_KOL] = NAN;
    // the stage vote of k_bands, for this sample
    const bool j2_bit = sail_j2_possible(c[C_KSL], c[C_LAI]) || sail_j2_possible(c[C_KOL], c[C_LAI]);
    CanopyPar<float> cp;
    cp.sob = c[C_SOB]; cp.sof = c[C_SOF]; cp.hbf = c[C_HBF]; cp.ks = c[C_KS]; cp.ko = c[C_KO]; cp.lai = c[C_LAI];
    cp.lai2 = c[C_LAI2]; cp.tss = c[C_TSS]; cp.too = c[C_TOO]; cp.Z = c[C_Z]; cp.hot = c[C_HOT]; cp.pso2w = c[C_PSO2W];
    for (int i = 0; i < NWL; ++i) {
      const BandTab<float> tb = tab_at<float>(tab, i);
      ++out[0];
      float refl, tran, absb, K;
      leaf_band<float>(tb, c[C_CAB], c[C_CCA], c[C_CDM], c[C_CW], c[C_CS], c[C_CANT], c[C_CBC], c[C_PROT], c[C_NM1], refl, tran, absb, K);
      // J2 with the arguments canopy_core_l gives it
      const float Mn = cp.hbf * (refl - tran);
      const float m = Mx<float>::sqrt(absb * (1.0f + 2.0f * Mn));
      const float e1 = Mx<float>::exp2(-m * cp.lai2);
      const float ksm = cp.ks + m, kom = cp.ko + m;
      const float iks = Mx<float>::rcp(ksm), iko = Mx<float>::rcp(kom);
      const float o1 = old_sail_j2_d(cp.lai, cp.tss, e1, ksm, iks), o2 = old_sail_j2_d(cp.lai, cp.too, e1, kom, iko);
      const float n1 = sail_j2_d<float>(cp.lai, cp.tss, e1, ksm, iks, j2_bit), n2 = sail_j2_d<float>(cp.lai, cp.too, e1, kom, iko, j2_bit);
      if (!same(o1, n1) || !same(o2, n2)) ++out[1];
      if (ksm * cp.lai < SailJ<float>::THRESH || kom * cp.lai < SailJ<float>::THRESH) ++out[2];
      if (!j2_bit) ++out[3];
      const CanopyCore<float> k0 = canopy_core_l<float>(cp, refl, tran, absb, c[C_KSL], c[C_KOL]);
      const CanopyCore<float> k1 = canopy_core_l<float>(cp, refl, tran, absb, c[C_KSL], c[C_KOL], j2_bit);
      if (!(same(k0.rho_so, k1.rho_so) && same(k0.rho_dd, k1.rho_dd) && same(k0.tau_dd, k1.tau_dd) && same(k0.tau_sd, k1.tau_sd) &&
            same(k0.tau_do, k1.tau_do) && same(k0.rho_sd, k1.rho_sd) && same(k0.rho_do, k1.rho_do)))
        ++out[4];
    }
  }
}

}  // extern "C"
