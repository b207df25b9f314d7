// Canopy products of a parameter row: fAPAR and albedo, black- and white-sky, and fCover (spart_products; the definition
// is in include/spart_hip.h).  Two parts:
//   1. canopy_flux: the four flux terms of SAILH that do not depend on the view direction, plain SPART_HD arithmetic like
//      spart_math.h (tests/hostmath/products_host.cpp compiles it with g++);
//   2. k_products: the kernel (hipcc only).
#pragma once

#include "spart_math.h"
#if defined(__HIPCC__)
#include "spart_kernels.h"
#endif

namespace spart {

constexpr int PRODUCTS_PAR_LAST = 300;     // 400 ... 700 nm: model bands 0 ... 300

// rho_dd, tau_dd, tau_sd, rho_sd of sailh.py:205-209 from the leaf of one band.  canopy_core_l computes these four beside the
// view-direction terms (J1K / J2K, the hot spot, rho_so, tau_do, rho_do and the three-way reciprocal that also serves
// 1 / (ko + m)); this function computes none of those and reads neither ko, too, Z, hot, pso2w, sob nor sof of CanopyPar.
// The arithmetic is canopy_core_l's float64 path term by term, with two reciprocals grouped differently: 1 / (a + m) and
// 1 / (ks + m) come from one reciprocal of their product (there: of the product with ko + m as well), and 1 / d1 is its own
// reciprocal (there: shared with 1 / d2).  The results therefore differ from canopy_core_l's in the last bits only.
template <typename T> struct CanopyFlux {
  T rho_dd, tau_dd, tau_sd, rho_sd;
};

template <typename T> SPART_HD CanopyFlux<T> canopy_flux(const CanopyPar<T>& c, T rho, T tau, T absb) {
  T P = T(0.5) * (rho + tau);
  T Mn = c.hbf * (rho - tau);
  T sigb = P + Mn;                     // diffuse backscatter (:142-148)
  T a = T(1) - P + Mn;                 // 1 - sigf  (:149)
  T m = Mx<T>::sqrt(absb * (T(1) + T(2) * Mn));      // (:150), as canopy_core_l
  T apm = a + m, ksm = c.ks + m;
  T i2 = Mx<T>::rcp(apm * ksm);
  T iam = i2 * ksm;                    // 1 / (a + m)
  T iks = i2 * apm;                    // 1 / (ks + m)
  T rinf = sigb * iam;                 // (:151)
  T rinf2 = rinf * rinf;
  T omr = (absb + m) * iam;            // 1 - rinf
  T opr = T(1) + rinf;
  T omr2 = omr * opr;                  // 1 - rinf^2
  T L = c.lai;
  T e1 = Mx<T>::exp2(-m * c.lai2);     // e^-mL
  T d1 = (m - c.ks) * L;
  T d1s = (Mx<T>::fabs(d1) < SailJ<T>::THRESH) ? T(1) : d1;    // (the Taylor side needs no 1 / d)
  T J1k = sail_j1_d<T>(L, c.tss, e1, d1, Mx<T>::rcp(d1s));
  T J2k = sail_j2_d<T>(L, c.tss, e1, ksm, iks);
  T ome2 = T(1) - e1 * e1;
  T re = rinf * e1;
  T i1 = Mx<T>::rcp(omr2 * (T(1) + rinf2));  // sic: 1 / (1 - rinf2**2) (:189)
  T U = P * opr, V = Mn * omr;
  T s1 = c.ks * U - V;
  T s2 = c.ks * U + V;
  T Pss = s1 * J1k, Qss = s2 * J2k;
  CanopyFlux<T> f;
  f.tau_dd = omr2 * e1 * i1;           // :205-209
  f.rho_dd = rinf * ome2 * i1;
  f.tau_sd = (Pss - re * Qss) * i1;
  f.rho_sd = (Qss - re * Pss) * i1;
  return f;
}

// One band of the definition: rsd, rdd (sailh.py:232-233, in canopy_soil's form) and the two canopy absorptances.
template <typename T>
SPART_HD void products_band(const CanopyPar<T>& c, const CanopyFlux<T>& k, T rs, T& rsd, T& rdd, T& a_s, T& a_d) {
  T id = Mx<T>::rcp(T(1) - rs * k.rho_dd);   // 1 / d
  T g = rs * id;
  T h = g * k.tau_dd;
  T tst = c.tss + k.tau_sd;
  rsd = k.rho_sd + tst * h;
  rdd = k.rho_dd + k.tau_dd * h;
  T soil = (T(1) - rs) * id;                 // what the soil keeps of the flux that reaches it
  a_s = T(1) - rsd - soil * tst;
  a_d = T(1) - rdd - soil * k.tau_dd;
}

// fCover = 1 - exp(-LAI G), G = sum_j lidf_j cos(litab_j), j ascending, one multiplication and one addition per class
SPART_HD double products_fcover(double lai, double lidfa, double lidfb) {
  SPART_NO_CONTRACT
  double G = 0.0, prev = 0.0;
  for (int j = 0; j < NLINCL; ++j) {         // leaf_angles' loop: lidf_j = F_j - F_(j-1), consumed as it appears
    const double F = (j < NLINCL - 1) ? lidf_dcum_lit(lidfa, lidfb, j) : 1.0;
    G = G + (F - prev) * lidf_cos_litab(j);
    prev = F;
  }
  return 1.0 - ::exp(-(lai * G));
}

#if defined(__HIPCC__)

struct ProductsOut {
  double *fapar_bs, *fapar_ws, *albedo_bs, *albedo_ws, *fcover;
};

// THE PRODUCTS KERNEL.  Mapping: k_columns_srf's -- a workgroup owns 64 consecutive samples (lane = sample), the
// NCONST_USED float64 constants of the block sit in LDS ([row][64]), and the band in flight is wave-uniform, so the 17 table
// values and Ea arrive by scalar loads.  Wave w of the four walks the model bands i = w, w + 4, ... < 2001 in ascending
// order: leaf, soil, canopy_flux, products_band, then one FMA per accumulator -- Ea_i a_s, Ea_i a_d for i <= 300 and
// Ea_i rsd, Ea_i rdd for every band.  The four partial sums p_w of each quantity meet in LDS and are joined as
// (p0 + p1) + (p2 + p3) and divided by the context's float64 sums of Ea (IEEE division): ONE order whatever the batch, so a
// row's values do not depend on where it stands.  The last wave adds fCover.  The thermal evaluation takes no part.
// 72 B are read and 40 B written per sample beside the constants: the kernel is pure arithmetic.
static __global__ __launch_bounds__(64 * COL_WAVES, COLUMNS_SIMD_WAVES) void k_products(
    const double* __restrict__ tab, const double* __restrict__ cst, int64_t Bp, const double* __restrict__ Ea, double ea_par,
    double ea_all, const double* __restrict__ lidfa, const double* __restrict__ lidfb, int64_t B, ProductsOut out) {
  __shared__ double lds_c[NCONST_USED * 64];
  __shared__ double lds_p[COL_WAVES * 4 * 64];          // [wave][quantity][lane]
  stage_f64_tables();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t s = (int64_t)blockIdx.x * 64 + lane;
  const bool ok = s < B;
  const int64_t sc = ok ? s : B - 1;                    // (lanes past the end repeat the last sample and store nothing)
  for (int i = wave; i < NCONST_USED; i += COL_WAVES) lds_c[i * 64 + lane] = cst[(int64_t)i * Bp + sc];
  __syncthreads();
  if (out.fapar_bs || out.fapar_ws || out.albedo_bs || out.albedo_ws) {     // (kernel-uniform)
    double f_bs = 0.0, f_ws = 0.0, al_bs = 0.0, al_ws = 0.0;
#pragma unroll 1
    for (int i = wave; i < NWL; i += COL_WAVES) {
      // The sample's constants are read from LDS inside the loop, band by band, through an offset the compiler cannot see
      // through: hoisted out of the loop as invariants they would be some 40 live registers more (k_columns_srf).
      int lo = lane;
      SPART_KEEP_BRANCH(lo);
      const LdsCol<double> c{lds_c + lo};
      const double ea = Ea[i];
      const BandTab<double> tb = load_tab(tab, i);
      double refl, tran, absb, K;
      leaf_band<double>(tb, c[C_CAB], c[C_CCA], c[C_CDM], c[C_CW], c[C_CS], c[C_CANT], c[C_CBC], c[C_PROT], c[C_NM1], refl,
                        tran, absb, K);
      CanopyPar<double> cp;                             // (what canopy_flux and products_band read; the rest is not loaded)
      cp.hbf = c[C_HBF]; cp.ks = c[C_KS]; cp.lai = c[C_LAI]; cp.lai2 = c[C_LAI2]; cp.tss = c[C_TSS];
      cp.sob = cp.sof = cp.ko = cp.too = cp.Z = cp.hot = cp.pso2w = 0.0;
      const CanopyFlux<double> fl = canopy_flux<double>(cp, refl, tran, absb);
      const double rdry = soil_dry<double>(tb, c[C_F1], c[C_F2], c[C_F3]);
      double fm[7] = {c[C_FM0], c[C_FM1], c[C_FM2], c[C_FM3], c[C_FM4], c[C_FM5], c[C_FM6]};
      double rwet;
      soil_band<double>(tb, rdry, c[C_WET], fm, c[C_FMSUM], c[C_FILM2L], rwet);
      double rsd, rdd, a_s, a_d;
      products_band<double>(cp, fl, rwet, rsd, rdd, a_s, a_d);
      al_bs = __builtin_fma(ea, rsd, al_bs);
      al_ws = __builtin_fma(ea, rdd, al_ws);
      if (i <= PRODUCTS_PAR_LAST) {                     // (wave-uniform)
        f_bs = __builtin_fma(ea, a_s, f_bs);
        f_ws = __builtin_fma(ea, a_d, f_ws);
      }
    }
    double* pw = lds_p + wave * (4 * 64);
    pw[lane] = f_bs;
    pw[64 + lane] = f_ws;
    pw[128 + lane] = al_bs;
    pw[192 + lane] = al_ws;
    __syncthreads();
    // wave q finishes quantity q: (p0 + p1) + (p2 + p3), then the division
    static_assert(COL_WAVES == 4, "four partial sums, four quantities");
    const double* pq = lds_p + wave * 64 + lane;
    const double sum = (pq[0] + pq[4 * 64]) + (pq[2 * 4 * 64] + pq[3 * 4 * 64]);
    const double v = sum / (wave < 2 ? ea_par : ea_all);
    double* const dst = wave == 0 ? out.fapar_bs : wave == 1 ? out.fapar_ws : wave == 2 ? out.albedo_bs : out.albedo_ws;
    int64_t sj = s;                                     // (the comparison is formed again here: kept as a lane mask across the
    SPART_KEEP_BRANCH(sj);                              //  band loop it is one more pair of SGPRs the loop has no room for)
    if (dst && sj < B) dst[sj] = v;
  }
  if (wave == COL_WAVES - 1 && out.fcover) {            // (wave-uniform; no barrier follows)
    // the lane's address and its "inside the batch" flag wait in VGPRs: the literals of the LIDF iteration fill the SGPRs
    double* dst = out.fcover + sc;
    int inside = s < B ? 1 : 0;
    SPART_KEEP_BRANCH(dst);
    SPART_KEEP_BRANCH(inside);
    const double fc = products_fcover(lds_c[C_LAI * 64 + lane], lidfa[sc], lidfb[sc]);
    if (inside) *dst = fc;
  }
}

#endif  // __HIPCC__

}  // namespace spart
