// TEST INFRASTRUCTURE ONLY (tests/test_refine_host.py): the per-observation arithmetic of spart_refine (csrc/spart_refine.h,
// part 1) for a g++ build with -ffp-contract=off, one observation per call, every array dense (stride 1).
#include <cstdint>

#include "../../spart-python_amd/csrc/spart_refine.h"

using namespace spart;

extern "C" {

int rh_max_f() { return REFINE_MAXF; }

void rh_clip(int64_t n, const double* v, const double* lo, const double* hi, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = refine_clip(v[i], lo[i], hi[i]);
}

void rh_fd_step(int64_t n, const double* t, const double* h, const double* hi, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = refine_fd_step(t[i], h[i], hi[i]);
}

void rh_lambda(int64_t n, const double* lam, const int32_t* accept, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = refine_lambda(lam[i], accept[i] != 0);
}

// step 3 of one observation: the trial cost; *bad = a weight that kills the observation
double rh_cost(int nb, const double* y0, const double* obs, const double* w, int32_t* bad) {
  bool b = false;
  const double c = refine_tile_cost(0.0, &b, nb, w, 1, y0, 1, obs, 1);
  *bad = b ? 1 : 0;
  return c;
}

// the decision of one call: out = {code, na} and *lam_out
void rh_decide(int it, double ct, int bad, double cost, double lam, int na, int32_t* out, double* lam_out) {
  const RefineDecision d = refine_decide(it, ct, bad != 0, cost, lam, na);
  out[0] = d.code;
  out[1] = d.na;
  *lam_out = d.lam;
}

// J_jf and r_j of one observation from its F + 1 evaluations Y ((F + 1, nb) row-major) and the steps sh (F,)
void rh_jacobian(int F, int nb, const double* Y, const double* obs, const double* w, const double* sh, double* J /* (nb, F) */,
                 double* r /* (nb,) */) {
  for (int j = 0; j < nb; ++j) {
    r[j] = w[j] != 0.0 ? refine_residual(Y[j], obs[j]) : 0.0;
    for (int f = 0; f < F; ++f) J[j * F + f] = refine_jacobian(Y[(f + 1) * nb + j], Y[j], sh[f]);
  }
}

// the packed sums of one observation: J (nb, F) row-major, r, w (nb,) -> packed (F (F + 1) / 2 + F)
void rh_normal(int F, int nb, const double* J, const double* r, const double* w, double* packed) {
  const int nt = refine_ntri(F);
  for (int e = 0; e < nt + F; ++e) {
    int a, b;
    refine_packed_pair(e, nt, &a, &b);
    packed[e] = b >= 0 ? refine_tile_sum(0.0, 0, nb, w, 1, J + a, F, J + b, F) : refine_tile_sum(0.0, 0, nb, w, 1, J + a, F, r, 1);
  }
}

void rh_propose(int F, const double* packed, double lam, const double* x, const double* lo, const double* hi, double* t) {
  double L[REFINE_MAXF * (REFINE_MAXF + 1) / 2], d[REFINE_MAXF];
  refine_propose(F, packed, 1, lam, x, 1, lo, hi, L, 1, d, 1, t, 1);
}

void rh_std(int F, const double* packed, double* out) {
  double L[REFINE_MAXF * (REFINE_MAXF + 1) / 2], z[REFINE_MAXF];
  refine_std(F, packed, 1, L, 1, z, 1, out, 1);
}

}  // extern "C"
