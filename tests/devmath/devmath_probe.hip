// Test-only probe of the DEVICE branches of csrc/spart_math.h: y[i] = f(x[i]), one lane per element, for the scalar math
// primitives and the forms built on them, exactly as hipcc compiles them for the product (same flags, SPART_FAST_MATH).
// tests/test_gpu_devmath.py compares every element with a long double / float64 reference; tests/helpers/devmath_probe.py
// builds this file into tests/devmath/libdevmath_probe.so.  Not part of libspart_hip.so: no C-ABI symbol of the product
// is defined here.
//
// The launchers take DEVICE pointers, run on the default stream and return the hipError_t of the launch and the
// synchronisation after it (0 = hipSuccess, -1 = refused arguments).  block is the workgroup size: 256 (TILE of the band
// kernels) or 64 (one wave: stage_f64_tables() then walks its 256 + 512 entries in 4 + 8 passes).
#include "../../spart-python_amd/csrc/spart_math.h"

namespace {

using spart::Mx;

// function ids (tests/test_gpu_devmath.py holds the same list)
enum : int {
  F_EXP = 0, F_EXP2, F_EXP_POLY, F_LOG, F_LOG2, F_SQRT, F_RCP, F_LOG1P, F_LOG2_1P,
  F_OMEN,        // one_minus_exp_neg(z)
  F_OMEN_EZ,     // one_minus_exp_neg(z, ez), ez = Mx<T>::exp(-z) as leaf_band forms it
  F_OMEN_POLY,   // one_minus_exp_neg_poly(z)                      (float64 only)
  F_OMEN2_E,     // one_minus_exp2_neg(z, e), e = Mx<T>::exp2(-z)  (float32 only)
  F_RCP_SEED,    // v_rcp_f64 / v_rsq_f64 alone, the seeds of Mx<double>::rcp / sqrt: the accuracy their one Newton step
  F_RSQ_SEED,    // squares                                         (float64 only)
  F_UNARY_END
};
enum : int { B_DIVX = 0, B_J1_D, B_J1_A, B_J2_D, B_END };

template <typename T> struct Only;
template <> struct Only<double> {
  static __device__ double f(int fid, double x, bool& ok) {
    switch (fid) {
      case F_EXP_POLY: return Mx<double>::exp_poly(x);
      case F_OMEN_POLY: return Mx<double>::one_minus_exp_neg_poly(x);
#if defined(__HIP_DEVICE_COMPILE__)
      case F_RCP_SEED: return __builtin_amdgcn_rcp(x);
      case F_RSQ_SEED: return __builtin_amdgcn_rsq(x);
#endif
    }
    ok = false;
    return 0.0;
  }
};
template <> struct Only<float> {
  static __device__ float f(int fid, float x, bool& ok) {
    switch (fid) {
      case F_LOG2: return Mx<float>::log2(x);
      case F_LOG2_1P: return Mx<float>::log2_1p(x);
      case F_OMEN2_E: return Mx<float>::one_minus_exp2_neg(x, Mx<float>::exp2(-x));
    }
    ok = false;
    return 0.0f;
  }
};

template <typename T> __device__ T unary(int fid, T x, bool& ok) {
  switch (fid) {
    case F_EXP: return Mx<T>::exp(x);
    case F_EXP2: return Mx<T>::exp2(x);
    case F_LOG: return Mx<T>::log(x);
    case F_SQRT: return Mx<T>::sqrt(x);
    case F_RCP: return Mx<T>::rcp(x);
    case F_LOG1P: return Mx<T>::log1p(x);
    case F_OMEN: return Mx<T>::one_minus_exp_neg(x);
    case F_OMEN_EZ: return Mx<T>::one_minus_exp_neg(x, Mx<T>::exp(-x));
  }
  return Only<T>::f(fid, x, ok);
}

// The SAIL J-functions take five arguments that canopy_core derives from two: a = d (J1: (m - k) L, J2: (k + m) L) and b = L.
// tk = e^-kL with k = 1/2, e1 = tk e^-d; the reciprocals are formed the way the callers do (a finite dummy / a clamped |d|
// where the Taylor side is taken).  Only the bits matter here: the test asks that a lane's result does not depend on which
// lanes share its wave.
template <typename T> __device__ T binary(int fid, T a, T b, bool& ok) {
  using S = spart::SailJ<T>;
  switch (fid) {
    case B_DIVX: return spart::divx(a, b);
    case B_J1_D: {
      const T tk = Mx<T>::exp(T(-0.5) * b), e1 = tk * Mx<T>::exp(-a);
      const T id = (Mx<T>::fabs(a) < S::THRESH) ? T(1) : Mx<T>::rcp(a);
      return spart::sail_j1_d(b, tk, e1, a, id);
    }
    case B_J1_A: {
      const T tk = Mx<T>::exp(T(-0.5) * b), e1 = tk * Mx<T>::exp(-a);
      const T ia = Mx<T>::rcp(Mx<T>::fmax(Mx<T>::fabs(a), S::THRESH));
      return spart::sail_j1_a(b, tk, e1, a, ia);
    }
    case B_J2_D: {
      const T tk = Mx<T>::exp(T(-0.5) * b), e1 = tk * Mx<T>::exp(-a);
      const T kpm = a * Mx<T>::rcp(b);
      return spart::sail_j2_d(b, tk, e1, kpm, Mx<T>::rcp(kpm));
    }
  }
  ok = false;
  return T(0);
}

// All threads of the workgroup, before any of them leaves.  LDS keeps what an earlier workgroup left there -- after one good
// launch a staging loop that skips entries would still find the right values -- so the two tables are filled with NaN first
// (a loop of the probe's own): an entry that stage_f64_tables() does not write then shows in every result read through it.
template <typename T> __device__ void stage() {
  if constexpr (sizeof(T) == 8) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int i = threadIdx.x; i < spart::F64_EXP_TAB; i += blockDim.x) spart::s_f64_exp_tab[i] = __builtin_nan("");
    for (int i = threadIdx.x; i < 2 * spart::F64_LOG_TAB; i += blockDim.x) spart::s_f64_log_tab[i] = __builtin_nan("");
    __syncthreads();
#endif
    spart::stage_f64_tables();
  }
}

template <typename T> __global__ void k_unary(int fid, const T* __restrict__ x, T* __restrict__ y, long long n) {
  stage<T>();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok = true;
  const T v = unary<T>(fid, x[i], ok);
  y[i] = ok ? v : T(-12345);
}

template <typename T> __global__ void k_binary(int fid, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, long long n) {
  stage<T>();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok = true;
  const T v = binary<T>(fid, a[i], b[i], ok);
  y[i] = ok ? v : T(-12345);
}

// plate_tau: (tau, u)
template <typename T> __global__ void k_plate(const T* __restrict__ x, T* __restrict__ y0, T* __restrict__ y1, long long n) {
  stage<T>();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T tau, u;
  spart::plate_tau<T>(x[i], tau, u);
  y0[i] = tau;
  y1[i] = u;
}

bool refused(long long n, int block) { return n <= 0 || n > (1ll << 30) || (block != 64 && block != 256); }

int finish() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

template <typename T> int run_unary(int fid, const void* x, void* y, long long n, int block) {
  if (refused(n, block) || fid < 0 || fid >= F_UNARY_END || !x || !y) return -1;
  hipLaunchKernelGGL(k_unary<T>, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, 0, fid, (const T*)x, (T*)y, n);
  return finish();
}
template <typename T> int run_binary(int fid, const void* a, const void* b, void* y, long long n, int block) {
  if (refused(n, block) || fid < 0 || fid >= B_END || !a || !b || !y) return -1;
  hipLaunchKernelGGL(k_binary<T>, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, 0, fid, (const T*)a, (const T*)b, (T*)y, n);
  return finish();
}
template <typename T> int run_plate(const void* x, void* y0, void* y1, long long n, int block) {
  if (refused(n, block) || !x || !y0 || !y1) return -1;
  hipLaunchKernelGGL(k_plate<T>, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, 0, (const T*)x, (T*)y0, (T*)y1, n);
  return finish();
}

}  // namespace

extern "C" {
// 1 when this file was compiled with SPART_FAST_MATH (the product's default build), 0 otherwise
int dm_fast_math() {
#if defined(SPART_FAST_MATH)
  return 1;
#else
  return 0;
#endif
}
// dtype: 1 = float64, 0 = float32 (the convention of tests/hostmath)
int dm_unary(int dtype, int fid, const void* x, void* y, long long n, int block) {
  return dtype ? run_unary<double>(fid, x, y, n, block) : run_unary<float>(fid, x, y, n, block);
}
int dm_binary(int dtype, int fid, const void* a, const void* b, void* y, long long n, int block) {
  return dtype ? run_binary<double>(fid, a, b, y, n, block) : run_binary<float>(fid, a, b, y, n, block);
}
int dm_plate_tau(int dtype, const void* x, void* tau, void* u, long long n, int block) {
  return dtype ? run_plate<double>(x, tau, u, n, block) : run_plate<float>(x, tau, u, n, block);
}
}
