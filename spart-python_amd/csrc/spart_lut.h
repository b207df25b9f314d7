// LUT inversion (no counterpart in the reference beyond its exact np.argmin nearest-index search,
// SPART.py:381-387): for every observed spectrum y_m find THE row b of the LUT that minimises
//
//     c_T(b, m) = sum_j w_j (x_bj - y_mj)^2   evaluated in the call's dtype T exactly like this:
//     c = 0;  for j = 0 .. nb-1:  d = x_bj - y_mj;  c = c + (w_j * d) * d      (every operation rounded to T, no FMA;
//                                                                                w = NULL: c = c + d * d)
//
// with ties going to the lowest row index and rows / observations with a non-finite cost never winning (-1 / +inf).
// That is what k_lut_reduce_exact / k_lut_fallback evaluate (under SPART_NO_CONTRACT; bands padded with zeros add exactly 0)
// and what the tests' brute force computes in numpy (tools/lut_brute_force.py).
//
// The search itself is a GEMM + argmin on the matrix cores, used as a FILTER with a proven error bound:
//   1. k_lut_centre   c_j = mean of a strided sample of LUT column j (any c is correct; a good one makes the bound small)
//   2. k_lut_prep     x' = x - c, n_b = sum w x'^2, laid out tile-major for the MFMA operand registers; rows with a
//                     non-finite entry become (0, .., 0, n = +inf): they can never come out as a minimum.
//                     Nmax = max_b sum |w| x'^2 over the finite rows (atomicMax on the bit pattern)
//   3. k_lut_scan_*   a~(b, m) = n_b - 2 sum_j w_j x'_bj y'_mj  on v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64
//                     (K = nb + 1: A[b][k] = x'_bk, n_b in column nb; Bq[k][m] = -2 w_k y'_mk, 1 in row nb).  Per
//                     (slice of the LUT, lane group) and observation the kernel keeps the smallest tile minimum, the tile
//                     it came from, and the SECOND smallest tile minimum (value only).
//   4. k_lut_reduce_exact   g = the smallest a~ over all partial results.  Every tile whose minimum is <= g + Delta is
//                     evaluated with the direct cost, row by row; if some partial result's SECOND minimum is also
//                     <= g + Delta there may be a candidate tile the scan did not remember: the observation goes to
//   5. k_lut_fallback / k_lut_fallback_merge   a plain vector-ALU brute force over the whole LUT with the direct cost
//                     (64 flagged observations on the lanes of a wave, LUT rows staged in LDS and read as broadcasts).
// So the result is the exact argmin whatever the data look like; the data only decide how much work steps 4-5 are.
//
// Delta.  u = unit roundoff of T (2^-24 / 2^-53), K = fused multiply-adds per accumulator chain (2 KS / 4 KS),
// N_b = sum |w| x'_b^2, Y = sum |w| y'^2, c(b) = the real-number cost.  With x' = (x - c)(1 + e), |e| <= u (same for y'):
//   (i)   | sum w (x - y)^2 - sum w (x' - y')^2 |          <= 4 u (N_b + Y)        (|d - (x'-y')| <= u (|x'| + |y'|))
//   (ii)  | n_b computed - sum w x'^2 |                    <= (nb + 2) u N_b
//   (iii) Bq = fl(-2 w y'): | 2 sum w x' y' e |            <= u (N_b + Y)          (2 |x' y'| <= x'^2 + y'^2)
//   (iv)  a chain of K fmas (any order):                   <= K u (|n_b| + 2 sum |w x' y'|) <= 2 K u (N_b + Y)
//   =>    | a~(b) + Y - c(b) | <= E = (nb + 2 K + 7) u (N_b + Y)
//   (v)   direct evaluation:  | c_T(b) - c(b) | <= F = (nb + 3) u sum |w| d^2 <= (2 nb + 6) u (N_b + Y)
// If b is the argmin of c_T and a the row with a~(a) = g:  a~(b) + Y <= c(b) + E_b <= c_T(b) + E_b + F_b <= c_T(a) + E_b + F_b
// <= c(a) + F_a + E_b + F_b <= g + Y + (E_a + F_a) + (E_b + F_b), i.e. a~(b) <= g + Delta with
//     Delta = (3 nb + 2 K + 13) u [(N_a + Y) + (N_b + Y)].
// N_a and N_b are not known to the reduce kernel, but bounded:
//   * always:  N_a, N_b <= Nmax  (the prep kernel's maximum over all finite rows);
//   * with non-negative weights (c is then a squared distance in the |w|-weighted norm), per observation:
//       N_a <= Na = max of n over the rows of the tile that produced g (read back from the operand image);
//       c(a) <= max(0, g + Y) + E_a =: cub;  c(b) <= c(a) (1 + 3 (nb + 3) u);  sqrt(N_b) <= sqrt(Y) + sqrt(c'(b)) with
//       c'(b) = sum w (x'_b - y')^2 <= c(b) + 4 u (Nmax + Y)   =>   N_b <= Nstar = (sqrt(Y) + sqrt(cub + 4 u (Nmax + Y)))^2.
//     For a LUT of spectra and an observation that resembles some of them Na and Nstar are ~Y, an order of magnitude below
//     Nmax: fewer candidate tiles, and far fewer observations for which the scan's top-1 + runner-up per slice is not enough.
// The code uses (3 nb + 2 K + 16) * 1.01 (second-order terms, the rounding of g + Delta and of Y itself, the square roots)
// plus 2^-100 / 1e-290 for products that underflow.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spart_math.h"      // SPART_NO_CONTRACT

namespace spart {

template <typename T> struct LutNum;
template <> struct LutNum<float> {
  static constexpr float u = 5.9604644775390625e-8f, tiny = 7.888609052210118e-31f;
  static constexpr float centre_cap = 4.611686018427387904e18f;           // 2^62 = sqrt(2^128) / 4
  static __device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
  static __device__ __forceinline__ unsigned long long bits(float v) { return (unsigned long long)__float_as_uint(v); }
  static __device__ __forceinline__ float from_bits(unsigned long long b) { return __uint_as_float((unsigned)b); }
};
template <> struct LutNum<double> {
  static constexpr double u = 1.1102230246251565e-16, tiny = 1e-290;
  static constexpr double centre_cap = 0x1p510;                           // sqrt(2^1024) / 4
  static __device__ __forceinline__ bool finite(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
  }
  static __device__ __forceinline__ unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }
  static __device__ __forceinline__ double from_bits(unsigned long long b) { return __longlong_as_double((long long)b); }
};

// ctl[0] = bit pattern of Nmax (non-negative floats order like unsigned integers), ctl[1] = number of flagged observations
constexpr int LUT_CTL_WORDS = 2;
constexpr int LUT_CENTRE_ROWS = 8192;      // rows sampled for the column means
constexpr int LUT_FB_BLOCKS = 2048;        // workgroups (x 4 waves) of the brute-force fallback
// float32 scan: 32-observation blocks per wave (256 observations, 8 KS operand registers + 8 x 16 accumulators: 106 ... 226
// VGPRs for KS = 4 ... 16).  Eight independent accumulator chains per wave keep the matrix pipe fed from TWO or three resident
// waves per SIMD -- v_mfma_f32_32x32x2_f32 sustains 27.2 ns per instruction and SIMD (154 Tflop/s) with two issuing waves
// and 33.9 ns with four (tools/ubench/mfma_f32_rate2.hip) -- and every LUT tile loaded is used for twice the observations.
// Measured 1M x 65 536, nb = 13: 4 / 6 / 7 / 8 / 10 / 12 / 16 blocks: 15.25 / 15.24 / 15.11 / 14.45 / 15.46 / 15.71 / 14.97 ms
// (profiles/r4_lut_to_sweep2.txt); nb = 6: 9.25 -> 9.10 ms, nb = 21: unchanged.
constexpr int LUT_TO = 8;

// column means of a strided sample -> centre[nb]; also resets the control words.  Entries that are not finite, or so large
// that their own square overflows (|v| > centre_cap), are left out of the mean: one fill value such as FLT_MAX would otherwise
// drag the centre so far that EVERY row's centred norm overflows and no row is eligible.  The row that holds such an entry is
// judged like any other, by its own norm (k_lut_prep / k_lutw_norm): rejected if that overflows (an entry above ~2^64 / 2^512),
// eligible otherwise; a LUT without such an entry gets the centres it always got.
template <typename T>
__global__ __launch_bounds__(256) void k_lut_centre(const T* __restrict__ lut, int nb, int64_t B, T* __restrict__ centre,
                                                    unsigned long long* __restrict__ ctl) {
  __shared__ double ss[256];
  __shared__ int sn[256];
  const int j = blockIdx.x;
  const int64_t ns = B < LUT_CENTRE_ROWS ? B : LUT_CENTRE_ROWS;
  const int64_t stride = ns > 0 ? B / ns : 1;
  double s = 0.0;
  int n = 0;
  for (int64_t i = threadIdx.x; i < ns; i += 256) {
    const T v = lut[i * stride * nb + j];
    if (__builtin_fabs((double)v) <= (double)LutNum<T>::centre_cap) {      // (false for NaN and +-inf)
      s += (double)v;
      ++n;
    }
  }
  ss[threadIdx.x] = s;
  sn[threadIdx.x] = n;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      ss[threadIdx.x] += ss[threadIdx.x + off];
      sn[threadIdx.x] += sn[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const T c = sn[0] > 0 ? (T)(ss[0] / sn[0]) : T(0);
    centre[j] = LutNum<T>::finite(c) ? c : T(0);
    if (j == 0) {
      ctl[0] = 0ull;
      ctl[1] = 0ull;
    }
  }
}

// One thread per LUT row (padding rows of the last tile included): centred row -> the operand-register image of its
// tile, [tile][kk][lane] with lane = (column % KPER) * ROWS + row % ROWS, column = KPER kk + lane / ROWS.
//   ROWS = 32, KPER = 2: v_mfma_f32_32x32x2_f32;  ROWS = 16, KPER = 4: v_mfma_f64_16x16x4_f64.
template <typename T, int KS, int ROWS>
__global__ __launch_bounds__(256) void k_lut_prep(const T* __restrict__ lut, const T* __restrict__ w, const T* __restrict__ centre,
                                                  int nb, int64_t B, int64_t ntile, T* __restrict__ tiles,
                                                  unsigned long long* __restrict__ ctl) {
  constexpr int KPER = 64 / ROWS;
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  T na = T(0);
  if (row < ntile * ROWS) {
    bool ok = row < B;
    T n = T(0);
    if (ok) {
      const T* x = lut + row * nb;
      for (int j = 0; j < nb; ++j) {
        const T v = x[j];
        ok = ok && LutNum<T>::finite(v);
        const T xc = v - centre[j];
        const T wj = w ? w[j] : T(1);
        n += wj * xc * xc;
        na += (wj < T(0) ? -wj : wj) * xc * xc;
      }
      ok = ok && LutNum<T>::finite(n) && LutNum<T>::finite(na);
    }
    if (!ok) na = T(0);
    T* dst = tiles + (row / ROWS) * (int64_t)(KS * 64) + (row % ROWS);
    for (int c = 0; c < KS * KPER; ++c) {
      T v = T(0);
      if (c < nb) v = ok ? lut[row * nb + c] - centre[c] : T(0);
      else if (c == nb) v = ok ? n : (T)INFINITY;
      dst[(c / KPER) * 64 + (c % KPER) * ROWS] = v;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_down(na, off, 64);
    na = o > na ? o : na;
  }
  if ((threadIdx.x & 63) == 0 && na > T(0)) atomicMax(&ctl[0], LutNum<T>::bits(na));
}

// float32 scan on the exact-f32 matrix cores.  A 32 x 32 x 2 MFMA takes ONE register of A (lane l: row l % 32,
// k = l / 32) and one of Bq (lane l: column l % 32, k = l / 32); K = 2 KS is covered by KS of them chained on one
// 16-register accumulator (lane l ends up with 16 LUT rows of observation l % 32).  Each wave keeps LUT_TO = 8 blocks of 32
// observations in registers (LUT_TO x KS operand registers) and streams the LUT tiles of its slice past them.
// The matrix pipe does the arithmetic (KS x 64 cycles per 1024 comparisons); the vector ALU only takes the minimum of
// the 16 accumulator values (v_min3) and keeps, per lane, the smallest and second smallest of those tile minima and
// WHICH TILE the smallest came from (v_cmp, v_med3, two v_cndmask per tile and block).
typedef float spart_f16v __attribute__((ext_vector_type(16)));

template <int KS>
__global__ __launch_bounds__(256, 2) void k_lut_scan_mfma(const float* __restrict__ tiles, const float* __restrict__ obs,
                                                          const float* __restrict__ w, const float* __restrict__ centre, int nb,
                                                          int64_t ntile, int64_t M, int nslice, float* __restrict__ part_cost,
                                                          float* __restrict__ part_sec, int* __restrict__ part_tile) {
  const int lane = threadIdx.x & 63;
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (32 * LUT_TO);   // this wave's first observation
  if (m0 >= M) return;                                                                 // (whole wave; no barrier below)
  const int slice = blockIdx.y;
  const int j = lane & 31, half = lane >> 5;
  float bq[LUT_TO][KS];
#pragma unroll
  for (int blk = 0; blk < LUT_TO; ++blk) {
    const int64_t m = m0 + blk * 32 + j;
    const int64_t mc = m < M ? m : M - 1;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int col = 2 * kk + half;
      bq[blk][kk] = col < nb ? -2.0f * (w ? w[col] : 1.0f) * (obs[mc * nb + col] - centre[col]) : (col == nb ? 1.0f : 0.0f);
    }
  }
  const int64_t per = (ntile + nslice - 1) / nslice;
  const int64_t t0 = per * slice;
  const int64_t t1 = (t0 + per < ntile) ? t0 + per : ntile;
  float best[LUT_TO], sec[LUT_TO];
  int bt[LUT_TO];
#pragma unroll
  for (int blk = 0; blk < LUT_TO; ++blk) {
    best[blk] = INFINITY;
    sec[blk] = INFINITY;
    bt[blk] = -1;
  }
  if (t0 < t1) {
    const float* __restrict__ ap = tiles + t0 * (KS * 64) + lane;
    float a[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) a[kk] = ap[kk * 64];
    for (int64_t t = t0; t < t1; ++t) {
      if (t + 1 < t1) ap += KS * 64;                   // next tile's operands in flight during this tile's MFMAs
      float an[KS];
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) an[kk] = ap[kk * 64];
#pragma unroll
      for (int blk = 0; blk < LUT_TO; ++blk) {
        spart_f16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bq[blk][kk], acc, 0, 0, 0);
        // minimum of the 16 accumulator values: v_min3_f32 written out (fminf() makes the compiler canonicalise the MFMA
        // results first, two v_max per block; v_min / v_min3 return the non-NaN operand whatever its kind)
        float mn;
        asm("v_min3_f32 %0, %1, %2, %3" : "=v"(mn) : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]));
#pragma unroll
        for (int r = 3; r < 15; r += 2) asm("v_min3_f32 %0, %1, %2, %3" : "=v"(mn) : "v"(mn), "v"(acc[r]), "v"(acc[r + 1]));
        asm("v_min_f32 %0, %1, %2" : "=v"(mn) : "v"(mn), "v"(acc[15]));
        // (best, sec) <- the two smallest of (best, sec, mn); a tile minimum EQUAL to the best so far becomes `sec`, so
        // an exact tie between tiles is seen by the reduce kernel
        const bool lt = mn < best[blk];
        sec[blk] = __builtin_amdgcn_fmed3f(best[blk], mn, sec[blk]);
        best[blk] = lt ? mn : best[blk];
        bt[blk] = lt ? (int)(t - t0) : bt[blk];
      }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) a[kk] = an[kk];
    }
  }
#pragma unroll
  for (int blk = 0; blk < LUT_TO; ++blk) {
    const int64_t m = m0 + blk * 32 + j;
    if (m < M) {
      const int64_t o = ((int64_t)slice * 2 + half) * M + m;
      part_cost[o] = best[blk];
      part_sec[o] = sec[blk];
      part_tile[o] = bt[blk] < 0 ? -1 : (int)(t0 + bt[blk]);
    }
  }
}

// float64: the same scan on v_mfma_f64_16x16x4_f64 (K steps of 4, 16 x 16 tiles, four accumulator values per lane: lane l
// holds four LUT rows of observation l % 16; the four lane groups l / 16 keep separate partial results).
typedef double spart_d4v __attribute__((ext_vector_type(4)));

template <int KS, int TO>
__global__ __launch_bounds__(256, 2) void k_lut_scan_mfma64(const double* __restrict__ tiles, const double* __restrict__ obs,
                                                            const double* __restrict__ w, const double* __restrict__ centre, int nb,
                                                            int64_t ntile, int64_t M, int nslice, double* __restrict__ part_cost,
                                                            double* __restrict__ part_sec, int* __restrict__ part_tile) {
  const int lane = threadIdx.x & 63;
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (16 * TO);
  if (m0 >= M) return;
  const int slice = blockIdx.y;
  const int j = lane & 15, q = lane >> 4;
  double bq[TO][KS];
#pragma unroll
  for (int blk = 0; blk < TO; ++blk) {
    const int64_t m = m0 + blk * 16 + j;
    const int64_t mc = m < M ? m : M - 1;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int col = 4 * kk + q;
      bq[blk][kk] = col < nb ? -2.0 * (w ? w[col] : 1.0) * (obs[mc * nb + col] - centre[col]) : (col == nb ? 1.0 : 0.0);
    }
  }
  const int64_t per = (ntile + nslice - 1) / nslice;
  const int64_t t0 = per * slice;
  const int64_t t1 = (t0 + per < ntile) ? t0 + per : ntile;
  double best[TO], sec[TO];
  int bt[TO];
#pragma unroll
  for (int blk = 0; blk < TO; ++blk) {
    best[blk] = INFINITY;
    sec[blk] = INFINITY;
    bt[blk] = -1;
  }
  if (t0 < t1) {
    const double* __restrict__ ap = tiles + t0 * (KS * 64) + lane;
    double a[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) a[kk] = ap[kk * 64];
    for (int64_t t = t0; t < t1; ++t) {
      if (t + 1 < t1) ap += KS * 64;
      double an[KS];
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) an[kk] = ap[kk * 64];
#pragma unroll
      for (int blk = 0; blk < TO; ++blk) {
        spart_d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bq[blk][kk], acc, 0, 0, 0);
        const double mn = __builtin_fmin(__builtin_fmin(acc[0], acc[1]), __builtin_fmin(acc[2], acc[3]));
        // mn is never NaN for a finite observation (non-finite rows were replaced by n = +inf in k_lut_prep)
        const bool lt = mn < best[blk];
        sec[blk] = __builtin_fmin(sec[blk], __builtin_fmax(best[blk], mn));
        best[blk] = lt ? mn : best[blk];
        bt[blk] = lt ? (int)(t - t0) : bt[blk];
      }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) a[kk] = an[kk];
    }
  }
#pragma unroll
  for (int blk = 0; blk < TO; ++blk) {
    const int64_t m = m0 + blk * 16 + j;
    if (m < M) {
      const int64_t o = ((int64_t)slice * 4 + q) * M + m;
      part_cost[o] = best[blk];
      part_sec[o] = sec[blk];
      part_tile[o] = bt[blk] < 0 ? -1 : (int)(t0 + bt[blk]);
    }
  }
}

// the verdict of k_lut_prep on row r, read back from the operand image (column nb of its tile holds n_b, +inf for a rejected
// row): the exact evaluations ask it too, so that a row whose centred norm overflows never wins whichever path decides
template <typename T, int ROWS>
__device__ __forceinline__ bool lut_row_ok(const T* __restrict__ tiles, int ks, int nb, int64_t r) {
  constexpr int NG = 64 / ROWS;
  return LutNum<T>::finite(tiles[((r / ROWS) * ks + nb / NG) * 64 + (nb % NG) * ROWS + (r % ROWS)]);
}

// One WAVE per observation (four per workgroup): lanes over the partial results (threshold), then the candidate tiles
// are evaluated with the direct cost by 64 / ROWS lane groups at a time, one LUT row per lane.
// coef = 2 (3 nb + 2 K + 16) * 1.01 * u (host: lut_delta_coef).
template <typename T>
__device__ __forceinline__ bool lut_better(T oc, int64_t oi, T bc, int64_t bi) {     // (cost, row) lexicographic; (inf, -1) is worst
  // a cost of -inf (negative weights whose products overflow) is NOT FINITE and never wins, like NaN and +inf
  return (oc < bc && oc > -(T)INFINITY) || (oc == bc && oi >= 0 && oi < bi);
}

template <typename T, int ROWS>
__global__ __launch_bounds__(256) void k_lut_reduce_exact(const T* __restrict__ part_cost, const T* __restrict__ part_sec,
                                                          const int* __restrict__ part_tile, const T* __restrict__ tiles, int ks,
                                                          const T* __restrict__ lut, const T* __restrict__ obs,
                                                          const T* __restrict__ w, const T* __restrict__ centre, int nb, int64_t B,
                                                          int64_t M, int npart, T coef_e, T coef_ef,
                                                          unsigned long long* __restrict__ ctl, int* __restrict__ flag_list,
                                                          int64_t* __restrict__ best_idx, T* __restrict__ best_cost) {
  constexpr int NG = 64 / ROWS;                        // candidate tiles evaluated side by side (= k columns per operand register)
  __shared__ T ysm[4][32], wsm[32];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t mraw = (int64_t)blockIdx.x * 4 + wv;
  const bool active = mraw < M;
  const int64_t m = active ? mraw : M - 1;
  const T yv = lane < nb ? obs[m * nb + lane] : T(0);
  if (lane < 32) ysm[wv][lane] = yv;                   // zero-padded to 32: a padded band adds (w * 0) * 0 = 0 to the cost
  if (threadIdx.x < 32) wsm[threadIdx.x] = (w && (int)threadIdx.x < nb) ? w[threadIdx.x] : T(0);
  __syncthreads();
  if (!active) return;
  const bool yfin = __all(LutNum<T>::finite(yv)) != 0;
  if (!yfin) {                                         // every direct cost is NaN or +inf: nothing wins
    if (lane == 0) {
      best_idx[m] = -1;
      best_cost[m] = (T)INFINITY;
    }
    return;
  }
  T ya = T(0);
  bool wneg = false;
  if (lane < nb) {
    const T yc = yv - centre[lane];
    const T wj = w ? w[lane] : T(1);
    wneg = wj < T(0);
    ya = (wneg ? -wj : wj) * yc * yc;
  }
  wneg = __any(wneg) != 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ya += __shfl_xor(ya, off, 64);
  T g = (T)INFINITY;
  int ta = -1;
  for (int p = lane; p < npart; p += 64) {
    const T c = part_cost[(int64_t)p * M + m];
    const int t = part_tile[(int64_t)p * M + m];
    if (t >= 0 && c < g) {
      g = c;
      ta = t;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(g, off, 64);
    const int ot = __shfl_xor(ta, off, 64);
    if (o < g || (o == g && ot > ta)) {                // (any tile that attains g will do; the tie rule only makes all lanes agree)
      g = o;
      ta = ot;
    }
  }
  const T nmax = LutNum<T>::from_bits(ctl[0]);
  T na = nmax, nstar = nmax;
  if (!wneg && ta >= 0) {
    // N_a <= the largest n among the rows of tile ta (n = sum w x'^2 = N for w >= 0; padding / non-finite rows hold +inf)
    T v = T(0);
    if (lane < ROWS) {
      const T n = tiles[((int64_t)ta * ks + nb / NG) * 64 + (nb % NG) * ROWS + lane];
      v = LutNum<T>::finite(n) ? n : T(0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const T o = __shfl_xor(v, off, 64);
      v = o > v ? o : v;
    }
    const T gy = g + ya;
    const T cub = ((gy > T(0) ? gy : T(0)) + T(2) * coef_e * (v + ya) + T(4) * LutNum<T>::u * (nmax + ya)) * T(1.001);
    const T r = (T)__builtin_sqrt((double)ya) + (T)__builtin_sqrt((double)cub);
    const T ns = r * r * T(1.001);
    if (v < na) na = v;
    if (ns < nstar) nstar = ns;                        // (never above the global bound; NaN / inf leave it in place)
  }
  const T thr = g + (coef_ef * ((na + ya) + (nstar + ya)) + LutNum<T>::tiny);
  // no finite filter value (e.g. an all-NaN LUT) or no finite threshold (overflow): let the brute force decide
  bool over = !(g < (T)INFINITY) || !LutNum<T>::finite(thr);
  T bc = (T)INFINITY;
  int64_t bi = -1;
  const T* ys = ysm[wv];
  const int grp = lane / ROWS, rl = lane % ROWS;
  for (int p0 = 0; p0 < npart && !over; p0 += 64) {
    const int p = p0 + lane;
    int t = -1;
    bool cand = false, second = false;
    if (p < npart) {
      t = part_tile[(int64_t)p * M + m];
      cand = t >= 0 && part_cost[(int64_t)p * M + m] <= thr;
      second = cand && part_sec[(int64_t)p * M + m] <= thr;     // a second tile of this partial result may hold the minimum
    }
    if (__any(second)) {
      over = true;
      break;
    }
    unsigned long long mask = __ballot(cand);
    while (mask) {                                     // NG candidate tiles per round, one row per lane
      int myt = -1;
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        if (mask) {
          const int L = __builtin_ctzll(mask);
          mask &= mask - 1;
          const int tq = __shfl(t, L, 64);
          if (grp == q) myt = tq;
        }
      }
      const int64_t r = (int64_t)myt * ROWS + rl;
      if (myt >= 0 && r < B) {
        SPART_NO_CONTRACT
        const T* x = lut + r * nb;
        T c = T(0);
        for (int j = 0; j < nb; j += 4) {              // four bands in flight; the padded ones contribute exactly 0
          const T x0 = x[j], x1 = j + 1 < nb ? x[j + 1] : T(0), x2 = j + 2 < nb ? x[j + 2] : T(0), x3 = j + 3 < nb ? x[j + 3] : T(0);
          const T d0 = x0 - ys[j], d1 = x1 - ys[j + 1], d2 = x2 - ys[j + 2], d3 = x3 - ys[j + 3];
          if (w) {
            c = c + (wsm[j] * d0) * d0;
            c = c + (wsm[j + 1] * d1) * d1;
            c = c + (wsm[j + 2] * d2) * d2;
            c = c + (wsm[j + 3] * d3) * d3;
          } else {
            c = c + d0 * d0;
            c = c + d1 * d1;
            c = c + d2 * d2;
            c = c + d3 * d3;
          }
        }
        if (lut_row_ok<T, ROWS>(tiles, ks, nb, r) && lut_better(c, r, bc, bi)) {
          bc = c;
          bi = r;
        }
      }
    }
  }
  if (over) {
    if (lane == 0) {
      const unsigned long long pos = atomicAdd(&ctl[1], 1ull);
      flag_list[pos] = (int)m;
    }
    return;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T oc = __shfl_xor(bc, off, 64);
    const int64_t oi = __shfl_xor(bi, off, 64);
    if (lut_better(oc, oi, bc, bi)) {
      bc = oc;
      bi = oi;
    }
  }
  if (lane == 0) {
    best_idx[m] = bi;
    best_cost[m] = bc;
  }
}

// Work split of the fallback: `count` flagged observations in groups of 64 (one per lane), each group's scan of the
// LUT cut into `spg` slices of `per` rows so that the W waves of the launch all have work.
__host__ __device__ inline void lut_fb_partition(unsigned count, int64_t B, int W, int& ngroups, int& spg, int64_t& per) {
  ngroups = (int)((count + 63u) / 64u);
  int64_t cap = (B + 255) / 256;
  if (cap < 1) cap = 1;
  int64_t s = ngroups > 0 ? W / ngroups : 1;
  if (s < 1) s = 1;
  if (s > cap) s = cap;
  spg = (int)s;
  per = (B + s - 1) / s;
}

// Brute force with the direct cost for the flagged observations.  Lane = observation (its bands and the weights in
// registers, NBC = nb rounded up to a multiple of 4, zero-padded: a padded band adds exactly 0); the wave stages LUT_FB_ROWS
// LUT rows at a time in its own LDS block (zero-padded to NBC) and reads them back as wave-uniform broadcasts.
// Dynamic LDS: 4 waves x LUT_FB_ROWS x NBC x sizeof(T).
constexpr int LUT_FB_ROWS = 32;

template <typename T, int NBC>
__global__ __launch_bounds__(256) void k_lut_fallback(const T* __restrict__ lut, const T* __restrict__ obs, const T* __restrict__ w,
                                                      int nb, int64_t B, const T* __restrict__ tiles, int ks,
                                                      const unsigned long long* __restrict__ ctl,
                                                      const int* __restrict__ flag_list, T* __restrict__ fb_cost,
                                                      int64_t* __restrict__ fb_idx) {
  SPART_NO_CONTRACT
  extern __shared__ char lut_smem[];
  const unsigned count = (unsigned)ctl[1];
  if (count == 0u) return;
  const int W = (int)gridDim.x * 4;
  int ngroups, spg;
  int64_t per;
  lut_fb_partition(count, B, W, ngroups, spg, per);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  T* xs = reinterpret_cast<T*>(lut_smem) + (size_t)wv * LUT_FB_ROWS * NBC;
  T wr[NBC];
#pragma unroll
  for (int j = 0; j < NBC; ++j) wr[j] = (w && j < nb) ? w[j] : T(0);
  const int64_t nitem = (int64_t)ngroups * spg;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wv; item < nitem; item += W) {
    const int group = (int)(item / spg), s = (int)(item % spg);
    const unsigned f = (unsigned)group * 64u + (unsigned)lane;
    const int64_t m = flag_list[f < count ? f : (unsigned)group * 64u];     // (lanes past the end repeat the group's first)
    T y[NBC];
#pragma unroll
    for (int j = 0; j < NBC; ++j) y[j] = j < nb ? obs[m * nb + j] : T(0);
    const int64_t r0 = (int64_t)s * per, r1 = (r0 + per < B) ? r0 + per : B;
    T bc = (T)INFINITY;
    int64_t bi = -1;
    for (int64_t rb = r0; rb < r1; rb += LUT_FB_ROWS) {
      const int nrow = (int)(r1 - rb < LUT_FB_ROWS ? r1 - rb : LUT_FB_ROWS);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                 // (the previous block has been read)
      __builtin_amdgcn_wave_barrier();
      for (int e = lane; e < LUT_FB_ROWS * NBC; e += 64) {
        const int rr = e / NBC, j = e % NBC;
        xs[e] = (rr < nrow && j < nb) ? lut[(rb + rr) * nb + j] : T(0);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      for (int rr = 0; rr < nrow; ++rr) {
        if (!lut_row_ok<T, (sizeof(T) == 4 ? 32 : 16)>(tiles, ks, nb, rb + rr)) continue;      // (wave-uniform)
        const T* x = xs + rr * NBC;
        T c = T(0);
        if (w) {
#pragma unroll
          for (int j = 0; j < NBC; ++j) {
            const T d = x[j] - y[j];
            c = c + (wr[j] * d) * d;
          }
        } else {
#pragma unroll
          for (int j = 0; j < NBC; ++j) {
            const T d = x[j] - y[j];
            c = c + d * d;
          }
        }
        if (c < bc && c > -(T)INFINITY) {              // ascending rows + strict '<': ties to the lowest row; -inf is not finite
          bc = c;
          bi = rb + rr;
        }
      }
    }
    fb_cost[item * 64 + lane] = bc;
    fb_idx[item * 64 + lane] = bi;
  }
}

// one wave per flagged observation, lanes over the slices of its brute-force scan
template <typename T>
__global__ __launch_bounds__(256) void k_lut_fallback_merge(int64_t B, int W, const unsigned long long* __restrict__ ctl,
                                                            const int* __restrict__ flag_list, const T* __restrict__ fb_cost,
                                                            const int64_t* __restrict__ fb_idx, int64_t* __restrict__ best_idx,
                                                            T* __restrict__ best_cost) {
  const unsigned count = (unsigned)ctl[1];
  const int lane = threadIdx.x & 63;
  const unsigned nwave = gridDim.x * 4u;
  int ngroups, spg;
  int64_t per;
  lut_fb_partition(count, B, W, ngroups, spg, per);
  for (unsigned f = blockIdx.x * 4u + (threadIdx.x >> 6); f < count; f += nwave) {
    const int64_t base = (int64_t)(f / 64u) * spg;
    const int l = (int)(f % 64u);
    T bc = (T)INFINITY;
    int64_t bi = -1;
    for (int s = lane; s < spg; s += 64) {
      const T c = fb_cost[(base + s) * 64 + l];
      const int64_t i = fb_idx[(base + s) * 64 + l];
      if (lut_better(c, i, bc, bi)) {
        bc = c;
        bi = i;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const T oc = __shfl_xor(bc, off, 64);
      const int64_t oi = __shfl_xor(bi, off, 64);
      if (lut_better(oc, oi, bc, bi)) {
        bc = oc;
        bi = oi;
      }
    }
    if (lane == 0) {
      const int m = flag_list[f];
      best_idx[m] = bi;
      best_cost[m] = bc;
    }
  }
}

// ---- top-k (spart_lut_topk): the k rows of smallest c_T per observation, ordered by (cost, row)
//
// Steps, per chunk of at most LUT_TOPK_CHUNK observations (after k_lut_centre / k_lut_prep, which are shared):
//   1. k_lut_scan_mfma / _mfma64 as above, with at least 2k / G slices (G = lane groups: 2 for f32, 4 for f64), so that the
//      partial results hold at least 2k values.  Every partial result belongs to ONE lane group of ONE slice, and each lane
//      group holds its own rows of every tile (the MFMA output layout), so its smallest and second smallest tile minima
//      (best, sec) are the filter values a~ of two DIFFERENT rows, and no row appears behind two partial results.
//   2. k_lut_topk_bound  U = the k-th smallest finite value among the 2 npart values (best, sec) of the observation: the
//      largest of k filter values a~(a_1) .. a~(a_k) of k DISTINCT rows (bisection on the order-preserving bit pattern).
//   3. k_lut_collect_mfma / _mfma64  the same GEMM once more; every tile whose minimum (over all its rows) is
//      <= thr = U + Delta is appended to the observation's candidate list (capacity lut_topk_cap(k) tiles).
//   4. k_lut_topk_select<BRUTE = false>  one wave per observation evaluates every row of every candidate tile with the
//      direct cost (the arithmetic of k_lut_reduce_exact) and keeps the k best by (cost, row) in LDS (a 512-entry buffer,
//      bitonic-sorted and cut back to k whenever it fills; entries at or above the current k-th are not admitted).
//      An observation whose U or thr is not finite, whose list overflowed, or for which fewer than k rows with a finite cost
//      were found, is flagged; after the last chunk
//   5. k_lut_topk_select<BRUTE = true> evaluates EVERY row for the flagged observations (same buffer, same arithmetic).
//
// Why the candidate tiles hold the answer.  Let c_k be the k-th smallest c_T over all rows and b any row with c_T(b) <= c_k
// (every row of the answer, and every row tied with its last place).  The k rows a_1..a_k behind U are distinct, so
// c_k <= max_i c_T(a_i) = c_T(a*).  With the bounds (i)-(v) above:
//   a~(b) + Y <= c(b) + E_b <= c_T(b) + E_b + F_b <= c_T(a*) + E_b + F_b <= c(a*) + F_a* + E_b + F_b
//             <= a~(a*) + Y + (E_a* + F_a*) + (E_b + F_b) <= U + Y + Delta,
// Delta = (3 nb + 2 K + 13) u [(N_a* + Y) + (N_b + Y)] <= the k = 1 coefficient times 2 (Nmax + Y).  The Na / N* refinements
// of the k = 1 path are NOT used: a* is not known, and N* rests on c(a) being the smallest cost.  So the tile of b has a
// minimum <= thr and is a candidate; the select evaluates c_T(b) exactly and orders by (cost, row), which is the stable
// argsort order, ties included.  If the k rows behind U had no finite direct cost (overflow), fewer than k rows would be
// found among the candidates: that observation is flagged and decided by the brute force, like every other doubt.
constexpr int LUT_TOPK_MAXK = 256;
constexpr int LUT_TOPK_BUF = 512;            // LDS entries per wave of the select (>= LUT_TOPK_MAXK + 64)
constexpr int LUT_TOPK_MAXPART = 512;        // partial results per observation the bound kernel holds in registers (16 / lane)
constexpr int LUT_TOPK_CHUNK = 65536;        // observations per pass (bounds the partial results and candidate lists)
// ctl words of the top-k call: [0] Nmax, [1] flagged observations, [2] candidate tiles (sum), [3] candidate tiles (maximum)
constexpr int LUT_TOPK_CTL_WORDS = 4;
__host__ __device__ inline int lut_topk_cap(int k) { return 4 * k + 64; }

template <typename T> struct LutKey;
template <> struct LutKey<float> {            // order-preserving map of a finite float onto an unsigned integer
  static __device__ __forceinline__ unsigned long long key(float v) {
    const unsigned u = __float_as_uint(v);
    return (unsigned long long)((u >> 31) ? ~u : (u | 0x80000000u));
  }
  static __device__ __forceinline__ float value(unsigned long long k) {
    const unsigned q = (unsigned)k;
    return __uint_as_float((q >> 31) ? (q ^ 0x80000000u) : ~q);
  }
  static constexpr int bits = 32;
};
template <> struct LutKey<double> {
  static __device__ __forceinline__ unsigned long long key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
  }
  static constexpr int bits = 64;
};
constexpr unsigned long long LUT_NOKEY = ~0ull;     // above every finite key of either type

// U of observation m: the k-th smallest finite value among its 2 npart partial values (best, sec); +inf if fewer than k are
// finite.  Called by the whole wave (lane = threadIdx.x & 63); every lane returns U.
template <typename T>
__device__ __forceinline__ T lut_topk_kth(const T* __restrict__ part_cost, const T* __restrict__ part_sec, int64_t m, int64_t M,
                                          int npart, int k, int lane) {
  constexpr int NV = 2 * LUT_TOPK_MAXPART / 64;
  unsigned long long v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int q = lane + 64 * i;
    T c = (T)INFINITY;
    if (q < npart) c = part_cost[(int64_t)q * M + m];
    else if (q < 2 * npart) c = part_sec[(int64_t)(q - npart) * M + m];
    v[i] = LutNum<T>::finite(c) ? LutKey<T>::key(c) : LUT_NOKEY;
  }
  auto count_le = [&](unsigned long long x) {          // finite values <= x, over the wave
    int n = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) n += v[i] <= x ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
  };
  const unsigned long long top = LutKey<T>::bits == 64 ? LUT_NOKEY - 1 : 0xffffffffull;
  T U = (T)INFINITY;
  if (count_le(top) >= k) {
    // the smallest x with count(<= x) >= k: built bit by bit from the top, keeping count(<= x - 1) < k
    unsigned long long x = 0;
    for (int b = LutKey<T>::bits - 1; b >= 0; --b) {
      const unsigned long long step = 1ull << b;
      if (count_le(x + step - 1) < k) x += step;
    }
    U = LutKey<T>::value(x);
  }
  return U;
}

// One wave per observation of the chunk: U (k-th smallest finite partial value) and thr = U + Delta; resets the
// observation's candidate count.  A non-finite thr (fewer than k finite values, a non-finite observation, overflow) makes
// the select flag the observation.
template <typename T>
__global__ __launch_bounds__(256) void k_lut_topk_bound(const T* __restrict__ part_cost, const T* __restrict__ part_sec,
                                                        const T* __restrict__ obs, const T* __restrict__ w,
                                                        const T* __restrict__ centre, int nb, int64_t M, int npart, int k,
                                                        T coef_ef, const unsigned long long* __restrict__ ctl,
                                                        T* __restrict__ thr, int* __restrict__ cand_n) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                                  // (whole wave)
  const T U = lut_topk_kth<T>(part_cost, part_sec, m, M, npart, k, lane);
  T ya = T(0);
  if (lane < nb) {
    const T yc = obs[m * nb + lane] - centre[lane];
    const T wj = w ? w[lane] : T(1);
    ya = (wj < T(0) ? -wj : wj) * yc * yc;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ya += __shfl_xor(ya, off, 64);
  const T nmax = LutNum<T>::from_bits(ctl[0]);
  if (lane == 0) {
    thr[m] = U + (coef_ef * ((nmax + ya) + (nmax + ya)) + LutNum<T>::tiny);
    cand_n[m] = 0;
  }
}

// The collect scans: k_lut_scan_mfma's GEMM, then per tile and observation the minimum over ALL the tile's rows (the lane
// groups exchange theirs) compared with thr; a hit is appended to the observation's list (order irrelevant: the select
// sorts).  The list may overflow its capacity: the count keeps growing and the select flags the observation.
template <int KS>
__global__ __launch_bounds__(256, 2) void k_lut_collect_mfma(const float* __restrict__ tiles, const float* __restrict__ obs,
                                                             const float* __restrict__ w, const float* __restrict__ centre, int nb,
                                                             int64_t ntile, int64_t M, int nslice, const float* __restrict__ thr,
                                                             int cap, int* __restrict__ cand_n, int* __restrict__ cand) {
  const int lane = threadIdx.x & 63;
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (32 * LUT_TO);
  if (m0 >= M) return;
  const int slice = blockIdx.y;
  const int j = lane & 31, half = lane >> 5;
  float bq[LUT_TO][KS], th[LUT_TO];
#pragma unroll
  for (int blk = 0; blk < LUT_TO; ++blk) {
    const int64_t m = m0 + blk * 32 + j;
    const int64_t mc = m < M ? m : M - 1;
    // NaN compares false: nothing is appended past the chunk's end, nor for a non-finite threshold (the select flags m)
    th[blk] = (m < M && LutNum<float>::finite(thr[mc])) ? thr[mc] : __builtin_nanf("");
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int col = 2 * kk + half;
      bq[blk][kk] = col < nb ? -2.0f * (w ? w[col] : 1.0f) * (obs[mc * nb + col] - centre[col]) : (col == nb ? 1.0f : 0.0f);
    }
  }
  const int64_t per = (ntile + nslice - 1) / nslice;
  const int64_t t0 = per * slice;
  const int64_t t1 = (t0 + per < ntile) ? t0 + per : ntile;
  if (t0 >= t1) return;
  const float* __restrict__ ap = tiles + t0 * (KS * 64) + lane;
  float a[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) a[kk] = ap[kk * 64];
  for (int64_t t = t0; t < t1; ++t) {
    if (t + 1 < t1) ap += KS * 64;
    float an[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) an[kk] = ap[kk * 64];
#pragma unroll
    for (int blk = 0; blk < LUT_TO; ++blk) {
      spart_f16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bq[blk][kk], acc, 0, 0, 0);
      float mn;
      asm("v_min3_f32 %0, %1, %2, %3" : "=v"(mn) : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]));
#pragma unroll
      for (int r = 3; r < 15; r += 2) asm("v_min3_f32 %0, %1, %2, %3" : "=v"(mn) : "v"(mn), "v"(acc[r]), "v"(acc[r + 1]));
      asm("v_min_f32 %0, %1, %2" : "=v"(mn) : "v"(mn), "v"(acc[15]));
      const float o = __shfl_xor(mn, 32, 64);          // the other lane group's rows of the same tile and observation
      mn = o < mn ? o : mn;
      if (half == 0 && mn <= th[blk]) {
        const int64_t m = m0 + blk * 32 + j;
        const int pos = atomicAdd(&cand_n[m], 1);
        if (pos < cap) cand[m * cap + pos] = (int)t;
      }
    }
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) a[kk] = an[kk];
  }
}

template <int KS, int TO>
__global__ __launch_bounds__(256, 2) void k_lut_collect_mfma64(const double* __restrict__ tiles, const double* __restrict__ obs,
                                                               const double* __restrict__ w, const double* __restrict__ centre,
                                                               int nb, int64_t ntile, int64_t M, int nslice,
                                                               const double* __restrict__ thr, int cap, int* __restrict__ cand_n,
                                                               int* __restrict__ cand) {
  const int lane = threadIdx.x & 63;
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (16 * TO);
  if (m0 >= M) return;
  const int slice = blockIdx.y;
  const int j = lane & 15, q = lane >> 4;
  double bq[TO][KS], th[TO];
#pragma unroll
  for (int blk = 0; blk < TO; ++blk) {
    const int64_t m = m0 + blk * 16 + j;
    const int64_t mc = m < M ? m : M - 1;
    th[blk] = (m < M && LutNum<double>::finite(thr[mc])) ? thr[mc] : __builtin_nan("");
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int col = 4 * kk + q;
      bq[blk][kk] = col < nb ? -2.0 * (w ? w[col] : 1.0) * (obs[mc * nb + col] - centre[col]) : (col == nb ? 1.0 : 0.0);
    }
  }
  const int64_t per = (ntile + nslice - 1) / nslice;
  const int64_t t0 = per * slice;
  const int64_t t1 = (t0 + per < ntile) ? t0 + per : ntile;
  if (t0 >= t1) return;
  const double* __restrict__ ap = tiles + t0 * (KS * 64) + lane;
  double a[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) a[kk] = ap[kk * 64];
  for (int64_t t = t0; t < t1; ++t) {
    if (t + 1 < t1) ap += KS * 64;
    double an[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) an[kk] = ap[kk * 64];
#pragma unroll
    for (int blk = 0; blk < TO; ++blk) {
      spart_d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bq[blk][kk], acc, 0, 0, 0);
      double mn = __builtin_fmin(__builtin_fmin(acc[0], acc[1]), __builtin_fmin(acc[2], acc[3]));
      mn = __builtin_fmin(mn, __shfl_xor(mn, 16, 64));  // the four lane groups' rows of the same tile and observation
      mn = __builtin_fmin(mn, __shfl_xor(mn, 32, 64));
      if (q == 0 && mn <= th[blk]) {
        const int64_t m = m0 + blk * 16 + j;
        const int pos = atomicAdd(&cand_n[m], 1);
        if (pos < cap) cand[m * cap + pos] = (int)t;
      }
    }
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) a[kk] = an[kk];
  }
}

// (cost key, row) lexicographic
__device__ __forceinline__ bool lut_key_less(unsigned long long ka, int ra, unsigned long long kb, int rb) {
  return ka < kb || (ka == kb && ra < rb);
}

__device__ __forceinline__ void lut_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ascending bitonic sort of a wave's LUT_TOPK_BUF (key, row) entries in LDS
__device__ __forceinline__ void lut_topk_sort(unsigned long long* sk, int* sr, int lane) {
  for (int size = 2; size <= LUT_TOPK_BUF; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = lane; i < LUT_TOPK_BUF / 2; i += 64) {
        const int t = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
        const int p = t | stride;
        const unsigned long long kt = sk[t], kp = sk[p];
        const int rt = sr[t], rp = sr[p];
        const bool up = (t & size) == 0;
        if (lut_key_less(kp, rp, kt, rt) == up) {
          sk[t] = kp; sr[t] = rp;
          sk[p] = kt; sr[p] = rt;
        }
      }
      lut_wave_sync();
    }
  }
}

// The exact top-k of one observation over a stream of rows (64 per round, one per lane).  BRUTE = false: the rows of the
// candidate tiles of chunk observation blockIdx.x * 4 + wave; BRUTE = true: every row, for the flagged observations.
// LDS: 4 waves x LUT_TOPK_BUF x 12 bytes.
template <typename T, int ROWS, bool BRUTE>
__global__ __launch_bounds__(256) void k_lut_topk_select(const T* __restrict__ lut, const T* __restrict__ obs, const T* __restrict__ w,
                                                         int nb, int64_t B, const T* __restrict__ tiles, int ks, int64_t m_off,
                                                         int64_t Mc, int k, const T* __restrict__ thr,
                                                         const int* __restrict__ cand_n,
                                                         const int* __restrict__ cand, int cap, unsigned long long* __restrict__ ctl,
                                                         int* __restrict__ flag_list, int64_t* __restrict__ out_idx,
                                                         T* __restrict__ out_cost) {
  constexpr int NG = 64 / ROWS;
  __shared__ unsigned long long skey[4][LUT_TOPK_BUF];
  __shared__ int srow[4][LUT_TOPK_BUF];
  __shared__ T ysm[4][32], wsm[32];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (threadIdx.x < 32) wsm[threadIdx.x] = (w && (int)threadIdx.x < nb) ? w[threadIdx.x] : T(0);
  __syncthreads();
  unsigned long long* sk = skey[wv];
  int* sr = srow[wv];
  T* ys = ysm[wv];
  const unsigned count = BRUTE ? (unsigned)ctl[1] : 0u;
  const int64_t nwork = BRUTE ? (int64_t)count : Mc;
  const int64_t stride_w = BRUTE ? (int64_t)gridDim.x * 4 : nwork;
  for (int64_t item = (int64_t)blockIdx.x * 4 + wv; item < nwork; item += stride_w) {
    const int64_t m = BRUTE ? (int64_t)flag_list[item] : m_off + item;
    const T yv = lane < nb ? obs[m * nb + lane] : T(0);
    lut_wave_sync();                                   // (the previous item's reads of ys are done)
    if (lane < 32) ys[lane] = yv;                      // zero-padded to 32: a padded band adds (w * 0) * 0 = 0 to the cost
    lut_wave_sync();
    int64_t* oi = out_idx + m * k;
    T* oc = out_cost + m * k;
    if (__all(LutNum<T>::finite(yv)) == 0) {           // every direct cost is NaN or +inf: nothing qualifies
      for (int i = lane; i < k; i += 64) {
        oi[i] = -1;
        oc[i] = (T)INFINITY;
      }
      continue;
    }
    int64_t nrows = B;                                 // BRUTE: rows 0 .. B-1
    int ncand = 0;
    bool flag = false;
    if (!BRUTE) {
      ncand = cand_n[item];
      flag = !LutNum<T>::finite(thr[item]) || ncand > cap;
      if (lane == 0) {
        atomicAdd(&ctl[2], (unsigned long long)ncand);
        atomicMax(&ctl[3], (unsigned long long)ncand);
      }
      nrows = flag ? 0 : (int64_t)ncand * ROWS;
    }
    for (int i = lane; i < LUT_TOPK_BUF; i += 64) {
      sk[i] = LUT_NOKEY;
      sr[i] = 0x7fffffff;
    }
    lut_wave_sync();
    int cnt = 0;
    unsigned long long tk = LUT_NOKEY;                 // the k-th entry once k are held: only better ones are admitted
    int tr = 0x7fffffff;
    for (int64_t r0 = 0; r0 < nrows; r0 += 64) {
      int64_t r = -1;
      if (BRUTE) {
        r = r0 + lane;
      } else {
        const int ci = (int)(r0 / ROWS) + lane / ROWS;
        if (ci < ncand) r = (int64_t)cand[item * cap + ci] * ROWS + lane % ROWS;
      }
      unsigned long long key = LUT_NOKEY;
      if (r >= 0 && r < B) {
        SPART_NO_CONTRACT
        const T* x = lut + r * nb;
        T c = T(0);
        for (int j = 0; j < nb; j += 4) {              // k_lut_reduce_exact's arithmetic, band for band
          const T x0 = x[j], x1 = j + 1 < nb ? x[j + 1] : T(0), x2 = j + 2 < nb ? x[j + 2] : T(0), x3 = j + 3 < nb ? x[j + 3] : T(0);
          const T d0 = x0 - ys[j], d1 = x1 - ys[j + 1], d2 = x2 - ys[j + 2], d3 = x3 - ys[j + 3];
          if (w) {
            c = c + (wsm[j] * d0) * d0;
            c = c + (wsm[j + 1] * d1) * d1;
            c = c + (wsm[j + 2] * d2) * d2;
            c = c + (wsm[j + 3] * d3) * d3;
          } else {
            c = c + d0 * d0;
            c = c + d1 * d1;
            c = c + d2 * d2;
            c = c + d3 * d3;
          }
        }
        if (LutNum<T>::finite(c) && lut_row_ok<T, ROWS>(tiles, ks, nb, r)) key = LutKey<T>::key(c);
      }
      const int ri = (int)r;
      bool take = key != LUT_NOKEY && lut_key_less(key, ri, tk, tr);
      unsigned long long mask = __ballot(take);
      if (cnt + __builtin_popcountll(mask) > LUT_TOPK_BUF) {   // full: sort, keep the best k, raise the admission bar
        lut_topk_sort(sk, sr, lane);
        cnt = cnt < k ? cnt : k;
        for (int i = cnt + lane; i < LUT_TOPK_BUF; i += 64) {
          sk[i] = LUT_NOKEY;
          sr[i] = 0x7fffffff;
        }
        if (cnt == k) {
          tk = sk[k - 1];
          tr = sr[k - 1];
        }
        lut_wave_sync();
        take = take && lut_key_less(key, ri, tk, tr);
        mask = __ballot(take);
      }
      if (take) {
        const int pos = cnt + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        sk[pos] = key;
        sr[pos] = ri;
      }
      cnt += __builtin_popcountll(mask);
      lut_wave_sync();
    }
    lut_topk_sort(sk, sr, lane);
    const int found = cnt < k ? cnt : k;
    if (!BRUTE && (flag || found < k)) {               // let the brute force decide (it also writes the outputs)
      if (lane == 0) {
        const unsigned long long pos = atomicAdd(&ctl[1], 1ull);
        flag_list[pos] = (int)m;
      }
      continue;
    }
    for (int i = lane; i < k; i += 64) {
      const bool ok = i < found;
      oi[i] = ok ? (int64_t)sr[i] : (int64_t)-1;
      oc[i] = ok ? LutKey<T>::value(sk[i]) : (T)INFINITY;
    }
  }
}

// ---- wide top-k (spart_lut_topk_wide): the k rows of smallest c_T for any 1 <= nb <= 2162
//
// The answer is spart_lut_topk's, word for word (the same c_T, order, non-finite rules and padding); only the filter is built
// for long spectra.  Nothing of the LUT is copied or re-laid out (a 1M x 2001 float32 LUT is 8 GB): the workspace grows with B
// (one norm per row) and with the observations of a chunk times nb, never with B x nb.
//   1. k_lut_centre          as above (column centres c_j)
//   2. k_lutw_norm           n_b = sum_j w_j x'_bj^2 per row (+inf for a row k_lut_prep would reject: a non-finite entry or
//                            an overflowing norm, decided by k_lut_prep's own arithmetic) and Nmax.  float32: n_b is
//                            accumulated in float64 and rounded once.
//   per chunk of at most LUTW_CHUNK observations:
//   3. k_lutw_obs            Bq = fl(-2 w_j y'_j) (the narrow scan's rounding), 1 in column nb, zero-padded to nbp = a multiple
//                            of LUTW_KC; Y = sum_j |w_j| y'_j^2 (float64, rounded once; non-finite for a non-finite observation)
//   4. k_lutw_gemm<false>    the GEMM a~(b, m) = [x'_b, n_b] . Bq_m with K streamed: a workgroup stages 128 (float32) / 64
//                            (float64) LUT rows and as many observations, LUTW_KC bands at a time, through LDS, centring the
//                            rows on the way in (fl(x - c_j), k_lut_prep's rounding; rows with n_b = +inf enter as
//                            (0, .., 0, +inf)), on v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64.  Each K chunk has its
//                            own accumulators, added to a running sum: the rounding chain of a filter value is
//                            LUTW_KC + nch long, not nb.  Per (slice, row half of the workgroup, lane group) and observation
//                            it keeps the two smallest tile minima: filter values of two distinct rows, no row behind two
//                            partial results (the narrow scan's invariant)
//   5. k_lutw_bound          U = the k-th smallest partial value (lut_topk_kth), thr = U + Delta (below)
//   6. k_lutw_gemm<true>     the same GEMM; every tile (32 / 16 rows) with a minimum <= thr goes on the candidate list
//   7. k_lutw_select<false>  one wave per observation evaluates the candidate rows with c_T (the observation and the
//                            weights in dynamic LDS, nb entries each) and keeps the k best: k_lut_topk_select's buffer
//   8. k_lutw_select<true>   brute force over every row for the flagged observations (lanes over rows, bands in order)
//
// Delta.  With the notation of the top of this file, a~(b) + Y - c(b) is bounded term by term as for the narrow scan except:
//   (ii)  float32: n_b = fl(sum w x'^2 accumulated in float64): <= (1 + (nb + 2) 2^-29) u N_b <= 1.01 u N_b;
//         float64: (nb + 2) u N_b as before;
//   (iv)  each term of the dot product (n_b included) passes through at most LUTW_KC roundings inside its chunk's MFMA chain
//         and nch - 1 additions of chunk sums (the first chunk is copied, not added): h = LUTW_KC + nch + 1 is a safe depth,
//         and the error is <= h u (|n_b| + 2 sum |w x' y'|) <= 2 h u (N_b + Y);
//   =>    E_b <= ce (N_b + Y),  ce = (4 + nn + 1 + 2 h) u,  nn = 1.01 (float32) / nb + 2 (float64)
//   (v)   the direct evaluation: |c_T(b) - c(b)| <= F_b = (nb + 3) u sum |w| d_b^2.
// For the k rows a_1..a_k behind U and a* the one of largest c_T (the narrow argument): every b with c_T(b) <= c_k satisfies
//     a~(b) <= U + E_a* + E_b + F_a* + F_b.
// E: N_a*, N_b <= Nmax.  F: with non-negative weights sum |w| d^2 = c itself, and
//     c(a*) <= a~(a*) + Y + E_a* <= C1 = U + Y + ce (Nmax + Y),   c(b) <= c(a*) (1 + f) / (1 - f),  f = (nb + 3) u,
// so F_a* + F_b <= 2.01 (nb + 3) u max(C1, 0).  That is the term that made the narrow Delta grow with 3 nb: here it scales with
// the cost of the rows that matter, not with their norms.  With a negative weight F falls back to (2 nb + 6) u (Nmax + Y) per row.
//     Delta = 2 ce (Nmax + Y) + F,   every coefficient times 1.01,
// evaluated in float64 and rounded up to the dtype (thr = t + 4 u |t| + tiny covers the rounding of t = U + Delta itself).
// float32, nb = 211: ce = 86 u (the narrow rule's 2 x (3 nb + 2 K + 16) u would be 2 146 u per (Nmax + Y)).
constexpr int LUTW_KC = 32;                  // bands per K chunk staged through LDS
constexpr int LUTW_TR = 2, LUTW_TB = 2;      // LUT tiles x observation blocks per wave; the four waves are 2 x 2
constexpr int LUTW_CHUNK = 16384;            // observations per pass (bounds Bq, the partial results and the candidate lists)
constexpr int LUTW_SELECT_BLOCKS = 8192;     // single-wave workgroups of the brute-force select

template <typename T> struct LutWide;
template <> struct LutWide<float> {          // v_mfma_f32_32x32x2_f32: 32 rows x 32 observations, K steps of 2, 2 lane groups
  static constexpr int ROWS = 32, KSTEP = 2, NACC = 16;
  typedef spart_f16v acc_t;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
template <> struct LutWide<double> {         // v_mfma_f64_16x16x4_f64: 16 x 16, K steps of 4, 4 lane groups
  static constexpr int ROWS = 16, KSTEP = 4, NACC = 4;
  typedef spart_d4v acc_t;
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};

// one thread per LUT row: k_lut_prep's acceptance test and Nmax, and the filter norm n_b (+inf for a rejected row)
template <typename T>
__global__ __launch_bounds__(256) void k_lutw_norm(const T* __restrict__ lut, const T* __restrict__ w, const T* __restrict__ centre,
                                                   int nb, int64_t B, T* __restrict__ norm, unsigned long long* __restrict__ ctl) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  T na = T(0);
  if (row < B) {
    bool ok = true;
    T n = T(0);
    double nd = 0.0;
    const T* x = lut + row * nb;
    for (int j = 0; j < nb; ++j) {                     // (k_lut_prep's loop, plus the float64 accumulation)
      const T v = x[j];
      ok = ok && LutNum<T>::finite(v);
      const T xc = v - centre[j];
      const T wj = w ? w[j] : T(1);
      n += wj * xc * xc;
      na += (wj < T(0) ? -wj : wj) * xc * xc;
      if (sizeof(T) == 4) nd += (double)wj * (double)xc * (double)xc;
    }
    ok = ok && LutNum<T>::finite(n) && LutNum<T>::finite(na);
    if (!ok) na = T(0);
    norm[row] = ok ? (sizeof(T) == 4 ? (T)nd : n) : (T)INFINITY;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_down(na, off, 64);
    na = o > na ? o : na;
  }
  if ((threadIdx.x & 63) == 0 && na > T(0)) atomicMax(&ctl[0], LutNum<T>::bits(na));
}

// one wave per observation of the chunk: the GEMM operand row Bq (nbp entries) and Y
template <typename T>
__global__ __launch_bounds__(256) void k_lutw_obs(const T* __restrict__ obs, const T* __restrict__ w, const T* __restrict__ centre,
                                                  int nb, int nbp, int64_t M, T* __restrict__ bq, T* __restrict__ ya) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                                  // (whole wave)
  double y = 0.0;
  for (int j = lane; j < nbp; j += 64) {
    T v = j == nb ? T(1) : T(0);
    if (j < nb) {
      const T wj = w ? w[j] : T(1);
      const T yc = obs[m * nb + j] - centre[j];
      v = T(-2) * wj * yc;                             // the narrow scan's operand, -2.0 * w * (y - c)
      y += (double)(wj < T(0) ? -wj : wj) * (double)yc * (double)yc;
    }
    bq[m * nbp + j] = v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) y += __shfl_xor(y, off, 64);
  if (lane == 0) ya[m] = (T)y;
}

// The K-streamed GEMM of the scan (COLLECT = false: partial results) and of the collect pass (COLLECT = true: candidate
// tiles).  Grid (observation blocks of 2 TB ROWS, slices of row blocks of 2 TR ROWS); wave (wr, wc) computes TR tiles x TB
// observation blocks of the workgroup's block.
template <typename T, bool COLLECT>
__global__ __launch_bounds__(256) void k_lutw_gemm(const T* __restrict__ lut, const T* __restrict__ norm, const T* __restrict__ centre,
                                                   int nb, int64_t B, const T* __restrict__ bq, int nbp, int64_t M, int nslice,
                                                   T* __restrict__ part_cost, T* __restrict__ part_sec, const T* __restrict__ thr,
                                                   int cap, int* __restrict__ cand_n, int* __restrict__ cand) {
  using W = LutWide<T>;
  constexpr int ROWS = W::ROWS, KSTEP = W::KSTEP, NACC = W::NACC, G = 64 / ROWS, KC = LUTW_KC;
  constexpr int TR = LUTW_TR, TB = LUTW_TB, RWG = 2 * TR * ROWS, OWG = 2 * TB * ROWS;
  constexpr int PA = RWG + 1, PB = OWG + 1;            // LDS row pitches ([k][row]; +1: the transposing stores spread over banks)
  __shared__ T As[KC * PA], Bs[KC * PB], nsm[RWG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int col = lane % ROWS, grp = lane / ROWS;      // operand lane: row / observation col of the tile, k = grp
  const int64_t m0 = (int64_t)blockIdx.x * OWG;
  const int slice = blockIdx.y;
  const int64_t ntile = (B + ROWS - 1) / ROWS;
  const int64_t nrb = (B + RWG - 1) / RWG;
  const int64_t per = (nrb + nslice - 1) / nslice;
  const int64_t rb0 = per * slice;
  const int64_t rb1 = rb0 + per < nrb ? rb0 + per : nrb;
  T best[TB], sec[TB], th[TB];
#pragma unroll
  for (int b2 = 0; b2 < TB; ++b2) {
    const int64_t m = m0 + (wc * TB + b2) * ROWS + col;
    best[b2] = (T)INFINITY;
    sec[b2] = (T)INFINITY;
    // NaN compares false: nothing is appended past the chunk's end, nor for a non-finite threshold (the select flags m)
    th[b2] = (T)__builtin_nan("");
    if (COLLECT && m < M && LutNum<T>::finite(thr[m])) th[b2] = thr[m];
  }
  for (int64_t rb = rb0; rb < rb1; ++rb) {
    const int64_t r0 = rb * RWG;
    __syncthreads();                                   // (the previous block's LDS is read)
    if (tid < RWG) nsm[tid] = r0 + tid < B ? norm[r0 + tid] : (T)INFINITY;
    typename W::acc_t run[TR][TB];
    for (int k0 = 0; k0 < nbp; k0 += KC) {
      __syncthreads();
      for (int e = tid; e < RWG * KC; e += 256) {     // LUT rows, centred on the way in; column nb = n_b
        const int r = e / KC, j = e % KC, kk = k0 + j;
        const T n = nsm[r];
        T v = T(0);
        if (kk < nb) {
          if (LutNum<T>::finite(n)) v = lut[(r0 + r) * nb + kk] - centre[kk];
        } else if (kk == nb) {
          v = n;
        }
        As[j * PA + r] = v;
      }
      for (int e = tid; e < OWG * KC; e += 256) {
        const int mm = e / KC, j = e % KC;
        const int64_t m = m0 + mm;
        Bs[j * PB + mm] = m < M ? bq[m * nbp + k0 + j] : T(0);
      }
      __syncthreads();
      typename W::acc_t acc[TR][TB];
#pragma unroll
      for (int t2 = 0; t2 < TR; ++t2)
#pragma unroll
        for (int b2 = 0; b2 < TB; ++b2)
#pragma unroll
          for (int i = 0; i < NACC; ++i) acc[t2][b2][i] = T(0);
#pragma unroll
      for (int s = 0; s < KC / KSTEP; ++s) {
        const int kq = s * KSTEP + grp;
        T a[TR], b[TB];
#pragma unroll
        for (int t2 = 0; t2 < TR; ++t2) a[t2] = As[kq * PA + (wr * TR + t2) * ROWS + col];
#pragma unroll
        for (int b2 = 0; b2 < TB; ++b2) b[b2] = Bs[kq * PB + (wc * TB + b2) * ROWS + col];
#pragma unroll
        for (int t2 = 0; t2 < TR; ++t2)
#pragma unroll
          for (int b2 = 0; b2 < TB; ++b2) acc[t2][b2] = W::mfma(a[t2], b[b2], acc[t2][b2]);
      }
#pragma unroll
      for (int t2 = 0; t2 < TR; ++t2)
#pragma unroll
        for (int b2 = 0; b2 < TB; ++b2) {
          if (k0 == 0) run[t2][b2] = acc[t2][b2];
          else {
#pragma unroll
            for (int i = 0; i < NACC; ++i) run[t2][b2][i] = run[t2][b2][i] + acc[t2][b2][i];
          }
        }
    }
#pragma unroll
    for (int t2 = 0; t2 < TR; ++t2) {
      const int64_t tg = rb * (2 * TR) + wr * TR + t2;  // tile of ROWS LUT rows
      if (tg >= ntile) break;                           // (wave-uniform)
#pragma unroll
      for (int b2 = 0; b2 < TB; ++b2) {
        T mn = run[t2][b2][0];
#pragma unroll
        for (int i = 1; i < NACC; ++i) mn = __builtin_fmin(mn, run[t2][b2][i]);
        if (mn != mn) mn = (T)INFINITY;                // (an overflowing dot product of a rejected row: never a minimum)
        if (!COLLECT) {
          sec[b2] = __builtin_fmin(sec[b2], __builtin_fmax(best[b2], mn));   // a tie with the best becomes `sec`
          best[b2] = __builtin_fmin(best[b2], mn);
        } else {
#pragma unroll
          for (int off = ROWS; off < 64; off <<= 1) mn = __builtin_fmin(mn, __shfl_xor(mn, off, 64));   // all rows of the tile
          if (grp == 0 && mn <= th[b2]) {
            const int64_t m = m0 + (wc * TB + b2) * ROWS + col;
            const int pos = atomicAdd(&cand_n[m], 1);
            if (pos < cap) cand[m * cap + pos] = (int)tg;
          }
        }
      }
    }
  }
  if (!COLLECT) {
#pragma unroll
    for (int b2 = 0; b2 < TB; ++b2) {
      const int64_t m = m0 + (wc * TB + b2) * ROWS + col;
      if (m < M) {
        const int64_t o = (((int64_t)slice * 2 + wr) * G + grp) * M + m;
        part_cost[o] = best[b2];
        part_sec[o] = sec[b2];
      }
    }
  }
}

// one wave per observation of the chunk: thr = U + Delta (the derivation above; ce, cf, cw are its coefficients with the
// 1 % slack), resets the candidate count
template <typename T>
__global__ __launch_bounds__(256) void k_lutw_bound(const T* __restrict__ part_cost, const T* __restrict__ part_sec,
                                                    const T* __restrict__ ya, const T* __restrict__ w, int nb, int64_t M, int npart,
                                                    int k, double ce, double cf, double cw, const unsigned long long* __restrict__ ctl,
                                                    T* __restrict__ thr, int* __restrict__ cand_n) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                                  // (whole wave)
  const T U = lut_topk_kth<T>(part_cost, part_sec, m, M, npart, k, lane);
  bool neg = false;
  if (w)
    for (int j = lane; j < nb; j += 64) neg = neg || w[j] < T(0);
  neg = __any(neg) != 0;
  if (lane == 0) {
    const double Y = (double)ya[m], nmax = (double)LutNum<T>::from_bits(ctl[0]);
    const double E = ce * (nmax + Y);
    double F;
    if (!neg) {
      const double c1 = (double)U + Y + E;
      F = cf * (c1 > 0.0 ? c1 : 0.0);
    } else {
      F = cw * (nmax + Y);
    }
    double t = (double)U + (2.0 * E + F);
    t = t + (4.0 * (double)LutNum<T>::u * __builtin_fabs(t) + (double)LutNum<T>::tiny);
    T tt = (T)t;                                       // (NaN / inf stay non-finite: the select flags m)
    if constexpr (sizeof(T) == 4) {
      if ((double)tt < t) {                            // round up: the next float above
        const unsigned b = __float_as_uint(tt);
        tt = tt > 0.0f ? __uint_as_float(b + 1u) : (tt == 0.0f ? __uint_as_float(1u) : __uint_as_float(b - 1u));
      }
    }
    thr[m] = tt;
    cand_n[m] = 0;
  }
}

// The exact top-k of one observation (k_lut_topk_select for any nb): single-wave workgroups; dynamic LDS = the key / row
// buffer, the observation and the weights (LUT_TOPK_BUF x 12 + 2 nb sizeof(T) bytes: 40.7 KB at nb = 2162 in float64).
// BRUTE = false: the rows of the candidate tiles of chunk observation blockIdx.x; BRUTE = true: every row, for the flagged ones.
// OBSW = true (spart_lut_topk_obs_weights): w is (M, nb), one weight row per observation, loaded with the observation; a band
// of weight zero is skipped; an observation with a negative or non-finite weight, or a non-finite value in a band of non-zero
// weight, matches nothing.  In every variant a row counts only if its norm is finite (k_lutw_norm's verdict: with the shared
// weights, or without weights for OBSW), whatever the observation and whichever path evaluates it.
template <typename T, int ROWS, bool BRUTE, bool OBSW = false>
__global__ __launch_bounds__(64) void k_lutw_select(const T* __restrict__ lut, const T* __restrict__ obs, const T* __restrict__ w,
                                                    int nb, int64_t B, int64_t m_off, int64_t Mc, int k, const T* __restrict__ thr,
                                                    const int* __restrict__ cand_n, const int* __restrict__ cand, int cap,
                                                    unsigned long long* __restrict__ ctl, int* __restrict__ flag_list,
                                                    int64_t* __restrict__ out_idx, T* __restrict__ out_cost,
                                                    const T* __restrict__ norm) {
  extern __shared__ __attribute__((aligned(16))) char lutw_smem[];
  unsigned long long* sk = reinterpret_cast<unsigned long long*>(lutw_smem);
  int* sr = reinterpret_cast<int*>(sk + LUT_TOPK_BUF);
  T* ys = reinterpret_cast<T*>(sr + LUT_TOPK_BUF);
  T* wsm = ys + nb;
  const int lane = threadIdx.x & 63;
  if constexpr (!OBSW) {
    if (w)
      for (int j = lane; j < nb; j += 64) wsm[j] = w[j];
  }
  const unsigned count = BRUTE ? (unsigned)ctl[1] : 0u;
  const int64_t nwork = BRUTE ? (int64_t)count : Mc;
  const int64_t stride_w = BRUTE ? (int64_t)gridDim.x : nwork;
  for (int64_t item = blockIdx.x; item < nwork; item += stride_w) {
    const int64_t m = BRUTE ? (int64_t)flag_list[item] : m_off + item;
    lut_wave_sync();                                   // (the previous item's reads of ys are done)
    bool fin = true;
    for (int j = lane; j < nb; j += 64) {
      const T v = obs[m * nb + j];
      ys[j] = v;
      if constexpr (OBSW) {
        const T wj = w[m * nb + j];
        wsm[j] = wj;
        fin = fin && wj >= T(0) && LutNum<T>::finite(wj) && (wj == T(0) || LutNum<T>::finite(v));
      } else {
        fin = fin && LutNum<T>::finite(v);
      }
    }
    lut_wave_sync();
    int64_t* oi = out_idx + m * k;
    T* oc = out_cost + m * k;
    if (__all(fin) == 0) {                             // every direct cost is NaN or +inf: nothing qualifies
      for (int i = lane; i < k; i += 64) {
        oi[i] = -1;
        oc[i] = (T)INFINITY;
      }
      continue;
    }
    int64_t nrows = B;
    int ncand = 0;
    bool flag = false;
    if (!BRUTE) {
      ncand = cand_n[item];
      flag = !LutNum<T>::finite(thr[item]) || ncand > cap;
      if (lane == 0) {
        atomicAdd(&ctl[2], (unsigned long long)ncand);
        atomicMax(&ctl[3], (unsigned long long)ncand);
      }
      nrows = flag ? 0 : (int64_t)ncand * ROWS;
    }
    for (int i = lane; i < LUT_TOPK_BUF; i += 64) {
      sk[i] = LUT_NOKEY;
      sr[i] = 0x7fffffff;
    }
    lut_wave_sync();
    int cnt = 0;
    unsigned long long tk = LUT_NOKEY;
    int tr = 0x7fffffff;
    for (int64_t r0 = 0; r0 < nrows; r0 += 64) {
      int64_t r = -1;
      if (BRUTE) {
        r = r0 + lane;
      } else {
        const int ci = (int)(r0 / ROWS) + lane / ROWS;
        if (ci < ncand) r = (int64_t)cand[item * cap + ci] * ROWS + lane % ROWS;
      }
      unsigned long long key = LUT_NOKEY;
      if (r >= 0 && r < B) {
        SPART_NO_CONTRACT
        const T* x = lut + r * nb;
        T c = T(0);
        if (!LutNum<T>::finite(norm[r])) {
          c = (T)INFINITY;                                              // a rejected row: never a candidate
        } else if constexpr (OBSW) {
          for (int j = 0; j < nb; ++j) {
            const T wj = wsm[j];
            if (wj == T(0)) continue;                                   // the mask: no operation at all
            const T d = x[j] - ys[j];
            c = c + (wj * d) * d;
          }
        } else if (w) {
          for (int j = 0; j < nb; ++j) {
            const T d = x[j] - ys[j];
            c = c + (wsm[j] * d) * d;
          }
        } else {
          for (int j = 0; j < nb; ++j) {
            const T d = x[j] - ys[j];
            c = c + d * d;
          }
        }
        if (LutNum<T>::finite(c)) key = LutKey<T>::key(c);
      }
      const int ri = (int)r;
      bool take = key != LUT_NOKEY && lut_key_less(key, ri, tk, tr);
      unsigned long long mask = __ballot(take);
      if (cnt + __builtin_popcountll(mask) > LUT_TOPK_BUF) {   // full: sort, keep the best k, raise the admission bar
        lut_topk_sort(sk, sr, lane);
        cnt = cnt < k ? cnt : k;
        for (int i = cnt + lane; i < LUT_TOPK_BUF; i += 64) {
          sk[i] = LUT_NOKEY;
          sr[i] = 0x7fffffff;
        }
        if (cnt == k) {
          tk = sk[k - 1];
          tr = sr[k - 1];
        }
        lut_wave_sync();
        take = take && lut_key_less(key, ri, tk, tr);
        mask = __ballot(take);
      }
      if (take) {
        const int pos = cnt + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        sk[pos] = key;
        sr[pos] = ri;
      }
      cnt += __builtin_popcountll(mask);
      lut_wave_sync();
    }
    lut_topk_sort(sk, sr, lane);
    const int found = cnt < k ? cnt : k;
    if (!BRUTE && (flag || found < k)) {               // let the brute force decide (it also writes the outputs)
      if (lane == 0) {
        const unsigned long long pos = atomicAdd(&ctl[1], 1ull);
        flag_list[pos] = (int)m;
      }
      continue;
    }
    for (int i = lane; i < k; i += 64) {
      const bool ok = i < found;
      oi[i] = ok ? (int64_t)sr[i] : (int64_t)-1;
      oc[i] = ok ? LutKey<T>::value(sk[i]) : (T)INFINITY;
    }
  }
}

// ---- per-observation weights (spart_lut_topk_obs_weights): the k rows of smallest
//
//     c_T(b, m):  c = 0;  for j = 0 .. nb-1:  if (w_mj == 0) continue;  d = x_bj - y_mj;  c = c + (w_mj * d) * d
//
// for any 1 <= nb <= 2162, with a weight row w_m per observation.  A band of weight zero adds no operation, so y_mj may be NaN
// or inf there: that is the mask.  A row is accepted by k_lutw_norm without weights (finite entries, finite unweighted centred
// norm), whatever the observation; an observation with a negative or non-finite weight, or a non-finite value in a band of
// non-zero weight, matches no row.  Order, padding and the non-finite rules are otherwise spart_lut_topk_wide's.
//   1. k_lut_centre, k_lutw_norm (w = NULL)   centres, and n_b = +inf for a rejected row (the filter norm itself is unused)
//   2. k_lutow_q             Q_j = max over the accepted rows of fl(x'_bj^2), the per-band scale of the bound
//   per chunk of observations:
//   3. k_lutow_obs           the operand row Bq_m = [(w_mj, fl(-2 w_mj y'_mj)) for j < nb, (1, 0), (0, 0) ...] (pairs, zero for a
//                            masked band), Y_m = sum w_mj y'_mj^2 and Nbound_m = sum w_mj Q_j (float64); Y_m = NaN for an
//                            observation the filter must not touch (invalid, or an operand that overflows)
//   4. k_lutow_gemm<false>   a~(b, m) = sum_j w_mj fl(x'_bj^2) - 2 w_mj y'_mj x'_bj: K = 2 nbp, LUT rows staged once per
//                            LUTW_KC-band chunk exactly as k_lutw_gemm does, the squares formed in registers.  On
//                            v_mfma_f32_32x32x2_f32 an MFMA takes one band (lane group 0: x'^2 against w, group 1: x' against
//                            -2 w y'); on v_mfma_f64_16x16x4_f64 two.  A rejected row enters as x' = 0 in every band and
//                            2^100 / 2^600 in the extra slot (band nb, operand (1, 0)): its square is +inf, its product with
//                            0 is 0, so its filter value is +inf and it is never a minimum.  Partial results as k_lutw_gemm.
//   5. k_lutow_bound         thr = U + Delta (below); NaN when Y_m or Nbound_m is non-finite or 4 (Nbound_m + Y_m) overflows
//   6. k_lutow_gemm<true>    candidate tiles under thr
//   7. k_lutw_select<., ., false, true>   the exact top-k over the candidate rows: the observation's own weight row in the
//                            select's dynamic LDS, the zero-skip rule, the row rule through n_b
//   8. k_lutw_select<., ., true, true>    the brute force for the flagged observations
//
// Delta.  N_bm = sum_j w_mj x'_bj^2 over the accepted row b, Y_m = sum_j w_mj y'_mj^2, c(b) the real-number cost, all sums over
// the bands of non-zero weight (a masked band adds exactly 0 to a~ and to c_T).  The weights are non-negative by definition.
//   (i)   centring: | sum w (x - y)^2 - sum w (x' - y')^2 |                <= 4 u (N_bm + Y_m)
//   (ii)  the squares: | sum w fl(x'^2) - sum w x'^2 |                      <= u N_bm
//   (iii) Bq = fl(-2 w y') (the -2 w is exact): | 2 sum w x' y' e |         <= u (N_bm + Y_m)
//   (iv)  a K chunk carries 2 LUTW_KC operand entries; every term passes through at most 2 LUTW_KC roundings in its chunk's MFMA
//         chain and nch - 1 additions of chunk sums: depth h = 2 LUTW_KC + nch + 1 over terms whose absolute sum is
//         sum w fl(x'^2) + 2 sum w |x' y'| <= 2 (N_bm + Y_m) (to first order), so the error is <= 2 h u (N_bm + Y_m)
//   =>    | a~(b) + Y_m - c(b) | <= E_b = ce (N_bm + Y_m),  ce = (4 + 1 + 1 + 2 h) u
//   (v)   the direct evaluation: skipping a band adds no rounding, so |c_T(b) - c(b)| <= F_b = (nb + 3) u c(b).
// For the k rows a_1..a_k behind U and a* the one of largest c_T (the narrow argument) every b with c_T(b) <= c_k satisfies
//     a~(b) <= U + E_a* + E_b + F_a* + F_b.
// N for the rows that matter (a* and every such b), with N_0 = Nbound_m = sum_j w_mj Q_j >= N_bm for every accepted row:
//     c(a*) <= a~(a*) + Y_m + E_a* <= C(N) = max(U + Y_m + ce (N + Y_m), 0)  and  c(b) <= c(a*) (1 + f) / (1 - f), f = (nb + 3) u;
//     sqrt(N_b) = |x'_b|_w <= |y'|_w + |x'_b - y'|_w = sqrt(Y_m) + sqrt(c'(b)), c'(b) <= c(b) + 4 u (N + Y_m) (term (i)),
//   so N_{i+1} = min(N_i, (sqrt(Y_m) + sqrt(C(N_i) (1 + f) / (1 - f) + 4 u (N_i + Y_m)))^2) bounds N_a* and N_b again; two steps
//   are taken.  With relative-noise weights (w ~ 1 / y^2) Nbound_m can be 10^4 x Y_m; N_2 is about Y_m.
// Then E_a* + E_b <= 2 ce (N_2 + Y_m) and F_a* + F_b <= 2.01 (nb + 3) u C(N_2):
//     Delta = 2 ce (N_2 + Y_m) + cf C(N_2),   every coefficient times 1.01,
// evaluated in float64 (the square roots and the squares with 1 % slack) and rounded up to the dtype as k_lutw_bound does.
// Workspace: Bq is 2 nbp entries per observation; the chunk is LUTW_CHUNK observations, cut so that Bq stays within
// LUTOW_BQ_BYTES (float64 at 2162 bands: 7 168 observations per chunk).
constexpr size_t LUTOW_BQ_BYTES = size_t(1) << 28;

// Q_j (bit patterns of non-negative values, combined with atomicMax): grid (bands / 64, row slices), a wave reads 64
// consecutive bands of one row at a time
template <typename T>
__global__ __launch_bounds__(256) void k_lutow_q(const T* __restrict__ lut, const T* __restrict__ norm, const T* __restrict__ centre,
                                                 int nb, int64_t B, unsigned long long* __restrict__ qb) {
  __shared__ T qs[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  T mx = T(0);
  if (j < nb) {
    const T c = centre[j];
    for (int64_t r = (int64_t)blockIdx.y * 4 + wv; r < B; r += (int64_t)gridDim.y * 4)
      if (LutNum<T>::finite(norm[r])) {
        const T xc = lut[r * nb + j] - c;
        const T sq = xc * xc;                          // k_lutow_gemm's square, rounding for rounding
        mx = sq > mx ? sq : mx;
      }
  }
  qs[wv][lane] = mx;
  __syncthreads();
  if (wv == 0 && j < nb) {
#pragma unroll
    for (int i = 1; i < 4; ++i) mx = qs[i][lane] > mx ? qs[i][lane] : mx;
    if (mx > T(0)) atomicMax(&qb[j], LutNum<T>::bits(mx));
  }
}

// one wave per observation of the chunk: the operand pairs Bq (2 nbp entries), and yn[2 m] = Y_m, yn[2 m + 1] = Nbound_m;
// ctl[0] = the largest finite Nbound_m (bit pattern in the dtype)
template <typename T>
__global__ __launch_bounds__(256) void k_lutow_obs(const T* __restrict__ obs, const T* __restrict__ w, const T* __restrict__ centre,
                                                   const unsigned long long* __restrict__ qb, int nb, int nbp, int64_t M,
                                                   T* __restrict__ bq, double* __restrict__ yn, unsigned long long* __restrict__ ctl) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                                  // (whole wave)
  double y = 0.0, nq = 0.0;
  bool bad = false;
  for (int j = lane; j < nbp; j += 64) {
    T v0 = j == nb ? T(1) : T(0), v1 = T(0);
    if (j < nb) {
      const T wj = w[m * nb + j];
      bad = bad || !(wj >= T(0)) || !LutNum<T>::finite(wj);
      if (wj != T(0)) {
        const T yv = obs[m * nb + j];
        const T yc = yv - centre[j];
        v0 = wj;
        v1 = T(-2) * wj * yc;                          // k_lutw_obs's operand, -2.0 * w * (y - c)
        bad = bad || !LutNum<T>::finite(yv) || !LutNum<T>::finite(v1);
        y += (double)wj * (double)yc * (double)yc;
        nq += (double)wj * (double)LutNum<T>::from_bits(qb[j]);
      }
      if (!LutNum<T>::finite(v0) || !LutNum<T>::finite(v1)) v0 = v1 = T(0);   // no NaN reaches the GEMM
    }
    bq[m * 2 * nbp + 2 * j] = v0;
    bq[m * 2 * nbp + 2 * j + 1] = v1;
  }
  bad = __any(bad) != 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    y += __shfl_xor(y, off, 64);
    nq += __shfl_xor(nq, off, 64);
  }
  if (lane == 0) {
    yn[2 * m] = bad ? __builtin_nan("") : y;
    yn[2 * m + 1] = nq;
    const T nt = (T)nq;
    if (!bad && LutNum<T>::finite(nt)) atomicMax(&ctl[0], LutNum<T>::bits(nt));
  }
}

// k_lutw_gemm with K = 2 nbp: the operand pairs of the observation-weighted cost (the derivation above)
template <typename T, bool COLLECT>
__global__ __launch_bounds__(256) void k_lutow_gemm(const T* __restrict__ lut, const T* __restrict__ norm, const T* __restrict__ centre,
                                                    int nb, int64_t B, const T* __restrict__ bq, int nbp, int64_t M, int nslice,
                                                    T* __restrict__ part_cost, T* __restrict__ part_sec, const T* __restrict__ thr,
                                                    int cap, int* __restrict__ cand_n, int* __restrict__ cand) {
  using W = LutWide<T>;
  constexpr int ROWS = W::ROWS, KSTEP = W::KSTEP, NACC = W::NACC, G = 64 / ROWS, KC = LUTW_KC, KQ = 2 * KC;
  constexpr int TR = LUTW_TR, TB = LUTW_TB, RWG = 2 * TR * ROWS, OWG = 2 * TB * ROWS;
  constexpr int PA = RWG + 1, PB = OWG + 1;            // LDS row pitches ([k][row]; +1: the transposing stores spread over banks)
  const T huge = sizeof(T) == 4 ? (T)0x1p100 : (T)0x1p600;   // squares to +inf
  __shared__ T As[KC * PA], Bs[KQ * PB], nsm[RWG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int col = lane % ROWS, grp = lane / ROWS;      // operand lane: row / observation col of the tile, k = grp
  const bool sq = (grp & 1) == 0;                      // this lane's K entries are the squares (against w)
  const int64_t m0 = (int64_t)blockIdx.x * OWG;
  const int slice = blockIdx.y;
  const int64_t ntile = (B + ROWS - 1) / ROWS;
  const int64_t nrb = (B + RWG - 1) / RWG;
  const int64_t per = (nrb + nslice - 1) / nslice;
  const int64_t rb0 = per * slice;
  const int64_t rb1 = rb0 + per < nrb ? rb0 + per : nrb;
  const int64_t bqp = 2 * (int64_t)nbp;
  T best[TB], sec[TB], th[TB];
#pragma unroll
  for (int b2 = 0; b2 < TB; ++b2) {
    const int64_t m = m0 + (wc * TB + b2) * ROWS + col;
    best[b2] = (T)INFINITY;
    sec[b2] = (T)INFINITY;
    th[b2] = (T)__builtin_nan("");
    if (COLLECT && m < M && LutNum<T>::finite(thr[m])) th[b2] = thr[m];
  }
  for (int64_t rb = rb0; rb < rb1; ++rb) {
    const int64_t r0 = rb * RWG;
    __syncthreads();                                   // (the previous block's LDS is read)
    if (tid < RWG) nsm[tid] = r0 + tid < B ? norm[r0 + tid] : (T)INFINITY;
    typename W::acc_t run[TR][TB];
    for (int k0 = 0; k0 < nbp; k0 += KC) {
      __syncthreads();
      for (int e = tid; e < RWG * KC; e += 256) {     // LUT rows, centred on the way in; band nb = the rejection slot
        const int r = e / KC, j = e % KC, kk = k0 + j;
        const bool ok = LutNum<T>::finite(nsm[r]);
        T v = T(0);
        if (kk < nb) {
          if (ok) v = lut[(r0 + r) * nb + kk] - centre[kk];
        } else if (kk == nb) {
          v = ok ? T(0) : huge;
        }
        As[j * PA + r] = v;
      }
      for (int e = tid; e < OWG * KQ; e += 256) {
        const int mm = e / KQ, j = e % KQ;
        const int64_t m = m0 + mm;
        Bs[j * PB + mm] = m < M ? bq[m * bqp + 2 * (int64_t)k0 + j] : T(0);
      }
      __syncthreads();
      typename W::acc_t acc[TR][TB];
#pragma unroll
      for (int t2 = 0; t2 < TR; ++t2)
#pragma unroll
        for (int b2 = 0; b2 < TB; ++b2)
#pragma unroll
          for (int i = 0; i < NACC; ++i) acc[t2][b2][i] = T(0);
#pragma unroll
      for (int s = 0; s < KQ / KSTEP; ++s) {
        const int kq = s * KSTEP + grp, band = kq >> 1;
        T a[TR], b[TB];
#pragma unroll
        for (int t2 = 0; t2 < TR; ++t2) {
          const T x = As[band * PA + (wr * TR + t2) * ROWS + col];
          a[t2] = x * (sq ? x : T(1));                 // fl(x'^2), or x' itself
        }
#pragma unroll
        for (int b2 = 0; b2 < TB; ++b2) b[b2] = Bs[kq * PB + (wc * TB + b2) * ROWS + col];
#pragma unroll
        for (int t2 = 0; t2 < TR; ++t2)
#pragma unroll
          for (int b2 = 0; b2 < TB; ++b2) acc[t2][b2] = W::mfma(a[t2], b[b2], acc[t2][b2]);
      }
#pragma unroll
      for (int t2 = 0; t2 < TR; ++t2)
#pragma unroll
        for (int b2 = 0; b2 < TB; ++b2) {
          if (k0 == 0) run[t2][b2] = acc[t2][b2];
          else {
#pragma unroll
            for (int i = 0; i < NACC; ++i) run[t2][b2][i] = run[t2][b2][i] + acc[t2][b2][i];
          }
        }
    }
#pragma unroll
    for (int t2 = 0; t2 < TR; ++t2) {
      const int64_t tg = rb * (2 * TR) + wr * TR + t2;  // tile of ROWS LUT rows
      if (tg >= ntile) break;                           // (wave-uniform)
#pragma unroll
      for (int b2 = 0; b2 < TB; ++b2) {
        T mn = run[t2][b2][0];
#pragma unroll
        for (int i = 1; i < NACC; ++i) mn = __builtin_fmin(mn, run[t2][b2][i]);
        if (mn != mn) mn = (T)INFINITY;
        if (!COLLECT) {
          sec[b2] = __builtin_fmin(sec[b2], __builtin_fmax(best[b2], mn));   // a tie with the best becomes `sec`
          best[b2] = __builtin_fmin(best[b2], mn);
        } else {
#pragma unroll
          for (int off = ROWS; off < 64; off <<= 1) mn = __builtin_fmin(mn, __shfl_xor(mn, off, 64));   // all rows of the tile
          if (grp == 0 && mn <= th[b2]) {
            const int64_t m = m0 + (wc * TB + b2) * ROWS + col;
            const int pos = atomicAdd(&cand_n[m], 1);
            if (pos < cap) cand[m * cap + pos] = (int)tg;
          }
        }
      }
    }
  }
  if (!COLLECT) {
#pragma unroll
    for (int b2 = 0; b2 < TB; ++b2) {
      const int64_t m = m0 + (wc * TB + b2) * ROWS + col;
      if (m < M) {
        const int64_t o = (((int64_t)slice * 2 + wr) * G + grp) * M + m;
        part_cost[o] = best[b2];
        part_sec[o] = sec[b2];
      }
    }
  }
}

// one wave per observation of the chunk: thr = U + cut + Delta(cut) (ce, cf with the 1 % slack), resets the candidate count.
// cut = 0.0 is the top-k rule above, operation for operation (x + 0.0 == x for every x >= 0 and every NaN); cut > 0 is the
// radius rule of spart_lut_bayes ("likelihood-weighted posterior" below, which derives it); cut = +inf gives thr = +inf
template <typename T>
__global__ __launch_bounds__(256) void k_lutow_bound(const T* __restrict__ part_cost, const T* __restrict__ part_sec,
                                                     const double* __restrict__ yn, int nb, int64_t M, int npart, int k, double ce,
                                                     double cf, double cut, T* __restrict__ thr, int* __restrict__ cand_n) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                                  // (whole wave)
  const T U = lut_topk_kth<T>(part_cost, part_sec, m, M, npart, k, lane);
  if (lane == 0) {
    const double Y = yn[2 * m], nq = yn[2 * m + 1];
    const double big = sizeof(T) == 4 ? 3.4028234663852886e38 : 1.7976931348623157e308;
    const double u = (double)LutNum<T>::u, f = (nb + 3.0) * u, grow = 1.01 * (1.0 + f) / (1.0 - f);
    double N = nq, C = 0.0;
    for (int it = 0; it < 3; ++it) {                   // C(N_0), N_1, C(N_1), N_2, C(N_2); C carries + cut
      C = (double)U + Y + ce * (N + Y);
      C = (C > 0.0 ? C : 0.0) + cut;
      if (it == 2) break;
      const double s = __builtin_sqrt(Y) + __builtin_sqrt(C * grow + 4.04 * u * (N + Y));
      const double ns = 1.01 * s * s;
      N = ns < N ? ns : N;
    }
    double t = (double)U + ((2.0 * ce * (N + Y) + cf * C) + cut);
    t = t + (4.0 * (double)LutNum<T>::u * __builtin_fabs(t) + (double)LutNum<T>::tiny);
    if (!(4.0 * (nq + Y) < big)) t = __builtin_nan("");   // (NaN Y: an observation the filter must not decide)
    T tt = (T)t;                                       // (NaN / inf stay non-finite: the select flags m)
    if constexpr (sizeof(T) == 4) {
      if ((double)tt < t) {                            // round up: the next float above
        const unsigned b = __float_as_uint(tt);
        tt = tt > 0.0f ? __uint_as_float(b + 1u) : (tt == 0.0f ? __uint_as_float(1u) : __uint_as_float(b - 1u));
      }
    }
    thr[m] = tt;
    cand_n[m] = 0;
  }
}

// ---- parameter summaries (spart_lut_summarise): count, mean, median and standard deviation of the parameter rows a
// search selected, per observation and parameter, as include/spart_hip.h defines them (float64, place order, no FMA).
//
// Mapping.  Single-wave workgroups; lane = (observation g of the wave, parameter p) with G observations side by side:
// G = 64 / P for k <= LUT_SUM_SMALL_K (two at P = 27, one above 32 parameters), G = 1 above it.  A = G P lanes work, and
// lane l of work item t writes the output elements t A + l: the stores of a wave are one contiguous run.
//   gather   place j of observation m is ONE row of P doubles read by the P lanes of its group (216 B at P = 27); the index
//            idx[m, j] is read by every lane of the group (one address: a broadcast) and range-checked by the lane that uses
//            it, as an unsigned compare against B, before it becomes part of an address; four places are in flight per lane.
//   LDS      the accepted values x_1 .. x_n of a lane sit at [i][l], row stride A doubles: a lane only ever touches its own
//            column, so the wave needs no barrier, and the A consecutive doubles of a row are conflict-free (ds_read_b64:
//            two groups of 32 lanes over 64 banks).  k (rounded up to a multiple of 4) x A x 8 bytes of dynamic LDS: 5.2 KB at
//            k = 10, P = 27; at most
//            LUT_SUM_SMALL_LDS_BYTES = 32 KB for k <= 64, so the common case is never sized by k = 256 (where it is k P 8
//            bytes, 128 KB at P = 64: one wave per CU, a case that is recorded, not tuned).
//   mean     the running sum of the gather; std re-reads the column.
//   median   by rank, not by sorting: in the order (value, place) x_i has rank #{j < i: x_j <= x_i} + #{j > i: x_j < x_i}, and
//            the value of rank r is s[r].  n^2 compares per lane with no data-dependent branch; four x_i are held in
//            registers per sweep over the column, which is read four places at a time.
constexpr int LUT_SUM_MAXP = 64;
constexpr int LUT_SUM_SMALL_K = 64;
constexpr int LUT_SUM_SMALL_LDS_BYTES = 32768;       // the most dynamic LDS a launch with k <= LUT_SUM_SMALL_K asks for
constexpr int LUT_SUM_MAX_BLOCKS = 1 << 16;
static_assert(LUT_SUM_SMALL_K * 64 * 8 == LUT_SUM_SMALL_LDS_BYTES, "k <= LUT_SUM_SMALL_K: at most 64 working lanes x k doubles");

// observations per wave and dynamic LDS bytes of a launch
inline int lut_sum_group(int P, int k) { return k <= LUT_SUM_SMALL_K ? 64 / P : 1; }
inline size_t lut_sum_lds_bytes(int P, int k) { return (size_t)((k + 3) & ~3) * (size_t)(lut_sum_group(P, k) * P) * 8; }

__global__ __launch_bounds__(64) void k_lut_summarise(const double* __restrict__ params, int64_t B, int P,
                                                      const int64_t* __restrict__ idx, int64_t M, int k, int G,
                                                      double* __restrict__ mean, double* __restrict__ median,
                                                      double* __restrict__ sdev, int32_t* __restrict__ count) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char lut_sum_smem[];
  double* xs = reinterpret_cast<double*>(lut_sum_smem);
  const int lane = threadIdx.x;
  const int A = G * P;
  const int g = lane / P, p = lane - g * P;
  const int64_t items = (M + G - 1) / G;
  const double qnan = __builtin_nan("");
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t m = item * G + g;
    if (lane >= A || m >= M) continue;                 // (no barrier below: a lane works on its own LDS column only)
    const int64_t* row = idx + m * k;
    double* x = xs + lane;
    int n = 0;
    double sum = 0.0;
    bool has_nan = false;
    for (int j0 = 0; j0 < k; j0 += 4) {
      int64_t r[4];
      double v[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = j0 + u < k ? row[j0 + u] : (int64_t)-1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        // THE range check: 0 <= r < B as one unsigned compare.  Nothing below forms an address from r[u] itself: a refused
        // index is replaced by row 0 (B > 0 here) and its load is skipped as well
        ok[u] = (unsigned long long)r[u] < (unsigned long long)B;
        const int64_t rr = ok[u] ? r[u] : (int64_t)0;
        v[u] = ok[u] ? params[rr * P + p] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!ok[u]) continue;
        x[n * A] = v[u];
        sum = n == 0 ? v[u] : sum + v[u];
        has_nan = has_nan || v[u] != v[u];
        ++n;
      }
    }
    const int64_t o = m * P + p;
    if (count && p == 0) count[m] = n;
    if (n == 0) {
      if (mean) mean[o] = qnan;
      if (median) median[o] = qnan;
      if (sdev) sdev[o] = qnan;
      continue;
    }
    const double mu = sum / (double)n;
    if (mean) mean[o] = mu;
    if (sdev) {
      double s2 = 0.0;
      for (int i = 0; i < n; ++i) {
        const double d = x[i * A] - mu;
        const double q = d * d;
        s2 = i == 0 ? q : s2 + q;
      }
      sdev[o] = __builtin_sqrt(s2 / (double)n);
    }
    if (median) {
      double med = qnan;
      if (!has_nan) {
        // rank of x_i in the order (value, place): #{j < i: x_j <= x_i} + #{j > i: x_j < x_i}, one compare per pair; the
        // ranks are a permutation of 0 .. n-1, and the value of rank r is s[r].  Four x_i per sweep, four x_j per step;
        // the column is padded to a multiple of four with +inf, which lies behind every x_i and is never "<" anything
        const int npad = (n + 3) & ~3;
        for (int i = n; i < npad; ++i) x[i * A] = __builtin_inf();
        const int r1 = (n - 1) >> 1, r2 = n >> 1;
        double s1 = 0.0, s2 = 0.0;
        for (int i0 = 0; i0 < n; i0 += 4) {
          double xi[4];
          int rank[4] = {0, 0, 0, 0};
#pragma unroll
          for (int u = 0; u < 4; ++u) xi[u] = x[(i0 + u) * A];
          for (int j0 = 0; j0 < i0; j0 += 4) {
            double xj[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) xj[v] = x[(j0 + v) * A];
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
              for (int u = 0; u < 4; ++u) rank[u] += xj[v] <= xi[u] ? 1 : 0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
              if (v != u) rank[u] += (v < u ? xi[v] <= xi[u] : xi[v] < xi[u]) ? 1 : 0;
          for (int j0 = i0 + 4; j0 < npad; j0 += 4) {
            double xj[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) xj[v] = x[(j0 + v) * A];
#pragma unroll
            for (int v = 0; v < 4; ++v)
#pragma unroll
              for (int u = 0; u < 4; ++u) rank[u] += xj[v] < xi[u] ? 1 : 0;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (i0 + u < n && rank[u] == r1) s1 = xi[u];
            if (i0 + u < n && rank[u] == r2) s2 = xi[u];
          }
        }
        med = r1 == r2 ? s1 : (s1 + s2) / 2.0;
      }
      median[o] = med;
    }
  }
}

// ---- likelihood-weighted posterior (spart_lut_bayes): for observation m, over E = the accepted rows with a finite c_T(b, m)
// (cost, row rule and observation rule of the per-observation-weights search above), c* = min c_T, e_b = (double)c_T(b) -
// (double)c*, S = {b in E: e_b <= cut} in ascending row order, omega_b = exp(-(e_b / (2 tau))): count = |S|, sum_w, ess and the
// omega-weighted mean and spread of the parameter rows, as include/spart_hip.h defines them (float64, ascending rows, no FMA).
//
// A radius query is the per-observation-weights pipeline with another threshold and another consumer:
//   1-4.  k_lut_centre, k_lutw_norm (w = NULL), k_lutow_q, k_lutow_obs, k_lutow_gemm<false>: unchanged
//   5.    k_lutow_bound with k = 1 and cut: U = the smallest partial value, thr = U + cut + Delta(cut) (below)
//   6.    k_lutow_gemm<true>: the candidate tiles under thr, capacity lut_topk_cap(LUT_BAYES_CAPK) tiles per observation
//   7.    k_lut_bayes<., ., false>: one wave per observation over the rows of its candidate tiles
//   8.    k_lut_bayes<., ., true>: the same passes over EVERY row for the flagged observations
//
// The threshold.  a^1 is the row behind U, so a~(a^1) = U, and with (i)-(v) of the per-observation weights
//     c* <= c_T(a^1) <= c(a^1) + F_a1 <= U + Y + E_a1 + F_a1.
// b in S means fl64(c_T(b) - c*) <= cut.  The float64 subtraction of two values of T rounds once and rounding is monotone, so
// c_T(b) - c* <= cut' = cut (1 + 2^-50) (what the host hands to k_lutow_bound as `cut`; 0 stays 0, +inf stays +inf).  Then
//     a~(b) <= c(b) - Y + E_b <= c_T(b) + F_b - Y + E_b <= c* + cut' + F_b - Y + E_b <= U + cut' + (E_a1 + E_b) + (F_a1 + F_b).
// The F terms: c(a^1) <= C(N) = max(U + Y + ce (N + Y), 0) as before, and c(b) <= c_T(b) / (1 - f) <= (c_T(a^1) + cut') / (1 - f)
// <= (C(N) + cut') (1 + f) / (1 - f), f = (nb + 3) u; so F_a1 + F_b <= 2.01 f (C(N) + cut').  The N iteration bounds N_a1 and N_b
// through sqrt(N_b) <= sqrt(Y) + sqrt(c'(b)) with c'(b) <= c(b) + 4 u (N + Y): the same step with C(N) + cut' in place of C(N)
// (it bounds c(a^1) as well, cut' >= 0).  So
//     thr = U + cut' + 2 ce (N_2 + Y) + cf (C(N_2) + cut'),
// k_lutow_bound's expression with C + cut' for C, evaluated in float64 and rounded up to T.  cut = +inf gives thr = +inf, a
// finite cut whose thr overflows T likewise: such observations are flagged for the brute force, as a non-finite threshold
// always is.  If the rows of the candidate tiles hold no finite cost (the rows behind U overflowed in the direct evaluation) the
// observation is flagged too.
//
// k_lut_bayes.  Single-wave workgroups; dynamic LDS = LUT_BAYES_SORT tile numbers, the observation and its weight row.
//   sort    the collect pass appends candidate tiles in atomic order; a bitonic sort of the tile numbers (padded with INT_MAX to
//           a power of two) makes the row order, and with it every sum, reproducible.  A tile is appended at most once.
//   pass A  lanes over rows (64 per round, ascending with the lane): exact c_T, the wave minimum and its lowest row
//   pass B  the same rows again; a ballot of e <= cut gives the included rows of the round, which are then taken one at a time
//           in row order: omega and the row number come from the owning lane by a shuffle, lane p < P reads params[r P + p]
//           (one coalesced row of P doubles) and adds omega, omega^2 and omega x to its own running sums
//   pass C  the same for (omega d) d with d = x - mean
//   The costs are recomputed in every pass (deterministic: one lane, one sequential loop), not cached: the candidate rows of
//   one observation can be 34 816 values.  Traffic per pass and observation: rows x nb values of the LUT (a lane reads one row,
//   as in k_lutw_select), and in passes B and C count x P doubles of the parameter table.
//   Every row number is range-checked (0 <= r < B) and norm-checked before an address is formed from it.
constexpr int LUT_BAYES_CAPK = LUT_TOPK_MAXK;         // the candidate capacity is that of a k = 256 search: 1088 tiles
constexpr int LUT_BAYES_SORT = 2048;                  // tile numbers sorted in LDS: the power of two above the capacity
constexpr int LUT_BAYES_MAXP = LUT_SUM_MAXP;
static_assert(LUT_BAYES_SORT >= 4 * LUT_BAYES_CAPK + 64 && (LUT_BAYES_SORT & (LUT_BAYES_SORT - 1)) == 0,
              "k_lut_bayes sorts a whole candidate list, padded to a power of two");
static_assert(LUT_BAYES_MAXP <= 64, "k_lut_bayes: lane = parameter");

struct LutBayesOut {                                  // spart_lut_bayes_out
  double *mean, *sdev, *sum_w, *ess;
  int64_t *count, *best_idx;
  void* best_cost;
};

inline size_t lut_bayes_lds_bytes(int nb, size_t es) { return (size_t)LUT_BAYES_SORT * 4 + 2 * (size_t)nb * es; }

// the outputs of an observation with an empty E, written by the whole wave
template <typename T>
__device__ __forceinline__ void lut_bayes_empty(const LutBayesOut& out, int64_t m, int P, int lane) {
  const double qnan = __builtin_nan("");
  if (lane < P) {
    if (out.mean) out.mean[m * P + lane] = qnan;
    if (out.sdev) out.sdev[m * P + lane] = qnan;
  }
  if (lane == 0) {
    if (out.sum_w) out.sum_w[m] = 0.0;
    if (out.ess) out.ess[m] = qnan;
    if (out.count) out.count[m] = 0;
    if (out.best_idx) out.best_idx[m] = -1;
    if (out.best_cost) static_cast<T*>(out.best_cost)[m] = (T)INFINITY;
  }
}

// B = 0: every observation is empty
template <typename T>
__global__ __launch_bounds__(64) void k_lut_bayes_empty(int64_t M, int P, LutBayesOut out) {
  for (int64_t m = blockIdx.x; m < M; m += gridDim.x) lut_bayes_empty<T>(out, m, P, threadIdx.x);
}

// c_T(b, m) of the per-observation weights, operation for operation (k_lutw_select<., ., ., true>)
template <typename T>
__device__ __forceinline__ T lut_bayes_cost(const T* __restrict__ x, const T* ys, const T* wsm, int nb) {
  SPART_NO_CONTRACT
  T c = T(0);
  for (int j = 0; j < nb; ++j) {
    const T wj = wsm[j];
    if (wj == T(0)) continue;                          // the mask: no operation at all
    const T d = x[j] - ys[j];
    c = c + (wj * d) * d;
  }
  return c;
}

template <typename T, int ROWS, bool BRUTE>
__global__ __launch_bounds__(64) void k_lut_bayes(const T* __restrict__ lut, const T* __restrict__ obs, const T* __restrict__ w,
                                                  const T* __restrict__ norm, const double* __restrict__ params, int nb, int64_t B,
                                                  int P, int64_t m_off, int64_t Mc, double cut, double two_tau, int force,
                                                  const T* __restrict__ thr, const int* __restrict__ cand_n,
                                                  const int* __restrict__ cand, int cap, unsigned long long* __restrict__ ctl,
                                                  int* __restrict__ flag_list, LutBayesOut out) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char lutb_smem[];
  int* tiles = reinterpret_cast<int*>(lutb_smem);
  T* ys = reinterpret_cast<T*>(tiles + LUT_BAYES_SORT);
  T* wsm = ys + nb;
  const int lane = threadIdx.x & 63;
  const unsigned count = BRUTE ? (unsigned)ctl[1] : 0u;
  const int64_t nwork = BRUTE ? (int64_t)count : Mc;
  const int64_t stride_w = BRUTE ? (int64_t)gridDim.x : nwork;
  for (int64_t item = blockIdx.x; item < nwork; item += stride_w) {
    const int64_t m = BRUTE ? (int64_t)flag_list[item] : m_off + item;
    lut_wave_sync();                                   // (the previous item's reads of ys / tiles are done)
    bool fin = true;
    for (int j = lane; j < nb; j += 64) {
      const T v = obs[m * nb + j], wj = w[m * nb + j];
      ys[j] = v;
      wsm[j] = wj;
      fin = fin && wj >= T(0) && LutNum<T>::finite(wj) && (wj == T(0) || LutNum<T>::finite(v));
    }
    lut_wave_sync();
    if (__all(fin) == 0) {                             // an invalid observation matches no row
      lut_bayes_empty<T>(out, m, P, lane);
      continue;
    }
    auto to_brute = [&] {
      if (lane == 0) {
        const unsigned long long pos = atomicAdd(&ctl[1], 1ull);
        flag_list[pos] = (int)m;
      }
    };
    int64_t nrows = B;
    int ncand = 0;
    if (!BRUTE) {
      bool flag = force != 0;
      if (!flag) {
        ncand = cand_n[item];
        flag = !LutNum<T>::finite(thr[item]) || ncand > cap;
        if (lane == 0) {
          atomicAdd(&ctl[2], (unsigned long long)ncand);
          atomicMax(&ctl[3], (unsigned long long)ncand);
        }
      }
      if (flag) {
        to_brute();
        continue;
      }
      // the candidate tiles in ascending order (bitonic, n2 = the power of two >= ncand, padded with INT_MAX)
      int n2 = 2;
      while (n2 < ncand) n2 <<= 1;
      for (int i = lane; i < n2; i += 64) tiles[i] = i < ncand ? cand[item * cap + i] : 0x7fffffff;
      lut_wave_sync();
      for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          for (int i = lane; i < n2 / 2; i += 64) {
            const int t = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
            const int p = t | stride;
            const int vt = tiles[t], vp = tiles[p];
            if ((vp < vt) == ((t & size) == 0)) {
              tiles[t] = vp;
              tiles[p] = vt;
            }
          }
          lut_wave_sync();
        }
      nrows = (int64_t)ncand * ROWS;
    }
    // this lane's row of the round that starts at r0, or -1: range- and norm-checked, ascending with the lane
    auto row_of = [&](int64_t r0) -> int {
      int64_t r = -1;
      if (BRUTE) {
        r = r0 + lane;
      } else {
        const int ci = (int)(r0 / ROWS) + lane / ROWS;
        if (ci < ncand) {
          const int tl = tiles[ci];
          if (tl >= 0) r = (int64_t)tl * ROWS + lane % ROWS;
        }
      }
      if (r < 0 || r >= B) return -1;
      return LutNum<T>::finite(norm[r]) ? (int)r : -1;
    };
    // pass A: c* and its lowest row
    T bc = (T)INFINITY;
    int br = -1;
    for (int64_t r0 = 0; r0 < nrows; r0 += 64) {
      const int r = row_of(r0);
      if (r >= 0) {
        const T c = lut_bayes_cost<T>(lut + (int64_t)r * nb, ys, wsm, nb);
        if (LutNum<T>::finite(c) && c < bc) {          // (a lane's rows ascend: the first of equal costs stays)
          bc = c;
          br = r;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const T oc = __shfl_xor(bc, off, 64);
      const int orow = __shfl_xor(br, off, 64);
      if (orow >= 0 && (br < 0 || oc < bc || (oc == bc && orow < br))) {
        bc = oc;
        br = orow;
      }
    }
    if (br < 0) {                                      // E is empty among these rows
      if (BRUTE) lut_bayes_empty<T>(out, m, P, lane);
      else to_brute();
      continue;
    }
    const double cstar = (double)bc;
    // passes B and C.  second = false: sum_w, s2 and the sums of omega x; second = true: the sums of (omega d) d
    double sw = 0.0, s2 = 0.0, sx = 0.0, sv = 0.0, mu = 0.0;
    int64_t n = 0;
    for (int second = 0; second < 2; ++second) {
      for (int64_t r0 = 0; r0 < nrows; r0 += 64) {
        const int r = row_of(r0);
        bool inc = false;
        double om = 0.0;
        if (r >= 0) {
          const T c = lut_bayes_cost<T>(lut + (int64_t)r * nb, ys, wsm, nb);
          if (LutNum<T>::finite(c)) {
            const double e = (double)c - cstar;
            if (e <= cut) {
              inc = true;
              om = Mx<double>::exp_poly(-(e / two_tau));
            }
          }
        }
        unsigned long long mask = __ballot(inc);
        if (!second) n += __builtin_popcountll(mask);
        while (mask) {
          const int src = __builtin_ctzll(mask);
          mask &= mask - 1;
          const int rr = __shfl(r, src, 64);
          const double o = __shfl(om, src, 64);
          const double x = lane < P ? params[(int64_t)rr * P + lane] : 0.0;
          if (!second) {
            sw = sw + o;
            s2 = s2 + o * o;
            sx = sx + o * x;
          } else {
            const double d = x - mu;
            sv = sv + (o * d) * d;
          }
        }
      }
      if (!second) mu = sx / sw;
      if (!out.sdev) break;
    }
    if (lane < P) {
      if (out.mean) out.mean[m * P + lane] = mu;
      if (out.sdev) out.sdev[m * P + lane] = __builtin_sqrt(sv / sw);
    }
    if (lane == 0) {
      if (out.sum_w) out.sum_w[m] = sw;
      if (out.ess) out.ess[m] = (sw * sw) / s2;
      if (out.count) out.count[m] = n;
      if (out.best_idx) out.best_idx[m] = (int64_t)br;
      if (out.best_cost) static_cast<T*>(out.best_cost)[m] = bc;
    }
  }
}

// ---- weighted quantiles of the posterior (spart_lut_bayes_quantiles): for observation m, parameter p and level q_i the
// smallest value v among {x_b = params[b, p] : b in S} with F_p(v) >= q_i * sum_w, where F_p(v) is the ordered float64 sum of
// omega_b over the rows of S with x_b <= v (include/spart_hip.h defines it; E, c*, S, omega and sum_w are k_lut_bayes').
//
// k_lut_posterior_quant is a SECOND consumer of the same candidate lists, queued right after k_lut_bayes for the same chunk (the
// lists stay in the workspace until the next chunk's collect pass) and once more after the last chunk over the flag list.  It
// reaches k_lut_bayes' decisions by the same reads and writes nothing but quant: a forced, overflowing or non-finite-threshold
// observation, and one without a finite cost among its candidates, is skipped by the filter instance (k_lut_bayes flagged it)
// and picked up by the brute instance from flag_list; ctl and flag_list are read only.
//   sort, row_of, pass A   k_lut_bayes', line for line: the same rows in the same order, the same c*
//   pass 0   pass B's loop (ballot of e <= cut, the included rows one at a time in row order, lane p reads params[r P + p]):
//            sum_w by the same additions (the same bits), per lane the minimum and maximum of x, a NaN flag and the first zero
//            of the column (the sign a zero answer takes).  While they fit, (row, omega) of the included rows go to the part of
//            the LDS tile buffer the sorted list does not use (all of it in the brute instance): later passes then read the
//            members back instead of evaluating every row's cost again.  A set that does not fit is never truncated: its passes
//            recompute, as k_lut_bayes' do; omega is a pure function of the row, so the bits are the same either way.
//   search   per lane and level an interval [lo, hi] of DATA values that holds the answer, on the order-preserving unsigned
//            64-bit image of the doubles (-0.0 and +0.0 share one image).  A pass takes pivot = lo + (hi - lo) / 2 for every
//            level of every lane at once and gives F(pivot), the largest x <= pivot and the smallest x > pivot; F(pivot) >=
//            target moves hi to the former, otherwise lo to the latter.  hi - lo at least halves per pass, so 64 passes bound
//            the loop for any data; the snap to data values ends it after about log2(count) passes on spread-out columns.
//            F is non-decreasing in v (an ordered sum of non-negative terms over a larger subset is never smaller), so the
//            bisection finds THE smallest qualifying value; F(max) is sum_w by the same additions, so hi = max qualifies.
//   The loop runs while any (lane, level) is open (__any: wave-uniform); LUT_BAYES_QG levels are searched together, a call
//   with more takes the search again for the next group.
constexpr int LUT_BAYES_MAXQ = 8;                     // levels per call
constexpr int LUT_BAYES_QG = 4;                       // levels searched together (registers: 7 doubles per level and lane)

struct LutBayesLevels {                               // spart_lut_bayes_q_opt.levels, by value
  double q[LUT_BAYES_MAXQ];
  int nq;
};

// the order-preserving image of a non-NaN double (both zeros -> the image of +0.0) and its inverse
__device__ __forceinline__ unsigned long long lut_bayes_key(double x) {
  unsigned long long b = (unsigned long long)__double_as_longlong(x);
  if ((b << 1) == 0ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double lut_bayes_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// B = 0: every quantile is NaN
__global__ __launch_bounds__(256) void k_lut_posterior_quant_empty(int64_t n, double* __restrict__ quant) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) quant[i] = __builtin_nan("");
}

template <typename T, int ROWS, bool BRUTE>
__global__ __launch_bounds__(64) void k_lut_posterior_quant(const T* __restrict__ lut, const T* __restrict__ obs,
                                                        const T* __restrict__ w, const T* __restrict__ norm,
                                                        const double* __restrict__ params, int nb, int64_t B, int P, int64_t m_off,
                                                        int64_t Mc, double cut, double two_tau, int force,
                                                        const T* __restrict__ thr, const int* __restrict__ cand_n,
                                                        const int* __restrict__ cand, int cap,
                                                        const unsigned long long* __restrict__ ctl,
                                                        const int* __restrict__ flag_list, LutBayesLevels lv,
                                                        double* __restrict__ quant) {
  SPART_NO_CONTRACT
  extern __shared__ __attribute__((aligned(16))) char lutq_smem[];
  int* tiles = reinterpret_cast<int*>(lutq_smem);
  T* ys = reinterpret_cast<T*>(tiles + LUT_BAYES_SORT);
  T* wsm = ys + nb;
  const int lane = threadIdx.x & 63;
  const int nq = lv.nq;
  const double qnan = __builtin_nan("");
  const unsigned count = BRUTE ? (unsigned)ctl[1] : 0u;
  const int64_t nwork = BRUTE ? (int64_t)count : Mc;
  const int64_t stride_w = BRUTE ? (int64_t)gridDim.x : nwork;
  for (int64_t item = blockIdx.x; item < nwork; item += stride_w) {
    const int64_t m = BRUTE ? (int64_t)flag_list[item] : m_off + item;
    auto all_nan = [&] {
      if (lane < P)
        for (int i = 0; i < nq; ++i) quant[(m * P + lane) * nq + i] = qnan;
    };
    lut_wave_sync();                                   // (the previous item's reads of ys / tiles are done)
    bool fin = true;
    for (int j = lane; j < nb; j += 64) {
      const T v = obs[m * nb + j], wj = w[m * nb + j];
      ys[j] = v;
      wsm[j] = wj;
      fin = fin && wj >= T(0) && LutNum<T>::finite(wj) && (wj == T(0) || LutNum<T>::finite(v));
    }
    lut_wave_sync();
    if (__all(fin) == 0) {                             // an invalid observation matches no row
      all_nan();
      continue;
    }
    int64_t nrows = B;
    int ncand = 0;
    if (!BRUTE) {
      if (force != 0) continue;                        // (k_lut_bayes flagged it: the brute instance's)
      ncand = cand_n[item];
      if (!LutNum<T>::finite(thr[item]) || ncand > cap) continue;
      // the candidate tiles in ascending order (bitonic, n2 = the power of two >= ncand, padded with INT_MAX)
      int n2 = 2;
      while (n2 < ncand) n2 <<= 1;
      for (int i = lane; i < n2; i += 64) tiles[i] = i < ncand ? cand[item * cap + i] : 0x7fffffff;
      lut_wave_sync();
      for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          for (int i = lane; i < n2 / 2; i += 64) {
            const int t = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
            const int p = t | stride;
            const int vt = tiles[t], vp = tiles[p];
            if ((vp < vt) == ((t & size) == 0)) {
              tiles[t] = vp;
              tiles[p] = vt;
            }
          }
          lut_wave_sync();
        }
      nrows = (int64_t)ncand * ROWS;
    }
    // this lane's row of the round that starts at r0, or -1: range- and norm-checked, ascending with the lane
    auto row_of = [&](int64_t r0) -> int {
      int64_t r = -1;
      if (BRUTE) {
        r = r0 + lane;
      } else {
        const int ci = (int)(r0 / ROWS) + lane / ROWS;
        if (ci < ncand) {
          const int tl = tiles[ci];
          if (tl >= 0) r = (int64_t)tl * ROWS + lane % ROWS;
        }
      }
      if (r < 0 || r >= B) return -1;
      return LutNum<T>::finite(norm[r]) ? (int)r : -1;
    };
    // pass A: c* (its row only says whether E is empty here)
    T bc = (T)INFINITY;
    int br = -1;
    for (int64_t r0 = 0; r0 < nrows; r0 += 64) {
      const int r = row_of(r0);
      if (r >= 0) {
        const T c = lut_bayes_cost<T>(lut + (int64_t)r * nb, ys, wsm, nb);
        if (LutNum<T>::finite(c) && c < bc) {
          bc = c;
          br = r;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const T oc = __shfl_xor(bc, off, 64);
      const int orow = __shfl_xor(br, off, 64);
      if (orow >= 0 && (br < 0 || oc < bc || (oc == bc && orow < br))) {
        bc = oc;
        br = orow;
      }
    }
    if (br < 0) {                                      // E is empty among these rows
      if (BRUTE) all_nan();                            // (filter instance: flagged by k_lut_bayes, the brute instance's)
      continue;
    }
    const double cstar = (double)bc;
    // the (row, omega) cache: the 8-byte-aligned rest of the tile buffer behind the ncand sorted tile numbers
    const int c_off = BRUTE ? 0 : (ncand + 1) & ~1;    // in ints
    const int c_cap = (LUT_BAYES_SORT - c_off) / 3;    // 12 bytes per member
    double* c_om = reinterpret_cast<double*>(tiles + c_off);
    int* c_row = tiles + c_off + 2 * c_cap;
    // one pass over S in row order without the cache: feed(row, omega) is called by the whole wave, member by member
    auto recompute = [&](auto&& feed) {
      for (int64_t r0 = 0; r0 < nrows; r0 += 64) {
        const int r = row_of(r0);
        bool inc = false;
        double om = 0.0;
        if (r >= 0) {
          const T c = lut_bayes_cost<T>(lut + (int64_t)r * nb, ys, wsm, nb);
          if (LutNum<T>::finite(c)) {
            const double e = (double)c - cstar;
            if (e <= cut) {
              inc = true;
              om = Mx<double>::exp_poly(-(e / two_tau));
            }
          }
        }
        unsigned long long mask = __ballot(inc);
        while (mask) {
          const int src = __builtin_ctzll(mask);
          mask &= mask - 1;
          feed(__shfl(r, src, 64), __shfl(om, src, 64));
        }
      }
    };
    // pass 0: sum_w, the range of every column, its NaN flag and first zero; fills the cache while the members fit
    double sw = 0.0, zfirst = 0.0;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    bool has_nan = false, zseen = false;
    int n = 0;
    recompute([&](int rr, double o) {
      const double x = lane < P ? params[(int64_t)rr * P + lane] : 0.0;
      if (n < c_cap && lane == 0) {
        c_om[n] = o;
        c_row[n] = rr;
      }
      ++n;
      sw = sw + o;
      has_nan = has_nan || x != x;
      if (x == 0.0 && !zseen) {
        zseen = true;
        zfirst = x;
      }
      const unsigned long long kx = lut_bayes_key(x);
      kmin = kx < kmin ? kx : kmin;
      kmax = kx > kmax ? kx : kmax;
    });
    const bool cached = n <= c_cap;
    lut_wave_sync();                                   // (lane 0's cache entries are visible to the wave)
    for (int g0 = 0; g0 < nq; g0 += LUT_BAYES_QG) {
      unsigned long long lo[LUT_BAYES_QG], hi[LUT_BAYES_QG];
      double tg[LUT_BAYES_QG];
#pragma unroll
      for (int u = 0; u < LUT_BAYES_QG; ++u) {
        const bool live = g0 + u < nq && lane < P && !has_nan;
        tg[u] = lv.q[g0 + u < nq ? g0 + u : g0] * sw;
        lo[u] = kmin;
        hi[u] = live ? kmax : kmin;
      }
      for (int it = 0; it < 64; ++it) {                // (hi - lo at least halves per pass: never more than 64)
        bool open = false;
#pragma unroll
        for (int u = 0; u < LUT_BAYES_QG; ++u) open = open || lo[u] < hi[u];
        if (__any(open) == 0) break;
        unsigned long long piv[LUT_BAYES_QG], bel[LUT_BAYES_QG], abv[LUT_BAYES_QG];
        double F[LUT_BAYES_QG];
#pragma unroll
        for (int u = 0; u < LUT_BAYES_QG; ++u) {
          piv[u] = lo[u] + ((hi[u] - lo[u]) >> 1);
          bel[u] = lo[u];
          abv[u] = hi[u];
          F[u] = 0.0;
        }
        auto feed = [&](double x, double o) {
          const unsigned long long kx = lut_bayes_key(x);
#pragma unroll
          for (int u = 0; u < LUT_BAYES_QG; ++u) {
            const bool le = kx <= piv[u];
            F[u] = F[u] + (le ? o : 0.0);              // (a row that does not qualify adds +0.0: no change to F >= 0)
            bel[u] = le && kx > bel[u] ? kx : bel[u];
            abv[u] = !le && kx < abv[u] ? kx : abv[u];
          }
        };
        if (cached) {
          for (int j0 = 0; j0 < n; j0 += 4) {          // four parameter rows in flight
            double xs[4], os[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int j = j0 + v < n ? j0 + v : j0;
              os[v] = c_om[j];
              xs[v] = lane < P ? params[(int64_t)c_row[j] * P + lane] : 0.0;
            }
#pragma unroll
            for (int v = 0; v < 4; ++v)
              if (j0 + v < n) feed(xs[v], os[v]);
          }
        } else {
          recompute([&](int rr, double o) { feed(lane < P ? params[(int64_t)rr * P + lane] : 0.0, o); });
        }
#pragma unroll
        for (int u = 0; u < LUT_BAYES_QG; ++u)
          if (lo[u] < hi[u]) {
            if (F[u] >= tg[u]) hi[u] = bel[u];
            else lo[u] = abv[u];
          }
      }
#pragma unroll
      for (int u = 0; u < LUT_BAYES_QG; ++u)
        if (g0 + u < nq && lane < P) {
          double v = lut_bayes_unkey(hi[u]);
          if (v == 0.0) v = zfirst;                    // (of values that compare equal, the one in the lowest row)
          quant[(m * P + lane) * nq + g0 + u] = has_nan ? qnan : v;
        }
    }
  }
}

}  // namespace spart
