// The device pieces of the RVEA family's selection that rvea_select.hip (one problem, a grid of workgroups, b̂ in a
// global scratch) and rvea_small.hip (a workgroup per run, b̂ in LDS) share, so that the two cannot drift: the contract
// in the docstring of evoxmi/ops/rvea.py is written once, here.  Every operation is float64 in the order stated there;
// both files are compiled with -ffp-contract=off, so nothing in here fuses.  Everything is forced inline.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

namespace evx {

constexpr int RV_NO_ROW = INT_MAX;

// the bits of a double as an unsigned word whose order is the order of the values; a non-finite value ranks as +inf
__device__ __forceinline__ unsigned long long rv_ordered(double x) {
  if (!(fabs(x) <= 1.7976931348623157e308)) x = INFINITY;
  x = x + 0.0;  // −0 → +0
  unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// |b| = sqrt(((b_0² + b_1²) + b_2²) + …) of a row of B; b̂_t is then (double)b_t / |b|
__device__ __forceinline__ double rv_vector_norm(const float* __restrict__ b, int m) {
  double s = 0.0;
  for (int t = 0; t < m; ++t) {
    const double x = (double)b[t];
    s = t == 0 ? x * x : s + x * x;
  }
  return sqrt(s);
}

// a row of A into registers: a = (double)A_i − shift, raised to the floor (a NaN stays), then â = a / |a|.  Returns |a|;
// nan_row says whether the float32 row holds a NaN.  The entries from m on are 0
template <int MC>
__device__ __forceinline__ double rv_load_row(const float* __restrict__ row, const float* __restrict__ shift, int has_floor, double floor_v,
                                              int m, double (&a)[MC], bool& nan_row) {
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < MC; ++t)
    if (t < m) {
      const float x = row[t];
      nan_row |= x != x;
      double d = (double)x;
      if (shift != nullptr) d = d - (double)shift[t];
      if (has_floor && d < floor_v) d = floor_v;  // a NaN stays
      a[t] = d;
      s = t == 0 ? d * d : s + d * d;
    }
  const double nrm = sqrt(s);
#pragma unroll
  for (int t = 0; t < MC; ++t)
    if (t < m) a[t] = a[t] / nrm;
  return nrm;
}

// c = ((â_0·b̂_0 + â_1·b̂_1) + â_2·b̂_2) + … with b̂_t at bn[t · stride]; a NaN counts as −inf, otherwise the clamp to [0, 1]
// applies; is_self (the entry j = i under self_zero) counts as exactly 0
template <int MC>
__device__ __forceinline__ double rv_cosine(const double (&a)[MC], const double* bn, int stride, int m, int clamp, bool is_self) {
  double c = 0.0;
#pragma unroll
  for (int t = 0; t < MC; ++t)
    if (t < m) {
      const double p = a[t] * bn[t * stride];
      c = t == 0 ? p : c + p;
    }
  if (c != c) c = -INFINITY;
  else if (clamp) c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
  if (is_self) c = 0.0;
  return c;
}

// the 64 lanes' (value, position) → the largest value and the lowest position that holds it, in every lane
__device__ __forceinline__ void rv_wave_best(double& bst, int& arg) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(bst, off);
    const int oa = __shfl_xor(arg, off);
    if (ob > bst || (ob == bst && oa < arg)) {
      bst = ob;
      arg = oa;
    }
  }
}

// what lane 0 makes of the reduced pair: a NaN row gives arg −1 and best 0 (self_zero) or −inf; no entry above −inf gives arg 0
__device__ __forceinline__ void rv_settle(bool nan_row, int self_zero, double& bst, int& arg) {
  if (nan_row) {
    bst = self_zero ? 0.0 : -INFINITY;
    arg = -1;
  } else if (arg == RV_NO_ROW) {
    arg = 0;  // every entry −inf
  }
}

// apd = (1 + ((m · θ) · acos(best)) / γ) · |a|
__device__ __forceinline__ double rv_apd(int m, float theta, double bst, double gamma, double nrm) {
  const double angle = acos(bst);
  return (1.0 + (((double)m * (double)theta) * angle) / gamma) * nrm;
}

}  // namespace evx
