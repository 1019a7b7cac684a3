// The device pieces of BiGE's bi-goal estimate that bige_select.hip (one population, three chip-wide launches) and
// bige_small.hip (a workgroup per run) share, so that the two cannot drift: the contract in the docstring of
// evoxmi/ops/bige.py is written once, here.  Every operation is float64 on the float32 inputs in the order stated there;
// both files are compiled with -ffp-contract=off, so nothing in here fuses.  Everything is forced inline.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace evx {

// x_t = ((double)f_t − (double)fmin_t) / max((double)fmax_t − (double)fmin_t, 1e-6) of one masked row into x[t · stride], and
// its proximity ((x_0 + x_1) + x_2) + …; a row outside the mask gets +inf throughout: its distance to every masked row is
// +inf, never below r, so it contributes to nothing without a test of its own
__device__ __forceinline__ double bg_normalise_row(const float* __restrict__ row, bool masked, int m, const float* fmin, const float* fmax,
                                                   double* x, size_t stride) {
  if (!masked) {
    for (int t = 0; t < m; ++t) x[(size_t)t * stride] = INFINITY;
    return INFINITY;
  }
  double s = 0.0;
  for (int t = 0; t < m; ++t) {
    const double lo = (double)fmin[t];
    double span = (double)fmax[t] - lo;
    if (!(span >= 1e-6)) span = 1e-6;
    const double v = ((double)row[t] - lo) / span;
    x[(size_t)t * stride] = v;
    s = t == 0 ? v : s + v;
  }
  return s;
}

// r² · (1 + 2⁻⁴⁰): r² is exact, r being a float32, and the product rounds once.  A pair with d2 at or above it has an exact
// root above r, and a correctly rounded root is monotone, so d ≥ r: the prefilter never drops a pair that d < r keeps
__device__ __forceinline__ double bg_prefilter(double r) { return (r * r) * (1.0 + 0x1p-40); }

// The term of the pair (i, j): a is x_i, xj[t · stride] is x_jt, pi and *pj the proximities (pj is read only for a pair
// inside the radius).  d2 = ((δ_0² + δ_1²) + …); a pair at distance 0 is counted in dup (it is exactly 1: equal x, so equal
// pr, w = 2 and sh = (0.5 · (2 · (1 − 0 / r)))²), any other with d < r adds sh = (0.5 · (w · (1 − d / r)))² to acc
template <int MC>
__device__ __forceinline__ void bg_pair(const double (&a)[MC], const double* xj, int stride, int m, bool self, double pi, const double* pj,
                                        double r, double rr_hi, double& acc, int& dup) {
  double d2 = 0.0;
#pragma unroll
  for (int t = 0; t < MC; ++t)
    if (t < m) {
      const double dl = a[t] - xj[t * stride];
      const double p = dl * dl;
      d2 = t == 0 ? p : d2 + p;
    }
  if (d2 < rr_hi && !self) {  // a NaN fails the test
    const double d = sqrt(d2);
    if (d2 == 0.0 && 0.0 < r) {
      dup += 1;
    } else if (d < r) {
      const double q = *pj;
      const double wgt = 1.0 + (pi >= q ? 1.0 : 0.0) + (pi > q ? 1.0 : 0.0);
      const double h = 0.5 * (wgt * (1.0 - d / r));
      acc += h * h;
    }
  }
}

// cd of a row from its 64 lanes' partial sums: the xor butterfly 32, 16, …, 1, then sqrt(acc + dup).  Lane l has added its
// partners j ≡ l (mod 64) in ascending j; every term is ≥ 0 and the order is fixed, so the word is the same from call to call
__device__ __forceinline__ double bg_wave_cd(double acc, int dup) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_xor(acc, off);
    dup += __shfl_xor(dup, off);
  }
  return sqrt(acc + (double)dup);
}

}  // namespace evx
