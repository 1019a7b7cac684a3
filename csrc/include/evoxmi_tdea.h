// The device pieces of θ-DEA's θ-ranking that tdea_select.hip (one problem, after rvea_select.hip's launches) and
// tdea_small.hip (a workgroup per run) share, so that the two cannot drift: the contract in the docstring of
// evoxmi/ops/tdea.py is written once, here.  Every operation is float64 in the order stated there; both files are
// compiled with -ffp-contract=off, so nothing in here fuses.  Everything is forced inline.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace evx {

// cls and val of a row from (best, arg) of cos_best, mode 0: cls = arg, a NaN row's −1 as 0; c = best clamped to [−1, 1];
// |a| = sqrt(((a_0² + a_1²) + a_2²) + …); d1 = |a| · c, d2 = |a| · sqrt(max(1 − c · c, 0)); val = d1 + (double)θ_cls · d2
__device__ __forceinline__ void td_cls_val(const float* __restrict__ row, int m, int nw, double best, int arg, const float* theta, int& cls,
                                           double& val) {
  double s = 0.0;
  for (int t = 0; t < m; ++t) {
    const double d = (double)row[t];
    s = t == 0 ? d * d : s + d * d;
  }
  const double nrm = sqrt(s);
  cls = arg < 0 ? 0 : (arg >= nw ? nw - 1 : arg);  // a NaN row's −1
  double c = best;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  const double d1 = nrm * c;
  double q = 1.0 - c * c;
  if (q < 0.0) q = 0.0;
  const double d2 = nrm * sqrt(q);
  val = d1 + (double)theta[cls] * d2;
}

// whether row j orders before row i inside a cluster: by (val, position), a NaN after every number
__device__ __forceinline__ bool td_before(double vj, int j, double vi, int i) {
  const bool nan_i = vi != vi, nan_j = vj != vj;
  if (nan_i || nan_j) return nan_i && (!nan_j || j < i);
  return vj < vi || (vj == vi && j < i);
}

}  // namespace evx
