// What SRA's two selection files share, so that they cannot drift: sra_select.hip (one population: a grid of workgroups forms
// the indicators, one workgroup ranks) and sra_small.hip (a workgroup per run does both).  The indicator arithmetic of a pair
// (q, p), the fold of a wave's 64 partials, and the item, comparator and step window of the pipelined stochastic ranking are
// written once, here.  Both files are compiled with the default flags (no FILE_FLAGS entry), so the squares of I2 contract into
// the same FMAs and a run's I1 and I2 equal the solo kernel's bit for bit.  Everything is forced inline.
#pragma once
#include "evoxmi_mo.h"

namespace evx {

// ---------------------------------------------------------------- indicators
// These two are macros, not forced-inline functions: the compiler optimises such a function on its own before it inlines it, and
// with either as a function (references, values, one tree level per call, templates: all were tried) sra_indicators_kernel came
// out with other register assignments and another schedule than before the split.  As macros the kernel is the same code.
//
// One pair: row q (oq) seen from row p (op), m objectives.  sum gains exp(−max_k(o_qk − o_pk) / 0.05) (q = p included, as in
// torch); where `other` (q ≠ p) holds mn folds Σ_k max(o_qk − o_pk, 0)² (sqrtf is monotone and keeps NaN: the root is taken
// once, at the end).  Division and expf are the accurate ones (the terms reach e^20); max and min propagate NaN as torch's amax /
// clamp / min do.
#define EVX_SI_PAIR(oq, op, m, other, sum, mn)    \
  {                                               \
    float mx = (oq)[0] - (op)[0];                 \
    float c = mx < 0.f ? 0.f : mx;                \
    float d2 = c * c;                             \
    for (int k = 1; k < (m); ++k) {               \
      const float d = (oq)[k] - (op)[k];          \
      mx = evx::nan_max(mx, d);                   \
      c = d < 0.f ? 0.f : d;                      \
      d2 += c * c;                                \
    }                                             \
    sum += expf(-mx / 0.05f);                     \
    if (other) mn = evx::nan_min(mn, d2);         \
  }

// The 64 lanes' partials (lane l: q ≡ l (mod 64), ascending) in one fixed xor tree, sum and min together: the same bits in every
// run.  (As evx::wave_sum and wave_nan_min the code length changes, 3516 to 3488 B.)
#define EVX_SI_TREE(sum, mn)                              \
  _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) {    \
    sum += __shfl_xor(sum, o, 64);                        \
    mn = evx::nan_min(mn, __shfl_xor(mn, o, 64));         \
  }

// ---------------------------------------------------------------- ranking
struct SrItem {
  float a, b;  // I1, I2
  int id;
};

// the comparator of one position: by I1 (by_a) or I2, the larger first; a NaN never swaps
__device__ __forceinline__ void sr_cswap(bool active, bool by_a, SrItem& x, SrItem& y) {
  const float kx = by_a ? x.a : x.b, ky = by_a ? y.a : y.b;
  if (active && kx < ky) {
    const SrItem t = x;
    x = y;
    y = t;
  }
}

// S = ⌈n/2⌉ sweeps, sweep s at position j in step t = j + 2s: the last sweep trails the first by lag = 2(S − 1) steps, the sort is
// T = (n − 1) + lag steps, and in step t the comparators sit at j ≡ t (mod 2), sr_lo(t, lag) ≤ j ≤ sr_hi(t, n).  (The lag is an
// argument and not recomputed from S in each helper: in that form sra_rank_kernel compiled to other code than before the split.)
__device__ __forceinline__ int sr_lag(int n) { return 2 * ((n + 1) / 2 - 1); }
__device__ __forceinline__ int sr_steps(int n, int lag) { return (n - 1) + lag; }  // n = 1: 0 steps
__device__ __forceinline__ int sr_lo(int t, int lag) { return max(0, t - lag); }
__device__ __forceinline__ int sr_hi(int t, int n) { return min(t, n - 2); }

}  // namespace evx
