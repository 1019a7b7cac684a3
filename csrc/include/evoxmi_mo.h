// What the multi-objective selection kernels share: block-wide integer sum and scan, ordered key images of a
// float, the row-dominance test, the tile staging of the "wave per row, the other rows through LDS" kernels, and
// the parts of the one-workgroup removal kernels (spea2_select.hip, bce_select.hip) that are the same in both.
// Everything is forced inline; nothing here depends on -ffp-contract (no float expression that could fuse).
// The compiler optimises a forced-inline helper on its own before it inlines it, so a helper with a loop or a
// branch can reorder the caller's code: a kernel uses a helper only where its registers, scratch, LDS and code
// length stayed what they were, and says so in a comment where it keeps its own copy instead.
#pragma once
#include <type_traits>

#include "evoxmi_common.h"
#include "evoxmi_launchers.h"

namespace evx {

// ---------------------------------------------------------------- block primitives (WAVES waves of 64)
// Block sum of one int per thread, one barrier: callers alternate between two `buf`s so that a buffer is
// rewritten only after the barrier that follows its last read.
template <int WAVES>
__device__ __forceinline__ int block_sum(int v, int* buf) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) all += buf[w];
  return all;
}

// Exclusive block scan of one int per thread in thread order, one barrier; `total` gets the block sum.  `wsum`
// (WAVES ints) may be rewritten only after a later barrier.
template <int WAVES>
__device__ __forceinline__ int block_scan_excl(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int s = wsum[w];
    before += w < wave ? s : 0;
    all += s;
  }
  total = all;
  return before + inc - v;
}

// The lanes with `flag` append `v` to list[count …] in lane order; returns the new count (wave-uniform).  `below`
// is the caller's mask of the lanes before its own, (1ull << lane) − 1.  No barrier: the list belongs to the wave
// until its owner publishes the count.
__device__ __forceinline__ int wave_append(bool flag, uint16_t v, uint16_t* list, int count, unsigned long long below) {
  const unsigned long long bal = __ballot(flag);
  if (flag) list[count + __popcll(bal & below)] = v;
  return count + __popcll(bal);
}

// ---------------------------------------------------------------- ordered key images
// uint32 images of a float whose unsigned order is the float order.  The conventions differ only in where NaN and
// −0 go:
//   ord_bits       the raw image: −NaN < −inf < … < −0 < +0 < … < +inf < +NaN
//   ord_canon      NaN (either sign) → +qNaN's image 0xFFC00000, after +inf; −0 = +0.  Never 0, and its complement
//                  is never 0xFFFFFFFF.  sort.hip's ord_key differs at NaN only (0xFFFFFFFF there) and stays apart.
//   ord_nan_first  NaN → 0, below −inf's 0x007FFFFF; −0 < +0.  ord_nan_first_inv gives the float back (NaN as +qNaN).
__device__ __forceinline__ uint32_t ord_bits(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t ord_canon(float x) {
  uint32_t b = __float_as_uint(x);
  if (x != x) b = 0x7fc00000u;
  if (x == 0.f) b = 0u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t ord_nan_first(float x) { return x != x ? 0u : ord_bits(x); }
__device__ __forceinline__ float ord_nan_first_inv(uint32_t k) {
  if (k == 0u) return __int_as_float(0x7fc00000);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// (image, index) as one word: compared first on the image, then on the index word
__device__ __forceinline__ unsigned long long key64(uint32_t image, uint32_t index) {
  return ((unsigned long long)image << 32) | index;
}

// ---------------------------------------------------------------- dominance
// Row a dominates row b (minimisation): a ≤ b in every objective and a < b in one; a(k), b(k) give the k-th
// objective.  A NaN compares false on both sides, so neither flag follows from the other (!(x ≤ y) is not y < x):
// keep the &= / |= form.
template <class FA, class FB>
__device__ __forceinline__ bool dominates(FA a, FB b, int m) {
  bool le = true, lt = false;
  for (int k = 0; k < m; ++k) {
    const float x = a(k), y = b(k);
    le &= x <= y;
    lt |= x < y;
  }
  return le && lt;
}
// both directions from one read of each objective
template <class FA, class FB>
__device__ __forceinline__ void dominates_both(FA a, FB b, int m, bool& a_dom_b, bool& b_dom_a) {
  bool le = true, lt = false, ge = true, gt = false;
  for (int k = 0; k < m; ++k) {
    const float x = a(k), y = b(k);
    le &= x <= y;
    lt |= x < y;
    ge &= y <= x;
    gt |= y < x;
  }
  a_dom_b = le && lt;
  b_dom_a = ge && gt;
}

// ---------------------------------------------------------------- tiled row scan
// The staging step of the "wave per row, the other rows through LDS" kernels (spea2_fit1/2, sra_indicators,
// ibea_fitness): the THREADS threads of the workgroup copy rows i0 … i0 + rows − 1 of obj (n, m) into `tile` with
// the odd row stride ms = m | 1 (conflict free for the lane-per-row reads that follow).  No barrier: the caller
// has one before (the previous tile is consumed) and one after.  The frame around it (own row in LDS, two
// barriers, the lane-strided loop) stays in each kernel: as one template over a per-pair body it cost
// spea2_fit1 12 bytes of scratch and changed the code length of the other three.
template <int THREADS>
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ obj, int i0, int rows, int m, int ms, int tid) {
  for (int e = tid; e < rows * m; e += THREADS) tile[(e / m) * ms + e % m] = obj[(int64_t)i0 * m + e];
}

// ---------------------------------------------------------------- the one-workgroup removal frame
// spea2_truncate_kernel and bce_remove_kernel: one workgroup of TB = 256 or 512 threads, thread r keeps the IT
// rows r, r + TB, … in registers and bit i of `live` says that row r + i·TB is masked and not removed.  Per step
// every wave compacts the rows to rescan into its part of `wlist` (wave w: entries w·64·IT …, see wave_append)
// and publishes RemovalPart{its arg-best key, its list length}.
template <int TB>
struct RemovalShape {
  static_assert(TB == 256 || TB == 512, "a power of two, at most 512");
  static constexpr int lg = TB == 256 ? 8 : 9, nt = TB, nw = TB >> 6;
};

struct alignas(16) RemovalPart {
  unsigned long long key;
  int cnt;
};

// keep = the live bits, order padded with −1 from k_remove on, stats = {rescans, k_remove}
template <int IT, int TB>
__device__ __forceinline__ void removal_finish(uint32_t live, int n, int k_remove, int rescans, uint8_t* __restrict__ keep,
                                               int64_t* __restrict__ order, int n_order, int32_t* __restrict__ stats) {
  const int r = threadIdx.x;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = r + (i << RemovalShape<TB>::lg);
    if (p < n) keep[p] = (uint8_t)((live >> i) & 1u);
  }
  for (int t = k_remove + r; t < n_order; t += TB) order[t] = -1;
  if (r == 0) {
    stats[0] = rescans;
    stats[1] = k_remove;
  }
}

// ---------------------------------------------------------------- host side
// f(std::integral_constant<int, MM>{}) for the padded objective count M = evx_padded_m(m)
template <class F>
void dispatch_padded_m(int M, F f) {
  if (M == 2)
    f(std::integral_constant<int, 2>{});
  else if (M == 3)
    f(std::integral_constant<int, 3>{});
  else if (M == 4)
    f(std::integral_constant<int, 4>{});
  else if (M == 8)
    f(std::integral_constant<int, 8>{});
  else
    f(std::integral_constant<int, 16>{});
}

// f(IT, TB as integral constants) for a removal over n ≤ 8192 rows: four waves (one per SIMD) while eight rows
// per thread suffice, then eight waves
template <class F>
void dispatch_removal_shape(int n, F f) {
  using std::integral_constant;
  if (n <= 256)
    f(integral_constant<int, 1>{}, integral_constant<int, 256>{});
  else if (n <= 512)
    f(integral_constant<int, 2>{}, integral_constant<int, 256>{});
  else if (n <= 1024)
    f(integral_constant<int, 4>{}, integral_constant<int, 256>{});
  else if (n <= 2048)
    f(integral_constant<int, 8>{}, integral_constant<int, 256>{});
  else if (n <= 4096)
    f(integral_constant<int, 8>{}, integral_constant<int, 512>{});
  else
    f(integral_constant<int, 16>{}, integral_constant<int, 512>{});
}

}  // namespace evx
