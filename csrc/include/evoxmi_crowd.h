// NSGA-II crowding distance on one front and the pick of its best slots, in one workgroup of
// 1024 threads (shared by nsga_select.hip and m2m_select.hip).
//
// Per objective: a stable sort of the front by canonicalised cost (NaN → +qNaN, −0 → +0, so
// the bit-order radix sort agrees with torch.sort: NaN last, ±0 equal, stable ties), the
// extremes get +inf, an interior row (next − prev) / (last − first) as one float32 subtraction
// and one correctly rounded float32 division; the terms are added in objective order 0 … m−1
// starting from 0.  The final sort is by −cd (NaN last), ties by slot.  Every sort is rocPRIM's
// stable LDS block radix sort with IT ∈ {1, 2, 4, 8} items per thread in registers.
#pragma once
#include <rocprim/block/block_radix_sort.hpp>

#include "evoxmi_common.h"

namespace evx {

constexpr int CROWD_THREADS = 1024;
constexpr int CROWD_WAVES = CROWD_THREADS / 64;
constexpr int CROWD_MAXN = CROWD_THREADS * 8;  // 8192 front slots at most

template <int IT>
using crowd_sort_t = rocprim::block_radix_sort<float, CROWD_THREADS, IT, uint32_t>;

union CrowdSortStorage {
  typename crowd_sort_t<1>::storage_type k1;
  typename crowd_sort_t<2>::storage_type k2;
  typename crowd_sort_t<4>::storage_type k4;
  typename crowd_sort_t<8>::storage_type k8;
};

template <int IT>
__device__ __forceinline__ typename crowd_sort_t<IT>::storage_type& crowd_storage(CrowdSortStorage& st) {
  if constexpr (IT == 1) return st.k1;
  else if constexpr (IT == 2) return st.k2;
  else if constexpr (IT == 4) return st.k4;
  else return st.k8;
}

__device__ __forceinline__ float crowd_canon(float x) {
  if (x != x) return __int_as_float(0x7fc00000);
  return x == 0.f ? 0.f : x;
}

// Crowding distance on the front slots [0, F) (rows sh.srow[lo + slot]) and the `need`
// best slots by (−cd, slot), written to keep[lo ...]; IT items per thread cover F <= 1024·IT,
// so a small front sorts IT·1024 keys instead of 8192.  `Shared` provides srow[] (uint32 rows),
// cd[CROWD_MAXN], wave_first[], wave_last[] (CROWD_WAVES floats each), key0 and keyl.
template <int IT, class Shared>
__device__ __forceinline__ void crowd_select(Shared& sh, CrowdSortStorage& st, const float* __restrict__ f, int m, int lo, int F, int need,
                                             int64_t* __restrict__ keep) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int base = t * IT;
  using sort_t = crowd_sort_t<IT>;
#pragma unroll
  for (int i = 0; i < IT; ++i) sh.cd[base + i] = 0.f;
  for (int obj = 0; obj < m; ++obj) {
    float k[IT];
    uint32_t v[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int s = base + i;
      // +qNaN padding ties with real NaNs but sits after them (stable: larger slots)
      k[i] = s < F ? crowd_canon(f[(int64_t)sh.srow[lo + s] * m + obj]) : __int_as_float(0x7fc00000);
      v[i] = (uint32_t)s;
    }
    __syncthreads();  // sort storage reuse and the cd writes of the previous objective
    sort_t().sort(k, v, crowd_storage<IT>(st));
    // neighbour keys across the thread boundary: shuffles within the wave, LDS across waves
    float prev = __shfl_up(k[IT - 1], 1);
    float next = __shfl_down(k[0], 1);
    if (lane == 0) sh.wave_first[wave] = k[0];
    if (lane == 63) sh.wave_last[wave] = k[IT - 1];
    if (t == 0) sh.key0 = k[0];
#pragma unroll
    for (int i = 0; i < IT; ++i)
      if (base + i == F - 1) sh.keyl = k[i];
    __syncthreads();
    if (lane == 0 && wave > 0) prev = sh.wave_last[wave - 1];
    if (lane == 63 && wave < CROWD_WAVES - 1) next = sh.wave_first[wave + 1];
    const float rng = sh.keyl - sh.key0;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int p = base + i;
      if (p < F) {
        const float kp = i > 0 ? k[i - 1] : prev;
        const float kn = i < IT - 1 ? k[i + 1] : next;
        const float d = (p == 0 || p == F - 1) ? INFINITY : (kn - kp) / rng;
        sh.cd[v[i]] += d;  // v is a permutation of the slots: no two threads share a slot
      }
    }
  }
  __syncthreads();
  // the best `need` slots of the front by (−cd, slot)
  float k[IT];
  uint32_t v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int s = base + i;
    k[i] = s < F ? crowd_canon(-sh.cd[s]) : __int_as_float(0x7fc00000);
    v[i] = (uint32_t)s;
  }
  sort_t().sort(k, v, crowd_storage<IT>(st));
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = base + i;
    if (p < need) keep[lo + p] = (int64_t)sh.srow[lo + v[i]];
  }
}

}  // namespace evx
