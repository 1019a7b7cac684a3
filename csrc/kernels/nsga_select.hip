// NSGA-II environmental selection after the non-dominated sort (K10 of SURVEY §2.10;
// reference algorithms/mo/nsga2.py:86-100 and operators/selection/non_dominate.py:116-204).
//
// Semantics: worst = sorted(rank)[mask_pos]; crowding distance on the front
// `rank == worst` (per objective: stable sort by cost, extremes +inf, interior
// (c[p+1] − c[p−1]) / (c[last] − c[0]), summed over objectives; rows outside the front
// get −inf); survivors = lexsort((−cd, rank))[:N] (stable: ties by row index).
//
// The survivors are identical to the torch path (ops/nds.py:crowding_distance + lexsort)
// for finite objectives.  The crowding distance here is computed on the cut front alone:
// only its rows are sorted.  The torch path sorts all n rows with the masked-out ones keyed
// +inf, so a cut-front row that holds +inf (or NaN) ties with (or sorts after) masked rows
// there, its "last valid" slot can be a masked row, and the survivors then differ from this
// kernel's whenever other rows are masked out.
//
// One workgroup of 1024 threads × 8 items does it all on chip (n ≤ 8192).  Every sort is
// rocPRIM's stable LDS block radix sort with the items held in registers (blocked
// arrangement), so a sort is a handful of 4-bit digit passes instead of the 91
// compare-exchange rounds of a bitonic network:
//   1. (rank, row) over only the bits the ranks use → the survivors of ranks < worst in
//      output order, and the worst front [lo, hi) in row order;
//   2. per objective, (cost, slot) over the front → crowding distance, neighbours
//      exchanged through DPP shuffles + one LDS word per wave;
//   3. (−cd, slot) → the remaining survivors.
// Steps 2–3 sort 1024·IT keys with IT ∈ {1, 2, 4, 8} picked from the front size.  They are
// evx::crowd_select (evoxmi_crowd.h), shared with m2m_select.hip.
// Float keys are canonicalised first (NaN → +qNaN, −0 → +0) so the bit-order radix sort
// agrees with torch.sort (NaN last, ±0 equal, stable ties).
// It replaces ~60 small library launches (sorts, gathers, scatters, lexsort) per
// generation with one.
// Batched runs: workgroup b selects among run b's rows, rank (B, n) and f (B, n, m) → keep (B, N).  The
// workgroups share nothing, so row b is the single-run result on run b.
#include "evoxmi_crowd.h"

namespace {

constexpr int SEL_THREADS = evx::CROWD_THREADS;
constexpr int SEL_ITEMS = 8;
constexpr int SEL_MAXN = SEL_THREADS * SEL_ITEMS;  // 8192
constexpr int SEL_WAVES = SEL_THREADS / 64;

using rank_sort_t = rocprim::block_radix_sort<uint32_t, SEL_THREADS, SEL_ITEMS, uint32_t>;

union SortStorage {
  typename rank_sort_t::storage_type r;
  evx::CrowdSortStorage k;
};

struct SelShared {
  SortStorage sort;
  uint32_t srow[SEL_MAXN];  // rows in (rank, row) order
  uint32_t srank[SEL_MAXN];
  float cd[SEL_MAXN];       // crowding distance per front slot
  float wave_first[SEL_WAVES], wave_last[SEL_WAVES];
  float key0, keyl;
  int lo, hi, maxr;
};

__global__ void __launch_bounds__(SEL_THREADS) nsga_select_kernel(const int32_t* __restrict__ rank, const float* __restrict__ f, int n, int m,
                                                                   int N, int mask_pos, int64_t* __restrict__ keep) {
  __shared__ SelShared sh;
  const int t = threadIdx.x;
  const int base = t * SEL_ITEMS;
  rank += (int64_t)blockIdx.x * n;
  f += (int64_t)blockIdx.x * n * m;
  keep += (int64_t)blockIdx.x * N;

  // 1. stable sort of rows by rank.  Unranked rows (rank n, past the early stop) map to
  // max ranked + 1, so the radix sort only walks the bits the ranks actually use.
  uint32_t k[SEL_ITEMS], v[SEL_ITEMS];
  int mr = -1;
#pragma unroll
  for (int i = 0; i < SEL_ITEMS; ++i) {
    const int r = base + i;
    k[i] = r < n ? (uint32_t)min(max(rank[r], 0), n) : (uint32_t)n;
    if ((int)k[i] < n) mr = max(mr, (int)k[i]);
    v[i] = (uint32_t)r;
  }
  if (t == 0) { sh.lo = n; sh.hi = n; sh.maxr = -1; }
  __syncthreads();
  mr = (int)evx::wave_max((float)mr);  // exact: ranks ≤ 8192
  if ((t & 63) == 0) atomicMax(&sh.maxr, mr);
  __syncthreads();
  const uint32_t cap = (uint32_t)(sh.maxr + 1);  // ≤ n ≤ 8192
  int bits = 1;
  while ((1u << bits) <= cap) ++bits;
#pragma unroll
  for (int i = 0; i < SEL_ITEMS; ++i) k[i] = k[i] > cap ? cap : k[i];
  rank_sort_t().sort(k, v, sh.sort.r, 0, bits);
#pragma unroll
  for (int i = 0; i < SEL_ITEMS; ++i) { sh.srank[base + i] = k[i]; sh.srow[base + i] = v[i]; }
  __syncthreads();
  const uint32_t worst = sh.srank[mask_pos];
#pragma unroll
  for (int i = 0; i < SEL_ITEMS; ++i) {
    const int p = base + i;
    if (p < n) {
      const uint32_t r = sh.srank[p];
      const uint32_t rp = p > 0 ? sh.srank[p - 1] : 0xFFFFFFFFu;
      if (r == worst && (p == 0 || rp != worst)) sh.lo = p;  // first slot of the worst front
      if (r > worst && (p == 0 || rp <= worst)) sh.hi = p;   // first slot after it
    }
  }
  __syncthreads();
  const int lo = sh.lo, hi = sh.hi, F = hi - lo;
  // survivors of ranks < worst, already in (rank, row) order
  for (int i = t; i < lo && i < N; i += SEL_THREADS) keep[i] = (int64_t)sh.srow[i];
  const int need = N - lo;
  if (need <= 0) return;  // uniform: every thread leaves together
  if (F <= SEL_THREADS) evx::crowd_select<1>(sh, sh.sort.k, f, m, lo, F, need, keep);
  else if (F <= 2 * SEL_THREADS) evx::crowd_select<2>(sh, sh.sort.k, f, m, lo, F, need, keep);
  else if (F <= 4 * SEL_THREADS) evx::crowd_select<4>(sh, sh.sort.k, f, m, lo, F, need, keep);
  else evx::crowd_select<8>(sh, sh.sort.k, f, m, lo, F, need, keep);
}

}  // namespace

void evx_nsga_select(const int32_t* rank, const float* f, int n, int m, int N, int mask_pos, int64_t* keep, hipStream_t s, int batch) {
  nsga_select_kernel<<<batch, SEL_THREADS, 0, s>>>(rank, f, n, m, N, mask_pos, keep);
}
