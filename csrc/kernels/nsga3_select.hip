// NSGA-III niche-preserving selection from the last front (evoxmi/algorithms/mo/nsga3.py;
// reference algorithms/mo/nsga3.py:93-211, whose sequential while_loop the Python side
// already reformulates as "keep the K smallest (ρ_j + k, j)").
//
// Inputs per merged row i < n: its Pareto rank, its niche group_i ∈ [0, R) and the
// perpendicular distance group_dist_i to that niche's reference line; last_rank is a device
// word.  front = rank < last_rank survives outright, last = rank == last_rank are the
// candidates, K = N − Σ front of them are kept:
//   rho[j]  = #{front rows in niche j}
//   u_i     = uniform(key)[ordinal of i among the candidates]   (regenerated from the Philox key)
//   big[j]  = min group_dist over the candidates of niche j      (NaN if any is NaN: torch amin)
//   first_i = rho[group_i] == 0 and group_dist_i == big[group_i]
//   k_i     = position of i among its niche's candidates ordered by (first ? −1 : u_i, i)
//   keep the K smallest (level, niche) = (rho[group_i] + k_i, group_i); idx = kept rows, ascending.
//
// One workgroup of 1024 threads × IT items (IT ∈ {1, 2, 4, 8} from n ≤ 1024·IT ≤ 8192) does
// it all on chip, rows held in registers in blocked order so that every stable sort breaks
// ties by row index:
//   1. per niche, rho and the candidate count c (one packed LDS integer add) and big (LDS
//      integer min on order-preserving float bits; NaN maps below every number so it wins);
//   2. candidate ordinals and Σ front by a block scan; u from one Philox block per candidate;
//   3. stable LDS radix sort by the 24 uniform bits (0 for first), then by (niche, not first)
//      over the bits 2R uses (non-candidates get niche R: last) → (niche, key, row) order;
//   4. the first sorted position of each niche → k = position − start;
//   5. the K smallest (level, niche) without a third sort: niche j holds exactly the levels
//      rho_j … rho_j + c_j − 1, so #{level < L} = Σ_j clamp(L − rho_j, 0, c_j).  A bisection
//      on L (≤ 13 block sums) finds the last level L* taken only in part, a block scan over
//      the niches that own level L* admits the first K − #{level < L*} of them, and niche j
//      keeps its candidates at sorted positions below start_j + (L* + admitted_j) − rho_j;
//   6. scan-compaction of front | kept in row order → idx (int64).
// Steps 3–5 are skipped when K = 0.  Only integer LDS atomics: bitwise reproducible.  No
// global atomics, no spin, no grid barrier: every loop has a static trip bound.  group is
// clamped to [0, R) before it indexes LDS.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   IT  VGPR  SGPR  scratch  LDS [B]
//    1  48    88    0        106896
//    2  54    94    0        106896
//    4  62    102   0        106896
//    8  82    106   0        123216
// LDS at IT = 8: sort storage 32 KiB (keys and values are exchanged one after the other)
// + packed counts 32 KiB + niche word 32 KiB + sort-2 keys 16 KiB + marks 8 KiB + scan words =
// 120 KiB of the CU's 160 KiB.  No spill.
#include <rocprim/block/block_radix_sort.hpp>

#include "evoxmi_mo.h"

namespace {

constexpr int NS_THREADS = 1024;
constexpr int NS_MAX = 8192;  // cap on n and on R
constexpr int NS_WAVES = NS_THREADS / 64;
constexpr int NS_NICHES = NS_MAX / NS_THREADS;  // niches owned per thread in step 5

constexpr uint32_t NS_INF_KEY = 0xFF800000u;  // evx::ord_nan_first(+inf)

__device__ __forceinline__ int bits_for(uint32_t vmax) {  // smallest b with vmax < 2^b, ≥ 1
  int b = 1;
  while (b < 32 && (1u << b) <= vmax) ++b;
  return b;
}

template <int IT>
struct NicheShared {
  typename rocprim::block_radix_sort<uint32_t, NS_THREADS, IT, uint32_t>::storage_type sort;
  alignas(16) uint32_t rc[NS_MAX];  // per niche: rho (low half) | candidate count (high half); each ≤ 8192
  // per niche: big (ordered bits) while the sort keys are built, then its first sorted
  // position, then the sorted position below which its candidates are kept (int)
  alignas(16) uint32_t niche[NS_MAX + 1];
  uint16_t key2[NS_MAX];  // per row: (niche << 1) | not first for a candidate, R << 1 otherwise (≤ 16384)
  uint8_t mark[NS_MAX];
  int wsum[NS_WAVES], wsum2[NS_WAVES], red[2][NS_WAVES];
  uint32_t wave_last[NS_WAVES];
};

template <int IT>
__global__ void __launch_bounds__(NS_THREADS) nsga3_niche_select_kernel(const int32_t* __restrict__ rank, const int32_t* __restrict__ last_rank,
                                                                         const int64_t* __restrict__ group, const float* __restrict__ group_dist,
                                                                         const int64_t* __restrict__ key, int n, int N, int R,
                                                                         int64_t* __restrict__ idx) {
  using sort_t = rocprim::block_radix_sort<uint32_t, NS_THREADS, IT, uint32_t>;
  __shared__ NicheShared<IT> sh;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int base = t * IT;
  const int lr = *last_rank;

  for (int j = t; j < NS_MAX; j += NS_THREADS) {
    sh.rc[j] = 0u;
    sh.niche[j] = NS_INF_KEY;
    sh.mark[j] = 0;
  }
  __syncthreads();

  // 1. per niche: front rows, candidates, minimum distance over the candidates
  uint32_t g[IT];
  float gd[IT];
  uint32_t fmask = 0u, lmask = 0u;
  int nfront = 0, nlast = 0;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int r = base + i;
    g[i] = 0u;
    gd[i] = 0.f;
    if (r < n) {
      const int rk = rank[r];
      const int64_t gr = group[r];
      g[i] = (uint32_t)(gr < 0 ? 0 : (gr > R - 1 ? R - 1 : gr));
      gd[i] = group_dist[r];
      if (rk < lr) {
        fmask |= 1u << i;
        ++nfront;
        atomicAdd(&sh.rc[g[i]], 1u);
      } else if (rk == lr) {
        lmask |= 1u << i;
        ++nlast;
        atomicAdd(&sh.rc[g[i]], 0x10000u);
        atomicMin(&sh.niche[g[i]], evx::ord_nan_first(gd[i]));
      }
    }
  }
  // 2. Σ front → K; candidate ordinals (both scans end in a barrier that also publishes rc / big)
  int F, c;
  evx::block_scan_excl<NS_WAVES>(nfront, sh.wsum, F);
  int ord = evx::block_scan_excl<NS_WAVES>(nlast, sh.wsum2, c);
  const int K = min(max(N - F, 0), c);  // uniform over the block

  if (K > 0) {
    uint32_t k0, k1;
    evx::load_key(key, k0, k1);
    uint32_t k[IT], v[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      v[i] = (uint32_t)(base + i);
      k[i] = 0u;
      uint32_t k2 = (uint32_t)R << 1;
      if (lmask & (1u << i)) {
        const evx::u4 w = evx::philox_block((uint64_t)(ord >> 2), k0, k1);
        const int q = ord & 3;
        const uint32_t word = q == 0 ? w.x : (q == 1 ? w.y : (q == 2 ? w.z : w.w));
        // the closest member(s) of an empty niche go first, in row order
        const bool first = (sh.rc[g[i]] & 0xFFFFu) == 0u && gd[i] == evx::ord_nan_first_inv(sh.niche[g[i]]);
        k[i] = first ? 0u : word >> 8;  // the 24 bits of u24
        k2 = (g[i] << 1) | (first ? 0u : 1u);
        ++ord;
      }
      sh.key2[base + i] = (uint16_t)k2;
    }
    // 3. by (u, row), then stably by (niche, not first): candidates in (niche, key, row) order, the rest last
    sort_t().sort(k, v, sh.sort, 0, 24);
    __syncthreads();  // every read of big and write of key2 is done; the sort storage is free again
#pragma unroll
    for (int i = 0; i < IT; ++i) k[i] = sh.key2[v[i] & (NS_MAX - 1)];
    sort_t().sort(k, v, sh.sort, 0, bits_for((uint32_t)R << 1));
    // 4. the first sorted position of each niche
    uint32_t prev = __shfl_up(k[IT - 1], 1, 64) >> 1;
    if (lane == 63) sh.wave_last[wave] = k[IT - 1] >> 1;
    __syncthreads();
    if (lane == 0) prev = wave > 0 ? sh.wave_last[wave - 1] : 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const uint32_t gg = k[i] >> 1, gp = i > 0 ? k[i - 1] >> 1 : prev;
      if (gg != gp) sh.niche[gg] = (uint32_t)(base + i);  // gg ≤ R ≤ NS_MAX: inside niche[NS_MAX + 1]
    }
    // 5. L* = the largest L with #{level < L} < K, by bisection; this thread owns NS_NICHES niches
    int rj[NS_NICHES], cj[NS_NICHES];
#pragma unroll
    for (int i = 0; i < NS_NICHES; ++i) {
      const uint32_t x = sh.rc[t * NS_NICHES + i];  // zero for niches ≥ R
      rj[i] = (int)(x & 0xFFFFu);
      cj[i] = (int)(x >> 16);
    }
    int lo = 0, hi = n, below = 0;  // #{level < 0} = 0 < K ≤ c = #{level < n}
    for (int it = 0; it < 14 && hi - lo > 1; ++it) {
      const int mid = (lo + hi) >> 1;
      int s = 0;
#pragma unroll
      for (int i = 0; i < NS_NICHES; ++i) s += min(max(mid - rj[i], 0), cj[i]);
      s = evx::block_sum<NS_WAVES>(s, sh.red[it & 1]);
      if (s < K) { lo = mid; below = s; } else hi = mid;
    }
    const int need = K - below;  // ≥ 1 niches take their candidate at level lo, lowest niche first
    uint32_t own = 0u;
    int nown = 0;
#pragma unroll
    for (int i = 0; i < NS_NICHES; ++i) {
      const bool o = rj[i] <= lo && lo < rj[i] + cj[i];
      own |= (uint32_t)o << i;
      nown += o;
    }
    int tot;
    int before = evx::block_scan_excl<NS_WAVES>(nown, sh.wsum, tot);  // its barrier also publishes the niche starts
#pragma unroll
    for (int i = 0; i < NS_NICHES; ++i) {
      const int j = t * NS_NICHES + i;
      const bool o = (own >> i) & 1u;
      if (cj[i] > 0) sh.niche[j] = (uint32_t)((int)sh.niche[j] + lo + (o && before < need ? 1 : 0) - rj[i]);
      before += o;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const uint32_t gg = k[i] >> 1;
      if (gg < (uint32_t)R && base + i < (int)sh.niche[gg]) sh.mark[v[i] & (NS_MAX - 1)] = 1;
    }
    __syncthreads();
  }

  // 6. kept rows in ascending row order
  int cnt = 0;
  uint32_t keep = 0u;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const bool kp = base + i < n && (((fmask >> i) & 1u) || sh.mark[base + i]);
    keep |= (uint32_t)kp << i;
    cnt += kp;
  }
  int total;
  int pos = evx::block_scan_excl<NS_WAVES>(cnt, sh.wsum, total);  // a barrier lies between every earlier read of wsum and here
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    if ((keep >> i) & 1u) {
      if (pos < N) idx[pos] = (int64_t)(base + i);
      ++pos;
    }
  }
  // inconsistent inputs (fewer than N kept): defined output
  for (int p = total + t; p < N; p += NS_THREADS) idx[p] = 0;
}

}  // namespace

void evx_nsga3_niche_select(const int32_t* rank, const int32_t* last_rank, const int64_t* group, const float* group_dist,
                            const int64_t* key, int n, int N, int R, int64_t* idx, hipStream_t s) {
  if (n <= NS_THREADS)
    nsga3_niche_select_kernel<1><<<1, NS_THREADS, 0, s>>>(rank, last_rank, group, group_dist, key, n, N, R, idx);
  else if (n <= 2 * NS_THREADS)
    nsga3_niche_select_kernel<2><<<1, NS_THREADS, 0, s>>>(rank, last_rank, group, group_dist, key, n, N, R, idx);
  else if (n <= 4 * NS_THREADS)
    nsga3_niche_select_kernel<4><<<1, NS_THREADS, 0, s>>>(rank, last_rank, group, group_dist, key, n, N, R, idx);
  else
    nsga3_niche_select_kernel<8><<<1, NS_THREADS, 0, s>>>(rank, last_rank, group, group_dist, key, n, N, R, idx);
}
