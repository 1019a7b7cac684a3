// Non-dominated sort of B independent runs in one launch: workgroup b ranks rows [b·n, (b+1)·n) of f (B, n, m).
//
// Per run the contract is nds.hip's: minimisation (a dominates b when a ≤ b in every objective and a < b in
// one; equal rows and rows with a NaN dominate nothing), front k = the rows all of whose dominators sit in
// fronts < k, and with limit < n the run stops peeling once at least `limit` of its rows are ranked, the
// others getting rank n.  The stop is per run.
//
// nds.hip ranks one large population with a chip-wide persistent grid and a grid barrier, which cannot take a
// run axis.  Here a run is small (n ≤ 8192) and a workgroup does all of it, the way m2m_select.hip ranks a
// region's members (evoxmi_peel.h): dominator counts in registers from one pass over the run's row pairs, the
// candidates staged through an LDS tile, then one front per iteration: the unranked rows with count 0, laid
// out in row order by an ordered compaction, after which every thread lowers its owned counts by the rows of
// the new front that dominate them.  Dominance is a strict partial order, so every iteration ranks at least
// one row and a run takes at most n of them, ±inf and NaN included.  No grid barrier, no global atomics, no
// workspace in global memory, nothing shared between runs.
//
// A workgroup has 256 threads for n ≤ 512 (at most 2 owned rows per thread) and 1024 above; the ranks do not
// depend on it.  m is padded to MT ∈ {4, 8}.
#include "evoxmi_launchers.h"
#include "evoxmi_peel.h"

namespace {

constexpr int NDSB_SMALL_THREADS = 256;
constexpr int NDSB_SMALL_N = 512;
constexpr int NDSB_THREADS = 1024;

template <int THREADS>
struct NdsbShared {
  float tile[evx::PEEL_TILE];
  uint32_t front[THREADS * evx::PEEL_ITEMS];  // the rows of the new front, ascending
  int wcnt[evx::PEEL_ITEMS * THREADS / 64];
};

template <int MT, int THREADS>
__global__ void __launch_bounds__(THREADS) nds_batched_kernel(const float* __restrict__ f, int n, int m, int limit,
                                                              int32_t* __restrict__ rank) {
  __shared__ NdsbShared<THREADS> sh;
  const int t = threadIdx.x;
  f += (int64_t)blockIdx.x * n * m;
  rank += (int64_t)blockIdx.x * n;

  const int nit = (n + THREADS - 1) / THREADS;  // ≤ PEEL_ITEMS: n ≤ THREADS · PEEL_ITEMS
  int cnt[evx::PEEL_ITEMS], pre[evx::PEEL_ITEMS];
  uint32_t alive = 0;
#pragma unroll
  for (int it = 0; it < evx::PEEL_ITEMS; ++it) {
    cnt[it] = 0;
    alive |= (it * THREADS + t < n ? 1u : 0u) << it;
  }
  const auto row = [](int i) { return i; };
  evx::peel_count_pass<MT, THREADS, false>(f, m, sh.tile, n, nit, alive, cnt, false, row, row);

  int ranked = 0, k = 0;
  bool force = false;
  for (;;) {
    uint32_t flags = 0;
#pragma unroll
    for (int it = 0; it < evx::PEEL_ITEMS; ++it) flags |= (((alive >> it) & 1u) && (cnt[it] <= 0 || force) ? 1u : 0u) << it;
    const int tot = evx::peel_compact<THREADS>(flags, nit, sh.wcnt, pre);  // its barriers also end the reads of tile and front
    if (tot == 0) {  // cannot happen while a row is unranked (strict partial order); keeps the loop finite regardless
      force = true;
      continue;
    }
#pragma unroll
    for (int it = 0; it < evx::PEEL_ITEMS; ++it) {
      if ((flags >> it) & 1u) {
        const int r = it * THREADS + t;
        sh.front[pre[it]] = (uint32_t)r;
        rank[r] = k;
      }
    }
    alive &= ~flags;
    ranked += tot;
    if (ranked >= n) return;  // uniform: tot and ranked are the same in every thread
    if (ranked >= limit || k + 1 >= n) {
#pragma unroll
      for (int it = 0; it < evx::PEEL_ITEMS; ++it)
        if ((alive >> it) & 1u) rank[it * THREADS + t] = n;
      return;
    }
    evx::peel_count_pass<MT, THREADS, true>(f, m, sh.tile, tot, nit, alive, cnt, true, [&](int i) { return (int)sh.front[i]; }, row);
    ++k;
  }
}

template <int THREADS>
void launch(const float* f, int B, int n, int m, int limit, int32_t* rank, hipStream_t s) {
  if (m <= 4)
    nds_batched_kernel<4, THREADS><<<B, THREADS, 0, s>>>(f, n, m, limit, rank);
  else
    nds_batched_kernel<8, THREADS><<<B, THREADS, 0, s>>>(f, n, m, limit, rank);
}

}  // namespace

int evx_nds_batched_max_n() { return NDSB_THREADS * evx::PEEL_ITEMS; }
int evx_nds_batched_max_m() { return 8; }

void evx_nds_batched(const float* f, int B, int n, int m, int limit, int32_t* rank, hipStream_t s) {
  if (n <= NDSB_SMALL_N)
    launch<NDSB_SMALL_THREADS>(f, B, n, m, limit, rank, s);
  else
    launch<NDSB_THREADS>(f, B, n, m, limit, rank, s);
}
