// MOEA/D-M2M's association (reference algorithms/mo/moeadm2m.py:60-95): every one of the K regions keeps
// S rows, chosen by an NSGA-II selection among the rows assigned to it.  One launch, one workgroup of 1024
// threads per region; the workgroups are independent (no grid barrier, no global atomics).
//
// Per region k, with c the number of rows whose region == k:
//   c < S   the member rows in ascending row order, then rad[c:S];  worst[k] = −1;
//   c ≥ S   fronts of the members are peeled (minimisation: a dominates b when a ≤ b in every objective and
//           a < b in one; equal rows and rows with a NaN dominate nothing) until at least S members are
//           ranked; worst[k] is that last rank and lo the number of members ranked before it.  The first lo
//           outputs are the members of ranks < worst in (rank, row) order, the other S − lo the cut front's
//           members by (−cd, row), cd the crowding distance on the cut front alone (evoxmi_crowd.h).
//
// part is identical to the CPU torch path (algorithms/mo/moeadm2m.py::association_indices) for finite
// objectives: dominance is comparisons only, the crowding arithmetic is the same float32 operations in the
// same order, every sort is stable.  One known difference: the torch path keys masked-out rows +inf and
// sorts all n rows, so a cut-front row that holds +inf (or NaN) ties with (or sorts after) masked rows there,
// its "last valid" slot can be a masked row, and its choice among the cut front can then differ from this
// kernel's (the same caveat as nsga_select.hip's).  With ±inf or NaN the kernel still terminates, writes all
// K·S entries, and the first min(c, S) entries of a region are distinct members of it.
//
// Steps of a workgroup:
//   1. ordered compaction of the member rows into LDS (wave ballots + a prefix over the wave counts), so
//      the members sit in ascending row order: slot s, owned by thread s mod 1024;
//   2. dominator counts in registers, up to 8 owned members per thread: one pass over all member pairs,
//      the candidates' objectives staged through a 16 KB LDS tile that every lane reads at one address
//      (a broadcast), the owner's objectives in registers.  No (c, c) matrix anywhere;
//   3. peel, one front per iteration: the unranked members with count 0, appended in slot (= row) order at
//      the running offset by the same compaction; stop when the offset reaches S, else every thread
//      lowers its owned counts by the members of the new front that dominate them.  Each iteration ranks
//      at least one member, so there are at most c of them;
//   4. crowding on the cut front and the (−cd, slot) sort: evx::crowd_select.
// The compaction and the count passes of steps 2 and 3 are evoxmi_peel.h, shared with nds_batched.hip.
// The objectives are padded with zeros to MT ∈ {4, 16} per row (equal in both rows of a pair, so the
// padding never changes a comparison), which keeps the pair loop free of a loop over m.
#include "evoxmi_crowd.h"
#include "evoxmi_launchers.h"
#include "evoxmi_peel.h"

namespace {

constexpr int M2M_THREADS = evx::CROWD_THREADS;
constexpr int M2M_WAVES = M2M_THREADS / 64;
constexpr int M2M_ITEMS = evx::PEEL_ITEMS;
constexpr int M2M_MAXN = M2M_THREADS * M2M_ITEMS;  // 8192
constexpr int M2M_TILE = evx::PEEL_TILE;           // floats: 1024 candidates at MT = 4, 256 at MT = 16

struct M2MShared {
  union {
    evx::CrowdSortStorage sort;  // step 4
    float tile[M2M_TILE];        // steps 2 and 3
  } u;
  union {
    uint32_t mem[M2M_MAXN];  // member rows, ascending (steps 1-3)
    float cd[M2M_MAXN];      // crowding distance per front slot (step 4)
  };
  uint32_t srow[M2M_MAXN];  // the new front: member slots while peeling, rows for the cut front
  int wcnt[M2M_ITEMS * M2M_WAVES];
  float wave_first[M2M_WAVES], wave_last[M2M_WAVES];
  float key0, keyl;
};

template <int MT>
__global__ void __launch_bounds__(M2M_THREADS) m2m_select_kernel(const float* __restrict__ f, const void* __restrict__ region, int region64,
                                                                  const int64_t* __restrict__ rad, int n, int m, int S,
                                                                  int64_t* __restrict__ part, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ worst) {
  __shared__ M2MShared sh;
  const int t = threadIdx.x, k = blockIdx.x;
  int64_t* out = part + (int64_t)k * S;
  int pre[M2M_ITEMS];

  // 1. the members of region k, ascending
  const int nch = (n + M2M_THREADS - 1) / M2M_THREADS;
  uint32_t flags = 0;
#pragma unroll
  for (int ch = 0; ch < M2M_ITEMS; ++ch) {
    const int r = ch * M2M_THREADS + t;
    if (r < n) {
      const int64_t g = region64 ? ((const int64_t*)region)[r] : (int64_t)((const int32_t*)region)[r];
      flags |= (g == (int64_t)k ? 1u : 0u) << ch;
    }
  }
  const int c = evx::peel_compact<M2M_THREADS>(flags, nch, sh.wcnt, pre);
#pragma unroll
  for (int ch = 0; ch < M2M_ITEMS; ++ch)
    if ((flags >> ch) & 1u) sh.mem[pre[ch]] = (uint32_t)(ch * M2M_THREADS + t);
  __syncthreads();
  if (t == 0) counts[k] = c;
  if (c < S) {  // uniform: every thread leaves together
    for (int j = t; j < S; j += M2M_THREADS) out[j] = j < c ? (int64_t)sh.mem[j] : rad[j];
    if (t == 0) worst[k] = -1;
    return;
  }

  // 2. unranked-dominator counts of the owned members (slot it·1024 + t)
  const int nit = (c + M2M_THREADS - 1) / M2M_THREADS;
  int cnt[M2M_ITEMS];
  uint32_t alive = 0;
#pragma unroll
  for (int it = 0; it < M2M_ITEMS; ++it) {
    cnt[it] = 0;
    alive |= (it * M2M_THREADS + t < c ? 1u : 0u) << it;
  }
  const auto member = [&](int slot) { return (int)sh.mem[slot]; };
  evx::peel_count_pass<MT, M2M_THREADS, false>(f, m, sh.u.tile, c, nit, alive, cnt, false, member, member);

  // 3. peel
  int off = 0, rank = 0, F = 0;
  bool force = false;
  for (;;) {
    flags = 0;
#pragma unroll
    for (int it = 0; it < M2M_ITEMS; ++it) flags |= (((alive >> it) & 1u) && (cnt[it] <= 0 || force) ? 1u : 0u) << it;
    const int tot = evx::peel_compact<M2M_THREADS>(flags, nit, sh.wcnt, pre);  // its barriers also end the reads of tile and srow
    if (tot == 0) {  // cannot happen (dominance is a strict partial order); keeps the loop finite regardless
      force = true;
      continue;
    }
    if (off + tot >= S) {  // the cut front: its rows, in row order
#pragma unroll
      for (int it = 0; it < M2M_ITEMS; ++it)
        if ((flags >> it) & 1u) sh.srow[pre[it]] = sh.mem[it * M2M_THREADS + t];
      F = tot;
      break;
    }
#pragma unroll
    for (int it = 0; it < M2M_ITEMS; ++it) {
      if ((flags >> it) & 1u) {
        const int slot = it * M2M_THREADS + t;
        sh.srow[pre[it]] = (uint32_t)slot;
        out[off + pre[it]] = (int64_t)sh.mem[slot];
      }
    }
    alive &= ~flags;
    // srow is written and the tile is read no more after the pass's first barrier
    evx::peel_count_pass<MT, M2M_THREADS, true>(f, m, sh.u.tile, tot, nit, alive, cnt, true, [&](int i) { return (int)sh.mem[sh.srow[i]]; }, member);
    off += tot;
    ++rank;
  }
  if (t == 0) worst[k] = rank;
  __syncthreads();  // srow holds the cut front; mem (under cd) and the tile (under the sort storage) are dead

  // 4. the other S − off outputs: the cut front by (−cd, row)
  const int need = S - off;
  if (F <= M2M_THREADS) evx::crowd_select<1>(sh, sh.u.sort, f, m, 0, F, need, out + off);
  else if (F <= 2 * M2M_THREADS) evx::crowd_select<2>(sh, sh.u.sort, f, m, 0, F, need, out + off);
  else if (F <= 4 * M2M_THREADS) evx::crowd_select<4>(sh, sh.u.sort, f, m, 0, F, need, out + off);
  else evx::crowd_select<8>(sh, sh.u.sort, f, m, 0, F, need, out + off);
}

}  // namespace

void evx_m2m_select(const float* f, const void* region, int region64, const int64_t* rad, int n, int m, int K, int S, int64_t* part,
                    int32_t* counts, int32_t* worst, hipStream_t s) {
  if (m <= 4)
    m2m_select_kernel<4><<<K, M2M_THREADS, 0, s>>>(f, region, region64, rad, n, m, S, part, counts, worst);
  else
    m2m_select_kernel<16><<<K, M2M_THREADS, 0, s>>>(f, region, region64, rad, n, m, S, part, counts, worst);
}
