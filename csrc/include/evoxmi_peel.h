// Front peeling by dominator counts inside one workgroup (shared by m2m_select.hip and nds_batched.hip).
//
// A workgroup of THREADS threads owns up to PEEL_ITEMS·THREADS rows: slot it·THREADS + t belongs to thread t,
// bit `it` of a per-thread word says whether the slot is still unranked, and cnt[it] holds the number of
// unranked rows that dominate it (minimisation: a dominates b when a ≤ b in every objective and a < b in one;
// equal rows and rows with a NaN dominate nothing).  The counts live in registers.  They come from one pass
// over all row pairs and are lowered, front by front, by the rows of the new front that dominate the slot:
// peel_count_pass does both, with the candidates' objectives staged through a 16 KB LDS tile that every lane
// reads at one address (a broadcast) and the owner's objectives in registers.  No (n, n) matrix anywhere.
// peel_compact is the ordered compaction that lays a front out in slot order.
// The objectives are padded with zeros to MT per row (equal in both rows of a pair, so the padding never
// changes a comparison), which keeps the pair loop free of a loop over m.
#pragma once
#include "evoxmi_common.h"

namespace evx {

constexpr int PEEL_ITEMS = 8;
constexpr int PEEL_TILE = 4096;  // floats: 1024 candidates at MT = 4, 512 at MT = 8, 256 at MT = 16

// Ordered compaction of up to 8 flags per thread, flag `ch` (bit ch of `flags`) standing for element
// ch·THREADS + t: pre[ch] becomes the number of flagged elements before it, the return value their total.
// wcnt holds PEEL_ITEMS · THREADS / 64 words of LDS.
template <int THREADS>
__device__ __forceinline__ int peel_compact(uint32_t flags, int nch, int* wcnt, int (&pre)[PEEL_ITEMS]) {
  constexpr int WAVES = THREADS / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int ch = 0; ch < PEEL_ITEMS; ++ch) {
    pre[ch] = 0;
    if (ch < nch) {
      const unsigned long long b = __ballot((flags >> ch) & 1u);
      pre[ch] = __popcll(b & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[ch * WAVES + wave] = __popcll(b);
    }
  }
  __syncthreads();
  int tot = 0;
  for (int j = 0; j < nch * WAVES; ++j) {
    const int v = wcnt[j];
#pragma unroll
    for (int ch = 0; ch < PEEL_ITEMS; ++ch) pre[ch] += j < ch * WAVES + wave ? v : 0;
    tot += v;
  }
  __syncthreads();  // wcnt is free again
  return tot;
}

template <int MT>
__device__ __forceinline__ void peel_load_row(const float* __restrict__ f, int row, int m, float (&x)[MT]) {
#pragma unroll
  for (int o = 0; o < MT; ++o) x[o] = o < m ? f[(int64_t)row * m + o] : 0.f;
}

// the number of the tile's first `tl` rows that dominate `own`
template <int MT>
__device__ __forceinline__ int peel_count_dominators(const float* tile, int tl, const float (&own)[MT]) {
  int cnt = 0;
  for (int i = 0; i < tl; ++i) {
    bool le = true, lt = false;  // the test of evx::dominates (evoxmi_mo.h), written out: with the helper m2m_select grows by 24 bytes
#pragma unroll
    for (int o = 0; o < MT; ++o) {
      const float a = tile[i * MT + o];
      le = le && a <= own[o];
      lt = lt || a < own[o];
    }
    cnt += (le && lt) ? 1 : 0;
  }
  return cnt;
}

// For every owned slot whose bit of `alive` is set, cnt[it] += (SUB: −=) the number of the `ncand` candidates
// that dominate it.  cand(i) is the row of f of candidate i < ncand, own(slot) that of a slot; nit is the number
// of owned slots per thread in use.  `tile` is PEEL_TILE floats of LDS; with sync_first the pass begins with a
// barrier (the tile, or what cand reads, was touched by other threads just before).
template <int MT, int THREADS, bool SUB, class Cand, class Own>
__device__ __forceinline__ void peel_count_pass(const float* __restrict__ f, int m, float* tile, int ncand, int nit, uint32_t alive,
                                                int (&cnt)[PEEL_ITEMS], bool sync_first, Cand cand, Own own) {
  constexpr int TL = PEEL_TILE / MT;
  const int t = threadIdx.x;
  for (int tb = 0; tb < ncand; tb += TL) {
    const int tl = min(TL, ncand - tb);
    if (tb || sync_first) __syncthreads();  // the tile is read no more
    for (int e = t; e < PEEL_TILE; e += THREADS) {
      const int i = e / MT, o = e % MT;
      tile[e] = (i < tl && o < m) ? f[(int64_t)cand(tb + i) * m + o] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < nit; ++it) {
      int d = 0;
      if ((alive >> it) & 1u) {
        float x[MT];
        peel_load_row<MT>(f, own(it * THREADS + t), m, x);
        d = peel_count_dominators<MT>(tile, tl, x);
      }
      if (SUB) d = -d;
#pragma unroll
      for (int j = 0; j < PEEL_ITEMS; ++j) cnt[j] += j == it ? d : 0;  // cnt stays in registers
    }
  }
}

}  // namespace evx
