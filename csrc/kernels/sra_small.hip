// SRA's environmental selection for B independent runs in ONE launch: a workgroup of 1024 threads per run (blockIdx.x = run)
// forms both indicators and ranks the rows, and I1 and I2 never pass through global memory between the two phases.  What one run
// costs in sra_select.hip is two launches, the second on a single compute unit; the bubble sort's T ≈ 2n steps depend on each
// other, so the only way to fill the chip is a run per compute unit.  The arithmetic, the item and the step window are
// evoxmi_sra.h's; this file has no FILE_FLAGS entry, like sra_select.hip, so a run's I1 and I2 are the solo kernel's bit for bit.
//
// A. Indicators.  The run's n rows are staged into LDS once (row stride m | 1).  The 16 waves stride over the rows p; lane l of
// a row's wave sums q ≡ l (mod 64) in ascending q, then the fixed xor tree: the order of sra_indicators_kernel, whose 256-row
// tiles are a multiple of 64.  Lane 0 writes the item (I1, I2, p) into an LDS item array, and I1 and I2 to global memory for the
// caller; the ranking reads the items, not those words.                                                     one barrier
//
// B. Ranking, the comparator schedule of sra_rank_kernel (evoxmi_sra.h: sr_lag, sr_steps, sr_lo, sr_hi): ⌈n/2⌉ threads rounded up
// to whole waves hold two items each, the other waves leave after the barrier.  An even step stays inside a thread; an odd step
// passes the edges through double-buffered LDS with one barrier per two steps, and both owners of an edge evaluate the same compare
// on the same two items.  The edge buffers alias the objective rows, which are dead after phase A.  At n = 200–400 the barrier
// spans two to four waves instead of the solo kernel's sixteen.
// Static trip counts, no atomics, no spin: bitwise reproducible.
//
// A one-wave variant for n ≤ 512 (2, 4 or 8 items per lane, edges by __shfl_up / __shfl_down, no barrier in the loop) was built
// and measured on an MI355X: 362 µs at (B 32, n 512, m 3) against 300 µs for this scheme at n = 514, the single wave being bound
// by the latency of its dependent compare chain and cross-lane moves.  It was deleted (profiles/NOTES.md).
//
// Caps per run: n ≤ 2048 at m ≤ 8, n ≤ 1024 at m ≤ 16.  Dynamic LDS = max(n · (m | 1) · 4, the edge buffers' 49152) + 12 n bytes:
// 98304 at (2048, 8), 81920 at (1024, 16), 51552 at (200, 3), of the CU's 160 KiB.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel             VGPR  SGPR  scratch  static LDS [B]
//   sra_small_select   51    51    0        0
// No spill; phase A sets the register count.
#include "evoxmi_sra.h"

namespace {

using evx::SrItem;
using evx::sr_cswap;

constexpr int SS_THREADS = 1024;
constexpr int SS_WAVES = SS_THREADS / 64;

struct SsEdges {
  SrItem first[SS_THREADS], last[SS_THREADS];
};

__global__ void __launch_bounds__(SS_THREADS) sra_small_select_kernel(const float* __restrict__ obj, const float* __restrict__ u, int u_stride,
                                                                      const float* __restrict__ pc_runs, int n, int m, int rows_bytes,
                                                                      int64_t* __restrict__ idx, float* __restrict__ I1, float* __restrict__ I2) {
  constexpr int IT = 2;  // items per thread: even, so an even step stays inside a thread
  extern __shared__ __align__(16) unsigned char ss_lds[];
  float* rows = reinterpret_cast<float*>(ss_lds);                    // [n][m | 1]; the edge buffers after phase A
  SrItem* items = reinterpret_cast<SrItem*>(ss_lds + rows_bytes);    // [n]
  const int run = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  obj += (size_t)run * n * m;
  u += (size_t)run * u_stride;
  idx += (size_t)run * n;
  I1 += (size_t)run * n;
  I2 += (size_t)run * n;
  const float pc = pc_runs[run];
  const int ms = m | 1;  // odd row stride

  // A. indicators
  evx::stage_tile<SS_THREADS>(rows, obj, 0, n, m, ms, tid);
  __syncthreads();
  for (int p = wave; p < n; p += SS_WAVES) {
    const float* op = rows + p * ms;  // a broadcast read
    float sum = 0.f, mn = __int_as_float(0x7f800000);
    for (int q = lane; q < n; q += 64) {
      const float* oq = rows + q * ms;
      EVX_SI_PAIR(oq, op, m, q != p, sum, mn)
    }
    EVX_SI_TREE(sum, mn)
    if (lane == 0) {
      const SrItem item = {1.f - sum, sqrtf(mn), p};
      items[p] = item;
      I1[p] = item.a;
      I2[p] = item.b;
    }
  }
  __syncthreads();  // the items are complete, the rows are dead

  // B. ranking: thread r holds the positions [r·IT, (r+1)·IT)
  const int r = tid, base = r * IT;
  if (base >= ((n + 127) & ~127)) return;  // whole waves leave; none of them owns a row
  SrItem it[IT];
  uint32_t sel = 0u;  // bit i: position base + i compares by I1
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = base + i;
    if (p < n) {
      it[i] = items[p];
    } else {
      it[i].a = 0.f;
      it[i].b = 0.f;
      it[i].id = p;
    }
    if (p < n - 1 && u[p] < pc) sel |= 1u << i;
  }
  const bool sel_left = r > 0 && base - 1 < n - 1 && u[base - 1] < pc;  // the selector of position base − 1

  const int lag = evx::sr_lag(n), T = evx::sr_steps(n, lag);
  SsEdges* edges = reinterpret_cast<SsEdges*>(ss_lds);  // two buffers
  for (int t = 0; t < T; t += 2) {
    // even step t: comparators at even positions, all inside the thread
    {
      const int lo = evx::sr_lo(t, lag), hi = evx::sr_hi(t, n);
#pragma unroll
      for (int i = 0; i < IT; i += 2) {
        const int j = base + i;
        sr_cswap(j >= lo && j <= hi, (sel >> i) & 1u, it[i], it[i + 1]);
      }
    }
    if (t + 1 >= T) break;  // uniform over the block
    // odd step t + 1: the comparators at odd positions are the two at the thread's edges
    {
      const int lo = evx::sr_lo(t + 1, lag), hi = evx::sr_hi(t + 1, n);
      const int jl = base - 1, jr = base + IT - 1;
      const bool left = r > 0 && jl >= lo && jl <= hi, right = r + 1 < SS_THREADS && jr >= lo && jr <= hi;
      SrItem x, y;  // the left neighbour's last item, the right neighbour's first
      SsEdges& e = edges[(t >> 1) & 1];   // rewritten two barriers after it was read
      if (left) e.first[r] = it[0];       // read by thread r − 1, whose right edge is this position
      if (right) e.last[r] = it[IT - 1];  // read by thread r + 1
      __syncthreads();
      if (left) x = e.last[r - 1];
      if (right) y = e.first[r + 1];
      if (left) sr_cswap(true, sel_left, x, it[0]);
      if (right) sr_cswap(true, (sel >> (IT - 1)) & 1u, it[IT - 1], y);
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i)
    if (base + i < n) idx[base + i] = (int64_t)it[i].id;
}

}  // namespace

bool evx_sra_small_ok(int64_t n, int64_t m) { return n >= 1 && m >= 1 && ((m <= 8 && n <= 2048) || (m <= 16 && n <= 1024)); }

void evx_sra_small_select(const float* obj, const float* u, int u_stride, const float* pc, int B, int n, int m, int64_t* idx, float* I1,
                          float* I2, hipStream_t s) {
  if (B <= 0) return;
  size_t rows_bytes = (size_t)n * (m | 1) * sizeof(float);
  if (rows_bytes < 2 * sizeof(SsEdges)) rows_bytes = 2 * sizeof(SsEdges);
  rows_bytes = (rows_bytes + 15) & ~(size_t)15;
  const size_t lds = rows_bytes + (size_t)n * sizeof(SrItem);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)sra_small_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  sra_small_select_kernel<<<B, SS_THREADS, lds, s>>>(obj, u, u_stride, pc, n, m, (int)rows_bytes, idx, I1, I2);
}
