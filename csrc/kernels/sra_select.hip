// SRA's environmental selection on the device (evoxmi/algorithms/mo/sra.py, evoxmi/ops/sra.py):
// the stochastic ranking of csrc/host/stochastic_ranking.h (the oracle) and the two indicators
// it balances.
//
// A. sra_rank_kernel — stochastic ranking.  The host op runs S = ⌈n/2⌉ bubble sweeps over the
// positions j = 0 … n−2, position j comparing by I1 when u[j] < pc and by I2 otherwise, and
// swapping when key[rank[j]] < key[rank[j+1]] (float compares: NaN never swaps).  Sweep s may
// compare position j as soon as sweep s−1 has passed position j+1, so sweep s runs position j
// in time step t = j + 2s and the sort is T = (n−1) + 2(S−1) steps; in step t the comparators
// sit at j ≡ t (mod 2), max(0, t − 2(S−1)) ≤ j ≤ min(t, n−2), and are disjoint.  The host's
// early exit needs nothing: every sweep uses the same u, so a sweep without a swap leaves a
// state that no later sweep changes.
//
// One workgroup of 1024 threads; thread r holds the IT items (I1, I2, index) at positions
// [r·IT, (r+1)·IT) in registers, IT ∈ {2, 4, 8} from n ≤ 1024·IT ≤ 8192, and its IT selector
// bits.  IT is even, so an even step's comparators lie inside one thread: no LDS, no barrier.
// An odd step has IT/2 − 1 inner comparators and the two at the thread's edges: each thread
// publishes its first and last item in LDS, one __syncthreads(), and both owners of an edge
// evaluate the same compare on the same two items.  The LDS exchange is double buffered (a
// buffer is rewritten two barriers after it was read), so the sort costs one barrier per
// two steps.  Static trip bounds, no atomics, no spin: bitwise reproducible.
//
// B. sra_indicators_kernel — both indicators of row p in one pass over q, from the same
// differences o_q − o_p, with no n × n × m temporary:
//   I1[p] = 1 − Σ_q exp(−(max_k(o_qk − o_pk)) / 0.05)        (q = p included, as in torch)
//   I2[p] = min_{q≠p} sqrt(Σ_k max(o_qk − o_pk, 0)²)
// A wave per row p, four rows per workgroup; the q rows pass through LDS in tiles of 256
// (row stride m | 1: conflict free), row p is read from LDS as a broadcast.  Lane l sums
// q ≡ l (mod 64) in ascending order, then a fixed xor tree: the same bits in every run.
// Division, expf and sqrtf are the accurate ones (the terms reach e^20); max and min
// propagate NaN as torch's amax / clamp / min do.  m ≤ SRA_MAX_M = 16.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel             VGPR  SGPR  scratch  LDS [B]
//   sra_rank<2>        15    34    0        49152
//   sra_rank<4>        25    44    0        49152
//   sra_rank<8>        45    62    0        49152
//   sra_indicators     62    58    0        17664
// No spill; the ranking's LDS is the two edge buffers (2 × 2 × 1024 items of 12 B) of the CU's
// 160 KiB.
#include "evoxmi_mo.h"

namespace {

constexpr int SR_THREADS = 1024;
constexpr int SR_MAX = 8192;  // cap on n

struct SrItem {
  float a, b;
  int id;
};

struct SrEdges {
  SrItem first[SR_THREADS], last[SR_THREADS];
};

__device__ __forceinline__ void sr_cswap(bool active, bool by_a, SrItem& x, SrItem& y) {
  const float kx = by_a ? x.a : x.b, ky = by_a ? y.a : y.b;
  if (active && kx < ky) {
    const SrItem t = x;
    x = y;
    y = t;
  }
}

template <int IT>
__global__ void __launch_bounds__(SR_THREADS) sra_rank_kernel(const float* __restrict__ I1, const float* __restrict__ I2,
                                                               const float* __restrict__ u, const float* __restrict__ pc_word, int n,
                                                               int64_t* __restrict__ rank) {
  static_assert(IT >= 2 && IT % 2 == 0, "an even step must stay inside a thread");
  __shared__ SrEdges edges[2];
  const int r = threadIdx.x, base = r * IT;
  const float pc = *pc_word;

  SrItem it[IT];
  uint32_t sel = 0u;  // bit i: position base + i compares by I1
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = base + i;
    it[i].a = p < n ? I1[p] : 0.f;
    it[i].b = p < n ? I2[p] : 0.f;
    it[i].id = p;
    if (p < n - 1 && u[p] < pc) sel |= 1u << i;
  }
  const bool sel_left = r > 0 && base - 1 < n - 1 && u[base - 1] < pc;  // the selector of position base − 1

  const int S = (n + 1) / 2;
  const int T = (n - 1) + 2 * (S - 1);  // n = 1: 0 steps
  // positions this thread takes part in: base − 1 (left edge) … base + IT − 1 (right edge)
  for (int t = 0; t < T; t += 2) {
    // even step t: comparators at even positions, all inside the thread
    {
      const int lo = max(0, t - 2 * (S - 1)), hi = min(t, n - 2);
#pragma unroll
      for (int i = 0; i < IT; i += 2) {
        const int j = base + i;
        sr_cswap(j >= lo && j <= hi, (sel >> i) & 1u, it[i], it[i + 1]);
      }
    }
    if (t + 1 >= T) break;  // uniform over the block
    // odd step t + 1: inner comparators at odd positions, and the two edges through LDS
    {
      const int lo = max(0, t + 1 - 2 * (S - 1)), hi = min(t + 1, n - 2);
      SrEdges& e = edges[(t >> 1) & 1];
      const int jl = base - 1, jr = base + IT - 1;
      const bool left = r > 0 && jl >= lo && jl <= hi, right = r + 1 < SR_THREADS && jr >= lo && jr <= hi;
      if (left) e.first[r] = it[0];       // read by thread r − 1, whose right edge is this position
      if (right) e.last[r] = it[IT - 1];  // read by thread r + 1
#pragma unroll
      for (int i = 1; i + 1 < IT; i += 2) {
        const int j = base + i;
        sr_cswap(j >= lo && j <= hi, (sel >> i) & 1u, it[i], it[i + 1]);
      }
      __syncthreads();
      // left edge: the left neighbour's last item against my first
      if (left) {
        SrItem x = e.last[r - 1];
        sr_cswap(true, sel_left, x, it[0]);
      }
      // right edge: my last item against the right neighbour's first
      if (right) {
        SrItem y = e.first[r + 1];
        sr_cswap(true, (sel >> (IT - 1)) & 1u, it[IT - 1], y);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < IT; ++i)
    if (base + i < n) rank[base + i] = (int64_t)it[i].id;
}

constexpr int SI_WAVES = 4;           // rows p per workgroup
constexpr int SI_THREADS = 64 * SI_WAVES;
constexpr int SI_TILE = 256;          // rows q per LDS tile
constexpr int SI_MAX_M = 16;

using evx::nan_max;
using evx::nan_min;

__global__ void __launch_bounds__(SI_THREADS) sra_indicators_kernel(const float* __restrict__ obj, int n, int m, float* __restrict__ I1,
                                                                     float* __restrict__ I2) {
  __shared__ float qs[SI_TILE * (SI_MAX_M + 1)];
  __shared__ float ps[SI_WAVES][SI_MAX_M];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = blockIdx.x * SI_WAVES + wave;
  const int ms = m | 1;  // odd row stride
  if (lane < m) ps[wave][lane] = p < n ? obj[(int64_t)p * m + lane] : 0.f;

  float sum = 0.f, mn = __int_as_float(0x7f800000);
  for (int q0 = 0; q0 < n; q0 += SI_TILE) {
    const int rows = min(SI_TILE, n - q0);
    __syncthreads();  // the previous tile is consumed (first pass: ps is published below)
    evx::stage_tile<SI_THREADS>(qs, obj, q0, rows, m, ms, tid);
    __syncthreads();
    if (p < n) {
      for (int ql = lane; ql < rows; ql += 64) {
        const float* oq = qs + ql * ms;
        float mx = oq[0] - ps[wave][0];
        float c = mx < 0.f ? 0.f : mx;
        float d2 = c * c;
        for (int k = 1; k < m; ++k) {
          const float d = oq[k] - ps[wave][k];
          mx = nan_max(mx, d);
          c = d < 0.f ? 0.f : d;
          d2 += c * c;
        }
        sum += expf(-mx / 0.05f);
        if (q0 + ql != p) mn = nan_min(mn, d2);  // sqrtf is monotone and keeps NaN: the root is taken once, below
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // sum and min in one tree: as evx::wave_sum and wave_nan_min the code length changes (3516 to 3488 B)
    sum += __shfl_xor(sum, o, 64);
    mn = nan_min(mn, __shfl_xor(mn, o, 64));
  }
  if (lane == 0 && p < n) {
    I1[p] = 1.f - sum;
    I2[p] = sqrtf(mn);
  }
}

}  // namespace

int evx_sra_rank_max_n() { return SR_MAX; }
int evx_sra_indicators_max_m() { return SI_MAX_M; }

void evx_sra_rank(const float* I1, const float* I2, const float* u, const float* pc, int n, int64_t* rank, hipStream_t s) {
  if (n <= 0) return;
  if (n <= 2 * SR_THREADS)
    sra_rank_kernel<2><<<1, SR_THREADS, 0, s>>>(I1, I2, u, pc, n, rank);
  else if (n <= 4 * SR_THREADS)
    sra_rank_kernel<4><<<1, SR_THREADS, 0, s>>>(I1, I2, u, pc, n, rank);
  else
    sra_rank_kernel<8><<<1, SR_THREADS, 0, s>>>(I1, I2, u, pc, n, rank);
}

void evx_sra_indicators(const float* obj, int n, int m, float* I1, float* I2, hipStream_t s) {
  if (n <= 0) return;
  sra_indicators_kernel<<<(n + SI_WAVES - 1) / SI_WAVES, SI_THREADS, 0, s>>>(obj, n, m, I1, I2);
}
