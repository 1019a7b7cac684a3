// IBEA's environmental selection on the device (evoxmi/algorithms/mo/ibea.py, evoxmi/ops/ibea.py):
// the I_ε+ fitness of the normalised objectives o (n, m) and the one-by-one removal of the worst
// row with its fitness correction.  I[i, j] = max_k(o_ik − o_jk) is never stored: both kernels
// recompute the entries they need from the m ≤ 16 objectives.
//
// A. ibea_fitness_kernel — C[j] = max_i |I[i, j]| and f[j] = 1 − Σ_i exp(−I[i, j] / C[j] / κ)
// (i = j included, as in torch).  A wave per column j, four columns per workgroup; the rows i
// pass through LDS in tiles of 256 (row stride m | 1: conflict free), row j is read from LDS
// as a broadcast.  Two sweeps over i, the max and then the sum, each recomputing I: no per-lane
// copy of a column, so one kernel serves every n.  Lane l takes i ≡ l (mod 64) in ascending
// order, then a fixed xor tree: the order does not depend on j, so duplicate rows get bit-equal
// f and every run gives the same bits.  IEEE division and the accurate expf (the terms reach
// e^20); max and abs propagate NaN as torch's amax does.
//
// B. ibea_truncate_kernel — n_remove steps of
//     x = argmin f  (all n rows, removed ones too; NaN is the minimum; lowest index on ties)
//     f[j] += exp(−I[x, j] / C[x] / κ) for every j;   f[x] = max_j f[j];   mark x, order[t] = x
// on one workgroup of T = 256, 512 or 1024 threads.  Thread r keeps the running f of the IT rows
// r, r + T, …, r + (IT − 1)·T in registers and its removal marks as bits of one register; the
// objectives arrive transposed (m, n), so a wave's loads of one objective are contiguous.  A step
// is bound by the instructions the waves of one CU issue (two IEEE divisions and an expf per
// row), so n ≤ 2048 runs on four waves, one per SIMD, with IT ∈ {1, 2, 4, 8} from n ≤ 256·IT;
// above that IT = 8 and T = 512 (n ≤ 4096) or 1024.  Measured with 1024 threads at every size,
// a step of n = 200 took 3.5 µs: sixteen waves each issued the whole step for 100 busy lanes.
// The max of step t and the arg-min of step t + 1 share one block reduction: every thread
// reduces (max over its rows, arg-min over its rows ≠ x), the arg-min as one unsigned 64-bit
// word (ordered value bits, NaN lowest, then the index), six xor shuffles make the wave's
// pair, lane 0 publishes it and lanes k ≤ m publish the wave candidate's objectives and C (the
// wave that owns x republishes row x) in LDS; after the one __syncthreads() of the step every
// thread folds the wave partials in the same order, sets f[x] = max if it owns x, and
// resolves the next x between (max, x) and the arg-min of the others.  Row x then comes out of
// LDS as a broadcast.  The LDS partials are double buffered (a buffer is rewritten two
// barriers after it was read).  The thread's own objective rows stay in registers for m = 2
// and m = 3 (IT·m ≤ 24 registers); for every other m they are re-read each step (n·m·4 ≤ 512
// KiB: L2 resident, coalesced).  Static trip counts, no atomics, no spin: bitwise
// reproducible.  After the loop ballots over each stripe of T rows and the wave counts in LDS
// give every unmarked row its place, and idx gets the first n_keep of them in ascending order
// (the stable argsort of the removal mask).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel                     VGPR  SGPR  scratch  LDS [B]
//   ibea_fitness               62    60    0        17664
//   ibea_truncate<1, m = 2>    46    70    0        2896
//   ibea_truncate<1, m = 3>    49    68    0        2896
//   ibea_truncate<1, any m>    47    77    0        2896
//   ibea_truncate<2, m = 2>    52    72    0        2960
//   ibea_truncate<2, m = 3>    56    70    0        2960
//   ibea_truncate<2, any m>    51    98    0        2960
//   ibea_truncate<4, m = 2>    63    92    0        3088
//   ibea_truncate<4, m = 3>    55    66    0        3088
//   ibea_truncate<4, any m>    63    102   0        3088
//   ibea_truncate<8, m = 2>    78    82    0        3344
//   ibea_truncate<8, m = 3>    86    82    0        3344
//   ibea_truncate<8, any m>    78    83    0        3344
// No spill: 1024 threads are four waves per SIMD, 128 VGPRs each.
#include "evoxmi_mo.h"

namespace {

constexpr int IF_WAVES = 4;  // columns j per workgroup
constexpr int IF_THREADS = 64 * IF_WAVES;
constexpr int IF_TILE = 256;  // rows i per LDS tile
constexpr int IB_MAX_M = 16;
constexpr int IB_MAX_N = 8192;
constexpr int IB_THREADS = 1024;
constexpr int IB_WAVES = IB_THREADS / 64;

using evx::nan_max;

__global__ void __launch_bounds__(IF_THREADS) ibea_fitness_kernel(const float* __restrict__ obj, int n, int m, float kappa,
                                                                   float* __restrict__ f, float* __restrict__ C) {
  __shared__ float is[IF_TILE * (IB_MAX_M + 1)];
  __shared__ float js[IF_WAVES][IB_MAX_M];
  const int64_t run = blockIdx.y;  // obj (B, n, m), f and C (B, n): the run's slices from here on
  obj += run * n * m;
  f += run * n;
  C += run * n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.x * IF_WAVES + wave;
  const int ms = m | 1;  // odd row stride
  if (lane < m) js[wave][lane] = j < n ? obj[(int64_t)j * m + lane] : 0.f;

  float c = 0.f, sum = 0.f;  // |I[j, j]| = 0 is among the terms of the max
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int i0 = 0; i0 < n; i0 += IF_TILE) {
      const int rows = min(IF_TILE, n - i0);
      __syncthreads();  // the previous tile is consumed (first pass: js is published below)
      evx::stage_tile<IF_THREADS>(is, obj, i0, rows, m, ms, tid);
      __syncthreads();
      if (j < n) {
        for (int il = lane; il < rows; il += 64) {
          const float* oi = is + il * ms;
          float mx = oi[0] - js[wave][0];
          for (int k = 1; k < m; ++k) mx = nan_max(mx, oi[k] - js[wave][k]);
          if (sweep == 0)
            c = nan_max(c, fabsf(mx));
          else
            sum += expf(-mx / c / kappa);
        }
      }
    }
    if (sweep == 0) c = evx::wave_nan_max(c);  // every lane gets the column's C (no −0 among absolute values; a NaN stays a NaN)
  }
  sum = evx::wave_sum(sum);
  if (lane == 0 && j < n) {
    C[j] = c;
    f[j] = 1.f - sum;
  }
}

struct alignas(16) IbPart {
  float mx;
  unsigned long long key;
};

constexpr unsigned long long IB_NO_KEY = ~0ull;

// torch.argmin's order on (value, index) as one unsigned word: a NaN is below every number, −0 = +0,
// the lower index first among equals
__device__ __forceinline__ unsigned long long arg_key(float v, int i) {
  return evx::key64(v == v ? evx::ord_bits(v + 0.f) : 0u, (uint32_t)i);
}

// MR > 0: m == MR and the thread's objective rows live in registers; MR == 0: any m, re-read each step.
// oT is the (m, n) transpose of the objectives; blockDim.x = 2^lg.  A workgroup per run: blockIdx.x is the run, oT (B, m, n),
// f0 and C (B, n), idx (B, n_keep), order (B, n_remove); the runs share nothing.
template <int IT, int MR>
__global__ void __launch_bounds__(IB_THREADS) ibea_truncate_kernel(const float* __restrict__ oT, const float* __restrict__ f0,
                                                                    const float* __restrict__ C, float kappa, int n, int m, int lg,
                                                                    int n_remove, int n_keep, int64_t* __restrict__ idx,
                                                                    int64_t* __restrict__ order) {
  __shared__ IbPart part[2][IB_WAVES];
  __shared__ float rows[2][IB_WAVES + 1][IB_MAX_M + 1];  // a candidate's m objectives, then its C; slot 16: row x again
  __shared__ int wsum[IT][IB_WAVES];
  const int64_t run = blockIdx.x;
  oT += run * m * n;
  f0 += run * n;
  C += run * n;
  idx += run * n_keep;
  order += run * n_remove;
  const int r = threadIdx.x, lane = r & 63, wave = r >> 6, nt = 1 << lg, nw = nt >> 6;
  constexpr int MRR = MR > 0 ? MR : 1;
  const float inf = __int_as_float(0x7f800000);

  float f[IT];
  float own[IT][MRR];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = r + (i << lg);
    f[i] = p < n ? f0[p] : 0.f;
#pragma unroll
    for (int k = 0; k < MRR; ++k) own[i][k] = (MR > 0 && p < n) ? oT[(int64_t)k * n + p] : 0.f;
  }
  uint32_t removed = 0u;  // bit i: row r + i·nt is marked

  int x = -1;                  // the row being removed; −1 before the first arg-min
  const float* xrow = nullptr;  // its objectives and C, in LDS
  for (int t = 0; t <= n_remove; ++t) {
    const int buf = t & 1;
    const bool mine = x >= 0 && (x & (nt - 1)) == r;
    if (t > 0) {
      if (r == 0) order[t - 1] = (int64_t)x;
      if (mine) removed |= 1u << (x >> lg);
      if (t == n_remove) break;  // the last removal needs no correction
      // f[j] += exp(−I[x, j] / C[x] / κ), I[x, j] = max_k(o_xk − o_jk)
      const float cx = xrow[m];
      float mx[IT];
      if (MR > 0) {
#pragma unroll
        for (int k = 0; k < MRR; ++k) {
          const float ox = xrow[k];
#pragma unroll
          for (int i = 0; i < IT; ++i) mx[i] = k == 0 ? ox - own[i][0] : nan_max(mx[i], ox - own[i][k]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < IT; ++i) mx[i] = 0.f;
        for (int k = 0; k < m; ++k) {
          const float ox = xrow[k];
          const float* ok = oT + (int64_t)k * n;
#pragma unroll
          for (int i = 0; i < IT; ++i) {
            const int p = r + (i << lg);
            const float d = ox - (p < n ? ok[p] : 0.f);
            mx[i] = k == 0 ? d : nan_max(mx[i], d);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < IT; ++i) f[i] += expf(-mx[i] / cx / kappa);
    } else if (n_remove == 0) {
      break;
    }
    // one reduction: the max over all rows (step t's f[x]) and the arg-min over the rows ≠ x
    float pm = -inf;
    unsigned long long pk = IB_NO_KEY;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int p = r + (i << lg);
      if (p < n) {
        pm = nan_max(pm, f[i]);
        const unsigned long long key = arg_key(f[i], p);
        if (p != x && key < pk) pk = key;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(pm, o, 64);
      const unsigned long long ok = __shfl_xor(pk, o, 64);
      pm = nan_max(pm, om);
      pk = ok < pk ? ok : pk;
    }
    if (lane == 0) part[buf][wave] = IbPart{pm, pk};
    const uint32_t pa = (uint32_t)pk;  // the wave's candidate row (all lanes agree: the keys are distinct)
    if (lane <= m && pa < (uint32_t)n) rows[buf][wave][lane] = lane < m ? oT[(int64_t)lane * n + pa] : C[pa];
    if (x >= 0 && wave == ((x & (nt - 1)) >> 6) && lane <= m) rows[buf][IB_WAVES][lane] = xrow[lane];
    __syncthreads();
    float M = -inf;
    unsigned long long key = IB_NO_KEY;
    for (int w = 0; w < nw; ++w) {
      const IbPart q = part[buf][w];
      M = nan_max(M, q.mx);
      key = q.key < key ? q.key : key;
    }
    int slot = (int)(((uint32_t)key & (uint32_t)(nt - 1)) >> 6);
    if (x >= 0) {
#pragma unroll
      for (int i = 0; i < IT; ++i)
        if (mine && (x >> lg) == i) f[i] = M;
      const unsigned long long kx = arg_key(M, x);
      if (kx < key) {  // x again: every other row is no smaller (or x is the first NaN)
        key = kx;
        slot = IB_WAVES;
      }
    }
    x = (int)(uint32_t)key;
    xrow = rows[buf][slot];
  }

  // idx: the unmarked rows in ascending order (stripe i before stripe i + 1), the first n_keep of them
  int pre[IT];
  bool live[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    live[i] = r + (i << lg) < n && !((removed >> i) & 1u);
    const unsigned long long b = __ballot(live[i]);
    pre[i] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[i][wave] = __popcll(b);
  }
  __syncthreads();
  int pos = 0;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    int before = 0, total = 0;
    for (int w = 0; w < nw; ++w) {
      const int c = wsum[i][w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int q = pos + before + pre[i];
    if (live[i] && q < n_keep) idx[q] = (int64_t)(r + (i << lg));
    pos += total;
  }
}

template <int IT>
void launch_truncate(int lg, int B, const float* oT, const float* f, const float* C, float kappa, int n, int m, int n_remove, int n_keep,
                     int64_t* idx, int64_t* order, hipStream_t s) {
  if (m == 2)
    ibea_truncate_kernel<IT, 2><<<B, 1 << lg, 0, s>>>(oT, f, C, kappa, n, m, lg, n_remove, n_keep, idx, order);
  else if (m == 3)
    ibea_truncate_kernel<IT, 3><<<B, 1 << lg, 0, s>>>(oT, f, C, kappa, n, m, lg, n_remove, n_keep, idx, order);
  else
    ibea_truncate_kernel<IT, 0><<<B, 1 << lg, 0, s>>>(oT, f, C, kappa, n, m, lg, n_remove, n_keep, idx, order);
}

}  // namespace

int evx_ibea_max_n() { return IB_MAX_N; }
int evx_ibea_max_m() { return IB_MAX_M; }

void evx_ibea_fitness(const float* obj, int B, int n, int m, float kappa, float* f, float* C, hipStream_t s) {
  if (n <= 0 || B < 1 || B > EVX_MAX_RUNS) return;
  ibea_fitness_kernel<<<dim3((n + IF_WAVES - 1) / IF_WAVES, B), IF_THREADS, 0, s>>>(obj, n, m, kappa, f, C);
}

void evx_ibea_truncate(const float* oT, const float* f, const float* C, float kappa, int B, int n, int m, int n_remove, int n_keep,
                       int64_t* idx, int64_t* order, hipStream_t s) {
  if (n <= 0 || n > IB_MAX_N || m < 1 || m > IB_MAX_M || B < 1 || B > EVX_MAX_RUNS) return;
  // four waves (one per SIMD) while eight rows per thread suffice, then more waves
  if (n <= 256)
    launch_truncate<1>(8, B, oT, f, C, kappa, n, m, n_remove, n_keep, idx, order, s);
  else if (n <= 512)
    launch_truncate<2>(8, B, oT, f, C, kappa, n, m, n_remove, n_keep, idx, order, s);
  else if (n <= 1024)
    launch_truncate<4>(8, B, oT, f, C, kappa, n, m, n_remove, n_keep, idx, order, s);
  else
    launch_truncate<8>(n <= 2048 ? 8 : n <= 4096 ? 9 : 10, B, oT, f, C, kappa, n, m, n_remove, n_keep, idx, order, s);
}
