// SPEA2's fitness and truncation on the device (evoxmi/algorithms/mo/spea2.py, evoxmi/ops/spea2.py).
// No (n, n) distance or dominance matrix is stored: every kernel recomputes the entries it needs
// from the m ≤ 16 objectives.
//
// d2(i, j) = Σ_k fmaf(δ_k, δ_k, ·), δ_k = o_ik − o_jk, k ascending from 0.f, is the one squared distance
// of the file: bitwise symmetric (δ only changes sign) and bitwise equal at every call site (explicit
// fmaf; trailing zero-padded objectives add fmaf(0, 0, acc) = acc).  A NaN d2 is +inf: not a neighbour.
//
// A. Fitness, a wave per row, four rows per workgroup, the other rows through LDS in tiles of 256
// (row stride m | 1), lane l takes the rows ≡ l (mod 64) in ascending order, then a fixed xor tree:
// the order does not depend on the row, duplicate rows get bit-equal results.
//   spea2_fit1_kernel: S[i] = #{j : i dominates j} (evx::dominates), nd[i] = no
//     row dominates i, msk[i] = nd[i] and no NaN objective, D[i] = 1 / (sqrt(second smallest d2(i, j),
//     j ≠ i, with multiplicity) + 2) with IEEE sqrt and division; D = NaN for a row with a NaN objective.
//   spea2_fit2_kernel: R[j] = Σ_{i dominates j} S[i] in 32-bit integers (n ≤ 32768: below 2^30),
//     converted once; sig = D + R; for the rows of msk the nearest neighbour among the other rows of
//     msk, (nn_d2, nn_idx), the highest index among equal d2, (+inf, −1) where no d2 is finite.  With
//     S == nullptr only the neighbour pass runs (a mask given by the caller).
//
// B. spea2_truncate_kernel — one workgroup of T = 256 or 512 threads, n ≤ 8192.  k = max(0, #mask − n_keep)
// is counted on the device; k times the live masked row of least (nn_d2, index) leaves (all +inf: the
// lowest index).  Thread r keeps nn_d2, nn_idx and the live bits of the IT rows r, r + T, … in
// registers.  Removing x invalidates only the rows whose stored neighbour is x (1.6 to 2 rows per
// removal on random inputs): the waves compact them into LDS lists and they rescan the live rows, up
// to B = 4 (M ≤ 4, IT ≤ 8) or 2 of them per pass, one barrier per pass.  A pass is instantiated for
// every target count 1 … B, so a thread computes d2 of its rows against the targets that exist and
// nothing else; the list lookups and the folds of the wave partials are wave-uniform and run on the
// scalar unit (readfirstlane).  Six xor shuffles and the wave partials in LDS make each target's new
// neighbour, again the highest index among equals.  Because removal takes the lowest index among
// equals and every row of a group of duplicates stores the highest one, removing a duplicate triggers
// no rescan.  The arg-min over the rows that are not rescanned travels with the flag phase's barrier
// and the rescanned rows' new keys are folded in after their pass: a step costs 1 + ⌈rescans / B⌉
// barriers.  A step is bound by the instructions the waves of one CU issue, most of them per-wave
// overhead (lists, folds, reductions), so few waves with many rows each win: four waves with IT ∈ {1, 2,
// 4, 8} up to n = 2048, eight waves with IT = 8 (n ≤ 4096) or 16 above; sixteen waves of 8 rows took
// twice as long per step at n = 8192.  The objectives arrive transposed and zero padded to M ∈ {2, 3,
// 4, 8, 16} rows, (M, n): compile-time trip counts; for M ≤ 3 the thread's rows stay in registers,
// above they are re-read each pass (L2 resident, coalesced, 64 loads in flight per thread).  Static
// trip counts apart from k and the rescan count, no atomics, no spin: bitwise reproducible.  LDS
// partials are double buffered (a buffer is rewritten two barriers after it was read).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel <IT, M, T>              VGPR  SGPR  scratch  LDS [B]
//   spea2_fit1                     63    106   0        17664
//   spea2_fit2                     31    86    0        18944
//   spea2_truncate<1, 2, 256>      62    69    0        17184
//   spea2_truncate<1, 3, 256>      64    73    0        17184
//   spea2_truncate<1, 4, 256>      66    83    0        17184
//   spea2_truncate<1, 8, 256>      58    84    0        16928
//   spea2_truncate<1, 16, 256>     96    100   0        16928
//   spea2_truncate<2, 2, 256>      66    75    0        17184
//   spea2_truncate<2, 3, 256>      62    77    0        17184
//   spea2_truncate<2, 4, 256>      65    89    0        17184
//   spea2_truncate<2, 8, 256>      72    90    0        16928
//   spea2_truncate<2, 16, 256>     132   106   0        16928
//   spea2_truncate<4, 2, 256>      80    83    0        17184
//   spea2_truncate<4, 3, 256>      95    86    0        17184
//   spea2_truncate<4, 4, 256>      73    101   0        17184
//   spea2_truncate<4, 8, 256>      88    102   0        16928
//   spea2_truncate<4, 16, 256>     160   106   0        16928
//   spea2_truncate<8, 2, 256>      122   101   0        17184
//   spea2_truncate<8, 3, 256>      158   106   0        17184
//   spea2_truncate<8, 4, 256>      127   106   0        17184
//   spea2_truncate<8, 8, 256>      244   106   0        16928
//   spea2_truncate<8, 16, 256>     173   106   0        16928
//   spea2_truncate<8, 2, 512>      155   106   0        17184
//   spea2_truncate<8, 3, 512>      158   106   0        17184
//   spea2_truncate<8, 4, 512>      169   106   0        17184
//   spea2_truncate<8, 8, 512>      216   106   0        16928
//   spea2_truncate<8, 16, 512>     173   106   0        16928
//   spea2_truncate<16, 2, 512>     221   106   0        16928
//   spea2_truncate<16, 3, 512>     253   106   0        16928
//   spea2_truncate<16, 4, 512>     129   100   0        16928
//   spea2_truncate<16, 8, 512>     170   106   0        16928
//   spea2_truncate<16, 16, 512>    196   106   0        16928
// 256 threads are one wave per SIMD, 512 threads two (256 VGPRs each): no spill.
#include "evoxmi_mo.h"

namespace {

constexpr int SF_WAVES = 4;  // rows per workgroup
constexpr int SF_THREADS = 64 * SF_WAVES;
constexpr int SF_TILE = 256;  // rows per LDS tile
constexpr int SP_MAX_M = 16;
constexpr int SP_MAX_N = 8192;       // truncation: one workgroup
constexpr int SP_FIT_MAX_N = 32768;  // fitness: R in 32 bits
constexpr int SP_THREADS = 512;      // truncation: at most
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr uint32_t SP_INF = 0x7f800000u;
constexpr unsigned long long SP_NO_KEY = ~0ull;

// the squared distance of the whole file; a(k), b(k) give the k-th objective of the two rows
template <class FA, class FB>
__device__ __forceinline__ float d2(FA a, FB b, int m) {
  float acc = 0.f;
  for (int k = 0; k < m; ++k) {
    const float d = a(k) - b(k);
    acc = fmaf(d, d, acc);
  }
  return acc == acc ? acc : __uint_as_float(SP_INF);
}

// (d2, row) as one word whose minimum is the least d2 and, among equals, the highest row (d2 ≥ +0: its bits are ordered)
__device__ __forceinline__ unsigned long long nn_key(float d, int row) { return evx::key64(__float_as_uint(d), (uint32_t)~row); }
// (nn_d2, row): least nn_d2, lowest row among equals
__device__ __forceinline__ unsigned long long arg_key(float d, int row) { return evx::key64(__float_as_uint(d), (uint32_t)row); }

__global__ void __launch_bounds__(SF_THREADS) spea2_fit1_kernel(const float* __restrict__ obj, int n, int m, int32_t* __restrict__ S,
                                                                 uint8_t* __restrict__ nd, uint8_t* __restrict__ msk,
                                                                 float* __restrict__ D) {
  __shared__ float is[SF_TILE * (SP_MAX_M + 1)];
  __shared__ float js[SF_WAVES][SP_MAX_M];
  const int64_t run = blockIdx.y;  // obj (B, n, m), the outputs (B, n): the run's slices from here on
  obj += run * n * m;
  S += run * n;
  nd += run * n;
  msk += run * n;
  D += run * n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x * SF_WAVES + wave;
  const int ms = m | 1;
  const float inf = __uint_as_float(SP_INF);
  const float mine = (lane < m && r < n) ? obj[(int64_t)r * m + lane] : 0.f;
  if (lane < m) js[wave][lane] = mine;
  const bool nanrow = __ballot(mine != mine) != 0ull;
  const float* orow = js[wave];

  int s = 0;
  bool dominated = false;
  float a = inf, b = inf;  // the lane's two smallest d2, a ≤ b
  for (int j0 = 0; j0 < n; j0 += SF_TILE) {
    const int rows = min(SF_TILE, n - j0);
    __syncthreads();  // the previous tile is consumed (first pass: js is published below)
    evx::stage_tile<SF_THREADS>(is, obj, j0, rows, m, ms, tid);
    __syncthreads();
    if (r < n) {
      for (int jl = lane; jl < rows; jl += 64) {
        const float* oj = is + jl * ms;
        bool dom, domd;  // r dominates j, j dominates r
        evx::dominates_both([&](int k) { return orow[k]; }, [&](int k) { return oj[k]; }, m, dom, domd);
        s += dom ? 1 : 0;
        dominated |= domd;
        if (j0 + jl != r) {
          const float d = d2([&](int k) { return orow[k]; }, [&](int k) { return oj[k]; }, m);
          if (d < a) {
            b = a;
            a = d;
          } else if (d < b) {
            b = d;
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // the count and the two smallest in one tree
    s += __shfl_xor(s, o, 64);
    const float oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64);
    const float hi = fmaxf(a, oa);
    a = fminf(a, oa);
    b = fminf(hi, fminf(b, ob));
  }
  const bool free_row = __ballot(dominated) == 0ull;
  if (lane == 0 && r < n) {
    S[r] = s;
    nd[r] = free_row ? 1 : 0;
    msk[r] = (free_row && !nanrow) ? 1 : 0;
    D[r] = nanrow ? __uint_as_float(0x7fc00000u) : __fdiv_rn(1.f, __fsqrt_rn(b) + 2.f);
  }
}

__global__ void __launch_bounds__(SF_THREADS) spea2_fit2_kernel(const float* __restrict__ obj, int n, int m, const int32_t* __restrict__ S,
                                                                 const uint8_t* __restrict__ msk, const float* __restrict__ D,
                                                                 float* __restrict__ R, float* __restrict__ sig,
                                                                 float* __restrict__ nn_d2, int32_t* __restrict__ nn_idx) {
  __shared__ float is[SF_TILE * (SP_MAX_M + 1)];
  __shared__ float js[SF_WAVES][SP_MAX_M];
  __shared__ int32_t ss[SF_TILE];
  __shared__ uint8_t mk[SF_TILE];
  const bool fit = S != nullptr;
  const int64_t run = blockIdx.y;  // as in spea2_fit1_kernel
  obj += run * n * m;
  msk += run * n;
  nn_d2 += run * n;
  nn_idx += run * n;
  if (fit) {
    S += run * n;
    D += run * n;
    R += run * n;
    sig += run * n;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x * SF_WAVES + wave;
  const int ms = m | 1;
  const float inf = __uint_as_float(SP_INF);
  if (lane < m) js[wave][lane] = r < n ? obj[(int64_t)r * m + lane] : 0.f;
  const bool masked = r < n && msk[r] != 0;
  const float* orow = js[wave];

  uint32_t racc = 0u;
  unsigned long long best = SP_NO_KEY;
  for (int i0 = 0; i0 < n; i0 += SF_TILE) {
    const int rows = min(SF_TILE, n - i0);
    __syncthreads();
    evx::stage_tile<SF_THREADS>(is, obj, i0, rows, m, ms, tid);
    if (tid < rows) {
      ss[tid] = fit ? S[i0 + tid] : 0;
      mk[tid] = msk[i0 + tid];
    }
    __syncthreads();
    if (r < n) {
      for (int il = lane; il < rows; il += 64) {
        const float* oi = is + il * ms;
        if (fit) racc += evx::dominates([&](int k) { return oi[k]; }, [&](int k) { return orow[k]; }, m) ? (uint32_t)ss[il] : 0u;
        if (masked && mk[il] != 0 && i0 + il != r) {
          const float d = d2([&](int k) { return orow[k]; }, [&](int k) { return oi[k]; }, m);
          if (d < inf) {
            const unsigned long long key = nn_key(d, i0 + il);
            best = key < best ? key : best;
          }
        }
      }
    }
  }
  racc = evx::wave_sum(racc);
  best = evx::wave_min(best);
  if (lane == 0 && r < n) {
    if (fit) {
      const float rr = (float)racc;
      R[r] = rr;
      sig[r] = D[r] + rr;
    }
    const bool none = best == SP_NO_KEY;
    nn_d2[r] = none ? inf : __uint_as_float((uint32_t)(best >> 32));
    nn_idx[r] = none ? -1 : (int32_t)~(uint32_t)best;
  }
}

// oT: the objectives transposed and zero padded to (M, n); blockDim.x = TB; order has n_order entries.  A workgroup per run:
// blockIdx.x is the run, oT (B, M, n), mask, nn_d2, nn_idx and keep (B, n), order (B, n_order), stats (B, 2); every run counts
// its own k and the runs share nothing.
template <int IT, int M, int TB>
__global__ void __launch_bounds__(TB) spea2_truncate_kernel(const float* __restrict__ oT, const uint8_t* __restrict__ mask,
                                                            const float* __restrict__ nn_d2, const int32_t* __restrict__ nn_idx, int n,
                                                            int n_keep, uint8_t* __restrict__ keep, int64_t* __restrict__ order,
                                                            int n_order, int32_t* __restrict__ stats) {
  constexpr bool REG = M <= 3;                    // the thread's objective rows live in registers
  constexpr int B = (M <= 4 && IT <= 8) ? 4 : 2;  // rescanned rows per pass
  constexpr int MO = REG ? M : 1;
  __shared__ evx::RemovalPart partF[2][SP_WAVES];
  __shared__ unsigned long long partP[2][SP_WAVES][B];
  __shared__ uint16_t wlist[SP_MAX_N];  // wave w: entries w·64·IT …
  __shared__ int wcount[SP_WAVES];
  using Shape = evx::RemovalShape<TB>;
  constexpr int lg = Shape::lg, nt = Shape::nt, nw = Shape::nw;
  const int64_t run = blockIdx.x;
  oT += run * M * n;
  mask += run * n;
  nn_d2 += run * n;
  nn_idx += run * n;
  keep += run * n;
  order += run * n_order;
  stats += run * 2;
  const int r = threadIdx.x, lane = r & 63, wave = r >> 6;
  const float inf = __uint_as_float(SP_INF);
  const unsigned long long below = (1ull << lane) - 1ull;

  float nnd[IT];
  int nni[IT];
  float own[IT][MO];
  uint32_t live = 0u;  // bit i: row r + i·nt is masked and not removed
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = r + (i << lg);
    const bool in = p < n && mask[p] != 0;
    live |= in ? (1u << i) : 0u;
    nnd[i] = in ? nn_d2[p] : inf;
    nni[i] = in ? nn_idx[p] : -1;
#pragma unroll
    for (int k = 0; k < MO; ++k) own[i][k] = (REG && p < n) ? oT[(int64_t)k * n + p] : 0.f;
  }
  // the count and the target lookup below are the same in spea2_select.hip and bce_select.hip and stay written out: as shared
  // helpers their unrolled wave loops are reassociated before inlining and every instantiation's code length changes
  const int c = evx::wave_sum((int)__popc(live));
  if (lane == 0) wcount[wave] = c;
  __syncthreads();
  int count = 0;
  for (int w = 0; w < nw; ++w) count += wcount[w];
  const int k_remove = min(max(0, count - n_keep), n_order);

  int x = -1, rescans = 0, pq = 0;
  for (int t = 0; t <= k_remove; ++t) {
    if (t > 0) {
      if (r == 0) order[t - 1] = (int64_t)x;
      if ((x & (nt - 1)) == r) live &= ~(1u << (x >> lg));
    }
    if (t == k_remove) break;
    const int buf = t & 1;
    // the rows that lose their neighbour, compacted per wave; the arg-min over the others
    int cw = 0;
    unsigned long long key = SP_NO_KEY;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int p = r + (i << lg);
      const bool on = (live >> i) & 1u;
      const bool flag = on && x >= 0 && nni[i] == x;
      cw = evx::wave_append(flag, (uint16_t)p, wlist + wave * (64 * IT), cw, below);
      if (on && !flag) {
        const unsigned long long q = arg_key(nnd[i], p);
        key = q < key ? q : key;
      }
    }
    key = evx::wave_min(key);
    if (lane == 0) partF[buf][wave] = evx::RemovalPart{key, cw};
    __syncthreads();
    // wave-uniform from here to the pass: readfirstlane moves the folds and the list lookups to the scalar unit
    int total = 0;
    key = SP_NO_KEY;
    for (int w = 0; w < nw; ++w) {
      const evx::RemovalPart q = partF[buf][w];
      const unsigned long long qk = evx::uniform(q.key);
      total += __builtin_amdgcn_readfirstlane(q.cnt);
      key = qk < key ? qk : key;
    }
    rescans += total;
    // one pass over the live rows for the NB targets b0 … b0 + NB − 1 of the waves' lists (in wave order), NB at compile time
    auto pass = [&](auto nbc, int b0) {
      constexpr int NB = decltype(nbc)::value;
      constexpr int UNR = M <= 3 ? IT : M <= 8 ? (IT < 8 ? IT : 8) : (IT < 4 ? IT : 4);  // re-read rows: 64 loads in flight at a time, not IT·M registers
      int tg[NB], bi[NB];
      float tv[NB][M], bd[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        int g = b0 + b, ws = 0, ss = 0;
        for (int w = 0; w < nw; ++w) {
          const int cnt = __builtin_amdgcn_readfirstlane(partF[buf][w].cnt);
          const bool hit = g >= 0 && g < cnt;
          ws = hit ? w : ws;
          ss = hit ? g : ss;
          g -= cnt;
        }
        tg[b] = __builtin_amdgcn_readfirstlane((int)wlist[ws * (64 * IT) + ss]);
        bd[b] = inf;
        bi[b] = -1;
#pragma unroll
        for (int k = 0; k < M; ++k) tv[b][k] = oT[(int64_t)k * n + tg[b]];
      }
#pragma unroll UNR
      for (int i = 0; i < IT; ++i) {
        const int p = r + (i << lg);
        const bool on = (live >> i) & 1u;
        float o[M];
#pragma unroll
        for (int k = 0; k < M; ++k) o[k] = REG ? own[i][k < MO ? k : 0] : (p < n ? oT[(int64_t)k * n + p] : 0.f);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          float d = d2([&](int k) { return o[k]; }, [&](int k) { return tv[b][k]; }, M);
          d = (on && p != tg[b]) ? d : inf;
          const bool take = d <= bd[b];  // p ascends: the highest row among equals (a row taken at +inf is dropped below)
          bd[b] = take ? d : bd[b];
          bi[b] = take ? p : bi[b];
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const unsigned long long kb = evx::wave_min(bd[b] < inf ? nn_key(bd[b], bi[b]) : SP_NO_KEY);
        if (lane == 0) partP[pq][wave][b] = kb;
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        unsigned long long q = SP_NO_KEY;
        for (int w = 0; w < nw; ++w) {
          const unsigned long long u = evx::uniform(partP[pq][w][b]);
          q = u < q ? u : q;
        }
        const bool none = q == SP_NO_KEY;
        const float nd_ = none ? inf : __uint_as_float((uint32_t)(q >> 32));
        const int ni_ = none ? -1 : (int)~(uint32_t)q;
        const bool mine = (tg[b] & (nt - 1)) == r;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
          const bool hit = mine && (tg[b] >> lg) == i;
          nnd[i] = hit ? nd_ : nnd[i];
          nni[i] = hit ? ni_ : nni[i];
        }
        const unsigned long long ak = arg_key(nd_, tg[b]);
        key = ak < key ? ak : key;
      }
      pq ^= 1;
    };
    for (int b0 = 0; b0 < total; b0 += B) {
      const int nb = total - b0;
      if (nb == 1)
        pass(std::integral_constant<int, 1>{}, b0);
      else if (B == 2 || nb == 2)
        pass(std::integral_constant<int, 2>{}, b0);
      else if (nb == 3)
        pass(std::integral_constant<int, B == 2 ? 2 : 3>{}, b0);
      else
        pass(std::integral_constant<int, B>{}, b0);
    }
    x = (int)(uint32_t)key;
  }

  evx::removal_finish<IT, TB>(live, n, k_remove, rescans, keep, order, n_order, stats);
}

}  // namespace

int evx_spea2_max_n() { return SP_MAX_N; }
int evx_spea2_fitness_max_n() { return SP_FIT_MAX_N; }
int evx_spea2_max_m() { return SP_MAX_M; }

void evx_spea2_fitness(const float* obj, int B, int n, int m, int32_t* S, uint8_t* nd, uint8_t* msk, float* D, float* R, float* sig,
                       float* nn_d2, int32_t* nn_idx, hipStream_t s) {
  if (n <= 0 || n > SP_FIT_MAX_N || m < 1 || m > SP_MAX_M || B < 1 || B > EVX_MAX_RUNS) return;
  const dim3 grid((n + SF_WAVES - 1) / SF_WAVES, B);
  spea2_fit1_kernel<<<grid, SF_THREADS, 0, s>>>(obj, n, m, S, nd, msk, D);
  spea2_fit2_kernel<<<grid, SF_THREADS, 0, s>>>(obj, n, m, S, msk, D, R, sig, nn_d2, nn_idx);
}

void evx_spea2_neighbours(const float* obj, int B, int n, int m, const uint8_t* mask, float* nn_d2, int32_t* nn_idx, hipStream_t s) {
  if (n <= 0 || m < 1 || m > SP_MAX_M || B < 1 || B > EVX_MAX_RUNS) return;
  spea2_fit2_kernel<<<dim3((n + SF_WAVES - 1) / SF_WAVES, B), SF_THREADS, 0, s>>>(obj, n, m, nullptr, mask, nullptr, nullptr, nullptr,
                                                                                  nn_d2, nn_idx);
}

void evx_spea2_truncate(const float* objT, int B, int n, int M, const uint8_t* mask, const float* nn_d2, const int32_t* nn_idx, int n_keep,
                        uint8_t* keep, int64_t* order, int n_order, int32_t* stats, hipStream_t s) {
  if (n <= 0 || n > SP_MAX_N || M != evx_padded_m(M) || B < 1 || B > EVX_MAX_RUNS) return;
  evx::dispatch_removal_shape(n, [&](auto it, auto tb) {
    evx::dispatch_padded_m(M, [&](auto mm) {
      constexpr int IT = decltype(it)::value, TB = decltype(tb)::value, MM = decltype(mm)::value;
      spea2_truncate_kernel<IT, MM, TB><<<B, TB, 0, s>>>(objT, mask, nn_d2, nn_idx, n, n_keep, keep, order, n_order, stats);
    });
  });
}
