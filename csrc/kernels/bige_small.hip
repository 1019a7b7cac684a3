// BiGE's bi-goal estimate AND the Pareto rank of the bi-goal points for B independent runs in ONE launch: a workgroup of 1024
// threads per run does what the three launches of bige_select.hip and a non-dominated sort of the (n, 2) result do for one
// population, and gives every run the same words.  The arithmetic is evoxmi_bige.h's, the contract the one stated in
// evoxmi/ops/bige.py; this file is compiled with -ffp-contract=off like bige_select.hip.  The rank's contract is nds.hip's.
//
// A run's normalised rows x stay resident in LDS as float64, laid [t][n] so that the lanes of a wave read consecutive words,
// with pr beside them; the bi-goal points then stay in LDS as float32 pairs and are ranked there.  Nothing goes through a
// global scratch, no global atomic and no float atomic is issued:
//
//   1. the float32 column extremes of the masked rows (exact, so their order is free): thread t scans column t % m of the
//      rows t / m, t / m + 1024 / m, …, then thread k < m folds column k                                    two barriers
//   2. thread i, i + 1024: x_i and pr_i into LDS, +inf for a row outside the mask                            barrier
//   3. a wave takes the rows i = wave, wave + 16, …: its x in registers, lane l adds the partners j ≡ l (mod 64) in ascending
//      j from LDS, the butterfly adds the 64 lanes (the order of bige_crowd_kernel, whose tiles are multiples of 64 rows);
//      lane 0 writes pr, cd and bi out and the float32 pair into LDS                                         barrier
//   4. rank: thread t owns the rows t and t + 1024.  One pass over all n pairs, every lane reading the same LDS word, counts a
//      row's dominators in a register; all n candidates are resident, so there is no staging tile and no padding of the two
//      columns.  Then one front per iteration: the unranked rows with count 0, laid out in row order by evx::peel_compact, their
//      pairs copied into a list over the x words, which are dead by now, after which every thread lowers its owned counts by
//      the rows of the list that dominate them.  Dominance is a strict partial order, so every iteration ranks at least one
//      row; the loop is kept finite regardless, as in nds_batched.hip.
//
// LDS, sized by the run's own shape: m · n float64 of x, later the front list (64 KiB at the caps n ≤ 2048 / 1024 / 512 for
// m ≤ 4 / 8 / 16, evx_bige_small_ok), n float64 of pr (16 KiB), n float32 pairs of bi (16 KiB), and statically 2 · 1024 float32
// of the extremes' partials (8 KiB), 2 · 16 float32 of extremes and 32 ints of the compaction: at most 104.3 KiB of gfx950's 160.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evoxmi_bige.h"
#include "evoxmi_launchers.h"
#include "evoxmi_peel.h"

namespace {

using namespace evx;

constexpr int BS_THREADS = 1024;
constexpr int BS_WAVES = BS_THREADS / 64;
constexpr int BS_ITEMS = 2;  // owned rows per thread in the rank: n ≤ 2048
constexpr int BS_MAX_M = 16;

__device__ __forceinline__ bool bs_dominates(float2 a, float2 b) { return a.x <= b.x && a.y <= b.y && (a.x < b.x || a.y < b.y); }

template <int MC>
__global__ void __launch_bounds__(BS_THREADS)
    bige_small_kernel(const float* __restrict__ f, const bool* __restrict__ mask, const float* __restrict__ r_in, int n, int m,
                      float* __restrict__ bi, int32_t* __restrict__ rank, double* __restrict__ pr_out, double* __restrict__ cd_out) {
  extern __shared__ __align__(16) double bs_lds[];
  __shared__ float smn[BS_THREADS], smx[BS_THREADS], sfmin[BS_MAX_M], sfmax[BS_MAX_M];
  __shared__ int wcnt[BS_ITEMS * BS_WAVES];
  double* sx = bs_lds;                                  // [m][n], steps 2 and 3
  float2* front = reinterpret_cast<float2*>(bs_lds);    // [n], step 4: the pairs of the new front, in row order
  double* spr = bs_lds + (size_t)m * n;                 // [n]
  float2* sbi = reinterpret_cast<float2*>(spr + n);     // [n]
  const int run = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  f += (size_t)run * n * m;
  mask += (size_t)run * n;
  bi += (size_t)run * n * 2;
  rank += (size_t)run * n;
  pr_out += (size_t)run * n;
  cd_out += (size_t)run * n;

  // 1. the column extremes
  {
    const int per = BS_THREADS / m, col = t % m, sub = t / m;
    float mn = INFINITY, mx = -INFINITY;
    if (sub < per)
      for (int i = sub; i < n; i += per)
        if (mask[i]) {
          const float v = f[(size_t)i * m + col];
          if (v < mn) mn = v;
          if (v > mx) mx = v;
        }
    smn[t] = mn;
    smx[t] = mx;
    __syncthreads();
    if (t < m) {
      for (int s = 1; s < per; ++s) {
        const float a = smn[s * m + t], b = smx[s * m + t];
        if (a < mn) mn = a;
        if (b > mx) mx = b;
      }
      sfmin[t] = mn;
      sfmax[t] = mx;
    }
    __syncthreads();
  }

  // 2. x and pr
  for (int i = t; i < n; i += BS_THREADS) spr[i] = bg_normalise_row(f + (size_t)i * m, mask[i], m, sfmin, sfmax, sx + i, (size_t)n);
  __syncthreads();

  // 3. the crowding degree
  const double r = (double)r_in[run];
  const double rr_hi = bg_prefilter(r);
  for (int i = wave; i < n; i += BS_WAVES) {
    const bool scan = mask[i];
    double a[MC];
#pragma unroll
    for (int k = 0; k < MC; ++k) a[k] = (scan && k < m) ? sx[k * n + i] : 0.0;
    const double pi = scan ? spr[i] : 0.0;
    double acc = 0.0;
    int dup = 0;
    if (scan)
      for (int j = lane; j < n; j += 64) bg_pair<MC>(a, sx + j, n, m, j == i, pi, spr + j, r, rr_hi, acc, dup);
    const double sum = bg_wave_cd(acc, dup);
    if (lane == 0) {
      const double cd = scan ? sum : INFINITY, p = scan ? pi : INFINITY;
      pr_out[i] = p;
      cd_out[i] = cd;
      const float2 b = make_float2((float)p, (float)cd);
      bi[(size_t)i * 2] = b.x;
      bi[(size_t)i * 2 + 1] = b.y;
      sbi[i] = b;
    }
  }
  __syncthreads();  // x is dead from here on

  // 4. the rank of the bi-goal points
  const int nit = (n + BS_THREADS - 1) / BS_THREADS;  // ≤ BS_ITEMS
  float2 own[BS_ITEMS];
  int cnt[BS_ITEMS], pre[PEEL_ITEMS];
  uint32_t alive = 0;
#pragma unroll
  for (int it = 0; it < BS_ITEMS; ++it) {
    const int i = it * BS_THREADS + t;
    cnt[it] = 0;
    own[it] = make_float2(0.f, 0.f);
    if (i < n) {
      alive |= 1u << it;
      own[it] = sbi[i];
    }
  }
  for (int j = 0; j < n; ++j) {
    const float2 c = sbi[j];
#pragma unroll
    for (int it = 0; it < BS_ITEMS; ++it) cnt[it] += bs_dominates(c, own[it]) ? 1 : 0;  // a slot past n is never read
  }

  int ranked = 0, k = 0;
  bool force = false;
  for (;;) {
    uint32_t flags = 0;
#pragma unroll
    for (int it = 0; it < BS_ITEMS; ++it) flags |= (((alive >> it) & 1u) && (cnt[it] <= 0 || force) ? 1u : 0u) << it;
    const int tot = peel_compact<BS_THREADS>(flags, nit, wcnt, pre);  // its barriers also end the reads of the list
    if (tot == 0) {  // cannot happen while a row is unranked (strict partial order); keeps the loop finite regardless
      force = true;
      continue;
    }
#pragma unroll
    for (int it = 0; it < BS_ITEMS; ++it)
      if ((flags >> it) & 1u) {
        front[pre[it]] = own[it];
        rank[it * BS_THREADS + t] = k;
      }
    alive &= ~flags;
    ranked += tot;
    if (ranked >= n) return;  // uniform: tot and ranked are the same in every thread
    if (k + 1 >= n) {
#pragma unroll
      for (int it = 0; it < BS_ITEMS; ++it)
        if ((alive >> it) & 1u) rank[it * BS_THREADS + t] = n;
      return;
    }
    __syncthreads();
    for (int j = 0; j < tot; ++j) {
      const float2 c = front[j];
#pragma unroll
      for (int it = 0; it < BS_ITEMS; ++it) cnt[it] -= bs_dominates(c, own[it]) ? 1 : 0;
    }
    ++k;
  }
}

size_t bs_lds_bytes(int n, int m) { return ((size_t)m * n + n) * sizeof(double) + (size_t)n * sizeof(float2); }

template <int MC>
void bs_launch(const float* f, const bool* mask, const float* r, int B, int n, int m, float* bi, int32_t* rank, double* pr, double* cd,
               hipStream_t s) {
  const size_t lds = bs_lds_bytes(n, m);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)bige_small_kernel<MC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  bige_small_kernel<MC><<<B, BS_THREADS, lds, s>>>(f, mask, r, n, m, bi, rank, pr, cd);
}

}  // namespace

bool evx_bige_small_ok(int64_t n, int64_t m) {
  if (n < 1 || m < 1 || m > BS_MAX_M) return false;
  const int64_t mc = m <= 4 ? 4 : (m <= 8 ? 8 : 16);
  return n * mc <= 8192;
}

void evx_bige_small_estimate_rank(const float* f, const bool* mask, const float* r, int B, int n, int m, float* bi, int32_t* rank, double* pr,
                                  double* cd, hipStream_t s) {
  if (m <= 4)
    bs_launch<4>(f, mask, r, B, n, m, bi, rank, pr, cd, s);
  else if (m <= 8)
    bs_launch<8>(f, mask, r, B, n, m, bi, rank, pr, cd, s);
  else
    bs_launch<16>(f, mask, r, B, n, m, bi, rank, pr, cd, s);
}
