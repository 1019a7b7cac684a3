// BiGE's bi-goal estimate (reference algorithms/mo/bige.py:64-142): the proximity of every masked row, the sum of its
// normalised objectives, and its crowding degree, a sharing function summed over the masked rows inside the niche
// radius r.  The contract is stated in evoxmi/ops/bige.py; every operation is float64 on the float32 inputs in the
// order written there, and this file is compiled with -ffp-contract=off so that no multiply and add fuse.  No (n, n)
// array exists: the pairs are formed in registers from an LDS tile.
//
// Launches:
//   bige_extremes_kernel  one workgroup: the float32 column minima and maxima over the masked rows (exact, so their
//                         order is free); +inf and −inf for an empty mask.
//   bige_prepare_kernel   one thread per row: x = (f − fmin) / span into a float64 scratch laid out (m, n), so that the
//                         lanes of a wave read consecutive words, and pr = ((x_0 + x_1) + …) into an (n,) scratch.  A row
//                         outside the mask gets x = pr = +inf: its distance to every masked row is +inf, which is never
//                         below r, so it contributes to nothing without a test of its own.
//   bige_crowd_kernel     a wave per row i, 16 waves per workgroup.  The row's x stays in registers; x and pr of the rows
//                         j pass through an LDS tile of 4096 / MC rows that the 16 waves share; lanes stride over j and
//                         keep a float64 partial sum; a butterfly adds the 64 lanes (every term is ≥ 0, the order is
//                         fixed, so a second call is bitwise equal).  A pair at distance 0 contributes exactly 1; those
//                         are counted in an integer and added last, so the equal rows of a block, whose other terms
//                         are the same words at the same positions, get bitwise equal sums.  The square root and the division are skipped for
//                         pairs with d2 ≥ r²·(1 + 2⁻⁴⁰) (r² is exact, r being a float32; the product rounds once): there
//                         the exact root exceeds r, and a correctly rounded root is monotone, so d ≥ r.  The prefilter
//                         never drops a pair that the test d < r keeps, and that test still decides every pair it lets by.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evoxmi_launchers.h"

namespace {

constexpr int BG_THREADS = 1024;
constexpr int BG_WAVES = BG_THREADS / 64;
constexpr int BG_TILE_WORDS = 4096;  // float64 words of x per LDS tile; the tile holds 4096 / MC rows

__global__ void __launch_bounds__(BG_THREADS)
    bige_extremes_kernel(const float* __restrict__ f, const bool* __restrict__ mask, int n, int m, float* __restrict__ fmin,
                         float* __restrict__ fmax) {
  __shared__ float smn[BG_THREADS], smx[BG_THREADS];
  // thread t owns column t % m of the rows t / m, t / m + rows_per_pass, …; m ≤ 16 divides into 1024 threads with a rest
  const int per = BG_THREADS / m, col = threadIdx.x % m, sub = threadIdx.x / m;
  float mn = INFINITY, mx = -INFINITY;
  if (sub < per)
    for (int i = sub; i < n; i += per)
      if (mask[i]) {
        const float v = f[(size_t)i * m + col];
        if (v < mn) mn = v;
        if (v > mx) mx = v;
      }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  if (threadIdx.x < m) {
    for (int s = 1; s < per; ++s) {
      const float a = smn[s * m + threadIdx.x], b = smx[s * m + threadIdx.x];
      if (a < mn) mn = a;
      if (b > mx) mx = b;
    }
    fmin[threadIdx.x] = mn;
    fmax[threadIdx.x] = mx;
  }
}

__global__ void bige_prepare_kernel(const float* __restrict__ f, const bool* __restrict__ mask, int n, int m, const float* __restrict__ fmin,
                                    const float* __restrict__ fmax, double* __restrict__ x, double* __restrict__ pr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!mask[i]) {
    for (int t = 0; t < m; ++t) x[(size_t)t * n + i] = INFINITY;
    pr[i] = INFINITY;
    return;
  }
  double s = 0.0;
  for (int t = 0; t < m; ++t) {
    const double lo = (double)fmin[t];
    double span = (double)fmax[t] - lo;
    if (!(span >= 1e-6)) span = 1e-6;
    const double v = ((double)f[(size_t)i * m + t] - lo) / span;
    x[(size_t)t * n + i] = v;
    s = t == 0 ? v : s + v;
  }
  pr[i] = s;
}

template <int MC>
__global__ void __launch_bounds__(BG_THREADS)
    bige_crowd_kernel(const double* __restrict__ x, const double* __restrict__ pr, const bool* __restrict__ mask, const float* __restrict__ r_in,
                      int n, int m, float* __restrict__ bi, double* __restrict__ pr_out, double* __restrict__ cd_out) {
  constexpr int TJ = BG_TILE_WORDS / MC;
  __shared__ double tile[BG_TILE_WORDS];  // [t][TJ]
  __shared__ double tpr[TJ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * BG_WAVES + wave;
  const bool live = i < n;
  const bool scan = live && mask[i];
  const double r = (double)r_in[0];
  const double rr_hi = (r * r) * (1.0 + 0x1p-40);
  double a[MC];
#pragma unroll
  for (int t = 0; t < MC; ++t) a[t] = 0.0;
  double pi = 0.0;
  if (scan) {
#pragma unroll
    for (int t = 0; t < MC; ++t)
      if (t < m) a[t] = x[(size_t)t * n + i];
    pi = pr[i];
  }
  double acc = 0.0;
  int dup = 0;
  for (int j0 = 0; j0 < n; j0 += TJ) {
    const int w = min(TJ, n - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < BG_TILE_WORDS; e += BG_THREADS) {
      const int t = e / TJ, jj = e % TJ;
      if (t < m && jj < w) tile[e] = x[(size_t)t * n + j0 + jj];
    }
    for (int jj = threadIdx.x; jj < w; jj += BG_THREADS) tpr[jj] = pr[j0 + jj];
    __syncthreads();
    if (scan) {
      for (int jj = lane; jj < w; jj += 64) {
        double d2 = 0.0;
#pragma unroll
        for (int t = 0; t < MC; ++t)
          if (t < m) {
            const double dl = a[t] - tile[t * TJ + jj];
            const double p = dl * dl;
            d2 = t == 0 ? p : d2 + p;
          }
        if (d2 < rr_hi && j0 + jj != i) {  // a NaN fails the test
          const double d = sqrt(d2);
          if (d2 == 0.0 && 0.0 < r) {
            dup += 1;  // an equal row: equal x, so equal pr, w = 2 and sh = (0.5 · (2 · (1 − 0 / r)))² = 1 exactly
          } else if (d < r) {
            const double pj = tpr[jj];
            const double wgt = 1.0 + (pi >= pj ? 1.0 : 0.0) + (pi > pj ? 1.0 : 0.0);
            const double h = 0.5 * (wgt * (1.0 - d / r));
            acc += h * h;
          }
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_xor(acc, off);
    dup += __shfl_xor(dup, off);
  }
  if (lane != 0) return;
  const double cd = scan ? sqrt(acc + (double)dup) : INFINITY;
  const double p = scan ? pi : INFINITY;
  pr_out[i] = p;
  cd_out[i] = cd;
  bi[(size_t)i * 2] = (float)p;
  bi[(size_t)i * 2 + 1] = (float)cd;
}

}  // namespace

void evx_bige_estimate(const float* f, const bool* mask, const float* r, int n, int m, float* fmin, float* fmax, double* x, double* prs,
                       float* bi, double* pr, double* cd, hipStream_t s) {
  bige_extremes_kernel<<<1, BG_THREADS, 0, s>>>(f, mask, n, m, fmin, fmax);
  bige_prepare_kernel<<<(n + 255) / 256, 256, 0, s>>>(f, mask, n, m, fmin, fmax, x, prs);
  const int grid = (n + BG_WAVES - 1) / BG_WAVES;
  if (m <= 4)
    bige_crowd_kernel<4><<<grid, BG_THREADS, 0, s>>>(x, prs, mask, r, n, m, bi, pr, cd);
  else if (m <= 8)
    bige_crowd_kernel<8><<<grid, BG_THREADS, 0, s>>>(x, prs, mask, r, n, m, bi, pr, cd);
  else
    bige_crowd_kernel<16><<<grid, BG_THREADS, 0, s>>>(x, prs, mask, r, n, m, bi, pr, cd);
}
