// NSGA-III's normalisation and association (evoxmi/algorithms/mo/nsga3.py; reference algorithms/mo/nsga3.py:60-92): the
// steps between the non-dominated sort and nsga3_select.hip.  The contract is stated in evoxmi/ops/nsga3.py; every
// operation is float64 on the float32 inputs in the order written there, and this file is compiled with
// -ffp-contract=off.  Per-run operands carry a leading run axis (B = 1 is the solo call); the reference points are
// shared by the runs.  No (n, K) array exists, nothing is sorted, no atomics: bitwise reproducible, and run b of a
// batched launch is the solo launch on that run bit for bit (a workgroup never reads another run's words).
//
// nsga3_normalize_kernel   one workgroup of 1024 threads per run (n ≤ 8192, m ≤ 16, N < n).
//   1. thread t keeps the ranks of rows t, t + 1024, … (≤ 8) in registers.  last_rank = the smallest r with
//      #{rank ≤ r} > N: a bisection on r between the block minimum and maximum of the ranks, one block count per
//      step (≤ 32 steps, 14 for ranks in [0, n]).  valid = rank ≤ last_rank goes to LDS as a bit per row (ballots).
//   2. thread t then owns column j = t mod mp (mp = m rounded up to a power of two) of rows t / mp, t / mp + 1024 / mp, …:
//      ideal_j = min over the valid rows (a NaN wins, as torch's min) by a shuffle butterfly over the lanes of equal
//      j, the 16 waves through LDS, thread j over the waves in wave order.
//   3. the same threads: asf_j(row) = max_k (f_k − ideal_k) / (δ_jk + 1e-6) (+inf on a row outside valid, a NaN
//      wins the max) and the first row that holds its minimum (a NaN wins the min: torch's argmin), as a
//      (value, row) butterfly; worst_j = max over the valid rows of f_j − ideal_j in the same pass.
//   4. thread 0: E = the extreme rows minus ideal, E·x = 1 by Gaussian elimination with partial pivoting in LDS
//      (the operation order of knea_select.hip's plane: the first row on equal magnitudes, row r ← row r −
//      (A_rc / A_cc)·row c, back substitution with k ascending), intercept = 1 / x; nadir = intercept when no
//      pivot was exactly 0 (or NaN) and every intercept is finite and > 1e-6, else worst.
//   Every row of f passes through registers once in step 2 and m times (through the cache) in step 3.
//   LDS: valid bits 1 KiB, wave partials 2 × 2 KiB + 1 KiB, the system 16 × 17 doubles, ideal / worst / x, counts.
//
// nsga3_ref_prepare_kernel  one thread per reference point: ŵ_k = w_k / sqrt(Σ_j w_kj², j ascending) into the float64
//   scratch what (m, K), once for all runs.  A zero reference point gives NaN, which no row is associated with.
//
// nsga3_associate_kernel<MM>  grid (⌈n / 16⌉, B), 1024 threads: a wave per row, 16 rows per workgroup.
//   Lanes j < m form x_j = (f_j − ideal_j) / nadir_j into LDS; every lane keeps x in MM registers (MM = m padded to
//   2, 3, 4, 8, 16 with zeros) and s = |x|² = Σ_j x_j², j ascending.  ŵ passes through one LDS tile of 4096 doubles
//   (32 KiB) shared by the 16 waves: TK = 4096 / (MM rounded up to a power of two) reference points, objective j at
//   tile[j·TK …], so the lanes of a wave read consecutive doubles.  Lane l scans the points l, l + 64, … of the tile
//   and keeps the smallest d² = max(s − (Σ_j x_j·ŵ_jk, j ascending)², 0) with the lowest k that holds it; a
//   (value, position) butterfly finishes the row and lane 0 takes one square root.  A row with s = 0 or s not
//   finite writes (group, group_dist) = (0, NaN), which is what the torch expression yields for it.
//   LDS: the tile 32 KiB + x of the 16 rows 2 KiB.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage):
//   kernel                 VGPR  SGPR  scratch  LDS [B]  occupancy [waves/SIMD]
//   nsga3_normalize        51    52    0        9920     8
//   nsga3_ref_prepare      16    14    0        0        8
//   nsga3_associate<2>     29    38    0        34816    8
//   nsga3_associate<3>     31    42    0        34816    8
//   nsga3_associate<4>     33    42    0        34816    8
//   nsga3_associate<8>     41    50    0        34816    8
//   nsga3_associate<16>    57    66    0        34816    8
// No spill.
#include <climits>
#include <math.h>

#include "evoxmi_mo.h"

namespace {

constexpr int NA_THREADS = 1024;
constexpr int NA_WAVES = NA_THREADS / 64;
constexpr int NA_MAXN = 8192;
constexpr int NA_MAXM = 16;
constexpr int NA_IT = NA_MAXN / NA_THREADS;  // ranks per thread in the bisection
constexpr int NA_TILE = 4096;                // doubles of ŵ per LDS tile

__device__ __forceinline__ double nan_max_d(double a, double b) { return (b > a || b != b) ? b : a; }

// (a, ra) orders before (b, rb) in torch's argmin: a NaN before every number, then the value, then the row
__device__ __forceinline__ bool argmin_before(double a, int ra, double b, int rb) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ra < rb);
  return a < b || (a == b && ra < rb);
}

struct NormShared {
  unsigned long long valid[NA_MAXN / 64];
  double wasf[NA_WAVES][NA_MAXM], wworst[NA_WAVES][NA_MAXM];
  float wmin[NA_WAVES][NA_MAXM];
  int wrow[NA_WAVES][NA_MAXM];
  double A[NA_MAXM][NA_MAXM + 1];
  double ideal[NA_MAXM], worst[NA_MAXM], x[NA_MAXM];
  int ext[NA_MAXM];
  int red[2][NA_WAVES];
};

__global__ void __launch_bounds__(NA_THREADS)
    nsga3_normalize_kernel(const float* __restrict__ f, const int32_t* __restrict__ rank, int n, int m, int mp, int N,
                           int32_t* __restrict__ last_rank, double* __restrict__ scale) {
  __shared__ NormShared sh;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  f += (size_t)b * n * m;
  rank += (size_t)b * n;

  // 1. last_rank by bisection on the rank value
  int rk[NA_IT];
  int mn = INT_MAX, mx = INT_MIN;
#pragma unroll
  for (int i = 0; i < NA_IT; ++i) {
    const int r = i * NA_THREADS + t;
    rk[i] = r < n ? rank[r] : INT_MAX;
    if (r < n) {
      mn = min(mn, rk[i]);
      mx = max(mx, rk[i]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, 64));
    mx = max(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    sh.red[0][wave] = mn;
    sh.red[1][wave] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NA_WAVES; ++w) {
    mn = min(mn, sh.red[0][w]);
    mx = max(mx, sh.red[1][w]);
  }
  __syncthreads();                  // red is free again
  long long lo = mn, hi = mx;       // #{rank ≤ hi} = n > N: the answer lies in [lo, hi]
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const long long mid = lo + ((hi - lo) >> 1);
    int c = 0;
#pragma unroll
    for (int i = 0; i < NA_IT; ++i) c += (i * NA_THREADS + t < n && (long long)rk[i] <= mid) ? 1 : 0;
    c = evx::block_sum<NA_WAVES>(c, sh.red[it & 1]);
    if (c > N) hi = mid; else lo = mid + 1;
  }
  const int lr = (int)lo;
#pragma unroll
  for (int i = 0; i < NA_IT; ++i) {
    const unsigned long long bal = __ballot(i * NA_THREADS + t < n && rk[i] <= lr);
    if (lane == 0) sh.valid[i * NA_WAVES + wave] = bal;
  }
  __syncthreads();

  // 2. ideal: thread (row slice r0, column j)
  const int j = t & (mp - 1), rstep = NA_THREADS / mp, r0 = t / mp;
  {
    float v = INFINITY;
    if (j < m)
      for (int r = r0; r < n; r += rstep)
        if ((sh.valid[r >> 6] >> (r & 63)) & 1ull) v = evx::nan_min(v, f[(size_t)r * m + j]);
    for (int o = mp; o < 64; o <<= 1) v = evx::nan_min(v, __shfl_xor(v, o, 64));
    if (lane < mp) sh.wmin[wave][lane] = v;
    __syncthreads();
    if (t < m) {
      float a = sh.wmin[0][t];
      for (int w = 1; w < NA_WAVES; ++w) a = evx::nan_min(a, sh.wmin[w][t]);
      sh.ideal[t] = (double)a;
    }
    __syncthreads();
  }

  // 3. the extreme row of every axis and worst
  {
    double best = INFINITY, wst = -INFINITY;
    int brow = INT_MAX;
    if (j < m)
      for (int r = r0; r < n; r += rstep) {
        double a = INFINITY;
        if ((sh.valid[r >> 6] >> (r & 63)) & 1ull) {
          a = -INFINITY;
          for (int k = 0; k < m; ++k) {
            const double fn = (double)f[(size_t)r * m + k] - sh.ideal[k];
            a = nan_max_d(a, fn / (k == j ? 1.0 + 1e-6 : 1e-6));
            if (k == j) wst = nan_max_d(wst, fn);
          }
        }
        if (argmin_before(a, r, best, brow)) best = a, brow = r;
      }
    for (int o = mp; o < 64; o <<= 1) {
      const double ob = __shfl_xor(best, o, 64), ow = __shfl_xor(wst, o, 64);
      const int orow = __shfl_xor(brow, o, 64);
      if (argmin_before(ob, orow, best, brow)) best = ob, brow = orow;
      wst = nan_max_d(wst, ow);
    }
    if (lane < mp) {
      sh.wasf[wave][lane] = best;
      sh.wrow[wave][lane] = brow;
      sh.wworst[wave][lane] = wst;
    }
    __syncthreads();
    if (t < m) {
      best = sh.wasf[0][t], brow = sh.wrow[0][t], wst = sh.wworst[0][t];
      for (int w = 1; w < NA_WAVES; ++w) {
        if (argmin_before(sh.wasf[w][t], sh.wrow[w][t], best, brow)) best = sh.wasf[w][t], brow = sh.wrow[w][t];
        wst = nan_max_d(wst, sh.wworst[w][t]);
      }
      sh.ext[t] = brow < n ? brow : 0;  // every row takes part, so brow < n; the guard keeps the read below in range
      sh.worst[t] = wst;
    }
    __syncthreads();
  }

  // 4. the hyperplane through the extremes, on one thread (the arrays are indexed dynamically: LDS, not scratch)
  if (t == 0) {
    bool ok = true;
    for (int a = 0; a < m; ++a) {
      for (int c = 0; c < m; ++c) sh.A[a][c] = (double)f[(size_t)sh.ext[a] * m + c] - sh.ideal[c];
      sh.A[a][m] = 1.0;
    }
    for (int c = 0; c < m; ++c) {
      int piv = c;
      double best = fabs(sh.A[c][c]);
      for (int r = c + 1; r < m; ++r)
        if (fabs(sh.A[r][c]) > best) best = fabs(sh.A[r][c]), piv = r;
      if (!(best > 0.0)) {  // an exact zero or NaN pivot
        ok = false;
        break;
      }
      if (piv != c)
        for (int k = 0; k <= m; ++k) {
          const double tmp = sh.A[c][k];
          sh.A[c][k] = sh.A[piv][k];
          sh.A[piv][k] = tmp;
        }
      for (int r = c + 1; r < m; ++r) {
        const double fct = sh.A[r][c] / sh.A[c][c];
        for (int k = c; k <= m; ++k) sh.A[r][k] = sh.A[r][k] - fct * sh.A[c][k];
      }
    }
    if (ok) {
      for (int c = m - 1; c >= 0; --c) {
        double s = sh.A[c][m];
        for (int k = c + 1; k < m; ++k) s = s - sh.A[c][k] * sh.x[k];
        sh.x[c] = s / sh.A[c][c];
      }
      for (int c = 0; c < m; ++c) {
        const double ic = 1.0 / sh.x[c];
        sh.x[c] = ic;
        ok = ok && isfinite(ic) && ic > 1e-6;
      }
    }
    double* sc = scale + (size_t)b * 2 * m;
    for (int c = 0; c < m; ++c) {
      sc[c] = sh.ideal[c];
      sc[m + c] = ok ? sh.x[c] : sh.worst[c];
    }
    last_rank[b] = lr;
  }
}

__global__ void nsga3_ref_prepare_kernel(const float* __restrict__ ref, int K, int m, double* __restrict__ what) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int j = 0; j < m; ++j) {
    const double w = (double)ref[(size_t)k * m + j];
    s = j == 0 ? w * w : s + w * w;
  }
  const double nrm = sqrt(s);
  for (int j = 0; j < m; ++j) what[(size_t)j * K + k] = (double)ref[(size_t)k * m + j] / nrm;
}

template <int MM>
__global__ void __launch_bounds__(NA_THREADS)
    nsga3_associate_kernel(const float* __restrict__ f, const double* __restrict__ scale, const double* __restrict__ what, int n, int m,
                           int K, int64_t* __restrict__ group, float* __restrict__ group_dist) {
  constexpr int MP = MM == 3 ? 4 : MM;
  constexpr int TK = NA_TILE / MP;  // reference points per tile
  __shared__ double tile[NA_TILE];
  __shared__ double xs[NA_WAVES][NA_MAXM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const int i = blockIdx.x * NA_WAVES + wave;
  const bool live = i < n;
  f += (size_t)b * n * m;
  scale += (size_t)b * 2 * m;
  group += (size_t)b * n;
  group_dist += (size_t)b * n;

  if (lane < NA_MAXM) {
    double v = 0.0;
    if (live && lane < m) v = ((double)f[(size_t)i * m + lane] - scale[lane]) / scale[m + lane];
    xs[wave][lane] = v;
  }
  __syncthreads();
  double x[MM];
#pragma unroll
  for (int j = 0; j < MM; ++j) x[j] = xs[wave][j];
  double s = x[0] * x[0];
#pragma unroll
  for (int j = 1; j < MM; ++j) s = s + x[j] * x[j];  // the padding adds +0

  double bd = INFINITY;
  int bp = INT_MAX;
  for (int k0 = 0; k0 < K; k0 += TK) {
    const int w = min(TK, K - k0);
    __syncthreads();  // the previous tile is consumed
    for (int e = threadIdx.x; e < m * w; e += NA_THREADS) {
      const int jj = e / w, kk = e - jj * w;
      tile[jj * TK + kk] = what[(size_t)jj * K + k0 + kk];
    }
    __syncthreads();
    if (live)
      for (int kk = lane; kk < w; kk += 64) {
        double dot = x[0] * tile[kk];
#pragma unroll
        for (int j = 1; j < MM; ++j)
          if (j < m) dot = dot + x[j] * tile[j * TK + kk];
        double d2 = s - dot * dot;
        d2 = d2 < 0.0 ? 0.0 : d2;
        if (d2 < bd) bd = d2, bp = k0 + kk;  // k ascends within a lane: the lowest position of the lane's minimum
      }
  }
  if (!live) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o, 64);
    const int op = __shfl_xor(bp, o, 64);
    if (od < bd || (od == bd && op < bp)) bd = od, bp = op;
  }
  if (lane == 0) {
    const bool bad = !(s > 0.0 && s < (double)INFINITY) || bp == INT_MAX;
    group[i] = bad ? 0 : (int64_t)bp;
    group_dist[i] = bad ? __int_as_float(0x7fc00000) : (float)sqrt(bd);
  }
}

}  // namespace

void evx_nsga3_associate(const float* f, const int32_t* rank, const float* ref, int B, int n, int m, int K, int N, double* what,
                         int32_t* last_rank, double* scale, int64_t* group, float* group_dist, hipStream_t s) {
  int mp = 1;
  while (mp < m) mp <<= 1;
  nsga3_normalize_kernel<<<B, NA_THREADS, 0, s>>>(f, rank, n, m, mp, N, last_rank, scale);
  nsga3_ref_prepare_kernel<<<(K + 255) / 256, 256, 0, s>>>(ref, K, m, what);
  const dim3 grid((n + NA_WAVES - 1) / NA_WAVES, B);
  evx::dispatch_padded_m(evx_padded_m(m), [&](auto mm) {
    nsga3_associate_kernel<decltype(mm)::value><<<grid, NA_THREADS, 0, s>>>(f, scale, what, n, m, K, group, group_dist);
  });
}
