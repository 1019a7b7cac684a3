// The RVEA family's selection primitives (reference operators/selection/rvea_selection.py:9-54 and
// algorithms/mo/rveaa.py:22-61): for every row of A the largest cosine to a row of B and the first position that holds
// it, the angle-penalised distance on top of that, and the per-vector pick of the least distance.  The contract is
// stated in evoxmi/ops/rvea.py; every operation is float64 on the float32 inputs in the order written there, and this
// file is compiled with -ffp-contract=off so that no multiply and add fuse.
//
// Launches:
//   rvea_prepare_kernel   one thread per row of B: b̂ = B_j / |B_j| into a float64 scratch laid out (m, k), so that the
//                         lanes of a wave read consecutive words; it also resets the pick's (key, row) words.
//   rvea_cos_best_kernel  a wave per row of A, 16 waves per workgroup.  The row's â stays in registers; b̂ passes
//                         through a 32 KiB LDS tile of 4096 / MC columns that the 16 waves share; lanes stride over the
//                         columns and keep (value, lowest position); a butterfly reduces the 64 lanes.  Lane 0 then writes
//                         best, arg and, by mode, γ = acos(best) or the row's apd, whose ordered bits it folds into its
//                         vector's key with an integer atomic min (a min does not depend on the order of its operands).
//   rvea_pick_rows_kernel one thread per row: a row whose apd bits equal its vector's key folds its position into the
//                         vector's row word, again with an atomic min: the lowest position among equal values.
//   rvea_pick_out_kernel  one thread per vector: next_ind and empty from the row word.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "evoxmi_launchers.h"

namespace {

constexpr int RV_THREADS = 1024;
constexpr int RV_WAVES = RV_THREADS / 64;
constexpr int RV_TILE_WORDS = 4096;  // float64 words of b̂ per LDS tile
constexpr int RV_NO_ROW = INT_MAX;

// the bits of a double as an unsigned word whose order is the order of the values; a non-finite value ranks as +inf
__device__ inline unsigned long long rv_ordered(double x) {
  if (!(fabs(x) <= 1.7976931348623157e308)) x = INFINITY;
  x = x + 0.0;  // −0 → +0
  unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void rvea_prepare_kernel(const float* __restrict__ B, int k, int m, double* __restrict__ bn, unsigned long long* __restrict__ key,
                                    int* __restrict__ pick, int nkey) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < k) {
    double s = 0.0;
    for (int t = 0; t < m; ++t) {
      const double b = (double)B[(size_t)j * m + t];
      s = t == 0 ? b * b : s + b * b;
    }
    const double nrm = sqrt(s);
    for (int t = 0; t < m; ++t) bn[(size_t)t * k + j] = (double)B[(size_t)j * m + t] / nrm;
  }
  if (key != nullptr && j < nkey) {
    key[j] = ~0ull;
    pick[j] = RV_NO_ROW;
  }
}

// mode 0: best, arg.  mode 1: also aux = acos(best).  mode 2: also aux = apd (gamma, theta given) and the key fold.
template <int MC>
__global__ void __launch_bounds__(RV_THREADS)
    rvea_cos_best_kernel(const float* __restrict__ A, const float* __restrict__ shift, int has_floor, double floor_v,
                         const double* __restrict__ bn, int n, int k, int m, int clamp, int self_zero, int mode,
                         const double* __restrict__ gamma, const float* __restrict__ theta, double* __restrict__ best_out,
                         int* __restrict__ arg_out, double* __restrict__ aux, unsigned long long* __restrict__ key) {
  constexpr int TJ = RV_TILE_WORDS / MC;
  __shared__ double tile[RV_TILE_WORDS];  // [t][TJ]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * RV_WAVES + wave;
  const bool live = i < n;
  double a[MC];
  double nrm = 0.0;
  bool nan_row = false;
#pragma unroll
  for (int t = 0; t < MC; ++t) a[t] = 0.0;
  if (live) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < MC; ++t)
      if (t < m) {
        const float x = A[(size_t)i * m + t];
        nan_row |= x != x;
        double d = (double)x;
        if (shift != nullptr) d = d - (double)shift[t];
        if (has_floor && d < floor_v) d = floor_v;  // a NaN stays
        a[t] = d;
        s = t == 0 ? d * d : s + d * d;
      }
    nrm = sqrt(s);
#pragma unroll
    for (int t = 0; t < MC; ++t)
      if (t < m) a[t] = a[t] / nrm;
  }
  const bool scan = live && !nan_row;
  double bst = -INFINITY;
  int arg = RV_NO_ROW;
  for (int j0 = 0; j0 < k; j0 += TJ) {
    const int w = min(TJ, k - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < RV_TILE_WORDS; e += RV_THREADS) {
      const int t = e / TJ, jj = e % TJ;
      if (t < m && jj < w) tile[e] = bn[(size_t)t * k + j0 + jj];
    }
    __syncthreads();
    if (scan) {
      for (int jj = lane; jj < w; jj += 64) {
        double c = 0.0;
#pragma unroll
        for (int t = 0; t < MC; ++t)
          if (t < m) {
            const double p = a[t] * tile[t * TJ + jj];
            c = t == 0 ? p : c + p;
          }
        if (c != c) c = -INFINITY;
        else if (clamp) c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
        const int j = j0 + jj;
        if (self_zero && j == i) c = 0.0;
        if (c > bst) {
          bst = c;
          arg = j;
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(bst, off);
    const int oa = __shfl_xor(arg, off);
    if (ob > bst || (ob == bst && oa < arg)) {
      bst = ob;
      arg = oa;
    }
  }
  if (lane != 0) return;
  if (nan_row) {
    bst = self_zero ? 0.0 : -INFINITY;
    arg = -1;
  } else if (arg == RV_NO_ROW) {
    arg = 0;  // every entry −inf
  }
  best_out[i] = bst;
  arg_out[i] = arg;
  if (mode == 1) {
    aux[i] = acos(bst);
  } else if (mode == 2) {
    double apd = INFINITY;
    if (arg >= 0) {
      const double angle = acos(bst);
      apd = (1.0 + (((double)m * (double)theta[0]) * angle) / gamma[arg]) * nrm;
      atomicMin(&key[arg], rv_ordered(apd));
    }
    aux[i] = apd;
  }
}

__global__ void rvea_pick_rows_kernel(const int* __restrict__ arg, const double* __restrict__ apd, int n, int nv,
                                      const unsigned long long* __restrict__ key, int* __restrict__ pick) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = arg[i];
  if (j < 0 || j >= nv) return;
  if (rv_ordered(apd[i]) == key[j]) atomicMin(&pick[j], i);
}

__global__ void rvea_pick_out_kernel(const int* __restrict__ pick, int nv, int64_t* __restrict__ next_ind, bool* __restrict__ empty) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nv) return;
  const int p = pick[j];
  empty[j] = p == RV_NO_ROW;
  next_ind[j] = p == RV_NO_ROW ? 0 : (int64_t)p;
}

}  // namespace

void evx_rvea_prepare(const float* B, int k, int m, double* bn, uint64_t* key, int* pick, int nkey, hipStream_t s) {
  const int rows = k > nkey ? k : nkey;
  rvea_prepare_kernel<<<(rows + 255) / 256, 256, 0, s>>>(B, k, m, bn, (unsigned long long*)key, pick, key != nullptr ? nkey : 0);
}

void evx_rvea_cos_best(const float* A, const float* shift, int has_floor, double floor_v, const double* bn, int n, int k, int m, int clamp,
                       int self_zero, int mode, const double* gamma, const float* theta, double* best, int* arg, double* aux, uint64_t* key,
                       hipStream_t s) {
  const int grid = (n + RV_WAVES - 1) / RV_WAVES;
  unsigned long long* kp = (unsigned long long*)key;
  if (m <= 4)
    rvea_cos_best_kernel<4><<<grid, RV_THREADS, 0, s>>>(A, shift, has_floor, floor_v, bn, n, k, m, clamp, self_zero, mode, gamma, theta, best,
                                                        arg, aux, kp);
  else if (m <= 8)
    rvea_cos_best_kernel<8><<<grid, RV_THREADS, 0, s>>>(A, shift, has_floor, floor_v, bn, n, k, m, clamp, self_zero, mode, gamma, theta, best,
                                                        arg, aux, kp);
  else
    rvea_cos_best_kernel<16><<<grid, RV_THREADS, 0, s>>>(A, shift, has_floor, floor_v, bn, n, k, m, clamp, self_zero, mode, gamma, theta, best,
                                                         arg, aux, kp);
}

void evx_rvea_pick(const int* arg, const double* apd, int n, int nv, const uint64_t* key, int* pick, int64_t* next_ind, bool* empty,
                   hipStream_t s) {
  rvea_pick_rows_kernel<<<(n + 255) / 256, 256, 0, s>>>(arg, apd, n, nv, (const unsigned long long*)key, pick);
  rvea_pick_out_kernel<<<(nv + 255) / 256, 256, 0, s>>>(pick, nv, next_ind, empty);
}
