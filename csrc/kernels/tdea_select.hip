// θ-DEA's θ-ranking (reference algorithms/mo/tdea.py:100-178) on top of rvea_select.hip's best cosine of every row to
// the reference directions: the penalised distance val = d1 + θ·d2 of every row to its direction, and the rank of every
// masked row among the masked rows of its direction.  The contract is stated in evoxmi/ops/tdea.py; every operation is
// float64 on the float32 inputs in the order written there, and this file is compiled with -ffp-contract=off.  No
// (n, nw) array exists and nothing is sorted: a rank is an exact count of the rows that order before.
//
// Launches (after rvea_prepare_kernel and rvea_cos_best_kernel, mode 0):
//   tdea_val_kernel    one thread per row: cls from arg, the norm as rvea_cos_best_kernel forms it, d1, d2 and val.
//   tdea_count_kernel  a wave per row i, 16 waves per workgroup.  (cls, val) of the rows j pass through an LDS tile of
//                      2048 rows that the 16 waves share, a row outside the mask as cls = −1; lanes stride over j and
//                      count the rows of the same cls with (val_j, j) < (val_i, i), a NaN after every number; a
//                      butterfly adds the 64 integer counts.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evoxmi_launchers.h"

namespace {

constexpr int TD_THREADS = 1024;
constexpr int TD_WAVES = TD_THREADS / 64;
constexpr int TD_TILE = 2048;  // rows j per LDS tile

__global__ void tdea_val_kernel(const float* __restrict__ obj, const double* __restrict__ best, const int* __restrict__ arg,
                                const float* __restrict__ theta, int n, int m, int nw, int* __restrict__ cls_out, double* __restrict__ val_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int t = 0; t < m; ++t) {
    const double d = (double)obj[(size_t)i * m + t];
    s = t == 0 ? d * d : s + d * d;
  }
  const double nrm = sqrt(s);
  int cls = arg[i];
  cls = cls < 0 ? 0 : (cls >= nw ? nw - 1 : cls);  // a NaN row's −1
  double c = best[i];
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  const double d1 = nrm * c;
  double q = 1.0 - c * c;
  if (q < 0.0) q = 0.0;
  const double d2 = nrm * sqrt(q);
  cls_out[i] = cls;
  val_out[i] = d1 + (double)theta[cls] * d2;
}

__global__ void __launch_bounds__(TD_THREADS)
    tdea_count_kernel(const int* __restrict__ cls, const double* __restrict__ val, const bool* __restrict__ mask, int n,
                      float* __restrict__ t_rank) {
  __shared__ double tval[TD_TILE];
  __shared__ int tcls[TD_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * TD_WAVES + wave;
  const bool live = i < n;
  const bool scan = live && mask[i];
  const int ci = scan ? cls[i] : -2;
  const double vi = scan ? val[i] : 0.0;
  const bool nan_i = vi != vi;
  int count = 0;
  for (int j0 = 0; j0 < n; j0 += TD_TILE) {
    const int w = min(TD_TILE, n - j0);
    __syncthreads();
    for (int jj = threadIdx.x; jj < w; jj += TD_THREADS) {
      tval[jj] = val[j0 + jj];
      tcls[jj] = mask[j0 + jj] ? cls[j0 + jj] : -1;
    }
    __syncthreads();
    if (scan) {
      for (int jj = lane; jj < w; jj += 64) {
        if (tcls[jj] != ci) continue;
        const double vj = tval[jj];
        const int j = j0 + jj;
        const bool nan_j = vj != vj;
        bool before;
        if (nan_i || nan_j)
          before = nan_i && (!nan_j || j < i);
        else
          before = vj < vi || (vj == vi && j < i);
        count += before ? 1 : 0;
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
  if (lane == 0) t_rank[i] = scan ? (float)(1 + count) : INFINITY;
}

}  // namespace

void evx_tdea_theta_rank(const float* obj, const double* best, const int* arg, const float* theta, const bool* mask, int n, int m, int nw,
                         int* cls, double* val, float* t_rank, hipStream_t s) {
  tdea_val_kernel<<<(n + 255) / 256, 256, 0, s>>>(obj, best, arg, theta, n, m, nw, cls, val);
  tdea_count_kernel<<<(n + TD_WAVES - 1) / TD_WAVES, TD_THREADS, 0, s>>>(cls, val, mask, n, t_rank);
}
