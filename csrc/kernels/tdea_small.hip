// θ-DEA's θ-ranking for B independent runs in ONE launch: a workgroup of 1024 threads per run does what the four launches
// rvea_prepare, rvea_cos_best (mode 0), tdea_val and tdea_count do for one problem, and gives every run the same words.  The
// arithmetic is evoxmi_rvea.h's and evoxmi_tdea.h's, the contract the one stated in evoxmi/ops/tdea.py; this file is compiled
// with -ffp-contract=off like rvea_select.hip and tdea_select.hip.
//
// A run's normalised directions b̂ stay resident in LDS as float64, laid [t][nw] as rvea_small.hip lays them, with θ, and then
// cls and val of the run's rows beside them.  Nothing goes through a global scratch and no global atomic is issued:
//
//   1. thread j: b̂_j and θ_j into LDS                                                                          barrier
//   2. a wave per group of RW rows: their â in registers, lanes stride over the LDS columns, butterfly; lane 0: cls and val
//      (evoxmi_tdea.h) to LDS and out, a row outside the mask as cls −1                                       barrier
//   3. the rank of a masked row is 1 + the count of the masked rows of its cluster that order before it.  The clusters'
//      member lists are built over the b̂ words, which are dead by now: a count per direction (LDS integer atomic add), an
//      exclusive block scan of the nw counts, and a scatter of the row indices into one segment per direction, each with a
//      barrier after it.  Thread i then scans only the segment of its own cluster.  A count does not depend on the order in
//      which the atomics filled a segment, so the ranks are deterministic.
//
// With nw ≈ n / 2 directions, as in θ-DEA, a cluster holds about two rows and step 3 is O(n); all rows in one cluster is n
// compares per row.  A wave keeps RW rows in registers (4 for m ≤ 4, 2 for m ≤ 8, 1 above), as rvea_small.hip does and
// for its reason: one LDS read of a b̂ column serves all of them.
//
// LDS: max(m · nw float64, nw + n ints) for b̂ and then the lists, n float64 of val, nw float32 of θ, n ints of cls and the scan's
// 16: at most 64 + 32 + 8 + 16 KiB under the caps of evx_rvea_small_ok (nw · MC ≤ 8192, n ≤ 4096), sized by the run's own shape.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evoxmi_launchers.h"
#include "evoxmi_mo.h"
#include "evoxmi_rvea.h"
#include "evoxmi_tdea.h"

namespace {

using namespace evx;

constexpr int TS_THREADS = 1024;
constexpr int TS_WAVES = TS_THREADS / 64;

// the float64 words that hold b̂ first and the member lists (nw offsets, n row indices) after it
size_t ts_region_words(int n, int nw, int m) {
  const size_t bn = (size_t)m * nw, lists = ((size_t)nw + n + 1) / 2;
  return bn > lists ? bn : lists;
}

template <int MC>
__global__ void __launch_bounds__(TS_THREADS)
    tdea_small_theta_rank_kernel(const float* __restrict__ obj, const float* __restrict__ w, int64_t w_run_stride,
                                 const float* __restrict__ theta, int64_t theta_run_stride, const bool* __restrict__ mask, int n, int nw, int m,
                                 size_t region_words, int* __restrict__ cls_out, double* __restrict__ val_out, float* __restrict__ t_rank) {
  constexpr int RW = MC == 4 ? 4 : (MC == 8 ? 2 : 1);  // what 128 VGPRs hold without scratch
  extern __shared__ __align__(16) double ts_lds[];
  double* bn = ts_lds;                                    // [m][nw], steps 1 and 2
  int* off = reinterpret_cast<int*>(ts_lds);              // [nw], step 3: a direction's count, then its segment's end
  int* seg = off + nw;                                    // [n], step 3: the masked rows, cluster by cluster
  double* sval = ts_lds + region_words;                   // [n]
  float* sth = reinterpret_cast<float*>(sval + n);        // [nw]
  int* scls = reinterpret_cast<int*>(sth + nw);           // [n]
  int* wsum = scls + n;                                   // [TS_WAVES], the block scan's
  const int run = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  obj += (size_t)run * n * m;
  w += (size_t)run * w_run_stride;
  theta += (size_t)run * theta_run_stride;
  mask += (size_t)run * n;
  cls_out += (size_t)run * n;
  val_out += (size_t)run * n;
  t_rank += (size_t)run * n;

  // 1. b̂ and θ
  for (int j = threadIdx.x; j < nw; j += TS_THREADS) {
    const float* b = w + (size_t)j * m;
    const double nrm = rv_vector_norm(b, m);
    for (int t = 0; t < m; ++t) bn[t * nw + j] = (double)b[t] / nrm;
    sth[j] = theta[j];
  }
  __syncthreads();

  // 2. cls and val
  for (int i0 = wave * RW; i0 < n; i0 += TS_WAVES * RW) {
    double a[RW][MC] = {}, bst[RW];
    int arg[RW];
    bool nan_row[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      nan_row[r] = false;
      if (i0 + r < n) (void)rv_load_row<MC>(obj + (size_t)(i0 + r) * m, nullptr, 0, 0.0, m, a[r], nan_row[r]);
      bst[r] = -INFINITY;
      arg[r] = RV_NO_ROW;
    }
    // a row past the end or with a NaN goes through with whatever â it has: a NaN cosine counts as −inf and rv_settle overrules it
    for (int j = lane; j < nw; j += 64) {
      double b[MC];
#pragma unroll
      for (int t = 0; t < MC; ++t) b[t] = t < m ? bn[t * nw + j] : 0.0;
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const double c = rv_cosine<MC>(a[r], b, 1, m, 0, false);
        if (c > bst[r]) {
          bst[r] = c;
          arg[r] = j;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) rv_wave_best(bst[r], arg[r]);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
        if (i0 + r < n) {
          const int i = i0 + r;
          rv_settle(nan_row[r], 0, bst[r], arg[r]);
          int cls;
          double val;
          td_cls_val(obj + (size_t)i * m, m, nw, bst[r], arg[r], sth, cls, val);
          cls_out[i] = cls;
          val_out[i] = val;
          scls[i] = mask[i] ? cls : -1;
          sval[i] = val;
        }
    }
  }
  __syncthreads();  // b̂ is dead from here on

  // 3. the member lists over the b̂ words, then the count inside the own cluster
  for (int j = threadIdx.x; j < nw; j += TS_THREADS) off[j] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += TS_THREADS) {
    const int c = scls[i];
    if (c >= 0) atomicAdd(&off[c], 1);
  }
  __syncthreads();
  {
    // nw ≤ 2048: thread t owns the directions 2t and 2t + 1
    const int j0 = 2 * threadIdx.x;
    const int c0 = j0 < nw ? off[j0] : 0, c1 = j0 + 1 < nw ? off[j0 + 1] : 0;
    int total;
    const int start = block_scan_excl<TS_WAVES>(c0 + c1, wsum, total);
    if (j0 < nw) off[j0] = start;
    if (j0 + 1 < nw) off[j0 + 1] = start + c0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += TS_THREADS) {
    const int c = scls[i];
    if (c >= 0) seg[atomicAdd(&off[c], 1)] = i;  // afterwards off[c] is the end of c's segment, the start of c + 1's
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += TS_THREADS) {
    const int c = scls[i];
    float rank = INFINITY;
    if (c >= 0) {
      const double vi = sval[i];
      const int end = off[c];
      int count = 0;
      for (int p = c == 0 ? 0 : off[c - 1]; p < end; ++p) {
        const int j = seg[p];
        count += td_before(sval[j], j, vi, i) ? 1 : 0;
      }
      rank = (float)(1 + count);
    }
    t_rank[i] = rank;
  }
}

template <int MC>
void ts_launch(const float* obj, const float* w, int64_t w_run_stride, const float* theta, int64_t theta_run_stride, const bool* mask, int B,
               int n, int nw, int m, int* cls, double* val, float* t_rank, hipStream_t s) {
  const size_t region = ts_region_words(n, nw, m);
  const size_t lds = (region + (size_t)n) * sizeof(double) + (size_t)nw * sizeof(float) + ((size_t)n + TS_WAVES) * sizeof(int);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)tdea_small_theta_rank_kernel<MC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  tdea_small_theta_rank_kernel<MC><<<B, TS_THREADS, lds, s>>>(obj, w, w_run_stride, theta, theta_run_stride, mask, n, nw, m, region, cls, val,
                                                              t_rank);
}

}  // namespace

void evx_tdea_small_theta_rank(const float* obj, const float* w, int64_t w_run_stride, const float* theta, int64_t theta_run_stride,
                               const bool* mask, int B, int n, int nw, int m, int* cls, double* val, float* t_rank, hipStream_t s) {
  if (m <= 4)
    ts_launch<4>(obj, w, w_run_stride, theta, theta_run_stride, mask, B, n, nw, m, cls, val, t_rank, s);
  else if (m <= 8)
    ts_launch<8>(obj, w, w_run_stride, theta, theta_run_stride, mask, B, n, nw, m, cls, val, t_rank, s);
  else
    ts_launch<16>(obj, w, w_run_stride, theta, theta_run_stride, mask, B, n, nw, m, cls, val, t_rank, s);
}
