// RVEA's APD selection for B independent runs in ONE launch: a workgroup of 1024 threads per run does what the five launches
// of rvea_select.hip do for one problem, and gives every run the same words.  The arithmetic is evoxmi_rvea.h's, the contract
// the one stated in evoxmi/ops/rvea.py; this file is compiled with -ffp-contract=off like rvea_select.hip.
//
// What differs is where the data lives.  A run's normalised vectors b̂ stay resident in LDS as float64, laid [t][nv] so that
// the lanes of a wave read consecutive words; γ, the per-vector key word (the ordered bits of the least apd) and pick word (the
// lowest row that holds it) live beside them.  Nothing goes through a global scratch and no global atomic is issued:
//
//   1. thread j: b̂_j into LDS, key_j and pick_j reset                                                        barrier
//   2. a wave per group of RW vectors: their â (= b̂, formed from v as the 2-D launch forms it) in registers, lanes stride
//      over the LDS columns (clamp, self-zero), butterfly; lane 0: γ_j = acos(best) to LDS and out              barrier
//   3. a wave per group of RW rows of f: â from f − shift raised to the floor, the same scan; lane 0: arg_i and apd_i from
//      γ in LDS and the run's θ, and the 64-bit LDS atomic min of rv_ordered(apd_i) into key[arg_i]            barrier
//   4. thread i: a row whose ordered apd equals its vector's key folds i into pick with an LDS atomic min    barrier
//      thread j: next_ind_j and empty_j from pick_j
//
// A wave keeps RW rows in registers (4 for m ≤ 4, 2 for m ≤ 8, 1 above) and reads each b̂ column once for all of them: one ds_read_b64 per
// row and objective would leave the scan bound by LDS bandwidth (a wave's read takes as long as its multiply and add, and
// the four SIMDs share one LDS).  Both folds are minima, so the result does not depend on the order the waves arrive in.
//
// LDS: (m + 2) · nv float64 words and nv ints, sized by the run's own nv and m (182 rows on 91 vectors of 3 objectives take
// 4 KiB, so small runs share a CU); the caps keep b̂ within 8192 words: nv · MC ≤ 8192 for the padded objective count
// MC ∈ {4, 8, 16}, and n ≤ 4096 (at most 104 KiB).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "evoxmi_launchers.h"
#include "evoxmi_rvea.h"

namespace {

using namespace evx;

constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_BN_WORDS = 8192;  // float64 words of b̂ a run may hold
constexpr int RS_N_CAP = 4096;

constexpr int rs_padded_m(int64_t m) { return m <= 4 ? 4 : (m <= 8 ? 8 : 16); }

// RW rows' â against the nv columns of b̂ in LDS: every lane's (value, lowest position) over its columns, then the butterfly.
// A row that is not to be scanned (past the end, or a NaN row) goes through with whatever â it has: rv_settle overrules it
template <int MC, int RW>
__device__ __forceinline__ void rs_scan(const double (&a)[RW][MC], int i0, const double* bn, int nv, int m, int self_zero, int lane,
                                        double (&bst)[RW], int (&arg)[RW]) {
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    bst[r] = -INFINITY;
    arg[r] = RV_NO_ROW;
  }
  for (int j = lane; j < nv; j += 64) {
    double b[MC];
#pragma unroll
    for (int t = 0; t < MC; ++t) b[t] = t < m ? bn[t * nv + j] : 0.0;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const double c = rv_cosine<MC>(a[r], b, 1, m, 1, self_zero && j == i0 + r);
      if (c > bst[r]) {
        bst[r] = c;
        arg[r] = j;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RW; ++r) rv_wave_best(bst[r], arg[r]);
}

template <int MC>
__global__ void __launch_bounds__(RS_THREADS)
    rvea_small_select_kernel(const float* __restrict__ f, const float* __restrict__ shift, double floor_v, const float* __restrict__ v,
                             const float* __restrict__ theta, int n, int nv, int m, int64_t* __restrict__ next_ind, bool* __restrict__ empty,
                             int* arg_out, double* apd_out, double* __restrict__ gamma_out) {
  constexpr int RW = MC == 4 ? 4 : (MC == 8 ? 2 : 1);  // what 128 VGPRs hold without scratch
  extern __shared__ __align__(16) double rs_lds[];
  double* bn = rs_lds;                                                      // [m][nv]
  double* gam = bn + (size_t)m * nv;                                        // [nv]
  unsigned long long* key = reinterpret_cast<unsigned long long*>(gam + nv);  // [nv]
  int* pick = reinterpret_cast<int*>(key + nv);                             // [nv]
  const int run = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f += (size_t)run * n * m;
  v += (size_t)run * nv * m;
  shift += (size_t)run * m;
  next_ind += (size_t)run * nv;
  empty += (size_t)run * nv;
  arg_out += (size_t)run * n;
  apd_out += (size_t)run * n;
  gamma_out += (size_t)run * nv;
  const float th = theta[run];

  // 1. b̂ and the reset of the fold words
  for (int j = threadIdx.x; j < nv; j += RS_THREADS) {
    const float* b = v + (size_t)j * m;
    const double nrm = rv_vector_norm(b, m);
    for (int t = 0; t < m; ++t) bn[t * nv + j] = (double)b[t] / nrm;
    key[j] = ~0ull;
    pick[j] = RV_NO_ROW;
  }
  __syncthreads();

  double a[RW][MC] = {}, nrm[RW] = {}, bst[RW];
  int arg[RW];
  bool nan_row[RW];

  // 2. γ
  for (int i0 = wave * RW; i0 < nv; i0 += RS_WAVES * RW) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      nan_row[r] = false;
      if (i0 + r < nv) nrm[r] = rv_load_row<MC>(v + (size_t)(i0 + r) * m, nullptr, 0, 0.0, m, a[r], nan_row[r]);
    }
    rs_scan<MC, RW>(a, i0, bn, nv, m, 1, lane, bst, arg);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
        if (i0 + r < nv) {
          rv_settle(nan_row[r], 1, bst[r], arg[r]);
          const double g = acos(bst[r]);
          gam[i0 + r] = g;
          gamma_out[i0 + r] = g;
        }
    }
  }
  __syncthreads();

  // 3. association and apd
  for (int i0 = wave * RW; i0 < n; i0 += RS_WAVES * RW) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      nan_row[r] = false;
      if (i0 + r < n) nrm[r] = rv_load_row<MC>(f + (size_t)(i0 + r) * m, shift, 1, floor_v, m, a[r], nan_row[r]);
    }
    rs_scan<MC, RW>(a, i0, bn, nv, m, 0, lane, bst, arg);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
        if (i0 + r < n) {
          rv_settle(nan_row[r], 0, bst[r], arg[r]);
          double apd = INFINITY;
          if (arg[r] >= 0) {
            apd = rv_apd(m, th, bst[r], gam[arg[r]], nrm[r]);
            atomicMin(&key[arg[r]], rv_ordered(apd));
          }
          arg_out[i0 + r] = arg[r];
          apd_out[i0 + r] = apd;
        }
    }
  }
  __syncthreads();  // also orders lane 0's arg_out and apd_out before the reads below (one workgroup, one CU)

  // 4. the pick
  for (int i = threadIdx.x; i < n; i += RS_THREADS) {
    const int j = arg_out[i];
    if (j >= 0 && j < nv && rv_ordered(apd_out[i]) == key[j]) atomicMin(&pick[j], i);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nv; j += RS_THREADS) {
    const int p = pick[j];
    empty[j] = p == RV_NO_ROW;
    next_ind[j] = p == RV_NO_ROW ? 0 : (int64_t)p;
  }
}

template <int MC>
void rs_launch(const float* f, const float* shift, double floor_v, const float* v, const float* theta, int B, int n, int nv, int m,
               int64_t* next_ind, bool* empty, int* arg, double* apd, double* gamma, hipStream_t s) {
  const size_t lds = ((size_t)m * nv + 2 * (size_t)nv) * sizeof(double) + (size_t)nv * sizeof(int);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)rvea_small_select_kernel<MC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  rvea_small_select_kernel<MC><<<B, RS_THREADS, lds, s>>>(f, shift, floor_v, v, theta, n, nv, m, next_ind, empty, arg, apd, gamma);
}

}  // namespace

bool evx_rvea_small_ok(int64_t n, int64_t nv, int64_t m) {
  return m >= 1 && m <= 16 && n >= 1 && n <= RS_N_CAP && nv >= 1 && nv * rs_padded_m(m) <= RS_BN_WORDS;
}

void evx_rvea_small_select(const float* f, const float* shift, double floor_v, const float* v, const float* theta, int B, int n, int nv, int m,
                           int64_t* next_ind, bool* empty, int* arg, double* apd, double* gamma, hipStream_t s) {
  if (m <= 4)
    rs_launch<4>(f, shift, floor_v, v, theta, B, n, nv, m, next_ind, empty, arg, apd, gamma, s);
  else if (m <= 8)
    rs_launch<8>(f, shift, floor_v, v, theta, B, n, nv, m, next_ind, empty, arg, apd, gamma, s);
  else
    rs_launch<16>(f, shift, floor_v, v, theta, B, n, nv, m, next_ind, empty, arg, apd, gamma, s);
}
