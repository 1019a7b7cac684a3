// Exact hypervolume of n boxes [0, p_i] at m = 2, 3, 4 objectives and the exclusive contribution of every row at m = 2, 3.
// The contract is stated in evoxmi/ops/hv.py.  Every sum is float64 over non-negative terms in a fixed order, and this
// file is compiled with -ffp-contract=off so that no multiply and add fuse.
//
// Everything reduces to one primitive, the masked staircase scan A(keep, cx, cy): walk the rows by x descending (ties by
// original index), skip the rows outside keep, clip the others to x' = min(x, cx), y' = min(y, cy), carry the running
// maximum pm of the y' seen before the row, and sum x' · max(0, y' − pm).  A row outside keep is scanned with y' = 0:
// its term is x' · max(0, 0 − pm) = 0 and it leaves pm where it was.
//
// The coordinates are non-negative float32 words, so their bit patterns order as they do, and min, max and the prefix
// maximum run on the 32-bit patterns: exact, and a DPP scan moves one register, not two.  The words become float64
// only where arithmetic starts (exactly).
//
// Launches (the sort of the columns is torch's stable sort, in the wrapper):
//   hv_rank_kernel     one thread per sorted position k: zrank and wrank of the row that holds it, and the slice heights
//                      h_k = z_(k) − z_(k+1), g_l likewise over w.  At m = 2 there is one slice of height 1 that keeps all.
//   hv_gather_kernel   one thread per position r of the x order: the row's x, y, its two ranks packed in one word, and
//                      its original index.
//   hv_flat_kernel     a wave per slice, 16 waves per workgroup, the x-ordered rows pass through a shared LDS tile of
//                      2048 rows.  TOTAL: slice k keeps zrank ≤ k, writes h_k · A to scratch[k].  CONTRIB (m = 2): slice r
//                      keeps j ≠ r clipped to (x_r, y_r) and writes the row's contribution.
//   hv_owned_kernel    n ≤ 2048, the rows are loaded to LDS once.  A workgroup owns one l (TOTAL, m = 4) or one row r
//                      (CONTRIB, m = 3); its waves take the slices k in turn, each wave adds its h_k · (…) in the order of
//                      k, and thread 0 adds the 16 wave sums in the order of the waves.
//   hv_reduce_kernel   one workgroup: the scratch words in a fixed order (thread t takes t, t + 1024, …, then a tree).
//
// Within a slice a lane keeps a float64 partial sum over its rows of every chunk of 64 and a butterfly adds the lanes.
// No float atomics anywhere: a second call is bitwise equal.
//
// The contributions are summed in the complementary form.  With d_j = max(0, y'_j − pm_j), Σ d_j = pm_end, so
//   x_i·y_i − A = x_i · (y_i − pm_end) + Σ_j (x_i − x'_j) · d_j,
// every term of which is ≥ 0 and at most the area of the clip box.  A row whose box lies inside another row's box
// meets that row in every slice of positive height; before it x' = x_i, after it d = 0, so all terms are exactly 0.
// Once pm reaches y_i all later terms are 0 and the scan of that slice stops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "evoxmi_launchers.h"

namespace {

constexpr int HV_THREADS = 1024;
constexpr int HV_WAVES = HV_THREADS / 64;
constexpr int HV_TILE = 2048;  // rows of the x order per LDS tile: 3 words each, 24 KiB

__device__ __forceinline__ double f64_of(uint32_t bits) { return (double)__uint_as_float(bits); }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {
  // lanes without a source, or outside ROW_MASK, read 0: the identity of max over non-negative patterns
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}

// the maximum of v over the lanes 0 … lane (inclusive), wave64
__device__ __forceinline__ uint32_t wave_prefix_max(uint32_t v) {
  v = max(v, dpp_or_zero<0x111, 0xf>(v));  // row_shr:1
  v = max(v, dpp_or_zero<0x112, 0xf>(v));  // row_shr:2
  v = max(v, dpp_or_zero<0x114, 0xf>(v));  // row_shr:4
  v = max(v, dpp_or_zero<0x118, 0xf>(v));  // row_shr:8
  v = max(v, dpp_or_zero<0x142, 0xa>(v));  // row_bcast:15 into rows 1 and 3
  v = max(v, dpp_or_zero<0x143, 0xc>(v));  // row_bcast:31 into rows 2 and 3
  return v;
}

// the inclusive prefix of the lane before (0 at lane 0): the neighbour inside a row of 16, and lane 15 of the row before,
// which is what lane 0 of a row needs and no more than what its other lanes already have
__device__ __forceinline__ uint32_t wave_shift_prefix(uint32_t inc) {
  return max(dpp_or_zero<0x111, 0xf>(inc), dpp_or_zero<0x142, 0xe>(inc));
}

struct Tile {
  uint32_t x[HV_TILE], y[HV_TILE], zw[HV_TILE];
};

__device__ __forceinline__ void load_tile(Tile& t, const uint32_t* __restrict__ X, const uint32_t* __restrict__ Y,
                                          const uint32_t* __restrict__ ZW, int j0, int w) {
  for (int e = threadIdx.x; e < w; e += HV_THREADS) {
    t.x[e] = X[j0 + e];
    t.y[e] = Y[j0 + e];
    t.zw[e] = ZW[j0 + e];
  }
}

// One slice over the w rows of a tile that starts at position j0 of the x order.  keep: zrank ≤ kz and wrank ≤ kw and
// position ≠ skip.  pm is the carried maximum (a pattern, wave-uniform), acc the lane's partial sum.  Returns true when
// CONTRIB and pm has reached cy, after which every term is 0.
template <bool CONTRIB>
__device__ __forceinline__ bool scan_tile(const Tile& t, int j0, int w, int lane, uint32_t kz, uint32_t kw, int skip, uint32_t cx,
                                          uint32_t cy, uint32_t& pm, double& acc) {
  for (int c0 = 0; c0 < w; c0 += 64) {
    const int jj = c0 + lane;
    uint32_t xb = 0, yb = 0;
    if (jj < w) {
      const uint32_t zw = t.zw[jj];
      const bool keep = (zw & 0xffffu) <= kz && (zw >> 16) <= kw && j0 + jj != skip;
      xb = t.x[jj];
      yb = keep ? t.y[jj] : 0u;
      if (CONTRIB) {
        xb = min(xb, cx);
        yb = min(yb, cy);
      }
    }
    const uint32_t inc = max(wave_prefix_max(yb), pm);
    const uint32_t prev = max(wave_shift_prefix(inc), pm);  // lane 0 sees the carry alone
    double d = f64_of(yb) - f64_of(prev);
    if (!(d > 0.0)) d = 0.0;
    if (CONTRIB)
      acc += (f64_of(cx) - f64_of(xb)) * d;
    else
      acc += f64_of(xb) * d;
    pm = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    if (CONTRIB && pm >= cy) return true;
  }
  return false;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ void hv_rank_kernel(const float* __restrict__ vals, const int64_t* __restrict__ idx, int n, int m, int* __restrict__ zrank,
                               int* __restrict__ wrank, double* __restrict__ h, double* __restrict__ g) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (m == 2) {
    h[k] = k == 0 ? 1.0 : 0.0;
    return;
  }
  const float* vz = vals + (size_t)2 * n;
  zrank[idx[(size_t)2 * n + k]] = k;
  h[k] = (double)vz[k] - (k + 1 < n ? (double)vz[k + 1] : 0.0);
  if (m == 4) {
    const float* vw = vals + (size_t)3 * n;
    wrank[idx[(size_t)3 * n + k]] = k;
    g[k] = (double)vw[k] - (k + 1 < n ? (double)vw[k + 1] : 0.0);
  }
}

__global__ void hv_gather_kernel(const float* __restrict__ pT, const float* __restrict__ vals, const int64_t* __restrict__ idx, int n, int m,
                                 const int* __restrict__ zrank, const int* __restrict__ wrank, uint32_t* __restrict__ X,
                                 uint32_t* __restrict__ Y, uint32_t* __restrict__ ZW, int* __restrict__ orig) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int i = (int)idx[r];
  X[r] = __float_as_uint(vals[r]);
  Y[r] = __float_as_uint(pT[(size_t)n + i]);
  const uint32_t zr = m >= 3 ? (uint32_t)zrank[i] : 0u, wr = m == 4 ? (uint32_t)wrank[i] : 0u;
  ZW[r] = zr | (wr << 16);  // n ≤ 32768: a rank fits 16 bits
  orig[r] = i;
}

// TOTAL: nsl slices k (n at m = 3, 1 at m = 2), out[k] = h_k · A(zrank ≤ k).  CONTRIB (m = 2): nsl = n slices r,
// out[orig_r] = x_r·y_r − A(j ≠ r, clip (x_r, y_r)).
template <bool CONTRIB>
__global__ void __launch_bounds__(HV_THREADS)
    hv_flat_kernel(const uint32_t* __restrict__ X, const uint32_t* __restrict__ Y, const uint32_t* __restrict__ ZW, const int* __restrict__ orig,
                   const double* __restrict__ h, int n, int nsl, double* __restrict__ out) {
  __shared__ Tile tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x * HV_WAVES + wave;
  const bool live = s < nsl;
  uint32_t cx = 0, cy = 0;
  double hk = 0.0;
  if (live) {
    if (CONTRIB) {
      cx = X[s];
      cy = Y[s];
    } else {
      hk = h[s];
    }
  }
  bool run = live && (CONTRIB ? cy > 0u : hk > 0.0);
  uint32_t pm = 0;
  double acc = 0.0;
  for (int j0 = 0; j0 < n; j0 += HV_TILE) {
    const int w = min(HV_TILE, n - j0);
    __syncthreads();
    load_tile(tile, X, Y, ZW, j0, w);
    __syncthreads();
    if (run && scan_tile<CONTRIB>(tile, j0, w, lane, CONTRIB ? 0xffffu : (uint32_t)s, 0xffffu, CONTRIB ? s : -1, cx, cy, pm, acc)) run = false;
  }
  if (!live) return;
  acc = wave_sum(acc);
  if (lane != 0) return;
  if (CONTRIB)
    out[orig[s]] = f64_of(cx) * (f64_of(cy) - f64_of(pm)) + acc;  // pm ≤ cy: every y' was clipped to cy
  else
    out[s] = hk * acc;
}

// n ≤ HV_TILE.  TOTAL (m = 4): workgroup l, out[l] = g_l · Σ_k h_k · A(wrank ≤ l and zrank ≤ k).  CONTRIB (m = 3): workgroup r,
// out[orig_r] = Σ_{k ≥ zrank_r} h_k · (x_r·y_r − A(j ≠ r and zrank_j ≤ k, clip (x_r, y_r))).
template <bool CONTRIB>
__global__ void __launch_bounds__(HV_THREADS)
    hv_owned_kernel(const uint32_t* __restrict__ X, const uint32_t* __restrict__ Y, const uint32_t* __restrict__ ZW, const int* __restrict__ orig,
                    const double* __restrict__ h, const double* __restrict__ g, int n, double* __restrict__ out) {
  __shared__ Tile tile;
  __shared__ double wsum[HV_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  uint32_t cx = 0, cy = 0, kw = 0xffffu;
  int k0 = 0, skip = -1;
  double gl = 1.0;
  if (CONTRIB) {
    cx = X[b];
    cy = Y[b];
    k0 = (int)(ZW[b] & 0xffffu);
    skip = b;
  } else {
    gl = g[b];
    kw = (uint32_t)b;
  }
  const bool any = CONTRIB ? cy > 0u : gl > 0.0;  // the same for the whole workgroup
  if (any) load_tile(tile, X, Y, ZW, 0, n);
  __syncthreads();
  double sum = 0.0;
  if (any)
    for (int k = k0 + wave; k < n; k += HV_WAVES) {
      const double hk = h[k];
      if (!(hk > 0.0)) continue;
      uint32_t pm = 0;
      double acc = 0.0;
      scan_tile<CONTRIB>(tile, 0, n, lane, (uint32_t)k, kw, skip, cx, cy, pm, acc);
      acc = wave_sum(acc);
      if (CONTRIB) acc = f64_of(cx) * (f64_of(cy) - f64_of(pm)) + acc;
      sum += hk * acc;
    }
  if (lane == 0) wsum[wave] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot = 0.0;
  for (int v = 0; v < HV_WAVES; ++v) tot += wsum[v];
  out[CONTRIB ? orig[b] : b] = CONTRIB ? tot : gl * tot;
}

__global__ void __launch_bounds__(HV_THREADS) hv_reduce_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double part[HV_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += HV_THREADS) s += v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = HV_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = part[0];
}

void prepare(const float* pT, const float* vals, const int64_t* idx, int n, int m, int* zrank, int* wrank, double* h, double* g, uint32_t* X,
             uint32_t* Y, uint32_t* ZW, int* orig, hipStream_t s) {
  const int grid = (n + 255) / 256;
  hv_rank_kernel<<<grid, 256, 0, s>>>(vals, idx, n, m, zrank, wrank, h, g);
  hv_gather_kernel<<<grid, 256, 0, s>>>(pT, vals, idx, n, m, zrank, wrank, X, Y, ZW, orig);
}

}  // namespace

int evx_hv_owned_max_n() { return HV_TILE; }

void evx_hv_exact(const float* pT, const float* vals, const int64_t* idx, int n, int m, int* zrank, int* wrank, double* h, double* g,
                  uint32_t* X, uint32_t* Y, uint32_t* ZW, int* orig, double* scratch, double* out, hipStream_t s) {
  prepare(pT, vals, idx, n, m, zrank, wrank, h, g, X, Y, ZW, orig, s);
  const int nsl = m == 2 ? 1 : n;
  if (m == 4)
    hv_owned_kernel<false><<<n, HV_THREADS, 0, s>>>(X, Y, ZW, orig, h, g, n, scratch);
  else
    hv_flat_kernel<false><<<(nsl + HV_WAVES - 1) / HV_WAVES, HV_THREADS, 0, s>>>(X, Y, ZW, orig, h, n, nsl, scratch);
  hv_reduce_kernel<<<1, HV_THREADS, 0, s>>>(scratch, nsl, out);
}

void evx_hv_contributions(const float* pT, const float* vals, const int64_t* idx, int n, int m, int* zrank, int* wrank, double* h, double* g,
                          uint32_t* X, uint32_t* Y, uint32_t* ZW, int* orig, double* out, hipStream_t s) {
  prepare(pT, vals, idx, n, m, zrank, wrank, h, g, X, Y, ZW, orig, s);
  if (m == 3)
    hv_owned_kernel<true><<<n, HV_THREADS, 0, s>>>(X, Y, ZW, orig, h, g, n, out);
  else
    hv_flat_kernel<true><<<(n + HV_WAVES - 1) / HV_WAVES, HV_THREADS, 0, s>>>(X, Y, ZW, orig, h, n, n, out);
}
