// Sorted-block refinement (SBR) of a warm-started symmetric eigendecomposition (K4):
// the residual statistics and the Taylor operand pass shared by the host driver
// (evoxmi/ops/sbr.py) and the device driver (evoxmi/ops/sbr_device.py).
//
//   sbr_stats_kernel        partials of ‖offdiag A‖², ‖diag A‖², min / max diag of A
//   sbr_symstats_kernel     A = (T + Tᵀ)/2 of T = Bᵀ C B and the same partials, one pass
//   sbr_stats_final_kernel  fixed-order reduction of the partials → [off², diag², dmin, dmax],
//                           read by the drivers' convergence / damping decisions
//   sbr_taylor_prep_kernel  the elementwise operands P, M of exp(αX) ≈ M + X³·P
// The block, far and Bq steps of an iteration (the block solves of the sorted diagonal, the
// rotation generator X, Bq = B[:, perm]·blockdiag(Q)) are in eigh_sbr16.hip.
#include "evoxmi_common.h"
#include <float.h>

namespace {

constexpr int kStatParts = 128;

// ------------------------------------------------------------------ stats
__global__ void __launch_bounds__(256) sbr_stats_kernel(const float* __restrict__ A, int n, int64_t lda, double* __restrict__ part) {
  __shared__ double s_off[256], s_dg[256];
  __shared__ float s_mn[256], s_mx[256];
  double off = 0.0, dg = 0.0;
  float mn = FLT_MAX, mx = -FLT_MAX;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const float* row = A + (int64_t)r * lda;
    float acc = 0.f;
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
      float v = row[c];
      if (c == r) {
        dg += (double)v * v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
      } else {
        acc = fmaf(v, v, acc);
      }
    }
    off += acc;
  }
  s_off[threadIdx.x] = off;
  s_dg[threadIdx.x] = dg;
  s_mn[threadIdx.x] = mn;
  s_mx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      s_off[threadIdx.x] += s_off[threadIdx.x + o];
      s_dg[threadIdx.x] += s_dg[threadIdx.x + o];
      s_mn[threadIdx.x] = fminf(s_mn[threadIdx.x], s_mn[threadIdx.x + o]);
      s_mx[threadIdx.x] = fmaxf(s_mx[threadIdx.x], s_mx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[4 * blockIdx.x + 0] = s_off[0];
    part[4 * blockIdx.x + 1] = s_dg[0];
    part[4 * blockIdx.x + 2] = s_mn[0];
    part[4 * blockIdx.x + 3] = s_mx[0];
  }
}

// fixed-order tree reduction of `nparts` partials (deterministic); out = [off², diag², dmin, dmax]
__global__ void __launch_bounds__(256) sbr_stats_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
  __shared__ double s[4][256];
  const int t = threadIdx.x;
  double off = 0.0, dg = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
  for (int i = t; i < nparts; i += 256) {
    off += part[4 * i];
    dg += part[4 * i + 1];
    mn = fmin(mn, part[4 * i + 2]);
    mx = fmax(mx, part[4 * i + 3]);
  }
  s[0][t] = off;
  s[1][t] = dg;
  s[2][t] = mn;
  s[3][t] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      s[0][t] += s[0][t + o];
      s[1][t] += s[1][t + o];
      s[2][t] = fmin(s[2][t], s[2][t + o]);
      s[3][t] = fmax(s[3][t], s[3][t + o]);
    }
    __syncthreads();
  }
  if (t < 4) out[t] = s[t][0];
}

// A = (T + Tᵀ)/2 and its stats partials, one 64×64 tile per workgroup (the mirrored tile is
// read through LDS so both global reads are row-contiguous)
__global__ void __launch_bounds__(256) sbr_symstats_kernel(const float* __restrict__ T, int n, int64_t ldt, float* __restrict__ A,
                                                           int64_t lda, double* __restrict__ part) {
  __shared__ float M[64][65];
  __shared__ double r_off[256], r_dg[256];
  __shared__ float r_mn[256], r_mx[256];
  const int bi = blockIdx.y, bj = blockIdx.x;
  // mirrored tile T[bj-block rows][bi-block cols] → M (row-contiguous loads)
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;
    const int gr = bj * 64 + r, gc = bi * 64 + c;
    M[r][c] = (gr < n && gc < n) ? T[(int64_t)gr * ldt + gc] : 0.f;
  }
  __syncthreads();
  double off = 0.0, dg = 0.0;
  float mn = FLT_MAX, mx = -FLT_MAX;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;
    const int gr = bi * 64 + r, gc = bj * 64 + c;
    if (gr < n && gc < n) {
      const float v = 0.5f * (T[(int64_t)gr * ldt + gc] + M[c][r]);
      A[(int64_t)gr * lda + gc] = v;
      if (gr == gc) {
        dg += (double)v * v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
      } else {
        off += (double)v * v;
      }
    }
  }
  const int t = threadIdx.x;
  r_off[t] = off;
  r_dg[t] = dg;
  r_mn[t] = mn;
  r_mx[t] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      r_off[t] += r_off[t + o];
      r_dg[t] += r_dg[t + o];
      r_mn[t] = fminf(r_mn[t], r_mn[t + o]);
      r_mx[t] = fmaxf(r_mx[t], r_mx[t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const int64_t b = (int64_t)bi * gridDim.x + bj;
    part[4 * b + 0] = r_off[0];
    part[4 * b + 1] = r_dg[0];
    part[4 * b + 2] = r_mn[0];
    part[4 * b + 3] = r_mx[0];
  }
}

// Taylor terms of exp(αX) (α: damping factor on the device, 1 if null):
// P = α³(Y/24 + Y²/120 + Y³/720), M = I + Y + Y²/2 + Y³/6 with Y = αX, so that
// exp(αX) ≈ M + X³·P (one pass; X³·P carries the α³ of Y³)
// mt = 1: M of exp(−αX) = exp(αX)ᵀ (odd terms negated) — with P unchanged the transposed
// product Vᵀ = M(−α) − X³·Pᵀ is an A·Bᵀ GEMM on P's rows (ops/sbr.py)
__global__ void __launch_bounds__(256) sbr_taylor_prep_kernel(const float* __restrict__ X, const float* __restrict__ X2,
                                                              const float* __restrict__ X3, int n, const float* __restrict__ alpha,
                                                              float* __restrict__ P, float* __restrict__ M, int mt) {
  const float a = alpha ? alpha[0] : 1.f, a2 = a * a, a3 = a2 * a;
  const float so = mt ? -1.f : 1.f;
  const int64_t total = (int64_t)n * n;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const float x = a * X[e], x2 = a2 * X2[e], x3 = a3 * X3[e];
    P[e] = a3 * (x * (1.f / 24.f) + x2 * (1.f / 120.f) + x3 * (1.f / 720.f));
    const int64_t i = e / n, j = e - i * n;
    M[e] = (i == j ? 1.f : 0.f) + so * x + 0.5f * x2 + so * x3 * (1.f / 6.f);
  }
}

}  // namespace

void evx_sbr_stats(const float* A, int n, int64_t lda, double* part, double* out, hipStream_t s) {
  sbr_stats_kernel<<<kStatParts, 256, 0, s>>>(A, n, lda, part);
  sbr_stats_final_kernel<<<1, 256, 0, s>>>(part, kStatParts, out);
}

int evx_sbr_stat_parts() { return kStatParts; }

int evx_sbr_symstats_parts(int n) {
  const int nt = (n + 63) / 64;
  return nt * nt;
}

void evx_sbr_symstats(const float* T, int n, int64_t ldt, float* A, int64_t lda, double* part, double* out, hipStream_t s) {
  const int nt = (n + 63) / 64;
  sbr_symstats_kernel<<<dim3(nt, nt), 256, 0, s>>>(T, n, ldt, A, lda, part);
  sbr_stats_final_kernel<<<1, 256, 0, s>>>(part, nt * nt, out);
}

void evx_sbr_taylor_prep(const float* X, const float* X2, const float* X3, int n, const float* alpha, float* P, float* M,
                         hipStream_t s, int mt) {
  const int64_t total = (int64_t)n * n;
  int g = (int)((total + 255) / 256);
  if (g > 2048) g = 2048;
  sbr_taylor_prep_kernel<<<g, 256, 0, s>>>(X, X2, X3, n, alpha, P, M, mt);
}
