// HypE's Monte-Carlo fitness (Bader & Zitzler 2011; reference algorithms/mo/hype.py:21-53) without a sample array:
//   f_i = Σ_s [p_i ≤ x_s in every objective] · α[c_s − 1],   c_s = #{i : p_i ≤ x_s},   terms with c_s = 0 dropping out,
// for the samples x_s = u_s · (ref − fmin) + fmin, where u = uniform(key, (n_sample, m)) and fmin is the column minimum of the points.
// The run is on grid.y: B runs (points (B, n, m), ref (B, m), key (B, 2), α (n) shared) cost the launches of one.
//
// Contract: f equals, bit for bit, hv_contrib(samples, points, hv_count(samples, points, false), α) of mo_geom.hip on the sample
// array that rng.hip would have written.  That fixes
//   * the samples: element s·m + k of the stream is word (s·m + k) & 3 of Philox block (s·m + k) >> 2 through u24, then
//     u · (ref_k − fmin_k) + fmin_k with two roundings (this file is compiled with -ffp-contract=off); fmin is a minimum, so exact,
//     and a NaN wins it as in torch;
//   * the order of the weighted sum: partial t (0 ≤ t < 256) adds the terms of s = t, t + 256, … in increasing s from 0.f, and
//     the 256 partials reduce by the tree o = 128, 64, …, 1 with red[t] += red[t + o].
//
// Two kernels, because the weight of a sample needs every point and the sum of a point needs every weight:
//   hype_weight_kernel   a thread per sample (256 per workgroup, sample chunks on grid.x).  It draws its sample in registers, walks the
//                        run's points in LDS (every lane reads the same point: broadcast reads, tiles of 4096 words) and writes
//                        the one float w_s = c_s > 0 ? α[c_s − 1] : 0.  The column minima come first, a wave per column straight
//                        from the points; chunk 0 leaves them behind the weights for the second kernel.
//   hype_contrib_kernel  a workgroup per kPts points of a run.  Thread t is partial t: it draws the samples t, t + 256, … again
//                        (no block of the stream is read from memory; the weights are, coalesced), tests each against the kPts
//                        points held in LDS and keeps kPts running sums in registers, so a drawn sample serves kPts chains.
//                        The kPts trees then run side by side in LDS.
// A sample of m words spans at most MM / 4 + 1 Philox blocks (MM the compiled bound on m); they are generated whole and the words
// are picked by the stream offset with selects, so no register array is indexed by a lane-varying value.
#include "evoxmi_common.h"

namespace {

constexpr int kThreads = 256;  // the partial count of the contract
constexpr int kTile = 4096;    // words of points per LDS tile in hype_weight_kernel
constexpr int kPts = 8;        // points per workgroup in hype_contrib_kernel
constexpr int kMaxM = 16, kMaxN = 2048, kMaxSamples = 1 << 20;

// sample s of the run: x[k] = u24(stream word s·m + k) · sc[k] + lo[k] for k < m
template <int MM>
__device__ __forceinline__ void draw_sample(float (&x)[MM], int s, int m, uint32_t k0, uint32_t k1, const float (&lo)[MM],
                                            const float (&sc)[MM]) {
  constexpr int NB = MM / 4 + 1;
  const uint32_t e0 = (uint32_t)s * (uint32_t)m;  // < 2^24: s < 2^20, m ≤ 16
  const uint32_t b0 = e0 >> 2, off = e0 & 3u;
  uint32_t w[4 * NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    evx::u4 b{0u, 0u, 0u, 0u};
    if (4 * j < m + 3) b = evx::philox_block((uint64_t)(b0 + j), k0, k1);  // wave-uniform: the last block any offset can reach
    w[4 * j] = b.x;
    w[4 * j + 1] = b.y;
    w[4 * j + 2] = b.z;
    w[4 * j + 3] = b.w;
  }
  // shift the words down by off in two stages (by 1, then by 2).  Bit selects (v_bfi_b32), not ?: on array elements: those the
  // compiler folds into one load at a lane-varying index, which puts w[] in scratch
  const uint32_t by1 = 0u - (off & 1u), by2 = 0u - ((off >> 1) & 1u);
  uint32_t h[MM + 2];
#pragma unroll
  for (int k = 0; k < MM + 2; ++k) h[k] = (w[k + 1] & by1) | (w[k] & ~by1);
#pragma unroll
  for (int k = 0; k < MM; ++k) {
    const uint32_t word = (h[k + 2] & by2) | (h[k] & ~by2);
    x[k] = k < m ? evx::u24(word) * sc[k] + lo[k] : 0.f;
  }
}

template <int MM>
__global__ void __launch_bounds__(kThreads) hype_weight_kernel(const float* __restrict__ P, const float* __restrict__ ref,
                                                              const float* __restrict__ alpha, const int64_t* __restrict__ key, int n,
                                                              int m, int ns, float* __restrict__ aux) {
  __shared__ float ps[kTile];
  __shared__ float fm[kMaxM];
  const int run = blockIdx.y, t = threadIdx.x;
  P += (int64_t)run * n * m;
  ref += (int64_t)run * m;
  key += 2 * (int64_t)run;
  aux += (int64_t)run * (ns + m);
  // column minima: wave w takes the columns w, w + 4, …
  for (int k = t >> 6; k < m; k += kThreads / 64) {
    float v = INFINITY;
    for (int i = t & 63; i < n; i += 64) v = evx::nan_min(v, P[(int64_t)i * m + k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = evx::nan_min(v, __shfl_xor(v, o, 64));
    if ((t & 63) == 0) fm[k] = v;
  }
  __syncthreads();
  if (blockIdx.x == 0 && t < m) aux[ns + t] = fm[t];
  float lo[MM], sc[MM], x[MM];
#pragma unroll
  for (int k = 0; k < MM; ++k) {
    lo[k] = k < m ? fm[k] : 0.f;
    sc[k] = k < m ? ref[k] - lo[k] : 0.f;
  }
  uint32_t k0, k1;
  evx::load_key(key, k0, k1);
  const int s = blockIdx.x * kThreads + t;
  draw_sample<MM>(x, s < ns ? s : 0, m, k0, k1, lo, sc);
  int c = 0;
  const int per = kTile / m;
  for (int i0 = 0; i0 < n; i0 += per) {
    const int nr = min(per, n - i0);
    if (i0 > 0) __syncthreads();
    for (int e = t; e < nr * m; e += kThreads) ps[e] = P[(int64_t)i0 * m + e];
    __syncthreads();
#pragma unroll 4  // four points' LDS reads in flight (a workgroup has one wave per SIMD); no measurable gain, profiles/NOTES.md
    for (int i = 0; i < nr; ++i) {
      const float* p = ps + i * m;
      bool dom = true;
#pragma unroll
      for (int k = 0; k < MM; ++k)
        if (k < m) dom = dom && (p[k] <= x[k]);
      c += dom ? 1 : 0;
    }
  }
  if (s < ns) aux[s] = c > 0 ? alpha[c - 1] : 0.f;
}

template <int MM>
__global__ void __launch_bounds__(kThreads) hype_contrib_kernel(const float* __restrict__ P, const float* __restrict__ ref,
                                                               const int64_t* __restrict__ key, const float* __restrict__ aux, int n,
                                                               int m, int ns, float* __restrict__ f) {
  __shared__ float pp[kPts * MM];
  __shared__ float red[kPts][kThreads];
  const int run = blockIdx.y, t = threadIdx.x, i0 = blockIdx.x * kPts;
  P += (int64_t)run * n * m;
  ref += (int64_t)run * m;
  key += 2 * (int64_t)run;
  aux += (int64_t)run * (ns + m);
  f += (int64_t)run * n;
  // this workgroup's points; a row past n is NaN, which is ≤ nothing
  if (t < kPts * MM) {
    const int p = t / MM, k = t - p * MM;
    pp[t] = (i0 + p < n && k < m) ? P[(int64_t)(i0 + p) * m + k] : NAN;
  }
  float lo[MM], sc[MM], x[MM];
#pragma unroll
  for (int k = 0; k < MM; ++k) {
    lo[k] = k < m ? aux[ns + k] : 0.f;
    sc[k] = k < m ? ref[k] - lo[k] : 0.f;
  }
  uint32_t k0, k1;
  evx::load_key(key, k0, k1);
  float acc[kPts];
#pragma unroll
  for (int p = 0; p < kPts; ++p) acc[p] = 0.f;
  __syncthreads();
  for (int s = t; s < ns; s += kThreads) {
    draw_sample<MM>(x, s, m, k0, k1, lo, sc);
    const float w = aux[s];
#pragma unroll
    for (int p = 0; p < kPts; ++p) {
      bool dom = true;
#pragma unroll
      for (int k = 0; k < MM; ++k)
        if (k < m) dom = dom && (pp[p * MM + k] <= x[k]);
      acc[p] += dom ? w : 0.f;
    }
  }
#pragma unroll
  for (int p = 0; p < kPts; ++p) red[p][t] = acc[p];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int p = 0; p < kPts; ++p) red[p][t] += red[p][t + o];
    }
    __syncthreads();
  }
  if (t < kPts && i0 + t < n) f[i0 + t] = red[t][0];
}

template <int MM>
void launch(const float* P, const float* ref, const float* alpha, const int64_t* key, int B, int n, int m, int ns, float* aux, float* f,
            hipStream_t s) {
  hype_weight_kernel<MM><<<dim3((ns + kThreads - 1) / kThreads, B), kThreads, 0, s>>>(P, ref, alpha, key, n, m, ns, aux);
  hype_contrib_kernel<MM><<<dim3((n + kPts - 1) / kPts, B), kThreads, 0, s>>>(P, ref, key, aux, n, m, ns, f);
}

}  // namespace

bool evx_hype_fused_ok(int64_t n, int64_t m, int64_t n_sample) {
  return n >= 1 && n <= kMaxN && m >= 1 && m <= kMaxM && n_sample >= 1 && n_sample <= kMaxSamples;
}

// aux: B · (n_sample + m) floats of scratch (the weights of a run, then its column minima)
void evx_hype_fitness(const float* P, const float* ref, const float* alpha, const int64_t* key, int B, int n, int m, int n_sample,
                      float* aux, float* f, hipStream_t s) {
  if (m <= 4) launch<4>(P, ref, alpha, key, B, n, m, n_sample, aux, f, s);
  else if (m <= 8) launch<8>(P, ref, alpha, key, B, n, m, n_sample, aux, f, s);
  else launch<16>(P, ref, alpha, key, B, n, m, n_sample, aux, f, s);
}
