// Device routines shared by the MOEA/D generation kernels (moead.hip: the chip-wide passes at the north-star shape;
// moead_small.hip: the per-run kernels of BatchedRuns).  One definition each, so a run of the small kernels draws
// the Philox words, aggregates and varies genes exactly as the solo launches do.
#pragma once
#include "evoxmi_common.h"

namespace evx {
namespace moead {

constexpr int MAXM = 16;

__device__ __forceinline__ uint32_t word_at(uint64_t i, uint32_t k0, uint32_t k1) {
  u4 w = philox_block(i >> 2, k0, k1);
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
  return ws[i & 3];
}

// 0 tchebycheff, 1 pbi (theta 5), 2 weighted sum, 3 modified tchebycheff, 4 normalised tchebycheff
__device__ __forceinline__ float agg(int func, const float* f, const float* w, const float* z, const float* zmax, int M) {
  if (func == 2) {
    float s = 0.f;
    for (int k = 0; k < M; ++k) s += f[k] * w[k];
    return s;
  }
  if (func == 1) {
    float nw = 0.f, d1 = 0.f;
    for (int k = 0; k < M; ++k) {
      nw += w[k] * w[k];
      d1 += (f[k] - z[k]) * w[k];
    }
    nw = sqrtf(nw);
    d1 /= nw;
    float d2 = 0.f;
    for (int k = 0; k < M; ++k) {
      const float r = f[k] - z[k] - d1 * w[k] / nw;
      d2 += r * r;
    }
    return d1 + 5.f * sqrtf(d2);
  }
  // fmaxf drops a NaN operand; the aggregate of a row with a NaN term is NaN (as amax in the
  // torch path and the sequential oracle), so such a row neither takes a slot nor loses one:
  // one flag per aggregate, not a NaN-aware max per term
  float g = -INFINITY;
  bool bad = false;
  for (int k = 0; k < M; ++k) {
    const float a = fabsf(f[k] - z[k]);
    float v;
    if (func == 3) v = a / w[k];
    else if (func == 4) v = a / (zmax[k] - z[k]) * w[k];
    else v = a * w[k];
    bad |= v != v;
    g = fmaxf(g, v);
  }
  return bad ? NAN : g;
}

__device__ __forceinline__ void min2_merge(uint64_t& a1, uint64_t& a2, uint64_t b1, uint64_t b2) {
  const uint64_t lo = a1 < b1 ? a1 : b1, hi = a1 < b1 ? b1 : a1;
  const uint64_t s = a2 < b2 ? a2 : b2;
  a1 = lo;
  a2 = hi < s ? hi : s;
}

// the two smallest (u24, j) keys of row `row` of uniform(key, (N, T)), one wave; every lane returns both
__device__ __forceinline__ void row_min2(uint64_t row, int T, uint32_t k0, uint32_t k1, uint64_t& m1, uint64_t& m2) {
  const int lane = threadIdx.x & 63;
  m1 = ~0ull;
  m2 = ~0ull;
  const uint64_t base = row * T;
  for (int j = lane; j < T; j += 64) {
    const uint64_t kv = ((uint64_t)(word_at(base + j, k0, k1) >> 8) << 32) | (uint32_t)j;
    if (kv < m1) { m2 = m1; m1 = kv; }
    else if (kv < m2) m2 = kv;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t b1 = __shfl_xor(m1, o, 64), b2 = __shfl_xor(m2, o, 64);
    min2_merge(m1, m2, b1, b2);
  }
}

struct VarKeys {
  uint32_t g0, g1, pr0, pr1;  // SBX: split(key_x, 2) → per-gene word, per-pair rate
  uint32_t st0, st1, pm0, pm1;  // PM:  split(key_m, 2) → site, mu
};

// keys live on the device (graph-capturable): uniform scalar loads at kernel start
__device__ __forceinline__ VarKeys load_keys(const int64_t* __restrict__ kx, const int64_t* __restrict__ km) {
  return VarKeys{(uint32_t)kx[0], (uint32_t)kx[1], (uint32_t)kx[2], (uint32_t)kx[3],
                 (uint32_t)km[0], (uint32_t)km[1], (uint32_t)km[2], (uint32_t)km[3]};
}

// SBX child from the per-gene word: μ = top 24 bits, bit 0 = sign of β, bit 1 = skip gene
__device__ __forceinline__ float sbx_child(float a, float b, uint32_t w, bool no_x, float e) {
  float beta = 1.f;
  if (!no_x && !(w & 2u)) {
    const float mu = u24(w);
    beta = mu <= 0.5f ? exp2f(e * __log2f(2.f * mu)) : exp2f(-e * __log2f(2.f - 2.f * mu));
    if (w & 1u) beta = -beta;
  }
  return 0.5f * (a + b) + beta * (0.5f * (a - b));
}

// PM at one gene; μ is drawn (one more Philox block) only at the rare mutation sites
__device__ __forceinline__ float pm_gene(float v, float lo, float hi, uint32_t wst, uint64_t t, const VarKeys& K, float pr, float e1,
                                         float inv) {
  v = fmaxf(fminf(v, hi), lo);
  if (u24(wst) < pr) {
    const float span = hi - lo;
    const float mu = u24(word_at(t, K.pm0, K.pm1));
    if (mu <= 0.5f) {
      const float nrm = (v - lo) / span;
      v = v + span * (powf(2.f * mu + (1.f - 2.f * mu) * powf(1.f - nrm, e1), inv) - 1.f);
    } else {
      const float nrm = (hi - v) / span;
      v = v + span * (1.f - powf(2.f * (1.f - mu) + 2.f * (mu - 0.5f) * powf(1.f - nrm, e1), inv));
    }
  }
  return v;
}

// offspring i, genes j .. j+3 (d % 4 == 0 ⇒ they share one Philox block per stream): SBX, PM for the rows below nm, clip
__device__ __forceinline__ float4 child4(float4 a, float4 b, float4 lo, float4 hi, uint64_t g0, bool pm_row, bool no_x, const VarKeys& K,
                                         float e, float pr, float e1, float inv) {
  const u4 w = philox_block(g0 >> 2, K.g0, K.g1);
  float4 y;
  y.x = sbx_child(a.x, b.x, w.x, no_x, e);
  y.y = sbx_child(a.y, b.y, w.y, no_x, e);
  y.z = sbx_child(a.z, b.z, w.z, no_x, e);
  y.w = sbx_child(a.w, b.w, w.w, no_x, e);
  if (pm_row) {
    const u4 ws = philox_block(g0 >> 2, K.st0, K.st1);
    y.x = pm_gene(y.x, lo.x, hi.x, ws.x, g0, K, pr, e1, inv);
    y.y = pm_gene(y.y, lo.y, hi.y, ws.y, g0 + 1, K, pr, e1, inv);
    y.z = pm_gene(y.z, lo.z, hi.z, ws.z, g0 + 2, K, pr, e1, inv);
    y.w = pm_gene(y.w, lo.w, hi.w, ws.w, g0 + 3, K, pr, e1, inv);
  }
  y.x = fmaxf(fminf(y.x, hi.x), lo.x);
  y.y = fmaxf(fminf(y.y, hi.y), lo.y);
  y.z = fmaxf(fminf(y.z, hi.z), lo.z);
  y.w = fmaxf(fminf(y.w, hi.w), lo.w);
  return y;
}

// offspring i, gene counter t = i·d + j
__device__ __forceinline__ float child1(float a, float b, float lo, float hi, uint64_t t, bool pm_row, bool no_x, const VarKeys& K, float e,
                                        float pr, float e1, float inv) {
  float y = sbx_child(a, b, word_at(t, K.g0, K.g1), no_x, e);
  if (pm_row) y = pm_gene(y, lo, hi, word_at(t, K.st0, K.st1), t, K, pr, e1, inv);
  return fmaxf(fminf(y, hi), lo);
}

}  // namespace moead
}  // namespace evx
