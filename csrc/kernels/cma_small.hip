// CMA-ES at benchmark dimensions (d ≤ 64, λ ≤ 1024): a whole generation in two launches, one run
// per workgroup, R independent runs in one launch (BatchedRuns; R = 1 is a single optimiser).
// Everything is float32, deterministic (fixed summation orders, no float atomics) and stays on
// the device.
//
// cma_small_ask — grid (⌈λ/32⌉, R), 256 threads.  x[i, :] = mean + σ · (B∘D) · z[i, :].
//   * The workgroup stages (B∘D)ᵀ once in LDS, k-major: sBD[k·d + j] = B[j, k]·D[k], so lane j of
//     a wave reads consecutive words for every k (no bank conflict).
//   * A wave owns one population row at a time (rows wave, wave + 4, … of the workgroup's 32).
//     Lane k < d draws z[i, k]: element i·d + k of the run's normal stream — component (i·d + k) & 3
//     of normal4(philox_block((i·d + k) >> 2)), the value philox_fill(key, λ·d, 1, 0) holds there.
//     z lives in one register per lane and is never written to memory.
//   * Lane j < d then owns column j: acc = Σ_k sBD[k][j]·z_k in ascending k (one FMA chain), z_k
//     read from lane k (v_readlane, k is wave-uniform); x = mean[j] + σ·acc.
//
// cma_small_tell — grid R, 256 threads (4 waves), the whole of CMAES.tell for one run.  Three
// 64 × 65 LDS matrices M0, M1, M2 (pitch 65: row-wise and column-wise walks are both conflict-free)
// carry, in turn, invsqrtC / C' / A, B, and the y chunk / Cs·B / B∘D⁻¹.
//   1. rank: fitness in LDS; thread i counts the keys (value, index) below its own — an equal value
//      goes to the lower index, −0 = +0, NaN after every number (the order of argsort_i32) — and the
//      μ best write their index to sel[rank].
//   2. wave 0, lane j < d: dm_j = Σ_r w_r·(x[sel[r], j] − m_j) in rank order r = 0 … μ−1 (FMA chain),
//      mean' = m + cm·dm, δ = mean' − m, (invsqrtC·δ)_j = Σ_k M0[j][k]·δ_k in ascending k (δ_k by
//      v_readlane), p_σ, ‖p_σ‖ (xor-butterfly wave sum), hσ, p_c, σ', a — the formulas of
//      CMAES._finish_tell, count_iter as ask left it.
//   3. rank-μ sum: the selected rows stream from global memory in chunks of 64 (y = (x − m)/σ into
//      M2); thread (wave w, lane b) owns S[a, b] for a = w, w + 4, … and adds (w_r·y_ra)·y_rb in
//      rank order r = 0 … μ−1, one FMA per term.  C' = (a·C + c1·p_c p_cᵀ) + cμ·S.
//   4. when count_iter % decomp_per_iter == 0: Cs = triu(C') + triu(C', 1)ᵀ, T = Cs·B, A = Bᵀ·T
//      (sums in ascending k), A ← (A + Aᵀ)/2, then cyclic parallel Jacobi on the n × n matrix (n = d
//      rounded up to even; the extra item is a zero row/column, whose rotations are the identity):
//        * round r of a sweep pairs position i with position n−1−i of the circle method (item 0
//          fixed, the others rotate by r), n/2 disjoint rotations;
//        * thread t owns the 2 × 2 blocks (pair k, pair l) with k·n/2 + l = t, t + 256, …  It reads
//          the blocks' four words, the two B rows 2k, 2k+1 at columns (p_l, q_l) and the diagonal
//          blocks of pairs k and l, computes (c, s) of both pairs (rot_params of eigh_jacobi.hip)
//          and applies the column rotation l, then the row rotation k, in registers.  Barrier;
//          every word is written back by its one owner; barrier.  Two barriers per round.
//        * pitch 65 ≡ 1 modulo the bank count (32 or 64), so the bank of A[p][q] is p + q: the two rows
//          and the two columns of a rotated pair differ in bank, and the lanes that share a row pair
//          read distinct columns.
//      A sweep in which no pair had |a_pq| > 2⁻²⁴·sqrt(|a_pp·a_qq|) ends the solve; at most
//      CS_MAX_SWEEPS sweeps.  Converged: D = sqrt(max(diag A, 1e-30)), invsqrtC = (B/D)·Bᵀ (ascending
//      k), count_eigen + 1; eigenvalues keep the order the warm start carries.  Capped: the old B, D,
//      invsqrtC and count_eigen go out unchanged and the capped word is set.
#include "evoxmi_common.h"
#include "evoxmi_launchers.h"

namespace {
using namespace evx;

constexpr int CS_MAX_D = 64;
constexpr int CS_MAX_LAM = 1024;
constexpr int CS_P = 65;
constexpr int CS_THREADS = 256;
constexpr int CS_ASK_ROWS = 32;
constexpr int CS_MAX_SWEEPS = 32;

__device__ __forceinline__ float lane_read(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

__global__ void __launch_bounds__(CS_THREADS) cma_small_ask_kernel(const int64_t* __restrict__ key, const float* __restrict__ mean,
                                                                   const float* __restrict__ sigma, const float* __restrict__ B,
                                                                   const float* __restrict__ D, float* __restrict__ x, int lam, int d) {
  __shared__ float sBD[CS_MAX_D * CS_MAX_D];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  key += 2 * (int64_t)r;
  mean += (int64_t)r * d;
  B += (int64_t)r * d * d;
  D += (int64_t)r * d;
  x += (int64_t)r * lam * d;
  for (int e = tid; e < d * d; e += CS_THREADS) {
    const int j = e / d, k = e - j * d;
    sBD[k * d + j] = B[e] * D[k];
  }
  __syncthreads();
  uint32_t k0, k1;
  load_key(key, k0, k1);
  const float sig = sigma[r];
  const bool own = lane < d;
  const int jc = own ? lane : d - 1;
  const float mj = mean[jc];
  const int row0 = blockIdx.x * CS_ASK_ROWS;
  const int row1 = min(lam, row0 + CS_ASK_ROWS);
  for (int i = row0 + wave; i < row1; i += CS_THREADS / 64) {
    float z = 0.f;
    if (own) {
      const uint32_t e = (uint32_t)i * (uint32_t)d + (uint32_t)lane;  // < 2^16
      const float4 n4 = normal4(philox_block((uint64_t)(e >> 2), k0, k1));
      const int q = (int)(e & 3u);
      z = q == 0 ? n4.x : (q == 1 ? n4.y : (q == 2 ? n4.z : n4.w));
    }
    float acc = 0.f;
    for (int k = 0; k < d; ++k) acc = fmaf(sBD[k * d + jc], lane_read(z, k), acc);
    if (own) x[(int64_t)i * d + lane] = mj + sig * acc;
  }
}

struct SmallConsts {
  float cs, c_ps, cc, c_pc, chiN, damps, c1, cmu, hs_thresh, cm;
};

struct TellIn {
  const float *population, *fitness, *mean, *sigma, *ps, *pc, *C, *B, *D, *invsqrtC, *weights;
  const int64_t *count_iter, *count_eigen;
  const double* eig_stats;
};
struct TellOut {
  float *mean, *ps, *pc, *sigma, *C, *B, *D, *invsqrtC;
  int64_t* count_eigen;
  double* eig_stats;
};

// circle method on n items (n even): the item at position i in round r
__device__ __forceinline__ int circle_item(int i, int r, int nm1) {
  if (i == 0) return 0;
  int x = i - 1 + r;  // < 2(n−1)
  if (x >= nm1) x -= nm1;
  return x + 1;
}

// eigh_jacobi.hip's rot_params
__device__ __forceinline__ void rot_params(float app, float aqq, float apq, float& c, float& s) {
  c = 1.f;
  s = 0.f;
  if (apq != 0.f) {
    float tau = (aqq - app) / (2.f * apq);
    float t = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(fmaf(tau, tau, 1.f)));
    c = rsqrtf(fmaf(t, t, 1.f));
    s = t * c;
  }
}

__global__ void __launch_bounds__(CS_THREADS) cma_small_tell_kernel(const TellIn in, const TellOut out, const SmallConsts k, int lam, int d,
                                                                    int mu, int decomp_per_iter) {
  __shared__ float M0[CS_MAX_D * CS_P], M1[CS_MAX_D * CS_P], M2[CS_MAX_D * CS_P];
  __shared__ float fit[CS_MAX_LAM];
  __shared__ int sel[CS_MAX_LAM];
  __shared__ float vpc[CS_MAX_D], vD[CS_MAX_D], vw[64], scal[2], red[8];

  const int run = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t od = (int64_t)run * d, odd = (int64_t)run * d * d;
  const float* X = in.population + (int64_t)run * lam * d;
  const float* fitness = in.fitness + (int64_t)run * lam;
  const float* mean = in.mean + od;
  const float sig = in.sigma[run];
  const int64_t count_iter = in.count_iter[run];
  const bool own = lane < d;
  const int jc = own ? lane : d - 1;

  // ---- stage: fitness, invsqrtC → M0, B → M1, zero padding everywhere else
  for (int i = tid; i < lam; i += CS_THREADS) fit[i] = fitness[i];
  for (int e = tid; e < CS_MAX_D * CS_P; e += CS_THREADS) {
    M0[e] = 0.f;
    M1[e] = 0.f;
    M2[e] = 0.f;
  }
  __syncthreads();
  for (int i = wave; i < d; i += 4)
    if (own) {
      M0[i * CS_P + lane] = in.invsqrtC[odd + i * d + lane];
      M1[i * CS_P + lane] = in.B[odd + i * d + lane];
    }
  // ---- 1. rank by counting on (value, index); NaN last
  for (int i = tid; i < lam; i += CS_THREADS) {
    const float fi = fit[i];
    const bool nan_i = fi != fi;
    int cnt = 0;
    for (int j = 0; j < lam; ++j) {
      const float fj = fit[j];
      const bool less = nan_i ? (fj == fj || j < i) : (fj < fi || (fj == fi && j < i));
      cnt += less ? 1 : 0;
    }
    if (cnt < mu) sel[cnt] = i;
  }
  __syncthreads();

  // ---- 2. mean shift, evolution paths, σ, blend factor (wave 0)
  const float mj = mean[jc];
  if (wave == 0) {
    float dm = 0.f;
    for (int r = 0; r < mu; ++r) dm = fmaf(in.weights[r], X[(int64_t)sel[r] * d + jc] - mj, dm);
    const float mn = mj + k.cm * dm;
    const float delta = mn - mj;
    float zz = 0.f;
    for (int c = 0; c < d; ++c) zz = fmaf(M0[jc * CS_P + c], lane_read(delta, c), zz);
    const float psn = (1.f - k.cs) * in.ps[od + jc] + k.c_ps * zz / sig;
    const float nrm = sqrtf(wave_sum(own ? psn * psn : 0.f));
    const float hs = (nrm / sqrtf(1.f - powf(1.f - k.cs, 2.f * (float)count_iter)) < k.hs_thresh) ? 1.f : 0.f;
    const float pcn = (1.f - k.cc) * in.pc[od + jc] + hs * k.c_pc * delta / sig;
    if (own) {
      out.mean[od + lane] = mn;
      out.ps[od + lane] = psn;
      out.pc[od + lane] = pcn;
      vpc[lane] = pcn;
    }
    if (lane == 0) {
      out.sigma[run] = sig * expf((k.cs / k.damps) * (nrm / k.chiN - 1.f));
      scal[0] = (1.f - k.c1 - k.cmu) + k.c1 * (1.f - hs) * k.cc * (2.f - k.cc);
    }
  }

  // ---- 3. S = Σ_r w_r y_r y_rᵀ, rows streamed in chunks of 64; thread (wave, lane) owns S[wave + 4u][lane]
  float acc[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) acc[u] = 0.f;
  for (int c0 = 0; c0 < mu; c0 += 64) {
    const int nc = min(64, mu - c0);
    for (int c = wave; c < nc; c += 4)
      if (own) M2[c * CS_P + lane] = (X[(int64_t)sel[c0 + c] * d + lane] - mj) / sig;
    if (tid < nc) vw[tid] = in.weights[c0 + tid];
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      const float wc = vw[c], yb = M2[c * CS_P + lane];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u] = fmaf(wc * M2[c * CS_P + wave + 4 * u], yb, acc[u]);
    }
    __syncthreads();  // also: wave 0 is past its reads of M0 (invsqrtC), vpc and scal are written
  }
  {
    const float af = scal[0];
    const float pcb = vpc[jc];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int a = wave + 4 * u;
      if (a < d && own) {
        const float v = (af * in.C[odd + a * d + lane] + k.c1 * (vpc[a] * pcb)) + k.cmu * acc[u];
        out.C[odd + a * d + lane] = v;
        M0[a * CS_P + lane] = v;
      }
    }
  }
  const bool decomp = (count_iter % (int64_t)decomp_per_iter) == 0;  // workgroup-uniform
  bool keep_old = !decomp;
  float off_rel = 0.f;
  int sweeps = 0;
  if (decomp) {
    __syncthreads();
    // ---- 4. Cs = triu(C') + triu(C', 1)ᵀ (the strictly lower words are written, the upper ones only read)
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int a = wave + 4 * u;
      if (a < d && own && a > lane) M0[a * CS_P + lane] = M0[lane * CS_P + a];
    }
    __syncthreads();
    // T = Cs·B → M2
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = 0.f;
    for (int c = 0; c < d; ++c) {
      const float bk = M1[c * CS_P + lane];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u] = fmaf(M0[(wave + 4 * u) * CS_P + c], bk, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) M2[(wave + 4 * u) * CS_P + lane] = acc[u];  // zero outside d × d: the operands' padding is zero
    __syncthreads();
    // A = Bᵀ·T → M0
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = 0.f;
    for (int c = 0; c < d; ++c) {
      const float tk = M2[c * CS_P + lane];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u] = fmaf(M1[c * CS_P + wave + 4 * u], tk, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) M0[(wave + 4 * u) * CS_P + lane] = acc[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = 0.5f * (M0[(wave + 4 * u) * CS_P + lane] + M0[lane * CS_P + wave + 4 * u]);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) M0[(wave + 4 * u) * CS_P + lane] = acc[u];
    __syncthreads();

    // cyclic parallel Jacobi on A (M0) and B (M1)
    const int n = (d + 1) & ~1, m = n >> 1, mm = m * m, nm1 = n - 1;
    int bk_[4], bl_[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int blk = tid + CS_THREADS * u;
      bk_[u] = blk < mm ? blk / m : -1;
      bl_[u] = blk < mm ? blk - (blk / m) * m : 0;
    }
    bool converged = false;
    for (int sweep = 0; sweep < CS_MAX_SWEEPS && !converged; ++sweep) {
      int flag = 0;
      for (int r = 0; r < nm1; ++r) {
        float oa[4][4], ob[4][4];
        int pk[4], qk[4], pl[4], ql[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (bk_[u] < 0) continue;
          const int kk = bk_[u], ll = bl_[u];
          pk[u] = circle_item(kk, r, nm1);
          qk[u] = circle_item(nm1 - kk, r, nm1);
          pl[u] = circle_item(ll, r, nm1);
          ql[u] = circle_item(nm1 - ll, r, nm1);
          const float alp = M0[pl[u] * CS_P + pl[u]], alq = M0[ql[u] * CS_P + ql[u]], alo = M0[pl[u] * CS_P + ql[u]];
          float cl, sl, ck, sk;
          rot_params(alp, alq, alo, cl, sl);
          if (kk == ll) {
            ck = cl;
            sk = sl;
            if (fabsf(alo) > 5.9604644775390625e-8f * sqrtf(fabsf(alp * alq))) flag = 1;
          } else {
            rot_params(M0[pk[u] * CS_P + pk[u]], M0[qk[u] * CS_P + qk[u]], M0[pk[u] * CS_P + qk[u]], ck, sk);
          }
          const float x00 = M0[pk[u] * CS_P + pl[u]], x01 = M0[pk[u] * CS_P + ql[u]];
          const float x10 = M0[qk[u] * CS_P + pl[u]], x11 = M0[qk[u] * CS_P + ql[u]];
          // column rotation l, then row rotation k
          const float y00 = x00 * cl - x01 * sl, y01 = x00 * sl + x01 * cl;
          const float y10 = x10 * cl - x11 * sl, y11 = x10 * sl + x11 * cl;
          oa[u][0] = ck * y00 - sk * y10;
          oa[u][1] = ck * y01 - sk * y11;
          oa[u][2] = sk * y00 + ck * y10;
          oa[u][3] = sk * y01 + ck * y11;
          if (kk == ll) {
            oa[u][1] = 0.f;
            oa[u][2] = 0.f;
          }
          const int r0 = 2 * kk, r1 = 2 * kk + 1;
          const float v0a = M1[r0 * CS_P + pl[u]], v0b = M1[r0 * CS_P + ql[u]];
          const float v1a = M1[r1 * CS_P + pl[u]], v1b = M1[r1 * CS_P + ql[u]];
          ob[u][0] = v0a * cl - v0b * sl;
          ob[u][1] = v0a * sl + v0b * cl;
          ob[u][2] = v1a * cl - v1b * sl;
          ob[u][3] = v1a * sl + v1b * cl;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (bk_[u] < 0) continue;
          const int r0 = 2 * bk_[u], r1 = r0 + 1;
          M0[pk[u] * CS_P + pl[u]] = oa[u][0];
          M0[pk[u] * CS_P + ql[u]] = oa[u][1];
          M0[qk[u] * CS_P + pl[u]] = oa[u][2];
          M0[qk[u] * CS_P + ql[u]] = oa[u][3];
          M1[r0 * CS_P + pl[u]] = ob[u][0];
          M1[r0 * CS_P + ql[u]] = ob[u][1];
          M1[r1 * CS_P + pl[u]] = ob[u][2];
          M1[r1 * CS_P + ql[u]] = ob[u][3];
        }
        __syncthreads();
      }
      ++sweeps;
      converged = __syncthreads_or(flag) == 0;
    }
    keep_old = !converged;

    // relative off-norm of the last A
    float off = 0.f, dia = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int a = wave + 4 * u;
      if (a < d && own) {
        const float v = M0[a * CS_P + lane];
        if (a == lane) dia += v * v; else off += v * v;
      }
    }
    off = wave_sum(off);
    dia = wave_sum(dia);
    if (lane == 0) {
      red[wave] = off;
      red[4 + wave] = dia;
    }
    __syncthreads();
    off = (red[0] + red[1]) + (red[2] + red[3]);
    dia = (red[4] + red[5]) + (red[6] + red[7]);
    off_rel = sqrtf(off / dia);

    if (converged) {
      if (tid < d) {
        const float dj = sqrtf(fmaxf(M0[tid * CS_P + tid], 1e-30f));
        vD[tid] = dj;
        out.D[od + tid] = dj;
      }
      __syncthreads();
      const float dl = vD[jc];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int a = wave + 4 * u;
        if (a < d && own) {
          const float b = M1[a * CS_P + lane];
          out.B[odd + a * d + lane] = b;
          M2[a * CS_P + lane] = b / dl;
        }
      }
      __syncthreads();
      // invsqrtC = (B/D)·Bᵀ
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u] = 0.f;
      for (int c = 0; c < d; ++c) {
        const float bj = M1[jc * CS_P + c];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] = fmaf(M2[(wave + 4 * u) * CS_P + c], bj, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int a = wave + 4 * u;
        if (a < d && own) out.invsqrtC[odd + a * d + lane] = acc[u];
      }
    }
  }
  if (keep_old) {
    for (int e = tid; e < d * d; e += CS_THREADS) {
      out.B[odd + e] = in.B[odd + e];
      out.invsqrtC[odd + e] = in.invsqrtC[odd + e];
    }
    if (tid < d) out.D[od + tid] = in.D[od + tid];
  }
  if (tid == 0) {
    out.count_eigen[run] = in.count_eigen[run] + ((decomp && !keep_old) ? 1 : 0);
    double* es = out.eig_stats + 4 * (int64_t)run;
    if (decomp) {
      es[0] = (double)off_rel;
      es[1] = (double)sweeps;
      es[2] = 0.0;
      es[3] = keep_old ? 1.0 : 0.0;
    } else {
      const double* ei = in.eig_stats + 4 * (int64_t)run;
      for (int q = 0; q < 4; ++q) es[q] = ei[q];
    }
  }
}

}  // namespace

int evx_cma_small_max_d() { return CS_MAX_D; }
int evx_cma_small_max_lambda() { return CS_MAX_LAM; }

void evx_cma_small_ask(const int64_t* key, const float* mean, const float* sigma, const float* B, const float* D, float* x, int R, int lam,
                       int d, hipStream_t s) {
  if (R < 1 || R > EVX_MAX_RUNS || d < 1 || d > CS_MAX_D || lam < 1 || lam > CS_MAX_LAM) return;
  const dim3 grid((unsigned)((lam + CS_ASK_ROWS - 1) / CS_ASK_ROWS), (unsigned)R);
  cma_small_ask_kernel<<<grid, CS_THREADS, 0, s>>>(key, mean, sigma, B, D, x, lam, d);
}

void evx_cma_small_tell(const EvxCmaSmallTell& a, int R, int lam, int d, int mu, const float* consts, int decomp_per_iter, hipStream_t s) {
  if (R < 1 || R > EVX_MAX_RUNS || d < 1 || d > CS_MAX_D || lam < 1 || lam > CS_MAX_LAM || mu < 1 || mu > lam || decomp_per_iter < 1) return;
  const TellIn in{a.population, a.fitness, a.mean, a.sigma, a.ps, a.pc, a.C, a.B, a.D, a.invsqrtC, a.weights, a.count_iter, a.count_eigen,
                  a.eig_stats};
  const TellOut out{a.mean_out, a.ps_out, a.pc_out, a.sigma_out, a.C_out, a.B_out, a.D_out, a.invsqrtC_out, a.count_eigen_out,
                    a.eig_stats_out};
  const SmallConsts k{consts[0], consts[1], consts[2], consts[3], consts[4], consts[5], consts[6], consts[7], consts[8], consts[9]};
  cma_small_tell_kernel<<<(unsigned)R, CS_THREADS, 0, s>>>(in, out, k, lam, d, mu, decomp_per_iter);
}
