// Device helpers shared by the sorted-block-refinement kernels (eigh_sbr16.hip, eigh_sbr_dev.hip).
#pragma once
#include "evoxmi_common.h"
#include <float.h>
#include <math.h>

#include <cstdint>

// α = min(1, τ / sqrt(max_c ‖V3_c‖ / ‖V2_c‖)) of the power-step vectors, reduced by one
// 256-thread workgroup (every workgroup that calls it computes the same bits)
__device__ __forceinline__ float evx_sbr_damping_alpha(const float* __restrict__ V2, const float* __restrict__ V3, int n, float tau) {
  __shared__ float red[2][8][4];
  __shared__ float out;
  float s2[8] = {}, s3[8] = {};
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float a = V2[(int64_t)j * 8 + c], b = V3[(int64_t)j * 8 + c];
      s2[c] = fmaf(a, a, s2[c]);
      s3[c] = fmaf(b, b, s3[c]);
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    s2[c] = evx::wave_sum(s2[c]);
    s3[c] = evx::wave_sum(s3[c]);
    if (lane == 0) {
      red[0][c][w] = s2[c];
      red[1][c][w] = s3[c];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float lam = 0.f;
    for (int c = 0; c < 8; ++c) {
      const float a = red[0][c][0] + red[0][c][1] + red[0][c][2] + red[0][c][3];
      const float b = red[1][c][0] + red[1][c][1] + red[1][c][2] + red[1][c][3];
      lam = fmaxf(lam, sqrtf(b) / fmaxf(sqrtf(a), 1e-30f));
    }
    out = fminf(1.f, tau / sqrtf(fmaxf(lam, 1e-30f)));
  }
  __syncthreads();
  return out;
}


// Bounds of ‖X‖₂² for the skew generator X from the stats partials of its X² = −X·Xᵀ GEMM
// (gemm_ks MODE 1: per workgroup [Σ offdiag², Σ diag², min diag, max diag]): the diagonal of X²
// is −‖row_i‖², so max_i ‖row_i‖² = −min diag ≤ ‖X‖₂² ≤ ‖X‖_F² = −Σ diag ≤ sqrt(n · Σ diag²).
// Free — the GEMM's epilogue computed them — and every workgroup that calls it gets the same bits.
__device__ __forceinline__ float2 evx_sbr_xbounds(const double* __restrict__ part, int nparts, int n) {
  __shared__ double red[2][4];
  __shared__ float2 out;
  double s = 0.0, mn = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    s += part[4 * i + 1];
    mn = fmin(mn, part[4 * i + 2]);
  }
  s = evx::wave_sum_d(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o));
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = mn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0, m = 0.0;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) {
      t += red[0][w];
      m = fmin(m, red[1][w]);
    }
    out = make_float2((float)(-m), (float)sqrt((double)n * t));  // (lower, upper) bound of ‖X‖₂²
  }
  __syncthreads();
  return out;
}

// Whether the damping's power iteration runs for a far step (control word c2 of the device
// schedule: 0 the κ rule asked for it, 2 the bounds decide, else skipped): never when the
// upper bound proves ‖X‖₂ ≤ τ (α = 1 exact); with c2 = 2 only when some row of X is longer
// than τ/2 (the lower bound), where an undamped step is at risk
__device__ __forceinline__ bool evx_sbr_damp_runs(int c2, float2 b, float tau2) {
  if (c2 == 0) return !(b.y <= tau2);
  if (c2 == 2) return b.x > 0.25f * tau2 && !(b.y <= tau2);
  return false;
}

// ------------------------------------------------------------------ ranks → shifted perm
// Body of sbr16_rank_kernel (eigh_sbr16.hip), also run by the ranking workgroups of the device
// schedule's fused control + rank launch (eigh_sbr_dev.hip).  64 indices per workgroup; its 16
// waves each count over a sixteenth of the keys (16 waves: the counting loop is 4× shorter than
// with 4, and the launch stays at ⌈n/64⌉ workgroups).  Reads diag(A), writes perm.
constexpr int kSbrRankMax = 8192;  // largest n of the rank kernel (32 KB of keys in LDS)
constexpr int kSbrRankWaves = 16;

__device__ __forceinline__ float evx_sbr_sort_key(float v) { return isnan(v) ? INFINITY : v; }

// blk: the 64-index group this workgroup ranks (blockIdx.x in the rank kernel)
__device__ __forceinline__ void evx_sbr16_rank_body(const float* __restrict__ A, int n, int64_t lda, int shift, int* __restrict__ perm,
                                                    int blk) {
  __shared__ __attribute__((aligned(16))) float key[kSbrRankMax + 16];
  __shared__ int part[kSbrRankWaves][64];
  const int np = (n + 15) & ~15;  // padded with +inf: never below a real key (NaN keys are +inf too, ties by index)
  for (int i = threadIdx.x; i < np; i += blockDim.x) key[i] = i < n ? evx_sbr_sort_key(A[(int64_t)i * lda + i]) : INFINITY;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blk * 64 + lane;
  const float ki = i < n ? key[i] : 0.f;
  // each wave counts over a sixteenth of the keys, 4 keys per LDS broadcast read (ds_read_b128)
  const int q = ((np / kSbrRankWaves) + 3) & ~3, j0 = min(np, w * q), j1 = min(np, j0 + q);
  int cnt = 0;
#pragma unroll 4
  for (int j = j0; j < j1; j += 4) {
    const float4 k4 = *(const float4*)(key + j);  // same address across the wave: broadcast
    cnt += (k4.x < ki) | ((k4.x == ki) & (j < i));
    cnt += (k4.y < ki) | ((k4.y == ki) & (j + 1 < i));
    cnt += (k4.z < ki) | ((k4.z == ki) & (j + 2 < i));
    cnt += (k4.w < ki) | ((k4.w == ki) & (j + 3 < i));
  }
  part[w][lane] = cnt;
  __syncthreads();
  if (w == 0 && i < n) {
    int r = 0;
#pragma unroll
    for (int v = 0; v < kSbrRankWaves; ++v) r += part[v][lane];
    int pos = r - shift;
    if (pos < 0) pos += n;
    perm[pos] = i;
  }
}

// ------------------------------------------------------------------ device schedule: control step
// control words per refinement slot (documented in eigh_sbr_dev.hip)
constexpr int kSbrCW = 8;

struct SbrDevParams {
  float tol, ns_kappa, damp_kappa, t4_kappa, near_only;
  float theta0;  // local far threshold factor once κ ≤ theta_kappa (0: only after a stall)
  float theta_kappa;
  int ns_iters;
  int lean_from;  // slots ≥ lean_from carry no damping / Newton–Schulz / X³ kernels (order 4, undamped)
  int recover;    // divergences recovered by a forced damped step before the solve gives up (0: stop at the first)
  int lean_guard; // 1: a lean slot whose step would need damping / Newton–Schulz / order 6 stops the solve (capped)
  int xgate;      // 1: the damping kernels are scheduled for every full-slot far step and gate themselves (sbr_dev_prep)
  int damp_from;  // slots ≥ damp_from carry no damping kernels (≤ lean_from; the late schedule keeps them in slot 0 only)
};

__device__ __forceinline__ void evx_sbr_rel_kappa(const double* h, double& r, double& k) {
  const double off = fmax(h[0], 0.0), dg = h[1], mn = h[2], mx = h[3];
  r = dg > 0.0 ? sqrt(off / dg) : (double)NAN;
  k = mx > mn ? sqrt(off) / (mx - mn) : (double)INFINITY;
}

// Body of sbr_dev_ctrl_kernel: the control step after iteration j (j = −1: after the initial
// Bᵀ C B), run by ONE workgroup on its first 256 threads.  Every thread of that workgroup must
// call it (the barriers); a wider workgroup (the fused control + rank launch has 1024 threads)
// only meets the barriers with its other threads, so the loop strides, the 4-wave LDS reduction
// and with them the float64 sums are those of the 256-thread kernel.
__device__ __forceinline__ void evx_sbr_dev_ctrl_body(const double* __restrict__ part, int nparts, int j, int K,
                                                      double* __restrict__ hist, float* __restrict__ alpha,
                                                      float* __restrict__ theta, int* __restrict__ ctrl, int* __restrict__ st,
                                                      const SbrDevParams& prm, const float* __restrict__ A, int64_t lda, int n,
                                                      float* __restrict__ w_out, double* __restrict__ eig_stats,
                                                      float* __restrict__ w_init, double* __restrict__ log, int log_len,
                                                      int* __restrict__ log_count, int* __restrict__ rep_seq, double* rep_ring,
                                                      int rep_len) {
  constexpr int kCW = kSbrCW;
  __shared__ double s[4][4];
  __shared__ int s_keep;
  const int t = threadIdx.x;
  const bool act = t < 256;  // wave-uniform
  const bool executed = j < 0 || ctrl[kCW * j] == 0;
  double* hj1 = hist + 4 * (j + 1);
  if (executed) {
    if (act) {
      double off = 0.0, dg = 0.0, mn = DBL_MAX, mx = -DBL_MAX;
      for (int i = t; i < nparts; i += 256) {
        off += part[4 * i];
        dg += part[4 * i + 1];
        mn = fmin(mn, part[4 * i + 2]);
        mx = fmax(mx, part[4 * i + 3]);
      }
      // wave reductions (no barrier), then the four wave results through LDS: one barrier
      // instead of the eight of a 256-wide tree (this step sits on the schedule's serial path)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        off += __shfl_xor(off, o);
        dg += __shfl_xor(dg, o);
        mn = fmin(mn, __shfl_xor(mn, o));
        mx = fmax(mx, __shfl_xor(mx, o));
      }
      if ((t & 63) == 0) {
        s[0][t >> 6] = off;
        s[1][t >> 6] = dg;
        s[2][t >> 6] = mn;
        s[3][t >> 6] = mx;
      }
    }
    __syncthreads();
    if (t == 0) {
      hj1[0] = (s[0][0] + s[0][1]) + (s[0][2] + s[0][3]);
      hj1[1] = (s[1][0] + s[1][1]) + (s[1][2] + s[1][3]);
      hj1[2] = fmin(fmin(s[2][0], s[2][1]), fmin(s[2][2], s[2][3]));
      hj1[3] = fmax(fmax(s[3][0], s[3][1]), fmax(s[3][2], s[3][3]));
    }
  } else if (t < 4) {
    hj1[t] = hist[4 * j + t];
  }
  if (j < 0 && act) {  // the warm-start diagonal: the result if the refinement has to be abandoned
    for (int i = t; i < n; i += 256) w_init[i] = A[(int64_t)i * lda + i];
  }
  __syncthreads();
  if (t == 0) {
    if (j < 0) {
      st[0] = 0;  // stopped
      st[1] = 0;  // fallback
      st[2] = 0;  // iterations run
      st[3] = 1;  // last_far
      st[4] = 0;  // theta sticky
      st[6] = 0;  // converged
      st[7] = 0;  // status bits | recoveries << 8
      alpha[0] = 1.f;
    }
    double r, k;
    evx_sbr_rel_kappa(hj1, r, k);
    double r0, k0;
    evx_sbr_rel_kappa(hist, r0, k0);  // the warm start's off-norm
    // orthogonality monitor for free: ‖BᵀCB‖_F = ‖C‖_F for an orthogonal B, so the Frobenius
    // norm of A (off + diag parts, both in the stats) drifting from the warm start's means the
    // basis lost orthogonality — which the relative off-norm alone does not see
    const double F0 = hist[0] + hist[1], F = hj1[0] + hj1[1];
    const bool ortho = F0 > 0.0 && fabs(F / F0 - 1.0) <= 1e-3;
    bool force = false;       // the next iteration must be damped + re-orthonormalised
    // the solve stops here keeping the better basis: the current one (finite, orthogonal and
    // closer to diagonal), or the warm start
    auto give_up = [&](bool finite_now) {
      st[0] = 1;
      st[1] = (finite_now && ortho && r < r0) ? 0 : 1;
    };
    if (j >= 0 && executed && !st[0]) {
      st[2] = j + 1;
      double rp, kp;
      evx_sbr_rel_kappa(hist + 4 * j, rp, kp);
      const bool far_j = ctrl[kCW * j + 1] == 0;
      if (!ortho) st[7] |= 4;
      if (!isfinite(r)) {
        give_up(false);  // the basis itself is broken: back to the warm start
      } else if (r > 1.5 * rp || !ortho) {
        if ((st[7] >> 8) < prm.recover) {
          st[7] = (st[7] | 1) + (1 << 8);
          force = true;
          st[3] = far_j ? 1 : 0;
        } else {
          give_up(true);
        }
      } else {
        // an undamped far iteration close to the tolerance that barely helped: pairs in a
        // cluster denser than the global threshold assumes — local threshold from now on
        if (far_j && alpha[j + 1] >= 1.f && r < 100.0 * prm.tol && r > 0.6 * rp) st[4] = 1;
        st[3] = far_j ? 1 : 0;
      }
    }
    if (!st[0] && r <= prm.tol && ortho) {
      st[0] = 1;
      st[6] = 1;
    }
    const int nx = j + 1;
    if (nx < K) {
      int* c = ctrl + kCW * nx;
      const bool lean = nx >= prm.lean_from;
      const bool nodamp = nx >= prm.damp_from;  // no damping kernels in this slot (lean slots have none either)
      if (!st[0]) {
        // step size of the iteration just run (1 at the start); a lean slot's step is bounded
        // to a negligible Taylor remainder (sbr_dev_prep), so its α < 1 asks for no Newton–Schulz
        const float a_prev = (nx - 1 >= prm.lean_from) ? 1.f : alpha[nx];
        // after a divergence every further far step is damped and re-orthonormalised (sticky):
        // in the clustered spectra that diverge, an undamped step right after the recovery
        // diverges again (profiles/r5_eigh_recover.txt)
        const bool sticky = (st[7] & 1) != 0;
        const bool ns = force || sticky || nx < prm.ns_iters || a_prev < 1.f || k > prm.ns_kappa;
        const bool damp = force || sticky || nx == 0 || k > prm.damp_kappa;

        const bool far = force || !(nx > 0 && r <= prm.near_only * prm.tol && st[3]);
        const bool six = !(k < prm.t4_kappa);
        // (a lean slot still takes an order-4 step where the rules would pick order 6: the
        // truncation is O(‖X‖⁵/120) and stays orthogonal to that order; damping and
        // Newton–Schulz are the safety steps it cannot skip)
        if (far && prm.lean_guard && ((lean && (ns || damp)) || (nodamp && damp))) {
          // the lean slot has no damping / Newton–Schulz / order-6 kernels: taking its plain
          // order-4 step here is unguarded — stop, capped (the host escalates the schedule)
          st[7] |= 2;
          give_up(true);
        } else {
          c[0] = 0;
          c[1] = far ? 0 : 1;
          // 0: damp (κ rule), 2: the generator's free bounds decide (xgate), 1: no damping
          c[2] = (far && !lean && !nodamp) ? (damp ? 0 : (prm.xgate ? 2 : 1)) : 1;
          c[3] = (far && six && !lean) ? 0 : 1;
          c[4] = (six && !lean) ? 1 : 0;
          c[5] = (far && ns && !lean) ? 0 : 1;
          c[6] = (ns && !lean) ? 1 : 0;
          c[7] = far ? 1 : 0;
          // local far threshold: sticky after a stalled far iteration, or (theta0) once the far
          // step is small (κ ≤ theta_kappa: with larger steps the extra strongly coupled far pairs
          // rotated at once can make a cold-start iteration diverge)
          const bool th = st[4] || (prm.theta0 > 0.f && k <= prm.theta_kappa);
          theta[nx] = th ? (prm.theta0 > 0.f ? prm.theta0 : 1.f) : 0.f;
          alpha[nx + 1] = 1.f;  // the damping kernel of iteration nx overwrites it when it runs
        }
      }
      if (st[0]) {
        c[0] = 1; c[1] = 1; c[2] = 1; c[3] = 1; c[4] = 0; c[5] = 1; c[6] = 0; c[7] = 1;
      }
    }
    if (nx == K) {
      const bool fb = st[1] != 0;
      double rf, kf;
      evx_sbr_rel_kappa(fb ? hist : hist + 4 * K, rf, kf);
      eig_stats[0] = rf;
      const bool conv = st[6] != 0 && rf <= prm.tol;
      eig_stats[1] = (double)((conv ? 0 : 1) | ((st[7] & 1) ? 2 : 0) | ((st[7] & 2) ? 4 : 0) | ((st[7] & 4) ? 8 : 0));
      eig_stats[2] = (double)st[2];
      eig_stats[3] = fb ? 1.0 : 0.0;
      // keep: the restore copy (warm-start basis → output) is skipped unless the refinement
      // diverged or no iteration ran at all (the solve then never wrote its output basis: the
      // warm start is read directly by the first BᵀCB and the first iteration, no copy launch)
      st[5] = (fb || st[2] == 0) ? 0 : 1;
      if (log && log_len > 0) {  // per-solve history ring (read by benches after the timed loop)
        const int c = *log_count;
        double* o = log + 4 * (int64_t)(c % log_len);
        o[0] = eig_stats[0];
        o[1] = eig_stats[1];
        o[2] = eig_stats[2];
        o[3] = eig_stats[3];
        *log_count = c + 1;
      }
      if (rep_seq) {  // the solve's health into the host-mapped ring (CMAES schedule; was sbr_report_kernel)
        const int q = *rep_seq;
        double* o = rep_ring + 5 * (int64_t)(q % rep_len);
        o[0] = eig_stats[0];
        o[1] = eig_stats[1];
        o[2] = eig_stats[2];
        o[3] = eig_stats[3];
        o[4] = (double)q;
        __threadfence_system();
        *rep_seq = q + 1;
      }
    }
    s_keep = st[1] ? 0 : 1;
  }
  __syncthreads();
  if (j + 1 == K && act) {
    const bool keep = s_keep != 0;
    for (int i = t; i < n; i += 256) w_out[i] = keep ? A[(int64_t)i * lda + i] : w_init[i];
  }
}
