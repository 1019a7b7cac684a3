// Device-controlled schedule of the sorted-block-refinement eigensolver (K4, round 3).
//
// The host-driven solver (evoxmi/ops/sbr.py:eigh_warm) reads the convergence statistics
// back after every iteration (or once per planned solve) to choose the next iteration's
// variant — Newton–Schulz or not, damping, far step, Taylor order, local threshold — and
// when to stop.  That split every CMA-ES generation into graph segments around a host
// phase.  Here the same decisions run on the device: the solve is a fixed schedule of K
// iterations captured once into the generation's graph, every kernel of an iteration reads
// a control word and returns at once when its variant is off (or the solve has converged),
// and one single-workgroup kernel per iteration (sbr_dev_ctrl_kernel) reduces the stats
// partials that the Bᵀ C B GEMM wrote in its epilogue and writes the next iteration's
// control words.  No host read, no plan, nothing outside the checkpointed state.
//
// Control words per iteration j (int32[8]):
//   0 skip_all   1 skip_far   2 skip_damp   3 skip_x3 (order 4)   4 sel6 (order 6)
//   5 skip_ns    6 sel_ns (Bq·V lands in the Newton–Schulz input)   7 skip_copy (near-only: Bq → B)
// Persistent words st[8]: 0 stopped, 1 fallback (diverged), 2 refinement iterations run,
//   3 last_far, 4 theta sticky, 5 keep (0 ⇒ restore the warm-start basis), 6 converged,
//   7 status bits (1 recovered from a divergence, 2 stopped by the lean-slot guard, 4 the basis
//     lost orthogonality at some iteration) | recoveries << 8.
//
// Divergence (round 5): an iteration whose off-norm grew past 1.5× the previous one no longer
// ends the solve with the warm-start basis.  While recoveries remain (prm.recover) the next
// iteration is forced damped (‖αX‖ ≤ τ) with a Newton–Schulz re-orthonormalisation, from the
// current basis; a non-finite off-norm, or a divergence with no recovery left / no full slot
// left, stops the solve and keeps the better of the current and the warm-start basis.  A lean
// slot (no damping / Newton–Schulz / order-6 kernels) whose iteration the full rules would have
// damped, re-orthonormalised or expanded to order 6 is not taken: the solve stops there,
// capped.  An iteration after which ‖BᵀCB‖_F moved off ‖C‖_F (the warm start's) by more than
// 1e-3 relative lost orthogonality: it is treated as a divergence, and such a basis is never
// kept.  eig_stats = [off_rel, status, iterations, fallback] with status bit 1 = not
// converged (capped), 2 = recovered from a divergence, 4 = stopped by the lean-slot guard,
// 8 = orthogonality drift seen —
// read by the host one generation late (CMAES.graph_variant escalates the schedule).
#include "evoxmi_common.h"
#include "evoxmi_sbr.h"
#include <float.h>
#include <math.h>

namespace {

// Taylor operands of exp(αX) for the order the control word selects (sel6), with M of
// exp(−αX) (the transposed product, ops/sbr.py:expm_t_device).  V2 != null: when this
// iteration's damping ran (ctrl[2] == 0) every workgroup forms α from its power-step vectors
// itself and workgroup 0 stores it — the damping's own single-workgroup final launch is gone.
//
// Step size (round 5).  With the X² GEMM's stats partials (xpart) the damping also follows
// free bounds of the generator (evx_sbr_xbounds: max row norm² ≤ ‖X‖₂² ≤ sqrt(n·Σ diag(X²)²)):
// the power iteration never runs when the upper bound proves ‖X‖₂ ≤ τ (α = 1 exact), and a far
// step the κ rule would leave undamped still gets it when some row of X is longer than τ/2
// (evx_sbr_damp_runs).  An undamped step on a large generator — which diverged the d = 2000 cold start at
// κ = 0.4 < damp_kappa (profiles/r5_eigh_recover.txt) — no longer happens.  (Using the
// Frobenius bound itself as the step size throttled normal solves: ‖X‖_F ≫ ‖X‖₂ when many
// pairs rotate at once.)
__global__ void __launch_bounds__(256) sbr_dev_prep_kernel(const float* __restrict__ X, const float* __restrict__ X2,
                                                           const float* __restrict__ X3, int n, float* __restrict__ alpha,
                                                           float* __restrict__ P, float* __restrict__ MT, int* __restrict__ ctrl,
                                                           const float* __restrict__ V2, const float* __restrict__ V3, float tau,
                                                           const double* __restrict__ xpart, int nparts,
                                                           const float* __restrict__ copy_src, float* __restrict__ copy_dst,
                                                           int minus_id) {
  if (ctrl[1]) {
    // no far step this iteration: a near-only iteration (ctrl[7] == 0) takes the block-rotated
    // basis Bq as the new basis — the copy runs here, in the launch the schedule makes anyway
    if (copy_src && ctrl[7] == 0) {
      const int64_t n4 = (int64_t)n * n / 4;
      const float4* s4 = reinterpret_cast<const float4*>(copy_src);
      float4* d4 = reinterpret_cast<float4*>(copy_dst);
      const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
      for (int64_t e = g; e < n4; e += stride) d4[e] = s4[e];
      for (int64_t e = 4 * n4 + g; e < (int64_t)n * n; e += stride) copy_dst[e] = copy_src[e];
    }
    return;
  }
  const bool six = ctrl[4] != 0;
  float a;
  if (xpart) {
    const bool ran = V2 && evx_sbr_damp_runs(ctrl[2], evx_sbr_xbounds(xpart, nparts, n), tau * tau);
    a = ran ? evx_sbr_damping_alpha(V2, V3, n, tau) : 1.f;
  } else if (V2 && ctrl[2] == 0) {
    a = evx_sbr_damping_alpha(V2, V3, n, tau);
  } else {
    a = alpha[0];
  }
  if (xpart || (V2 && ctrl[2] == 0)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      alpha[0] = a;
      // the generator's bounds damped a step the κ rule had left undamped and without
      // Newton–Schulz (xgate): near-degenerate spectra (κ small, gaps ≈ 1e-5 — a CMA-ES C after
      // a few small-λ updates) give generators of 2-norm ≈ 5 and a damped step of ‖αX‖ = τ whose
      // order-4 truncation, un-re-orthonormalised, grew the off-norm 100× and sent the solve
      // into its divergence recovery (profiles/NOTES.md, round 6).  Re-orthonormalise this
      // iteration too: the B·V product (launched after this kernel) reads sel_ns, and the
      // Newton–Schulz kernels skip_ns, at run time; damping only runs in full slots, which
      // carry the Newton–Schulz kernels.
      if (xpart && a < 1.f && ctrl[5] != 0) {
        ctrl[5] = 0;
        ctrl[6] = 1;
      }
    }
  }

  const float a2 = a * a, a3 = a2 * a;
  // rows over the grid, columns over the threads (float4 when n % 4 == 0): no per-element
  // 64-bit division (the flat-index form spent most of its time in the i = e / n expansion)
  const bool v4 = (n & 3) == 0;
  const int nc = v4 ? n >> 2 : n;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t r = (int64_t)i * n;
    for (int c = threadIdx.x; c < nc; c += blockDim.x) {
      const int w = v4 ? 4 : 1;
      float xs[4] = {}, x2s[4] = {}, x3s[4] = {};
      if (v4) {
        const float4 x = reinterpret_cast<const float4*>(X + r)[c], y = reinterpret_cast<const float4*>(X2 + r)[c];
        xs[0] = x.x; xs[1] = x.y; xs[2] = x.z; xs[3] = x.w;
        x2s[0] = y.x; x2s[1] = y.y; x2s[2] = y.z; x2s[3] = y.w;
        if (six) {
          const float4 z = reinterpret_cast<const float4*>(X3 + r)[c];
          x3s[0] = z.x; x3s[1] = z.y; x3s[2] = z.z; x3s[3] = z.w;
        }
      } else {
        xs[0] = X[r + c];
        x2s[0] = X2[r + c];
        if (six) x3s[0] = X3[r + c];
      }
      float ps[4], ms[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = c * w + q;
        const float x = a * xs[q], x2 = a2 * x2s[q];
        // minus_id: M − I (the caller adds the exact basis itself: B·V = Bq + Bq·(V − I), whose
        // correction product then runs at bf16x3)
        const float id = (i == j && !minus_id) ? 1.f : 0.f;
        if (six) {
          const float x3 = a3 * x3s[q];
          ps[q] = a3 * (x * (1.f / 24.f) + x2 * (1.f / 120.f) + x3 * (1.f / 720.f));
          ms[q] = id - x + 0.5f * x2 - x3 * (1.f / 6.f);
        } else {
          ps[q] = a2 * (x * (1.f / 6.f) + x2 * (1.f / 24.f));
          ms[q] = id - x + 0.5f * x2;
        }
      }
      if (v4) {
        reinterpret_cast<float4*>(P + r)[c] = make_float4(ps[0], ps[1], ps[2], ps[3]);
        reinterpret_cast<float4*>(MT + r)[c] = make_float4(ms[0], ms[1], ms[2], ms[3]);
      } else {
        P[r + c] = ps[0];
        MT[r + c] = ms[0];
      }
    }
  }
}

__global__ void __launch_bounds__(256) sbr_dev_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n,
                                                           const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int64_t n4 = n / 4;
  const float4* s4 = reinterpret_cast<const float4*>(src);
  float4* d4 = reinterpret_cast<float4*>(dst);
  const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = g; e < n4; e += stride) d4[e] = s4[e];
  for (int64_t e = 4 * n4 + g; e < n; e += stride) dst[e] = src[e];
}

// j = −1: the initial Bᵀ C B; j ≥ 0: after iteration j.  One workgroup (body in evoxmi_sbr.h).
__global__ void __launch_bounds__(256) sbr_dev_ctrl_kernel(const double* __restrict__ part, int nparts, int j, int K,
                                                           double* __restrict__ hist, float* __restrict__ alpha,
                                                           float* __restrict__ theta, int* __restrict__ ctrl, int* __restrict__ st,
                                                           SbrDevParams prm, const float* __restrict__ A, int64_t lda, int n,
                                                           float* __restrict__ w_out, double* __restrict__ eig_stats,
                                                           float* __restrict__ w_init, double* __restrict__ log, int log_len,
                                                           int* __restrict__ log_count, int* __restrict__ rep_seq, double* rep_ring,
                                                           int rep_len) {
  evx_sbr_dev_ctrl_body(part, nparts, j, K, hist, alpha, theta, ctrl, st, prm, A, lda, n, w_out, eig_stats, w_init, log, log_len,
                        log_count, rep_seq, rep_ring, rep_len);
}

// The control step after iteration j (j + 1 < K) and the ranking of slot j + 1 in ONE launch:
// the rank kernel followed the control kernel directly and took nothing from it but its skip
// word.  Workgroups 1 … ⌈n/64⌉ rank, unconditionally — diag(A) is final (the previous launch
// wrote it) and perm is read only by slot j + 1's block and far / Bq kernels, which still test
// their skip words — and workgroup 0 runs the control step beside them, in place on the same
// buffers.  No workgroup reads what another writes: no inter-workgroup communication.
// (Workgroup 0 running the control step AND a ranking tile made the launch as long as the two
// kernels it replaced — 1.3108 vs 1.3173 ms per flagship generation, profiles/NOTES.md — because
// both are latency chains; a workgroup of its own puts the two chains side by side.)
__global__ void __launch_bounds__(64 * kSbrRankWaves) sbr_dev_ctrl_rank_kernel(const double* __restrict__ part, int nparts, int j,
                                                                               int K, double* __restrict__ hist,
                                                                               float* __restrict__ alpha, float* __restrict__ theta,
                                                                               int* __restrict__ ctrl, int* __restrict__ st,
                                                                               SbrDevParams prm, const float* __restrict__ A,
                                                                               int64_t lda, int n, float* __restrict__ w_init, int shift,
                                                                               int* __restrict__ perm) {
  if (blockIdx.x == 0) {
    evx_sbr_dev_ctrl_body(part, nparts, j, K, hist, alpha, theta, ctrl, st, prm, A, lda, n, nullptr, nullptr, w_init, nullptr, 0, nullptr,
                          nullptr, nullptr, 0);
    return;
  }
  evx_sbr16_rank_body(A, n, lda, shift, perm, blockIdx.x - 1);
}

}  // namespace

void evx_sbr_dev_prep(const float* X, const float* X2, const float* X3, int n, float* alpha, float* P, float* MT, int* ctrl,
                      hipStream_t s, const float* V2, const float* V3, float tau, const double* xpart, int nparts, const float* copy_src,
                      float* copy_dst, int minus_id) {
  // a grid-stride loop over 256 workgroups: the schedule skips this kernel in most
  // iterations, and an empty launch costs in proportion to its workgroup count
  const int64_t total = (int64_t)n * n;
  int g = (int)((total + 255) / 256);
  if (g > 256) g = 256;
  sbr_dev_prep_kernel<<<g, 256, 0, s>>>(X, X2, X3, n, alpha, P, MT, ctrl, V2, V3, tau, xpart, nparts, copy_src, copy_dst,
                                        minus_id);
}

void evx_sbr_dev_copy(const float* src, float* dst, int64_t n, const int* skip, hipStream_t s) {
  int g = (int)((n / 4 + 255) / 256);
  if (g < 1) g = 1;
  if (g > 256) g = 256;  // mostly skipped: keep the empty launch small
  sbr_dev_copy_kernel<<<g, 256, 0, s>>>(src, dst, n, skip);
}

void evx_sbr_dev_ctrl(const double* part, int nparts, int j, int K, double* hist, float* alpha, float* theta, int* ctrl, int* st,
                      const float* prm6, int ns_iters, const float* A, int64_t lda, int n, float* w_out, double* eig_stats, float* w_init,
                      double* log, int log_len, int* log_count, hipStream_t s, int lean_from, int recover, int lean_guard, int xgate,
                      int damp_from, int* rep_seq, double* rep_ring, int rep_len) {
  SbrDevParams p{prm6[0], prm6[1], prm6[2], prm6[3], prm6[4], prm6[5], prm6[6], ns_iters, lean_from, recover, lean_guard, xgate,
                 damp_from < 0 ? lean_from : min(damp_from, lean_from)};
  sbr_dev_ctrl_kernel<<<1, 256, 0, s>>>(part, nparts, j, K, hist, alpha, theta, ctrl, st, p, A, lda, n, w_out, eig_stats, w_init, log,
                                        log_len, log_count, j + 1 == K ? rep_seq : nullptr, rep_ring, rep_len);
}

void evx_sbr_dev_ctrl_rank(const double* part, int nparts, int j, int K, double* hist, float* alpha, float* theta, int* ctrl, int* st,
                           const float* prm6, int ns_iters, const float* A, int64_t lda, int n, float* w_init, int shift, int* perm,
                           hipStream_t s, int lean_from, int recover, int lean_guard, int xgate, int damp_from) {
  SbrDevParams p{prm6[0], prm6[1], prm6[2], prm6[3], prm6[4], prm6[5], prm6[6], ns_iters, lean_from, recover, lean_guard, xgate,
                 damp_from < 0 ? lean_from : min(damp_from, lean_from)};
  sbr_dev_ctrl_rank_kernel<<<1 + (n + 63) / 64, 64 * kSbrRankWaves, 0, s>>>(part, nparts, j, K, hist, alpha, theta, ctrl, st, p, A, lda, n,
                                                                        w_init, shift, perm);
}
