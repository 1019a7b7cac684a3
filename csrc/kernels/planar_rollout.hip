// Persistent rollout of the planar articulated-tree tasks (hopper, walker2d, halfcheetah, swimmer,
// inverted_pendulum, inverted_double_pendulum, reacher and any model of the same combinations) with a
// per-individual MLP policy.
//
// Execution model of the Ant rollout's LDS-resident kernel (ant_rollout_kernel in neuro.hip, the one of its two
// kernels that keeps the weights in LDS; the physics there is Ant-specific and packed f32, here it is table-driven
// and scalar): one wave64 owns one individual for the whole
// episode, its MLP obs-h1-h2-act (tanh) weights live in LDS with lanes striding over units (the first
// layer's in registers when it has at most 128 units, see w1_in_registers), waves
// leave independently (sticky done, the terminating step earns nothing) and there is no block
// barrier after the weight load.
//
// The model is data: the float32 table that PlanarChain.model_table() packs from the model spec
// (evoxmi/problems/neuroevolution/reinforcement_learning/planar.py, the CPU oracle) arrives by
// value in the kernel-argument segment, so every parameter is a wave-uniform scalar load and the
// launch captures into a hipGraph with no device copy of the table.  The tree shape, the root
// constraint, the task kind and what the actions drive are compile-time: the kernel is instantiated
// per combination (VARIANTS), every loop over bodies and degrees of freedom is fully unrolled, and
// no register array is indexed by a run-time value.  A locked root coordinate keeps its initial
// value, has velocity 0 and drops out of the mass matrix, the right-hand side and the LDLᵀ
// elimination as a structural zero; with a fully locked root the system is the hinges alone.
//
// Physics per sub-step, lane-uniform float32 (PlanarChain._substep): q ← q + dt·u; kinematics down
// the tree relative to the root point; per-body external wrenches (gravity, cap contacts, fluid
// drag, root damping) about the root point, summed up the tree into every subtree's wrench, which
// gives the generalized forces Q_k = N_k − h_k × F_k; ∂T/∂φ_k = v_hinge × P_subtree; the momentum
// update; the mass matrix by the composite-rigid-body recursion (subtree mass, first and second
// moment about the hinge); one sparse LDLᵀ solve eliminated from the leaves (no fill-in on a tree).
// A root with two chains (walker2d, halfcheetah) is spread over lanes: even lanes own the first chain,
// odd lanes the second, both integrate the root.  Each lane runs the chain-of-4 code on its own chain's
// parameters (held in VGPRs); what the chains add to the root (wrench, composite mass / first / second
// moment, and the Schur complement of the mass matrix and right-hand side left by eliminating a chain's
// three hinges) is summed across the lane pair by DPP, 16 sums per sub-step, so the root's 3 × 3 system
// and everything lane-uniform stays bit-identical in both lanes.
// Like the Ant kernel (neuro.hip), the sub-step uses the hardware approximations __sinf / __cosf,
// v_rcp_f32 and v_rsq_f32 (about 1 ulp; the measured returns sit at the float32 torch loop's error).
// The root's angular momentum is carried about the root point, π_θ ← π_θ + dt·(N_root − u_root × P):
// algebraically the oracle's world-origin form L − r × P without its large cancelling terms.
#include "evoxmi_common.h"

namespace {

constexpr int HDR = 24, BODY = 16, HINGE = 10, MAXB = 8, TABLE = HDR + MAXB * (BODY + HINGE);
enum { H_NB, H_SKIP, H_SUB, H_DT, H_G, H_KC, H_CC, H_MU, H_EPS, H_LIN, H_ANG, H_CN, H_CT, H_CW, H_CLIP, H_HEALTHY, H_CTRL, H_ZLO, H_ZHI, H_PITCH,
       H_LOCK, H_KIND, H_TIPX, H_TIPGOAL };  // the last four are 0 for a free root and the run task
enum { B_PAR, B_AX, B_AZ, B_CX, B_CZ, B_M, B_I, B_CAP0, B_CAP1 = B_CAP0 + 4 };  // cap: x, z, radius, contact
enum { J_GEAR, J_ARM, J_DAMP, J_STIFF, J_REST, J_LO, J_HI, J_LIMK, J_INIT, J_VELCOST };  // hinge row 0: the root slider's gear, lo, hi, limit_k
enum { K_RUN, K_BALANCE, K_BALANCE_TIP, K_REACH };

struct PlanarModel {
  float v[TABLE];
};

// tree shapes: chain of 3 (swimmer, inverted_double_pendulum, reacher), chain of 4 (hopper), torso + two chains of 3
// (walker2d, halfcheetah), chain of 2 (inverted_pendulum)
constexpr int NTOPO = 4;
constexpr int TOPO_NB[NTOPO] = {3, 4, 7, 2};
constexpr int TOPO_PAR[NTOPO][MAXB] = {{-1, 0, 1, 0, 0, 0, 0, 0}, {-1, 0, 1, 2, 0, 0, 0, 0}, {-1, 0, 1, 2, 0, 4, 5, 0}, {-1, 0, 0, 0, 0, 0, 0, 0}};

// what the kernel is instantiated for: tree shape, mask of locked root coordinates (1 x, 2 z, 4 θ), task kind, and what
// the actions drive (the root slider first, then every hinge or none: a passive hinge reads no action)
struct Variant {
  int topo, lock, kind;
  bool root_act, hinge_act;
};
constexpr int NVARIANT = 6;
constexpr Variant VARIANTS[NVARIANT] = {{0, 0, K_RUN, false, true},        {1, 0, K_RUN, false, true},         {2, 0, K_RUN, false, true},
                                        {3, 6, K_BALANCE, true, false},   {0, 6, K_BALANCE_TIP, true, false}, {0, 7, K_REACH, false, true}};
// observations of a variant before obs_skip (run: q ++ u of the whole model; the others are built from free coordinates)
constexpr int variant_obs(int v) {
  const int nb = TOPO_NB[VARIANTS[v].topo], nj = nb - 1;
  int nfr = 0;
  for (int i = 0; i < 3; ++i) nfr += !((VARIANTS[v].lock >> i) & 1);
  switch (VARIANTS[v].kind) {
    case K_RUN: return 2 * (nb + 2);
    case K_BALANCE: return 2 * (nfr + nj);
    case K_BALANCE_TIP: return nfr + 2 * nj + nfr + nj;
    default: return 3 * nj + 5;  // cos, sin, target (2), velocities, tip − target (2), 0
  }
}
constexpr int variant_act(int v) { return (VARIANTS[v].root_act ? 1 : 0) + (VARIANTS[v].hinge_act ? TOPO_NB[VARIANTS[v].topo] - 1 : 0); }
constexpr int variant_aux(int v) { return VARIANTS[v].kind == K_REACH ? 2 : 0; }

constexpr bool anc(int T, int b, int k) {  // body k is b or an ancestor of b
  while (b >= 0) {
    if (b == k) return true;
    b = TOPO_PAR[T][b];
  }
  return false;
}
struct Rel {  // rel[i] bit j: degrees of freedom i and j share a mass-matrix entry
  unsigned anc[NTOPO][MAXB], rel[NTOPO][MAXB + 2];
};
constexpr Rel make_rel() {
  Rel r{};
  for (int t = 0; t < NTOPO; ++t) {
    for (int b = 0; b < TOPO_NB[t]; ++b)
      for (int k = 0; k < TOPO_NB[t]; ++k)
        if (anc(t, b, k)) r.anc[t][b] |= 1u << k;
    for (int i = 0; i < TOPO_NB[t] + 2; ++i)
      for (int j = 0; j < TOPO_NB[t] + 2; ++j)
        if (i < 2 || j < 2 || anc(t, i - 2, j - 2) || anc(t, j - 2, i - 2)) r.rel[t][i] |= 1u << j;
  }
  return r;
}
constexpr Rel REL = make_rel();

// the first layer's weights live in registers (two columns per lane) when it has at most 128 units: one LDS
// stream less per control step, and (obs·h1)·4 bytes of LDS less per wave, which at hidden 96 lets four waves
// (one per SIMD) share a CU where three did
__host__ __device__ constexpr bool w1_in_registers(int h1) { return h1 <= 128; }

// v + the lane pair's other v (lane ^ 1); both lanes get the same bits
__device__ __forceinline__ float pair_sum(float v) {
  return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}

// T: the tree shape this lane integrates.  SPLIT: the lane's chain is one of two hanging on the same root
// (the other one lives in lane ^ 1); whatever a chain adds to the root is summed over the lane pair.
// LOCK: mask of locked root coordinates.  SLIDER: root x is driven along a slider with a limit spring.
// TIP: keep the world position of the last body's far end cap (tipx, tipz) at the pose of the last sub-step.
template <int T, bool SPLIT, int LOCK = 0, bool SLIDER = false, bool TIP = false>
struct Chain {
  static constexpr int NB = TOPO_NB[T], ND = NB + 2;
  // π_θ is advanced with the linear momenta, so a free θ needs free translations
  static_assert(LOCK == 0 || LOCK == 6 || LOCK == 7, "root constraints: free, x only, or fully locked");
  static_assert(!(SPLIT && LOCK), "the two-chain root is free");
  static __device__ __forceinline__ constexpr bool fr(int i) { return i >= 3 || !((LOCK >> i) & 1); }  // coordinate i is free
  float tipx, tipz;
  float q[ND], u[ND], pi[ND];  // π: P_x, P_z, angular momentum about the root point, hinge momenta
  float Bp[NB][BODY - 1], Jp[NB][J_LIMK + 1];  // this lane's body and hinge rows of the model table
  bool cap_on[NB][2];  // wave-uniform: the cap is a contact sphere in some lane (SPLIT: in either chain)

  // rows of the table: body b of this lane is body b + off of the model (off = 0, or 3 for the second chain)
  __device__ __forceinline__ void load(const PlanarModel& m, bool second) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int i = 0; i < BODY - 1; ++i) {
        float v = m.v[HDR + b * BODY + i];
        if (SPLIT && b > 0) {
          v = second ? m.v[HDR + (b + 3) * BODY + i] : v;
          asm volatile("" : "+v"(v));  // keep the selected row in a VGPR instead of re-selecting at every use
        }
        Bp[b][i] = v;
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
        cap_on[b][c] = m.v[HDR + b * BODY + B_CAP0 + 4 * c + 3] > 0.f || (SPLIT && b > 0 && m.v[HDR + (b + 3) * BODY + B_CAP0 + 4 * c + 3] > 0.f);
#pragma unroll
      for (int i = 0; i <= J_LIMK; ++i) {
        float v = m.v[HDR + MAXB * BODY + b * HINGE + i];
        if (SPLIT && b > 0) {
          v = second ? m.v[HDR + MAXB * BODY + (b + 3) * HINGE + i] : v;
          asm volatile("" : "+v"(v));
        }
        Jp[b][i] = v;
      }
    }
  }

  static __device__ __forceinline__ constexpr int par(int b) { return TOPO_PAR[T][b]; }
  static __device__ __forceinline__ constexpr bool rel(int i, int j) { return (REL.rel[T][i] >> j) & 1u; }

  // pose of the tree relative to the root point, and velocities of the hinge points and CoMs
  struct Pose {
    float ca[NB], sa[NB], hx[NB], hz[NB], rx[NB], rz[NB];
    float w[NB], vhx[NB], vhz[NB], vcx[NB], vcz[NB];
  };
  __device__ __forceinline__ void pose(const PlanarModel& m, Pose& k) {
    float al[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float* B = Bp[b];
      if (b == 0) {
        al[0] = q[2];
        k.hx[0] = k.hz[0] = 0.f;
        k.w[0] = u[2];
        k.vhx[0] = u[0];
        k.vhz[0] = u[1];
      } else {
        const int p = par(b);
        al[b] = al[p] + q[2 + b];
        const float dx = k.ca[p] * B[B_AX] - k.sa[p] * B[B_AZ], dz = k.sa[p] * B[B_AX] + k.ca[p] * B[B_AZ];
        k.hx[b] = k.hx[p] + dx;
        k.hz[b] = k.hz[p] + dz;
        k.w[b] = k.w[p] + u[2 + b];
        k.vhx[b] = k.vhx[p] - k.w[p] * dz;
        k.vhz[b] = k.vhz[p] + k.w[p] * dx;
      }
      k.ca[b] = __cosf(al[b]);
      k.sa[b] = __sinf(al[b]);
      k.rx[b] = k.ca[b] * B[B_CX] - k.sa[b] * B[B_CZ];
      k.rz[b] = k.sa[b] * B[B_CX] + k.ca[b] * B[B_CZ];
      k.vcx[b] = k.vhx[b] - k.w[b] * k.rz[b];
      k.vcz[b] = k.vhz[b] + k.w[b] * k.rx[b];
    }
    if (TIP) {
      const float* C = Bp[NB - 1] + B_CAP1;
      tipx = q[0] + k.hx[NB - 1] + (k.ca[NB - 1] * C[0] - k.sa[NB - 1] * C[1]);
      tipz = q[1] + k.hz[NB - 1] + (k.sa[NB - 1] * C[0] + k.ca[NB - 1] * C[1]);
    }
  }

  // u = M(q)⁻¹ π at the pose k
  __device__ __forceinline__ void solve(const PlanarModel& m, const Pose& k, bool momenta_from_u) {
    float ms[NB], Sx[NB], Sz[NB], Ic[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float* B = Bp[b];
      ms[b] = B[B_M];
      Sx[b] = B[B_M] * k.rx[b];
      Sz[b] = B[B_M] * k.rz[b];
      Ic[b] = B[B_I] + B[B_M] * (k.rx[b] * k.rx[b] + k.rz[b] * k.rz[b]);
    }
#pragma unroll
    for (int b = NB - 1; b >= 1; --b) {
      const int p = par(b);
      const float dx = k.hx[b] - k.hx[p], dz = k.hz[b] - k.hz[p];
      float dI = Ic[b] + 2.f * (dx * Sx[b] + dz * Sz[b]) + ms[b] * (dx * dx + dz * dz);
      float dSx = Sx[b] + ms[b] * dx, dSz = Sz[b] + ms[b] * dz, dm = ms[b];
      if (SPLIT && p == 0) {  // the root carries both chains
        dI = pair_sum(dI);
        dSx = pair_sum(dSx);
        dSz = pair_sum(dSz);
        dm = pair_sum(dm);
      }
      Ic[p] += dI;
      Sx[p] += dSx;
      Sz[p] += dSz;
      ms[p] += dm;
    }
    float A[ND][ND];  // lower triangle, structural zeros never touched
    A[0][0] = ms[0];
    A[1][0] = 0.f;
    A[1][1] = ms[0];
#pragma unroll
    for (int l = 0; l < NB; ++l) {
      A[2 + l][0] = -Sz[l];
      A[2 + l][1] = Sx[l];
#pragma unroll
      for (int kk = 0; kk <= l; ++kk)
        if ((REL.anc[T][l] >> kk) & 1u)
          A[2 + l][2 + kk] = Ic[l] + (k.hx[l] - k.hx[kk]) * Sx[l] + (k.hz[l] - k.hz[kk]) * Sz[l];
      if (l > 0) A[2 + l][2 + l] += Jp[l][J_ARM];
    }
    if (momenta_from_u) {  // π = M u (episode start)
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        if (!fr(i)) {
          pi[i] = 0.f;  // never read
          continue;
        }
        float acc = 0.f, chain = 0.f;  // chain: what this lane's hinges add to a root momentum
#pragma unroll
        for (int j = 0; j < ND; ++j)
          if (rel(i, j) && fr(j) && !(i < 2 && j < 2 && i != j)) {
            const float t = (j <= i ? A[i][j] : A[j][i]) * u[j];
            if (SPLIT && i < 3 && j >= 3)
              chain += t;
            else
              acc += t;
          }
        pi[i] = (SPLIT && i < 3) ? acc + pair_sum(chain) : acc;
      }
      return;
    }
    float r[ND], inv[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) r[i] = pi[i];
    float D[3][3] = {}, dr[3] = {};  // SPLIT: what eliminating this lane's hinges takes from the root's 3 × 3 system
#pragma unroll
    for (int l = ND - 1; l >= 0; --l) {
      if (!fr(l)) continue;
      if (SPLIT && l == 2) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) A[i][j] -= pair_sum(D[i][j]);
          r[i] -= pair_sum(dr[i]);
        }
      }
      inv[l] = __builtin_amdgcn_rcpf(A[l][l]);
#pragma unroll
      for (int i = l - 1; i >= 0; --i) {
        if (!rel(i, l) || !fr(i)) continue;
        const float f = A[l][i] * inv[l];
        if (SPLIT && l >= 3 && i < 3) {
#pragma unroll
          for (int j = 0; j <= i; ++j) D[i][j] += f * A[l][j];
          dr[i] += f * r[l];
        } else {
#pragma unroll
          for (int j = 0; j <= i; ++j)
            if (rel(j, l) && fr(j)) A[i][j] -= f * A[l][j];
          r[i] -= f * r[l];
        }
        A[l][i] = f;
      }
    }
#pragma unroll
    for (int l = 0; l < ND; ++l) {
      if (!fr(l)) continue;
      float acc = r[l] * inv[l];
#pragma unroll
      for (int i = 0; i < l; ++i)
        if (rel(i, l) && fr(i)) acc -= A[l][i] * u[i];
      u[l] = acc;
    }
  }

  // tau: the hinge torques; froot: the force of the root slider's actuator (SLIDER)
  __device__ __forceinline__ void substep(const PlanarModel& m, const float* tau, float froot) {
    const float* H = m.v;
    const float dt = H[H_DT];
#pragma unroll
    for (int i = 0; i < ND; ++i)
      if (fr(i)) q[i] += dt * u[i];
    Pose k;
    pose(m, k);
    // external wrench per body about the root point, and the bodies' linear momenta
    float Fx[NB], Fz[NB], Nr[NB], Px[NB], Pz[NB];
    const bool contacts = H[H_KC] > 0.f, fluid = (H[H_CN] > 0.f) || (H[H_CT] > 0.f) || (H[H_CW] > 0.f);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float* B = Bp[b];
      const float cx = k.hx[b] + k.rx[b], cz = k.hz[b] + k.rz[b];
      float fx = 0.f, fz = -B[B_M] * H[H_G];
      float n = cx * fz;
      if (fluid) {
        float tx0 = B[B_CAP1] - B[B_CAP0], tz0 = B[B_CAP1 + 1] - B[B_CAP0 + 1];
        const float il = __builtin_amdgcn_rsqf(fmaxf(tx0 * tx0 + tz0 * tz0, 1e-24f));
        tx0 *= il;
        tz0 *= il;
        const float tx = k.ca[b] * tx0 - k.sa[b] * tz0, tz = k.sa[b] * tx0 + k.ca[b] * tz0;
        const float vt = k.vcx[b] * tx + k.vcz[b] * tz, vn = -k.vcx[b] * tz + k.vcz[b] * tx;
        const float dfx = -H[H_CT] * vt * tx + H[H_CN] * vn * tz, dfz = -H[H_CT] * vt * tz - H[H_CN] * vn * tx;
        fx += dfx;
        fz += dfz;
        n += cx * dfz - cz * dfx - H[H_CW] * k.w[b];
      }
      if (contacts) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float* C = B + B_CAP0 + 4 * c;
          if (cap_on[b][c]) {  // a uniform branch; a lane whose own cap is no contact sphere gets zero force
            const float ex = k.ca[b] * C[0] - k.sa[b] * C[1], ez = k.sa[b] * C[0] + k.ca[b] * C[1];
            const float X = k.hx[b] + ex, Z = k.hz[b] + ez;
            const float vx = k.vhx[b] - k.w[b] * ez, vz = k.vhz[b] + k.w[b] * ex;
            const float pen = fmaxf(C[2] - (q[1] + Z), 0.f);
            float fn = fmaxf(H[H_KC] * pen - (pen > 0.f ? H[H_CC] * vz : 0.f), 0.f);
            if (SPLIT) fn = C[3] > 0.f ? fn : 0.f;
            const float ft = -H[H_MU] * fn * vx * __builtin_amdgcn_rsqf(vx * vx + H[H_EPS] * H[H_EPS]);
            fx += ft;
            fz += fn;
            n += X * fn - Z * ft;
          }
        }
      }
      if (b == 0) {
        fx -= H[H_LIN] * u[0];
        fz -= H[H_LIN] * u[1];
        n -= H[H_ANG] * u[2];
        if (SLIDER) fx += froot + Jp[0][J_LIMK] * (fmaxf(Jp[0][J_LO] - q[0], 0.f) - fmaxf(q[0] - Jp[0][J_HI], 0.f));
      }
      Fx[b] = fx;
      Fz[b] = fz;
      Nr[b] = n;
      Px[b] = B[B_M] * k.vcx[b];
      Pz[b] = B[B_M] * k.vcz[b];
    }
#pragma unroll
    for (int b = NB - 1; b >= 1; --b) {
      const int p = par(b);
      if (SPLIT && p == 0) {  // the root takes both chains' wrenches (its own subtree momentum is not used)
        Fx[0] += pair_sum(Fx[b]);
        Fz[0] += pair_sum(Fz[b]);
        Nr[0] += pair_sum(Nr[b]);
      } else {
        Fx[p] += Fx[b];
        Fz[p] += Fz[b];
        Nr[p] += Nr[b];
        Px[p] += Px[b];
        Pz[p] += Pz[b];
      }
    }
#pragma unroll
    for (int j = 1; j < NB; ++j) {
      const float* J = Jp[j];
      const float phi = q[2 + j], phid = u[2 + j];
      const float lim = fmaxf(J[J_LO] - phi, 0.f) - fmaxf(phi - J[J_HI], 0.f);
      const float tj = tau[j - 1] - J[J_DAMP] * phid - J[J_STIFF] * (phi - J[J_REST]) + J[J_LIMK] * lim;
      const float Q = Nr[j] - (k.hx[j] * Fz[j] - k.hz[j] * Fx[j]);
      const float dT = k.vhz[j] * Px[j] - k.vhx[j] * Pz[j];
      pi[2 + j] += dt * (tj + Q + dT);
    }
    if (fr(2)) pi[2] += dt * (Nr[0] - (u[0] * pi[1] - u[1] * pi[0]));
    if (fr(0)) pi[0] += dt * Fx[0];
    if (fr(1)) pi[1] += dt * Fz[0];
    solve(m, k, false);
  }
};

template <int V>
__global__ void __launch_bounds__(256) planar_rollout_kernel(const float* __restrict__ W, int64_t P, int N, int h1, int h2,
                                                             const PlanarModel m, const float* __restrict__ init, int cap,
                                                             float* __restrict__ ret, int* __restrict__ steps_out, int waves_per_block) {
  constexpr int T = VARIANTS[V].topo, LOCK = VARIANTS[V].lock, KIND = VARIANTS[V].kind;
  constexpr bool ROOT_ACT = VARIANTS[V].root_act, HINGE_ACT = VARIANTS[V].hinge_act;
  // T == 2 (a root with two chains of 3): every lane integrates the chain of 4 made of the root and its own chain
  constexpr bool SPLIT = T == 2;
  using C = Chain<SPLIT ? 1 : T, SPLIT, LOCK, ROOT_ACT, KIND == K_BALANCE_TIP || KIND == K_REACH>;
  constexpr int NBT = TOPO_NB[T], NDT = NBT + 2, NA = variant_act(V);  // the whole model
  constexpr int ND = C::ND, NJ = C::NB - 1;                            // this lane's part
  constexpr int NOV = variant_obs(V);                                  // observation entries before obs_skip
  extern __shared__ float smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ind = blockIdx.x * waves_per_block + wv;
  const bool w1reg = w1_in_registers(h1);
  const float* H = m.v;
  const int skip = (int)H[H_SKIP], nsub = (int)H[H_SUB];
  const int no = NOV - skip;
  // per-wave LDS: weights (P, without W1 when it lives in registers) | 32 spare | act1 (h1) | act2 (h2) | actions (8)
  const int64_t w0 = w1reg ? (int64_t)no * h1 : 0, Pl = P - w0;
  const int64_t per = Pl + 32 + h1 + h2 + 8;
  float* wl = smem + wv * per;
  float* a1 = wl + Pl + 32;
  float* a2 = a1 + h1;
  float* a3 = a2 + h2;
  if (ind >= N) return;
  const float* wg = W + (int64_t)ind * P;
  for (int64_t i = lane; i < Pl; i += 64) wl[i] = wg[w0 + i];
  // W1 in registers: lane j keeps columns j and j + 64, one row per observation entry (zero for the skipped entries)
  float w1r[2][NOV];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = lane + 64 * c;
#pragma unroll
    for (int i = 0; i < NOV; ++i) w1r[c][i] = (w1reg && j < h1 && i >= skip) ? wg[(int64_t)(i - skip) * h1 + j] : 0.f;
  }
  const float* W1 = wl;  // (not read when W1 is in registers)
  const float* B1 = wl + ((int64_t)no * h1 - w0);
  const float* W2 = B1 + h1;
  const float* B2 = W2 + h1 * h2;
  const float* W3 = B2 + h2;
  const float* B3 = W3 + h2 * NA;
  const bool second = SPLIT && (lane & 1);
  const int joff = second ? NJ : 0;  // this lane's first hinge among the model's
  C s;
  s.load(m, second);
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int g = i < 3 ? i : i + joff;
    s.q[i] = init[g];
    s.u[i] = C::fr(i) ? init[NDT + g] : 0.f;  // a locked coordinate is at rest
  }
  float tgx = 0.f, tgz = 0.f;  // the reach task's target: the two words after q ++ u
  if (KIND == K_REACH) {
    tgx = init[2 * NDT];
    tgz = init[2 * NDT + 1];
  }
  {
    typename C::Pose k;
    s.pose(m, k);
    s.solve(m, k, true);
  }
  const float clip = H[H_CLIP] > 0.f ? H[H_CLIP] : __builtin_inff();
  const float idtc = 1.f / (H[H_DT] * (float)nsub);
  float total = 0.f;
  int t = 0;
  __builtin_amdgcn_wave_barrier();
  for (; t < cap; ++t) {
    float o[NOV];  // the observation entries, lane-uniform
    if constexpr (KIND == K_RUN) {  // the whole model's q ++ u
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const float ui = fminf(fmaxf(s.u[i], -clip), clip);
        if (SPLIT && i >= 3) {  // hinges: the first chain's from lane 0, the second's from lane 1
          o[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.q[i]), 0));
          o[i + NJ] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s.q[i]), 1));
          o[NDT + i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ui), 0));
          o[NDT + i + NJ] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ui), 1));
        } else {
          o[i] = s.q[i];
          o[NDT + i] = ui;
        }
      }
    } else {
      int n = 0;  // a constant after unrolling
      if constexpr (KIND == K_BALANCE || KIND == K_BALANCE_TIP) {  // free root coordinates, hinges, free velocities
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (C::fr(i)) o[n++] = s.q[i];
        if constexpr (KIND == K_BALANCE) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) o[n++] = s.q[3 + j];
        } else {
#pragma unroll
          for (int j = 0; j < NJ; ++j) o[n++] = __sinf(s.q[3 + j]);
#pragma unroll
          for (int j = 0; j < NJ; ++j) o[n++] = __cosf(s.q[3 + j]);
        }
#pragma unroll
        for (int i = 0; i < ND; ++i)
          if (C::fr(i)) o[n++] = s.u[i];
      } else {  // reach: cos φ, sin φ, target, φ̇, tip − target, 0 (the out-of-plane component of Brax's layout)
#pragma unroll
        for (int j = 0; j < NJ; ++j) o[n++] = __cosf(s.q[3 + j]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) o[n++] = __sinf(s.q[3 + j]);
        o[n++] = tgx;
        o[n++] = tgz;
#pragma unroll
        for (int j = 0; j < NJ; ++j) o[n++] = s.u[3 + j];
        o[n++] = s.tipx - tgx;
        o[n++] = s.tipz - tgz;
        o[n++] = 0.f;
      }
    }
    if (w1reg) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int j = lane + 64 * c;
        if (j < h1) {
          float acc = B1[j];
#pragma unroll
          for (int i = 0; i < NOV; ++i) acc = fmaf(o[i], w1r[c][i], acc);
          a1[j] = tanhf(acc);
        }
      }
    } else {
      for (int j = lane; j < h1; j += 64) {
        float acc = B1[j];
#pragma unroll
        for (int i = 0; i < NOV; ++i)
          if (i >= skip) acc = fmaf(o[i], W1[(i - skip) * h1 + j], acc);
        a1[j] = tanhf(acc);
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int j = lane; j < h2; j += 64) {
      float acc = B2[j];
      for (int i = 0; i < h1; ++i) acc = fmaf(a1[i], W2[i * h2 + j], acc);
      a2[j] = tanhf(acc);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < NA) {
      float acc = B3[lane];
      for (int i = 0; i < h2; ++i) acc = fmaf(a2[i], W3[i * NA + lane], acc);
      a3[lane] = tanhf(acc);
    }
    __builtin_amdgcn_wave_barrier();
    float tau[NJ], csum = 0.f, froot = 0.f;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const float a = fminf(fmaxf(a3[j], -1.f), 1.f);
      csum += a * a;
    }
    // action columns: the root slider's first, then the hinges in body order; a passive hinge reads none
    if (ROOT_ACT) froot = s.Jp[0][J_GEAR] * fminf(fmaxf(a3[0], -1.f), 1.f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) tau[j] = HINGE_ACT ? s.Jp[j + 1][J_GEAR] * fminf(fmaxf(a3[(ROOT_ACT ? 1 : 0) + joff + j], -1.f), 1.f) : 0.f;
    __builtin_amdgcn_wave_barrier();  // a1..a3 are rewritten next step
    const float x0 = s.q[0];
    for (int kk = 0; kk < nsub; ++kk) s.substep(m, tau, froot);
    float nf = 0.f;
#pragma unroll
    for (int i = 0; i < ND; ++i) nf += s.q[i] * 0.f + s.u[i] * 0.f;  // NaN unless every entry is finite
    if (SPLIT) nf = pair_sum(nf);
    bool healthy = nf == 0.f;
    float reward;
    if constexpr (KIND == K_RUN) {
      healthy = (s.q[1] > H[H_ZLO]) && (s.q[1] < H[H_ZHI]) && (fabsf(s.q[2]) < H[H_PITCH]) && healthy;
      reward = (s.q[0] - x0) * idtc + H[H_HEALTHY] - H[H_CTRL] * csum;
    } else if constexpr (KIND == K_BALANCE) {  // the first pole's absolute angle
      healthy = (fabsf(s.q[2] + s.q[3]) < H[H_PITCH]) && healthy;
      reward = H[H_HEALTHY] - H[H_CTRL] * csum;
    } else if constexpr (KIND == K_BALANCE_TIP) {
      healthy = (s.tipz > H[H_ZLO]) && healthy;
      float vel = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) vel += m.v[HDR + MAXB * BODY + (j + 1) * HINGE + J_VELCOST] * (s.u[3 + j] * s.u[3 + j]);
      const float dz = s.tipz - H[H_TIPGOAL];
      reward = H[H_HEALTHY] - (H[H_TIPX] * (s.tipx * s.tipx) + dz * dz) - vel;
    } else {
      const float dx = s.tipx - tgx, dz = s.tipz - tgz;
      healthy = healthy && ((tgx + tgz) * 0.f == 0.f);
      reward = -sqrtf(dx * dx + dz * dz) - H[H_CTRL] * csum;
    }
    if (!healthy) break;  // sticky done: the terminating step earns nothing
    total += reward;
  }
  if (lane == 0) {
    ret[ind] = total;
    steps_out[ind] = t;
  }
}

// what the actions of the table's model drive, against a variant's pattern
bool actuation_matches(const float* model, int v) {
  const int nb = TOPO_NB[VARIANTS[v].topo];
  const float* J0 = model + HDR + MAXB * BODY;
  const bool slider = J0[J_GEAR] != 0.f || J0[J_LIMK] != 0.f;
  if (VARIANTS[v].root_act ? J0[J_GEAR] == 0.f : slider) return false;
  for (int j = 1; j < nb; ++j)
    if ((J0[j * HINGE + J_GEAR] != 0.f) != VARIANTS[v].hinge_act) return false;
  return true;
}

// the instantiation for the table's tree shape, locked root coordinates, task kind and actuation, or -1
int variant_of(const float* model) {
  const int nb = (int)model[H_NB];
  for (int v = 0; v < NVARIANT; ++v) {
    const int t = VARIANTS[v].topo;
    if (TOPO_NB[t] != nb || model[H_LOCK] != (float)VARIANTS[v].lock || model[H_KIND] != (float)VARIANTS[v].kind) continue;
    bool same = actuation_matches(model, v);
    for (int b = 0; b < nb; ++b) same = same && (int)model[HDR + b * BODY + B_PAR] == TOPO_PAR[t][b];
    if (same) return v;
  }
  return -1;
}

template <int V>
void launch(const float* W, int64_t P, int N, int h1, int h2, const PlanarModel& m, const float* init, int cap, float* ret, int* steps,
            hipStream_t s) {
  const int no = variant_obs(V) - (int)m.v[H_SKIP];
  const int64_t per = (P - (w1_in_registers(h1) ? (int64_t)no * h1 : 0) + 32 + h1 + h2 + 8) * 4;
  int waves = 4;
  while (waves > 1 && per * waves > 160 * 1024) --waves;
  const int blocks = (N + waves - 1) / waves;
  (void)hipFuncSetAttribute((const void*)planar_rollout_kernel<V>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(per * waves));
  planar_rollout_kernel<V><<<blocks, 64 * waves, per * waves, s>>>(W, P, N, h1, h2, m, init, cap, ret, steps, waves);
}

}  // namespace

int evx_planar_table_words() { return TABLE; }

// 0 when the kernel is instantiated for the table's combination of tree shape, root constraint, task kind and
// actuation, else -1 (the table is host memory)
int evx_planar_supported(const float* model) { return variant_of(model) >= 0 ? 0 : -1; }

// observations (after obs_skip), actions and auxiliary state words of a supported table's model; -1 when it is not supported
int evx_planar_dims(const float* model, int* no, int* na, int* naux) {
  const int v = variant_of(model);
  if (v < 0) return -1;
  *no = variant_obs(v) - (int)model[H_SKIP];
  *na = variant_act(v);
  *naux = variant_aux(v);
  return 0;
}

void evx_planar_rollout(const float* W, int64_t P, int N, int h1, int h2, const float* model, const float* init, int cap, float* ret,
                        int* steps, hipStream_t s) {
  PlanarModel m;
  for (int i = 0; i < TABLE; ++i) m.v[i] = model[i];
  switch (variant_of(model)) {
    case 0: launch<0>(W, P, N, h1, h2, m, init, cap, ret, steps, s); break;
    case 1: launch<1>(W, P, N, h1, h2, m, init, cap, ret, steps, s); break;
    case 2: launch<2>(W, P, N, h1, h2, m, init, cap, ret, steps, s); break;
    case 3: launch<3>(W, P, N, h1, h2, m, init, cap, ret, steps, s); break;
    case 4: launch<4>(W, P, N, h1, h2, m, init, cap, ret, steps, s); break;
    case 5: launch<5>(W, P, N, h1, h2, m, init, cap, ret, steps, s); break;
    default: break;  // rejected by the binding (evx_planar_supported)
  }
}
