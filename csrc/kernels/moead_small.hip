// MOEA/D generation at benchmark shapes (N = 91…300 subproblems, T = 10…30 neighbours, d = 12…30), R independent
// runs per launch: the kernels behind BatchedRuns(MOEAD).  moead.hip is built for N = 16 290, d = 10 000 (four passes
// over a chip-wide grid and a reverse-neighbour CSR from torch sorts); here a generation is two launches.
//
//   ask  — a wave per offspring, the run on grid.y.  The wave draws its two parents (the two smallest (u24, j) of
//          row i of uniform(key, (N, T)), as parents_kernel), keeps them in registers, and its lanes stride over the
//          d genes of the row: gather both parent genes, regenerate the SBX word, the pair rate and the PM site / μ
//          from the counters of variation4_kernel / variation1_kernel, clip, write the child once.  No LDS, and
//          (p0, p1) go to memory only as an output.
//   tell — one workgroup of 1024 threads per run, no reverse-neighbour CSR.  (1) z' = min(z, colmin(off_obj)) and
//          z_max = colmax(pop_obj), a wave per objective, NaN propagating as torch's; z', z_max and (where N·m ≤ 8192)
//          the offspring objectives go to LDS.  (2) The N·T (offspring i, slot s = nb[i, t]) pairs are dealt over
//          the threads in the forward direction; a pair whose aggregate v is not NaN does a 64-bit LDS atomic min of
//          (ordered_bits(v + 0) << 32) | i into best[s].  The minimum of packed words does not depend on the
//          schedule and is the replace_kernel order (v < best) || (v == best && i < bi): the first strict minimiser
//          over the offspring whose neighbourhood holds s.  (The v + 0 keeps the packed order equal to the float order
//          by construction.  No input shows it: every candidate of a slot is aggregated with the slot's own weights, so
//          the zeros of one slot's candidates carry one sign, and the weighted sum and PBI add onto +0.)  (3) Slot s unpacks its word, aggregates its occupant and
//          takes the winner iff there is one and best < old, strictly, as floats.  (4) The workgroup copies the N·d
//          genes: new_pop[s] = win[s] ≥ 0 ? off[win[s]] : pop[s].
//
// Run r of either kernel is bit-identical to the solo launches of moead.hip on run r's operands: the counters are
// run-local and the gene and aggregation routines are the same definitions (evoxmi_moead.h).
#include "evoxmi_launchers.h"
#include "evoxmi_moead.h"

namespace {
using namespace evx;
using namespace evx::moead;

constexpr int TELL_THREADS = 1024;
constexpr int TELL_MAX_N = 2048;       // best[] and win[] in LDS
constexpr int TELL_STAGE_FLOATS = 8192;  // offspring objectives staged in LDS up to this many floats (32 KB)

// V4: d % 4 == 0 and every row 16-byte aligned
template <bool V4>
__global__ void __launch_bounds__(256) small_ask_kernel(const float* __restrict__ pop, const int64_t* __restrict__ nb, int64_t nb_run,
                                                        const int64_t* __restrict__ key, const int64_t* __restrict__ kx,
                                                        const int64_t* __restrict__ km, const float* __restrict__ lb,
                                                        const float* __restrict__ ub, float pro_c, float dis_c, float pro_m,
                                                        float dis_m, int nm, int N, int T, int d, float* __restrict__ off,
                                                        int32_t* __restrict__ parents) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const int64_t run = blockIdx.y;
  pop += run * N * d;
  off += run * N * d;
  nb += run * nb_run + (int64_t)i * T;
  uint32_t k0, k1;
  load_key(key + run * 2, k0, k1);
  uint64_t m1, m2;
  row_min2((uint64_t)i, T, k0, k1, m1, m2);
  const int p0 = (int)nb[(uint32_t)m1], p1 = (int)nb[(uint32_t)(T > 1 ? m2 : m1)];
  if (lane == 0) {
    parents[run * 2 * N + i] = p0;
    parents[run * 2 * N + N + i] = p1;
  }
  float* out = off + (int64_t)i * d;
  if ((unsigned)p0 >= (unsigned)N || (unsigned)p1 >= (unsigned)N) {  // a neighbour outside the population: no row to read
    for (int j = lane; j < d; j += 64) out[j] = NAN;
    return;
  }
  const VarKeys K = load_keys(kx + run * 4, km + run * 4);
  const float e = 1.f / (dis_c + 1.f), e1 = dis_m + 1.f, inv = 1.f / (dis_m + 1.f), pr = pro_m / d;
  const bool no_x = u24(word_at((uint64_t)i, K.pr0, K.pr1)) > pro_c;
  const float* ra = pop + (int64_t)p0 * d;
  const float* rb = pop + (int64_t)p1 * d;
  if (V4) {
    for (int j = lane << 2; j < d; j += 256) {
      const float4 a = *reinterpret_cast<const float4*>(ra + j), b = *reinterpret_cast<const float4*>(rb + j);
      const float4 lo = *reinterpret_cast<const float4*>(lb + j), hi = *reinterpret_cast<const float4*>(ub + j);
      *reinterpret_cast<float4*>(out + j) = child4(a, b, lo, hi, (uint64_t)i * d + j, i < nm, no_x, K, e, pr, e1, inv);
    }
  } else {
    for (int j = lane; j < d; j += 64)
      out[j] = child1(ra[j], rb[j], lb[j], ub[j], (uint64_t)i * d + j, i < nm, no_x, K, e, pr, e1, inv);
  }
}

// an image of a float that orders as the float does (no NaN comes here)
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

template <int MT, bool V4>
__global__ void __launch_bounds__(TELL_THREADS) small_tell_kernel(const float* __restrict__ pop, const float* __restrict__ off,
                                                                  const float* __restrict__ pop_obj, const float* __restrict__ off_obj,
                                                                  const float* __restrict__ W, int64_t w_run,
                                                                  const int64_t* __restrict__ nb, int64_t nb_run,
                                                                  const float* __restrict__ zin, int func, int N, int T, int Mrt, int d,
                                                                  int stage, float* __restrict__ new_pop, float* __restrict__ new_obj,
                                                                  float* __restrict__ zout, int32_t* __restrict__ win_out) {
  constexpr int MA = MT > 0 ? MT : MAXM;
  const int M = MT > 0 ? MT : Mrt;
  __shared__ unsigned long long best[TELL_MAX_N];
  __shared__ int32_t win[TELL_MAX_N];
  __shared__ float zs[MAXM], zms[MAXM];
  extern __shared__ float fo[];  // stage: the run's offspring objectives
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t run = blockIdx.x;
  pop += run * N * d;
  off += run * N * d;
  new_pop += run * N * d;
  pop_obj += run * N * M;
  off_obj += run * N * M;
  new_obj += run * N * M;
  W += run * w_run;
  nb += run * nb_run;

  // (1) reference points: wave k reduces objective k
  if (wave < M) {
    float lo = INFINITY, hi = -INFINITY;
    for (int r = lane; r < N; r += 64) {
      lo = nan_min(lo, off_obj[(int64_t)r * M + wave]);
      hi = nan_max(hi, pop_obj[(int64_t)r * M + wave]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = nan_min(lo, __shfl_xor(lo, o, 64));
      hi = nan_max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
      const float z0 = zin[run * M + wave];
      const float z1 = (z0 != z0) ? z0 : nan_min(z0, lo);  // torch.minimum: either NaN stays
      zs[wave] = z1;
      zms[wave] = hi;
      zout[run * M + wave] = z1;
    }
  }
  for (int s = tid; s < N; s += TELL_THREADS) best[s] = ~0ull;
  if (stage)
    for (int e = tid; e < N * M; e += TELL_THREADS) fo[e] = off_obj[e];
  __syncthreads();

  float z[MA], zm[MA], f[MA], w[MA];
  for (int k = 0; k < M; ++k) {
    z[k] = zs[k];
    zm[k] = zms[k];
  }
  // (2) forward: every (offspring, neighbour slot) pair bids for its slot
  const float* fsrc = stage ? fo : off_obj;
  const int pairs = N * T;
  for (int p = tid; p < pairs; p += TELL_THREADS) {
    const int i = p / T;
    const int64_t s = nb[p];
    if ((uint64_t)s >= (uint64_t)N) continue;  // a neighbour outside the population holds no slot
    for (int k = 0; k < M; ++k) {
      f[k] = fsrc[i * M + k];
      w[k] = W[s * M + k];
    }
    const float v = agg(func, f, w, z, zm, M);
    if (v == v) atomicMin(&best[s], ((unsigned long long)ordered_bits(v + 0.0f) << 32) | (uint32_t)i);
  }
  __syncthreads();

  // (3) every slot against its occupant
  for (int s = tid; s < N; s += TELL_THREADS) {
    const unsigned long long word = best[s];
    const int bi = (int)(uint32_t)word;
    for (int k = 0; k < M; ++k) {
      f[k] = pop_obj[(int64_t)s * M + k];
      w[k] = W[(int64_t)s * M + k];
    }
    const float old = agg(func, f, w, z, zm, M);
    const bool take = word != ~0ull && from_ordered((uint32_t)(word >> 32)) < old;
    win[s] = take ? bi : -1;
    win_out[run * N + s] = take ? bi : -1;
    for (int k = 0; k < M; ++k) new_obj[(int64_t)s * M + k] = take ? fsrc[bi * M + k] : f[k];
  }
  __syncthreads();

  // (4) rows
  if (V4) {
    const int q = d >> 2;
    for (int e = tid; e < N * q; e += TELL_THREADS) {
      const int s = e / q, c = e - s * q;
      const int wi = win[s];
      const float* src = wi >= 0 ? off + (int64_t)wi * d : pop + (int64_t)s * d;
      reinterpret_cast<float4*>(new_pop + (int64_t)s * d)[c] = reinterpret_cast<const float4*>(src)[c];
    }
  } else {
    for (int e = tid; e < N * d; e += TELL_THREADS) {
      const int s = e / d, c = e - s * d;
      const int wi = win[s];
      new_pop[e] = wi >= 0 ? off[(int64_t)wi * d + c] : pop[e];
    }
  }
}

template <int MT>
void launch_tell(bool v4, int R, size_t lds, hipStream_t st, const float* pop, const float* off, const float* pop_obj, const float* off_obj,
                 const float* W, int64_t w_run, const int64_t* nb, int64_t nb_run, const float* z, int func, int N, int T, int M, int d,
                 int stage, float* new_pop, float* new_obj, float* zout, int32_t* win) {
  if (v4)
    small_tell_kernel<MT, true><<<R, TELL_THREADS, lds, st>>>(pop, off, pop_obj, off_obj, W, w_run, nb, nb_run, z, func, N, T, M, d, stage,
                                                              new_pop, new_obj, zout, win);
  else
    small_tell_kernel<MT, false><<<R, TELL_THREADS, lds, st>>>(pop, off, pop_obj, off_obj, W, w_run, nb, nb_run, z, func, N, T, M, d, stage,
                                                               new_pop, new_obj, zout, win);
}

}  // namespace

int evx_moead_small_max_n() { return TELL_MAX_N; }
int evx_moead_small_max_m() { return MAXM; }

void evx_moead_small_ask(const float* pop, const int64_t* nb, int nb_per_run, const int64_t* key, const int64_t* kx, const int64_t* km,
                         const float* lb, const float* ub, float pro_c, float dis_c, float pro_m, float dis_m, int nm, int R, int N, int T,
                         int d, bool vec4, float* off, int32_t* parents, hipStream_t s) {
  if (R < 1 || R > EVX_MAX_RUNS || N < 1 || T < 1 || d < 1) return;
  const dim3 grid((N + 3) / 4, R);
  const int64_t nb_run = nb_per_run ? (int64_t)N * T : 0;
  if (vec4 && (d & 3) == 0)
    small_ask_kernel<true><<<grid, 256, 0, s>>>(pop, nb, nb_run, key, kx, km, lb, ub, pro_c, dis_c, pro_m, dis_m, nm, N, T, d, off, parents);
  else
    small_ask_kernel<false><<<grid, 256, 0, s>>>(pop, nb, nb_run, key, kx, km, lb, ub, pro_c, dis_c, pro_m, dis_m, nm, N, T, d, off, parents);
}

void evx_moead_small_tell(const float* pop, const float* off, const float* pop_obj, const float* off_obj, const float* W, int w_per_run,
                          const int64_t* nb, int nb_per_run, const float* z, int func, int R, int N, int T, int M, int d, bool vec4,
                          float* new_pop, float* new_obj, float* zout, int32_t* win, hipStream_t s) {
  if (R < 1 || R > EVX_MAX_RUNS || N < 1 || N > TELL_MAX_N || M < 1 || M > MAXM || T < 1 || T > N || d < 1) return;
  const int stage = N * M <= TELL_STAGE_FLOATS;
  const size_t lds = stage ? (size_t)N * M * sizeof(float) : 0;
  const int64_t w_run = w_per_run ? (int64_t)N * M : 0, nb_run = nb_per_run ? (int64_t)N * T : 0;
  const bool v4 = vec4 && (d & 3) == 0;
  if (M == 3) launch_tell<3>(v4, R, lds, s, pop, off, pop_obj, off_obj, W, w_run, nb, nb_run, z, func, N, T, M, d, stage, new_pop, new_obj, zout, win);
  else if (M == 2) launch_tell<2>(v4, R, lds, s, pop, off, pop_obj, off_obj, W, w_run, nb, nb_run, z, func, N, T, M, d, stage, new_pop, new_obj, zout, win);
  else launch_tell<0>(v4, R, lds, s, pop, off, pop_obj, off_obj, W, w_run, nb, nb_run, z, func, N, T, M, d, stage, new_pop, new_obj, zout, win);
}
