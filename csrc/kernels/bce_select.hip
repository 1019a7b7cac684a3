// BCE-IBEA's PC selection and exploration on the device (evoxmi/algorithms/mo/bce_ibea.py, evoxmi/ops/bce.py).
// No (n, n) distance or ratio matrix is stored: every kernel recomputes the entries it needs from the
// m ≤ 16 objectives, which arrive transposed and zero padded to M ∈ {2, 3, 4, 8, 16} rows, (M, n).
//
// The contract (the float64 reference of the tests implements the same formulas):
//   mask     the rows that no row dominates (the test of evx::dominates), or the caller's mask;
//            n_nd its count
//   span_k   max(f_max_k − f_min_k, 1e-12) over the masked rows (fminf / fmaxf; a padded objective gets 1e-12
//            and contributes δ = 0)
//   d2(i, j) Σ_k fmaf(δ_k, δ_k, ·), δ_k = (o_ik − o_jk) / span_k with an IEEE division, k ascending from 0.f:
//            the difference is taken first (normalising first cancels for close neighbours); bitwise
//            symmetric (δ only changes sign) and bitwise equal at every call site.  A NaN d2 is +inf.
//   t_i      sqrt(third smallest d2(i, j)) over the other masked rows with multiplicity, +inf where there are
//            fewer than three; 0 is stored for a row outside the mask
//   r        (Σ_i t_i) / n_nd.  Order of the sum: thread τ of 256 adds t[τ], t[τ + 256], … in ascending
//            order from 0.f, a xor tree (offsets 32 … 1) adds the 64 lanes of a wave, and the four wave sums
//            are added in ascending wave order.
//   R(i, j)  q = sqrt(d2) / r (IEEE), R = q > 1 ? 1 : q: a NaN q stays NaN
//   P_j      Π R(i, j) over the live masked rows i ≠ j.  Order of the product, the same in the score pass
//            and in the removal kernel whatever their launch shapes: the rows i ≡ c (mod 512) are multiplied
//            in ascending order from 1.f for each class c; a xor tree (offsets 32 … 1) multiplies the 64
//            classes 64·W … 64·W + 63; the eight results W = 0 … 7 are multiplied in ascending order from 1.f.
//            The absorbing factors are counted apart (C_j: NaN factors in its low half, zero factors in its
//            high half; at most 8191 each) and left out of the product: P_j is NaN exactly when there is a NaN
//            factor and otherwise 0 exactly when there is a zero factor, as the plain product would be, and
//            removing a row whose factor was NaN or 0 only decrements the count.  Duplicate rows have factor 0
//            to one another (NaN where r = 0), and BCE pads PC with copies of one row: without the counts every
//            removal of a copy rescanned every other copy (1.1 ms per removal with 800 copies at n = 2048).
//   score_j  1 − P_j; k = max(0, n_nd − n_keep) times (at most n − n_keep: the host bound of the loop) the
//            live masked row of greatest (score, lowest index) leaves, a NaN score counting as greatest.  The
//            difference is never formed: the greatest 1 − P is the least P, and the rows are compared on P
//            itself, whose float32 error is relative to the product (1 − P would round every P < 2⁻²⁵ to 1).
//
// Launches of a PC selection, and why they are split so:
//   bce_mask_kernel    a wave per row, grid-wide: the mask needs every row against every row.
//   bce_bounds_kernel  one workgroup: count and the m spans need the whole mask; ordered, no atomics.
//   bce_niche_kernel   a wave per row, grid-wide, needs the spans: each lane keeps its three smallest d2 over
//                      the rows ≡ lane (mod 64), a xor merge of the triples gives the third smallest.
//   bce_radius_kernel  one workgroup: the ordered sum of t, r left in a device word (ws[16]).
//   bce_score_kernel   a wave per row, grid-wide, needs r: P_j and C_j of every masked row.  Inside the
//                      removal kernel this start-up would be n² factors on one CU.
//   bce_remove_kernel  one workgroup of T = 256 or 512 threads, n ≤ 8192.
// Merging any two would need a grid-wide barrier (spin) or atomics; both are ruled out for reproducibility.
// Inside a PC selection the niche, radius and score launches return at once where n_nd ≤ n_keep (the count is
// read from the device word): nothing will be removed and t, r, P are not needed.
//
// bce_remove_kernel.  Thread r keeps P, C and the live bits of the IT rows r, r + T, … in registers.  A step:
// every live row computes its factor against the row x that left in the previous step; a NaN or zero factor
// decrements its count in C, any other factor ≠ 1 (d2 < r² up to rounding: the exact test is on the factor itself, so a stale
// product can never differ from a recomputed one) puts the row on its wave's LDS list; the arg-max of
// (score, lowest index) over the other live rows travels with the same barrier.  The listed rows (2.6–3.3 per
// removal on random fronts) recompute P cooperatively, up to B = 8 (M ≤ 4), 4 (M = 8) or 2 of them per pass with
// one barrier per pass (a pass is instantiated for 1, 2, 3, 4 and 8 targets): every thread multiplies the factors
// of its live rows per class, a xor tree per class wave, partials through LDS, folded in the fixed order above.
// The listed rows' new keys are folded into the arg-max after their pass: a step costs one barrier and one per pass,
// 1 + ⌈rescans / B⌉ for B = 4 and 2.  For B = 8 a remainder of 5 to 7 targets runs as a pass of 4 and a pass of 1
// to 3 (no pass is instantiated for 5, 6 or 7 targets): ⌊rescans / 8⌋ passes plus one for a remainder of 1 to 4 and
// two for 5 to 7, so 5 to 7 rescans are 3 barriers.
// Both the test against x and the passes first compare a distance formed with reciprocal spans against
// r²·(1 + 2⁻¹⁶): above it the factor is exactly 1 and nothing is multiplied, so the IEEE divisions and the
// square root of the contract run only for the few rows inside the radius (a NaN takes the exact path).  Without
// this filter a step at n = 8192, m = 3 took 21.9 µs, with it 8.8 µs.  With T = 256 a thread's rows alternate between the
// classes r and r + 256, so it keeps two partial products and its wave writes two of the eight partials.
// Static trip counts apart from k and the rescan count, no atomics, no spin: bitwise reproducible.  LDS
// partials are double buffered (a buffer is rewritten two barriers after it was read).
//
// Exploration: the bounds, niche and radius launches over all N rows of PC (no mask) give r0 = mean t_i;
// bce_count_kernel, a wave per PC row, counts the NPC rows with d2 ≤ (n_nd / N · r0)² on the PC spans and
// writes count ≤ 1; n_nd is read from device memory.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage); no kernel uses scratch.  A thread's
// objective rows stay in registers for M ≤ 3; the rows of M ≥ 4 are re-read from L2 in groups of 8 (M = 4) or 4.
//   kernel <IT, M, T>              VGPR  AGPR  SGPR  scratch  LDS [B]
//   bce_mask                       44    0     62    0        256
//   bce_bounds                     22    0     38    0        48
//   bce_niche                      40    0     52    0        320
//   bce_radius                     8     0     17    0        16
//   bce_score                      30    0     41    0        320
//   bce_count                      39    0     40    0        320
//   bce_remove<1, 2, 256>          76    0     79    0        17696
//   bce_remove<1, 3, 256>          66    0     89    0        17696
//   bce_remove<1, 4, 256>          72    0     106   0        17696
//   bce_remove<1, 8, 256>          99    0     106   0        17184
//   bce_remove<1, 16, 256>         146   0     106   0        16928
//   bce_remove<2, 2, 256>          82    0     86    0        17696
//   bce_remove<2, 3, 256>          86    0     93    0        17696
//   bce_remove<2, 4, 256>          99    0     106   0        17696
//   bce_remove<2, 8, 256>          127   0     106   0        17184
//   bce_remove<2, 16, 256>         184   0     106   0        16928
//   bce_remove<4, 2, 256>          98    0     95    0        17696
//   bce_remove<4, 3, 256>          100   0     102   0        17696
//   bce_remove<4, 4, 256>          109   0     106   0        17696
//   bce_remove<4, 8, 256>          138   0     106   0        17184
//   bce_remove<4, 16, 256>         196   0     106   0        16928
//   bce_remove<8, 2, 256>          128   0     104   0        17696
//   bce_remove<8, 3, 256>          135   0     104   0        17696
//   bce_remove<8, 4, 256>          209   0     104   0        17696
//   bce_remove<8, 8, 256>          129   0     106   0        17184
//   bce_remove<8, 16, 256>         134   0     106   0        16928
//   bce_remove<8, 2, 512>          131   0     104   0        17696
//   bce_remove<8, 3, 512>          134   0     104   0        17696
//   bce_remove<8, 4, 512>          233   0     104   0        17696
//   bce_remove<8, 8, 512>          129   0     106   0        17184
//   bce_remove<8, 16, 512>         123   0     106   0        16928
//   bce_remove<16, 2, 512>         202   0     106   0        17696
//   bce_remove<16, 3, 512>         217   0     106   0        17696
//   bce_remove<16, 4, 512>         160   0     104   0        17696
//   bce_remove<16, 8, 512>         170   0     106   0        17184
//   bce_remove<16, 16, 512>        194   0     106   0        16928
// 256 threads are one wave per SIMD, 512 threads two (256 VGPRs each).
#include "evoxmi_mo.h"

namespace {

constexpr int BC_ROWS = 4;  // rows (waves) per workgroup of the grid-wide kernels
constexpr int BC_GRID_THREADS = 64 * BC_ROWS;
constexpr int BC_MAX_M = 16;
constexpr int BC_MAX_N = 8192;
constexpr int BC_THREADS = 512;  // removal: at most
constexpr int BC_WAVES = BC_THREADS / 64;
constexpr int BC_R = 16;  // ws[0 … 15] the spans, ws[16] the radius
constexpr uint32_t BC_INF = 0x7f800000u;
constexpr unsigned long long BC_NO_KEY = 0ull;

// the squared normalised distance of the whole file; a(k), b(k), s(k) give the k-th objective of the two rows and its span
template <class FA, class FB, class FS>
__device__ __forceinline__ float nd2(FA a, FB b, FS s, int m) {
  float acc = 0.f;
  for (int k = 0; k < m; ++k) {
    const float d = __fdiv_rn(a(k) - b(k), s(k));
    acc = fmaf(d, d, acc);
  }
  return acc == acc ? acc : __uint_as_float(BC_INF);
}

// R(i, j) from d2 and the radius; a NaN quotient stays NaN
__device__ __forceinline__ float factor(float d, float r) {
  const float q = __fdiv_rn(__fsqrt_rn(d), r);
  return q > 1.f ? 1.f : q;
}

// (score, row) as one word whose maximum is the greatest score (the least P, a NaN first) and, among equals, the lowest row; a
// live row's key is never 0
__device__ __forceinline__ unsigned long long arg_key(float P, int C, int row) {
  // C counts the absorbing factors apart: NaN factors in its low half, zero factors in its high half
  const uint32_t s = (C & 0xffff) ? 0xffffffffu : 0x7fffffffu - ((C >> 16) ? 0u : __float_as_uint(P));  // +0 ≤ P ≤ 1: its bits are ordered
  return evx::key64(s, (uint32_t)~row);
}

// mask[i] = no row dominates row i
__global__ void __launch_bounds__(BC_GRID_THREADS) bce_mask_kernel(const float* __restrict__ oT, int n, int M, uint8_t* __restrict__ mask) {
  __shared__ float js[BC_ROWS][BC_MAX_M];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * BC_ROWS + wave;
  if (lane < M) js[wave][lane] = i < n ? oT[(int64_t)lane * n + i] : 0.f;
  __syncthreads();
  if (i >= n) return;
  const float* oi = js[wave];
  bool dominated = false;
  for (int j = lane; j < n; j += 64) {
    bool le = true, lt = false;  // row j dominates row i; not evx::dominates: with it the kernel takes two more SGPRs
    for (int k = 0; k < M; ++k) {
      const float x = oT[(int64_t)k * n + j], y = oi[k];
      le &= x <= y;
      lt |= x < y;
    }
    dominated |= le && lt;
  }
  const bool free_row = __ballot(dominated) == 0ull;
  if (lane == 0) mask[i] = free_row ? 1 : 0;
}

// cnt[0] = #mask, ws[k] = span_k; mask == nullptr: every row
__global__ void __launch_bounds__(256) bce_bounds_kernel(const float* __restrict__ oT, const uint8_t* __restrict__ mask, int n, int M,
                                                         float* __restrict__ ws, int64_t* __restrict__ cnt) {
  __shared__ float lo_s[4], hi_s[4];
  __shared__ int c_s[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inf = __uint_as_float(BC_INF);
  for (int k = 0; k < BC_MAX_M; ++k) {
    float lo = inf, hi = -inf;
    int c = 0;
    if (k < M) {
      for (int p = tid; p < n; p += 256) {
        if (mask == nullptr || mask[p] != 0) {
          const float v = oT[(int64_t)k * n + p];
          lo = fminf(lo, v);
          hi = fmaxf(hi, v);
          ++c;
        }
      }
    }
    lo = evx::wave_min(lo);
    hi = evx::wave_max(hi);
    c = evx::wave_sum(c);
    __syncthreads();  // the previous objective's partials are consumed
    if (lane == 0) {
      lo_s[wave] = lo;
      hi_s[wave] = hi;
      c_s[wave] = c;
    }
    __syncthreads();
    if (tid == 0) {
      lo = fminf(fminf(lo_s[0], lo_s[1]), fminf(lo_s[2], lo_s[3]));
      hi = fmaxf(fmaxf(hi_s[0], hi_s[1]), fmaxf(hi_s[2], hi_s[3]));
      ws[k] = fmaxf(hi - lo, 1e-12f);
      if (k == 0) cnt[0] = (int64_t)(c_s[0] + c_s[1] + c_s[2] + c_s[3]);
    }
  }
}

// t[i] = sqrt(third smallest d2(i, j)) over the other masked rows, 0 outside the mask
__global__ void __launch_bounds__(BC_GRID_THREADS) bce_niche_kernel(const float* __restrict__ oT, const uint8_t* __restrict__ mask, int n,
                                                                    int M, const float* __restrict__ ws, float* __restrict__ t,
                                                                    const int64_t* __restrict__ cnt, int n_keep) {
  if (n_keep >= 0 && cnt[0] <= (int64_t)n_keep) return;  // nothing will be removed: t and r are not needed
  __shared__ float js[BC_ROWS][BC_MAX_M];
  __shared__ float sp[BC_MAX_M];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * BC_ROWS + wave;
  if (lane < M) js[wave][lane] = i < n ? oT[(int64_t)lane * n + i] : 0.f;
  if (threadIdx.x < BC_MAX_M) sp[threadIdx.x] = ws[threadIdx.x];
  __syncthreads();
  if (i >= n) return;
  const bool masked = mask == nullptr || mask[i] != 0;
  const float inf = __uint_as_float(BC_INF);
  const float* oi = js[wave];
  float a = inf, b = inf, c = inf;  // the lane's three smallest d2, a ≤ b ≤ c
  auto insert = [&](float x) {
    const float u = fmaxf(a, x);
    a = fminf(a, x);
    const float v = fmaxf(b, u);
    b = fminf(b, u);
    c = fminf(c, v);
  };
  if (masked) {
    for (int j = lane; j < n; j += 64) {
      if (j != i && (mask == nullptr || mask[j] != 0))
        insert(nd2([&](int k) { return oi[k]; }, [&](int k) { return oT[(int64_t)k * n + j]; }, [&](int k) { return sp[k]; }, M));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oa = __shfl_xor(a, o, 64), ob = __shfl_xor(b, o, 64), oc = __shfl_xor(c, o, 64);
    insert(oa);
    insert(ob);
    insert(oc);
  }
  if (lane == 0) t[i] = masked ? __fsqrt_rn(c) : 0.f;
}

// ws[16] = (Σ t) / cnt in the order of the file header
__global__ void __launch_bounds__(256) bce_radius_kernel(const float* __restrict__ t, int n, const int64_t* __restrict__ cnt,
                                                         float* __restrict__ ws, int n_keep) {
  if (n_keep >= 0 && cnt[0] <= (int64_t)n_keep) return;
  __shared__ float part[4];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int p = tid; p < n; p += 256) s += t[p];
  s = evx::wave_sum(s);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) ws[BC_R] = __fdiv_rn(((part[0] + part[1]) + part[2]) + part[3], (float)cnt[0]);
}

// P[j], C[j] of the masked rows (1, 0 outside the mask)
__global__ void __launch_bounds__(BC_GRID_THREADS) bce_score_kernel(const float* __restrict__ oT, const uint8_t* __restrict__ mask, int n,
                                                                    int M, const float* __restrict__ ws, float* __restrict__ P,
                                                                    int32_t* __restrict__ C, const int64_t* __restrict__ cnt, int n_keep) {
  if (cnt[0] <= (int64_t)n_keep) return;  // nothing will be removed
  __shared__ float js[BC_ROWS][BC_MAX_M];
  __shared__ float sp[BC_MAX_M];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * BC_ROWS + wave;
  if (lane < M) js[wave][lane] = j < n ? oT[(int64_t)lane * n + j] : 0.f;
  if (threadIdx.x < BC_MAX_M) sp[threadIdx.x] = ws[threadIdx.x];
  __syncthreads();
  if (j >= n) return;
  const float r = ws[BC_R];
  const float* oj = js[wave];
  const bool masked = mask[j] != 0;
  float prod = 1.f;
  int nans = 0;
  for (int W = 0; W < 8; ++W) {
    float pw = 1.f;
    if (masked) {
      for (int p = 64 * W + lane; p < n; p += 512) {
        if (p != j && mask[p] != 0) {
          const float f = factor(
              nd2([&](int k) { return oT[(int64_t)k * n + p]; }, [&](int k) { return oj[k]; }, [&](int k) { return sp[k]; }, M), r);
          if (f != f)
            ++nans;
          else if (f == 0.f)
            nans += 0x10000;
          else
            pw *= f;
        }
      }
    }
    prod *= evx::wave_prod(pw);
  }
  nans = evx::wave_sum(nans);
  if (lane == 0) {
    P[j] = prod;
    C[j] = nans;
  }
}

// out[i] = #{npc row j : d2(pc_i, npc_j) ≤ (n_nd / N · r0)²} ≤ 1, on the PC spans
__global__ void __launch_bounds__(BC_GRID_THREADS) bce_count_kernel(const float* __restrict__ pcT, int N, const float* __restrict__ npcT,
                                                                    int Nn, int M, const float* __restrict__ ws,
                                                                    const int64_t* __restrict__ n_nd, uint8_t* __restrict__ out) {
  __shared__ float js[BC_ROWS][BC_MAX_M];
  __shared__ float sp[BC_MAX_M];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * BC_ROWS + wave;
  if (lane < M) js[wave][lane] = i < N ? pcT[(int64_t)lane * N + i] : 0.f;
  if (threadIdx.x < BC_MAX_M) sp[threadIdx.x] = ws[threadIdx.x];
  __syncthreads();
  if (i >= N) return;
  const float rr = __fdiv_rn((float)n_nd[0], (float)N) * ws[BC_R];
  const float thr = rr * rr;
  const float* oi = js[wave];
  int c = 0;
  for (int j = lane; j < Nn; j += 64) {
    const float d = nd2([&](int k) { return oi[k]; }, [&](int k) { return npcT[(int64_t)k * Nn + j]; }, [&](int k) { return sp[k]; }, M);
    c += d <= thr ? 1 : 0;
  }
  c = evx::wave_sum(c);
  if (lane == 0) out[i] = c <= 1 ? 1 : 0;
}

struct alignas(8) BcProd {
  float p;
  int c;
};

// oT: (M, n); blockDim.x = TB; order has n_order entries
template <int IT, int M, int TB>
__global__ void __launch_bounds__(TB) bce_remove_kernel(const float* __restrict__ oT, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ P0, const int32_t* __restrict__ C0,
                                                        const float* __restrict__ ws, int n, int n_keep, uint8_t* __restrict__ keep,
                                                        int64_t* __restrict__ order, int n_order, int32_t* __restrict__ stats) {
  constexpr bool REG = M <= 3;                       // the thread's objective rows live in registers
  constexpr int B = M <= 4 ? 8 : M <= 8 ? 4 : 2;     // rescanned rows per pass
  constexpr int MO = REG ? M : 1;
  constexpr int NC = (TB == 256 && IT > 1) ? 2 : 1;  // classes (mod 512) of a thread's rows
  constexpr int NWC = (TB == 512 || IT > 1) ? 8 : 4;  // class waves that hold rows
  // rows per unrolled group: all of them while they live in registers (one group: own[u] is own[i]); re-read rows in groups that keep
  // 64 loads in flight, not IT·M registers
  constexpr int UNR = REG ? IT : M <= 4 ? (IT < 8 ? IT : 8) : (IT < 4 ? IT : 4);
  __shared__ evx::RemovalPart partF[2][BC_WAVES];
  __shared__ BcProd partP[2][8][B];
  __shared__ uint16_t wlist[BC_MAX_N];  // wave w: entries w·64·IT …
  __shared__ int wcount[BC_WAVES];
  using Shape = evx::RemovalShape<TB>;
  constexpr int lg = Shape::lg, nt = Shape::nt, nw = Shape::nw;
  const int r = threadIdx.x, lane = r & 63, wave = r >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;

  float sp[M];
#pragma unroll
  for (int k = 0; k < M; ++k) sp[k] = ws[k];
  const float rad = ws[BC_R];
  // the cheap test that spares the divisions: a factor can differ from 1 only where the distance with reciprocal spans is not above
  // r²·(1 + 2⁻¹⁶) (the two distances differ by a few 2⁻²⁴; a NaN on either side of the comparison takes the exact path)
  float isp[M];
#pragma unroll
  for (int k = 0; k < M; ++k) isp[k] = __frcp_rn(sp[k]);
  const float thr = rad * rad * (1.f + 0x1p-16f);
  auto near = [&](const float(&a)[M], const float(&b)[M]) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const float d = (a[k] - b[k]) * isp[k];
      acc = fmaf(d, d, acc);
    }
    return !(acc > thr);
  };

  float P[IT];
  int C[IT];
  float own[IT][MO];
  uint32_t live = 0u;  // bit i: row r + i·nt is masked and not removed
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int p = r + (i << lg);
    const bool in = p < n && mask[p] != 0;
    live |= in ? (1u << i) : 0u;
    P[i] = in ? P0[p] : 1.f;
    C[i] = in ? C0[p] : 0;
#pragma unroll
    for (int k = 0; k < MO; ++k) own[i][k] = (REG && p < n) ? oT[(int64_t)k * n + p] : 0.f;
  }
  // the count and the target lookup below are the same in spea2_select.hip and bce_select.hip and stay written out: as shared
  // helpers their unrolled wave loops are reassociated before inlining and every instantiation's code length changes
  const int c = evx::wave_sum((int)__popc(live));
  if (lane == 0) wcount[wave] = c;
  __syncthreads();
  int count = 0;
  for (int w = 0; w < nw; ++w) count += wcount[w];
  const int k_remove = min(max(0, count - n_keep), n_order);

  int x = -1, rescans = 0, pq = 0;
  for (int t = 0; t <= k_remove; ++t) {
    if (t > 0) {
      if (r == 0) order[t - 1] = (int64_t)x;
      if ((x & (nt - 1)) == r) live &= ~(1u << (x >> lg));
    }
    if (t == k_remove) break;
    const int buf = t & 1;
    // every live row against the row that left: a NaN factor leaves the count, a factor below 1 asks for a rescan
    uint32_t fl = 0u;
    if (x >= 0) {
      float xv[M];
#pragma unroll
      for (int k = 0; k < M; ++k) xv[k] = oT[(int64_t)k * n + x];
      uint32_t nanb = 0u, zerob = 0u;
#pragma unroll 1
      for (int i0 = 0; i0 < IT; i0 += UNR) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int i = i0 + u, p = r + (i << lg);
          const bool on = (live >> i) & 1u;
          float o[M];
#pragma unroll
          for (int k = 0; k < M; ++k) o[k] = REG ? own[u][k < MO ? k : 0] : (p < n ? oT[(int64_t)k * n + p] : 0.f);
          if (on && near(o, xv)) {
            const float f = factor(nd2([&](int k) { return o[k]; }, [&](int k) { return xv[k]; }, [&](int k) { return sp[k]; }, M), rad);
            if (f != f)
              nanb |= 1u << i;
            else if (f == 0.f)
              zerob |= 1u << i;
            else if (f != 1.f)
              fl |= 1u << i;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < IT; ++i) C[i] -= (int)((nanb >> i) & 1u) + (int)(((zerob >> i) & 1u) << 16);
    }
    // the rows to rescan, compacted per wave; the arg-max over the others
    int cw = 0;
    unsigned long long key = BC_NO_KEY;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int p = r + (i << lg);
      const bool on = (live >> i) & 1u;
      const bool flag = (fl >> i) & 1u;
      cw = evx::wave_append(flag, (uint16_t)p, wlist + wave * (64 * IT), cw, below);
      if (on && !flag) {
        const unsigned long long q = arg_key(P[i], C[i], p);
        key = q > key ? q : key;
      }
    }
    key = evx::wave_max(key);
    if (lane == 0) partF[buf][wave] = evx::RemovalPart{key, cw};
    __syncthreads();
    int total = 0;
    key = BC_NO_KEY;
    for (int w = 0; w < nw; ++w) {
      const evx::RemovalPart q = partF[buf][w];
      const unsigned long long qk = evx::uniform(q.key);
      total += __builtin_amdgcn_readfirstlane(q.cnt);
      key = qk > key ? qk : key;
    }
    rescans += total;
    // one pass over the live rows for the NB targets b0 … b0 + NB − 1 of the waves' lists (in wave order), NB at compile time
    auto pass = [&](auto nbc, int b0) {
      constexpr int NB = decltype(nbc)::value;
      int tg[NB], cn[NB];
      float tv[NB][M], pr[NB][NC];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        int g = b0 + b, ws_ = 0, ss = 0;
        for (int w = 0; w < nw; ++w) {
          const int cnt = __builtin_amdgcn_readfirstlane(partF[buf][w].cnt);
          const bool hit = g >= 0 && g < cnt;
          ws_ = hit ? w : ws_;
          ss = hit ? g : ss;
          g -= cnt;
        }
        tg[b] = __builtin_amdgcn_readfirstlane((int)wlist[ws_ * (64 * IT) + ss]);
        cn[b] = 0;
#pragma unroll
        for (int q = 0; q < NC; ++q) pr[b][q] = 1.f;
#pragma unroll
        for (int k = 0; k < M; ++k) tv[b][k] = oT[(int64_t)k * n + tg[b]];
      }
#pragma unroll 1
      for (int i0 = 0; i0 < IT; i0 += UNR) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int i = i0 + u, p = r + (i << lg);
          const bool on = (live >> i) & 1u;
          float o[M];
#pragma unroll
          for (int k = 0; k < M; ++k) o[k] = REG ? own[u][k < MO ? k : 0] : (p < n ? oT[(int64_t)k * n + p] : 0.f);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (on && p != tg[b] && near(o, tv[b])) {  // elsewhere the factor is 1 and multiplies exactly
              const float f = factor(nd2([&](int k) { return o[k]; }, [&](int k) { return tv[b][k]; }, [&](int k) { return sp[k]; }, M), rad);
              if (f != f)
                ++cn[b];
              else if (f == 0.f)
                cn[b] += 0x10000;
              else
                pr[b][u & (NC - 1)] *= f;  // UNR is even where NC = 2: u and i have one parity
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int cs = evx::wave_sum(cn[b]);
#pragma unroll
        for (int q = 0; q < NC; ++q) {
          const float v = evx::wave_prod(pr[b][q]);
          if (lane == 0) partP[pq][wave + q * nw][b] = BcProd{v, q == 0 ? cs : 0};
        }
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float np = 1.f;
        int nc = 0;
#pragma unroll
        for (int W = 0; W < NWC; ++W) {
          const BcProd q = partP[pq][W][b];
          np *= q.p;
          nc += q.c;
        }
        const bool mine = (tg[b] & (nt - 1)) == r;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
          const bool hit = mine && (tg[b] >> lg) == i;
          P[i] = hit ? np : P[i];
          C[i] = hit ? nc : C[i];
        }
        const unsigned long long ak = evx::uniform(arg_key(np, nc, tg[b]));
        key = ak > key ? ak : key;
      }
      pq ^= 1;
    };
    for (int b0 = 0; b0 < total;) {
      const int nb = total - b0;
      if constexpr (B >= 8) {
        if (nb >= 8) {
          pass(std::integral_constant<int, 8>{}, b0);
          b0 += 8;
          continue;
        }
      }
      if constexpr (B >= 4) {
        if (nb >= 3) {
          if (nb == 3)
            pass(std::integral_constant<int, 3>{}, b0);
          else
            pass(std::integral_constant<int, 4>{}, b0);
          b0 += 4;
          continue;
        }
      }
      if (nb >= 2)
        pass(std::integral_constant<int, 2>{}, b0);
      else
        pass(std::integral_constant<int, 1>{}, b0);
      b0 += 2;
    }
    x = key == BC_NO_KEY ? -1 : (int)~(uint32_t)key;
  }

  evx::removal_finish<IT, TB>(live, n, k_remove, rescans, keep, order, n_order, stats);
}

inline int grid_rows(int n) { return (n + BC_ROWS - 1) / BC_ROWS; }

}  // namespace

int evx_bce_max_n() { return BC_MAX_N; }
int evx_bce_max_m() { return BC_MAX_M; }
int evx_bce_ws_floats() { return BC_R + 1; }

void evx_bce_mask(const float* objT, int n, int M, uint8_t* mask, hipStream_t s) {
  if (n <= 0 || M != evx_padded_m(M)) return;
  bce_mask_kernel<<<grid_rows(n), BC_GRID_THREADS, 0, s>>>(objT, n, M, mask);
}

void evx_bce_niche(const float* objT, int n, int M, const uint8_t* mask, float* t, float* ws, int64_t* cnt, int n_keep, hipStream_t s) {
  if (n <= 0 || M != evx_padded_m(M)) return;
  bce_bounds_kernel<<<1, 256, 0, s>>>(objT, mask, n, M, ws, cnt);
  bce_niche_kernel<<<grid_rows(n), BC_GRID_THREADS, 0, s>>>(objT, mask, n, M, ws, t, cnt, n_keep);
  bce_radius_kernel<<<1, 256, 0, s>>>(t, n, cnt, ws, n_keep);
}

void evx_bce_remove(const float* objT, int n, int M, const uint8_t* mask, const float* ws, const int64_t* cnt, float* P, int32_t* C,
                    int n_keep, uint8_t* keep, int64_t* order, int n_order, int32_t* stats, hipStream_t s) {
  if (n <= 0 || n > BC_MAX_N || M != evx_padded_m(M)) return;
  bce_score_kernel<<<grid_rows(n), BC_GRID_THREADS, 0, s>>>(objT, mask, n, M, ws, P, C, cnt, n_keep);
  evx::dispatch_removal_shape(n, [&](auto it, auto tb) {
    evx::dispatch_padded_m(M, [&](auto mm) {
      constexpr int IT = decltype(it)::value, TB = decltype(tb)::value, MM = decltype(mm)::value;
      bce_remove_kernel<IT, MM, TB><<<1, TB, 0, s>>>(objT, mask, P, C, ws, n, n_keep, keep, order, n_order, stats);
    });
  });
}

void evx_bce_count(const float* pcT, int N, const float* npcT, int Nn, int M, const float* ws, const int64_t* n_nd, uint8_t* out,
                   hipStream_t s) {
  if (N <= 0 || M != evx_padded_m(M)) return;
  bce_count_kernel<<<grid_rows(N), BC_GRID_THREADS, 0, s>>>(pcT, N, npcT, Nn, M, ws, n_nd, out);
}
