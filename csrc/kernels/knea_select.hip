// KnEA's environmental selection (reference algorithms/mo/knea.py:125-179): the knee points of every front up to
// the critical one and the cut of that front, in one launch of one workgroup of 1024 threads (the fronts are
// serial through the running radius factor r and the knee ratio t).  Nothing is read on the host.
//
// Inputs: obj (n, m) float32, rank (n,) int32 or int64 sorted non-decreasing (the caller applied the stable
// argsort of the NDS ranks), 1 ≤ N < n ≤ 8192, m ≤ 16, r and t one float64 device word each.
//
// The contract.  All arithmetic is float64 on the float32 objectives, compiled without contraction (no FMA), so a
// host implementation that performs the same operations in the same order differs only in exp().
// With last = rank[N], for every front (a maximal run of equal ranks) up to the one that holds position N, its
// rows taken in position order:
//   1. extremes  mx_j, mn_j the column max and min, e_j the FIRST position that holds the column-j maximum;
//   2. plane     if the e_j are not m distinct positions: plane_j = 1 / max(E_jj, 1e-6), E the matrix of the
//                extreme rows.  Otherwise E·plane = 1 by Gaussian elimination with partial pivoting (the first
//                row on equal magnitudes; row r ← row r − (A_rc / A_cc)·row c; back substitution
//                x_c = (b_c − Σ_{k>c} A_ck·x_k) / A_cc, k ascending).  The same fallback when a pivot is
//                exactly 0 (or NaN) or a component of the result is not finite;
//   3. key       key = (float)(Σ_j obj_j·plane_j), summed in objective order from 0 in float64 and then rounded
//                to float32 (NaN → +qNaN, −0 → +0).  The scan order is ascending (key, position): the
//                extremes, whose distance is 1 ± rounding, tie at 1.0f and scan in position order;
//   4. radius    r ← r·exp(−(1 − t / knee_rate) / m),  R_j = (mx_j − mn_j)·r;
//   5. scan      a row still marked when the scan reaches it is a knee; it unmarks every other row of the front
//                with |obj_j − own_j| < R_j for all j.  The box is symmetric, so only rows later in the scan
//                can still be marked, and only those are tested;
//   6. ratio     t ← knees / front size.
// The cut: selected = rank < last | knee; dif = |selected| − N.  dif > 0 unselects dif knees of the last front by
// descending key (the lower position first on equal keys), dif < 0 selects the −dif non-knees of the last front
// by ascending (key, position).  idx are the N selected positions ascending, knee is False beyond the last front.
//
// Every loop has a trip count bounded by n, m or the number of fronts.  With NaN or infinite objectives (or a
// rank array that is not sorted) the kernel still terminates and idx holds N distinct positions in range;
// nothing more is promised for them.
//
// Steps of a front of F rows, IT = ⌈F / 1024⌉ rounded up to {1, 2, 4, 8} items per thread:
//   a. column extremes with their positions: per thread, then wave shuffles, then thread 0 over the 16 waves;
//      thread 0 also solves the m×m system in LDS, updates r and writes plane and R to LDS;
//   b. keys of the thread's IT rows, rocPRIM's stable block radix sort on the order-preserving uint32 image of
//      the canonicalised float32 key with the front slot as value: thread t then owns the scan positions
//      t·IT … t·IT + IT − 1 and keeps their rows in registers (m ≤ 4; IT ≤ 2 for m ≤ 16; otherwise they are
//      re-read through the cache);
//   c. the marks are a bitmask in LDS in scan order.  Per knee: every wave finds the next marked position at or
//      after the cursor by a ballot over the mask words (all waves get the same answer, see next_marked()), reads
//      the knee's objectives at a wave-uniform address (from the front's scan-ordered rows in LDS when F·m ≤ 24576
//      floats, which covers n = 8192 at m = 3, else through the cache), tests its own later rows and clears bits
//      with LDS atomics; one barrier per knee;
//   d. knee flags and their count; on the last front the cut: a second sort of the same items by the removal
//      (dif > 0) or completion (dif < 0) order (the keys computed again by the same operations, so that they need
//      not stay in registers across the scan), a selection bitmask by slot, an ordered compaction into idx.
// One instantiation per (padded m ∈ {4, 16}, IT), each an out-of-line function with its own register allocation:
// 32 to 120 VGPRs for IT ≤ 4 at m ≤ 4 without scratch in the scan; 128 (the cap of a 1024-thread workgroup) with
// some scratch for IT = 8 and for m > 4.  Static LDS is 155 408 bytes, 96 KiB of it the scan-ordered rows.
#include <climits>
#include <rocprim/block/block_radix_sort.hpp>

#include "evoxmi_mo.h"

namespace {

constexpr int KN_THREADS = 1024;
constexpr int KN_WAVES = KN_THREADS / 64;
constexpr int KN_MAXN = KN_THREADS * 8;  // 8192
constexpr int KN_MAXM = 16;
constexpr int KN_ROWS = 24576;            // floats of scan-ordered rows kept in LDS: a front with F·m ≤ 24576 (n = 8192 at m = 3)
constexpr uint32_t KN_PAD = 0xFFFFFFFFu;  // sorts after every key image (the largest one is +qNaN's 0xFFC00000)

template <int IT>
using kn_sort_t = rocprim::block_radix_sort<uint32_t, KN_THREADS, IT, uint32_t>;

union KnSortStorage {
  typename kn_sort_t<1>::storage_type k1;
  typename kn_sort_t<2>::storage_type k2;
  typename kn_sort_t<4>::storage_type k4;
  typename kn_sort_t<8>::storage_type k8;
};

template <int IT>
__device__ __forceinline__ typename kn_sort_t<IT>::storage_type& kn_storage(KnSortStorage& st) {
  if constexpr (IT == 1) return st.k1;
  else if constexpr (IT == 2) return st.k2;
  else if constexpr (IT == 4) return st.k4;
  else return st.k8;
}

struct KnShared {
  KnSortStorage sort;
  unsigned long long mask[KN_MAXN / 64];  // marks, bit q = scan position q
  uint32_t sel[KN_MAXN / 32];             // the cut: selected rows of the last front, bit s = front slot s
  uint16_t sslot[KN_MAXN];                // scan position → front slot
  float rows[KN_ROWS];                    // the front's rows in scan order, m floats each, when they fit
  float wmx[KN_WAVES][KN_MAXM], wmn[KN_WAVES][KN_MAXM];
  int wpos[KN_WAVES][KN_MAXM];
  double A[KN_MAXM][KN_MAXM + 1];
  double plane[KN_MAXM], R[KN_MAXM], mx[KN_MAXM], mn[KN_MAXM];
  int e[KN_MAXM];
  double r, t;
  int wcnt[KN_WAVES];
};

__device__ __forceinline__ int64_t rank_at(const void* rank, int rank64, int p) {
  return rank64 ? ((const int64_t*)rank)[p] : (int64_t)((const int32_t*)rank)[p];
}

// a wave-uniform double moved to scalar registers where the vector registers run out: 8 rows per thread at m ≤ 4
// (sixteen objectives would not fit there; with fewer rows per thread the moves cost more than they save)
template <int MT, int IT>
__device__ __forceinline__ double uniform_d(double v) {
  if constexpr (MT > 4 || IT < 8) return v;
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// block-wide exclusive prefix of one int per thread; two barriers, wcnt is free again afterwards.  Not evx::block_scan_excl plus a
// barrier: with it front<16, 8> takes two SGPRs fewer and four bytes more
__device__ __forceinline__ int block_prefix(int v, int* wcnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wcnt[wave] = inc;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < KN_WAVES; ++w) off += w < wave ? wcnt[w] : 0;
  __syncthreads();
  return off + inc - v;
}

// The first marked scan position ≥ cursor among the nw mask words, −1 when there is none; wave-uniform.
// Every wave computes it for itself after the barrier that ends a knee's step.  A wave that is already clearing
// bits for this knee while another one still searches does not change the answer: it clears only positions after
// the knee, and the knee's own bit and the (zero) bits before it are never written.
__device__ __forceinline__ int next_marked(const unsigned long long* mask, int cursor, int nw) {
  const int lane = threadIdx.x & 63, cw = cursor >> 6;
  for (int h = cw >> 6; h * 64 < nw; ++h) {
    const int w = h * 64 + lane;
    unsigned long long x = (w < nw && w >= cw) ? mask[w] : 0ull;
    if (w == cw) x &= ~0ull << (cursor & 63);
    const unsigned long long b = __ballot(x != 0ull);
    if (b) {
      const int fl = __ffsll((unsigned long long)b) - 1;
      const unsigned long long xw = __shfl(x, fl, 64);
      return __builtin_amdgcn_readfirstlane((h * 64 + fl) * 64 + __ffsll(xw) - 1);
    }
  }
  return -1;
}

// Thread 0: the extremes over the waves, the plane, the new r, R.  Padded objectives (o ≥ m) get plane 0, R +inf.
__device__ __noinline__ void plane_and_radius(KnShared& sh, const float* __restrict__ f, int m, int lo, double knee_rate) {
  int* e = sh.e;  // dynamically indexed: LDS, not scratch
  double *mx = sh.mx, *mn = sh.mn;
  for (int o = 0; o < m; ++o) {
    float bv = sh.wmx[0][o], lv = sh.wmn[0][o];
    int bp = sh.wpos[0][o];
    for (int w = 1; w < KN_WAVES; ++w) {
      const float v = sh.wmx[w][o], u = sh.wmn[w][o];
      const int p = sh.wpos[w][o];
      if (v > bv || (v == bv && p < bp)) bv = v, bp = p;
      if (u < lv) lv = u;
    }
    e[o] = bp == INT_MAX ? lo : bp;  // a column of NaN only
    mx[o] = (double)bv;
    mn[o] = (double)lv;
  }
  bool ok = true;
  for (int a = 0; a < m; ++a)
    for (int b = a + 1; b < m; ++b) ok = ok && e[a] != e[b];
  if (ok) {
    for (int a = 0; a < m; ++a) {
      for (int b = 0; b < m; ++b) sh.A[a][b] = (double)f[(int64_t)e[a] * m + b];
      sh.A[a][m] = 1.0;
    }
    for (int c = 0; c < m && ok; ++c) {
      int piv = c;
      double best = fabs(sh.A[c][c]);
      for (int r = c + 1; r < m; ++r)
        if (fabs(sh.A[r][c]) > best) best = fabs(sh.A[r][c]), piv = r;
      if (!(best > 0.0)) {  // an exact zero or NaN pivot
        ok = false;
        break;
      }
      if (piv != c)
        for (int k = 0; k <= m; ++k) {
          const double tmp = sh.A[c][k];
          sh.A[c][k] = sh.A[piv][k];
          sh.A[piv][k] = tmp;
        }
      for (int r = c + 1; r < m; ++r) {
        const double fct = sh.A[r][c] / sh.A[c][c];
        for (int k = c; k <= m; ++k) sh.A[r][k] = sh.A[r][k] - fct * sh.A[c][k];
      }
    }
    if (ok) {
      for (int c = m - 1; c >= 0; --c) {
        double s = sh.A[c][m];
        for (int k = c + 1; k < m; ++k) s = s - sh.A[c][k] * sh.plane[k];
        sh.plane[c] = s / sh.A[c][c];
      }
      for (int c = 0; c < m; ++c) ok = ok && isfinite(sh.plane[c]);
    }
  }
  if (!ok)
    for (int o = 0; o < m; ++o) sh.plane[o] = 1.0 / fmax(mx[o], 1e-6);  // E_jj is the column-j maximum
  const double r = sh.r * exp(-(1.0 - sh.t / knee_rate) / (double)m);
  sh.r = r;
  for (int o = 0; o < KN_MAXM; ++o) {
    sh.R[o] = o < m ? (mx[o] - mn[o]) * r : (double)INFINITY;
    if (o >= m) sh.plane[o] = 0.0;
  }
}

// One front: the rows at positions [lo, lo + F).  Returns nothing; sh.r and sh.t are updated by thread 0.
template <int MT, int IT>
__device__ __noinline__ void front(KnShared& sh, const float* __restrict__ f, int m, int lo, int F, double knee_rate, bool is_last,
                                      int N, bool* __restrict__ knee, int64_t* __restrict__ idx) {
  constexpr bool REG = MT * IT <= 32;  // the rows stay in registers
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, base = t * IT;
  using sort_t = kn_sort_t<IT>;

  // a. extremes (slot s = base + i, in position order)
  {
    float mxv[MT], mnv[MT];
    int mxp[MT];
#pragma unroll
    for (int o = 0; o < MT; ++o) mxv[o] = -INFINITY, mnv[o] = INFINITY, mxp[o] = INT_MAX;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int s = base + i;
      if (s < F) {
#pragma unroll
        for (int o = 0; o < MT; ++o) {
          if (o < m) {
            const float v = f[(int64_t)(lo + s) * m + o];
            if (v > mxv[o] || (v == mxv[o] && lo + s < mxp[o])) mxv[o] = v, mxp[o] = lo + s;
            if (v < mnv[o]) mnv[o] = v;
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < MT; ++o) {
      if (o < m) {  // uniform
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
          const float ov = __shfl_xor(mxv[o], d, 64), on = __shfl_xor(mnv[o], d, 64);
          const int op = __shfl_xor(mxp[o], d, 64);
          if (ov > mxv[o] || (ov == mxv[o] && op < mxp[o])) mxv[o] = ov, mxp[o] = op;
          if (on < mnv[o]) mnv[o] = on;
        }
        if (lane == 0) sh.wmx[wave][o] = mxv[o], sh.wmn[wave][o] = mnv[o], sh.wpos[wave][o] = mxp[o];
      }
    }
  }
  if (t < KN_MAXN / 32) {
    ((uint32_t*)sh.mask)[t] = 0u;
    sh.sel[t] = 0u;
  }
  __syncthreads();
  if (t == 0) plane_and_radius(sh, f, m, lo, knee_rate);
  __syncthreads();

  // b. keys, the (key, position) sort, the rows in scan order
  uint32_t k[IT], v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int s = base + i;
    k[i] = KN_PAD;
    v[i] = (uint32_t)s;
    if (s < F) {
      double acc = 0.0;
#pragma unroll
      for (int o = 0; o < MT; ++o)
        if (o < m) acc = acc + (double)f[(int64_t)(lo + s) * m + o] * sh.plane[o];
      k[i] = evx::ord_canon((float)acc);
    }
  }
  sort_t().sort(k, v, kn_storage<IT>(sh.sort));
  const bool in_lds = F * m <= KN_ROWS;  // uniform: a knee's row is then read from LDS, else through the cache
  float x[REG ? IT * MT : 1];
  double R[MT];
#pragma unroll
  for (int o = 0; o < MT; ++o) R[o] = uniform_d<MT, IT>(sh.R[o]);
  {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int q = base + i;
      if (q < F) {
        sh.sslot[q] = (uint16_t)v[i];
        bits |= 1u << i;
      }
#pragma unroll
      for (int o = 0; o < MT; ++o) {
        if (REG || in_lds) {
          const float val = (q < F && o < m) ? f[(int64_t)(lo + (int)v[i]) * m + o] : 0.f;
          if constexpr (REG) x[i * MT + o] = val;
          if (in_lds && q < F && o < m) sh.rows[q * m + o] = val;
        }
      }
    }
    if (bits) atomicOr((uint32_t*)sh.mask + (base >> 5), bits << (base & 31));  // IT divides 32: one word
  }
  __syncthreads();

  // c. the scan
  const int nw = (F + 63) >> 6;
  int cursor = 0;
  for (;;) {  // one iteration per knee: at most F
    const int q = next_marked(sh.mask, cursor, nw);
    if (q < 0) break;
    if (base + IT - 1 > q) {
      double own[MT];
      if (in_lds) {
#pragma unroll
        for (int o = 0; o < MT; ++o) own[o] = o < m ? uniform_d<MT, IT>((double)sh.rows[q * m + o]) : 0.0;
      } else {
        const int p = __builtin_amdgcn_readfirstlane(lo + (int)sh.sslot[q]);
#pragma unroll
        for (int o = 0; o < MT; ++o) own[o] = o < m ? uniform_d<MT, IT>((double)f[(int64_t)p * m + o]) : 0.0;
      }
      uint32_t clear = 0;
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int qi = base + i;
        if (qi > q && qi < F) {
          bool inside = true;
#pragma unroll
          for (int o = 0; o < MT; ++o) {
            double xv;
            if constexpr (REG) xv = (double)x[i * MT + o];
            else xv = o < m ? (double)f[(int64_t)(lo + (int)v[i]) * m + o] : 0.0;
            inside = inside && fabs(xv - own[o]) < R[o];
          }
          clear |= (inside ? 1u : 0u) << i;
        }
      }
      if (clear) atomicAnd((uint32_t*)sh.mask + (base >> 5), ~(clear << (base & 31)));
    }
    cursor = q + 1;
    __syncthreads();
  }

  // d. the knees, their count, the ratio
  uint32_t kn = 0;
  {
    const uint32_t word = ((const uint32_t*)sh.mask)[base >> 5] >> (base & 31);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      if (base + i < F) {
        const uint32_t b = (word >> i) & 1u;
        kn |= b << i;
        knee[lo + (int)v[i]] = b != 0u;
      }
    }
  }
  const int knees = evx::block_sum<KN_WAVES>(__popc(kn), sh.wcnt);
  __syncthreads();  // wcnt is free again
  if (t == 0) sh.t = (double)knees / (double)F;
  if (!is_last) return;

  // the cut (lo ≤ N < lo + F): the rows before the front, its knees, then dif of them off or −dif others on
  const int dif = lo + knees - N;  // dif ≤ knees and −dif < F − knees
#pragma unroll
  for (int i = 0; i < IT; ++i)
    if ((kn >> i) & 1u) atomicOr(&sh.sel[v[i] >> 5], 1u << (v[i] & 31));
  if (dif != 0) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const bool is_knee = (kn >> i) & 1u;
      const bool cand = base + i < F && (dif > 0 ? is_knee : !is_knee);
      k[i] = KN_PAD;
      if (cand) {  // the key again, by the same operations (not kept in registers across the scan)
        double acc = 0.0;
#pragma unroll
        for (int o = 0; o < MT; ++o) {
          if (o < m) {
            float val;
            if constexpr (REG) val = x[i * MT + o];
            else val = f[(int64_t)(lo + (int)v[i]) * m + o];
            acc = acc + (double)val * sh.plane[o];
          }
        }
        const uint32_t img = evx::ord_canon((float)acc);
        k[i] = dif > 0 ? ~img : img;  // a key image is never 0: its complement stays below KN_PAD
      }
    }
    __syncthreads();  // the knees are in sel
    sort_t().sort(k, v, kn_storage<IT>(sh.sort));  // stable on the scan order: equal keys stay in position order
    const int cnt = dif > 0 ? dif : -dif;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      if (base + i < cnt && k[i] != KN_PAD) {
        if (dif > 0) atomicAnd(&sh.sel[v[i] >> 5], ~(1u << (v[i] & 31)));
        else atomicOr(&sh.sel[v[i] >> 5], 1u << (v[i] & 31));
      }
    }
  }
  __syncthreads();
  const uint32_t mine = (sh.sel[base >> 5] >> (base & 31)) & ((1u << IT) - 1u);  // the slots base … base + IT − 1
  int out = lo + block_prefix(__popc(mine), sh.wcnt);
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    if (((mine >> i) & 1u) && out < N) idx[out++] = (int64_t)(lo + base + i);
  }
  for (int p = t; p < lo; p += KN_THREADS) idx[p] = (int64_t)p;
}

template <int MT>
__global__ void __launch_bounds__(KN_THREADS) knea_select_kernel(const float* __restrict__ f, const void* __restrict__ rank, int rank64, int n,
                                                                 int m, int N, double knee_rate, const double* __restrict__ r_in,
                                                                 const double* __restrict__ t_in, int64_t* __restrict__ idx,
                                                                 bool* __restrict__ knee, double* __restrict__ r_out,
                                                                 double* __restrict__ t_out) {
  __shared__ KnShared sh;
  const int t = threadIdx.x;
  if (t == 0) {
    sh.r = *r_in;
    sh.t = *t_in;
  }
  int lo = 0, hi = 0;
  for (;;) {  // one iteration per front: hi grows every time and the loop ends once it passes N < n
    const int64_t rk = rank_at(rank, rank64, lo);
    int a = lo + 1, b = n;  // the first position after lo whose rank differs (the ranks are sorted)
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (rank_at(rank, rank64, mid) == rk) a = mid + 1;
      else b = mid;
    }
    hi = a;
    const int F = hi - lo;
    const bool is_last = N < hi;
    if (F <= KN_THREADS) front<MT, 1>(sh, f, m, lo, F, knee_rate, is_last, N, knee, idx);
    else if (F <= 2 * KN_THREADS) front<MT, 2>(sh, f, m, lo, F, knee_rate, is_last, N, knee, idx);
    else if (F <= 4 * KN_THREADS) front<MT, 4>(sh, f, m, lo, F, knee_rate, is_last, N, knee, idx);
    else front<MT, 8>(sh, f, m, lo, F, knee_rate, is_last, N, knee, idx);
    if (is_last) break;
    lo = hi;
    __syncthreads();  // the front's last LDS reads are done before the next one writes
  }
  for (int p = hi + t; p < n; p += KN_THREADS) knee[p] = false;
  if (t == 0) {
    *r_out = sh.r;
    *t_out = sh.t;
  }
}

}  // namespace

void evx_knea_select(const float* f, const void* rank, int rank64, int n, int m, int N, double knee_rate, const double* r_in,
                     const double* t_in, int64_t* idx, bool* knee, double* r_out, double* t_out, hipStream_t s) {
  if (m <= 4)
    knea_select_kernel<4><<<1, KN_THREADS, 0, s>>>(f, rank, rank64, n, m, N, knee_rate, r_in, t_in, idx, knee, r_out, t_out);
  else
    knea_select_kernel<16><<<1, KN_THREADS, 0, s>>>(f, rank, rank64, n, m, N, knee_rate, r_in, t_in, idx, knee, r_out, t_out);
}
