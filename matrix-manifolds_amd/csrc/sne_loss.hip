// Stochastic-neighbour KL objective on a pair vector (mm_sne_kl_loss): with theta a pair vector in the package's order,
//   Z_i = sum_{j != i} exp theta_ij,  A = sum_i log Z_i,  P_ij = exp(theta_ij) / Z_i,
//   L = A(theta_z) - A(theta_x) - sum_{i<j} (P_ij + P_ji)(theta_x) delta_ij,  delta = theta_z - theta_x
//     = sum_i (log Z_i(theta_z) - log Z_i(theta_x) - mu_i),  mu_i = sum_j P_ij(theta_x) delta_ij
// (graphembed/objectives.py:48-76 with inference/stochastic_neighbors.py:8-24 of the reference), inclusive
// (theta_x = -alpha g, theta_z = -m) or exclusive (theta_x = -m, theta_z = -alpha g), and dL/dm per pair.
//
// Three passes, no n x n array, no float atomics (loss and gradient are bitwise reproducible):
//   statistics  the strict upper triangle in tiles of 64 x 64 nodes, one workgroup of four wavefronts per tile, 16 rows per
//               wavefront; a lane owns column j, so the lanes of a wavefront read 64 consecutive pairs of a row.  g and m
//               are read once per unordered pair.  Every node of the row block and of the column block gets one partial
//               record {M_x, S_x, C_x, R_x, M_z, S_z} of the tile: M = max theta over the node's pairs in the tile (the shift
//               is PER NODE: a tile-wide one loses a node whose every distance is far above its neighbours' own),
//               S = sum exp(theta - M), and the weighted mean of delta as C_x + R_x (struct Stat: a centre and the mean of
//               delta - C_x; the plain sum T_x = sum exp(theta_x - M_x) delta loses mu for exactly such a node).  Column
//               side: in the lane's registers down its 16 rows, the four wavefronts folded through LDS in fixed order.
//               Row side: transposing wavefront reductions of the 16 rows' values (maxima first, then the shifted sums).
//               The records leave with plain stores into the slab [6][blocks + 1][n]: column records of tile (bi, bj) in
//               slot bi, row records in slot bj + 1, so a node of block b gets slots 0..b from the tiles above it and
//               b + 1..blocks from the tiles to its right — each slot exactly once, and nothing needs clearing.
//   merge       one lane per node folds its records in slot order (M' = max, S' = S1 e^(M1-M') + S2 e^(M2-M'), the means
//               combined with the same weights over the heavier side's centre, empty records skipped), writes the node
//               table {M_x, log S_x, C_x, R_x, M_z, log S_z} and the node's loss term in fp64 into per-workgroup partial
//               sums; a one-wavefront launch adds those in fixed order.
//   gradient    (only with a gradient buffer) the same tiles: g, m and the two nodes' table rows give dL/dm of each pair
//               once:  inclusive (P_ij + P_ji)(theta_x) - (P_ij + P_ji)(theta_z);
//                      exclusive P_ij(theta_x)(delta_ij - mu_i) + P_ji(theta_x)(delta_ij - mu_j), delta - mu = (delta - C) - R.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mm_manifolds.h"
#include "clear.hpp"
#include "launch.hpp"
#include "smallmat.hpp"

namespace mm {
namespace sne {

constexpr int kB = 64;                  // nodes per block
constexpr int kWaves = 4;               // wavefronts per tile
constexpr int kRows = kB / kWaves;      // rows per wavefront
constexpr int kF = 6;                   // values per record / table row
constexpr int kMergeBlk = 256;
constexpr int64_t kMaxNodes = 32768;    // pair offsets stay below 2^31 elements; the fp64 slab is 0.8 GB there

inline size_t round256(size_t b) { return (b + 255) & ~size_t(255); }
inline size_t slab_bytes(size_t el, int64_t n) { return round256(el * kF * size_t((n + kB - 1) / kB + 1) * size_t(n)); }
inline size_t table_bytes(size_t el, int64_t n) { return round256(el * kF * size_t(n)); }
inline size_t partial_count(int64_t n) { return size_t((n + kMergeBlk - 1) / kMergeBlk); }

template <typename T> __device__ __forceinline__ T neg_inf() { return -T(INFINITY); }

__device__ __forceinline__ float bcast(float x, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src));
}
__device__ __forceinline__ double bcast(double x, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src), __builtin_amdgcn_readlane(__double2loint(x), src));
}

// Transposing reduction of N = 16 values per lane across the wavefront: value r of every lane is combined with `op`, and
// the total of value r comes back in the four lanes 4 r .. 4 r + 3.  Halving steps over lane bits 5..2 (a lane keeps the
// half of the values its bit selects and combines it with its partner's), then a butterfly over bits 1, 0: 17 exchanges
// where 16 butterflies take 96.  The order of the combination is fixed.  `v` is consumed.
// (static_for, not `#pragma unroll`: the indices are constants from the start, so the values are split into registers before
// the two-way selects between them can be turned into one variably indexed access — which came out as compare-select chains
// and 800 spilled scalar registers)
template <int HALF, typename T, typename Op> __device__ __forceinline__ void halve(T (&v)[16], bool hi, int mask, Op op) {
  static_for<HALF>([&](auto K) {
    constexpr int k = decltype(K)::value;
    const T lo = v[k], up = v[k + HALF];
    v[k] = op(hi ? up : lo, __shfl_xor(hi ? lo : up, mask, 64));
  });
}
template <typename T, typename Op> __device__ __forceinline__ T wave_reduce16(T (&v)[16], int lane, Op op) {
  halve<8, T>(v, (lane & 32) != 0, 32, op);
  halve<4, T>(v, (lane & 16) != 0, 16, op);
  halve<2, T>(v, (lane & 8) != 0, 8, op);
  halve<1, T>(v, (lane & 4) != 0, 4, op);
  T r = v[0];
  r = op(r, __shfl_xor(r, 2, 64));
  r = op(r, __shfl_xor(r, 1, 64));
  return r;
}

// One family of node statistics: S = sum exp(theta - M) over the shift M, and (theta_x only) the weighted mean of delta as
// C + R — C a value of the working precision near the mean, R = sum exp(theta - M) (delta - C) / S.  mu itself is not
// representable where it counts: a node whose every distance is ~500 has mu ~ 500 and gradient terms P (delta - mu) of
// order 1, so a mean rounded to the working precision (half an ulp of 500) is already the whole error budget.
template <typename T> struct Stat {
  T M, S, C, R;
};
template <typename T> __device__ __forceinline__ Stat<T> empty_stat() { return {neg_inf<T>(), T(0), T(0), T(0)}; }

// a (+)= b, b.S > 0: the sums re-expressed over the larger shift, the mean over the centre of the heavier side
template <typename T, bool MEAN> __device__ __forceinline__ void fold(Stat<T>& a, const Stat<T>& b) {
  const bool up = b.M > a.M;
  const T e = Num<T>::exp(up ? a.M - b.M : b.M - a.M);   // (a empty: M = -inf, S = 0, e = 0)
  const T wa = up ? a.S * e : a.S, wb = up ? b.S : b.S * e;
  const T S = wa + wb;
  if constexpr (MEAN) {
    const bool take = wb > wa;
    const T ra = take ? a.R + (a.C - b.C) : a.R, rb = take ? b.R : b.R + (b.C - a.C);
    a.R = (wa * ra + wb * rb) / S;
    a.C = take ? b.C : a.C;
  }
  a.S = S;
  a.M = up ? b.M : a.M;
}

// theta_x, theta_z of one pair from its target and squared distance
template <typename T, int MODE> __device__ __forceinline__ void thetas(T gv, T mv, T alpha, T& tx, T& tz) {
  const T a = -alpha * gv, b = -mv;
  tx = MODE == MM_SNE_INCLUSIVE ? a : b;
  tz = MODE == MM_SNE_INCLUSIVE ? b : a;
}

template <typename T, int MODE>
__global__ __launch_bounds__(kB * kWaves) void sne_stats_kernel(const T* __restrict__ g, const T* __restrict__ m, int n, int nb,
                                                                T alpha, T* __restrict__ slab /* [kF][nb + 1][n] */) {
  const int bj = blockIdx.x, bi = blockIdx.y;
  if (bi > bj) return;
  __shared__ T colp[kWaves][kF][kB];
  __shared__ T rowp[kF][kB];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = bj * kB + lane;
  const int jv = j < n ? j : -1;      // (pair (i, j) is in the triangle iff jv > i)
  const int i0 = bi * kB + wave * kRows;
  const T ninf = neg_inf<T>();

  // The wavefront's 16 rows of this column.  Every lane loads from a pair of the row that exists — (ic, jc) with
  // ic = min(i, n - 2), jc = min(max(j, ic + 1), n - 1); that IS its pair when it has one — at a 32-bit offset from the first
  // row's slice; a pair outside the triangle then becomes theta = -inf, delta = 0.
  const int ic0 = min(i0, n - 2);
  const int64_t base0 = pair_off(n, ic0) - ic0 - 1;
  const T* __restrict__ g0 = g + base0;
  const T* __restrict__ m0 = m + base0;
  T tx[kRows], tz[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int ic = min(i0 + r, n - 2);
    const int off = int(pair_off(n, ic) - ic - 1 - base0) + min(max(j, ic + 1), n - 1);
    thetas<T, MODE>(g0[off], m0[off], alpha, tx[r], tz[r]);
  }
  T dl[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const bool ok = jv > i0 + r;
    dl[r] = ok ? tz[r] - tx[r] : T(0);
    tx[r] = ok ? tx[r] : ninf;
    tz[r] = ok ? tz[r] : ninf;
  }

  // column side: node j over the 16 rows, in registers
  {
    T Mx = ninf, Mz = ninf;
#pragma unroll
    for (int r = 0; r < kRows; ++r) { Mx = Num<T>::max(Mx, tx[r]); Mz = Num<T>::max(Mz, tz[r]); }
    const T sx = Mx == ninf ? T(0) : Mx, sz = Mz == ninf ? T(0) : Mz;   // (no pair: every term exp(-inf - 0) = 0)
    T Sx = T(0), T0 = T(0), Sz = T(0);
    T ex[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      ex[r] = Num<T>::exp(tx[r] - sx);
      Sx += ex[r];
      T0 += ex[r] * dl[r];
      Sz += Num<T>::exp(tz[r] - sz);
    }
    const T C = Sx > T(0) ? T0 / Sx : T(0);
    T Tc = T(0);
#pragma unroll
    for (int r = 0; r < kRows; ++r) Tc += ex[r] * (dl[r] - C);   // (no pair: ex = 0)
    colp[wave][0][lane] = Mx; colp[wave][1][lane] = Sx; colp[wave][2][lane] = C;
    colp[wave][3][lane] = Sx > T(0) ? Tc / Sx : T(0);
    colp[wave][4][lane] = Mz; colp[wave][5][lane] = Sz;
  }

  // row side: node i0 + r over the 64 columns; its totals arrive in lanes 4 r .. 4 r + 3
  {
    T v[kRows];
    auto vmax = [](T a, T b) { return Num<T>::max(a, b); };
    auto vadd = [](T a, T b) { return a + b; };
#pragma unroll
    for (int r = 0; r < kRows; ++r) v[r] = tx[r];
    const T Mx = wave_reduce16<T>(v, lane, vmax);
    T ex[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const T s = bcast(Mx, 4 * r);
      ex[r] = Num<T>::exp(tx[r] - (s == ninf ? T(0) : s));
      v[r] = ex[r];
    }
    const T Sx = wave_reduce16<T>(v, lane, vadd);
#pragma unroll
    for (int r = 0; r < kRows; ++r) v[r] = ex[r] * dl[r];
    const T T0 = wave_reduce16<T>(v, lane, vadd);
    const T C = Sx > T(0) ? T0 / Sx : T(0);
#pragma unroll
    for (int r = 0; r < kRows; ++r) v[r] = ex[r] * (dl[r] - bcast(C, 4 * r));
    const T Tc = wave_reduce16<T>(v, lane, vadd);
#pragma unroll
    for (int r = 0; r < kRows; ++r) v[r] = tz[r];
    const T Mz = wave_reduce16<T>(v, lane, vmax);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const T s = bcast(Mz, 4 * r);
      v[r] = Num<T>::exp(tz[r] - (s == ninf ? T(0) : s));
    }
    const T Sz = wave_reduce16<T>(v, lane, vadd);
    if ((lane & 3) == 0) {
      const int k = wave * kRows + (lane >> 2);
      rowp[0][k] = Mx; rowp[1][k] = Sx; rowp[2][k] = C; rowp[3][k] = Sx > T(0) ? Tc / Sx : T(0);
      rowp[4][k] = Mz; rowp[5][k] = Sz;
    }
  }
  __syncthreads();

  const size_t slot_stride = size_t(n), field_stride = size_t(nb + 1) * size_t(n);
  if (threadIdx.x < kB) {   // column records: the four wavefronts folded in order, slot bi
    if (j < n) {
      Stat<T> x = empty_stat<T>(), z = empty_stat<T>();
#pragma unroll
      for (int w = 0; w < kWaves; ++w)
        if (colp[w][1][lane] > T(0)) {
          fold<T, true>(x, Stat<T>{colp[w][0][lane], colp[w][1][lane], colp[w][2][lane], colp[w][3][lane]});
          fold<T, false>(z, Stat<T>{colp[w][4][lane], colp[w][5][lane], T(0), T(0)});
        }
      T* p = slab + size_t(bi) * slot_stride + j;
      p[0] = x.M; p[field_stride] = x.S; p[2 * field_stride] = x.C; p[3 * field_stride] = x.R;
      p[4 * field_stride] = z.M; p[5 * field_stride] = z.S;
    }
  } else if (threadIdx.x < 2 * kB) {   // row records, slot bj + 1
    const int i = bi * kB + lane;
    if (i < n) {
      T* p = slab + size_t(bj + 1) * slot_stride + i;
#pragma unroll
      for (int f = 0; f < kF; ++f) p[f * field_stride] = rowp[f][lane];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kMergeBlk) void sne_merge_kernel(const T* __restrict__ slab, int n, int nb,
                                                              T* __restrict__ table /* [kF][n] */,
                                                              double* __restrict__ partials /* [gridDim.x] */) {
  __shared__ double wsum[kMergeBlk / 64];
  const int v = blockIdx.x * kMergeBlk + threadIdx.x;
  double term = 0.0;
  if (v < n) {
    const size_t field_stride = size_t(nb + 1) * size_t(n);
    Stat<T> x = empty_stat<T>(), z = empty_stat<T>();
#pragma unroll 2
    for (int s = 0; s <= nb; ++s) {
      const T* p = slab + size_t(s) * n + v;
      const Stat<T> rx{p[0], p[field_stride], p[2 * field_stride], p[3 * field_stride]};
      const Stat<T> rz{p[4 * field_stride], p[5 * field_stride], T(0), T(0)};
      if (rx.S > T(0)) {   // (an empty record is S = 0, M = -inf: never exponentiated)
        fold<T, true>(x, rx);
        fold<T, false>(z, rz);
      }
    }
    // (n >= 2: every node has a pair, S >= 1)
    const double lsx = ::log(double(x.S)), lsz = ::log(double(z.S));
    const size_t ns = size_t(n);
    table[v] = x.M;
    table[ns + v] = T(lsx);
    table[2 * ns + v] = x.C;
    table[3 * ns + v] = x.R;
    table[4 * ns + v] = z.M;
    table[5 * ns + v] = T(lsz);
    term = (double(z.M) - double(x.M)) + (lsz - lsx) - (double(x.C) + double(x.R));
  }
  term = wave_sum(term);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wsum[0];
#pragma unroll
    for (int w = 1; w < kMergeBlk / 64; ++w) s += wsum[w];
    partials[blockIdx.x] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(64) void sne_finish_kernel(const double* __restrict__ partials, int count, T* __restrict__ loss_out) {
  double s = 0.0;
  for (int t = threadIdx.x; t < count; t += 64) s += partials[t];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss_out[0] = T(s);
}

template <typename T, int MODE>
__global__ __launch_bounds__(kB * kWaves) void sne_grad_kernel(const T* __restrict__ g, const T* __restrict__ m, int n, T alpha,
                                                               const T* __restrict__ table /* [kF][n] */,
                                                               T* __restrict__ grad) {
  const int bj = blockIdx.x, bi = blockIdx.y;
  if (bi > bj) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = bj * kB + lane;
  const int i0 = bi * kB + wave * kRows;
  if (j >= n) return;
  const size_t ns = size_t(n);
  const T cMx = table[j], cLx = table[ns + j], cC = table[2 * ns + j], cR = table[3 * ns + j], cMz = table[4 * ns + j],
          cLz = table[5 * ns + j];
  const int i1 = min(i0 + kRows, n);
  for (int i = i0; i < i1; ++i) {
    if (j <= i) continue;
    const int64_t idx = pair_off(n, i) + (j - i - 1);
    T tx, tz;
    thetas<T, MODE>(g[idx], m[idx], alpha, tx, tz);
    const T pxr = Num<T>::exp((tx - table[i]) - table[ns + i]), pxc = Num<T>::exp((tx - cMx) - cLx);
    T d;
    if constexpr (MODE == MM_SNE_INCLUSIVE) {
      const T pzr = Num<T>::exp((tz - table[4 * ns + i]) - table[5 * ns + i]), pzc = Num<T>::exp((tz - cMz) - cLz);
      d = (pxr + pxc) - (pzr + pzc);
    } else {
      const T dl = tz - tx;   // (delta - mu as (delta - C) - R: see Stat)
      d = pxr * ((dl - table[2 * ns + i]) - table[3 * ns + i]) + pxc * ((dl - cC) - cR);
    }
    grad[idx] = d;
  }
}

template <typename T, int MODE>
int launch(const T* g, const T* m, int64_t n, T alpha, T* grad, T* loss_out, void* ws, hipStream_t st) {
  const int nb = int((n + kB - 1) / kB);
  T* slab = static_cast<T*>(ws);
  T* table = reinterpret_cast<T*>(static_cast<char*>(ws) + slab_bytes(sizeof(T), n));
  double* partials = reinterpret_cast<double*>(static_cast<char*>(ws) + slab_bytes(sizeof(T), n) + table_bytes(sizeof(T), n));
  const int np = int(partial_count(n));
  const dim3 tiles(nb, nb), wg(kB * kWaves);
  sne_stats_kernel<T, MODE><<<tiles, wg, 0, st>>>(g, m, int(n), nb, alpha, slab);
  sne_merge_kernel<T><<<dim3(np), dim3(kMergeBlk), 0, st>>>(slab, int(n), nb, table, partials);
  sne_finish_kernel<T><<<dim3(1), dim3(64), 0, st>>>(partials, np, loss_out);
  if (grad) sne_grad_kernel<T, MODE><<<tiles, wg, 0, st>>>(g, m, int(n), alpha, table, grad);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MM_OK : int(e);
}

}  // namespace sne
}  // namespace mm

using namespace mm::sne;

extern "C" {

size_t mm_sne_kl_ws_bytes(int dtype, int64_t n) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || n > kMaxNodes) return 0;
  const size_t el = dtype == MM_F64 ? 8 : 4;
  return slab_bytes(el, n) + table_bytes(el, n) + round256(partial_count(n) * sizeof(double));
}

int mm_sne_kl_loss(int dtype, int mode, const void* target, const void* m, int64_t n, double alpha, void* grad_out,
                   void* loss_out, void* ws, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || (mode != MM_SNE_INCLUSIVE && mode != MM_SNE_EXCLUSIVE) || n < 0 || !loss_out)
    return MM_ERR_ARG;
  if (n >= 2 && (!target || !m || !ws)) return MM_ERR_ARG;
  if (n > kMaxNodes) return MM_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n < 2) {   // no pair: the loss is 0 and the gradient has no entry
    const hipError_t e = mm::clear_async(loss_out, dtype == MM_F64 ? 8 : 4, st);
    return e == hipSuccess ? MM_OK : int(e);
  }
  if (dtype == MM_F32) {
    using T = float;
    return mode == MM_SNE_INCLUSIVE
        ? launch<T, MM_SNE_INCLUSIVE>(static_cast<const T*>(target), static_cast<const T*>(m), n, T(alpha), static_cast<T*>(grad_out), static_cast<T*>(loss_out), ws, st)
        : launch<T, MM_SNE_EXCLUSIVE>(static_cast<const T*>(target), static_cast<const T*>(m), n, T(alpha), static_cast<T*>(grad_out), static_cast<T*>(loss_out), ws, st);
  }
  using T = double;
  return mode == MM_SNE_INCLUSIVE
      ? launch<T, MM_SNE_INCLUSIVE>(static_cast<const T*>(target), static_cast<const T*>(m), n, T(alpha), static_cast<T*>(grad_out), static_cast<T*>(loss_out), ws, st)
      : launch<T, MM_SNE_EXCLUSIVE>(static_cast<const T*>(target), static_cast<const T*>(m), n, T(alpha), static_cast<T*>(grad_out), static_cast<T*>(loss_out), ws, st);
}

}  // extern "C"
