// kappa-stereographic model of constant curvature (mm_stereo_*): the Poincare ball (c > 0) and the stereographically
// projected sphere (c < 0) in one formula, with the curvature read from DEVICE memory (manifolds/universal.py and
// manifolds/impl/math.py of the reference; c = get_c(c_raw), K = -c).
//
// For a pair: a = |x_i|^2, b = |x_j|^2, p = <x_i, x_j>, q = |x_i - x_j|^2 (formed from the differences, not as a + b - 2p),
//   D = 1 - 2 c p + c^2 a b = (1 - c a)(1 - c b) + c q,   t = |(-x_i) (+)_c x_j|^2 = q / D,   w = c t,
//   d = 2 sqrt(t) phi(w),  phi(w) = artanh(sqrt w) / sqrt w  (w > 0),  atan(sqrt -w) / sqrt -w  (w < 0),  phi(0) = 1:
// one analytic function 1 + w/3 + w^2/5 + ..., evaluated as that series for |w| <= 1/8 (fp32) or 1/16 (fp64) (no cancellation at the reference's
// initialisation, where the log form loses four digits in fp32) and through log1p / atan beyond.  c = 0 gives the Euclidean
// limit d^2 = 4 q where the reference returns NaN.
// Gradients: d(d^2)/dt = 4 phi / (1 - w), d(d)/dt = 1 / (sqrt t (1 - w)); with G = g dF/dt, A = 2 G / D, At = A t:
//   grad x_i += (A - c At)(x_i - x_j) + c At (1 - c b) x_i,   grad x_j += (A - c At)(x_j - x_i) + c At (1 - c a) x_j
// (the DIFFERENCE form: the plain one, (c At - A) x_j + (A - c^2 At b) x_i, cancels between the sum over x_j and the own-point
// term when two points are close and the distance is not squared - A grows like 1 / |x_i - x_j| there),
//   dF/dc = At (p - c a b) + g dF/dc|_t,  dF/dc|_t = 8 t^2 phi phi'  (squared),  2 t sqrt t phi'  (not squared),
// and the kernels return dF/dc_raw = dF/dc * dc/dc_raw.
//
// Pair kernels: tiles of TR rows x 64 columns (TR = 64 in fp32, 32 in fp64: the tile of pair scalars lives in LDS), four
// wavefronts.  Rows are wave-uniform (LDS broadcasts), a lane owns a column.  The backward visits every unordered pair once:
// phase 1 computes {A, At} per pair and leaves the two scalars in LDS; phase 2 forms the column sums in the lane's registers
// down the tile's rows, then turns the tile (a lane owns a ROW, columns are uniform) and forms the row sums - m + 1 fused
// multiply-adds per pair and side, no cross-lane traffic, and the transcendental code never meets the accumulators' registers.  The four wavefronts' sums are folded through LDS in
// fixed order and leave with plain stores into a slab of per-tile records (column records of row block bi in slot bi, row
// records of column block bj in slot nbr + bj): no float atomics, nothing to clear, bitwise reproducible.  A finalize launch
// adds a node's records in slot order; the curvature gradient goes through per-workgroup fp64 partials added in fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/mm_manifolds.h"
#include "adam.hpp"
#include "clear.hpp"
#include "launch.hpp"
#include "loss.hpp"

namespace mm {
namespace stereo {

constexpr int kC = 64;                   // columns per tile
constexpr int kWaves = 4;
constexpr int kMaxDim = 16;
constexpr int64_t kMaxNodes = 32768;     // pair offsets stay below 2^31 elements
constexpr int kPtBlk = 128;              // per-point kernels: points per workgroup
constexpr double kMinNorm = 1e-15;       // MIN_NORM (impl/math.py:15)
constexpr double kEps = 1e-8;            // EPS (utils.py:13), both precisions

template <typename T> struct Tile { static constexpr int rows = sizeof(T) == 4 ? 64 : 32; };

inline size_t round256(size_t b) { return (b + 255) & ~size_t(255); }

template <typename T> struct M;
template <> struct M<float> {
  static __device__ __forceinline__ float sqrt(float x) { return ::sqrtf(x); }
  static __device__ __forceinline__ float log1p(float x) { return ::log1pf(x); }
  static __device__ __forceinline__ float atan(float x) { return ::atanf(x); }
  static __device__ __forceinline__ float tanh(float x) { return ::tanhf(x); }
  static __device__ __forceinline__ float tan(float x) { return ::tanf(x); }
  static constexpr int terms = 8;                         // series of phi through w^8 for |w| <= 1/8: (1/8)^9 / 19 = 4e-10
  static constexpr float series = 0.125f;
  static constexpr float wmax = 1.0f - 9.5367431640625e-7f;  // 1 - 2^-20
  static constexpr float ball_eps = 4e-3f;                // BALL_EPS (impl/math.py:16)
};
template <> struct M<double> {
  static __device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
  static __device__ __forceinline__ double log1p(double x) { return ::log1p(x); }
  static __device__ __forceinline__ double atan(double x) { return ::atan(x); }
  static __device__ __forceinline__ double tanh(double x) { return ::tanh(x); }
  static __device__ __forceinline__ double tan(double x) { return ::tan(x); }
  static constexpr int terms = 12;                        // through w^12 for |w| <= 1/16: (1/16)^13 / 27 = 8e-18
  static constexpr double series = 0.0625;
  static constexpr double wmax = 1.0 - 1e-15;             // the reference's artanh clamp (impl/math.py:29)
  static constexpr double ball_eps = 1e-5;
};

// get_c (universal.py:27-31) and its derivative, in fp64 whatever the points' precision
template <typename T> struct Curv {
  T c, dc;
};
template <typename T> __device__ __forceinline__ Curv<T> load_curv(const T* __restrict__ c_raw, int mode, double c_min) {
  const double r = double(c_raw[0]);
  double c, dc;
  if (mode == MM_STEREO_C_FREE) {
    c = r + (r > 0 ? c_min : r < 0 ? -c_min : 0.0);      // sign(c_raw) c_min + c_raw; sign has no derivative
    dc = 1.0;
  } else {
    const double s = mode == MM_STEREO_C_POSITIVE ? 1.0 : -1.0;
    const bool lin = r > 20.0;                            // softplus' threshold
    const double e = ::exp(lin ? 0.0 : r);
    c = s * (c_min + (lin ? r : ::log1p(e)));
    dc = s * (lin ? 1.0 : e / (1.0 + e));
  }
  return {T(c), T(dc)};
}

// phi(w) = 1 + w phi1(w) and, when PSI, phi'(w) = (1 / (1 - w) - phi1(w)) / 2 with phi1 = (phi - 1) / w = 1/3 + w/5 + w^2/7 + ...
// (phi' = 1/3 + 2 w / 5 + 3 w^2 / 7 + ...: the form above has no cancellation at w = 0 and shares phi's coefficients)
template <typename T, bool PSI> __device__ __forceinline__ void phi_of(T w, T& phi, T& psi) {
  constexpr int K = M<T>::terms;
  T phi1;
  if (fabs(w) <= M<T>::series) {
    T f = T(1) / T(2 * K + 1);
#pragma unroll
    for (int k = K - 1; k >= 1; --k) f = f * w + T(1) / T(2 * k + 1);
    phi1 = f;
    phi = 1 + w * f;
  } else {
    const T u = M<T>::sqrt(fabs(w));
    phi = (w > 0 ? T(0.5) * M<T>::log1p(2 * u / (1 - u)) : M<T>::atan(u)) / u;
    phi1 = (phi - 1) / w;
  }
  psi = PSI ? T(0.5) * (1 / (1 - w) - phi1) : T(0);
}

// value of one pair from q, D
template <typename T> __device__ __forceinline__ T pair_value(T q, T D, T c, bool squared) {
  const T t = q / fmax(D, T(kMinNorm));                   // _mobius_add's denominator clamp (impl/math.py:345)
  const T w = fmin(c * t, M<T>::wmax);
  T phi, psi;
  phi_of<T, false>(w, phi, psi);
  const T v = squared ? 4 * t * phi * phi : 2 * M<T>::sqrt(t) * phi;
  return fmax(v, T(kEps));                                // universal.py:83 (the clamp is transparent to the gradient)
}

// {A, At, dF/dc} of one pair with upstream g
template <typename T> __device__ __forceinline__ void pair_grad(T q, T p, T a, T b, T D, T c, T g, bool squared, T& A, T& At, T& dcp) {
  const T Dc = fmax(D, T(kMinNorm));
  const T t = q / Dc;
  const T w = fmin(c * t, M<T>::wmax);
  T phi, psi;
  phi_of<T, true>(w, phi, psi);
  T dFdt, dFdc;
  if (squared) {
    dFdt = 4 * phi / (1 - w);
    dFdc = 8 * t * t * phi * psi;
  } else {
    const T rt = M<T>::sqrt(fmax(t, T(1e-30)));
    dFdt = 1 / (rt * (1 - w));
    dFdc = 2 * t * rt * psi;
  }
  A = 2 * g * dFdt / Dc;
  At = A * t;
  dcp = At * (p - c * a * b) + g * dFdc;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
template <typename T, int MP>
__global__ __launch_bounds__(kC* kWaves) void pdist_fwd_kernel(const T* __restrict__ x, const T* __restrict__ c_raw, int c_mode,
                                                               double c_min, int n, int m, int rb, int re, int squared,
                                                               T* __restrict__ out) {
  constexpr int RW = kC / kWaves;   // rows per wavefront
  const int bj = blockIdx.x, bi = rb / kC + blockIdx.y;
  if (bj < bi) return;
  __shared__ T sx[kC][MP + 1];
  __shared__ T ss[kC];
  const Curv<T> cv = load_curv(c_raw, c_mode, c_min);
  const T c = cv.c;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < kC) {           // the row block's points and their 1 - c a (once per tile, not per pair)
    const int i = min(bi * kC + int(threadIdx.x), n - 1);
    T a = 0;
#pragma unroll
    for (int k = 0; k < MP; ++k) {
      const T v = k < m ? x[size_t(i) * m + k] : T(0);
      sx[threadIdx.x][k] = v;
      a += v * v;
    }
    ss[threadIdx.x] = 1 - c * a;
  }
  const int j = bj * kC + lane, jc = min(j, n - 1);
  T xj[MP], b = 0;
#pragma unroll
  for (int k = 0; k < MP; ++k) {
    xj[k] = k < m ? x[size_t(jc) * m + k] : T(0);
    b += xj[k] * xj[k];
  }
  const T sj = 1 - c * b;
  __syncthreads();
  const int64_t base = pair_off(n, rb);
  // interior tiles (wholly above the diagonal and inside the table) store without a lane mask; diagonal and edge tiles mask
  auto rows = [&](auto masked) {
#pragma unroll 4
    for (int r = 0; r < RW; ++r) {
      const int il = wave * RW + r, i = bi * kC + il;
      if (i < rb || i >= re) continue;   // (wave-uniform)
      T q = 0;
#pragma unroll
      for (int k = 0; k < MP; ++k) {
        const T d = sx[il][k] - xj[k];
        q += d * d;
      }
      const T v = pair_value<T>(q, ss[il] * sj + c * q, c, squared != 0);
      if (!decltype(masked)::value || (j > i && j < n)) out[pair_off(n, i) - base + (j - i - 1)] = v;
    }
  };
  if (bj > bi && bj * kC + kC <= n)
    rows(std::false_type{});
  else
    rows(std::true_type{});
}

// ---- backward -----------------------------------------------------------------------------------------------------------
template <typename T, int MP>
__global__ __launch_bounds__(kC* kWaves) void pdist_bwd_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                               const T* __restrict__ c_raw, int c_mode, double c_min, int n, int m,
                                                               int rb, int re, int squared, int bi0, int nbr,
                                                               T* __restrict__ slab, double* __restrict__ partials) {
  constexpr int TR = Tile<T>::rows, RW = TR / kWaves, CW = kC / kWaves, LD = kC + 1, UNR = sizeof(T) == 4 ? 2 : 1, KUN = sizeof(T) == 4 ? MP : 4;
  const int bj = blockIdx.x, bi = bi0 + blockIdx.y;
  const int slot_p = blockIdx.y * gridDim.x + blockIdx.x;
  if (bj < (bi * TR + 1) / kC) {     // no pair i < j in this tile
    if (threadIdx.x == 0) partials[slot_p] = 0.0;
    return;
  }
  __shared__ T sxr[TR][MP + 1], sxc[kC][MP + 1];
  __shared__ T sar[TR], sbc[kC];
  __shared__ T sA[TR * LD], sAt[TR * LD];
  __shared__ T redc[MP + 1][kC], redr[MP + 1][TR];
  __shared__ double scv[kWaves];
  const Curv<T> cv = load_curv(c_raw, c_mode, c_min);
  const T c = cv.c;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < TR) {
    const int i = min(bi * TR + tid, n - 1);
    T a = 0;
#pragma unroll
    for (int k = 0; k < MP; ++k) {
      const T v = k < m ? x[size_t(i) * m + k] : T(0);
      sxr[tid][k] = v;
      a += v * v;
    }
    sar[tid] = a;
  }
  const int j = bj * kC + lane;
  if (wave == 1) {
    const int jc = min(j, n - 1);
    T b = 0;
#pragma unroll
    for (int k = 0; k < MP; ++k) {
      const T v = k < m ? x[size_t(jc) * m + k] : T(0);
      sxc[lane][k] = v;
      b += v * v;
    }
    sbc[lane] = b;
  }
  __syncthreads();

  // phase 1: a lane owns column j, the wavefront's rows are uniform; the pair's two scalars go to LDS
  T cacc = 0;
  {
    const T b = sbc[lane], sj = 1 - c * b;
    const int64_t base = pair_off(n, rb);
#pragma unroll UNR
    for (int r = 0; r < RW; ++r) {
      const int il = wave * RW + r, i = bi * TR + il;
      T q = 0, p = 0;
#pragma unroll KUN
      for (int k = 0; k < MP; ++k) {   // (fp64: four at a time - fully unrolled, the 2 MP loads are all issued ahead and held)
        const T xi = sxr[il][k], xj = sxc[lane][k], d = xi - xj;
        q += d * d;
        p += xi * xj;
      }
      const T a = sar[il];
      const bool live = j > i && j < n && i >= rb && i < re;
      T A = 0, At = 0, dcp = 0;
      if (live) {
        const T gv = g[pair_off(n, i) - base + (j - i - 1)];
        pair_grad<T>(q, p, a, b, (1 - c * a) * sj + c * q, c, gv, squared != 0, A, At, dcp);
      }
      sA[il * LD + lane] = A;
      sAt[il * LD + lane] = At;
      cacc += dcp;
    }
  }
  __syncthreads();

  // phase 2, columns: the same lanes and rows, sums in the lane's registers down the wavefront's rows
  T cw[MP], xo[MP], cvs = 0;
#pragma unroll
  for (int k = 0; k < MP; ++k) {
    cw[k] = 0;
    xo[k] = sxc[lane][k];
  }
#pragma unroll UNR
  for (int r = 0; r < RW; ++r) {
    const int il = wave * RW + r;
    const T A = sA[il * LD + lane], At = sAt[il * LD + lane];
    const T W = A - c * At;
    cvs += c * At * (1 - c * sar[il]);
#pragma unroll
    for (int k = 0; k < MP; ++k) cw[k] += W * (xo[k] - sxr[il][k]);
  }
  // the four wavefronts' column sums, folded in wavefront order
  for (int wv = 0; wv < kWaves; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int k = 0; k < MP; ++k) redc[k][lane] = wv == 0 ? cw[k] : redc[k][lane] + cw[k];
      redc[MP][lane] = wv == 0 ? cvs : redc[MP][lane] + cvs;
    }
    __syncthreads();
  }

  // phase 2, rows: the tile turned - a lane owns row il, the wavefront's columns are uniform
  T rw[MP], rvs = 0;
#pragma unroll
  for (int k = 0; k < MP; ++k) rw[k] = 0;
  if (lane < TR) {
#pragma unroll
    for (int k = 0; k < MP; ++k) xo[k] = sxr[lane][k];
#pragma unroll UNR
    for (int jj = 0; jj < CW; ++jj) {
      const int jl = wave * CW + jj;
      const T A = sA[lane * LD + jl], At = sAt[lane * LD + jl];
      const T W = A - c * At;
      rvs += c * At * (1 - c * sbc[jl]);
#pragma unroll
      for (int k = 0; k < MP; ++k) rw[k] += W * (xo[k] - sxc[jl][k]);
    }
  }
  for (int wv = 0; wv < kWaves; ++wv) {
    if (wave == wv && lane < TR) {
#pragma unroll
      for (int k = 0; k < MP; ++k) redr[k][lane] = wv == 0 ? rw[k] : redr[k][lane] + rw[k];
      redr[MP][lane] = wv == 0 ? rvs : redr[MP][lane] + rvs;
    }
    __syncthreads();
  }
  const size_t ns = size_t(n), comps = size_t(m) + 1;
  if (wave == 0 && j < n) {           // column records of row block bi
    T* rec = slab + size_t(bi) * comps * ns + j;
    for (int k = 0; k < m; ++k) rec[k * ns] = redc[k][lane];
    rec[size_t(m) * ns] = redc[MP][lane];
  }
  if (wave == 1 && lane < TR && bi * TR + lane < n) {   // row records of column block bj
    T* rec = slab + size_t(nbr + bj) * comps * ns + (bi * TR + lane);
    for (int k = 0; k < m; ++k) rec[k * ns] = redr[k][lane];
    rec[size_t(m) * ns] = redr[MP][lane];
  }
  double cd = double(cacc);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) cd += __shfl_xor(cd, s, 64);
  if (lane == 0) scv[wave] = cd;
  __syncthreads();
  if (tid == 0) partials[slot_p] = ((scv[0] + scv[1]) + scv[2]) + scv[3];
}

// grad_x[v] = sum of v's records: the sums of W (x_v - x_other) + the sum of c At (1 - c |x_other|^2) * x[v]
template <typename T>
__global__ __launch_bounds__(256) void pdist_bwd_finalize_kernel(const T* __restrict__ x, const T* __restrict__ slab, int n, int m,
                                                                 int rb, int re, int nbr, int nbc, T* __restrict__ grad) {
  constexpr int TR = Tile<T>::rows;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const size_t ns = size_t(n), comps = size_t(m) + 1;
  T acc[kMaxDim + 1];
#pragma unroll
  for (int k = 0; k <= kMaxDim; ++k) acc[k] = 0;
  if (re > rb) {
    const int bi0 = rb / TR, bi1 = (re - 1) / TR;
    // as a column: the row blocks of the range that hold a row above v
    const int last = v >= 1 ? min(bi1, (v - 1) / TR) : -1;
    for (int s = bi0; s <= last; ++s) {
      const T* rec = slab + size_t(s) * comps * ns + v;
#pragma unroll
      for (int k = 0; k <= kMaxDim; ++k)
        if (k <= m) acc[k] += rec[k * ns];
    }
    // as a row: every column block from the one that holds v + 1
    if (v >= rb && v < re) {
      const int bv = v / TR;
      for (int s = (bv * TR + 1) / kC; s < nbc; ++s) {
        const T* rec = slab + size_t(nbr + s) * comps * ns + v;
#pragma unroll
        for (int k = 0; k <= kMaxDim; ++k)
          if (k <= m) acc[k] += rec[k * ns];
      }
    }
  }
  T vs = 0;
#pragma unroll
  for (int k = 0; k <= kMaxDim; ++k)
    if (k == m) vs = acc[k];
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k)
    if (k < m) grad[size_t(v) * m + k] = acc[k] + vs * x[size_t(v) * m + k];
}

// grad_c[0] = dc/dc_raw * sum of the fp64 partials, in fixed order
template <typename T>
__global__ __launch_bounds__(256) void curv_finalize_kernel(const double* __restrict__ partials, int64_t count, const T* __restrict__ c_raw,
                                                            int c_mode, double c_min, T* __restrict__ grad_c) {
  __shared__ double sh[256];
  double s = 0;
  for (int64_t k = threadIdx.x; k < count; k += 256) s += partials[k];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) grad_c[0] = T(sh[0] * double(load_curv(c_raw, c_mode, c_min).dc));
}

// ---- per point ------------------------------------------------------------------------------------------------------------
template <typename T> struct Vec {
  T v[kMaxDim];
};
template <typename T> __device__ __forceinline__ Vec<T> load_vec(const T* __restrict__ p, int64_t row, int m) {
  Vec<T> r;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) r.v[k] = k < m ? p[row * m + k] : T(0);
  return r;
}
template <typename T> __device__ __forceinline__ void store_vec(T* __restrict__ p, int64_t row, int m, const Vec<T>& r) {
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k)
    if (k < m) p[row * m + k] = r.v[k];
}
template <typename T> __device__ __forceinline__ T dot(const Vec<T>& a, const Vec<T>& b) {
  T s = 0;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) s += a.v[k] * b.v[k];
  return s;
}
template <typename T> __device__ __forceinline__ Vec<T> axpby(T a, const Vec<T>& x, T b, const Vec<T>& y) {
  Vec<T> r;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) r.v[k] = a * x.v[k] + b * y.v[k];
  return r;
}
// 1 - c |x|^2 clamped as in _lambda_x (impl/math.py:187-190); lambda = 2 / it
template <typename T> __device__ __forceinline__ T conf_den(const Vec<T>& x, T c) { return fmax(1 - c * dot(x, x), T(kMinNorm)); }
// _mobius_add (impl/math.py:326-345)
template <typename T> __device__ __forceinline__ Vec<T> mobius_add(const Vec<T>& x, const Vec<T>& y, T c) {
  const T x2 = dot(x, x), y2 = dot(y, y), xy = dot(x, y);
  const T den = fmax(1 + 2 * c * xy + c * c * x2 * y2, T(kMinNorm));
  return axpby((1 + 2 * c * xy + c * y2) / den, x, (1 - c * x2) / den, y);
}
// _project (impl/math.py:142-156): acts for c > 0 only
template <typename T> __device__ __forceinline__ Vec<T> project(const Vec<T>& x, T c) {
  if (!(c > 0)) return x;
  const T nrm = fmax(M<T>::sqrt(dot(x, x)), T(kMinNorm));
  const T maxnorm = (1 - M<T>::ball_eps) / M<T>::sqrt(c);
  if (!(nrm > maxnorm)) return x;
  Vec<T> r;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) r.v[k] = x.v[k] / nrm * maxnorm;
  return r;
}
// tan_c(sqrt|c| z) / sqrt|c| (tan_func, impl/math.py:73-85; tanh's argument clamped at 15, :21-22); z for c = 0
template <typename T> __device__ __forceinline__ T tan_k(T z, T c) {
  const T s = M<T>::sqrt(fabs(c));
  if (s == 0) return z;
  const T arg = s * z;
  return (c > 0 ? M<T>::tanh(fmin(fmax(arg, T(-15)), T(15))) : M<T>::tan(arg)) / s;
}
// _expmap (impl/math.py:720-727)
template <typename T> __device__ __forceinline__ Vec<T> expmap(const Vec<T>& x, const Vec<T>& u, T c) {
  const T un = fmax(M<T>::sqrt(dot(u, u)), T(kMinNorm));
  const T scale = tan_k<T>(un / conf_den(x, c), c) / un;   // sqrt|c| / 2 * lambda * |u| = sqrt|c| |u| / (1 - c |x|^2)
  Vec<T> second;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) second.v[k] = scale * u.v[k];
  return mobius_add(x, second, c);
}
template <typename T> __device__ __forceinline__ Vec<T> neg(const Vec<T>& x) {
  Vec<T> r;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) r.v[k] = -x.v[k];
  return r;
}

template <typename T>
__global__ __launch_bounds__(kPtBlk) void map_kernel(int op, const T* __restrict__ x, const T* __restrict__ u, const T* __restrict__ y,
                                                     int64_t cnt, int m, const T* __restrict__ c_raw, int c_mode, double c_min,
                                                     T* __restrict__ out) {
  const int64_t row = int64_t(blockIdx.x) * kPtBlk + threadIdx.x;
  if (row >= cnt) return;
  const T c = load_curv(c_raw, c_mode, c_min).c;
  const Vec<T> xv = load_vec(x, row, m);
  Vec<T> r;
  switch (op) {
    case MM_STEREO_EGRAD2RGRAD: {   // u / lambda^2 (impl/math.py:1452-1453)
      const T h = conf_den(xv, c) * T(0.5);
      const Vec<T> uv = load_vec(u, row, m);
      r = axpby(h * h, uv, T(0), uv);
    } break;
    case MM_STEREO_PROJU: r = load_vec(u, row, m); break;   // universal.py:54-55
    case MM_STEREO_EXP: r = project(expmap(xv, load_vec(u, row, m), c), c); break;
    case MM_STEREO_EXP_NOPROJECT: r = expmap(xv, load_vec(u, row, m), c); break;
    case MM_STEREO_RETR: {          // universal.py:73-74
      const Vec<T> uv = load_vec(u, row, m);
      r = project(axpby(T(1), xv, T(1), uv), c);
    } break;
    case MM_STEREO_PROJX: r = project(xv, c); break;
    case MM_STEREO_LOG: {           // _logmap (impl/math.py:835-841): 2 / (sqrt|c| lambda) arctan_c(sqrt|c| |s|) s / |s| = (1 - c|x|^2) phi(c |s|^2) s
      const Vec<T> sub = mobius_add(neg(xv), load_vec(y, row, m), c);
      const T sn = fmax(M<T>::sqrt(dot(sub, sub)), T(kMinNorm));
      T phi, psi;
      phi_of<T, false>(fmin(c * sn * sn, M<T>::wmax), phi, psi);
      r = axpby(conf_den(xv, c) * phi, sub, T(0), sub);
    } break;
    default: {                      // MM_STEREO_TRANSP: gyr[y, -x] u lambda_x / lambda_y (impl/math.py:1282-1298, 1359-1362)
      const Vec<T> yv = load_vec(y, row, m), uv = load_vec(u, row, m), gu = yv, gv = neg(xv);
      const T u2 = dot(gu, gu), v2 = dot(gv, gv), uvd = dot(gu, gv), uw = dot(gu, uv), vw = dot(gv, uv), cc = c * c;
      const T a = -cc * uw * v2 + c * vw + 2 * cc * uvd * vw, b = -cc * vw * u2 - c * uw;
      const T d = fmax(1 + 2 * c * uvd + cc * u2 * v2, T(kMinNorm));
      const T ratio = conf_den(yv, c) / conf_den(xv, c);
#pragma unroll
      for (int k = 0; k < kMaxDim; ++k) r.v[k] = (uv.v[k] + 2 * (a * gu.v[k] + b * gv.v[k]) / d) * ratio;
    } break;
  }
  store_vec(out, row, m, r);
}

// element-wise distance over cnt pairs, forward and / or backward
template <typename T>
__global__ __launch_bounds__(kPtBlk) void dist_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ g, int64_t cnt,
                                                      int m, int squared, const T* __restrict__ c_raw, int c_mode, double c_min,
                                                      T* __restrict__ out, T* __restrict__ gx, T* __restrict__ gy,
                                                      double* __restrict__ partials) {
  __shared__ double sh[kPtBlk];
  const int64_t row = int64_t(blockIdx.x) * kPtBlk + threadIdx.x;
  const T c = load_curv(c_raw, c_mode, c_min).c;
  double dcd = 0;
  if (row < cnt) {
    const Vec<T> xv = load_vec(x, row, m), yv = load_vec(y, row, m);
    const T a = dot(xv, xv), b = dot(yv, yv), p = dot(xv, yv);
    const Vec<T> df = axpby(T(1), xv, T(-1), yv);
    const T q = dot(df, df), D = (1 - c * a) * (1 - c * b) + c * q;
    if (out) out[row] = pair_value<T>(q, D, c, squared != 0);
    if (gx) {
      T A, At, dcp;
      pair_grad<T>(q, p, a, b, D, c, g[row], squared != 0, A, At, dcp);
      const T W = A - c * At;   // (difference form, as in the pair kernel)
      store_vec(gx, row, m, axpby(W, df, c * At * (1 - c * b), xv));
      store_vec(gy, row, m, axpby(-W, df, c * At * (1 - c * a), yv));
      dcd = double(dcp);
    }
  }
  if (partials) {
    sh[threadIdx.x] = dcd;
    __syncthreads();
    for (int h = kPtBlk / 2; h >= 1; h >>= 1) {
      if (int(threadIdx.x) < h) sh[threadIdx.x] += sh[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
  }
}

// momentum-free RSGD update (optim/rsgd.py:63-68, 82 of the reference)
template <typename T>
__global__ __launch_bounds__(kPtBlk) void rsgd_kernel(const T* __restrict__ x, const T* __restrict__ eg, int64_t cnt, int m,
                                                      const T* __restrict__ c_raw, int c_mode, double c_min, T lr, T max_grad_norm,
                                                      int exact, T* __restrict__ out) {
  const int64_t row = int64_t(blockIdx.x) * kPtBlk + threadIdx.x;
  if (row >= cnt) return;
  const T c = load_curv(c_raw, c_mode, c_min).c;
  const Vec<T> xv = load_vec(x, row, m), ev = load_vec(eg, row, m);
  const T h = conf_den(xv, c) * T(0.5);
  T f = h * h;                       // egrad2rgrad
  if (max_grad_norm > 0) {
    // Universal.norm calls math.norm(x, u) WITHOUT c (universal.py:48-52): the conformal factor of the clip is taken at c = 1
    const T nrm = 2 / conf_den(xv, T(1)) * (f * M<T>::sqrt(dot(ev, ev)));
    if (nrm > max_grad_norm) f *= max_grad_norm / nrm;
  }
  Vec<T> step;
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) step.v[k] = -lr * (f * ev.v[k]);
  store_vec(out, row, m, exact ? project(expmap(xv, step, c), c) : project(axpby(T(1), xv, T(1), step), c));
}

// products/embedding.py:37-46 of the reference: x /= max(|x| / r_max, 1), then projx
template <typename T>
__global__ __launch_bounds__(kPtBlk) void stabilize_kernel(const T* __restrict__ x, int64_t cnt, int m, const T* __restrict__ c_raw,
                                                           int c_mode, double c_min, T r_max, T* __restrict__ out) {
  const int64_t row = int64_t(blockIdx.x) * kPtBlk + threadIdx.x;
  if (row >= cnt) return;
  const T c = load_curv(c_raw, c_mode, c_min).c;
  Vec<T> xv = load_vec(x, row, m);
  const T f = fmax(M<T>::sqrt(dot(xv, xv)) / r_max, T(1));
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) xv.v[k] = xv.v[k] / f;
  store_vec(out, row, m, project(xv, c));
}

// Riemannian Adam (optim/radam.py:62-98 of the reference on Universal), one thread per point: the Riemannian gradient, its norm
// (the second moment: ONE scalar per point, before clipping, stored broadcast over the point), clipping, both moments, the
// bias-corrected direction, exp / retr, and the transport of the first moment to the new point in map_kernel's gyration form.
template <typename T>
__global__ __launch_bounds__(kPtBlk) void radam_kernel(const T* __restrict__ x, const T* __restrict__ eg, T* __restrict__ exp_avg,
                                                       T* __restrict__ exp_avg_sq, int64_t cnt, int m, const T* __restrict__ c_raw,
                                                       int c_mode, double c_min, AdamArgs<T> a, double beta1_64, double beta2_64,
                                                       T* __restrict__ out) {
  const int64_t row = int64_t(blockIdx.x) * kPtBlk + threadIdx.x;
  // the step's coefficients once per workgroup, through LDS: the two fp64 pow() stay out of the per-point code, whose `k < m`
  // masks fill the scalar registers
  // 1 - beta is formed in fp64 from the caller's fp64 betas, as the reference forms it on the host: 1 - float(0.99) is 1e-6 off 0.01
  __shared__ T coef[4];
  if (threadIdx.x == 0) {
    adam_coeffs(a, coef[0], coef[1]);
    coef[2] = T(a.nc ? 1.0 / *a.step : 1.0 - beta2_64);
    coef[3] = T(1.0 - beta1_64);
  }
  __syncthreads();
  const T beta2 = coef[0], alpha = coef[1], omb2 = coef[2], omb1 = coef[3];
  if (row < cnt) {
    const T c = load_curv(c_raw, c_mode, c_min).c;
    const Vec<T> xv = load_vec(x, row, m), ev = load_vec(eg, row, m);
    Vec<T> mo = load_vec(exp_avg, row, m);
    const T h = conf_den(xv, c) * T(0.5), f = h * h;          // egrad2rgrad
    Vec<T> r;
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) r.v[k] = f * ev.v[k];
    // Universal.norm: the conformal factor at c = 1, as in rsgd_kernel
    const T nrm = 2 / conf_den(xv, T(1)) * M<T>::sqrt(dot(r, r));
    const T v = beta2 * exp_avg_sq[row * m] + omb2 * (nrm * nrm);
    const T clip = a.max_grad_norm > 0 ? fmin(a.max_grad_norm / nrm, T(1)) : T(1);   // (nrm = 0: min(inf, 1) = 1, the zero gradient stays)
    const T s = -alpha / (M<T>::sqrt(v) + a.eps);
    Vec<T> dir, vv;
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) {
      mo.v[k] = a.beta1 * mo.v[k] + omb1 * (r.v[k] * clip);
      dir.v[k] = mo.v[k] * s;
      vv.v[k] = v;
    }
    const Vec<T> yv = a.exact ? project(expmap(xv, dir, c), c) : project(axpby(T(1), xv, T(1), dir), c);
    // gyr[y, -x] exp_avg lambda_x / lambda_y, the arithmetic of MM_STEREO_TRANSP
    const Vec<T> gv = neg(xv);
    const T u2 = dot(yv, yv), v2 = dot(gv, gv), uvd = dot(yv, gv), uw = dot(yv, mo), vw = dot(gv, mo), cc = c * c;
    const T ga = -cc * uw * v2 + c * vw + 2 * cc * uvd * vw, gb = -cc * vw * u2 - c * uw;
    const T d = fmax(1 + 2 * c * uvd + cc * u2 * v2, T(kMinNorm));
    const T ratio = conf_den(yv, c) / conf_den(xv, c);
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) mo.v[k] = (mo.v[k] + 2 * (ga * yv.v[k] + gb * gv.v[k]) / d) * ratio;
    store_vec(out, row, m, yv);
    store_vec(exp_avg, row, m, mo);
    store_vec(exp_avg_sq, row, m, vv);
  }
  adam_tick(a.step, a.ticket, gridDim.x);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
inline int status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MM_OK : int(e);
}
inline int pad_of(int m) { return m <= 4 ? 4 : m <= 8 ? 8 : 16; }
inline bool bad_curv(const void* c_raw, int c_mode, double c_min) {
  return !c_raw || c_mode < MM_STEREO_C_FREE || c_mode > MM_STEREO_C_NEGATIVE || !(c_min >= 0);
}
// does [row_begin, row_end) hold a pair?  (the last row, [n - 1, n), holds none: its pair vector is empty and may be a null pointer)
inline bool has_pairs(int64_t n, int64_t rb, int64_t re) {
  return n <= kMaxNodes ? pair_off(n, re) > pair_off(n, rb) : re > rb;   // (beyond the node limit the product would overflow)
}
inline int rows_of(size_t el) { return el == 4 ? 64 : 32; }
inline size_t slab_bytes(size_t el, int64_t n, int m) {
  const size_t nbr = size_t((n + rows_of(el) - 1) / rows_of(el)), nbc = size_t((n + kC - 1) / kC);
  return round256(el * (nbr + nbc) * size_t(m + 1) * size_t(n));
}
inline size_t partial_bytes(size_t el, int64_t n) {
  const size_t nbr = size_t((n + rows_of(el) - 1) / rows_of(el)), nbc = size_t((n + kC - 1) / kC);
  return round256(sizeof(double) * (nbr * nbc + 1));
}

template <typename T>
int fwd(const T* x, int64_t n, int m, int64_t rb, int64_t re, int squared, const T* c_raw, int c_mode, double c_min, T* out,
        hipStream_t st) {
  const dim3 grid(unsigned((n + kC - 1) / kC), unsigned((re - 1) / kC - rb / kC + 1)), wg(kC * kWaves);
  switch (pad_of(m)) {
    case 4: pdist_fwd_kernel<T, 4><<<grid, wg, 0, st>>>(x, c_raw, c_mode, c_min, int(n), m, int(rb), int(re), squared, out); break;
    case 8: pdist_fwd_kernel<T, 8><<<grid, wg, 0, st>>>(x, c_raw, c_mode, c_min, int(n), m, int(rb), int(re), squared, out); break;
    default: pdist_fwd_kernel<T, 16><<<grid, wg, 0, st>>>(x, c_raw, c_mode, c_min, int(n), m, int(rb), int(re), squared, out); break;
  }
  return status();
}

template <typename T>
int bwd(const T* x, const T* g, int64_t n, int m, int64_t rb, int64_t re, int squared, const T* c_raw, int c_mode, double c_min,
        T* grad_x, T* grad_c, void* ws, hipStream_t st) {
  constexpr int TR = Tile<T>::rows;
  const int nbr = int((n + TR - 1) / TR), nbc = int((n + kC - 1) / kC);
  T* slab = static_cast<T*>(ws);
  double* partials = reinterpret_cast<double*>(static_cast<char*>(ws) + slab_bytes(sizeof(T), n, m));
  int64_t count = 0;
  if (re > rb) {
    const int bi0 = int(rb / TR), bi1 = int((re - 1) / TR);
    const dim3 grid(nbc, bi1 - bi0 + 1), wg(kC * kWaves);
    count = int64_t(grid.x) * grid.y;
    switch (pad_of(m)) {
      case 4: pdist_bwd_kernel<T, 4><<<grid, wg, 0, st>>>(x, g, c_raw, c_mode, c_min, int(n), m, int(rb), int(re), squared, bi0, nbr, slab, partials); break;
      case 8: pdist_bwd_kernel<T, 8><<<grid, wg, 0, st>>>(x, g, c_raw, c_mode, c_min, int(n), m, int(rb), int(re), squared, bi0, nbr, slab, partials); break;
      default: pdist_bwd_kernel<T, 16><<<grid, wg, 0, st>>>(x, g, c_raw, c_mode, c_min, int(n), m, int(rb), int(re), squared, bi0, nbr, slab, partials); break;
    }
  }
  pdist_bwd_finalize_kernel<T><<<dim3(unsigned((n + 255) / 256)), dim3(256), 0, st>>>(x, slab, int(n), m, int(rb), int(re), nbr, nbc, grad_x);
  curv_finalize_kernel<T><<<dim3(1), dim3(256), 0, st>>>(partials, count, c_raw, c_mode, c_min, grad_c);
  return status();
}


// ---- products of constant-curvature factors -------------------------------------------------------------------------------
// m = sum_k max(d_k^2, 1e-8) over up to kMaxFactors factors (products/embedding.py:48-52 of the reference: no scales), every
// factor with a curvature of its own.  The forward writes the summed pair vector in one launch; the objective kernel visits every
// unordered pair once and ALL factors: (a) m, the loss term and g = d loss / d m per pair (g is read from `target`'s place with
// MM_LOSS_NONE), (b) factor by factor the phases of pdist_bwd_kernel with that g - the tiles sA / sAt are reused, g stays in RW
// registers of the lane that owns the column (the phase-1 mapping is the same for every factor), the records go to the factor's
// segment of the slab.  The transcendental part of a factor is evaluated TWICE (pair_value in (a), pair_grad in (b)): carrying
// {t, phi} of every factor from (a) to (b) would cost 2 K RW registers per lane, g costs RW.  The loss and the curvature sums leave
// as (1 + nf) fp64 partials per workgroup and are added in fixed order by product_reduce_kernel.
constexpr int kMaxFactors = 8;
template <typename T> struct PFactor {
  const T* x;
  const T* c_raw;
  T* grad_x;
  T* grad_c;
  T* slab;        // this factor's records
  double c_min;
  int m, c_mode;
};
template <typename T> struct PFactors {
  PFactor<T> f[kMaxFactors];
  int nf;
};

template <typename T, int MP>
__global__ __launch_bounds__(kC* kWaves) void product_fwd_kernel(PFactors<T> pf, int n, int rb, int re, T* __restrict__ out) {
  constexpr int RW = kC / kWaves;
  const int bj = blockIdx.x, bi = rb / kC + blockIdx.y;
  if (bj < bi) return;
  __shared__ T sx[kC][MP + 1];
  __shared__ T ss[kC];
  __shared__ T sacc[kC * kC];       // the tile's sums: a cell is written and read by one lane only
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = bj * kC + lane, jc = min(j, n - 1);
  for (int f = 0; f < pf.nf; ++f) {
    const T* __restrict__ x = pf.f[f].x;
    const int m = pf.f[f].m;
    const T c = load_curv(pf.f[f].c_raw, pf.f[f].c_mode, pf.f[f].c_min).c;
    if (f) __syncthreads();         // the previous factor's rows have been read
    if (threadIdx.x < kC) {
      const int i = min(bi * kC + int(threadIdx.x), n - 1);
      T a = 0;
#pragma unroll
      for (int k = 0; k < MP; ++k) {
        const T v = k < m ? x[size_t(i) * m + k] : T(0);
        sx[threadIdx.x][k] = v;
        a += v * v;
      }
      ss[threadIdx.x] = 1 - c * a;
    }
    T xj[MP], b = 0;
#pragma unroll
    for (int k = 0; k < MP; ++k) {
      xj[k] = k < m ? x[size_t(jc) * m + k] : T(0);
      b += xj[k] * xj[k];
    }
    const T sj = 1 - c * b;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < RW; ++r) {
      const int il = wave * RW + r, i = bi * kC + il;
      if (i < rb || i >= re) continue;   // (wave-uniform)
      T q = 0;
#pragma unroll
      for (int k = 0; k < MP; ++k) {
        const T d = sx[il][k] - xj[k];
        q += d * d;
      }
      const T v = pair_value<T>(q, ss[il] * sj + c * q, c, true);
      sacc[il * kC + lane] = f ? sacc[il * kC + lane] + v : v;   // summed in factor order
    }
  }
  const int64_t base = pair_off(n, rb);
  const bool interior = bj > bi && bj * kC + kC <= n;
  for (int r = 0; r < RW; ++r) {
    const int il = wave * RW + r, i = bi * kC + il;
    if (i < rb || i >= re) continue;
    if (interior || (j > i && j < n)) out[pair_off(n, i) - base + (j - i - 1)] = sacc[il * kC + lane];
  }
}

// node id of batch position `pos`: the low 32 bits of the index, clamped into the table
__device__ __forceinline__ int node_of(const int64_t* __restrict__ idx, int pos, int n_total) {
  return min(max(int(idx[pos]), 0), n_total - 1);
}

// The tile body of product_loss_kernel.  SUB: a node minibatch - n counts the batch's POSITIONS, the tiles, records and
// partials are laid out over them exactly as over nodes, and only the point loads (row idx[pos] of the full table) and the
// target load (dense[idx[i]][idx[j]], `target` being the dense [n_total, n_total] matrix) go through idx.
template <typename T, int MP, int LOSS, bool SUB>
__device__ __forceinline__ void product_loss_tile(const PFactors<T>& pf, const T* __restrict__ target, const int64_t* __restrict__ idx,
                                                  int n_total, int n, int rb, int re, int bi0, int nbr, LossArgs<T> la,
                                                  double* __restrict__ partials) {
  constexpr int TR = Tile<T>::rows, RW = TR / kWaves, CW = kC / kWaves, LD = kC + 1, UNR = sizeof(T) == 4 ? 2 : 1, KUN = sizeof(T) == 4 ? MP : 4;
  const int bj = blockIdx.x, bi = bi0 + blockIdx.y;
  const int slot_p = blockIdx.y * gridDim.x + blockIdx.x, tiles = gridDim.x * gridDim.y;
  const int nf = pf.nf;
  if (bj < (bi * TR + 1) / kC) return;   // no pair i < j in this tile: it leaves no partials, product_reduce_kernel skips its slots
  __shared__ T sxr[TR][MP + 1], sxc[kC][MP + 1];
  __shared__ T sar[TR], sbc[kC];
  __shared__ T sA[TR * LD], sAt[TR * LD];
  __shared__ T redc[MP + 1][kC], redr[MP + 1][TR];
  __shared__ double scv[kWaves];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = bj * kC + lane;
  double* const ptile = partials + slot_p;
  const int pstride = tiles;

  // a factor's points of the tile: rows, columns and their squared norms
  auto load_points = [&](const T* __restrict__ x, int m) {
    if (tid < TR) {
      int i = min(bi * TR + tid, n - 1);
      if constexpr (SUB) i = node_of(idx, i, n_total);
      T a = 0;
#pragma unroll
      for (int k = 0; k < MP; ++k) {
        const T v = k < m ? x[size_t(i) * m + k] : T(0);
        sxr[tid][k] = v;
        a += v * v;
      }
      sar[tid] = a;
    }
    if (wave == 1) {
      int jc = min(j, n - 1);
      if constexpr (SUB) jc = node_of(idx, jc, n_total);
      T b = 0;
#pragma unroll
      for (int k = 0; k < MP; ++k) {
        const T v = k < m ? x[size_t(jc) * m + k] : T(0);
        sxc[lane][k] = v;
        b += v * v;
      }
      sbc[lane] = b;
    }
  };
  // the fp64 sum of one value per thread, in fixed order, into this tile's partial `which`
  auto tile_sum = [&](T v, int which) {
    double d = double(v);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) d += __shfl_xor(d, s, 64);
    if (lane == 0) scv[wave] = d;
    __syncthreads();
    if (tid == 0) ptile[size_t(which) * pstride] = ((scv[0] + scv[1]) + scv[2]) + scv[3];
    __syncthreads();
  };

  // (a) g of the lane's RW pairs: d loss / d m at m = sum_k d_k^2, or the upstream value
  T gr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) gr[r] = 0;
  if constexpr (LOSS != MM_LOSS_NONE) {
    for (int f = 0; f < nf; ++f) {
      const T c = load_curv(pf.f[f].c_raw, pf.f[f].c_mode, pf.f[f].c_min).c;
      if (f) __syncthreads();
      load_points(pf.f[f].x, pf.f[f].m);
      __syncthreads();
      const T sj = 1 - c * sbc[lane];
#pragma unroll UNR
      for (int r = 0; r < RW; ++r) {   // (r is wave-uniform: gr[r] is a register picked by a scalar index, not memory)
        const int il = wave * RW + r;
        T q = 0;
#pragma unroll KUN
        for (int k = 0; k < MP; ++k) {
          const T d = sxr[il][k] - sxc[lane][k];
          q += d * d;
        }
        gr[r] += pair_value<T>(q, (1 - c * sar[il]) * sj + c * q, c, true);   // summed in factor order, as the forward does
      }
    }
    __syncthreads();
  }
  loss_resolve<T, LOSS>(la);
  const int64_t base = pair_off(n, rb);
  size_t tcol = 0;                     // SUB: the lane's column of the dense matrix
  if constexpr (SUB) tcol = size_t(node_of(idx, min(j, n - 1), n_total));
  T lacc = 0;
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int i = bi * TR + wave * RW + r;
    const bool live = j > i && j < n && i >= rb && i < re;
    T tg = T(1);
    if constexpr (SUB) {
      if (live) tg = target[size_t(node_of(idx, min(i, n - 1), n_total)) * size_t(n_total) + tcol];
    } else {
      tg = live ? target[pair_off(n, i) - base + (j - i - 1)] : T(1);
    }
    if constexpr (LOSS == MM_LOSS_NONE) {
      gr[r] = live ? tg : T(0);
    } else {
      T dldm;
      const T l = loss_term<T, LOSS>(gr[r], tg, la, dldm);
      lacc += live ? l : T(0);
      gr[r] = live ? dldm : T(0);
    }
  }
  if constexpr (LOSS != MM_LOSS_NONE) tile_sum(lacc, 0);
  else if (tid == 0) ptile[0] = 0.0;

  // (b) factor by factor: the phases of pdist_bwd_kernel with g from the registers
  for (int f = 0; f < nf; ++f) {
    const T c = load_curv(pf.f[f].c_raw, pf.f[f].c_mode, pf.f[f].c_min).c;
    const int m = pf.f[f].m;
    T* __restrict__ slab = pf.f[f].slab;
    if (f || LOSS != MM_LOSS_NONE) __syncthreads();
    load_points(pf.f[f].x, m);
    __syncthreads();
    T cacc = 0;
    {
      const T b = sbc[lane], sj = 1 - c * b;
#pragma unroll UNR
      for (int r = 0; r < RW; ++r) {
        const int il = wave * RW + r;
        T q = 0, p = 0;
#pragma unroll KUN
        for (int k = 0; k < MP; ++k) {
          const T xi = sxr[il][k], xj = sxc[lane][k], d = xi - xj;
          q += d * d;
          p += xi * xj;
        }
        const T a = sar[il], gv = gr[r];
        T A = 0, At = 0, dcp = 0;
        if (gv != T(0)) pair_grad<T>(q, p, a, b, (1 - c * a) * sj + c * q, c, gv, true, A, At, dcp);   // (g = 0: no pair here, or none of its business)
        sA[il * LD + lane] = A;
        sAt[il * LD + lane] = At;
        cacc += dcp;
      }
    }
    __syncthreads();
    // columns
    T cw[MP], xo[MP], cvs = 0;
#pragma unroll
    for (int k = 0; k < MP; ++k) {
      cw[k] = 0;
      xo[k] = sxc[lane][k];
    }
#pragma unroll UNR
    for (int r = 0; r < RW; ++r) {
      const int il = wave * RW + r;
      const T A = sA[il * LD + lane], At = sAt[il * LD + lane];
      const T W = A - c * At;
      cvs += c * At * (1 - c * sar[il]);
#pragma unroll
      for (int k = 0; k < MP; ++k) cw[k] += W * (xo[k] - sxr[il][k]);
    }
    for (int wv = 0; wv < kWaves; ++wv) {
      if (wave == wv) {
#pragma unroll
        for (int k = 0; k < MP; ++k) redc[k][lane] = wv == 0 ? cw[k] : redc[k][lane] + cw[k];
        redc[MP][lane] = wv == 0 ? cvs : redc[MP][lane] + cvs;
      }
      __syncthreads();
    }
    // rows: the tile turned
    T rw[MP], rvs = 0;
#pragma unroll
    for (int k = 0; k < MP; ++k) rw[k] = 0;
    if (lane < TR) {
#pragma unroll
      for (int k = 0; k < MP; ++k) xo[k] = sxr[lane][k];
#pragma unroll UNR
      for (int jj = 0; jj < CW; ++jj) {
        const int jl = wave * CW + jj;
        const T A = sA[lane * LD + jl], At = sAt[lane * LD + jl];
        const T W = A - c * At;
        rvs += c * At * (1 - c * sbc[jl]);
#pragma unroll
        for (int k = 0; k < MP; ++k) rw[k] += W * (xo[k] - sxc[jl][k]);
      }
    }
    for (int wv = 0; wv < kWaves; ++wv) {
      if (wave == wv && lane < TR) {
#pragma unroll
        for (int k = 0; k < MP; ++k) redr[k][lane] = wv == 0 ? rw[k] : redr[k][lane] + rw[k];
        redr[MP][lane] = wv == 0 ? rvs : redr[MP][lane] + rvs;
      }
      __syncthreads();
    }
    const size_t ns = size_t(n), comps = size_t(m) + 1;
    if (wave == 0 && j < n) {           // column records of row block bi
      T* rec = slab + size_t(bi) * comps * ns + j;
      for (int k = 0; k < m; ++k) rec[k * ns] = redc[k][lane];
      rec[size_t(m) * ns] = redc[MP][lane];
    }
    if (wave == 1 && lane < TR && bi * TR + lane < n) {   // row records of column block bj
      T* rec = slab + size_t(nbr + bj) * comps * ns + (bi * TR + lane);
      for (int k = 0; k < m; ++k) rec[k * ns] = redr[k][lane];
      rec[size_t(m) * ns] = redr[MP][lane];
    }
    tile_sum(cacc, 1 + f);
  }
}

template <typename T, int MP, int LOSS>
__global__ __launch_bounds__(kC* kWaves) void product_loss_kernel(PFactors<T> pf, const T* __restrict__ target, int n, int rb, int re,
                                                                  int bi0, int nbr, LossArgs<T> la, double* __restrict__ partials) {
  product_loss_tile<T, MP, LOSS, false>(pf, target, nullptr, 0, n, rb, re, bi0, nbr, la, partials);
}

// the same pair pass over the bs positions of a node minibatch (mm_stereo_product_loss_subset)
template <typename T, int MP, int LOSS>
__global__ __launch_bounds__(kC* kWaves) void subset_loss_kernel(PFactors<T> pf, const T* __restrict__ dense, const int64_t* __restrict__ idx,
                                                                 int n_total, int bs, int rb, int re, int bi0, int nbr, LossArgs<T> la,
                                                                 double* __restrict__ partials) {
  product_loss_tile<T, MP, LOSS, true>(pf, dense, idx, n_total, bs, rb, re, bi0, nbr, la, partials);
}

// grad_x of factor blockIdx.y: a node's records in slot order, as pdist_bwd_finalize_kernel adds them (SUB: the records of batch
// position v, the point and the gradient row idx[v] of the full table)
template <typename T, bool SUB>
__device__ __forceinline__ void product_finalize_node(const PFactors<T>& pf, const int64_t* __restrict__ idx, int n_total, int n, int rb,
                                                      int re, int nbr, int nbc) {
  constexpr int TR = Tile<T>::rows;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const PFactor<T>& F = pf.f[blockIdx.y];
  const T* __restrict__ x = F.x;
  const T* __restrict__ slab = F.slab;
  T* __restrict__ grad = F.grad_x;
  const int m = F.m;
  const size_t ns = size_t(n), comps = size_t(m) + 1;
  T acc[kMaxDim + 1];
#pragma unroll
  for (int k = 0; k <= kMaxDim; ++k) acc[k] = 0;
  if (re > rb) {
    const int bi0 = rb / TR, bi1 = (re - 1) / TR;
    const int last = v >= 1 ? min(bi1, (v - 1) / TR) : -1;
    for (int s = bi0; s <= last; ++s) {
      const T* rec = slab + size_t(s) * comps * ns + v;
#pragma unroll
      for (int k = 0; k <= kMaxDim; ++k)
        if (k <= m) acc[k] += rec[k * ns];
    }
    if (v >= rb && v < re) {
      const int bv = v / TR;
      for (int s = (bv * TR + 1) / kC; s < nbc; ++s) {
        const T* rec = slab + size_t(nbr + s) * comps * ns + v;
#pragma unroll
        for (int k = 0; k <= kMaxDim; ++k)
          if (k <= m) acc[k] += rec[k * ns];
      }
    }
  }
  T vs = 0;
#pragma unroll
  for (int k = 0; k <= kMaxDim; ++k)
    if (k == m) vs = acc[k];
  int row = v;
  if constexpr (SUB) row = node_of(idx, v, n_total);
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k)
    if (k < m) grad[size_t(row) * m + k] = acc[k] + vs * x[size_t(row) * m + k];
}

template <typename T>
__global__ __launch_bounds__(256) void product_finalize_kernel(PFactors<T> pf, int n, int rb, int re, int nbr, int nbc) {
  product_finalize_node<T, false>(pf, nullptr, 0, n, rb, re, nbr, nbc);
}

template <typename T>
__global__ __launch_bounds__(256) void subset_finalize_kernel(PFactors<T> pf, const int64_t* __restrict__ idx, int n_total, int bs, int rb,
                                                              int re, int nbr, int nbc) {
  product_finalize_node<T, true>(pf, idx, n_total, bs, rb, re, nbr, nbc);
}

// exact zeros in every gradient table of a minibatch step (factor blockIdx.y): the rows outside the batch keep them
template <typename T> __global__ __launch_bounds__(256) void subset_clear_kernel(PFactors<T> pf, int64_t n_total) {
  const PFactor<T>& F = pf.f[blockIdx.y];
  const int64_t count = n_total * F.m;
  for (int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x; k < count; k += int64_t(gridDim.x) * 256) F.grad_x[k] = T(0);
}

// block 0: the loss; block 1 + k: grad_c of factor k = dc/dc_raw * its partials - fp64, fixed order
template <typename T>
__global__ __launch_bounds__(256) void product_reduce_kernel(PFactors<T> pf, const double* __restrict__ partials, int count, int gx,
                                                             int bi0, T* __restrict__ loss_out) {
  constexpr int TR = Tile<T>::rows;
  __shared__ double sh[256];
  const int which = blockIdx.x;
  const double* __restrict__ p = partials + size_t(which) * count;
  double s = 0;
  for (int k = threadIdx.x; k < count; k += 256) {
    const int by = k / gx, bx = k - by * gx;
    if (bx >= ((bi0 + by) * TR + 1) / kC) s += p[k];   // (a tile without a pair i < j wrote nothing)
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (which == 0) {
    if (loss_out) loss_out[0] = T(sh[0]);
  } else {
    const PFactor<T>& F = pf.f[which - 1];
    F.grad_c[0] = T(sh[0] * double(load_curv(F.c_raw, F.c_mode, F.c_min).dc));
  }
}

inline size_t product_partial_bytes(size_t el, int64_t n, int nf) {
  const size_t nbr = size_t((n + rows_of(el) - 1) / rows_of(el)), nbc = size_t((n + kC - 1) / kC);
  return round256(sizeof(double) * (size_t(nf + 1) * nbr * nbc + 1));
}
// what the product calls refuse, in the order MM_ERR_ARG before MM_ERR_UNSUPPORTED
inline int product_check(int dtype, const mm_stereo_factor* f, int nf, int64_t n, int64_t rb, int64_t re, bool back) {
  if ((dtype != MM_F32 && dtype != MM_F64) || !f || nf < 1 || n < 0 || rb < 0 || re < rb || re > n) return MM_ERR_ARG;
  bool wide = nf > kMaxFactors;
  for (int k = 0; k < nf && k < 64; ++k) {
    if (f[k].m < 1 || bad_curv(f[k].c_raw, f[k].c_mode, f[k].c_min)) return MM_ERR_ARG;
    if (back && !f[k].grad_c) return MM_ERR_ARG;
    if (n >= 1 && back && (!f[k].x || !f[k].grad_x)) return MM_ERR_ARG;
    if (n >= 2 && !back && has_pairs(n, rb, re) && !f[k].x) return MM_ERR_ARG;
    wide = wide || f[k].m > kMaxDim;
  }
  return wide || n > kMaxNodes ? MM_ERR_UNSUPPORTED : MM_OK;
}
template <typename T> PFactors<T> product_args(const mm_stereo_factor* f, int nf, int64_t n, void* ws, int* widest) {
  PFactors<T> pf{};
  pf.nf = nf;
  char* at = static_cast<char*>(ws);
  *widest = 1;
  for (int k = 0; k < nf; ++k) {
    pf.f[k] = PFactor<T>{static_cast<const T*>(f[k].x), static_cast<const T*>(f[k].c_raw), static_cast<T*>(f[k].grad_x),
                         static_cast<T*>(f[k].grad_c), reinterpret_cast<T*>(at), f[k].c_min, f[k].m, f[k].c_mode};
    if (ws) at += slab_bytes(sizeof(T), n, f[k].m);
    *widest = f[k].m > *widest ? f[k].m : *widest;
  }
  return pf;
}

template <typename T>
int product_fwd(const mm_stereo_factor* f, int nf, int64_t n, int64_t rb, int64_t re, T* out, hipStream_t st) {
  int widest;
  const PFactors<T> pf = product_args<T>(f, nf, n, nullptr, &widest);
  const dim3 grid(unsigned((n + kC - 1) / kC), unsigned((re - 1) / kC - rb / kC + 1)), wg(kC * kWaves);
  switch (pad_of(widest)) {
    case 4: product_fwd_kernel<T, 4><<<grid, wg, 0, st>>>(pf, int(n), int(rb), int(re), out); break;
    case 8: product_fwd_kernel<T, 8><<<grid, wg, 0, st>>>(pf, int(n), int(rb), int(re), out); break;
    default: product_fwd_kernel<T, 16><<<grid, wg, 0, st>>>(pf, int(n), int(rb), int(re), out); break;
  }
  return status();
}

template <typename T, int LOSS>
void product_loss_launch(int pad, dim3 grid, hipStream_t st, const PFactors<T>& pf, const T* target, int n, int rb, int re, int bi0,
                         int nbr, LossArgs<T> la, double* partials) {
  const dim3 wg(kC * kWaves);
  switch (pad) {
    case 4: product_loss_kernel<T, 4, LOSS><<<grid, wg, 0, st>>>(pf, target, n, rb, re, bi0, nbr, la, partials); break;
    case 8: product_loss_kernel<T, 8, LOSS><<<grid, wg, 0, st>>>(pf, target, n, rb, re, bi0, nbr, la, partials); break;
    default: product_loss_kernel<T, 16, LOSS><<<grid, wg, 0, st>>>(pf, target, n, rb, re, bi0, nbr, la, partials); break;
  }
}

template <typename T>
int product_loss(int loss_kind, const mm_stereo_factor* f, int nf, const T* target, int64_t n, int64_t rb, int64_t re, double alpha,
                 double eps, int terms, const double* loss_params, T* loss_out, void* ws, hipStream_t st) {
  constexpr int TR = Tile<T>::rows;
  int widest;
  const PFactors<T> pf = product_args<T>(f, nf, n, ws, &widest);
  const int nbr = int((n + TR - 1) / TR), nbc = int((n + kC - 1) / kC);
  size_t slabs = 0;
  for (int k = 0; k < nf; ++k) slabs += slab_bytes(sizeof(T), n, f[k].m);
  double* partials = reinterpret_cast<double*>(static_cast<char*>(ws) + slabs);
  const bool pairs = n >= 2 && has_pairs(n, rb, re);
  int count = 0, bi0 = 0;
  if (pairs) {
    bi0 = int(rb / TR);
    const int bi1 = int((re - 1) / TR);
    const dim3 grid(nbc, bi1 - bi0 + 1);
    count = int(grid.x * grid.y);
    LossArgs<T> la{nullptr, T(alpha), T(eps), terms, nullptr, loss_params};
    const int pad = pad_of(widest);
    if (loss_kind == MM_LOSS_STRESS)
      product_loss_launch<T, MM_LOSS_STRESS>(pad, grid, st, pf, target, int(n), int(rb), int(re), bi0, nbr, la, partials);
    else if (loss_kind == MM_LOSS_QUOTIENT)
      product_loss_launch<T, MM_LOSS_QUOTIENT>(pad, grid, st, pf, target, int(n), int(rb), int(re), bi0, nbr, la, partials);
    else
      product_loss_launch<T, MM_LOSS_NONE>(pad, grid, st, pf, target, int(n), int(rb), int(re), bi0, nbr, la, partials);
  }
  if (n >= 1)   // (a range without pairs: the sums over no record are the zero gradients)
    product_finalize_kernel<T><<<dim3(unsigned((n + 255) / 256), unsigned(nf)), dim3(256), 0, st>>>(pf, int(n), int(rb), pairs ? int(re) : int(rb), nbr, nbc);
  product_reduce_kernel<T><<<dim3(unsigned(nf + 1)), dim3(256), 0, st>>>(pf, partials, count, nbc, bi0, loss_kind == MM_LOSS_NONE ? nullptr : loss_out);
  return status();
}

template <typename T, int LOSS>
void subset_loss_launch(int pad, dim3 grid, hipStream_t st, const PFactors<T>& pf, const T* dense, const int64_t* idx, int n_total, int bs,
                        int rb, int re, int bi0, int nbr, LossArgs<T> la, double* partials) {
  const dim3 wg(kC * kWaves);
  switch (pad) {
    case 4: subset_loss_kernel<T, 4, LOSS><<<grid, wg, 0, st>>>(pf, dense, idx, n_total, bs, rb, re, bi0, nbr, la, partials); break;
    case 8: subset_loss_kernel<T, 8, LOSS><<<grid, wg, 0, st>>>(pf, dense, idx, n_total, bs, rb, re, bi0, nbr, la, partials); break;
    default: subset_loss_kernel<T, 16, LOSS><<<grid, wg, 0, st>>>(pf, dense, idx, n_total, bs, rb, re, bi0, nbr, la, partials); break;
  }
}

// product_loss over the batch's positions: the workspace, the tiles and the reduction are those of n = bs; one launch in front
// clears the full-size gradient tables, the finalize writes the batch's rows - four launches whatever nf is
template <typename T>
int product_loss_subset(int loss_kind, const mm_stereo_factor* f, int nf, const T* dense, int64_t n_total, const int64_t* idx, int64_t bs,
                        int64_t rb, int64_t re, double alpha, double eps, int terms, const double* loss_params, T* loss_out, void* ws,
                        hipStream_t st) {
  constexpr int TR = Tile<T>::rows;
  int widest;
  const PFactors<T> pf = product_args<T>(f, nf, bs, ws, &widest);
  const int nbr = int((bs + TR - 1) / TR), nbc = int((bs + kC - 1) / kC);
  size_t slabs = 0;
  for (int k = 0; k < nf; ++k) slabs += slab_bytes(sizeof(T), bs, f[k].m);
  double* partials = reinterpret_cast<double*>(static_cast<char*>(ws) + slabs);
  const bool pairs = bs >= 2 && has_pairs(bs, rb, re);
  int count = 0, bi0 = 0;
  if (n_total >= 1) {
    const int64_t blocks = (n_total * widest + 255) / 256;
    subset_clear_kernel<T><<<dim3(unsigned(blocks < 4096 ? blocks : 4096), unsigned(nf)), dim3(256), 0, st>>>(pf, n_total);
  }
  if (pairs) {
    bi0 = int(rb / TR);
    const int bi1 = int((re - 1) / TR);
    const dim3 grid(nbc, bi1 - bi0 + 1);
    count = int(grid.x * grid.y);
    LossArgs<T> la{nullptr, T(alpha), T(eps), terms, nullptr, loss_params};
    const int pad = pad_of(widest);
    if (loss_kind == MM_LOSS_STRESS)
      subset_loss_launch<T, MM_LOSS_STRESS>(pad, grid, st, pf, dense, idx, int(n_total), int(bs), int(rb), int(re), bi0, nbr, la, partials);
    else
      subset_loss_launch<T, MM_LOSS_QUOTIENT>(pad, grid, st, pf, dense, idx, int(n_total), int(bs), int(rb), int(re), bi0, nbr, la, partials);
    subset_finalize_kernel<T><<<dim3(unsigned((bs + 255) / 256), unsigned(nf)), dim3(256), 0, st>>>(pf, idx, int(n_total), int(bs), int(rb),
                                                                                                    int(re), nbr, nbc);
  }
  product_reduce_kernel<T><<<dim3(unsigned(nf + 1)), dim3(256), 0, st>>>(pf, partials, count, nbc, bi0, loss_out);
  return status();
}

}  // namespace stereo
}  // namespace mm

using namespace mm::stereo;

extern "C" {

size_t mm_stereo_pdist_ws_bytes(int dtype, int64_t n, int m) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || n > kMaxNodes || m < 1 || m > kMaxDim) return 0;
  const size_t el = dtype == MM_F64 ? 8 : 4;
  return slab_bytes(el, n, m) + partial_bytes(el, n);
}

int mm_stereo_pdist_fwd(int dtype, const void* x, int64_t n, int m, int64_t row_begin, int64_t row_end, int squared,
                        const void* c_raw, int c_mode, double c_min, void* out, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || m < 1 || row_begin < 0 || row_end < row_begin || row_end > n ||
      bad_curv(c_raw, c_mode, c_min))
    return MM_ERR_ARG;
  if (n >= 2 && has_pairs(n, row_begin, row_end) && (!x || !out)) return MM_ERR_ARG;
  if (m > kMaxDim || n > kMaxNodes) return MM_ERR_UNSUPPORTED;
  if (n < 2 || !has_pairs(n, row_begin, row_end)) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MM_F32)
    return fwd<float>(static_cast<const float*>(x), n, m, row_begin, row_end, squared, static_cast<const float*>(c_raw), c_mode, c_min,
                      static_cast<float*>(out), st);
  return fwd<double>(static_cast<const double*>(x), n, m, row_begin, row_end, squared, static_cast<const double*>(c_raw), c_mode,
                     c_min, static_cast<double*>(out), st);
}

int mm_stereo_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int m, int64_t row_begin, int64_t row_end, int squared,
                        const void* c_raw, int c_mode, double c_min, void* grad_x, void* grad_c, void* ws, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || m < 1 || row_begin < 0 || row_end < row_begin || row_end > n ||
      bad_curv(c_raw, c_mode, c_min) || !grad_c)
    return MM_ERR_ARG;
  if (n >= 2 && (!x || !grad_x || !ws || (has_pairs(n, row_begin, row_end) && !g))) return MM_ERR_ARG;
  if (m > kMaxDim || n > kMaxNodes) return MM_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n < 2) {   // no pair: nothing but a zero curvature gradient
    const hipError_t e = mm::clear_async(grad_c, dtype == MM_F64 ? 8 : 4, st);
    return e == hipSuccess ? MM_OK : int(e);
  }
  if (dtype == MM_F32)
    return bwd<float>(static_cast<const float*>(x), static_cast<const float*>(g), n, m, row_begin, row_end, squared,
                      static_cast<const float*>(c_raw), c_mode, c_min, static_cast<float*>(grad_x), static_cast<float*>(grad_c), ws, st);
  return bwd<double>(static_cast<const double*>(x), static_cast<const double*>(g), n, m, row_begin, row_end, squared,
                     static_cast<const double*>(c_raw), c_mode, c_min, static_cast<double*>(grad_x), static_cast<double*>(grad_c), ws, st);
}

int mm_stereo_dist(int dtype, const void* x, const void* y, const void* g, int64_t cnt, int m, int squared, const void* c_raw,
                   int c_mode, double c_min, void* out, void* grad_x, void* grad_y, void* grad_c, void* ws, mm_stream_t stream) {
  const bool back = grad_x || grad_y || grad_c;
  if ((dtype != MM_F32 && dtype != MM_F64) || cnt < 0 || m < 1 || bad_curv(c_raw, c_mode, c_min) || (!out && !back)) return MM_ERR_ARG;
  if (back && (!grad_x || !grad_y || !grad_c || !ws)) return MM_ERR_ARG;
  if (cnt > 0 && (!x || !y || (back && !g))) return MM_ERR_ARG;
  if (m > kMaxDim || cnt > (int64_t(1) << 31) * kPtBlk - 1) return MM_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t blocks = (cnt + kPtBlk - 1) / kPtBlk;
  double* partials = back ? static_cast<double*>(ws) : nullptr;
  if (dtype == MM_F32) {
    using T = float;
    if (cnt > 0)
      dist_kernel<T><<<dim3(unsigned(blocks)), dim3(kPtBlk), 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const T*>(g), cnt, m, squared,
                                                                      static_cast<const T*>(c_raw), c_mode, c_min, static_cast<T*>(out), static_cast<T*>(grad_x),
                                                                      static_cast<T*>(grad_y), partials);
    if (back) curv_finalize_kernel<T><<<dim3(1), dim3(256), 0, st>>>(partials, blocks, static_cast<const T*>(c_raw), c_mode, c_min, static_cast<T*>(grad_c));
  } else {
    using T = double;
    if (cnt > 0)
      dist_kernel<T><<<dim3(unsigned(blocks)), dim3(kPtBlk), 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const T*>(g), cnt, m, squared,
                                                                      static_cast<const T*>(c_raw), c_mode, c_min, static_cast<T*>(out), static_cast<T*>(grad_x),
                                                                      static_cast<T*>(grad_y), partials);
    if (back) curv_finalize_kernel<T><<<dim3(1), dim3(256), 0, st>>>(partials, blocks, static_cast<const T*>(c_raw), c_mode, c_min, static_cast<T*>(grad_c));
  }
  return status();
}

int mm_stereo_map(int dtype, int op, const void* x, const void* u, const void* y, int64_t cnt, int m, const void* c_raw, int c_mode,
                  double c_min, void* out, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || op < MM_STEREO_EGRAD2RGRAD || op > MM_STEREO_TRANSP || cnt < 0 || m < 1 ||
      bad_curv(c_raw, c_mode, c_min))
    return MM_ERR_ARG;
  const bool needs_u = op != MM_STEREO_PROJX && op != MM_STEREO_LOG, needs_y = op == MM_STEREO_LOG || op == MM_STEREO_TRANSP;
  if (cnt > 0 && (!x || !out || (needs_u && !u) || (needs_y && !y))) return MM_ERR_ARG;
  if (m > kMaxDim || cnt > (int64_t(1) << 31) * kPtBlk - 1) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned((cnt + kPtBlk - 1) / kPtBlk)), wg(kPtBlk);
  if (dtype == MM_F32) {
    using T = float;
    map_kernel<T><<<grid, wg, 0, st>>>(op, static_cast<const T*>(x), static_cast<const T*>(u), static_cast<const T*>(y), cnt, m,
                                       static_cast<const T*>(c_raw), c_mode, c_min, static_cast<T*>(out));
  } else {
    using T = double;
    map_kernel<T><<<grid, wg, 0, st>>>(op, static_cast<const T*>(x), static_cast<const T*>(u), static_cast<const T*>(y), cnt, m,
                                       static_cast<const T*>(c_raw), c_mode, c_min, static_cast<T*>(out));
  }
  return status();
}

int mm_stereo_rsgd_step(int dtype, const void* x, const void* egrad, int64_t cnt, int m, const void* c_raw, int c_mode, double c_min,
                        double lr, double max_grad_norm, int exact, void* x_new, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || cnt < 0 || m < 1 || bad_curv(c_raw, c_mode, c_min)) return MM_ERR_ARG;
  if (cnt > 0 && (!x || !egrad || !x_new)) return MM_ERR_ARG;
  if (m > kMaxDim || cnt > (int64_t(1) << 31) * kPtBlk - 1) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned((cnt + kPtBlk - 1) / kPtBlk)), wg(kPtBlk);
  if (dtype == MM_F32) {
    using T = float;
    rsgd_kernel<T><<<grid, wg, 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(egrad), cnt, m, static_cast<const T*>(c_raw), c_mode,
                                        c_min, T(lr), T(max_grad_norm), exact, static_cast<T*>(x_new));
  } else {
    using T = double;
    rsgd_kernel<T><<<grid, wg, 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(egrad), cnt, m, static_cast<const T*>(c_raw), c_mode,
                                        c_min, T(lr), T(max_grad_norm), exact, static_cast<T*>(x_new));
  }
  return status();
}

int mm_stereo_radam_step(int dtype, const void* x, const void* egrad, void* exp_avg, void* exp_avg_sq, double* step, unsigned* ticket,
                         int64_t cnt, int m, const void* c_raw, int c_mode, double c_min, double lr, double beta1, double beta2, int nc,
                         double eps, double max_grad_norm, int exact, void* x_new, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || cnt < 0 || m < 1 || bad_curv(c_raw, c_mode, c_min) || !step || !ticket) return MM_ERR_ARG;
  if (cnt > 0 && (!x || !egrad || !exp_avg || !exp_avg_sq || !x_new)) return MM_ERR_ARG;
  if (m > kMaxDim || cnt > (int64_t(1) << 31) * kPtBlk - 1) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned((cnt + kPtBlk - 1) / kPtBlk)), wg(kPtBlk);
  if (dtype == MM_F32) {
    using T = float;
    const mm::AdamArgs<T> a{T(lr), T(beta1), T(beta2), T(eps), T(max_grad_norm), nc, exact, step, ticket};
    radam_kernel<T><<<grid, wg, 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(egrad), static_cast<T*>(exp_avg),
                                         static_cast<T*>(exp_avg_sq), cnt, m, static_cast<const T*>(c_raw), c_mode, c_min, a,
                                         beta1, beta2, static_cast<T*>(x_new));
  } else {
    using T = double;
    const mm::AdamArgs<T> a{T(lr), T(beta1), T(beta2), T(eps), T(max_grad_norm), nc, exact, step, ticket};
    radam_kernel<T><<<grid, wg, 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(egrad), static_cast<T*>(exp_avg),
                                         static_cast<T*>(exp_avg_sq), cnt, m, static_cast<const T*>(c_raw), c_mode, c_min, a,
                                         beta1, beta2, static_cast<T*>(x_new));
  }
  return status();
}

int mm_stereo_stabilize(int dtype, const void* x, int64_t cnt, int m, const void* c_raw, int c_mode, double c_min, double r_max,
                        void* x_new, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || cnt < 0 || m < 1 || bad_curv(c_raw, c_mode, c_min) || !(r_max > 0)) return MM_ERR_ARG;
  if (cnt > 0 && (!x || !x_new)) return MM_ERR_ARG;
  if (m > kMaxDim || cnt > (int64_t(1) << 31) * kPtBlk - 1) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned((cnt + kPtBlk - 1) / kPtBlk)), wg(kPtBlk);
  if (dtype == MM_F32) {
    using T = float;
    stabilize_kernel<T><<<grid, wg, 0, st>>>(static_cast<const T*>(x), cnt, m, static_cast<const T*>(c_raw), c_mode, c_min, T(r_max), static_cast<T*>(x_new));
  } else {
    using T = double;
    stabilize_kernel<T><<<grid, wg, 0, st>>>(static_cast<const T*>(x), cnt, m, static_cast<const T*>(c_raw), c_mode, c_min, T(r_max), static_cast<T*>(x_new));
  }
  return status();
}

size_t mm_stereo_product_ws_bytes(int dtype, int64_t n, int nf, const int32_t* m) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || n > kMaxNodes || nf < 1 || nf > kMaxFactors || !m) return 0;
  const size_t el = dtype == MM_F64 ? 8 : 4;
  size_t b = product_partial_bytes(el, n, nf);
  for (int k = 0; k < nf; ++k) {
    if (m[k] < 1 || m[k] > kMaxDim) return 0;
    b += slab_bytes(el, n, m[k]);
  }
  return b;
}

int mm_stereo_product_pdist_fwd(int dtype, const mm_stereo_factor* f, int nf, int64_t n, int64_t row_begin, int64_t row_end, void* out,
                                mm_stream_t stream) {
  const int rc = product_check(dtype, f, nf, n, row_begin, row_end, false);
  if (rc == MM_ERR_ARG) return rc;
  if (n >= 2 && n <= kMaxNodes && has_pairs(n, row_begin, row_end) && !out) return MM_ERR_ARG;
  if (rc != MM_OK) return rc;
  if (n < 2 || !has_pairs(n, row_begin, row_end)) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MM_F32) return product_fwd<float>(f, nf, n, row_begin, row_end, static_cast<float*>(out), st);
  return product_fwd<double>(f, nf, n, row_begin, row_end, static_cast<double*>(out), st);
}

int mm_stereo_product_loss(int dtype, int loss_kind, const mm_stereo_factor* f, int nf, const void* target, int64_t n, int64_t row_begin,
                           int64_t row_end, double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* ws,
                           mm_stream_t stream) {
  const int rc = product_check(dtype, f, nf, n, row_begin, row_end, true);
  if (rc == MM_ERR_ARG) return rc;
  if ((loss_kind != MM_LOSS_NONE && loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) || !ws ||
      (loss_kind != MM_LOSS_NONE && !loss_out))
    return MM_ERR_ARG;
  if (n >= 2 && n <= kMaxNodes && has_pairs(n, row_begin, row_end) && !target) return MM_ERR_ARG;
  if (rc != MM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MM_F32)
    return product_loss<float>(loss_kind, f, nf, static_cast<const float*>(target), n, row_begin, row_end, alpha, eps, terms, loss_params,
                               static_cast<float*>(loss_out), ws, st);
  return product_loss<double>(loss_kind, f, nf, static_cast<const double*>(target), n, row_begin, row_end, alpha, eps, terms, loss_params,
                              static_cast<double*>(loss_out), ws, st);
}

int mm_stereo_product_loss_subset(int dtype, int loss_kind, const mm_stereo_factor* f, int nf, const void* dense, int64_t n_total,
                                  const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end, double alpha, double eps, int terms,
                                  const double* loss_params, void* loss_out, void* ws, mm_stream_t stream) {
  if (n_total < 0 || bs < 0 || bs > n_total) return MM_ERR_ARG;
  int rc = product_check(dtype, f, nf, bs, row_begin, row_end, true);
  if (rc == MM_ERR_ARG) return rc;
  for (int k = 0; k < nf && k < 64; ++k)   // (the tables are cleared even when the batch is empty)
    if (n_total >= 1 && (!f[k].x || !f[k].grad_x)) return MM_ERR_ARG;
  if ((loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) || !ws || !loss_out || !idx || !dense) return MM_ERR_ARG;
  if (n_total > INT32_MAX) rc = MM_ERR_UNSUPPORTED;   // node ids are the low 32 bits of an index
  if (rc != MM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MM_F32)
    return product_loss_subset<float>(loss_kind, f, nf, static_cast<const float*>(dense), n_total, idx, bs, row_begin, row_end, alpha, eps,
                                      terms, loss_params, static_cast<float*>(loss_out), ws, st);
  return product_loss_subset<double>(loss_kind, f, nf, static_cast<const double*>(dense), n_total, idx, bs, row_begin, row_end, alpha, eps,
                                     terms, loss_params, static_cast<double*>(loss_out), ws, st);
}

}  // extern "C"
