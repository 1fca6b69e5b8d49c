// SO(n), n in {2, 3, 4}: the geodesic distance of one pair, its gradient, log and exp — one n x n matrix per lane, in registers.
//
// For X, Y in SO(n), D = Y - X and R = X^T Y:  D^T D / 2 = I - sym(R), so the singular values of D are sigma_k = 2 sin(theta_k / 2)
// with theta_k the rotation angles of R (every rotation plane twice, the fixed axis gives sigma = 0), and the reference's distance
// (orthogonal.py:13-21: the sum of the squared arguments of all eigenvalues of R, = ||log R||_F^2) is
//     d^2(X, Y) = sum_k psi(sigma_k^2 / 2),   psi(x) = 4 asin^2(sqrt(x / 2))   (theta_k = 2 asin(sigma_k / 2)).
// No eigenproblem of a non-symmetric matrix, no acos of a cosine next to 1, no cancellation beyond the subtraction Y - X of nearby
// numbers, which is exact.  The library DEFINES d^2 as the ambient function F(X, Y) = tr psi((Y - X)^T (Y - X) / 2): smooth on all
// pairs of matrices with sigma < 2, equal to the geodesic distance on SO(n), and what inputs orthogonal only to rounding get.
// With D V = B from the one-sided Jacobi (svd_onesided, smallmat.hpp: the small singular values keep their relative accuracy, and
// repeated ones — the normal case here — only mean that any orthogonal basis of the plane serves):
//     dF/dY = B diag(psi'_k) V^T,  dF/dX = -dF/dY,   psi' = 2 theta / sin theta = 2 asin(s) / (s sqrt(1 - s^2)), s = sigma / 2,
// with the limit 2 at s -> 0.  theta = pi (sigma = 2, or a pair in different components of O(n)) is the cut locus: s is clamped
// to 1, so d^2 stays finite, and 1 - s^2 is floored at kCutFloor = 1e-12 (sin theta >= 2e-6 next to the cut), so the gradient —
// not defined there — is finite.
#pragma once
#include <hip/hip_runtime.h>

#include "mat_common.hpp"
#include "smallmat.hpp"

namespace mm {
namespace so {

constexpr double kCutFloor = 1e-12;   // floor under 1 - s^2 = cos^2(theta / 2)

template <typename T> __device__ __forceinline__ T asin_(T s);
template <> __device__ __forceinline__ float asin_<float>(float s) { return ::asinf(s); }
template <> __device__ __forceinline__ double asin_<double>(double s) { return ::asin(s); }

template <typename T, int N> __device__ __forceinline__ void load(const T* __restrict__ p, T (&a)[N][N]) {
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) a[r][c] = p[r * N + c];
}
template <typename T, int N> __device__ __forceinline__ void store(T* __restrict__ p, const T (&a)[N][N]) {
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) p[r * N + c] = a[r][c];
}

// squared column norms of b
template <typename T, int N> __device__ __forceinline__ void colnorm2(const T (&b)[N][N], T (&nn)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    T s = T(0);
#pragma unroll
    for (int r = 0; r < N; ++r) s = Num<T>::fma(b[r][k], b[r][k], s);
    nn[k] = s;
  }
}

// o = B diag(f) V^T
template <typename T, int N>
__device__ __forceinline__ void bfvt(const T (&b)[N][N], const T (&f)[N], const T (&v)[N][N], T (&o)[N][N]) {
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      T s = T(0);
#pragma unroll
      for (int k = 0; k < N; ++k) s = Num<T>::fma(b[r][k] * f[k], v[c][k], s);
      o[r][c] = s;
    }
}

// theta^2 and (GRAD) psi' of one singular value, from sigma^2
template <typename T, bool GRAD> __device__ __forceinline__ T psi_of(T sigma2, T& dpsi) {
  using Nm = Num<T>;
  const T s2 = Nm::min(T(0.25) * sigma2, T(1));   // value clamp at the cut locus
  const T s = Nm::sqrt(s2);
  const T half = asin_<T>(s);                     // theta / 2
  if (GRAD) {
    const T ratio = s > Nm::tiny() ? half / s : T(1);
    dpsi = (ratio + ratio) * Nm::rsqrt(Nm::max(T(1) - s2, T(kCutFloor)));
  }
  return T(4) * half * half;
}

// d^2 of one pair from D = Y - X; GRAD: dD = d(d^2)/dY (= -d(d^2)/dX)
template <typename T, int N, bool GRAD> __device__ __forceinline__ T so_pair(const T (&D)[N][N], T (&dD)[N][N]) {
  using Nm = Num<T>;
  T b[N][N], v[N][N], nn[N], f[N];
  svd_onesided<T, N, GRAD>(D, b, v, T(16) * Nm::eps() * Nm::eps());
  colnorm2<T, N>(b, nn);
  T val = T(0);
#pragma unroll
  for (int k = 0; k < N; ++k) val += psi_of<T, GRAD>(nn[k], f[k]);
  if constexpr (GRAD) bfvt<T, N>(b, f, v, dD);
  return val;
}

// W = skew(X^T U)
template <typename T, int N> __device__ __forceinline__ void skew_xtu(const T (&x)[N][N], const T (&u)[N][N], T (&w)[N][N]) {
  T g[N][N];
  mat::gram<T, N, N>(x, u, g);
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) w[r][c] = T(0.5) * (g[r][c] - g[c][r]);
}

// log_X(Y) = X skew(X^T D) V diag(psi'_k / 2) V^T   (theta / sin theta per rotation plane), D = Y - X = U S V^T
template <typename T, int N> __device__ __forceinline__ void log_op(const T (&x)[N][N], const T (&y)[N][N], T (&o)[N][N]) {
  using Nm = Num<T>;
  T D[N][N], b[N][N], v[N][N], nn[N], f[N], w[N][N], m[N][N], t[N][N];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) D[r][c] = y[r][c] - x[r][c];
  svd_onesided<T, N, true>(D, b, v, T(16) * Nm::eps() * Nm::eps());
  colnorm2<T, N>(b, nn);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    T d;
    psi_of<T, true>(nn[k], d);
    f[k] = T(0.5) * d;
  }
  mat::vfvt<T, N>(v, f, m);
  skew_xtu<T, N>(x, D, w);
  mat::mulr<T, N, N>(w, m, t);
  mat::mulr<T, N, N>(x, t, o);
}

// exp_X(U) = X (V diag(cos sigma_k) V^T + B diag(sin sigma_k / sigma_k) V^T),  Omega = skew(X^T U), Omega V = B, sigma_k = ||b_k||
template <typename T, int N> __device__ __forceinline__ void exp_op(const T (&x)[N][N], const T (&u)[N][N], T (&o)[N][N]) {
  using Nm = Num<T>;
  T w[N][N], b[N][N], v[N][N], nn[N], fc[N], fs[N], mc[N][N], ms[N][N];
  skew_xtu<T, N>(x, u, w);
  svd_onesided<T, N, true>(w, b, v, T(16) * Nm::eps() * Nm::eps());
  colnorm2<T, N>(b, nn);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const T sg = Nm::sqrt(nn[k]);
    T c;
    const T sn = mat::sincos_<T>(sg, &c);
    fc[k] = c;
    fs[k] = (sg > T(1e-6)) ? sn / sg : T(1) - sg * sg * T(1.0 / 6.0);
  }
  mat::vfvt<T, N>(v, fc, mc);
  bfvt<T, N>(b, fs, v, ms);
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) mc[r][c] += ms[r][c];
  mat::mulr<T, N, N>(x, mc, o);
}

}  // namespace so
}  // namespace mm
