// Device functions of the Grassmann / Stiefel kernels shared by mat.hip (per-point maps, dist, pdist), mat_step.hip (fused
// optimizer steps) and grass_loss.hip (fused objective): one small N x p matrix per lane, in registers.
// Points are stored [cnt][N][p] row-major; N is padded to NP in {4,6,9} (zero rows change nothing), p in {1,2,3,4} is a
// template parameter.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mm_manifolds.h"
#include "launch.hpp"
#include "smallmat.hpp"

namespace mm {
namespace mat {

constexpr double kEps = 1e-8;

template <typename T, int NP, int P> __device__ __forceinline__ void load(const T* __restrict__ p, int N, T (&a)[NP][P]) {
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) a[r][c] = (r < N) ? p[r * P + c] : T(0);
}
template <typename T, int NP, int P> __device__ __forceinline__ void store(T* __restrict__ p, int N, const T (&a)[NP][P]) {
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c)
      if (r < N) p[r * P + c] = a[r][c];
}

// G = A^T B (p x p)
template <typename T, int NP, int P>
__device__ __forceinline__ void gram(const T (&a)[NP][P], const T (&b)[NP][P], T (&g)[P][P]) {
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      T s = T(0);
#pragma unroll
      for (int r = 0; r < NP; ++r) s = Num<T>::fma(a[r][i], b[r][j], s);
      g[i][j] = s;
    }
}

// out = A * M (N x p times p x p)
template <typename T, int NP, int P>
__device__ __forceinline__ void mulr(const T (&a)[NP][P], const T (&m)[P][P], T (&o)[NP][P]) {
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) {
      T s = T(0);
#pragma unroll
      for (int k = 0; k < P; ++k) s = Num<T>::fma(a[r][k], m[k][c], s);
      o[r][c] = s;
    }
}

// symmetric p x p eigen-decomposition S = V diag(w) V^T
template <typename T, int P> __device__ __forceinline__ void symeig(const T (&s)[P][P], T (&w)[P], T (&v)[P][P]) {
  T a[Packed<P>::NP];
#pragma unroll
  for (int r = 0; r < P; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) a[pidx(r, c)] = T(0.5) * (s[r][c] + s[c][r]);
  jacobi_eig<T, P, true>(a, v);
#pragma unroll
  for (int k = 0; k < P; ++k) w[k] = a[pidx(k, k)];
}

// M = V diag(f) V^T
template <typename T, int P> __device__ __forceinline__ void vfvt(const T (&v)[P][P], const T (&f)[P], T (&m)[P][P]) {
#pragma unroll
  for (int r = 0; r < P; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) {
      T s = T(0);
#pragma unroll
      for (int k = 0; k < P; ++k) s = Num<T>::fma(v[r][k] * f[k], v[c][k], s);
      m[r][c] = s;
    }
}

// polar factor U V^T of Y = U S V^T   (grassmann.py:76-80, stiefel.py:66-69)
template <typename T, int NP, int P> __device__ __forceinline__ void polar(const T (&y)[NP][P], T (&q)[NP][P]) {
  T s[P][P], w[P], v[P][P], m[P][P], f[P];
  gram<T, NP, P>(y, y, s);
  symeig<T, P>(s, w, v);
#pragma unroll
  for (int k = 0; k < P; ++k) f[k] = Num<T>::rsqrt(Num<T>::max(w[k], Num<T>::tiny()));
  vfvt<T, P>(v, f, m);
  mulr<T, NP, P>(y, m, q);
}

// Q of the Householder QR of Y, LAPACK (geqrf/orgqr) sign convention: R_kk = -sgn(a_kk) ||.||.
// SIGNFIX multiplies column k by sgn(R_kk) (stiefel.py:47-50).
template <typename T, int NP, int P, bool SIGNFIX>
__device__ __forceinline__ void qr_q(const T (&y)[NP][P], int N, T (&q)[NP][P]) {
  T a[NP][P], tau[P], rs[P];
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) a[r][c] = y[r][c];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    T xn = T(0);
#pragma unroll
    for (int r = k + 1; r < NP; ++r) xn = Num<T>::fma(a[r][k], a[r][k], xn);
    const T alpha = a[k][k];
    T beta = -Num<T>::copysign(Num<T>::sqrt(Num<T>::fma(alpha, alpha, xn)), alpha);
    const bool trivial = !(xn > T(0));  // LAPACK: H = I when the sub-column is zero
    tau[k] = trivial ? T(0) : (beta - alpha) / beta;
    const T scal = trivial ? T(0) : T(1) / (alpha - beta);
    rs[k] = trivial ? alpha : beta;
#pragma unroll
    for (int r = k + 1; r < NP; ++r) a[r][k] *= scal;  // v below the diagonal (v_k = 1)
#pragma unroll
    for (int c = k + 1; c < P; ++c) {                  // apply H to the trailing columns
      T d = a[k][c];
#pragma unroll
      for (int r = k + 1; r < NP; ++r) d = Num<T>::fma(a[r][k], a[r][c], d);
      d *= tau[k];
      a[k][c] -= d;
#pragma unroll
      for (int r = k + 1; r < NP; ++r) a[r][c] = Num<T>::fma(-d, a[r][k], a[r][c]);
    }
  }
  // Q = H_0 ... H_{p-1} [I_p; 0]
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) q[r][c] = (r == c) ? T(1) : T(0);
#pragma unroll
  for (int k = P - 1; k >= 0; --k) {
#pragma unroll
    for (int c = 0; c < P; ++c) {
      T d = q[k][c];
#pragma unroll
      for (int r = k + 1; r < NP; ++r) d = Num<T>::fma(a[r][k], q[r][c], d);
      d *= tau[k];
      q[k][c] -= d;
#pragma unroll
      for (int r = k + 1; r < NP; ++r) q[r][c] = Num<T>::fma(-d, a[r][k], q[r][c]);
    }
  }
  if (SIGNFIX) {
#pragma unroll
    for (int c = 0; c < P; ++c) {
      const T sg = (rs[c] > T(0)) ? T(1) : ((rs[c] < T(0)) ? T(-1) : T(0));
#pragma unroll
      for (int r = 0; r < NP; ++r) q[r][c] *= sg;
    }
  }
  (void)N;
}

// inverse of a p x p matrix (Gauss-Jordan, partial pivoting)
template <typename T, int P> __device__ __forceinline__ void inv_pp(const T (&m)[P][P], T (&inv)[P][P]) {
  T a[P][2 * P];
#pragma unroll
  for (int r = 0; r < P; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) { a[r][c] = m[r][c]; a[r][P + c] = (r == c) ? T(1) : T(0); }
#pragma unroll
  for (int k = 0; k < P; ++k) {
#pragma unroll
    for (int r = k + 1; r < P; ++r) {  // bring the larger pivot up (select-swap: no dynamic indexing)
      const bool sw = Num<T>::abs(a[r][k]) > Num<T>::abs(a[k][k]);
#pragma unroll
      for (int c = 0; c < 2 * P; ++c) { const T x = a[k][c], y = a[r][c]; a[k][c] = sw ? y : x; a[r][c] = sw ? x : y; }
    }
    const T ip = T(1) / a[k][k];
#pragma unroll
    for (int c = 0; c < 2 * P; ++c) a[k][c] *= ip;
#pragma unroll
    for (int r = 0; r < P; ++r) {
      if (r == k) continue;
      const T f = a[r][k];
#pragma unroll
      for (int c = 0; c < 2 * P; ++c) a[r][c] = Num<T>::fma(-f, a[k][c], a[r][c]);
    }
  }
#pragma unroll
  for (int r = 0; r < P; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) inv[r][c] = a[r][P + c];
}

// One-sided Jacobi (Hestenes) on the columns of an NP x P matrix, in place: on exit b = B V has mutually orthogonal columns,
// i.e. B = U diag(sigma) V^T with sigma_k = ||b_k|| and u_k = b_k / sigma_k (svd_onesided of smallmat.hpp with NP rows; the
// same rotation, the same wave-uniform sweep loop).  log_x(y) needs it: B = (y - x x^T y)(x^T y)^-1 holds the tangents of the
// principal angles, 1e3 - 1e4 next to O(1) for nearly orthogonal subspaces, and through the eigenvalues of B^T B everything
// below sqrt(eps) sigma_max is rounding noise (0.2 absolute in fp32, 1e-9 in fp64 at Gr(8,4); the reference's own fp32: 5e-4).
template <typename T, int NP, int P> __device__ __forceinline__ void svd_onesided_tall(T (&b)[NP][P], T (&v)[P][P], T tol2) {
  using N = Num<T>;
#pragma unroll
  for (int r = 0; r < P; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) v[r][c] = (r == c) ? T(1) : T(0);
  if constexpr (P == 1) return;
  for (int sweep = 0; sweep < N::kMaxSweeps + 4; ++sweep) {
    bool active = false;
#pragma unroll
    for (int p = 0; p < P - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < P; ++q) {
        T app = T(0), aqq = T(0), apq = T(0);
#pragma unroll
        for (int r = 0; r < NP; ++r) {
          app = N::fma(b[r][p], b[r][p], app);
          aqq = N::fma(b[r][q], b[r][q], aqq);
          apq = N::fma(b[r][p], b[r][q], apq);
        }
        active = active || (apq * apq > tol2 * (app * aqq));
        const T h = aqq - app;
        const T ah = N::abs(h) + T(1e-15);
        const T sa_ = (h < T(0)) ? -apq : apq;
        const T sa2 = sa_ + sa_;
        const T rr = N::rsqrt(N::fma(ah, ah, sa2 * sa2));
        const T x = N::fma(ah * rr, T(0.5), T(0.5));  // cos^2 t
        const T ci = N::rsqrt(x);
        const T c = x * ci;
        const T sn = (sa_ * rr) * ci;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
          const T bp = b[r][p], bq = b[r][q];
          b[r][p] = N::fma(c, bp, -sn * bq);
          b[r][q] = N::fma(sn, bp, c * bq);
        }
#pragma unroll
        for (int r = 0; r < P; ++r) {
          const T vp = v[r][p], vq = v[r][q];
          v[r][p] = N::fma(c, vp, -sn * vq);
          v[r][q] = N::fma(sn, vp, c * vq);
        }
      }
    }
    if (!__any(active)) break;
  }
}

template <typename T> __device__ __forceinline__ T acos_(T c);
template <> __device__ __forceinline__ float acos_<float>(float c) { return ::acosf(c); }
template <> __device__ __forceinline__ double acos_<double>(double c) { return ::acos(c); }
template <typename T> __device__ __forceinline__ T sincos_(T x, T* c);
template <> __device__ __forceinline__ float sincos_<float>(float x, float* c) { *c = ::cosf(x); return ::sinf(x); }
template <> __device__ __forceinline__ double sincos_<double>(double x, double* c) { *c = ::cos(x); return ::sin(x); }
template <typename T> __device__ __forceinline__ T atan_(T x);
template <> __device__ __forceinline__ float atan_<float>(float x) { return ::atanf(x); }
template <> __device__ __forceinline__ double atan_<double>(double x) { return ::atan(x); }

// Grassmann distance of one pair from G = x^T y:  sum_k acos^2(sigma_k)  (grassmann.py:91-96).
// Returns the value; if WANT_GRAD, dG = d(value)/dG = G V diag(f'(s)/s) V^T with
// f = acos^2 (the reference's NaN at sigma = 1, acos'(1), is replaced by the finite limit -2).
template <typename T> __device__ __forceinline__ T dacos2(T sc, T th) {
  // d acos^2(s)/ds = -2 acos(s)/sqrt(1-s^2); the 0/0 at s = 1 is replaced by its limit -2
  const T om = Num<T>::fma(-sc, sc, T(1));
  return T(-2) * ((om > T(1e-12)) ? th * Num<T>::rsqrt(om) : T(1));
}

template <typename T, int P, bool WANT_GRAD>
__device__ __forceinline__ T grass_pair(const T (&g)[P][P], T (&dg)[P][P]) {
  using N = Num<T>;
  if constexpr (P == 2) {
    // the reference's closed form for 2x2 singular values INCLUDING its eps clamps
    // (linalg/fast.py:138-159; they bias d^2 by ~1e-4 at its own init, so they are part of
    // the specification): S2 = (s1^2-s2^2)^2 >= eps, s_k^2 = (S1 +- sqrt S2)/2 >= eps.
    const T a = g[0][0], b = g[0][1], c = g[1][0], d = g[1][1];
    const T S1 = a * a + b * b + c * c + d * d;
    const T Dd = a * a + b * b - c * c - d * d, E = a * c + b * d;
    const T R2 = N::fma(Dd, Dd, T(4) * E * E);
    const T R = N::sqrt(N::max(R2, T(kEps)));
    const T s1 = N::sqrt(N::max(T(0.5) * (S1 + R), T(kEps)));
    // (S1 - R)/2 = (S1^2 - R^2) / (2 (S1 + R)) and S1^2 - R^2 = 4 det^2 while the clamp on S2 is idle: the same number without
    // the cancellation, which costs eps S1 / sigma_2 of sigma_2 next to orthogonal subspaces (fp32, Gr(9,2): 2.4e-4 of d^2, 16 x
    // the reference's own fp32); under the clamp the reference's biased value is kept as it is
    const T det = N::fma(a, d, -b * c);
    const T s2 = N::sqrt(N::max(R2 >= T(kEps) ? (T(2) * det * det) / (S1 + R) : T(0.5) * (S1 - R), T(kEps)));
    const T c1 = N::min(s1, T(1 - 1e-16)), c2 = N::min(s2, T(1 - 1e-16));
    const T t1 = acos_<T>(c1), t2 = acos_<T>(c2);
    if (WANT_GRAD) {
      // value clamps are gradient-transparent: d s_k = d(s_k^2)/(2 s_k), d s_{1,2}^2 = (dS1 +- dR)/2,
      // dR = (2 D dD + 8 E dE)/(2R)
      const T a1 = dacos2<T>(c1, t1) / (T(4) * s1), a2 = dacos2<T>(c2, t2) / (T(4) * s2);
      const T ps = a1 + a2, pr = (a1 - a2) / R;
      dg[0][0] = ps * (a + a) + pr * (Dd * (a + a) + T(4) * E * c);
      dg[0][1] = ps * (b + b) + pr * (Dd * (b + b) + T(4) * E * d);
      dg[1][0] = ps * (c + c) + pr * (-Dd * (c + c) + T(4) * E * a);
      dg[1][1] = ps * (d + d) + pr * (-Dd * (d + d) + T(4) * E * b);
    }
    return N::fma(t1, t1, t2 * t2);
  } else {
    // singular values from a one-sided Jacobi on G itself (not from the eigenvalues of G^T G: see svd_onesided)
    T b[P][P], v[P][P], nn[P];
    // (4 eps: with eps itself the test sits at the rounding of the inner product and some matrices never pass it; emulated
    // in fp32 / fp64 on 400 matrices with cosines from 1 - 1e-8 to 1e-9: at most 6 sweeps, singular values to 4e-7 / 1e-15)
    svd_onesided<T, P, true>(g, b, v, T(16) * N::eps() * N::eps());
    // sigma_k^2: the column norm ||b_k||^2 for the small ones (what the one-sided method is for); for cosines next to 1
    // (small angles: the reference's own initialisation) the Rayleigh quotient v_k^T (G^T G) v_k / v_k^T v_k — the rotations
    // leave ~6 eps of norm drift in b and v, which the quotient cancels and which acos would amplify ~100 x at sigma ~ 1 - 1e-4
    // (emulated, angles ~1e-2: d^2 to 6.7e-3 from the column norms, 2.0e-3 from the quotient, 1.9e-3 through eig(G^T G))
    T sgram[P][P];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int j = 0; j < P; ++j) {
        T acc = T(0);
#pragma unroll
        for (int k = 0; k < P; ++k) acc = N::fma(g[k][i], g[k][j], acc);
        sgram[i][j] = acc;
      }
    T val = T(0), f[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      nn[k] = T(0);
      T num = T(0), den = T(0);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        nn[k] = N::fma(b[i][k], b[i][k], nn[k]);
        T sv = T(0);
#pragma unroll
        for (int j = 0; j < P; ++j) sv = N::fma(sgram[i][j], v[j][k], sv);
        num = N::fma(v[i][k], sv, num);
        den = N::fma(v[i][k], v[i][k], den);
      }
      const T s2 = nn[k] > T(0.25) ? num / den : nn[k];
      const T sg = N::sqrt(N::max(s2, T(0)));
      const T sc = N::min(sg, T(1 - 1e-16));  // value clamp (grassmann.py:94)
      const T th = acos_<T>(sc);
      val = N::fma(th, th, val);
      if (WANT_GRAD) f[k] = dacos2<T>(sc, th);
    }
    if (WANT_GRAD) {
      // dG = U diag(f') V^T with the left vectors u_k = b_k / ||b_k|| (b = G V).  Normalising by the ACTUAL norm keeps
      // every term bounded when a principal angle is ~pi/2 (sigma_k ~ 0) — tests/fuzz_misc.py once found 1e25-sized
      // gradients in fp32 with a division by sqrt(eigenvalue of G^T G).
#pragma unroll
      for (int k = 0; k < P; ++k) f[k] = f[k] * N::rsqrt(N::max(nn[k], T(1e-30)));
#pragma unroll
      for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
          T acc = T(0);
#pragma unroll
          for (int k = 0; k < P; ++k) acc = N::fma(b[i][k] * f[k], v[j][k], acc);
          dg[i][j] = acc;
        }
    }
    return val;
  }
}

// ------------------------------------------------------------ per-point maps (mat_map_kernel, the fused optimizer steps)
// u - x x^T u (grassmann.py:49-53) / u - x sym(x^T u) (stiefel.py:40-45)
template <typename T, int NP, int P>
__device__ __forceinline__ void proju_op(int kind, const T (&xa)[NP][P], const T (&ua)[NP][P], T (&o)[NP][P]) {
  T g[P][P];
  gram<T, NP, P>(xa, ua, g);  // x^T u
  if (kind == MM_STIEFEL) {   // u - x sym(x^T u)   stiefel.py:40-45
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int j = i + 1; j < P; ++j) { const T h = T(0.5) * (g[i][j] + g[j][i]); g[i][j] = h; g[j][i] = h; }
  }                           // else u - x x^T u   grassmann.py:49-53
  mulr<T, NP, P>(xa, g, o);
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) o[r][c] = ua[r][c] - o[r][c];
}

// retraction of x + u: polar factor (MM_MAT_RETR_SVD) or Q of QR (MM_MAT_RETR_QR; Stiefel sign-fixed)
template <typename T, int NP, int P>
__device__ __forceinline__ void retr_op(int kind, int op, int N, const T (&xa)[NP][P], const T (&ua)[NP][P], T (&o)[NP][P]) {
  T y[NP][P];
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) y[r][c] = xa[r][c] + ua[r][c];
  if (op == MM_MAT_RETR_SVD) {
    polar<T, NP, P>(y, o);
    // St(n, n) is the orthogonal group, where the points carry a metric (so.hip) and their orthogonality is all there is to
    // being on the manifold: the polar factor comes out with o^T o - I ~ 17 eps (v_rsq, the eigenvalues' rounding and the
    // drift of the Jacobi vectors, each twice), one Newton-Schulz step o (3 I - o^T o) / 2 squares that and leaves its own
    // rounding (~3 eps).  o = y M with M symmetric positive definite, so the step moves o towards polar(y) itself.
    if constexpr (NP == 4) {
      if (kind == MM_STIEFEL && N == P) {
        T g[P][P], t[NP][P];
        gram<T, NP, P>(o, o, g);
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int j = 0; j < P; ++j) g[i][j] = (i == j ? T(1.5) : T(0)) - T(0.5) * g[i][j];
        mulr<T, NP, P>(o, g, t);
#pragma unroll
        for (int r = 0; r < NP; ++r)
#pragma unroll
          for (int c = 0; c < P; ++c) o[r][c] = t[r][c];
      }
    }
  } else if (kind == MM_STIEFEL) qr_q<T, NP, P, true>(y, N, o);
  else qr_q<T, NP, P, false>(y, N, o);
}

// x V cos(S) V^T + U sin(S) V^T, u = U S V^T  (grassmann.py:63-69)
template <typename T, int NP, int P>
__device__ __forceinline__ void exp_op(const T (&xa)[NP][P], const T (&ua)[NP][P], T (&o)[NP][P]) {
  using Nm = Num<T>;
  T s[P][P], w[P], v[P][P], fc[P], fs[P], mc[P][P], ms[P][P], t1[NP][P], t2[NP][P];
  gram<T, NP, P>(ua, ua, s);
  symeig<T, P>(s, w, v);
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const T sg = Nm::sqrt(Nm::max(w[k], T(0)));
    T c;
    const T sn = sincos_<T>(sg, &c);
    fc[k] = c;
    fs[k] = (sg > T(1e-6)) ? sn / sg : T(1) - sg * sg * T(1.0 / 6.0);
  }
  vfvt<T, P>(v, fc, mc);
  vfvt<T, P>(v, fs, ms);
  mulr<T, NP, P>(xa, mc, t1);
  mulr<T, NP, P>(ua, ms, t2);
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) o[r][c] = t1[r][c] + t2[r][c];
}

constexpr int kBlk = 128;

constexpr int pad_rows(int N) { return N <= 4 ? 4 : N <= 6 ? 6 : 9; }

#define MMM_DISPATCH_NP_P(N, p, ...)                                            \
  switch (pad_rows(N) * 10 + (p)) {                                             \
    case 41: { constexpr int NP = 4, P = 1; __VA_ARGS__ }                        \
    case 42: { constexpr int NP = 4, P = 2; __VA_ARGS__ }                        \
    case 43: { constexpr int NP = 4, P = 3; __VA_ARGS__ }                        \
    case 44: { constexpr int NP = 4, P = 4; __VA_ARGS__ }                        \
    case 61: { constexpr int NP = 6, P = 1; __VA_ARGS__ }                        \
    case 62: { constexpr int NP = 6, P = 2; __VA_ARGS__ }                        \
    case 63: { constexpr int NP = 6, P = 3; __VA_ARGS__ }                        \
    case 64: { constexpr int NP = 6, P = 4; __VA_ARGS__ }                        \
    case 91: { constexpr int NP = 9, P = 1; __VA_ARGS__ }                        \
    case 92: { constexpr int NP = 9, P = 2; __VA_ARGS__ }                        \
    case 93: { constexpr int NP = 9, P = 3; __VA_ARGS__ }                        \
    case 94: { constexpr int NP = 9, P = 4; __VA_ARGS__ }                        \
    default: return MM_ERR_UNSUPPORTED;                                         \
  }

#define MMM_DISPATCH_T(dtype, ...)                               \
  if ((dtype) == MM_F32) { using T = float; __VA_ARGS__ }        \
  else if ((dtype) == MM_F64) { using T = double; __VA_ARGS__ }  \
  else return MM_ERR_ARG;

}  // namespace mat
}  // namespace mm
