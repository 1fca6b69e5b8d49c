// Fused RiemannianSGD updates of Grassmann / Stiefel points (mm_mat_rsgd_step, mm_mat_rsgd_momentum_step): one thread per
// point, one launch, in the reference's order (optim/rsgd.py:40-82) —
//   rgrad = proju(x, egrad);  clip by max_grad_norm / sqrt(max(||rgrad||_F^2, 1e-8)), at most 1 (base.py:29-33);
//   momentum-free: x_new = step(x, -lr rgrad);
//   heavy ball:    buf = momentum buf + (1 - dampening) rgrad;  x_new = step(x, -lr buf);  buf <- proju(x_new, buf)
//                  (the base class's transport, base.py:65-66), written in place;
// step = the polar or QR retraction, or Grassmann's exp.  The maps are the device functions of mat_map_kernel
// (mat_common.hpp).  x_new may equal x: a thread reads its whole point before it writes.
//
// Fused RiemannianAdam update (mm_mat_radam_step), the same layout, in the reference's order (optim/radam.py:62-98) —
//   rgrad = proju(x, egrad);  gn^2 = max(||rgrad||_F^2, 1e-8), taken BEFORE the clip by min(max_grad_norm / gn, 1);
//   m = beta1 m + (1 - beta1) rgrad;  v = beta2 v + (1 - beta2) gn^2 (ONE scalar per point, stored broadcast over it);
//   x_new = step(x, -alpha m / (sqrt v + eps)),  alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t);  m <- proju(x_new, m) in place.
// The step counter lives in device memory and is advanced by the last block (adam.hpp).  A point with a zero gradient and a
// zero first moment gets the zero tangent: exp gives x back bit for bit (the eigenvectors of the zero matrix are the identity,
// cos 0 = 1), the retractions give polar(x) / Q(x), which is x to rounding, as the reference's own maps do.
#include <hip/hip_runtime.h>

#include "../../include/mm_manifolds.h"
#include "adam.hpp"
#include "mat_common.hpp"
#include "smallmat.hpp"

namespace mm {
namespace mat {

// (x and xnew are deliberately not __restrict__: the update may be done in place, xnew == x)
template <typename T, int NP, int P, bool MOMENTUM>
__global__ __launch_bounds__(64) void mat_rsgd_kernel(int kind, int op, const T* x, const T* __restrict__ eg, T* __restrict__ buf,
                                                      int64_t cnt, int N, T lr, T momentum, T dampening, T max_grad_norm,
                                                      T* xnew) {
  using Nm = Num<T>;
  const int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in = p0 < cnt;
  const int64_t p = in ? p0 : 0;
  T xa[NP][P], u[NP][P], r[NP][P], o[NP][P];
  load<T, NP, P>(x + p * N * P, N, xa);
  load<T, NP, P>(eg + p * N * P, N, u);
  proju_op<T, NP, P>(kind, xa, u, r);
  T clip = T(1);
  if (max_grad_norm > T(0)) {
    T sq = T(0);
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int c = 0; c < P; ++c) sq = Nm::fma(r[i][c], r[i][c], sq);
    clip = Nm::min(max_grad_norm / Nm::sqrt(Nm::max(sq, T(kEps))), T(1));
  }
  if (MOMENTUM) load<T, NP, P>(buf + p * N * P, N, o);
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int c = 0; c < P; ++c) {
      if (MOMENTUM) r[i][c] = Nm::fma(momentum, o[i][c], (T(1) - dampening) * (r[i][c] * clip));
      else r[i][c] *= clip;
      u[i][c] = -lr * r[i][c];
    }
  if (op == MM_MAT_EXP) exp_op<T, NP, P>(xa, u, o);
  else retr_op<T, NP, P>(kind, op, N, xa, u, o);
  if (in) store<T, NP, P>(xnew + p * N * P, N, o);
  if (MOMENTUM) {
    proju_op<T, NP, P>(kind, o, r, u);
    if (in) store<T, NP, P>(buf + p * N * P, N, u);
  }
}

template <bool MOMENTUM>
int rsgd_launch(int dtype, int kind, int retr, const void* x, const void* egrad, void* buf, int64_t cnt, int N, int p, double lr,
                double momentum, double dampening, double max_grad_norm, int exact, void* x_new, mm_stream_t stream) {
  if (cnt < 0 || N < 1 || p < 1 || p > N || (kind != MM_GRASSMANN && kind != MM_STIEFEL) ||
      (retr != MM_MAT_RETR_SVD && retr != MM_MAT_RETR_QR) || (dtype != MM_F32 && dtype != MM_F64))
    return MM_ERR_ARG;
  if (cnt > 0 && (!x || !egrad || !x_new || (MOMENTUM && !buf))) return MM_ERR_ARG;
  if (kind == MM_STIEFEL && exact) return MM_ERR_UNSUPPORTED;  // stiefel.py:59-60, as mm_mat_map
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned nb = unsigned((cnt + 63) / 64);
  const int op = exact ? int(MM_MAT_EXP) : retr;
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    mat_rsgd_kernel<T, NP, P, MOMENTUM><<<dim3(nb), dim3(64), 0, st>>>(kind, op, static_cast<const T*>(x),
        static_cast<const T*>(egrad), static_cast<T*>(buf), cnt, N, T(lr), T(momentum), T(dampening), T(max_grad_norm),
        static_cast<T*>(x_new));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

// The step's coefficients are formed by one thread per workgroup and handed over through LDS: the two fp64 pow() stay out of
// the per-point code.  1 - beta is formed in fp64 from the caller's fp64 betas, as the reference forms it on the host
// (1 - float(0.999) is 1e-6 off 0.001).
template <typename T, int NP, int P>
__global__ __launch_bounds__(64) void mat_radam_kernel(int kind, int op, const T* x, const T* __restrict__ eg, T* __restrict__ exp_avg,
                                                       T* __restrict__ exp_avg_sq, int64_t cnt, int N, AdamArgs<T> a,
                                                       double beta1_64, double beta2_64, T* xnew) {
  using Nm = Num<T>;
  __shared__ T coef[4];
  if (threadIdx.x == 0) {
    adam_coeffs(a, coef[0], coef[1]);
    coef[2] = T(a.nc ? 1.0 / *a.step : 1.0 - beta2_64);
    coef[3] = T(1.0 - beta1_64);
  }
  __syncthreads();
  const T beta2 = coef[0], alpha = coef[1], omb2 = coef[2], omb1 = coef[3];
  const int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in = p0 < cnt;
  const int64_t p = in ? p0 : 0;
  T xa[NP][P], u[NP][P], r[NP][P], o[NP][P];
  load<T, NP, P>(x + p * N * P, N, xa);
  load<T, NP, P>(eg + p * N * P, N, u);
  proju_op<T, NP, P>(kind, xa, u, r);
  T sq = T(0);
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int c = 0; c < P; ++c) sq = Nm::fma(r[i][c], r[i][c], sq);
  const T gn2 = Nm::max(sq, T(kEps));   // base.py:29-33; the second moment sees it BEFORE the clip
  const T clip = a.max_grad_norm > T(0) ? Nm::min(a.max_grad_norm / Nm::sqrt(gn2), T(1)) : T(1);
  const T v = Nm::fma(beta2, exp_avg_sq[p * N * P], omb2 * gn2);
  const T s = -alpha / (Nm::sqrt(v) + a.eps);
  load<T, NP, P>(exp_avg + p * N * P, N, o);
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int c = 0; c < P; ++c) {
      r[i][c] = Nm::fma(a.beta1, o[i][c], omb1 * (r[i][c] * clip));
      u[i][c] = r[i][c] * s;
    }
  if (op == MM_MAT_EXP) exp_op<T, NP, P>(xa, u, o);
  else retr_op<T, NP, P>(kind, op, N, xa, u, o);
  if (in) store<T, NP, P>(xnew + p * N * P, N, o);
  proju_op<T, NP, P>(kind, o, r, u);
  if (in) {
    store<T, NP, P>(exp_avg + p * N * P, N, u);
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int c = 0; c < P; ++c)
        if (i < N) exp_avg_sq[p * N * P + i * P + c] = v;
  }
  adam_tick(a.step, a.ticket, gridDim.x);
}

}  // namespace mat
}  // namespace mm

using namespace mm::mat;

extern "C" {

int mm_mat_rsgd_step(int dtype, int kind, int retr_op, const void* x, const void* egrad, int64_t cnt, int N, int p, double lr,
                     double max_grad_norm, int exact, void* x_new, mm_stream_t stream) {
  return rsgd_launch<false>(dtype, kind, retr_op, x, egrad, nullptr, cnt, N, p, lr, 0.0, 0.0, max_grad_norm, exact, x_new, stream);
}

int mm_mat_rsgd_momentum_step(int dtype, int kind, int retr_op, const void* x, const void* egrad, void* momentum_buffer,
                              int64_t cnt, int N, int p, double lr, double momentum, double dampening, double max_grad_norm,
                              int exact, void* x_new, mm_stream_t stream) {
  return rsgd_launch<true>(dtype, kind, retr_op, x, egrad, momentum_buffer, cnt, N, p, lr, momentum, dampening, max_grad_norm,
                           exact, x_new, stream);
}

int mm_mat_radam_step(int dtype, int kind, int retr_op, const void* x, const void* egrad, void* exp_avg, void* exp_avg_sq,
                      double* step, unsigned* ticket, int64_t cnt, int N, int p, double lr, double beta1, double beta2, int nc,
                      double eps, double max_grad_norm, int exact, void* x_new, mm_stream_t stream) {
  if (cnt < 0 || N < 1 || p < 1 || p > N || (kind != MM_GRASSMANN && kind != MM_STIEFEL) ||
      (retr_op != MM_MAT_RETR_SVD && retr_op != MM_MAT_RETR_QR) || (dtype != MM_F32 && dtype != MM_F64) || !step || !ticket)
    return MM_ERR_ARG;
  if (cnt > 0 && (!x || !egrad || !exp_avg || !exp_avg_sq || !x_new)) return MM_ERR_ARG;
  if (kind == MM_STIEFEL && exact) return MM_ERR_UNSUPPORTED;  // stiefel.py:59-60, as mm_mat_rsgd_step
  if (N > 9 || p > 4 || cnt > (int64_t(1) << 31) * 64 - 1) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned nb = unsigned((cnt + 63) / 64);
  // Gr(N,N) is a single point and its tangent space is {0}: the Riemannian gradient there is the rounding of the frame, Adam
  // normalises that noise to size lr, and it is as much normal as tangent.  exp keeps x^T x only along tangents (three steps of
  // the reference's own fp64 arithmetic leave x^T x - I at 2e-2), so at N = p `exact` moves with the instance's retraction,
  // which agrees with exp to first order and returns an orthonormal frame.
  const int op = (exact && N > p) ? int(MM_MAT_EXP) : retr_op;
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    const mm::AdamArgs<T> a{T(lr), T(beta1), T(beta2), T(eps), T(max_grad_norm), nc, exact, step, ticket};
    mat_radam_kernel<T, NP, P><<<dim3(nb), dim3(64), 0, st>>>(kind, op, static_cast<const T*>(x), static_cast<const T*>(egrad),
        static_cast<T*>(exp_avg), static_cast<T*>(exp_avg_sq), cnt, N, a, beta1, beta2, static_cast<T*>(x_new));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

}  // extern "C"
