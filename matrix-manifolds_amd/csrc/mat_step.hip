// Fused RiemannianSGD updates of Grassmann / Stiefel points (mm_mat_rsgd_step, mm_mat_rsgd_momentum_step): one thread per
// point, one launch, in the reference's order (optim/rsgd.py:40-82) —
//   rgrad = proju(x, egrad);  clip by max_grad_norm / sqrt(max(||rgrad||_F^2, 1e-8)), at most 1 (base.py:29-33);
//   momentum-free: x_new = step(x, -lr rgrad);
//   heavy ball:    buf = momentum buf + (1 - dampening) rgrad;  x_new = step(x, -lr buf);  buf <- proju(x_new, buf)
//                  (the base class's transport, base.py:65-66), written in place;
// step = the polar or QR retraction, or Grassmann's exp.  The maps are the device functions of mat_map_kernel
// (mat_common.hpp).  x_new may equal x: a thread reads its whole point before it writes.
#include <hip/hip_runtime.h>

#include "../../include/mm_manifolds.h"
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
    MMM_CHECK(); return MM_OK; }))
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

}  // extern "C"
