// Grassmann Gr(N,p) and Stiefel St(N,p): projections, retractions, exp/log, the
// principal-angle distance and its gradient — one small N x p matrix per lane, in registers.
//
// Reference arithmetic: graphembed/graphembed/manifolds/grassmann.py:49-96 and
// stiefel.py:40-69, where every QR / SVD is shipped to the CPU (linalg/torch_batch.py:94-121).
// Here:  Q of QR    = Householder with LAPACK's sign convention (so Q matches torch.qr),
//        polar U V^T = Y (Y^T Y)^-1/2           via a p x p Jacobi eigensolve,
//        U f(S) V^T of a thin SVD = Y V f(s)/s V^T  with (s^2, V) = eig(Y^T Y)  (exp; log: one-sided Jacobi on B itself),
//        singular values of x^T y             = sqrt eig((x^T y)^T (x^T y)).
// Points are stored [cnt][N][p] row-major; N is padded to NP in {4,6,9} (zero rows change
// nothing), p in {1,2,3,4} is a template parameter.  The device functions live in mat_common.hpp
// (shared with mat_step.hip and grass_loss.hip).
#include <hip/hip_runtime.h>

#include "../../include/mm_manifolds.h"
#include "prof.hpp"
#include <type_traits>

#include "clear.hpp"
#include "mat_common.hpp"
#include "smallmat.hpp"

namespace mm {
namespace mat {

// ------------------------------------------------------------ per-point maps
template <typename T, int NP, int P>
__global__ void mat_map_kernel(int kind, int op, const T* __restrict__ x, const T* __restrict__ u, int64_t cnt, int N,
                               T* __restrict__ out) {
  using Nm = Num<T>;
  const int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in = p0 < cnt;
  const int64_t p = in ? p0 : 0;
  T xa[NP][P], ua[NP][P], o[NP][P];
  load<T, NP, P>(x + p * N * P, N, xa);
  if (op != MM_MAT_PROJX) load<T, NP, P>(u + p * N * P, N, ua);
  if (op == MM_MAT_PROJU) {
    proju_op<T, NP, P>(kind, xa, ua, o);
  } else if (op == MM_MAT_PROJX) {  // grassmann.py:55-61 / stiefel.py:47-57
    if (kind == MM_STIEFEL) qr_q<T, NP, P, true>(xa, N, o); else qr_q<T, NP, P, false>(xa, N, o);
  } else if (op == MM_MAT_RETR_SVD || op == MM_MAT_RETR_QR) {
    retr_op<T, NP, P>(kind, op, N, xa, ua, o);
  } else if (op == MM_MAT_EXP) {
    exp_op<T, NP, P>(xa, ua, o);
  } else {  // MM_MAT_LOG: log_x(y), y in `u`  (grassmann.py:82-89)
    T ytx[P][P], inv[P][P], b[NP][P];
    gram<T, NP, P>(ua, xa, ytx);  // y^T x
    inv_pp<T, P>(ytx, inv);
    // B = (y - x (y^T x)^T) (y^T x)^-T     (N x p);  B^T = solve(ytx, y^T - ytx x^T)
    T a[NP][P];
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c) {
        T acc = ua[r][c];
#pragma unroll
        for (int k = 0; k < P; ++k) acc = Nm::fma(-xa[r][k], ytx[c][k], acc);
        a[r][c] = acc;
      }
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c) {
        T acc = T(0);
#pragma unroll
        for (int k = 0; k < P; ++k) acc = Nm::fma(a[r][k], inv[c][k], acc);
        b[r][c] = acc;
      }
    // U atan(S) V^T of B = U S V^T = (B V) diag(atan(s) / s) V^T with the singular values from a one-sided Jacobi on B itself
    // (not from the eigenvalues of B^T B: see svd_onesided_tall)
    T v[P][P], f[P];
    svd_onesided_tall<T, NP, P>(b, v, T(16) * Nm::eps() * Nm::eps());
#pragma unroll
    for (int k = 0; k < P; ++k) {
      T nn = T(0);
#pragma unroll
      for (int r = 0; r < NP; ++r) nn = Nm::fma(b[r][k], b[r][k], nn);
      const T sg = Nm::sqrt(nn);
      f[k] = (sg > T(1e-6)) ? atan_<T>(sg) / sg : T(1) - sg * sg * T(1.0 / 3.0);
    }
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c) {
        T acc = T(0);
#pragma unroll
        for (int k = 0; k < P; ++k) acc = Nm::fma(b[r][k] * f[k], v[c][k], acc);
        o[r][c] = acc;
      }
  }
  if (in) store<T, NP, P>(out + p * N * P, N, o);
}

// ------------------------------------------------------- element-wise dist
template <typename T, int NP, int P>
__global__ void grass_dist_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ g,
                                  int64_t cnt, int N, int squared, T* __restrict__ out, T* __restrict__ gx,
                                  T* __restrict__ gy) {
  using Nm = Num<T>;
  const int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in = p0 < cnt;
  const int64_t p = in ? p0 : 0;
  T xa[NP][P], ya[NP][P], gm[P][P], dg[P][P];
  load<T, NP, P>(x + p * N * P, N, xa);
  load<T, NP, P>(y + p * N * P, N, ya);
  gram<T, NP, P>(xa, ya, gm);
  if (gx == nullptr) {
    const T v = grass_pair<T, P, false>(gm, dg);
    if (in && out) out[p] = squared ? v : Nm::sqrt(v);
    return;
  }
  const T v = grass_pair<T, P, true>(gm, dg);
  if (in && out) out[p] = squared ? v : Nm::sqrt(v);
  T w = g[p];
  if (!squared) w *= T(0.5) * Nm::rsqrt(v);
  T ox[NP][P], oy[NP][P];
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) {
      T ax = T(0), ay = T(0);
#pragma unroll
      for (int k = 0; k < P; ++k) { ax = Nm::fma(ya[r][k], dg[c][k], ax); ay = Nm::fma(xa[r][k], dg[k][c], ay); }
      ox[r][c] = w * ax;  // d/dx = y dG^T
      oy[r][c] = w * ay;  // d/dy = x dG
    }
  if (in) { store<T, NP, P>(gx + p * N * P, N, ox); store<T, NP, P>(gy + p * N * P, N, oy); }
}

// ------------------------------------------------------------------ pdist

template <typename T, int NP, int P, int TI>
__global__ __launch_bounds__(kBlk) void grass_pdist_fwd_kernel(const T* __restrict__ x, int n, int N, int row_begin,
                                                               int row_end, int squared, T* __restrict__ out) {
  const int i0 = row_begin + blockIdx.y * TI, i1 = min(i0 + TI, row_end);
  const int jbase = ((i0 + 1) / kBlk + blockIdx.x) * kBlk;
  if (jbase >= n) return;
  if (jbase + (int(threadIdx.x) & ~63) + 63 <= i0) return;
  const int j = jbase + threadIdx.x;
  const bool jin = j < n;
  T xj[NP][P];
  load<T, NP, P>(x + size_t(jin ? j : 0) * N * P, N, xj);
  const int64_t base = pair_off(n, row_begin);
  for (int i = i0; i < i1; ++i) {
    T xi[NP][P], gm[P][P], dg[P][P];
    load<T, NP, P>(x + size_t(i) * N * P, N, xi);  // wave-uniform -> scalar loads
    gram<T, NP, P>(xi, xj, gm);
    const T v = grass_pair<T, P, false>(gm, dg);
    if (jin && j > i) out[pair_off(n, i) - base + (j - i - 1)] = squared ? v : Num<T>::sqrt(v);
  }
}

// every ordered pair: a lane accumulates only its own column's gradient (as in vec.hip)
template <typename T, int NP, int P, int TI>
__global__ __launch_bounds__(kBlk) void grass_pdist_bwd_kernel(const T* __restrict__ x, const T* __restrict__ g, int n,
                                                               int N, int row_begin, int row_end, int squared,
                                                               T* __restrict__ acc /* [NP*P][n] */) {
  using Nm = Num<T>;
  const int j = blockIdx.x * kBlk + threadIdx.x;
  const int i0 = blockIdx.y * TI, i1 = min(i0 + TI, n);
  const bool jin = j < n;
  const bool jown = jin && j >= row_begin && j < row_end;
  T xj[NP][P], a[NP][P];
  load<T, NP, P>(x + size_t(jin ? j : 0) * N * P, N, xj);
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) a[r][c] = T(0);
  const int64_t base = pair_off(n, row_begin);
  for (int i = i0; i < i1; ++i) {
    T xi[NP][P], gm[P][P], dg[P][P];
    load<T, NP, P>(x + size_t(i) * N * P, N, xi);
    const bool up = i < j;
    const bool valid = jin && i != j && (up ? (i >= row_begin && i < row_end) : jown);
    const int lo = up ? i : j, hi = up ? j : i;
    T w = T(0);
    if (valid) w = g[pair_off(n, lo) - base + (hi - lo - 1)];
    gram<T, NP, P>(xi, xj, gm);  // x_i^T x_j ; d/dx_j = x_i dG
    const T v = grass_pair<T, P, true>(gm, dg);
    if (!squared) w *= T(0.5) * Nm::rsqrt(v);
    w = valid ? w : T(0);
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c) {
        T s = T(0);
#pragma unroll
        for (int k = 0; k < P; ++k) s = Nm::fma(xi[r][k], dg[k][c], s);
        a[r][c] = Nm::fma(w, s, a[r][c]);
      }
  }
  if (jin) {
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c)
        if (r < N) atomic_add(&acc[size_t(r * P + c) * n + j], a[r][c]);
  }
}

template <typename T>
__global__ void grass_finalize_kernel(const T* __restrict__ acc, int n, int np, T* __restrict__ grad) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  for (int k = 0; k < np; ++k) grad[size_t(j) * np + k] = acc[size_t(k) * n + j];
}

}  // namespace mat
}  // namespace mm

using namespace mm;
using namespace mm::mat;

extern "C" {

int mm_mat_max_rows(void) { return 9; }
int mm_mat_max_cols(void) { return 4; }

size_t mm_grass_pdist_ws_bytes(int dtype, int64_t n, int N, int p) {
  return (dtype == MM_F64 ? 8 : 4) * size_t(n) * size_t(N) * size_t(p);
}

int mm_mat_map(int dtype, int kind, int op, const void* x, const void* u, int64_t cnt, int N, int p, void* out,
               mm_stream_t stream) {
  if (cnt < 0 || N < 1 || p < 1 || p > N || op < 0 || op > MM_MAT_LOG || (kind != MM_GRASSMANN && kind != MM_STIEFEL))
    return MM_ERR_ARG;
  if (cnt > 0 && (!x || !out || (op != MM_MAT_PROJX && !u))) return MM_ERR_ARG;
  if (kind == MM_STIEFEL && (op == MM_MAT_EXP || op == MM_MAT_LOG)) return MM_ERR_UNSUPPORTED;  // stiefel.py:59-75
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned nb = unsigned((cnt + 63) / 64);
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    mat_map_kernel<T, NP, P><<<dim3(nb), dim3(64), 0, st>>>(kind, op, static_cast<const T*>(x),
        static_cast<const T*>(u), cnt, N, static_cast<T*>(out));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

int mm_grass_dist(int dtype, const void* x, const void* y, const void* g, int64_t cnt, int N, int p, int squared,
                  void* out, void* grad_x, void* grad_y, mm_stream_t stream) {
  if (cnt < 0 || N < 1 || p < 1 || p > N || (cnt > 0 && (!x || !y)) || ((grad_x != nullptr) != (grad_y != nullptr)) ||
      (grad_x && !g))
    return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned nb = unsigned((cnt + 63) / 64);
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    grass_dist_kernel<T, NP, P><<<dim3(nb), dim3(64), 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(y),
        static_cast<const T*>(g), cnt, N, squared, static_cast<T*>(out), static_cast<T*>(grad_x),
        static_cast<T*>(grad_y));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

int mm_grass_pdist_fwd(int dtype, const void* x, int64_t n, int N, int p, int64_t row_begin, int64_t row_end,
                       int squared, void* out, mm_stream_t stream) {
  if (!x || n < 0 || N < 1 || p < 1 || p > N || row_begin < 0 || row_end > n || row_begin > row_end || n > (1 << 30))
    return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  if (!out && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  if (row_end <= row_begin) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr int TI = 16;
  const int gx = int((n + kBlk - 1) / kBlk) - int((row_begin + 1) / kBlk);
  const int gy = int((row_end - row_begin + TI - 1) / TI);
  if (gx <= 0) return MM_OK;
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    grass_pdist_fwd_kernel<T, NP, P, TI><<<dim3(gx, gy), dim3(kBlk), 0, st>>>(static_cast<const T*>(x), int(n), N,
        int(row_begin), int(row_end), squared, static_cast<T*>(out));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

int mm_grass_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int N, int p, int64_t row_begin,
                       int64_t row_end, int squared, void* grad_x, void* ws, mm_stream_t stream) {
  if (!x || !grad_x || !ws || n < 1 || N < 1 || p < 1 || p > N || row_begin < 0 || row_end > n ||
      row_begin > row_end || n > (1 << 30))
    return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  if (!g && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr int TI = 32;
  hipError_t e = clear_async(ws, mm_grass_pdist_ws_bytes(dtype, n, N, p), st);   // (a kernel: clear.hpp says why)
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    if (row_end > row_begin) {
      grass_pdist_bwd_kernel<T, NP, P, TI><<<dim3(int((n + kBlk - 1) / kBlk), int((n + TI - 1) / TI)), dim3(kBlk), 0, st>>>(
          static_cast<const T*>(x), static_cast<const T*>(g), int(n), N, int(row_begin), int(row_end), squared,
          static_cast<T*>(ws));
      MM_CHECK_LAUNCH();
    }
    grass_finalize_kernel<T><<<dim3(int((n + 127) / 128)), dim3(128), 0, st>>>(static_cast<const T*>(ws), int(n),
                                                                              N * p, static_cast<T*>(grad_x));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

}  // extern "C"
