// SO(n), n <= 4: geodesic distance (element-wise and over the pair list, with gradients), log / exp, and the fused objective
// loss(target, softplus(scale) * pdist(x)^2).  The arithmetic of a pair is so_pair (so_pair.hpp); proju, projx, the retractions and
// the fused optimizer steps are those of St(n, n) (mat.hip, mat_step.hip).
//
// Pair kernels: the scheme of grass_loss_sym_kernel (grass_loss.hpp).  Tiles of 16 rows x 64 columns, one wavefront per workgroup;
// every unordered pair (i, j), row_begin <= i < row_end, j > i, is visited once.  A lane owns column j and keeps x_j and its column
// sums in registers; the row point x_i is wave-uniform (scalar loads).  From the pair's dD = d(d^2)/dx_j and the weight w
//   column side  acc_j += w dD     in registers, down the row tile; one atomic per value and tile at its end;
//   row side     -w dD             summed across the wavefront by the transposing reduction of smallmat.hpp (the whole matrix at once
//                                  in fp32, a matrix row at a time in fp64), parked in LDS, flushed with one atomic per value and row.
// The sums go into the transposed workspace acc [N*N][n]; a finalize launch writes grad [n][N][N] (and the loss record).
// LOSS = MM_LOSS_NONE is the backward of pdist: `target` then holds the upstream gradient of the pair vector and SQUARED says
// whether that vector held d^2 or d.  The forward writes the pair vector with one store per pair.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mm_manifolds.h"
#include "loss.hpp"
#include "mat_common.hpp"
#include "smallmat.hpp"
#include "so_pair.hpp"

namespace mm {
namespace so {

using mat::kBlk;
using mat::moff;

constexpr int kTI = 16;   // rows per tile
constexpr int kMaxDim = 4;

template <typename T, int N> constexpr int group_rows() { return sizeof(T) == 4 ? N : 1; }

template <typename T, int N> __device__ __forceinline__ void diff(const T (&y)[N][N], const T (&x)[N][N], T (&d)[N][N]) {
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) d[r][c] = y[r][c] - x[r][c];
}

// d(sqrt v)/dv, 0 for coincident points
template <typename T> __device__ __forceinline__ T half_rsqrt(T v) { return v > T(0) ? T(0.5) * Num<T>::rsqrt(v) : T(0); }

// ------------------------------------------------------------------------------------------------ element-wise
template <typename T, int N>
__global__ __launch_bounds__(64) void so_map_kernel(int op, const T* __restrict__ x, const T* __restrict__ u, int64_t cnt,
                                                    T* __restrict__ out) {
  const int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in = p0 < cnt;
  const int64_t p = in ? p0 : 0;
  T xa[N][N], ua[N][N], o[N][N];
  load<T, N>(x + p * N * N, xa);
  load<T, N>(u + p * N * N, ua);
  if (op == MM_SO_LOG) log_op<T, N>(xa, ua, o);
  else exp_op<T, N>(xa, ua, o);
  if (in) store<T, N>(out + p * N * N, o);
}

template <typename T, int N>
__global__ __launch_bounds__(64) void so_dist_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ g,
                                                     int64_t cnt, int squared, T* __restrict__ out, T* __restrict__ gx,
                                                     T* __restrict__ gy) {
  const int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in = p0 < cnt;
  const int64_t p = in ? p0 : 0;
  T xa[N][N], ya[N][N], D[N][N], dD[N][N];
  load<T, N>(x + p * N * N, xa);
  load<T, N>(y + p * N * N, ya);
  diff<T, N>(ya, xa, D);
  if (gx == nullptr) {
    const T v = so_pair<T, N, false>(D, dD);
    if (in && out) out[p] = squared ? v : Num<T>::sqrt(v);
    return;
  }
  const T v = so_pair<T, N, true>(D, dD);
  if (in && out) out[p] = squared ? v : Num<T>::sqrt(v);
  T w = g[p];
  if (!squared) w *= half_rsqrt(v);
  T ox[N][N];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) { dD[r][c] *= w; ox[r][c] = -dD[r][c]; }
  if (in) { store<T, N>(gx + p * N * N, ox); store<T, N>(gy + p * N * N, dD); }
}

// ------------------------------------------------------------------------------------------------ pair list
template <typename T, int N>
__global__ __launch_bounds__(kBlk) void so_pdist_fwd_kernel(const T* __restrict__ x, int n, int row_begin, int row_end, int squared,
                                                            T* __restrict__ out) {
  const int i0 = row_begin + blockIdx.y * kTI, i1 = min(i0 + kTI, row_end);
  const int jbase = ((i0 + 1) / kBlk + blockIdx.x) * kBlk;
  if (jbase >= n) return;
  if (jbase + (int(threadIdx.x) & ~63) + 63 <= i0) return;
  const int j = jbase + threadIdx.x;
  const bool jin = j < n;
  T xj[N][N];
  load<T, N>(x + size_t(jin ? j : 0) * N * N, xj);
  const int64_t base = moff(n, row_begin);
  for (int i = i0; i < i1; ++i) {
    T xi[N][N], D[N][N], dD[N][N];
    load<T, N>(x + size_t(i) * N * N, xi);  // wave-uniform -> scalar loads
    diff<T, N>(xj, xi, D);
    const T v = so_pair<T, N, false>(D, dD);
    if (jin && j > i) out[moff(n, i) - base + (j - i - 1)] = squared ? v : Num<T>::sqrt(v);
  }
}

template <typename T, int N, int LOSS, bool SQUARED>
__global__ __launch_bounds__(64) void so_pdist_sym_kernel(const T* __restrict__ x, const T* __restrict__ target, int n,
                                                          int row_begin, int row_end, int gx, int jb0, LossArgs<T> la,
                                                          T* __restrict__ acc /* [N*N][n] */) {
  static_assert(LOSS == MM_LOSS_NONE || SQUARED, "the objectives are functions of d^2");
  constexpr int GR = group_rows<T, N>(), GV = GR * N;
  __shared__ T red[kTI][N * N];
  const int lane = threadIdx.x;
  const int by = int(blockIdx.x) / gx, bx = int(blockIdx.x) - by * gx;
  const int i0 = row_begin + by * kTI, i1 = min(i0 + kTI, row_end);
  const int jbase = (jb0 + bx) * 64;   // (< n: gx = ceil(n / 64) - jb0)
  if (jbase + 63 <= i0) return;        // no column right of the tile's first row, so of none of its rows
  T sp = T(1);
  if constexpr (LOSS != MM_LOSS_NONE) {
    loss_resolve<T, LOSS>(la);
    sp = softplus_of(la.scale_raw);
  }
  const int j = jbase + lane;
  const bool jin = j < n;
  bool writer;
  const int slot = reduce_slot<GV>(lane, writer);
  T xj[N][N], a[N][N];
  load<T, N>(x + size_t(jin ? j : 0) * N * N, xj);   // (a lane past the end loads point 0 and contributes nothing)
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) a[r][c] = T(0);
  T loss_acc = T(0), ds_acc = T(0);
  const int64_t base = moff(n, row_begin);
  const int ilast = min(i1, jbase + 63);   // rows from here on have no column in this block
  for (int i = i0; i < ilast; ++i) {
    T xi[N][N], D[N][N], dD[N][N];
    load<T, N>(x + size_t(i) * N * N, xi);  // wave-uniform -> scalar loads
    const bool valid = jin && j > i;
    T tg = LOSS == MM_LOSS_NONE ? T(0) : T(1);
    if (valid) tg = target[moff(n, i) - base + (j - i - 1)];
    diff<T, N>(xj, xi, D);
    const T v = so_pair<T, N, true>(D, dD);
    T w;
    if constexpr (LOSS == MM_LOSS_NONE) {
      w = SQUARED ? tg : tg * half_rsqrt(v);
    } else {
      T dldm;
      const T l = loss_term<T, LOSS>(sp * v, tg, la, dldm);
      loss_acc += valid ? l : T(0);
      ds_acc += valid ? dldm * v : T(0);
      w = dldm * sp;
    }
    w = valid ? w : T(0);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
      for (int c = 0; c < N; ++c) {
        dD[r][c] *= w;
        a[r][c] += dD[r][c];
      }
#pragma unroll
    for (int g = 0; g < N / GR; ++g) {
      T rs[GV];
#pragma unroll
      for (int rr = 0; rr < GR; ++rr)
#pragma unroll
        for (int c = 0; c < N; ++c) rs[rr * N + c] = -dD[g * GR + rr][c];
      const T tot = wave_reduce_transposed<GV, T>(rs, lane);
      if (writer) red[i - i0][g * GV + slot] = tot;
    }
  }
  __builtin_amdgcn_wave_barrier();
  {
    constexpr int nn = N * N;
    const int cnt = (ilast - i0) * nn;
    for (int t = lane; t < cnt; t += 64) {
      const int il = t / nn, k = t - il * nn;
      atomic_add(&acc[size_t(k) * n + (i0 + il)], red[il][k]);
    }
  }
  if (jin) {
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
      for (int c = 0; c < N; ++c) atomic_add(&acc[size_t(r * N + c) * n + j], a[r][c]);
  }
  if constexpr (LOSS != MM_LOSS_NONE) {
    const T ls = wave_sum(loss_acc), dd = wave_sum(ds_acc);
    if (lane == 0) {
      const int s = blockIdx.x & (kLossSlots - 1);
      atomic_add(&la.slots[s], ls);
      atomic_add(&la.slots[kLossSlots + s], dd);
    }
  }
}

// grad [n][nn] from the transposed accumulators; with slots, the first wavefront of block 0 closes the loss record
template <typename T>
__global__ __launch_bounds__(128) void so_finalize_kernel(const T* __restrict__ acc, int n, int nn, T* __restrict__ grad,
                                                          T* __restrict__ slots, const T* __restrict__ scale_raw,
                                                          T* __restrict__ loss_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n)
    for (int k = 0; k < nn; ++k) grad[size_t(j) * nn + k] = acc[size_t(k) * n + j];
  if (slots && blockIdx.x == 0 && threadIdx.x < 64) loss_finalize<T>(slots, scale_raw, loss_out);
}

inline size_t acc_bytes(int dtype, int64_t n, int N) {
  const size_t b = (dtype == MM_F64 ? 8 : 4) * size_t(n) * size_t(N) * size_t(N);
  return (b + 255) & ~size_t(255);
}

template <typename T, int N, int LOSS, bool SQUARED>
int launch_sym(const T* x, const T* target, int64_t n, int64_t rb, int64_t re, LossArgs<T> la, T* acc, hipStream_t st) {
  const int jb0 = int((rb + 1) / 64);
  const int64_t gx = (n + 63) / 64 - jb0, gy = (re - rb + kTI - 1) / kTI;
  if (gx <= 0 || gy <= 0) return MM_OK;
  so_pdist_sym_kernel<T, N, LOSS, SQUARED><<<dim3(unsigned(gx * gy)), dim3(64), 0, st>>>(x, target, int(n), int(rb), int(re),
                                                                                        int(gx), jb0, la, acc);
  MMM_CHECK();
  return MM_OK;
}

// shared argument checks of the pair-list entry points (before anything touches the GPU)
inline int check_pairs(int dtype, const void* x, int64_t n, int N, int64_t rb, int64_t re) {
  if (!x || n < 1 || N < 1 || rb < 0 || re > n || rb > re || n > (1 << 30) || (dtype != MM_F32 && dtype != MM_F64))
    return MM_ERR_ARG;
  if (N < 2 || N > kMaxDim) return MM_ERR_UNSUPPORTED;
  // (the tiles are numbered in one grid dimension)
  if (((n + 63) / 64) * ((re - rb + kTI - 1) / kTI) > INT32_MAX) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

#define MMSO_DISPATCH_N(N_, ...)                          \
  switch (N_) {                                           \
    case 2: { constexpr int N = 2; __VA_ARGS__ }          \
    case 3: { constexpr int N = 3; __VA_ARGS__ }          \
    case 4: { constexpr int N = 4; __VA_ARGS__ }          \
    default: return MM_ERR_UNSUPPORTED;                   \
  }

}  // namespace so
}  // namespace mm

using namespace mm;
using namespace mm::so;

extern "C" {

int mm_so_max_dim(void) { return kMaxDim; }

int mm_so_map(int dtype, int op, const void* x, const void* u, int64_t cnt, int N, void* out, mm_stream_t stream) {
  if (cnt < 0 || N < 1 || (op != MM_SO_LOG && op != MM_SO_EXP) || (dtype != MM_F32 && dtype != MM_F64)) return MM_ERR_ARG;
  if (cnt > 0 && (!x || !u || !out)) return MM_ERR_ARG;
  if (N < 2 || N > kMaxDim) return MM_ERR_UNSUPPORTED;
  if ((cnt + 63) / 64 > INT32_MAX) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned nb = unsigned((cnt + 63) / 64);
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    so_map_kernel<T, N><<<dim3(nb), dim3(64), 0, st>>>(op, static_cast<const T*>(x), static_cast<const T*>(u), cnt,
                                                     static_cast<T*>(out));
    MMM_CHECK(); return MM_OK; }))
}

int mm_so_dist(int dtype, const void* x, const void* y, const void* g, int64_t cnt, int N, int squared, void* out, void* grad_x,
               void* grad_y, mm_stream_t stream) {
  if (cnt < 0 || N < 1 || (cnt > 0 && (!x || !y)) || ((grad_x != nullptr) != (grad_y != nullptr)) || (grad_x && !g) ||
      (dtype != MM_F32 && dtype != MM_F64))
    return MM_ERR_ARG;
  if (N < 2 || N > kMaxDim) return MM_ERR_UNSUPPORTED;
  if ((cnt + 63) / 64 > INT32_MAX) return MM_ERR_UNSUPPORTED;
  if (cnt == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned nb = unsigned((cnt + 63) / 64);
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    so_dist_kernel<T, N><<<dim3(nb), dim3(64), 0, st>>>(static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const T*>(g),
                                                      cnt, squared, static_cast<T*>(out), static_cast<T*>(grad_x),
                                                      static_cast<T*>(grad_y));
    MMM_CHECK(); return MM_OK; }))
}

size_t mm_so_pdist_ws_bytes(int dtype, int64_t n, int N) {
  if (n < 0 || N < 1) return 0;
  return acc_bytes(dtype, n, N);
}

int mm_so_pdist_fwd(int dtype, const void* x, int64_t n, int N, int64_t row_begin, int64_t row_end, int squared, void* out,
                    mm_stream_t stream) {
  const int rc = check_pairs(dtype, x, n, N, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (!out && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  if (row_end <= row_begin) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int gx = int((n + kBlk - 1) / kBlk) - int((row_begin + 1) / kBlk);
  const int64_t gy = (row_end - row_begin + kTI - 1) / kTI;
  if (gx <= 0) return MM_OK;
  if (gy > 65535) return MM_ERR_UNSUPPORTED;   // (grid.y; a range of 2^20 rows: shard it)
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    so_pdist_fwd_kernel<T, N><<<dim3(gx, int(gy)), dim3(kBlk), 0, st>>>(static_cast<const T*>(x), int(n), int(row_begin),
                                                                       int(row_end), squared, static_cast<T*>(out));
    MMM_CHECK(); return MM_OK; }))
}

int mm_so_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int N, int64_t row_begin, int64_t row_end, int squared,
                    void* grad_x, void* ws, mm_stream_t stream) {
  const int rc = check_pairs(dtype, x, n, N, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (!grad_x || !ws) return MM_ERR_ARG;
  const bool pairs = mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin);
  if (!g && pairs) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(ws, 0, mm_so_pdist_ws_bytes(dtype, n, N), st);
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    T* acc = static_cast<T*>(ws);
    if (pairs) {
      LossArgs<T> la{nullptr, T(1), T(0), 0, nullptr, nullptr};
      const int r2 = squared
          ? launch_sym<T, N, MM_LOSS_NONE, true>(static_cast<const T*>(x), static_cast<const T*>(g), n, row_begin, row_end, la, acc, st)
          : launch_sym<T, N, MM_LOSS_NONE, false>(static_cast<const T*>(x), static_cast<const T*>(g), n, row_begin, row_end, la, acc, st);
      if (r2 != MM_OK) return r2;
    }
    so_finalize_kernel<T><<<dim3(unsigned((n + 127) / 128)), dim3(128), 0, st>>>(acc, int(n), N * N, static_cast<T*>(grad_x),
                                                                                nullptr, nullptr, nullptr);
    MMM_CHECK(); return MM_OK; }))
}

size_t mm_so_pdist_loss_ws_bytes(int dtype, int64_t n, int N) {
  if (n < 0 || N < 1) return 0;
  return acc_bytes(dtype, n, N) + 2 * kLossSlots * (dtype == MM_F64 ? 8 : 4);
}

int mm_so_pdist_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n, int N,
                     int64_t row_begin, int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                     void* loss_out, void* grad_x, void* ws, mm_stream_t stream) {
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_ARG;
  const int rc = check_pairs(dtype, x, n, N, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (!grad_x || !ws || !loss_out) return MM_ERR_ARG;
  const bool pairs = mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin);
  if (!target && pairs) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(ws, 0, mm_so_pdist_loss_ws_bytes(dtype, n, N), st);
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    T* acc = static_cast<T*>(ws);
    T* slots = reinterpret_cast<T*>(static_cast<char*>(ws) + acc_bytes(dtype, n, N));
    const T* sr = static_cast<const T*>(scale_raw);
    if (pairs) {
      LossArgs<T> la{sr, T(alpha), T(eps), terms, slots, loss_params};
      const int r2 = loss_kind == MM_LOSS_STRESS
          ? launch_sym<T, N, MM_LOSS_STRESS, true>(static_cast<const T*>(x), static_cast<const T*>(target), n, row_begin, row_end, la, acc, st)
          : launch_sym<T, N, MM_LOSS_QUOTIENT, true>(static_cast<const T*>(x), static_cast<const T*>(target), n, row_begin, row_end, la, acc, st);
      if (r2 != MM_OK) return r2;
    }
    so_finalize_kernel<T><<<dim3(unsigned((n + 127) / 128)), dim3(128), 0, st>>>(acc, int(n), N * N, static_cast<T*>(grad_x), slots,
                                                                                sr, static_cast<T*>(loss_out));
    MMM_CHECK(); return MM_OK; }))
}

}  // extern "C"
