// SO(n), n <= 4, for a NODE MINIBATCH: the pair kernels of so.hip with the index vector (mm_so_pdist_fwd_subset,
// mm_so_pdist_bwd_subset, mm_so_pdist_loss_subset).  The scheme is that of grass_loss.hpp with SUB: the pairs are those of the
// BATCH POSITIONS 0 .. bs, the row point is x[node(i)] (wave-uniform: the node id is broadcast to a scalar register, the loads stay
// scalar), the column point x[node(j)], node(pos) = clamp(low 32 bits of idx[pos], 0, n_total - 1).  The forward writes the batch's
// pair vector; the symmetric kernel sums into accumulators addressed by NODE, acc [N*N][n_total], and the finalize launch over
// n_total writes the whole dense gradient: rows outside the batch come out as the +0 the memset left.  No gather, no scatter-add,
// no zero fill.
//   LOSS = MM_LOSS_NONE      the backward of the pair vector: `target` is the upstream gradient by batch pair position.  Repeated
//                            nodes are correct here: the sums are per node through atomics, and a pair of a node with itself has
//                            D = 0, so d = 0 and a zero gradient in the squared and the non-squared form.
//   STRESS / QUOTIENT        the target of batch pair (a, b), a < b, is dense[node(a)][node(b)]; the nodes of a batch are distinct.
// The lane's node id is not kept across the row loop: it is re-read where it is needed.  The arithmetic of a pair is so_pair
// (so_pair.hpp), unchanged.  A translation unit and a namespace of its own: the kernels of so.hip come out as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mm_manifolds.h"
#include "loss.hpp"
#include "mat_common.hpp"
#include "smallmat.hpp"
#include "so_pair.hpp"

namespace mm {
namespace so_sub {

using mat::kBlk;
using mat::moff;
using so::load;
using so::so_pair;

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

// node id of batch position `pos`: the low 32 bits of the index, clamped into the table
__device__ __forceinline__ int node_of(const int64_t* __restrict__ idx, int pos, int n_total) {
  return min(max(int(idx[pos]), 0), n_total - 1);
}

// the pair vector of the batch (positions 0 .. bs), rows row_begin .. row_end
template <typename T, int N>
__global__ __launch_bounds__(kBlk) void so_pdist_fwd_kernel(const T* __restrict__ x, const int64_t* __restrict__ idx, int bs,
                                                            int n_total, int row_begin, int row_end, int squared,
                                                            T* __restrict__ out) {
  const int i0 = row_begin + blockIdx.y * kTI, i1 = min(i0 + kTI, row_end);
  const int jbase = ((i0 + 1) / kBlk + blockIdx.x) * kBlk;
  if (jbase >= bs) return;
  if (jbase + (int(threadIdx.x) & ~63) + 63 <= i0) return;
  const int j = jbase + threadIdx.x;
  const bool jin = j < bs;
  T xj[N][N];
  load<T, N>(x + size_t(node_of(idx, jin ? j : 0, n_total)) * N * N, xj);
  const int64_t base = moff(bs, row_begin);
  for (int i = i0; i < i1; ++i) {
    T xi[N][N], D[N][N], dD[N][N];
    const int ni = __builtin_amdgcn_readfirstlane(node_of(idx, i, n_total));
    load<T, N>(x + size_t(ni) * N * N, xi);  // wave-uniform -> scalar loads
    diff<T, N>(xj, xi, D);
    const T v = so_pair<T, N, false>(D, dD);
    if (jin && j > i) out[moff(bs, i) - base + (j - i - 1)] = squared ? v : Num<T>::sqrt(v);
  }
}

// bs: the batch positions whose pairs are walked; acc is addressed by node
template <typename T, int N, int LOSS, bool SQUARED>
__global__ __launch_bounds__(64) void so_pdist_sym_kernel(const T* __restrict__ x, const T* __restrict__ target,
                                                          const int64_t* __restrict__ idx, int bs, int n_total, int row_begin,
                                                          int row_end, int gx, int jb0, LossArgs<T> la,
                                                          T* __restrict__ acc /* [N*N][n_total] */) {
  static_assert(LOSS == MM_LOSS_NONE || SQUARED, "the objectives are functions of d^2");
  constexpr int GR = group_rows<T, N>(), GV = GR * N;
  __shared__ T red[kTI][N * N];
  const int lane = threadIdx.x;
  const int by = int(blockIdx.x) / gx, bx = int(blockIdx.x) - by * gx;
  const int i0 = row_begin + by * kTI, i1 = min(i0 + kTI, row_end);
  const int jbase = (jb0 + bx) * 64;   // (< bs: gx = ceil(bs / 64) - jb0)
  if (jbase + 63 <= i0) return;        // no column right of the tile's first row, so of none of its rows
  T sp = T(1);
  if constexpr (LOSS != MM_LOSS_NONE) {
    loss_resolve<T, LOSS>(la);
    sp = softplus_of(la.scale_raw);
  }
  const int j = jbase + lane;
  const bool jin = j < bs;
  bool writer;
  const int slot = reduce_slot<GV>(lane, writer);
  T xj[N][N], a[N][N];
  // (a lane past the end loads the point of position 0 and contributes nothing)
  load<T, N>(x + size_t(node_of(idx, jin ? j : 0, n_total)) * N * N, xj);
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) a[r][c] = T(0);
  T loss_acc = T(0), ds_acc = T(0);
  const int64_t base = moff(bs, row_begin);
  const int ilast = min(i1, jbase + 63);   // rows from here on have no column in this block
  for (int i = i0; i < ilast; ++i) {
    T xi[N][N], D[N][N], dD[N][N];
    const int ni = __builtin_amdgcn_readfirstlane(node_of(idx, i, n_total));
    load<T, N>(x + size_t(ni) * N * N, xi);  // wave-uniform -> scalar loads
    const bool valid = jin && j > i;
    T tg = LOSS == MM_LOSS_NONE ? T(0) : T(1);
    if (valid) {
      if constexpr (LOSS == MM_LOSS_NONE) tg = target[moff(bs, i) - base + (j - i - 1)];
      else tg = target[size_t(ni) * size_t(n_total) + size_t(node_of(idx, j, n_total))];
    }
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
      atomic_add(&acc[size_t(k) * n_total + node_of(idx, i0 + il, n_total)], red[il][k]);
    }
  }
  if (jin) {
    const int col = node_of(idx, j, n_total);
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
      for (int c = 0; c < N; ++c) atomic_add(&acc[size_t(r * N + c) * n_total + col], a[r][c]);
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

// grad [n_total][nn] from the node-addressed accumulators; with slots, the first wavefront of block 0 closes the loss record
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
int launch_sym(const T* x, const T* target, const int64_t* idx, int64_t bs, int64_t n_total, int64_t rb, int64_t re, LossArgs<T> la,
               T* acc, hipStream_t st) {
  const int jb0 = int((rb + 1) / 64);
  const int64_t gx = (bs + 63) / 64 - jb0, gy = (re - rb + kTI - 1) / kTI;
  if (gx <= 0 || gy <= 0) return MM_OK;
  so_pdist_sym_kernel<T, N, LOSS, SQUARED><<<dim3(unsigned(gx * gy)), dim3(64), 0, st>>>(x, target, idx, int(bs), int(n_total),
                                                                                        int(rb), int(re), int(gx), jb0, la, acc);
  MMM_CHECK();
  return MM_OK;
}

// shared argument checks of the three entry points (before anything touches the GPU); bs_max: 2^30, or n_total where the nodes
// of a batch are distinct
inline int check_batch(int dtype, const void* x, int64_t n_total, int N, int64_t bs, int64_t bs_max, int64_t rb, int64_t re) {
  if (!x || n_total < 1 || n_total > (1 << 30) || N < 1 || bs < 0 || bs > bs_max || rb < 0 || re > bs || rb > re ||
      (dtype != MM_F32 && dtype != MM_F64))
    return MM_ERR_ARG;
  if (N < 2 || N > kMaxDim) return MM_ERR_UNSUPPORTED;
  // (the tiles are numbered in one grid dimension)
  if (((bs + 63) / 64) * ((re - rb + kTI - 1) / kTI) > INT32_MAX) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

inline bool has_pairs(int64_t bs, int64_t rb, int64_t re) {
  return bs >= 2 && mm_pair_offset(bs, re) > mm_pair_offset(bs, rb);
}

#define MMSOS_DISPATCH_N(N_, ...)                         \
  switch (N_) {                                           \
    case 2: { constexpr int N = 2; __VA_ARGS__ }          \
    case 3: { constexpr int N = 3; __VA_ARGS__ }          \
    case 4: { constexpr int N = 4; __VA_ARGS__ }          \
    default: return MM_ERR_UNSUPPORTED;                   \
  }

}  // namespace so_sub
}  // namespace mm

using namespace mm;
using namespace mm::so_sub;

extern "C" {

int mm_so_pdist_fwd_subset(int dtype, const void* x, int64_t n_total, int N, const int64_t* idx, int64_t bs, int64_t row_begin,
                           int64_t row_end, int squared, void* out, mm_stream_t stream) {
  const int rc = check_batch(dtype, x, n_total, N, bs, int64_t(1) << 30, row_begin, row_end);
  if (rc != MM_OK) return rc;
  const int64_t gy = (row_end - row_begin + kTI - 1) / kTI;
  if (gy > 65535) return MM_ERR_UNSUPPORTED;   // (grid.y; a range of 2^20 rows: shard it)
  const bool pairs = has_pairs(bs, row_begin, row_end);
  if (pairs && (!idx || !out)) return MM_ERR_ARG;
  if (!pairs) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int gx = int((bs + kBlk - 1) / kBlk) - int((row_begin + 1) / kBlk);
  if (gx <= 0) return MM_OK;
  MMM_DISPATCH_T(dtype, MMSOS_DISPATCH_N(N, {
    so_pdist_fwd_kernel<T, N><<<dim3(gx, int(gy)), dim3(kBlk), 0, st>>>(static_cast<const T*>(x), idx, int(bs), int(n_total),
                                                                       int(row_begin), int(row_end), squared, static_cast<T*>(out));
    MMM_CHECK(); return MM_OK; }))
}

int mm_so_pdist_bwd_subset(int dtype, const void* x, const void* g, int64_t n_total, int N, const int64_t* idx, int64_t bs,
                           int64_t row_begin, int64_t row_end, int squared, void* grad_x, void* ws, mm_stream_t stream) {
  const int rc = check_batch(dtype, x, n_total, N, bs, int64_t(1) << 30, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (!grad_x || !ws) return MM_ERR_ARG;
  const bool pairs = has_pairs(bs, row_begin, row_end);
  if (pairs && (!g || !idx)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(ws, 0, mm_so_pdist_ws_bytes(dtype, n_total, N), st);
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMSOS_DISPATCH_N(N, {
    T* acc = static_cast<T*>(ws);
    if (pairs) {
      LossArgs<T> la{nullptr, T(1), T(0), 0, nullptr, nullptr};
      const int r2 = squared
          ? launch_sym<T, N, MM_LOSS_NONE, true>(static_cast<const T*>(x), static_cast<const T*>(g), idx, bs, n_total, row_begin, row_end, la, acc, st)
          : launch_sym<T, N, MM_LOSS_NONE, false>(static_cast<const T*>(x), static_cast<const T*>(g), idx, bs, n_total, row_begin, row_end, la, acc, st);
      if (r2 != MM_OK) return r2;
    }
    so_finalize_kernel<T><<<dim3(unsigned((n_total + 127) / 128)), dim3(128), 0, st>>>(acc, int(n_total), N * N, static_cast<T*>(grad_x),
                                                                                      nullptr, nullptr, nullptr);
    MMM_CHECK(); return MM_OK; }))
}

int mm_so_pdist_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw, int64_t n_total, int N,
                            const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end, double alpha, double eps, int terms,
                            const double* loss_params, void* loss_out, void* grad_x, void* ws, mm_stream_t stream) {
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_ARG;
  const int rc = check_batch(dtype, x, n_total, N, bs, n_total, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (!grad_x || !ws || !loss_out) return MM_ERR_ARG;
  const bool pairs = has_pairs(bs, row_begin, row_end);
  if (pairs && (!dense || !idx)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(ws, 0, mm_so_pdist_loss_ws_bytes(dtype, n_total, N), st);
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMSOS_DISPATCH_N(N, {
    T* acc = static_cast<T*>(ws);
    T* slots = reinterpret_cast<T*>(static_cast<char*>(ws) + acc_bytes(dtype, n_total, N));
    const T* sr = static_cast<const T*>(scale_raw);
    if (pairs) {
      LossArgs<T> la{sr, T(alpha), T(eps), terms, slots, loss_params};
      const int r2 = loss_kind == MM_LOSS_STRESS
          ? launch_sym<T, N, MM_LOSS_STRESS, true>(static_cast<const T*>(x), static_cast<const T*>(dense), idx, bs, n_total, row_begin, row_end, la, acc, st)
          : launch_sym<T, N, MM_LOSS_QUOTIENT, true>(static_cast<const T*>(x), static_cast<const T*>(dense), idx, bs, n_total, row_begin, row_end, la, acc, st);
      if (r2 != MM_OK) return r2;
    }
    so_finalize_kernel<T><<<dim3(unsigned((n_total + 127) / 128)), dim3(128), 0, st>>>(acc, int(n_total), N * N, static_cast<T*>(grad_x),
                                                                                      slots, sr, static_cast<T*>(loss_out));
    MMM_CHECK(); return MM_OK; }))
}

}  // extern "C"
