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
//
// NODE MINIBATCHES (mm_so_pdist_fwd_subset, mm_so_pdist_bwd_subset, mm_so_pdist_loss_subset) are the same two kernels with SUB,
// as in grass_loss.hpp: the pairs are those of the BATCH POSITIONS 0 .. bs, the row point is x[node(i)] (wave-uniform: the node id
// is broadcast to a scalar register, the loads stay scalar), the column point x[node(j)], node(pos) = clamp(low 32 bits of
// idx[pos], 0, n_total - 1).  The forward writes the batch's pair vector; the symmetric kernel sums into accumulators addressed by
// NODE, acc [N*N][n_total], and the finalize launch over n_total writes the whole dense gradient: rows outside the batch come out
// as the +0 the memset left.  No gather, no scatter-add, no zero fill.
//   LOSS = MM_LOSS_NONE      `target` is the upstream gradient by batch pair position.  Repeated nodes are correct here: the sums
//                            are per node through atomics, and a pair of a node with itself has D = 0, so d = 0 and a zero
//                            gradient in the squared and the non-squared form.
//   STRESS / QUOTIENT        the target of batch pair (a, b), a < b, is dense[node(a)][node(b)]; the nodes of a batch are distinct.
// The lane's node id is not kept across the row loop: it is re-read where it is needed.  SUB is a template parameter of the
// kernels themselves and its two arguments trail the others: the SUB = false kernels are, instruction for instruction, the
// kernels this file had before the minibatch ones joined it (profiles/so_minibatch.md).
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mm_manifolds.h"
#include "clear.hpp"
#include "loss.hpp"
#include "mat_common.hpp"
#include "smallmat.hpp"
#include "so_pair.hpp"

namespace mm {
namespace so {

using mat::kBlk;

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
// node id of batch position `pos`: the low 32 bits of the index, clamped into the table
__device__ __forceinline__ int node_of(const int64_t* __restrict__ idx, int pos, int n_total) {
  return min(max(int(idx[pos]), 0), n_total - 1);
}

// n: the number of points whose pairs are walked (SUB: the batch size); n_total, idx: SUB only (the table's rows, the batch's nodes)
template <typename T, int N, bool SUB>
__global__ __launch_bounds__(kBlk) void so_pdist_fwd_kernel(const T* __restrict__ x, int n, int row_begin, int row_end, int squared,
                                                            T* __restrict__ out, int n_total, const int64_t* __restrict__ idx) {
  const int i0 = row_begin + blockIdx.y * kTI, i1 = min(i0 + kTI, row_end);
  const int jbase = ((i0 + 1) / kBlk + blockIdx.x) * kBlk;
  if (jbase >= n) return;
  if (jbase + (int(threadIdx.x) & ~63) + 63 <= i0) return;
  const int j = jbase + threadIdx.x;
  const bool jin = j < n;
  T xj[N][N];
  if constexpr (SUB) load<T, N>(x + size_t(node_of(idx, jin ? j : 0, n_total)) * N * N, xj);
  else load<T, N>(x + size_t(jin ? j : 0) * N * N, xj);
  const int64_t base = pair_off(n, row_begin);
  for (int i = i0; i < i1; ++i) {
    T xi[N][N], D[N][N], dD[N][N];
    int ni = i;
    if constexpr (SUB) ni = __builtin_amdgcn_readfirstlane(node_of(idx, i, n_total));
    load<T, N>(x + size_t(ni) * N * N, xi);  // wave-uniform -> scalar loads
    diff<T, N>(xj, xi, D);
    const T v = so_pair<T, N, false>(D, dD);
    if (jin && j > i) out[pair_off(n, i) - base + (j - i - 1)] = squared ? v : Num<T>::sqrt(v);
  }
}

// acc is addressed by point, with SUB by node: [N*N][n or n_total]
template <typename T, int N, int LOSS, bool SQUARED, bool SUB>
__global__ __launch_bounds__(64) void so_pdist_sym_kernel(const T* __restrict__ x, const T* __restrict__ target, int n,
                                                          int row_begin, int row_end, int gx, int jb0, LossArgs<T> la,
                                                          T* __restrict__ acc, int n_total, const int64_t* __restrict__ idx) {
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
  // (a lane past the end loads the point of position 0 and contributes nothing)
  if constexpr (SUB) load<T, N>(x + size_t(node_of(idx, jin ? j : 0, n_total)) * N * N, xj);
  else load<T, N>(x + size_t(jin ? j : 0) * N * N, xj);
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) a[r][c] = T(0);
  T loss_acc = T(0), ds_acc = T(0);
  const int64_t base = pair_off(n, row_begin);
  const int ilast = min(i1, jbase + 63);   // rows from here on have no column in this block
  for (int i = i0; i < ilast; ++i) {
    T xi[N][N], D[N][N], dD[N][N];
    int ni = i;
    if constexpr (SUB) ni = __builtin_amdgcn_readfirstlane(node_of(idx, i, n_total));
    load<T, N>(x + size_t(ni) * N * N, xi);  // wave-uniform -> scalar loads
    const bool valid = jin && j > i;
    T tg = LOSS == MM_LOSS_NONE ? T(0) : T(1);
    if (valid) {
      if constexpr (SUB && LOSS != MM_LOSS_NONE) tg = target[size_t(ni) * size_t(n_total) + size_t(node_of(idx, j, n_total))];
      else tg = target[pair_off(n, i) - base + (j - i - 1)];
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
  const int na = SUB ? n_total : n;   // accumulator stride
  {
    constexpr int nn = N * N;
    const int cnt = (ilast - i0) * nn;
    for (int t = lane; t < cnt; t += 64) {
      const int il = t / nn, k = t - il * nn;
      const int row = SUB ? node_of(idx, i0 + il, n_total) : i0 + il;
      atomic_add(&acc[size_t(k) * na + row], red[il][k]);
    }
  }
  if (jin) {
    const int col = SUB ? node_of(idx, j, n_total) : j;
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
      for (int c = 0; c < N; ++c) atomic_add(&acc[size_t(r * N + c) * na + col], a[r][c]);
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

// grad [n][nn] from the transposed accumulators (n: the table's rows); with slots, the first wavefront of block 0 closes the loss
// record
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

#define MMSO_DISPATCH_N(N_, ...)                          \
  switch (N_) {                                           \
    case 2: { constexpr int N = 2; __VA_ARGS__ }          \
    case 3: { constexpr int N = 3; __VA_ARGS__ }          \
    case 4: { constexpr int N = 4; __VA_ARGS__ }          \
    default: return MM_ERR_UNSUPPORTED;                   \
  }

inline int64_t row_tiles(int64_t rb, int64_t re) { return (re - rb + kTI - 1) / kTI; }

// Shared argument checks of the pair-list entry points (before anything touches the GPU).  n: the points whose pairs are walked,
// the table itself (n = n_total, n_max = 2^30: the tests on n_total are then the tests n < 1 and n > 2^30) or a batch of it
// (n_max: 2^30, or n_total where the nodes of a batch are distinct).
inline int check_pairs(int dtype, const void* x, int64_t n_total, int N, int64_t n, int64_t n_max, int64_t rb, int64_t re) {
  if (!x || n_total < 1 || n_total > (1 << 30) || N < 1 || n < 0 || n > n_max || rb < 0 || re > n || rb > re ||
      (dtype != MM_F32 && dtype != MM_F64))
    return MM_ERR_ARG;
  if (N < 2 || N > kMaxDim) return MM_ERR_UNSUPPORTED;
  // (the tiles are numbered in one grid dimension)
  if (((n + 63) / 64) * row_tiles(rb, re) > INT32_MAX) return MM_ERR_UNSUPPORTED;
  return MM_OK;
}

// (false for n < 2 and for a range that is empty or holds only the last row)
inline bool has_pairs(int64_t n, int64_t rb, int64_t re) { return mm_pair_offset(n, re) > mm_pair_offset(n, rb); }

// the forward launch behind both entry points, after their own checks; null idx: the full batch (n_total = n)
static int launch_fwd(int dtype, const void* x, int64_t n, int N, int64_t rb, int64_t re, int squared, void* out, int64_t n_total,
                      const int64_t* idx, hipStream_t st) {
  const int gx = int((n + kBlk - 1) / kBlk) - int((rb + 1) / kBlk);
  const int64_t gy = row_tiles(rb, re);
  if (gx <= 0) return MM_OK;
  if (gy > 65535) return MM_ERR_UNSUPPORTED;   // (grid.y; a range of 2^20 rows: shard it.  A minibatch has been tested already)
  const dim3 grid(gx, int(gy));
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    if (idx) so_pdist_fwd_kernel<T, N, true><<<grid, dim3(kBlk), 0, st>>>(static_cast<const T*>(x), int(n), int(rb), int(re), squared,
                                                                         static_cast<T*>(out), int(n_total), idx);
    else so_pdist_fwd_kernel<T, N, false><<<grid, dim3(kBlk), 0, st>>>(static_cast<const T*>(x), int(n), int(rb), int(re), squared,
                                                                      static_cast<T*>(out), int(n_total), idx);
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

// null idx: the full batch (n_total = n)
template <typename T, int N, int LOSS, bool SQUARED>
int launch_sym(const T* x, const T* target, int64_t n, int64_t rb, int64_t re, LossArgs<T> la, T* acc, int64_t n_total,
               const int64_t* idx, hipStream_t st) {
  const int jb0 = int((rb + 1) / 64);
  const int64_t gx = (n + 63) / 64 - jb0, gy = row_tiles(rb, re);
  if (gx <= 0 || gy <= 0) return MM_OK;
  const dim3 grid(unsigned(gx * gy));
  if (idx) so_pdist_sym_kernel<T, N, LOSS, SQUARED, true><<<grid, dim3(64), 0, st>>>(x, target, int(n), int(rb), int(re), int(gx), jb0,
                                                                                    la, acc, int(n_total), idx);
  else so_pdist_sym_kernel<T, N, LOSS, SQUARED, false><<<grid, dim3(64), 0, st>>>(x, target, int(n), int(rb), int(re), int(gx), jb0,
                                                                                 la, acc, int(n_total), idx);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

// The backward of the pair vector (loss = MM_LOSS_NONE: `target` is the upstream gradient, no loss record) and the fused objective
// behind their four entry points, which check and act in the same order: the clear kernel, the pair kernel if the range has pairs, the
// finalize launch over the table.  sub: a node minibatch (n = bs, idx needed where there are pairs); else n_total = n, idx null.
static int pdist_sym(int dtype, int loss, const void* x, const void* target, const void* scale_raw, int64_t n, int64_t n_max, int N,
                     int64_t rb, int64_t re, int squared, double alpha, double eps, int terms, const double* loss_params,
                     void* loss_out, void* grad_x, void* ws, int64_t n_total, const int64_t* idx, bool sub, mm_stream_t stream) {
  const int rc = check_pairs(dtype, x, n_total, N, n, n_max, rb, re);
  if (rc != MM_OK) return rc;
  if (!grad_x || !ws || (loss != MM_LOSS_NONE && !loss_out)) return MM_ERR_ARG;
  const bool pairs = has_pairs(n, rb, re);
  if (pairs && (!target || (sub && !idx))) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t slot_bytes = loss == MM_LOSS_NONE ? 0 : 2 * kLossSlots * (dtype == MM_F64 ? 8 : 4);
  hipError_t e = clear_async(ws, acc_bytes(dtype, n_total, N) + slot_bytes, st);   // (a kernel: clear.hpp says why)
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMSO_DISPATCH_N(N, {
    T* acc = static_cast<T*>(ws);
    T* slots = loss == MM_LOSS_NONE ? nullptr : reinterpret_cast<T*>(static_cast<char*>(ws) + acc_bytes(dtype, n_total, N));
    const T* sr = static_cast<const T*>(scale_raw);
    const T* xs = static_cast<const T*>(x);
    const T* tg = static_cast<const T*>(target);
    if (pairs) {
      LossArgs<T> la{sr, T(alpha), T(eps), terms, slots, loss_params};
      const int r2 = loss == MM_LOSS_STRESS   ? launch_sym<T, N, MM_LOSS_STRESS, true>(xs, tg, n, rb, re, la, acc, n_total, idx, st)
                   : loss == MM_LOSS_QUOTIENT ? launch_sym<T, N, MM_LOSS_QUOTIENT, true>(xs, tg, n, rb, re, la, acc, n_total, idx, st)
                   : squared                  ? launch_sym<T, N, MM_LOSS_NONE, true>(xs, tg, n, rb, re, la, acc, n_total, idx, st)
                                              : launch_sym<T, N, MM_LOSS_NONE, false>(xs, tg, n, rb, re, la, acc, n_total, idx, st);
      if (r2 != MM_OK) return r2;
    }
    so_finalize_kernel<T><<<dim3(unsigned((n_total + 127) / 128)), dim3(128), 0, st>>>(acc, int(n_total), N * N, static_cast<T*>(grad_x),
                                                                                      slots, sr, static_cast<T*>(loss_out));
    MM_CHECK_LAUNCH(); return MM_OK; }))
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
    MM_CHECK_LAUNCH(); return MM_OK; }))
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
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

size_t mm_so_pdist_ws_bytes(int dtype, int64_t n, int N) {
  if (n < 0 || N < 1) return 0;
  return acc_bytes(dtype, n, N);
}

size_t mm_so_pdist_loss_ws_bytes(int dtype, int64_t n, int N) {
  if (n < 0 || N < 1) return 0;
  return acc_bytes(dtype, n, N) + 2 * kLossSlots * (dtype == MM_F64 ? 8 : 4);
}

// The two forwards keep their own order of checks: a null `out` (MM_ERR_ARG) is tested before the 2^20-row limit
// (MM_ERR_UNSUPPORTED) for the full batch and after it for a minibatch, and a call can fail both.
int mm_so_pdist_fwd(int dtype, const void* x, int64_t n, int N, int64_t row_begin, int64_t row_end, int squared, void* out,
                    mm_stream_t stream) {
  const int rc = check_pairs(dtype, x, n, N, n, 1 << 30, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (!out && has_pairs(n, row_begin, row_end)) return MM_ERR_ARG;
  if (row_end <= row_begin) return MM_OK;
  return launch_fwd(dtype, x, n, N, row_begin, row_end, squared, out, n, nullptr, static_cast<hipStream_t>(stream));
}

int mm_so_pdist_fwd_subset(int dtype, const void* x, int64_t n_total, int N, const int64_t* idx, int64_t bs, int64_t row_begin,
                           int64_t row_end, int squared, void* out, mm_stream_t stream) {
  const int rc = check_pairs(dtype, x, n_total, N, bs, 1 << 30, row_begin, row_end);
  if (rc != MM_OK) return rc;
  if (row_tiles(row_begin, row_end) > 65535) return MM_ERR_UNSUPPORTED;
  if (!has_pairs(bs, row_begin, row_end)) return MM_OK;   // (before the null tests or after: they ask for pairs themselves)
  if (!idx || !out) return MM_ERR_ARG;
  return launch_fwd(dtype, x, bs, N, row_begin, row_end, squared, out, n_total, idx, static_cast<hipStream_t>(stream));
}

int mm_so_pdist_bwd(int dtype, const void* x, const void* g, int64_t n, int N, int64_t row_begin, int64_t row_end, int squared,
                    void* grad_x, void* ws, mm_stream_t stream) {
  return pdist_sym(dtype, MM_LOSS_NONE, x, g, nullptr, n, 1 << 30, N, row_begin, row_end, squared, 1.0, 0.0, 0, nullptr, nullptr,
                   grad_x, ws, n, nullptr, false, stream);
}

int mm_so_pdist_bwd_subset(int dtype, const void* x, const void* g, int64_t n_total, int N, const int64_t* idx, int64_t bs,
                           int64_t row_begin, int64_t row_end, int squared, void* grad_x, void* ws, mm_stream_t stream) {
  return pdist_sym(dtype, MM_LOSS_NONE, x, g, nullptr, bs, 1 << 30, N, row_begin, row_end, squared, 1.0, 0.0, 0, nullptr, nullptr,
                   grad_x, ws, n_total, idx, true, stream);
}

int mm_so_pdist_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n, int N,
                     int64_t row_begin, int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                     void* loss_out, void* grad_x, void* ws, mm_stream_t stream) {
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_ARG;
  return pdist_sym(dtype, loss_kind, x, target, scale_raw, n, 1 << 30, N, row_begin, row_end, 1, alpha, eps, terms, loss_params,
                   loss_out, grad_x, ws, n, nullptr, false, stream);
}

// (the nodes of a batch are distinct: bs <= n_total)
int mm_so_pdist_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw, int64_t n_total, int N,
                            const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end, double alpha, double eps, int terms,
                            const double* loss_params, void* loss_out, void* grad_x, void* ws, mm_stream_t stream) {
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_ARG;
  return pdist_sym(dtype, loss_kind, x, dense, scale_raw, bs, n_total, N, row_begin, row_end, 1, alpha, eps, terms, loss_params,
                   loss_out, grad_x, ws, n_total, idx, true, stream);
}

}  // extern "C"
