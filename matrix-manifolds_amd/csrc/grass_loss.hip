// Fused objective of a Grassmann embedding: loss(target, softplus(scale) * pdist(x)^2) and ALL its gradients from one pass
// over the pairs (mm_grass_pdist_loss) — no pair vector of distances or upstream gradients, and the p x p SVD of a pair runs
// once (the per-factor route runs it in the forward and, for both orders of the pair, in the backward).
//
// Form 1 (symmetric, every instantiation): every unordered pair (i, j), row_begin <= i < row_end, j > i, is visited once.  A lane owns column j
// and keeps x_j and its column sums in registers; the row point x_i is wave-uniform (scalar loads).  From the pair's single
// dG (grass_pair, mat_common.hpp) and w = dloss/dm * softplus(s):
//   column side  acc_j += w x_i dG      in registers, down the row tile; one atomic per value and tile at its end;
//   row side     w x_j dG^T             summed across the wavefront by the transposing reduction of smallmat.hpp, a group
//                                       of matrix rows at a time (all of them in fp32, one row in fp64), parked in LDS and
//                                       flushed with one atomic per value and row at the end of the tile.
// Form 0 (every ordered pair, a lane accumulates only its own column: the scheme of grass_pdist_bwd_kernel) is the way out for
// an instantiation whose form 1 needs scratch.  None does — compiled with the library's flags the widest, <double, 9, 4> and
// <double, 6, 4>, sit at 256 vector registers with 6 values parked in accumulation registers and 0 bytes of scratch — so the
// table below holds no 0 and no form-0 kernel is built.
// The sums go into the transposed workspace acc [N*p][n] (cleared at the head of the call, as mm_grass_pdist_bwd does) and
// the 2 x 256 loss slots of loss.hpp; a finalize launch writes grad_x and the loss record.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/mm_manifolds.h"
#include "loss.hpp"
#include "mat_common.hpp"
#include "smallmat.hpp"

namespace mm {
namespace mat {

constexpr int kLossTI = 16;    // rows per tile (one wavefront per workgroup)

// Which form an instantiation takes (reported by mm_grass_pdist_loss_form): 1 = symmetric; 0 would be the ordered scheme.
template <typename T, int NP, int P> constexpr int loss_form() { return 1; }
// matrix rows per transposing reduction (form 1)
template <typename T, int NP> constexpr int group_rows() { return sizeof(T) == 4 ? NP : 1; }

template <typename T, int NP, int P, int LOSS>
__global__ __launch_bounds__(64) void grass_loss_sym_kernel(const T* __restrict__ x, const T* __restrict__ target, int n, int N,
                                                            int row_begin, int row_end, int gx, int jb0, LossArgs<T> la,
                                                            T* __restrict__ acc /* [N*P][n] */) {
  using Nm = Num<T>;
  constexpr int TI = kLossTI, GR = group_rows<T, NP>(), GV = GR * P;
  static_assert(NP % GR == 0, "whole groups");
  __shared__ T red[TI][NP * P];
  const int lane = threadIdx.x;
  const int by = int(blockIdx.x) / gx, bx = int(blockIdx.x) - by * gx;
  const int i0 = row_begin + by * TI, i1 = min(i0 + TI, row_end);
  const int jbase = (jb0 + bx) * 64;   // (< n: gx = ceil(n / 64) - jb0)
  if (jbase + 63 <= i0) return;        // no column right of the tile's first row, so of none of its rows
  loss_resolve<T, LOSS>(la);
  const T sp = softplus_of(la.scale_raw);
  const int j = jbase + lane;
  const bool jin = j < n;
  bool writer;
  const int slot = reduce_slot<GV>(lane, writer);
  T xj[NP][P], a[NP][P];
  load<T, NP, P>(x + size_t(jin ? j : 0) * N * P, N, xj);
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) a[r][c] = T(0);
  T loss_acc = T(0), ds_acc = T(0);
  const int64_t base = moff(n, row_begin);
  const int ilast = min(i1, jbase + 63);   // rows from here on have no column in this block
  for (int i = i0; i < ilast; ++i) {
    T xi[NP][P], gm[P][P], dg[P][P];
    load<T, NP, P>(x + size_t(i) * N * P, N, xi);  // wave-uniform -> scalar loads
    const bool valid = jin && j > i;
    T tg = T(1);
    if (valid) tg = target[moff(n, i) - base + (j - i - 1)];
    gram<T, NP, P>(xi, xj, gm);  // x_i^T x_j ; d/dx_j = x_i dG, d/dx_i = x_j dG^T
    const T v = grass_pair<T, P, true>(gm, dg);
    T dldm;
    const T l = loss_term<T, LOSS>(sp * v, tg, la, dldm);
    loss_acc += valid ? l : T(0);
    ds_acc += valid ? dldm * v : T(0);
    const T w = valid ? dldm * sp : T(0);
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c) {
        T s = T(0);
#pragma unroll
        for (int k = 0; k < P; ++k) s = Nm::fma(xi[r][k], dg[k][c], s);
        a[r][c] = Nm::fma(w, s, a[r][c]);
      }
#pragma unroll
    for (int g = 0; g < NP / GR; ++g) {
      T rs[GV];
#pragma unroll
      for (int rr = 0; rr < GR; ++rr)
#pragma unroll
        for (int c = 0; c < P; ++c) {
          T s = T(0);
#pragma unroll
          for (int k = 0; k < P; ++k) s = Nm::fma(xj[g * GR + rr][k], dg[c][k], s);
          rs[rr * P + c] = w * s;
        }
      const T tot = wave_reduce_transposed<GV, T>(rs, lane);
      if (writer) red[i - i0][g * GV + slot] = tot;
    }
  }
  __builtin_amdgcn_wave_barrier();
  {
    const int np = N * P, cnt = (ilast - i0) * np;   // (rows r >= N of the padded point are not flushed)
    for (int t = lane; t < cnt; t += 64) {
      const int il = t / np, k = t - il * np;
      atomic_add(&acc[size_t(k) * n + (i0 + il)], red[il][k]);
    }
  }
  if (jin) {
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c)
        if (r < N) atomic_add(&acc[size_t(r * P + c) * n + j], a[r][c]);
  }
  const T ls = wave_sum(loss_acc), dd = wave_sum(ds_acc);
  if (lane == 0) {
    const int s = blockIdx.x & (kLossSlots - 1);
    atomic_add(&la.slots[s], ls);
    atomic_add(&la.slots[kLossSlots + s], dd);
  }
}

// grad [n][np] from the transposed accumulators; the first wavefront of block 0 closes the loss record
template <typename T>
__global__ __launch_bounds__(128) void grass_loss_finalize_kernel(const T* __restrict__ acc, int n, int np, T* __restrict__ grad,
                                                                  T* __restrict__ slots, const T* __restrict__ scale_raw,
                                                                  T* __restrict__ loss_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n)
    for (int k = 0; k < np; ++k) grad[size_t(j) * np + k] = acc[size_t(k) * n + j];
  if (blockIdx.x == 0 && threadIdx.x < 64) loss_finalize<T>(slots, scale_raw, loss_out);
}

inline size_t loss_acc_bytes(int dtype, int64_t n, int N, int p) {
  const size_t b = (dtype == MM_F64 ? 8 : 4) * size_t(n) * size_t(N) * size_t(p);
  return (b + 255) & ~size_t(255);
}

template <typename T, int NP, int P, int LOSS>
int launch_loss(const T* x, const T* target, int64_t n, int N, int64_t rb, int64_t re, LossArgs<T> la, T* acc, hipStream_t st) {
  static_assert(loss_form<T, NP, P>() == 1, "only the symmetric form is built");
  const int jb0 = int((rb + 1) / 64);
  const int64_t gx = (n + 63) / 64 - jb0, gy = (re - rb + kLossTI - 1) / kLossTI;
  if (gx <= 0 || gy <= 0) return MM_OK;
  grass_loss_sym_kernel<T, NP, P, LOSS><<<dim3(unsigned(gx * gy)), dim3(64), 0, st>>>(x, target, int(n), N, int(rb), int(re),
                                                                                    int(gx), jb0, la, acc);
  MMM_CHECK();
  return MM_OK;
}

}  // namespace mat
}  // namespace mm

using namespace mm;
using namespace mm::mat;

extern "C" {

size_t mm_grass_pdist_loss_ws_bytes(int dtype, int64_t n, int N, int p) {
  if (n < 0 || N < 1 || p < 1) return 0;
  return loss_acc_bytes(dtype, n, N, p) + 2 * kLossSlots * (dtype == MM_F64 ? 8 : 4);
}

int mm_grass_pdist_loss_form(int dtype, int N, int p) {
  if (N < 1 || p < 1 || p > N) return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, { return loss_form<T, NP, P>(); }))
}

int mm_grass_pdist_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n, int N,
                        int p, int64_t row_begin, int64_t row_end, double alpha, double eps, int terms,
                        const double* loss_params, void* loss_out, void* grad_x, void* ws, mm_stream_t stream) {
  if (!x || !grad_x || !ws || !loss_out || n < 1 || N < 1 || p < 1 || p > N || row_begin < 0 || row_end > n ||
      row_begin > row_end || n > (1 << 30) || (dtype != MM_F32 && dtype != MM_F64) ||
      (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT))
    return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  // (the tiles are numbered in one grid dimension)
  if (((n + 63) / 64) * ((row_end - row_begin + kLossTI - 1) / kLossTI) > INT32_MAX) return MM_ERR_UNSUPPORTED;
  const bool pairs = mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin);
  if (!target && pairs) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(ws, 0, mm_grass_pdist_loss_ws_bytes(dtype, n, N, p), st);
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    T* acc = static_cast<T*>(ws);
    T* slots = reinterpret_cast<T*>(static_cast<char*>(ws) + loss_acc_bytes(dtype, n, N, p));
    const T* sr = static_cast<const T*>(scale_raw);
    if (pairs) {
      LossArgs<T> la{sr, T(alpha), T(eps), terms, slots, loss_params};
      const int rc = loss_kind == MM_LOSS_STRESS
          ? launch_loss<T, NP, P, MM_LOSS_STRESS>(static_cast<const T*>(x), static_cast<const T*>(target), n, N, row_begin, row_end, la, acc, st)
          : launch_loss<T, NP, P, MM_LOSS_QUOTIENT>(static_cast<const T*>(x), static_cast<const T*>(target), n, N, row_begin, row_end, la, acc, st);
      if (rc != MM_OK) return rc;
    }
    grass_loss_finalize_kernel<T><<<dim3(unsigned((n + 127) / 128)), dim3(128), 0, st>>>(acc, int(n), N * p, static_cast<T*>(grad_x),
                                                                                        slots, sr, static_cast<T*>(loss_out));
    MMM_CHECK(); return MM_OK; }))
}

}  // extern "C"
