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

#include "clear.hpp"
#include "grass_loss.hpp"

namespace mm {
namespace mat {

// (the pair kernel lives in grass_loss.hpp, shared with the node-minibatch instantiations of grass_loss_subset.hip)
template <typename T, int NP, int P, int LOSS>
int launch_loss(const T* x, const T* target, int64_t n, int N, int64_t rb, int64_t re, LossArgs<T> la, T* acc, hipStream_t st) {
  static_assert(loss_form<T, NP, P>() == 1, "only the symmetric form is built");
  const int jb0 = int((rb + 1) / 64);
  const int64_t gx = (n + 63) / 64 - jb0, gy = (re - rb + kLossTI - 1) / kLossTI;
  if (gx <= 0 || gy <= 0) return MM_OK;
  grass_loss_sym_kernel<T, NP, P, LOSS, false><<<dim3(unsigned(gx * gy)), dim3(64), 0, st>>>(x, target, int(n), N, int(rb), int(re),
                                                                                           int(gx), jb0, la, acc, int(n), nullptr);
  MM_CHECK_LAUNCH();
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
  hipError_t e = clear_async(ws, mm_grass_pdist_loss_ws_bytes(dtype, n, N, p), st);   // (a kernel: clear.hpp says why)
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
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

}  // extern "C"
