// The fused Grassmann objective for a NODE MINIBATCH (mm_grass_pdist_loss_subset): the pair kernel of grass_loss.hpp with SUB —
// the points of the step are rows idx[0..bs) of the full table, the target of batch pair (a, b) is dense[idx[a]][idx[b]], and
// the sums land in accumulators addressed by node, acc [N*p][n_total].  A step is the clear kernel over the workspace (clear.hpp), the pair kernel
// over the batch's tiles and the full-batch finalize launch over n_total, which writes the whole dense gradient: rows outside
// the batch come out as the +0 the clear kernel left.  No gather, no scatter-add, no zero fill.  The price is the column side's
// atomics, which are scattered over the node ids instead of 64 consecutive addresses (one per value and tile, as before).
// A translation unit of its own, so that the library's build stays parallel.
//
// Every (T, NP, P) is built: with the lane's node id re-read where it is needed (grass_loss.hpp) none has scratch — see
// profiles/grass_minibatch.md for the registers.  subset_form() is the way out the full-batch table has: an instantiation
// marked 0 is not built and reports MM_ERR_UNSUPPORTED.
#include <hip/hip_runtime.h>

#include <climits>

#include "clear.hpp"
#include "grass_loss.hpp"

namespace mm {
namespace mat {

// 1: the subset instantiation is built; 0: it is not (scratch between the first and the last row of a tile)
template <typename T, int NP, int P> constexpr int subset_form() { return 1; }

template <typename T, int NP, int P, int LOSS>
int launch_subset(const T* x, const T* dense, int64_t n_total, const int64_t* idx, int64_t bs, int N, int64_t rb, int64_t re,
                  LossArgs<T> la, T* acc, hipStream_t st) {
  if constexpr (subset_form<T, NP, P>() == 1) {
    const int jb0 = int((rb + 1) / 64);
    const int64_t gx = (bs + 63) / 64 - jb0, gy = (re - rb + kLossTI - 1) / kLossTI;
    if (gx <= 0 || gy <= 0) return MM_OK;
    grass_loss_sym_kernel<T, NP, P, LOSS, true><<<dim3(unsigned(gx * gy)), dim3(64), 0, st>>>(x, dense, int(bs), N, int(rb), int(re),
                                                                                         int(gx), jb0, la, acc, int(n_total), idx);
    MM_CHECK_LAUNCH();
    return MM_OK;
  } else {
    return MM_ERR_UNSUPPORTED;
  }
}

}  // namespace mat
}  // namespace mm

using namespace mm;
using namespace mm::mat;

extern "C" {

int mm_grass_pdist_loss_subset_form(int dtype, int N, int p) {
  if (N < 1 || p < 1 || p > N) return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, { return subset_form<T, NP, P>() == 1 ? 1 : MM_ERR_UNSUPPORTED; }))
}

int mm_grass_pdist_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw, int64_t n_total,
                               int N, int p, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end, double alpha,
                               double eps, int terms, const double* loss_params, void* loss_out, void* grad_x, void* ws,
                               mm_stream_t stream) {
  if (!x || !grad_x || !ws || !loss_out || n_total < 1 || N < 1 || p < 1 || p > N || bs < 0 || bs > n_total || row_begin < 0 ||
      row_end > bs || row_begin > row_end || n_total > (1 << 30) || (dtype != MM_F32 && dtype != MM_F64) ||
      (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT))
    return MM_ERR_ARG;
  if (N > 9 || p > 4) return MM_ERR_UNSUPPORTED;
  const int form = mm_grass_pdist_loss_subset_form(dtype, N, p);
  if (form != 1) return form;
  // (the tiles are numbered in one grid dimension)
  if (((bs + 63) / 64) * ((row_end - row_begin + kLossTI - 1) / kLossTI) > INT32_MAX) return MM_ERR_UNSUPPORTED;
  const bool pairs = bs >= 2 && mm_pair_offset(bs, row_end) > mm_pair_offset(bs, row_begin);
  if (pairs && (!dense || !idx)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = clear_async(ws, mm_grass_pdist_loss_ws_bytes(dtype, n_total, N, p), st);   // (a kernel: clear.hpp says why)
  if (e != hipSuccess) return int(e);
  MMM_DISPATCH_T(dtype, MMM_DISPATCH_NP_P(N, p, {
    T* acc = static_cast<T*>(ws);
    T* slots = reinterpret_cast<T*>(static_cast<char*>(ws) + loss_acc_bytes(dtype, n_total, N, p));
    const T* sr = static_cast<const T*>(scale_raw);
    if (pairs) {
      LossArgs<T> la{sr, T(alpha), T(eps), terms, slots, loss_params};
      const int rc = loss_kind == MM_LOSS_STRESS
          ? launch_subset<T, NP, P, MM_LOSS_STRESS>(static_cast<const T*>(x), static_cast<const T*>(dense), n_total, idx, bs, N, row_begin, row_end, la, acc, st)
          : launch_subset<T, NP, P, MM_LOSS_QUOTIENT>(static_cast<const T*>(x), static_cast<const T*>(dense), n_total, idx, bs, N, row_begin, row_end, la, acc, st);
      if (rc != MM_OK) return rc;
    }
    grass_loss_finalize_kernel<T><<<dim3(unsigned((n_total + 127) / 128)), dim3(128), 0, st>>>(acc, int(n_total), N * p,
                                                                                              static_cast<T*>(grad_x), slots, sr,
                                                                                              static_cast<T*>(loss_out));
    MM_CHECK_LAUNCH(); return MM_OK; }))
}

}  // extern "C"
