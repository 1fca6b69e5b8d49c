// Stein-divergence SPD embeddings: the fused objective (loss + gradients in one pass over the pairs) and node minibatches
// inside the pair kernels — SymmetricPositiveDefinite(n, use_stein_div=True), the `spdstein` factor of the reference grid
// (experiments/utils.py:3-40), trained the way the other factors are.  Kernels: spd_stein_loss.hpp; the divergence itself and
// the plain forward / backward: spd_stein.hpp (instantiated by spd.hip).  A translation unit of its own: these
// instantiations compile next to spd.hip / spd_loss.hip / spd_subset.hip.
#include "clear.hpp"
#include "spd_pair.hpp"

namespace mm {

#include "spd_stein.hpp"
#include "spd_stein_loss.hpp"

}  // namespace mm

using namespace mm;

extern "C" {

int mm_spd_stein_pdiv_loss(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n, int d,
                           int64_t row_begin, int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                           double wmin, void* loss_out, void* grad_x, void* ws, int flags, mm_stream_t stream) {
  if (!x || !ws || !grad_x || !loss_out || n < 0 || n > kSpdMaxNodes || row_begin < 0 || row_end > n || row_begin > row_end)
    return MM_ERR_ARG;
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_UNSUPPORTED;
  if (loss_kind == MM_LOSS_QUOTIENT && !(terms & 3)) return MM_ERR_ARG;
  if (!target && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  if (dtype != MM_F32 && dtype != MM_F64) return MM_ERR_ARG;
  if (d < 2 || d > kSpdMaxD) return MM_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    const size_t es = dtype == MM_F64 ? 8 : 4;
    hipError_t e = clear_async(loss_out, 2 * es, st);
    return e == hipSuccess ? MM_OK : int(e);
  }
  MM_DISPATCH(dtype, d,
              (spd_stein_loss_t<T, D, false>(loss_kind, static_cast<const T*>(x), static_cast<const T*>(target),
                                             static_cast<const T*>(scale_raw), n, nullptr, n, row_begin, row_end, alpha, eps, terms,
                                             loss_params, wmin, static_cast<T*>(loss_out), static_cast<T*>(grad_x), ws, flags, st)));
}

int mm_spd_stein_pdiv_loss_subset(int dtype, int loss_kind, const void* x, const void* dense, const void* scale_raw, int64_t n_total,
                                  int d, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end, double alpha,
                                  double eps, int terms, const double* loss_params, double wmin, void* loss_out, void* grad_x,
                                  void* ws, int flags, mm_stream_t stream) {
  if (!x || !ws || !grad_x || !loss_out || n_total < 0 || n_total > kSpdMaxNodes || bs < 0 || bs > n_total || row_begin < 0 ||
      row_end > bs || row_begin > row_end)
    return MM_ERR_ARG;
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_UNSUPPORTED;
  if (loss_kind == MM_LOSS_QUOTIENT && !(terms & 3)) return MM_ERR_ARG;
  if ((!dense || !idx) && mm_pair_offset(bs, row_end) > mm_pair_offset(bs, row_begin)) return MM_ERR_ARG;
  if (dtype != MM_F32 && dtype != MM_F64) return MM_ERR_ARG;
  if (d < 2 || d > kSpdMaxD) return MM_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_total == 0) {
    const size_t es = dtype == MM_F64 ? 8 : 4;
    hipError_t e = clear_async(loss_out, 2 * es, st);
    return e == hipSuccess ? MM_OK : int(e);
  }
  MM_DISPATCH(dtype, d,
              (spd_stein_loss_t<T, D, true>(loss_kind, static_cast<const T*>(x), static_cast<const T*>(dense),
                                            static_cast<const T*>(scale_raw), n_total, idx, bs, row_begin, row_end, alpha, eps, terms,
                                            loss_params, wmin, static_cast<T*>(loss_out), static_cast<T*>(grad_x), ws, flags, st)));
}

int mm_spd_stein_pdiv_fwd_subset(int dtype, const void* x, int64_t n_total, int d, const int64_t* idx, int64_t bs, int64_t row_begin,
                                 int64_t row_end, int squared, double wmin, void* out, void* ws, int flags, mm_stream_t stream) {
  if (!x || !ws || n_total < 0 || n_total > kSpdMaxNodes || bs < 0 || bs > n_total || row_begin < 0 || row_end > bs ||
      row_begin > row_end)
    return MM_ERR_ARG;
  if ((!out || !idx) && mm_pair_offset(bs, row_end) > mm_pair_offset(bs, row_begin)) return MM_ERR_ARG;
  if (dtype != MM_F32 && dtype != MM_F64) return MM_ERR_ARG;
  if (d < 2 || d > kSpdMaxD) return MM_ERR_UNSUPPORTED;
  if (n_total == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MM_DISPATCH(dtype, d,
              (spd_stein_fwd_subset_t<T, D>(static_cast<const T*>(x), n_total, idx, bs, row_begin, row_end, squared, wmin,
                                            static_cast<T*>(out), ws, flags, st)));
}

int mm_spd_stein_pdiv_bwd_subset(int dtype, const void* x, const void* g, int64_t n_total, int d, const int64_t* idx, int64_t bs,
                                 int64_t row_begin, int64_t row_end, int squared, double wmin, void* grad_x, void* ws, int flags,
                                 mm_stream_t stream) {
  if (!x || !ws || !grad_x || n_total < 0 || n_total > kSpdMaxNodes || bs < 0 || bs > n_total || row_begin < 0 || row_end > bs ||
      row_begin > row_end)
    return MM_ERR_ARG;
  if ((!g || !idx) && mm_pair_offset(bs, row_end) > mm_pair_offset(bs, row_begin)) return MM_ERR_ARG;
  if (dtype != MM_F32 && dtype != MM_F64) return MM_ERR_ARG;
  if (d < 2 || d > kSpdMaxD) return MM_ERR_UNSUPPORTED;
  if (n_total == 0) return MM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MM_DISPATCH(dtype, d,
              (spd_stein_bwd_subset_t<T, D>(static_cast<const T*>(x), static_cast<const T*>(g), n_total, idx, bs, row_begin, row_end,
                                            squared, wmin, static_cast<T*>(grad_x), ws, flags, st)));
}

}  // extern "C"
