// The bit-deterministic SPD(d) pair gradients (spd_det.hpp): C entry points and their instantiations, every d = 2 ... 9 in fp32
// and fp64 x {upstream gradient of d^2, of d, stress, quotient}.  A translation unit of its own: compiled in parallel with the
// atomic kernels, whose instantiations it does not touch.
#include "clear.hpp"
#include "spd_det.hpp"

using namespace mm;

namespace {

int det_args_ok(const void* x, const void* ws, const void* det_ws, const void* grad_x, int64_t n, int64_t row_begin, int64_t row_end) {
  return x && ws && det_ws && grad_x && n >= 0 && row_begin >= 0 && row_end <= n && row_begin <= row_end && n <= kSpdMaxNodes;
}

}  // namespace

extern "C" {

int mm_spd_pdist_det_geometry(int dtype, int64_t n, int d, int64_t* chunks, int64_t* rows_per_chunk) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 1 || n > kSpdMaxNodes || d < 2 || d > kSpdMaxD || !chunks || !rows_per_chunk)
    return MM_ERR_ARG;
  const spd_det::DetGeometry g = spd_det::geometry(dtype == MM_F64 ? 8 : 4, n, d);
  *chunks = g.chunks;
  *rows_per_chunk = g.rows;
  return MM_OK;
}

size_t mm_spd_pdist_det_ws_bytes(int dtype, int64_t n, int d) {
  if (n < 1 || d < 1) return 64;
  return std::max<size_t>(64, spd_det::geometry(dtype == MM_F64 ? 8 : 4, n, d).bytes());
}

int mm_spd_pdist_bwd_det(int dtype, const void* x, const void* g, int64_t n, int d, int64_t row_begin, int64_t row_end, int squared,
                         double wmin, double wmax, void* grad_x, void* ws, void* det_ws, int flags, mm_stream_t stream) {
  if (!det_args_ok(x, ws, det_ws, grad_x, n, row_begin, row_end)) return MM_ERR_ARG;
  if (n == 0) return MM_OK;
  if (!g && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MM_DISPATCH(dtype, d,
              (spd_det::run_t<T, D>(MM_LOSS_NONE, static_cast<const T*>(x), static_cast<const T*>(g), static_cast<const T*>(nullptr), n,
                                    row_begin, row_end, squared, 1.0, 0.0, 0, nullptr, wmin, wmax, static_cast<T*>(nullptr),
                                    static_cast<T*>(grad_x), ws, det_ws, flags, st)));
}

int mm_spd_pdist_loss_det(int dtype, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n, int d,
                          int64_t row_begin, int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                          double wmin, double wmax, void* loss_out, void* grad_x, void* ws, void* det_ws, int flags,
                          mm_stream_t stream) {
  if (!det_args_ok(x, ws, det_ws, grad_x, n, row_begin, row_end) || !loss_out) return MM_ERR_ARG;
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_UNSUPPORTED;
  if (loss_kind == MM_LOSS_QUOTIENT && !(terms & 3)) return MM_ERR_ARG;
  if (!target && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    const size_t es = dtype == MM_F64 ? 8 : 4;
    hipError_t e = clear_async(loss_out, 2 * es, st);
    return e == hipSuccess ? MM_OK : int(e);
  }
  MM_DISPATCH(dtype, d,
              (spd_det::run_t<T, D>(loss_kind, static_cast<const T*>(x), static_cast<const T*>(target), static_cast<const T*>(scale_raw),
                                    n, row_begin, row_end, 1, alpha, eps, terms, loss_params, wmin, wmax, static_cast<T*>(loss_out),
                                    static_cast<T*>(grad_x), ws, det_ws, flags, st)));
}

}  // extern "C"
