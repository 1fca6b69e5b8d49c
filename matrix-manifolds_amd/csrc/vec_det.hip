// The bit-deterministic pair gradients of the vector manifolds (vec_det.hpp): C entry points and their instantiations — fp32 and
// fp64 x {Euclidean, Lorentz, sphere} x the 8 padded widths x {upstream gradient (d^2 or d at run time), stress, quotient}, and
// the node-minibatch form of the two losses.  A translation unit of its own: the atomic kernels' instantiations (vec.hip,
// vec_sym.hip, vec_gram.hip) are not touched, and no environment switch is read here.
#include "vec_det.hpp"

using namespace mm;

namespace {

#define MMVD_DISPATCH_MP(m, ...)                            \
  switch (pad_dim(m)) {                                     \
    case 4: { constexpr int MP = 4; return __VA_ARGS__; }   \
    case 8: { constexpr int MP = 8; return __VA_ARGS__; }   \
    case 12: { constexpr int MP = 12; return __VA_ARGS__; } \
    case 16: { constexpr int MP = 16; return __VA_ARGS__; } \
    case 24: { constexpr int MP = 24; return __VA_ARGS__; } \
    case 32: { constexpr int MP = 32; return __VA_ARGS__; } \
    case 48: { constexpr int MP = 48; return __VA_ARGS__; } \
    default: { constexpr int MP = 64; return __VA_ARGS__; } \
  }

#define MMVD_DISPATCH_KIND(kind, ...)                                        \
  switch (kind) {                                                            \
    case MM_EUCLIDEAN: { constexpr int KIND = MM_EUCLIDEAN; __VA_ARGS__ }    \
    case MM_LORENTZ: { constexpr int KIND = MM_LORENTZ; __VA_ARGS__ }        \
    case MM_SPHERE: { constexpr int KIND = MM_SPHERE; __VA_ARGS__ }          \
    default: return MM_ERR_ARG;                                              \
  }

#define MMVD_DISPATCH_T(dtype, ...)                              \
  if ((dtype) == MM_F32) { using T = float; __VA_ARGS__ }        \
  else if ((dtype) == MM_F64) { using T = double; __VA_ARGS__ }  \
  else return MM_ERR_ARG;

bool kind_ok(int kind) { return kind == MM_EUCLIDEAN || kind == MM_LORENTZ || kind == MM_SPHERE; }
bool dtype_ok(int dtype) { return dtype == MM_F32 || dtype == MM_F64; }

// one full-batch call: loss_kind MM_LOSS_NONE (bwd) or a loss
int run_full(int dtype, int kind, int loss_kind, const void* x, const void* g, const void* scale_raw, int64_t n, int m, int64_t rb,
             int64_t re, int squared, double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* grad_x,
             void* det_ws, hipStream_t st) {
  MMVD_DISPATCH_T(dtype, MMVD_DISPATCH_KIND(kind, MMVD_DISPATCH_MP(m, (vec_det::run_t<T, KIND, MP>(
      loss_kind, static_cast<const T*>(x), static_cast<const T*>(g), static_cast<const T*>(scale_raw), n, m, rb, re, squared, alpha,
      eps, terms, loss_params, static_cast<T*>(loss_out), static_cast<T*>(grad_x), det_ws, false, nullptr, n, st)))))
}

}  // namespace

extern "C" {

int mm_vec_pdist_det_geometry(int dtype, int kind, int64_t n, int m, int64_t* chunks, int64_t* rows_per_chunk) {
  if (!dtype_ok(dtype) || !kind_ok(kind) || n < 1 || n > vec_det::kMaxNodes || m < 1 || m > vec_det::kMaxDim || !chunks ||
      !rows_per_chunk)
    return MM_ERR_ARG;
  const vec_det::DetGeometry g = vec_det::geometry(dtype == MM_F64 ? 8 : 4, kind, n, m);
  *chunks = g.chunks;
  *rows_per_chunk = g.rows;
  return MM_OK;
}

size_t mm_vec_pdist_det_ws_bytes(int dtype, int kind, int64_t n, int m) {
  if (n < 1 || m < 1) return 64;
  return std::max<size_t>(64, vec_det::geometry(dtype == MM_F64 ? 8 : 4, kind, n, m).bytes());
}

int mm_vec_pdist_bwd_det(int dtype, int kind, const void* x, const void* g, int64_t n, int m, int64_t row_begin, int64_t row_end,
                         int squared, void* grad_x, void* det_ws, mm_stream_t stream) {
  if (!x || !grad_x || !det_ws || n < 1 || m < 1 || row_begin < 0 || row_end > n || row_begin > row_end || n > (1 << 30) ||
      !dtype_ok(dtype) || !kind_ok(kind))
    return MM_ERR_ARG;
  if (m > vec_det::kMaxDim || n > vec_det::kMaxNodes) return MM_ERR_UNSUPPORTED;
  if (!g && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  return run_full(dtype, kind, MM_LOSS_NONE, x, g, nullptr, n, m, row_begin, row_end, squared, 1.0, 0.0, 0, nullptr, nullptr, grad_x,
                  det_ws, static_cast<hipStream_t>(stream));
}

int mm_vec_pdist_loss_det(int dtype, int kind, int loss_kind, const void* x, const void* target, const void* scale_raw, int64_t n,
                          int m, int64_t row_begin, int64_t row_end, double alpha, double eps, int terms, const double* loss_params,
                          void* loss_out, void* grad_x, void* det_ws, mm_stream_t stream) {
  if (!x || !grad_x || !det_ws || !loss_out || n < 1 || m < 1 || row_begin < 0 || row_end > n || row_begin > row_end ||
      n > (1 << 30) || !dtype_ok(dtype) || !kind_ok(kind))
    return MM_ERR_ARG;
  if (m > vec_det::kMaxDim || n > vec_det::kMaxNodes) return MM_ERR_UNSUPPORTED;
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_UNSUPPORTED;
  if (loss_kind == MM_LOSS_QUOTIENT && !(terms & 3)) return MM_ERR_ARG;
  if (!target && mm_pair_offset(n, row_end) > mm_pair_offset(n, row_begin)) return MM_ERR_ARG;
  return run_full(dtype, kind, loss_kind, x, target, scale_raw, n, m, row_begin, row_end, 1, alpha, eps, terms, loss_params, loss_out,
                  grad_x, det_ws, static_cast<hipStream_t>(stream));
}

int mm_vec_pdist_loss_subset_det(int dtype, int kind, int loss_kind, const void* x, const void* dense, const void* scale_raw,
                                 int64_t n_total, int m, const int64_t* idx, int64_t bs, int64_t row_begin, int64_t row_end,
                                 double alpha, double eps, int terms, const double* loss_params, void* loss_out, void* grad_x,
                                 void* det_ws, mm_stream_t stream) {
  if (!x || !grad_x || !det_ws || !loss_out || n_total < 1 || n_total > (1 << 30) || m < 1 || bs < 0 || bs > n_total ||
      row_begin < 0 || row_end > bs || row_begin > row_end || !dtype_ok(dtype) || !kind_ok(kind))
    return MM_ERR_ARG;
  if (m > vec_det::kMaxDim || bs > vec_det::kMaxNodes) return MM_ERR_UNSUPPORTED;
  if (loss_kind != MM_LOSS_STRESS && loss_kind != MM_LOSS_QUOTIENT) return MM_ERR_UNSUPPORTED;
  if (loss_kind == MM_LOSS_QUOTIENT && !(terms & 3)) return MM_ERR_ARG;
  if ((!dense || !idx) && mm_pair_offset(bs, row_end) > mm_pair_offset(bs, row_begin)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MMVD_DISPATCH_T(dtype, MMVD_DISPATCH_KIND(kind, MMVD_DISPATCH_MP(m, (vec_det::run_t<T, KIND, MP>(
      loss_kind, static_cast<const T*>(x), static_cast<const T*>(dense), static_cast<const T*>(scale_raw), bs, m, row_begin, row_end,
      1, alpha, eps, terms, loss_params, static_cast<T*>(loss_out), static_cast<T*>(grad_x), det_ws, true, idx, n_total, st)))))
}

}  // extern "C"
