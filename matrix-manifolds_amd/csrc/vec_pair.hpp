// The inner quantity q of one pair and the padded load of one point, shared by the ordered-pair kernels of the vector manifolds
// (vec.hip: float atomics; vec_det.hpp: none).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mm_manifolds.h"
#include "smallmat.hpp"

namespace mm {

// q for one pair from register/scalar operands
template <typename T, int KIND, int MP, typename TI>
__device__ __forceinline__ T pair_q(const TI (&xi)[MP], const T (&xj)[MP]) {
  using N = Num<T>;
  T q = T(0);
  if (KIND == MM_EUCLIDEAN) {
#pragma unroll
    for (int k = 0; k < MP; ++k) { const T df = xj[k] - xi[k]; q = N::fma(df, df, q); }
  } else if (KIND == MM_LORENTZ) {
#pragma unroll
    for (int k = 1; k < MP; ++k) q = N::fma(xi[k], xj[k], q);
    q = N::fma(xi[0], xj[0], -q);  // -( -x0 y0 + sum x_k y_k )
  } else {
#pragma unroll
    for (int k = 0; k < MP; ++k) q = N::fma(xi[k], xj[k], q);
  }
  return q;
}

template <typename T, int MP>
__device__ __forceinline__ void load_point(const T* __restrict__ x, int64_t idx, int m, T (&r)[MP]) {
#pragma unroll
  for (int k = 0; k < MP; ++k) r[k] = (k < m) ? x[idx * m + k] : T(0);
}

}  // namespace mm
