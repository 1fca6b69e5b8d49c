// launch.hpp — the two one-liners every pair-kernel translation unit needs: where a row's pairs start, and "return the launch error".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mm {
// offset of pair (row, row + 1) in the row-major strict upper triangle of n nodes: mm_pair_offset (common.hip), host and device
__host__ __device__ inline int64_t pair_off(int64_t n, int64_t row) { return row * (2 * n - row - 1) / 2; }
}  // namespace mm

// after a kernel launch, inside a function that returns an mm status: a launch error is returned as it stands
#define MM_CHECK_LAUNCH()                              \
  do {                                                 \
    hipError_t e_ = hipGetLastError();                 \
    if (e_ != hipSuccess) return static_cast<int>(e_); \
  } while (0)
