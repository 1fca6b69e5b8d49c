// clear.hpp — zero-fill of a workspace region as a KERNEL on the caller's stream.
//
// Why not hipMemsetAsync: captured in a graph, the memset node of an entry point cleared its region on the first replay and
// filled it with foreign, non-zero words on every later one (MI355X; tests/test_replay_gpu.py, profiles/replay.md: the
// accumulators of csrc/so.hip, mat.hip, grass_loss.hip, grass_loss_subset.hip, vec.hip, vec_gram.hip, product.hip and
// product_pairs.hip came back as 2.5e35 per element in one run and as small non-zero values in another, eager calls and the
// first replay always right).  A kernel node carries its arguments in the graph and has shown no such behaviour.
//
// THE LIBRARY'S RULE: no memset node, ever, whatever the size of the region — csrc/ calls hipMemsetAsync nowhere.  Every clear
// goes through clear_async, down to the one- and two-word records of an empty table; stereo::subset_clear_kernel, which clears
// several factors' gradients in one launch, is the one clear with a kernel of its own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm {

template <typename W>
__global__ __launch_bounds__(256) void clear_words_kernel(W* __restrict__ p, size_t words) {
  for (size_t k = size_t(blockIdx.x) * 256 + threadIdx.x; k < words; k += size_t(gridDim.x) * 256) p[k] = W(0);
}

// p: 4-byte aligned, bytes: a multiple of 4 (every workspace part of this library is an array of float or double);
// hipErrorInvalidValue otherwise, before anything is launched.  bytes == 0 launches nothing.
inline hipError_t clear_async(void* p, size_t bytes, hipStream_t st) {
  if (bytes == 0) return hipSuccess;
  if (!p || (bytes & 3) || (reinterpret_cast<uintptr_t>(p) & 3)) return hipErrorInvalidValue;
  const size_t words = bytes / 4, blocks = (words + 255) / 256;
  clear_words_kernel<uint32_t><<<dim3(unsigned(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st>>>(static_cast<uint32_t*>(p), words);
  return hipGetLastError();
}

}  // namespace mm
