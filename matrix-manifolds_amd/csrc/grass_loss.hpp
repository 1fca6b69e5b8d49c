// The pair kernel of the fused Grassmann objective, instantiated for the full batch (grass_loss.hip, SUB = false) and for node
// minibatches (grass_loss_subset.hip, SUB = true); the scheme is described at the head of grass_loss.hip.  (The kernel itself
// carries SUB: as a device function called from two kernels the body compiled to different registers in eight instantiations.)  With SUB the pairs are
// those of the BATCH POSITIONS 0 .. n (n = bs) and three things change: the row's node id is the wave-uniform idx[i], the lane's
// is idx[j], and the target is dense[node_i][node_j].  The accumulators are addressed by NODE (acc [N*p][n_total]), so the
// finalize launch over n_total writes the dense gradient, zero rows included.
#pragma once
#include <hip/hip_runtime.h>

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

// node id of batch position `pos`: the low 32 bits of the index, clamped into the table
__device__ __forceinline__ int loss_node_of(const int64_t* __restrict__ idx, int pos, int n_total) {
  return min(max(int(idx[pos]), 0), n_total - 1);
}

// n: the number of points whose pairs are walked (SUB: the batch size); n_total, idx: SUB only (the table's rows, the batch's nodes)
template <typename T, int NP, int P, int LOSS, bool SUB>
__global__ __launch_bounds__(64) void grass_loss_sym_kernel(const T* __restrict__ x, const T* __restrict__ target, int n, int N,
                                                            int row_begin, int row_end, int gx, int jb0, LossArgs<T> la,
                                                            T* __restrict__ acc /* [N*P][n or n_total] */, int n_total,
                                                            const int64_t* __restrict__ idx) {
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
  // (SUB: the lane's node id is not kept across the row loop — it is re-read where it is needed, one cached load per row, so
  // that the instantiations at the register limit keep their accumulators in registers)
  if constexpr (SUB) load<T, NP, P>(x + size_t(loss_node_of(idx, jin ? j : 0, n_total)) * N * P, N, xj);
  else load<T, NP, P>(x + size_t(jin ? j : 0) * N * P, N, xj);
#pragma unroll
  for (int r = 0; r < NP; ++r)
#pragma unroll
    for (int c = 0; c < P; ++c) a[r][c] = T(0);
  T loss_acc = T(0), ds_acc = T(0);
  const int64_t base = SUB ? 0 : pair_off(n, row_begin);
  const int ilast = min(i1, jbase + 63);   // rows from here on have no column in this block
  for (int i = i0; i < ilast; ++i) {
    T xi[NP][P], gm[P][P], dg[P][P];
    int ni = i;
    if constexpr (SUB) ni = __builtin_amdgcn_readfirstlane(loss_node_of(idx, i, n_total));
    load<T, NP, P>(x + size_t(ni) * N * P, N, xi);  // wave-uniform -> scalar loads
    const bool valid = jin && j > i;
    T tg = T(1);
    if (valid) {
      if constexpr (SUB) tg = target[size_t(ni) * size_t(n_total) + size_t(loss_node_of(idx, j, n_total))];
      else tg = target[pair_off(n, i) - base + (j - i - 1)];
    }
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
  const int na = SUB ? n_total : n;   // accumulator stride
  {
    const int np = N * P, cnt = (ilast - i0) * np;   // (rows r >= N of the padded point are not flushed)
    for (int t = lane; t < cnt; t += 64) {
      const int il = t / np, k = t - il * np;
      const int row = SUB ? loss_node_of(idx, i0 + il, n_total) : i0 + il;
      atomic_add(&acc[size_t(k) * na + row], red[il][k]);
    }
  }
  if (jin) {
    const int col = SUB ? loss_node_of(idx, j, n_total) : j;
#pragma unroll
    for (int r = 0; r < NP; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c)
        if (r < N) atomic_add(&acc[size_t(r * P + c) * na + col], a[r][c]);
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

}  // namespace mat
}  // namespace mm
