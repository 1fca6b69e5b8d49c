// Vector-manifold pair gradients (Euclidean, Lorentz, sphere) WITHOUT float atomics: the bit-deterministic mode next to
// vec_pdist_bwd_kernel (vec.hip), vec_pdist_bwd_sym_kernel (vec_sym.hpp) and the matrix-core forms (vec_gram.hip).  The form, the
// loss record and the determinism contract are det_common.hpp's; this file holds what is the vector manifolds' own.
//
// A lane keeps x_j, a[MP] and wsum in registers; the row operand is read with scalar loads (LDS staging for a node minibatch).
// Per pair the ordered twin's arithmetic, unchanged: pair_q, PairFn::dq / ::value, loss_term, w, a[k] = fma(w, x_i[k], a[k]),
// upstream gradients fetched UNR rows ahead.  A node's chunk record holds the entries k < m, plus wsum for the Euclidean kind; the
// finalize kernel applies the manifold map of vec_pdist_finalize_kernel.  Every order of summation is a pure function of
// (dtype, kind, n, m): geometry() below.  All offsets are 64-bit, as in the twin.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/mm_manifolds.h"
#include "clear.hpp"
#include "det_common.hpp"
#include "launch.hpp"
#include "smallmat.hpp"
#include "loss.hpp"
#include "vecfn.hpp"
#include "vec_pair.hpp"

namespace mm {
namespace vec_det {

using det::DetGeometry;
using det::kCols;
using det::kWaves;
constexpr int kStageRows = 64;                   // node minibatch: rows of a chunk staged in LDS at a time
constexpr int kMaxDim = 64;                      // mm_vec_max_dim()
constexpr int64_t kMaxNodes = int64_t(1) << 22;
constexpr int kNodeBlock = 128;                  // finalize: nodes per workgroup

// entries of a node's chunk record: the m coefficient sums, and the sum of the weights where the map needs it
constexpr int entries_of(int kind, int m) { return m + (kind == MM_EUCLIDEAN ? 1 : 0); }
// rows per chunk: a multiple of det::kMinRows, the unroll of the row walk
inline DetGeometry geometry(size_t esz, int kind, int64_t n, int m) {
  return det::geometry(esz, size_t(entries_of(kind, m)) * esz, n, det::kMinRows);
}

// (node ids of a minibatch are clamped into the table: unvalidated caller data, as in the twin)
__device__ __forceinline__ int batch_node(const int64_t* __restrict__ idx, int pos, int n_total) {
  return int(min(uint64_t(idx[pos]), uint64_t(n_total - 1)));
}

// ---- the pair kernel ------------------------------------------------------------------------------------------------------------
// grid (groups, chunks); workgroup (x, y): columns [kCols x, kCols x + kCols), rows [rows y, rows y + rows) of ALL n rows.
// A pair (i, j) is live iff i != j, j < n and row_begin <= min(i, j) < row_end; its upstream gradient / target sits at
// pair_off(min) - base + (max - min - 1) of `g` (64-bit) — SUB: at dense[node(min)][node(max)], min / max by POSITION.  A dead
// pair adds w = 0.  slab [chunks][E][n], E = entries_of(KIND, m); slots [2][groups * chunks].  LOSS == MM_LOSS_NONE: `g` =
// upstream gradients, `squared` applies; else `g` = targets.
// SUB (a node minibatch): the n points of the launch are the nodes idx[0 .. n) of a table of n_total points; slab and slots are
// addressed by batch POSITION, with the geometry of a full batch of n points.
template <typename T, int KIND, int MP, int LOSS, bool SUB>
__global__ __launch_bounds__(kCols) void pair_kernel(const T* __restrict__ x, const T* __restrict__ g, int n, int m, int row_begin,
                                                     int row_end, int squared, int rows, T* __restrict__ slab, T* __restrict__ slots,
                                                     LossArgs<T> la, const int64_t* __restrict__ idx, int n_total) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the row operands stay scalar loads
  const int chunk = blockIdx.y;
  const int bc0 = int(blockIdx.x) * kCols;
  // the columns whose rows are cut together: the wavefront's; SUB: the workgroup's (its wavefronts meet at barriers)
  const int c0 = SUB ? bc0 : bc0 + wave * 64;
  const int c1 = min(c0 + (SUB ? kCols : 64), n);   // (c0 >= n: a wavefront beyond the last column walks nothing)
  const int j = bc0 + int(threadIdx.x);
  const bool jin = j < n;
  const int jn = SUB ? batch_node(idx, jin ? j : 0, n_total) : (jin ? j : 0);   // the column's node
  T xj[MP], a[MP];
  load_point<T, MP>(x, jn, m, xj);
#pragma unroll
  for (int k = 0; k < MP; ++k) a[k] = T(0);
  T wsum = T(0), sp = T(1), loss_acc = T(0), ds_acc = T(0);
  loss_resolve<T, LOSS>(la);
  if constexpr (LOSS != MM_LOSS_NONE) sp = softplus_of(la.scale_raw);
  // rows of the chunk that can hold a live pair for these columns: none below row_begin (min(i, j) >= row_begin needs
  // i >= row_begin), none at all if every column is below row_begin or beyond n, and none from row_end on if every column is at
  // or beyond row_end (then min(i, j) >= row_end)
  const int r0 = chunk * rows, r1 = min(r0 + rows, n);
  int lo = max(r0, row_begin), hi = r1;
  if (c0 >= row_end) hi = min(hi, row_end);
  if (c1 <= row_begin || c0 >= n) hi = lo;
  const int64_t base = pair_off(n, row_begin);
  const bool jown = jin && j >= row_begin && j < row_end;          // pairs (j, i > j) belong to this row range (i >= row_begin: the walk starts there)
  const int64_t gcol = SUB ? int64_t(0) : pair_off(n, j) - base - j - 1;   // pair (i, j), i > j: g[gcol + i]
  constexpr int kLdsRows = SUB ? kStageRows : 1;
  __shared__ T rowx[kLdsRows][SUB ? MP : 1];
  __shared__ int rown[kLdsRows];
  // The per-pair arithmetic is far too short to hide the latency of the load of g it depends on, so the upstream gradients of UNR
  // rows are fetched as one batch first (the twin's).
  constexpr int UNR = 8;
  for (int t0 = lo; t0 < hi; t0 += kStageRows) {
    const int t1 = SUB ? min(t0 + kStageRows, hi) : hi;
    if constexpr (SUB) {   // the rows' node ids with one request, all their points with one more (workgroup-uniform trip counts)
      __syncthreads();
      if (int(threadIdx.x) < t1 - t0) rown[threadIdx.x] = batch_node(idx, t0 + int(threadIdx.x), n_total);
      __syncthreads();
      for (int e = threadIdx.x; e < (t1 - t0) * MP; e += kCols) {
        const int r = e / MP, k = e % MP;
        rowx[r][k] = k < m ? x[size_t(rown[r]) * m + k] : T(0);
      }
      __syncthreads();
    }
    for (int ib = t0; ib < t1; ib += UNR) {
      T wv[UNR];
      bool ok[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int i = ib + u;
        // (one test, written twice: the register allocator keeps every instantiation free of spills with the form it gets here)
        const bool valid = SUB ? i < t1 && (i < j ? jin && i < row_end : jown && i > j)
                               : jin && j >= row_begin && i < t1 && i != j && min(i, j) < row_end;
        ok[u] = valid;
        int64_t off;
        if constexpr (SUB) {   // dense[node(lo)][node(hi)]: the row's node is wave-uniform, the column's is in a register
          const int64_t in_ = int64_t(rown[min(i, t1 - 1) - t0]);
          off = i < j ? in_ * int64_t(n_total) + int64_t(jn) : int64_t(jn) * int64_t(n_total) + in_;
        } else {
          const int64_t grow = pair_off(n, i) - base - i - 1;   // wave-uniform; pair (i, j), i < j: g[grow + j]
          off = i < j ? grow + j : gcol + i;
        }
        wv[u] = valid ? g[off] : T(0);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int i = min(ib + u, t1 - 1);  // (rows past the range carry wv = 0)
        T xi[MP];
        if constexpr (SUB) {
#pragma unroll
          for (int k = 0; k < MP; ++k) xi[k] = rowx[i - t0][k];   // (same address in every lane: LDS broadcast)
        } else {
          load_point<T, MP>(x, i, m, xi);
        }
        const T q = pair_q<T, KIND, MP>(xi, xj);
        T w;
        if constexpr (LOSS == MM_LOSS_NONE) {
          w = ok[u] ? wv[u] * PairFn<T, KIND>::dq(q, squared) : T(0);
        } else {
          const T d2 = PairFn<T, KIND>::value(q, 1);
          T dldm;
          const T l = loss_term<T, LOSS>(sp * d2, wv[u], la, dldm);
          const bool once = ok[u] && ib + u < j;
          loss_acc += once ? l : T(0);
          ds_acc += once ? dldm * d2 : T(0);
          w = ok[u] ? dldm * sp * PairFn<T, KIND>::dq(q, 1) : T(0);
        }
        wsum += w;
#pragma unroll
        for (int k = 0; k < MP; ++k) a[k] = Num<T>::fma(w, xi[k], a[k]);
      }
    }
  }
  if (jin) {
    const int ne = entries_of(KIND, m);
    T* rec = slab + size_t(chunk) * size_t(ne) * size_t(n) + size_t(j);
#pragma unroll
    for (int k = 0; k < MP; ++k)
      if (k < m) rec[size_t(k) * size_t(n)] = a[k];
    if (KIND == MM_EUCLIDEAN) rec[size_t(m) * size_t(n)] = wsum;
  }
  if constexpr (LOSS != MM_LOSS_NONE) {
    __shared__ T lossW[kWaves][2];
    const T l = wave_sum(loss_acc), dd = wave_sum(ds_acc);
    if (lane == 0) { lossW[wave][0] = l; lossW[wave][1] = dd; }
    __syncthreads();
    if (threadIdx.x == 0) {
      T ls = lossW[0][0], ds = lossW[0][1];
#pragma unroll
      for (int wq = 1; wq < kWaves; ++wq) { ls += lossW[wq][0]; ds += lossW[wq][1]; }
      const size_t nslots = size_t(gridDim.x) * gridDim.y;
      const size_t slot = size_t(blockIdx.y) * gridDim.x + blockIdx.x;
      slots[slot] = ls;
      slots[nslots + slot] = ds;
    }
  }
}

// ---- finalize: one thread per node -------------------------------------------------------------------------------------------
// The node's chunk records added in chunk order, in T; then the manifold map of vec_pdist_finalize_kernel: 2 (x_j sum w -
// sum w x_i) for the Euclidean kind, -J for Lorentz, identity for the sphere.  chunks == 0 (no pair launch): zero gradient, zero
// loss record.  idx != null (a node minibatch): thread p owns batch position p and writes row idx[p] of the table's gradient —
// ONE plain store per batch row, the rows outside the batch were cleared (clear_async) before the launch.
template <typename T, int KIND, int MP>
__global__ __launch_bounds__(kNodeBlock) void finalize_kernel(const T* __restrict__ x, const T* __restrict__ slab, int n, int m, int chunks,
                                                               T* __restrict__ grad, const T* __restrict__ slots, int64_t nslots,
                                                               const T* __restrict__ scale_raw, T* __restrict__ loss_out,
                                                               const int64_t* __restrict__ idx, int n_total) {
  if (loss_out && blockIdx.x == 0 && threadIdx.x < 64) {
    double l = 0.0, d = 0.0;
    for (int64_t t = threadIdx.x; t < nslots; t += 64) { l += double(slots[t]); d += double(slots[nslots + t]); }
    l = wave_sum(l);
    d = wave_sum(d);
    if (threadIdx.x == 0) {
      const double v = scale_raw ? double(*scale_raw) : 0.0;
      loss_out[0] = T(l);
      loss_out[1] = scale_raw ? T(d / (1.0 + ::exp(-v))) : T(0);   // d softplus = sigmoid
    }
  }
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int ne = entries_of(KIND, m);
  const size_t jn = idx ? size_t(batch_node(idx, j, n_total)) : size_t(j);
  T ws = T(0);
  if (KIND == MM_EUCLIDEAN) {
    for (int c = 0; c < chunks; ++c) ws += slab[(size_t(c) * size_t(ne) + size_t(m)) * size_t(n) + size_t(j)];
  }
  for (int k = 0; k < m; ++k) {
    T s = T(0);
    for (int c = 0; c < chunks; ++c) s += slab[(size_t(c) * size_t(ne) + size_t(k)) * size_t(n) + size_t(j)];
    T r;
    if (KIND == MM_EUCLIDEAN) r = T(2) * (ws * x[jn * size_t(m) + k] - s);   // sum w 2(x_j - x_i)
    else if (KIND == MM_LORENTZ) r = (k == 0) ? s : -s;                       // dq/dx_j = -J x_i
    else r = s;
    grad[jn * size_t(m) + k] = r;
  }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------------
// loss_kind: MM_LOSS_NONE (g = upstream gradient, loss_out unused) / MM_LOSS_STRESS / MM_LOSS_QUOTIENT (g = targets; squared
// distances).  !sub: a full batch of n points.  sub: a node minibatch (idx may be null only where it holds no pair): n = its size, x [n_total, m], g the dense
// n_total x n_total target matrix, grad [n_total, m].
template <typename T, int KIND, int MP>
int run_t(int loss_kind, const T* x, const T* g, const T* scale_raw, int64_t n, int m, int64_t rb, int64_t re, int squared, double alpha,
          double eps, int terms, const double* loss_params, T* loss_out, T* grad, void* det_ws, bool sub, const int64_t* idx, int64_t n_total,
          hipStream_t st) {
  const DetGeometry geo = geometry(sizeof(T), KIND, n, m);
  T* slab = static_cast<T*>(det_ws);
  T* slots = reinterpret_cast<T*>(static_cast<char*>(det_ws) + geo.slab_bytes);
  if (sub) {   // rows outside the batch: +0
    const hipError_t e = clear_async(grad, size_t(n_total) * size_t(m) * sizeof(T), st);   // (a kernel, never a memset node: clear.hpp)
    if (e != hipSuccess) return static_cast<int>(e);
  }
  int chunks = 0;
  int64_t nslots = 0;
  if (re > rb && n > 1 && pair_off(n, re) > pair_off(n, rb)) {
    LossArgs<T> la{scale_raw, T(alpha), T(eps), terms, nullptr, loss_params};
    const dim3 grid{unsigned(geo.groups), unsigned(geo.chunks), 1}, block{unsigned(kCols), 1, 1};
#define MM_VEC_DET_LAUNCH(LOSS, SUB)                                                                                              \
  pair_kernel<T, KIND, MP, LOSS, SUB><<<grid, block, 0, st>>>(x, g, int(n), m, int(rb), int(re), squared, int(geo.rows), slab, slots, \
                                                              la, idx, int(n_total))
    if (sub) {
      if (loss_kind == MM_LOSS_STRESS) MM_VEC_DET_LAUNCH(MM_LOSS_STRESS, true);
      else MM_VEC_DET_LAUNCH(MM_LOSS_QUOTIENT, true);
    } else {
      if (loss_kind == MM_LOSS_STRESS) MM_VEC_DET_LAUNCH(MM_LOSS_STRESS, false);
      else if (loss_kind == MM_LOSS_QUOTIENT) MM_VEC_DET_LAUNCH(MM_LOSS_QUOTIENT, false);
      else MM_VEC_DET_LAUNCH(MM_LOSS_NONE, false);
    }
#undef MM_VEC_DET_LAUNCH
    MM_CHECK_LAUNCH();
    chunks = int(geo.chunks);
    nslots = geo.groups * geo.chunks;
  }
  const int64_t nf = (sub && chunks == 0) ? 0 : n;   // (a minibatch without a pair: the cleared gradient stands; the loss record alone)
  const unsigned nb = unsigned(std::max<int64_t>(1, (nf + kNodeBlock - 1) / kNodeBlock));
  finalize_kernel<T, KIND, MP><<<dim3(nb), dim3(kNodeBlock), 0, st>>>(x, slab, int(nf), m, chunks, grad, slots, nslots, scale_raw,
                                                                     loss_kind == MM_LOSS_NONE ? static_cast<T*>(nullptr) : loss_out,
                                                                     idx, int(n_total));
  MM_CHECK_LAUNCH();
  return MM_OK;
}

}  // namespace vec_det
}  // namespace mm
