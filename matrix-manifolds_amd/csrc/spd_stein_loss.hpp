// Stein divergence: the fused objective and node minibatches inside the pair kernels (included by spd_stein_loss.hip inside
// namespace mm, after spd_stein.hpp).
//
// spd_stein_bwd_kernel (spd_stein.hpp) sends g P to both endpoints of a pair and finalize applies -(sum g) X_i^-1 / 2.  With g
// taken from the loss term instead of the pair vector that same pass is the whole objective (modules.py:84-88 +
// objectives.py:16-45 on the Stein divergence of spd.py:191-194):
//   S = max(stein_pair, wmin)        (the clamp is on the VALUE only: div.data.clamp_, spd.py:188,193)
//   m = softplus(scale_raw) S,  loss += loss_term(m, target),  g = d loss / d m * softplus(scale_raw)
// and d loss / d m * S leaves through the workspace's loss slots (loss_finalize applies the sigmoid).  One kernel source,
// templated on the loss and on SUB:
//   LOSS != 0, !SUB   g = the target pair vector of the rows [row_begin, row_end)          mm_spd_stein_pdiv_loss
//   LOSS != 0,  SUB   g = the dense n_total x n_total target matrix                        mm_spd_stein_pdiv_loss_subset
//   LOSS == 0,  SUB   g = the upstream gradient of the BATCH's pair vector                 mm_spd_stein_pdiv_bwd_subset
// (LOSS == 0, !SUB is spd_stein_bwd_kernel itself, left as it is.)
// SUB: the n points of the launch are the nodes idx[0..n) of a table of n_total points (spd_pair.hpp, spd_pdist_bwd_kernel):
// the pair list is that of the batch positions, everything per NODE — table rows, log dets, targets, accumulator slots — goes
// through batch_node(), which clamps the node id into the tables.  The row node is broadcast to a scalar register, so the row
// operand stays on scalar loads.  Prep and finalize run over the whole table: rows outside the batch come out +0.
#pragma once

template <typename T, int D, int TI, int LOSS, bool SUB>
__global__ __launch_bounds__(kBlock) void spd_stein_pair_kernel(const T* __restrict__ nodeX, const T* __restrict__ nodeLd,
                                                                const T* __restrict__ g, int n, int row_begin, int row_end,
                                                                int squared, T wmin, T* __restrict__ accM,
                                                                T* __restrict__ accS, LossArgs<T> la,
                                                                const int64_t* __restrict__ idx, int n_total) {
  static_assert(LOSS != MM_LOSS_NONE || SUB, "the plain backward is spd_stein_bwd_kernel");
  constexpr int NP = Packed<D>::NP;
  constexpr int NV = NP + 1;  // packed P and the pair's weight itself
  constexpr int NW = kBlock / 64;
  __shared__ T redR[NW][TI][NV];
  __shared__ T colS[NW][NV][64];
  const int ns = SUB ? n_total : n;                      // stride of the per-node accumulators
  const int* idx32 = reinterpret_cast<const int*>(idx);  // (little-endian low words: node ids are < 2^22)
  T sp = T(1), loss_acc = T(0), ds_acc = T(0);
  loss_resolve<T, LOSS>(la);
  if constexpr (LOSS != MM_LOSS_NONE) sp = softplus_of(la.scale_raw);
  const TileId tile = fold_tile<NW * TI, 64>(n, row_begin, row_end);
  if (!tile.ok) return;  // block-uniform
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int jbase = tile.jbase;
  const int i0 = tile.i0 + wave * TI, i1 = max(i0, min(i0 + TI, min(tile.i0 + NW * TI, row_end)));
  const bool wave_live = i0 < i1 && jbase + 63 > i0;
  const int j = jbase + lane;
  const bool jin = j < n;
  int jn = j;  // the column's node
  if constexpr (SUB) jn = batch_node(idx32, size_t(min(j, n - 1)), n_total);
  bool red_writer;
  const int red_slot = reduce_slot<NV>(lane, red_writer);
  T xj[NP], ldj = T(0), accJ[NV];
#pragma unroll
  for (int k = 0; k < NP; ++k) xj[k] = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) xj[pidx(k, k)] = T(1);
#pragma unroll
  for (int k = 0; k < NV; ++k) accJ[k] = T(0);
  if (jin) {
#pragma unroll
    for (int k = 0; k < NP; ++k) xj[k] = nodeX[size_t(jn) * NP + k];
    ldj = nodeLd[jn];
  }
  const int64_t base = pair_off(n, row_begin);
  if (wave_live) {
    for (int i = i0; i < i1; ++i) {
      T xi[NP], l[NP], li[NP], v[NV];
      // the row's node in a scalar register -> wave-uniform row operand, scalar loads
      const int in = SUB ? __builtin_amdgcn_readfirstlane(batch_node(idx32, size_t(i), n_total)) : i;
#pragma unroll
      for (int k = 0; k < NP; ++k) xi[k] = nodeX[size_t(in) * NP + k];
      const bool valid = jin && j > i;
      // upstream gradient or target of the pair; lanes outside the triangle read a valid element and are masked at use
      T loaded;
      if constexpr (SUB && LOSS != MM_LOSS_NONE) loaded = g[size_t(in) * size_t(n_total) + size_t(jn)];
      else loaded = pair_row_load<T>(g, n, base, i, j);
      const T div = stein_pair<T, D>(xi, xj, nodeLd[in] + ldj, l);
      T gs;
      if constexpr (LOSS != MM_LOSS_NONE) {
        const T s = Num<T>::max(div, wmin);
        T dldm;
        const T lt = loss_term<T, LOSS>(sp * s, loaded, la, dldm);
        loss_acc += valid ? lt : T(0);
        ds_acc += valid ? dldm * s : T(0);
        gs = valid ? dldm * sp : T(0);
      } else {
        gs = valid ? loaded : T(0);
        if (!squared) gs *= T(0.5) * Num<T>::rsqrt(Num<T>::max(div, wmin));  // d sqrt(clamp(S)) / dS, clamp transparent
      }
      invert_lower<T, D>(l, li);
      // P = L^-T L^-1 (packed symmetric), scaled by the pair's weight
#pragma unroll
      for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          T acc = T(0);
#pragma unroll
          for (int k = r; k < D; ++k) acc = Num<T>::fma(li[pidx(k, r)], li[pidx(k, c)], acc);
          v[pidx(r, c)] = gs * acc;
        }
      v[NP] = gs;
#pragma unroll
      for (int k = 0; k < NV; ++k) accJ[k] += v[k];
      // row side: transposing reduction, every lane ends with the wavefront total of ONE of the NV values
      const T tot = wave_reduce_transposed<NV, T>(v, lane);
      if (red_writer) redR[wave][i - i0][red_slot] = tot;
    }
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < TI * NV; t += 64) {
      const int k = t / TI, il = t % TI;
      if (i0 + il < i1) {
        const int node = SUB ? batch_node(idx32, size_t(i0 + il), n_total) : i0 + il;
        T* dst = k < NP ? &accM[size_t(k) * ns + node] : &accS[node];
        atomic_add(dst, redR[wave][il][k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) colS[wave][k][lane] = accJ[k];
  __syncthreads();
  if (jin) {
    for (int k = wave; k < NV; k += NW) {
      T sum = colS[0][k][lane];
#pragma unroll
      for (int wv = 1; wv < NW; ++wv) sum += colS[wv][k][lane];
      T* dst = k < NP ? &accM[size_t(k) * ns + jn] : &accS[jn];
      atomic_add(dst, sum);
    }
  }
  if constexpr (LOSS != MM_LOSS_NONE) {
    __shared__ T lossW[NW][2];
    const T ls = wave_sum(loss_acc), dd = wave_sum(ds_acc);
    if (lane == 0) { lossW[wave][0] = ls; lossW[wave][1] = dd; }
    __syncthreads();
    if (threadIdx.x == 0) {
      T lsum = lossW[0][0], dsum = lossW[0][1];
#pragma unroll
      for (int wv = 1; wv < NW; ++wv) { lsum += lossW[wv][0]; dsum += lossW[wv][1]; }
      const int slot = int(blockIdx.y * gridDim.x + blockIdx.x) & (kLossSlots - 1);
      atomic_add(&la.slots[slot], lsum);
      atomic_add(&la.slots[kLossSlots + slot], dsum);
    }
  }
}

// spd_stein_fwd_kernel for a node minibatch: the batch's pair vector from the full table
template <typename T, int D, int TI>
__global__ __launch_bounds__(kBlock) void spd_stein_fwd_subset_kernel(const T* __restrict__ nodeX, const T* __restrict__ nodeLd,
                                                                      int n, int row_begin, int row_end, int squared, T wmin,
                                                                      T* __restrict__ out, const int64_t* __restrict__ idx,
                                                                      int n_total) {
  constexpr int NP = Packed<D>::NP;
  const int* idx32 = reinterpret_cast<const int*>(idx);
  const TileId tile = fold_tile<TI>(n, row_begin, row_end);
  if (!tile.ok) return;
  const int i0 = tile.i0, i1 = min(i0 + TI, row_end), jbase = tile.jbase;
  if (jbase + (int(threadIdx.x) & ~63) + 63 <= i0) return;  // whole wavefront below the diagonal
  const int j = jbase + threadIdx.x;
  const bool jin = j < n;
  const int jn = batch_node(idx32, size_t(min(j, n - 1)), n_total);
  T xj[NP], ldj = T(0);
#pragma unroll
  for (int k = 0; k < NP; ++k) xj[k] = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) xj[pidx(k, k)] = T(1);
  if (jin) {
#pragma unroll
    for (int k = 0; k < NP; ++k) xj[k] = nodeX[size_t(jn) * NP + k];
    ldj = nodeLd[jn];
  }
  const int64_t base = pair_off(n, row_begin);
  for (int i = i0; i < i1; ++i) {
    T xi[NP], l[NP];  // wave-uniform row operand -> scalar loads
    const int in = __builtin_amdgcn_readfirstlane(batch_node(idx32, size_t(i), n_total));
#pragma unroll
    for (int k = 0; k < NP; ++k) xi[k] = nodeX[size_t(in) * NP + k];
    T s = Num<T>::max(stein_pair<T, D>(xi, xj, nodeLd[in] + ldj, l), wmin);
    if (!squared) s = Num<T>::sqrt(s);
    if (jin && j > i) out[pair_off(n, i) - base + (j - i - 1)] = s;
  }
}

// spd_stein_finalize_kernel's arithmetic, and the loss record from the workspace's slots
template <typename T, int D>
__global__ void spd_stein_loss_finalize_kernel(const T* __restrict__ nodeL, T* __restrict__ accM, T* __restrict__ accS, int n,
                                               T* __restrict__ grad, T* __restrict__ slots, const T* __restrict__ scale_raw,
                                               T* __restrict__ loss_out) {
  constexpr int NP = Packed<D>::NP;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 64) loss_finalize<T>(slots, scale_raw, loss_out);
  if (i >= n) return;
  T li[NP], out[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) li[k] = nodeL[size_t(i) * NP + k];
  const T gsum = accS[i];
  accS[i] = T(0);
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      T xinv = T(0);  // X^-1 = L^-T L^-1
#pragma unroll
      for (int k = r; k < D; ++k) xinv = Num<T>::fma(li[pidx(k, r)], li[pidx(k, c)], xinv);
      const size_t a = size_t(pidx(r, c)) * n + i;
      out[pidx(r, c)] = T(0.5) * (accM[a] - gsum * xinv);
      accM[a] = T(0);
    }
  store_sym_full<T, D>(grad + size_t(i) * D * D, out);
}

constexpr int kSteinTI = 8;   // rows per wavefront of a pair tile, as spd_stein_bwd_t

// Objective and gradients of the pair rows [rb, re) of `np` points: all n_total = np points (SUB = false; g = target pair vector)
// or the batch idx[0..np) of a table of n_total points (SUB = true; g = dense targets).  Prep and finalize over the table.
template <typename T, int D, bool SUB>
int spd_stein_loss_t(int kind, const T* x, const T* g, const T* scale_raw, int64_t n_total, const int64_t* idx, int64_t np,
                     int64_t rb, int64_t re, double alpha, double eps, int terms, const double* loss_params, double wmin,
                     T* loss_out, T* grad, void* wsp, int flags, hipStream_t st) {
  Ws<T> ws(wsp, n_total, D);
  int rc = spd_pdist_prepare<T, D>(x, n_total, ws, flags, st);
  if (rc) return rc;
  if (re > rb && pair_off(np, re) > pair_off(np, rb)) {
    ProfScope prof(PROF_SPD_BWD, st);
    LossArgs<T> la{scale_raw, T(alpha), T(eps), terms, ws.loss, loss_params};
    const dim3 grid = fold_grid<(kBlock / 64) * kSteinTI, 64>(np, rb, re);
    if (kind == MM_LOSS_STRESS)
      spd_stein_pair_kernel<T, D, kSteinTI, MM_LOSS_STRESS, SUB><<<grid, dim3(kBlock), 0, st>>>(
          ws.nodeX, ws.nodeLd, g, int(np), int(rb), int(re), 1, T(wmin), ws.accM, ws.accS, la, idx, int(n_total));
    else
      spd_stein_pair_kernel<T, D, kSteinTI, MM_LOSS_QUOTIENT, SUB><<<grid, dim3(kBlock), 0, st>>>(
          ws.nodeX, ws.nodeLd, g, int(np), int(rb), int(re), 1, T(wmin), ws.accM, ws.accS, la, idx, int(n_total));
  }
  MM_CHECK_LAUNCH();
  spd_stein_loss_finalize_kernel<T, D><<<dim3((n_total + kNodeBlock - 1) / kNodeBlock), dim3(kNodeBlock), 0, st>>>(
      ws.nodeL, ws.accM, ws.accS, int(n_total), grad, ws.loss, scale_raw, loss_out);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

template <typename T, int D>
int spd_stein_fwd_subset_t(const T* x, int64_t n_total, const int64_t* idx, int64_t bs, int64_t rb, int64_t re, int squared,
                           double wmin, T* out, void* wsp, int flags, hipStream_t st) {
  Ws<T> ws(wsp, n_total, D);
  int rc = spd_pdist_prepare<T, D>(x, n_total, ws, flags, st);
  if (rc) return rc;
  if (re <= rb || pair_off(bs, re) == pair_off(bs, rb)) return MM_OK;
  {
    ProfScope prof(PROF_SPD_FWD, st);
    spd_stein_fwd_subset_kernel<T, D, kSteinTI><<<fold_grid<kSteinTI>(bs, rb, re), dim3(kBlock), 0, st>>>(
        ws.nodeX, ws.nodeLd, int(bs), int(rb), int(re), squared, T(wmin), out, idx, int(n_total));
  }
  MM_CHECK_LAUNCH();
  return MM_OK;
}

template <typename T, int D>
int spd_stein_bwd_subset_t(const T* x, const T* g, int64_t n_total, const int64_t* idx, int64_t bs, int64_t rb, int64_t re,
                           int squared, double wmin, T* grad, void* wsp, int flags, hipStream_t st) {
  Ws<T> ws(wsp, n_total, D);
  int rc = spd_pdist_prepare<T, D>(x, n_total, ws, flags, st);
  if (rc) return rc;
  if (re > rb && pair_off(bs, re) > pair_off(bs, rb)) {
    ProfScope prof(PROF_SPD_BWD, st);
    LossArgs<T> la{nullptr, T(1), T(0), 0, nullptr, nullptr};
    spd_stein_pair_kernel<T, D, kSteinTI, MM_LOSS_NONE, true>
        <<<fold_grid<(kBlock / 64) * kSteinTI, 64>(bs, rb, re), dim3(kBlock), 0, st>>>(
            ws.nodeX, ws.nodeLd, g, int(bs), int(rb), int(re), squared, T(wmin), ws.accM, ws.accS, la, idx, int(n_total));
  }
  MM_CHECK_LAUNCH();
  spd_stein_finalize_kernel<T, D><<<dim3((n_total + kNodeBlock - 1) / kNodeBlock), dim3(kNodeBlock), 0, st>>>(
      ws.nodeL, ws.accM, ws.accS, int(n_total), grad);
  MM_CHECK_LAUNCH();
  return MM_OK;
}
