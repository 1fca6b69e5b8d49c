// SPD(d) pair gradients WITHOUT float atomics: the bit-deterministic mode next to spd_pdist_bwd_kernel (spd_pair.hpp).  The form,
// the loss record and the determinism contract are det_common.hpp's; this file holds what is SPD's own.
//
// Per visited pair a lane does the column side of the atomic backward:
//     A = L_r^-1 X_c L_r^-T,   M = 2 g log A,   S_c += L_r^-T M L_r^T
// d^2(X_r, X_c) is symmetric in its arguments, so summed over EVERY r != c this is the whole gradient: grad_c = sym(S_c X_c^-1),
// applied by the finalize kernel to the d^2 sums of a node's chunk records.  The row operand {L_r^-1, L_r} is read with scalar
// loads.  Every order of summation is a pure function of (dtype, n, d): geometry() below.
//
// The logarithm of a pair takes the gates and device functions of the atomic kernel (log_pair2_chol; close_gate / log_close, the
// recentred series, log_cayley, pair_core with the fp32 second solve; log_close_mat / log_centred_mat), one column per lane at
// every D, so the two modes agree to rounding.  The dispatch is written out here: spd_pdist_bwd_kernel is not touched.
#pragma once
#include "det_common.hpp"
#include "spd_pair.hpp"

namespace mm {
namespace spd_det {

using det::DetGeometry;
using det::kCols;
using det::kWaves;
// one node's chunk record: d^2 sums; rows per chunk in steps of one
inline DetGeometry geometry(size_t esz, int64_t n, int d) { return det::geometry(esz, size_t(d) * d * esz, n, 1); }

// ---- one pair: M = 2 g log A (packed), g from the upstream gradient / the fused loss ---------------------------------------
// `loaded`: upstream gradient or target of the pair (0 for a dead pair), `live`: the pair counts, `upper`: r < c (the visit
// that carries the loss term).  The paths are chosen per WAVEFRONT, as in the atomic kernel.
template <typename T, int D, int LOSS, bool SQ>
__device__ __forceinline__ void pair_m(const T (&li)[Packed<D>::NP], const T (&xc)[Packed<D>::NP], T loaded, bool live, bool upper,
                                       T wmin, T wmax, T sp, const LossArgs<T>& la, T& loss_acc, T& ds_acc,
                                       T (&m)[Packed<D>::NP]) {
  constexpr int NP = Packed<D>::NP;
  constexpr int squared = SQ ? 1 : 0;
  constexpr bool g_first = LOSS == MM_LOSS_NONE && SQ;   // the upstream gradient is known before log A
  T gs = live ? loaded : T(0);
  auto upstream = [&](T dsq) __attribute__((always_inline)) {
    T l = T(0), ds = T(0);
    gs = upstream_of<T, LOSS>(gs, dsq, live, squared, wmin, sp, la, l, ds);
    if constexpr (LOSS != MM_LOSS_NONE) {
      loss_acc += upper ? l : T(0);
      ds_acc += upper ? ds : T(0);
    }
  };
  auto jacobi_path = [&]() __attribute__((always_inline)) {
    T w[D], lw[D], v[D][D];
    const T s = pair_core<T, D, true, true, 1>(li, xc, wmin, wmax, w, lw, v);
    upstream(s);
    T cm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) cm[k] = (gs + gs) * lw[k];
    vdvt<T, D>(v, cm, m);
  };
  auto finish = [&](const T (&m0)[NP], bool scaled) __attribute__((always_inline)) {
    if (scaled) {
#pragma unroll
      for (int k = 0; k < NP; ++k) m[k] = m0[k];
      return;
    }
    T s = T(0);
    if (LOSS != MM_LOSS_NONE || !SQ) s = frob2<T, D>(m0);
    upstream(s);
    const T g2 = gs + gs;
#pragma unroll
    for (int k = 0; k < NP; ++k) m[k] = g2 * m0[k];
  };
  if constexpr (D == 2) {
    T m0[NP];
    const T s = log_pair2_chol<T>(li, xc, wmin, wmax, m0);
    upstream(s);
    const T g2 = gs + gs;
#pragma unroll
    for (int k = 0; k < NP; ++k) m[k] = g2 * m0[k];
  } else if constexpr (D == 3 || D == 4) {
    constexpr bool kCentred = std::is_same<T, float>::value;
    T a[NP];
    congr_chol<T, D>(li, xc, a);
    const bool far = !(close_gate<T, D>(a) <= T(kCloseGate));
    bool far2 = true;
    if (__builtin_expect(!__any(far), 1)) {
      T m0[NP];
      log_close<T, D>(a, m0, g_first ? gs + gs : T(1));
      finish(m0, g_first);
      far2 = false;
    } else if constexpr (kCentred) {
      bool f2;
      if constexpr (D == 3) f2 = centred_far3<T>(a); else f2 = centred_far4<T>(a);
      far2 = __any(f2);
      if (!far2) {
        T m0[NP];
        if constexpr (D == 3) log_series3_centred<T>(a, m0, g_first ? gs + gs : T(1));
        else log_series4_centred<T>(a, m0, g_first ? gs + gs : T(1));
        finish(m0, g_first);
      }
    }
    if (far2) {
      T m0[NP];
      const T gate = log_cayley<T, D>(a, m0, g_first ? gs + gs : T(1));
      if (__builtin_expect(!__any(!(gate <= T(kCayleyGate))), 1)) finish(m0, g_first); else jacobi_path();
    }
  } else {
    // SPD(5 .. 9): matrix-Horner series per wavefront (close pairs, pairs at moderate distance), else Jacobi — with the atomic
    // kernel's exception (fp64 SPD(8) keeps the eigensolve at moderate distance)
    constexpr bool kWideBwd = !(std::is_same<T, double>::value && D == 8);
    T a[NP], m0[NP];
    congr_chol<T, D>(li, xc, a);
    bool done = false;
    if (__builtin_expect(!__any(!(close_gate<T, D>(a) <= T(kCloseGate))), 1)) {
      log_close_mat<T, D>(a, m0);
      done = true;
    } else if (kWideBwd && !__any(centred_far_mat<T, D>(a))) {
      log_centred_mat<T, D>(a, m0);
      done = true;
    }
    if (done) finish(m0, false); else jacobi_path();
  }
}

// ---- the pair kernel ---------------------------------------------------------------------------------------------------
// grid (groups, chunks); workgroup (x, y): columns [kCols x, kCols x + kCols), rows [rows y, rows y + rows) of ALL n rows.
// A pair (r, c) is live iff r != c, c < n and row_begin <= min(r, c) < row_end; its upstream gradient / target sits at
// pair_off(min) - base + (max - min - 1) of `g` (64-bit).  The row cut is wave-uniform.  slab [chunks][D*D][n]; slots [2][groups * chunks].
template <typename T, int D, int LOSS, bool SQ>
__global__ __launch_bounds__(64 * kWaves) void pair_kernel(const T* __restrict__ nodeLC /* {L_r^-1, L_r} */,
                                                            const T* __restrict__ nodeY /* chol(X_c) */, const T* __restrict__ g,
                                                            int n, int row_begin, int row_end, int rows, T wmin, T wmax,
                                                            T* __restrict__ slab, T* __restrict__ slots, LossArgs<T> la) {
  constexpr int NP = Packed<D>::NP;
  T sp = T(1), loss_acc = T(0), ds_acc = T(0);
  loss_resolve<T, LOSS>(la);
  if constexpr (LOSS != MM_LOSS_NONE) sp = softplus_of(la.scale_raw);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the row operands stay scalar loads
  const int chunk = blockIdx.y;
  const int wc0 = int(blockIdx.x) * kCols + wave * 64;                 // the wavefront's first column
  const int c = wc0 + lane;
  const bool cin = c < n;
  if (wc0 < n) {   // (wave-uniform; a wavefront beyond the last column has nothing to store)
    T xc[NP], acc[D][D];
#pragma unroll
    for (int k = 0; k < NP; ++k) xc[k] = T(0);
#pragma unroll
    for (int k = 0; k < D; ++k) xc[pidx(k, k)] = T(1);
    if (cin) {
#pragma unroll
      for (int k = 0; k < NP; ++k) xc[k] = nodeY[size_t(c) * NP + k];
    }
#pragma unroll
    for (int rr = 0; rr < D; ++rr)
#pragma unroll
      for (int cc = 0; cc < D; ++cc) acc[rr][cc] = T(0);
    // rows of the chunk that can hold a live pair for these 64 columns: none below row_begin (min(r, c) >= row_begin needs
    // r >= row_begin), none at all if every column is below row_begin, and none from row_end on if every column is at or beyond
    // row_end (then min(r, c) >= row_end)
    const int r0 = chunk * rows, r1 = min(r0 + rows, n);
    int lo = max(r0, row_begin), hi = r1;
    if (wc0 >= row_end) hi = min(hi, row_end);
    if (wc0 + 63 < row_begin) hi = lo;
    const int64_t base = pair_off(n, row_begin);
    const bool cband = cin && c >= row_begin;            // the column passes its own part of the liveness test
    const int64_t gcol = pair_off(n, c) - base - c - 1;   // pair (r, c), r > c: g[gcol + r]
    auto live_of = [&](int r) __attribute__((always_inline)) { return cband && r != c && min(r, c) < row_end; };
    auto load_g = [&](int r, bool live) __attribute__((always_inline)) {
      const int64_t grow = pair_off(n, r) - base - r - 1;   // wave-uniform; pair (r, c), r < c: g[grow + c]
      const int64_t off = r < c ? grow + c : gcol + r;
      return live ? g[off] : T(0);
    };
    bool live_next = lo < hi ? live_of(lo) : false;
    T g_next = lo < hi ? load_g(lo, live_next) : T(0);
    // (the row operands are loaded where they are used.  Requested one row ahead as the pair vector is — 24 / 40 scalar registers
    // more at D = 3 / 4 — the replayed SPD(3) step measured 167 - 170 us against 164 - 168: not kept, profiles/spd_deterministic.md)
    for (int r = lo; r < hi; ++r) {
      T li[NP], lc[NP];
      const T* rowp = nodeLC + size_t(r) * (2 * NP);   // wave-uniform address: scalar loads
#pragma unroll
      for (int k = 0; k < NP; ++k) { li[k] = rowp[k]; lc[k] = rowp[NP + k]; }
      const bool live = live_next;
      const T loaded = g_next;
      if (r + 1 < hi) {   // the next row's request, ahead of this row's arithmetic
        live_next = live_of(r + 1);
        g_next = load_g(r + 1, live_next);
      }
      T m[NP];
      pair_m<T, D, LOSS, SQ>(li, xc, loaded, live, r < c, wmin, wmax, sp, la, loss_acc, ds_acc, m);
      if (!live) {   // (a dead pair adds exact zeros, whatever its logarithm came out as)
#pragma unroll
        for (int k = 0; k < NP; ++k) m[k] = T(0);
      }
      lt_m_lt_acc<T, D>(li, lc, m, acc);
    }
    if (cin) {
      T* rec = slab + size_t(chunk) * (D * D) * size_t(n) + c;
#pragma unroll
      for (int rr = 0; rr < D; ++rr)
#pragma unroll
        for (int cc = 0; cc < D; ++cc) rec[size_t(rr * D + cc) * size_t(n)] = acc[rr][cc];
    }
  }
  if constexpr (LOSS != MM_LOSS_NONE) {
    __shared__ T lossW[kWaves][2];
    const T l = wave_sum(loss_acc), dd = wave_sum(ds_acc);
    if (lane == 0) { lossW[wave][0] = l; lossW[wave][1] = dd; }
    __syncthreads();
    if (threadIdx.x == 0) {
      T ls = lossW[0][0], ds = lossW[0][1];
#pragma unroll
      for (int wv = 1; wv < kWaves; ++wv) { ls += lossW[wv][0]; ds += lossW[wv][1]; }
      const size_t nslots = size_t(gridDim.x) * gridDim.y;
      const size_t slot = size_t(blockIdx.y) * gridDim.x + blockIdx.x;
      slots[slot] = ls;
      slots[nslots + slot] = ds;
    }
  }
}

// ---- finalize: one thread per node ------------------------------------------------------------------------------------------
// S_c = the node's chunk records added in chunk order; grad_c = sym(S_c X_c^-1), X_c^-1 = L_c^-T L_c^-1.  chunks == 0 (an
// empty row range: no pair launch): zero gradient, zero loss.  The first wavefront of block 0 closes the loss record.
template <typename T, int D>
__global__ __launch_bounds__(kNodeBlock) void finalize_kernel(const T* __restrict__ nodeL, const T* __restrict__ slab, int n, int chunks, T* __restrict__ grad,
                                const T* __restrict__ slots, int64_t nslots, const T* __restrict__ scale_raw, T* __restrict__ loss_out) {
  constexpr int NP = Packed<D>::NP;
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
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T li[NP], xinv[NP], sc[D][D], gi[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) li[k] = nodeL[size_t(i) * NP + k];
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c) sc[r][c] = T(0);
  for (int k = 0; k < chunks; ++k) {
    const T* rec = slab + size_t(k) * (D * D) * size_t(n) + i;
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
      for (int c = 0; c < D; ++c) sc[r][c] += rec[size_t(r * D + c) * size_t(n)];
  }
#pragma unroll
  for (int r = 0; r < D; ++r)       // X^-1 = L^-T L^-1
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      T a = T(0);
#pragma unroll
      for (int k = r; k < D; ++k) a = Num<T>::fma(li[pidx(k, r)], li[pidx(k, c)], a);
      xinv[pidx(r, c)] = a;
    }
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      T a = T(0), b = T(0);         // (S X^-1)[r][c] and (S X^-1)[c][r]
#pragma unroll
      for (int k = 0; k < D; ++k) {
        a = Num<T>::fma(sc[r][k], xinv[pidx(k, c)], a);
        b = Num<T>::fma(sc[c][k], xinv[pidx(k, r)], b);
      }
      gi[pidx(r, c)] = T(0.5) * (a + b);
    }
  store_sym_full<T, D>(grad + size_t(i) * D * D, gi);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
template <typename T, int D, int LOSS, bool SQ>
int launch_pairs(Ws<T>& ws, const T* g, int64_t n, int64_t rb, int64_t re, double wmin, double wmax, const DetGeometry& geo, T* slab,
                 T* slots, LossArgs<T> la, hipStream_t st) {
  if (!spd_clamps_supported<D, LOSS>(wmin, wmax)) return MM_ERR_UNSUPPORTED;
  const dim3 grid{unsigned(geo.groups), unsigned(geo.chunks), 1};
  const T* nlc = ws.nodeLC;
  const T* nc = ws.nodeC;
  pair_kernel<T, D, LOSS, SQ><<<grid, dim3(64 * kWaves), 0, st>>>(nlc, nc, g, int(n), int(rb), int(re), int(geo.rows), T(wmin), T(wmax),
                                                                  slab, slots, la);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

// kind: MM_LOSS_NONE (g = upstream gradient, loss_out unused) / MM_LOSS_STRESS / MM_LOSS_QUOTIENT (g = target)
template <typename T, int D>
int run_t(int kind, const T* x, const T* g, const T* scale_raw, int64_t n, int64_t rb, int64_t re, int squared, double alpha,
          double eps, int terms, const double* loss_params, double wmin, double wmax, T* loss_out, T* grad, void* wsp, void* det_ws,
          int flags, hipStream_t st) {
  Ws<T> ws(wsp, n, D);
  if (kind == MM_LOSS_NONE ? !spd_clamps_supported<D, MM_LOSS_NONE>(wmin, wmax) : !spd_clamps_supported<D, MM_LOSS_STRESS>(wmin, wmax))
    return MM_ERR_UNSUPPORTED;
  int rc = spd_pdist_prepare<T, D>(x, n, ws, flags, st);
  if (rc) return rc;
  const DetGeometry geo = geometry(sizeof(T), n, D);
  T* slab = static_cast<T*>(det_ws);
  T* slots = reinterpret_cast<T*>(static_cast<char*>(det_ws) + geo.slab_bytes);
  int chunks = 0;
  int64_t nslots = 0;
  if (re > rb && pair_off(n, re) > pair_off(n, rb)) {
    LossArgs<T> la{scale_raw, T(alpha), T(eps), terms, nullptr, loss_params};
    if (kind == MM_LOSS_STRESS) rc = launch_pairs<T, D, MM_LOSS_STRESS, true>(ws, g, n, rb, re, wmin, wmax, geo, slab, slots, la, st);
    else if (kind == MM_LOSS_QUOTIENT) rc = launch_pairs<T, D, MM_LOSS_QUOTIENT, true>(ws, g, n, rb, re, wmin, wmax, geo, slab, slots, la, st);
    else if (squared) rc = launch_pairs<T, D, MM_LOSS_NONE, true>(ws, g, n, rb, re, wmin, wmax, geo, slab, slots, la, st);
    else rc = launch_pairs<T, D, MM_LOSS_NONE, false>(ws, g, n, rb, re, wmin, wmax, geo, slab, slots, la, st);
    if (rc) return rc;
    chunks = int(geo.chunks);
    nslots = geo.groups * geo.chunks;
  }
  const T* nl = ws.nodeL;
  finalize_kernel<T, D><<<dim3((n + kNodeBlock - 1) / kNodeBlock), dim3(kNodeBlock), 0, st>>>(
      nl, slab, int(n), chunks, grad, slots, nslots, scale_raw, kind == MM_LOSS_NONE ? static_cast<T*>(nullptr) : loss_out);
  MM_CHECK_LAUNCH();
  return MM_OK;
}

}  // namespace spd_det
}  // namespace mm
