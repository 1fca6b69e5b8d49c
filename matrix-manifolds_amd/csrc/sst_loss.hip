// Spanning-tree KL objective on a pair vector (mm_sst_kl_loss): with theta a pair vector in the package's order, w = exp theta,
// L(theta) the weighted graph Laplacian without the row and column of node 0 (N = n - 1 rows), G = L^-1 (zero for node 0),
//   A = log det L,  mu_ij = w_ij q(G)_ij,  q(S)_ij = S_ii + S_jj - 2 S_ij,  delta = theta_z - theta_x,
//   loss = A(theta_z) - A(theta_x) - mu(theta_x) . delta = KL(trees(theta_x) || trees(theta_z))
// (the reference's KLDiveregenceLoss('sste', inclusive): objectives.py:48-76 with inference/stochastic_trees.py), inclusive
// (theta_x = -alpha g, theta_z = -m) or exclusive (theta_x = -m, theta_z = -alpha g), and d loss / d m per pair:
//   inclusive            mu(theta_x) - mu(theta_z)
//   exclusive            mu delta - w q(G M G),  M the reduced Laplacian of the weights w delta, all at theta_x
//   exclusive reference  mu delta               (what the reference returns: it drops dG / dtheta)
//
// Every model is evaluated on the shifted weights w' = exp(theta - c), c = max theta: L' = e^-c L, G' = e^c G, and
// sum mu = n - 1 turns the shift of A and of mu . delta into one another, so with delta' = (theta_z - c_z) - (theta_x - c_x)
//   loss = 2 (sum log C_z - sum log C_x) - sum mu delta',   exact exclusive gradient = mu delta' - w' q(G' M' G')
// (M' from w' delta'): a constant added to every m leaves the loss and these gradients unchanged to the last bit.
//
// Launches (grid z = the model, x first; the z model is inverted only for the inclusive gradient):
//   max       partial maxima of theta_x and theta_z (max is exact: the order does not matter)
//   assemble  one workgroup per row: the lower triangle of L' (and, exact exclusive, the full M'), row sums in fixed order
//   per panel k of kNB rows (right-looking):
//     diag    one workgroup: Cholesky of the diagonal block in LDS, its inverse Z[k,k], sum log C_jj in fp64
//     panel   C[i,k] = A[i,k] Z[k,k]^T (i > k)  and  Z[k,j] = Z[k,k] W[k,j] (j < k)
//     trail   A[i,j] -= C[i,k] C[j,k]^T (i >= j > k)  and  W[i,j] -= C[i,k] Z[k,j] (i > k >= j)
//             — W is the forward substitution of C Z = I carried along, so Z = C^-1 is complete when the factor is
//   G         G = Z^T Z, lower tiles computed, stored with their mirror image (into the storage of the factor)
//   GM, TG    exact exclusive only: T = G M', Y = T G (lower tiles, mirrored)
//   pair      one store per pair, fixed-order fp64 partial sums of mu delta' per row
//   finish    one wavefront adds the partials
// All products go through gemm_tile: a kT x kT output tile per workgroup of four wavefronts, operands staged through LDS
// in chunks of kT, v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (exact f32 / f64).  In-place products (panel) have K <= kT:
// their one chunk is in LDS before the first store.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mm_manifolds.h"
#include "clear.hpp"
#include "smallmat.hpp"

namespace mm {
namespace sst {

constexpr int kT = 32;                 // GEMM tile = panel width kNB
constexpr int kNB = kT;
constexpr int kBlk = 256;              // threads of every kernel but diag
constexpr int kMaxP = 256;             // partial maxima
constexpr int64_t kMaxNodes = 4096;    // five (n - 1)^2 matrices: 0.67 GB in fp64 there

inline size_t round256(size_t b) { return (b + 255) & ~size_t(255); }
inline size_t mat_bytes(size_t el, int64_t n) { return round256(el * size_t(n - 1) * size_t(n - 1)); }
inline int panels(int64_t n) { return int((n - 1 + kNB - 1) / kNB); }

__host__ __device__ inline int poff(int n, int row) { return row * (2 * n - row - 1) / 2; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Mma;
template <> struct Mma<float> {
  using Acc = f32x4;
  static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};
template <> struct Mma<double> {
  using Acc = f64x4;
  static __device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

template <typename T> struct Ws {
  T* A[2];        // L', then the factor C (lower), then G (full)
  T* Z[2];        // W / Z = C^-1 (lower tiles); x: then T = G M'
  T* M;           // M' (full), then Y (full)
  T* maxp;        // [2][kMaxP]
  double* logp;   // [2][panels]
  double* pairp;  // [n - 1]
};

// (the product is rounded on its own: contracted into the subtraction of the shift, theta - max theta would keep the
// product's rounding error, and the pair that IS the maximum would not come out as exp(0))
template <typename T, bool INCL> __device__ __forceinline__ void thetas(T gv, T mv, T alpha, T& tx, T& tz) {
#pragma clang fp contract(off)
  const T a = -alpha * gv, b = -mv;
  tx = INCL ? a : b;
  tz = INCL ? b : a;
}

// max / sum over the workgroup (kBlk threads) in fixed order; every thread gets the result
template <typename T> __device__ __forceinline__ T block_max(T v, T* sh) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = Num<T>::max(v, __shfl_xor(v, m, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return Num<T>::max(Num<T>::max(sh[0], sh[1]), Num<T>::max(sh[2], sh[3]));
}
template <typename T> __device__ __forceinline__ T block_sum(T v, T* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

template <typename T, bool INCL>
__global__ __launch_bounds__(kBlk) void sst_max_kernel(const T* __restrict__ g, const T* __restrict__ m, int npairs, T alpha,
                                                       T* __restrict__ maxp) {
  __shared__ T sh[4];
  T mx = -T(INFINITY), mz = -T(INFINITY);
  for (int p = blockIdx.x * kBlk + threadIdx.x; p < npairs; p += gridDim.x * kBlk) {
    T tx, tz;
    thetas<T, INCL>(g[p], m[p], alpha, tx, tz);
    mx = Num<T>::max(mx, tx);
    mz = Num<T>::max(mz, tz);
  }
  mx = block_max(mx, sh);
  mz = block_max(mz, sh);
  if (threadIdx.x == 0) {
    maxp[blockIdx.x] = mx;
    maxp[kMaxP + blockIdx.x] = mz;
  }
}

// the two shifts from the partial maxima
template <typename T> __device__ __forceinline__ void shifts(const T* __restrict__ maxp, int np, T* sh, T& cx, T& cz) {
  const int t = threadIdx.x;
  cx = block_max(t < np ? maxp[t] : -T(INFINITY), sh);
  cz = block_max(t < np ? maxp[kMaxP + t] : -T(INFINITY), sh);
}

// Row r (node r + 1) of L' of the model blockIdx.y, and (EXACT, the x model) of M'.  A node without a finite positive
// degree — node 0 included, whose degree is not in L' — poisons the diagonal: the graph is disconnected.
template <typename T, bool INCL, bool EXACT>
__global__ __launch_bounds__(kBlk) void sst_assemble_kernel(const T* __restrict__ g, const T* __restrict__ m, int n, T alpha,
                                                            int np, Ws<T> ws) {
  __shared__ T sh[4];
  const int r = blockIdx.x, model = blockIdx.y, a = r + 1, N = n - 1;
  T cx, cz;
  shifts(ws.maxp, np, sh, cx, cz);
  T* __restrict__ Lr = ws.A[model] + size_t(r) * N;
  T* __restrict__ Mr = ws.M + size_t(r) * N;
  const bool wm = EXACT && model == 0;
  T sum = T(0), sumd = T(0), deg0 = T(0);
  for (int j = threadIdx.x; j < n; j += kBlk) {
    if (j == a) continue;
    const int p = j < a ? poff(n, j) + (a - j - 1) : poff(n, a) + (j - a - 1);
    T tx, tz;
    thetas<T, INCL>(g[p], m[p], alpha, tx, tz);
    const T w = Num<T>::exp(model ? tz - cz : tx - cx);
    sum += w;
    if (j >= 1 && j < a) Lr[j - 1] = -w;
    if (wm) {
      const T wd = w * ((tz - cz) - (tx - cx));
      sumd += wd;
      if (j >= 1) Mr[j - 1] = -wd;
    }
  }
  if (r == 0)   // the degree of node 0: its pairs are the first n - 1
    for (int j = 1 + threadIdx.x; j < n; j += kBlk) {
      T tx, tz;
      thetas<T, INCL>(g[j - 1], m[j - 1], alpha, tx, tz);
      deg0 += Num<T>::exp(model ? tz - cz : tx - cx);
    }
  sum = block_sum(sum, sh);
  if (wm) sumd = block_sum(sumd, sh);
  if (r == 0) deg0 = block_sum(deg0, sh);
  if (threadIdx.x == 0) {
    const bool ok = sum > T(0) && sum < T(INFINITY) && (r != 0 || (deg0 > T(0) && deg0 < T(INFINITY)));
    Lr[r] = ok ? sum : T(NAN);
    if (wm) Mr[r] = sumd;
  }
}

// Cholesky of the diagonal block k (nb x nb, lower triangle of A) and the inverse of its factor, in LDS; one thread per entry.
// A pivot that is not finite and positive becomes NaN.  The block is padded to kNB with the identity.
template <typename T>
__global__ __launch_bounds__(kNB * kNB) void sst_diag_kernel(Ws<T> ws, int N, int k, int nt) {
  __shared__ T sC[kNB][kNB + 1];
  __shared__ T sX[kNB][kNB + 1];
  const int model = blockIdx.z, r = threadIdx.x >> 5, c = threadIdx.x & 31;
  const int k0 = k * kNB, nb = min(kNB, N - k0);
  T* __restrict__ A = ws.A[model] + size_t(k0) * N + k0;
  T* __restrict__ Z = ws.Z[model] + size_t(k0) * N + k0;
  sC[r][c] = (r < nb && c <= r) ? A[r * N + c] : (r == c ? T(1) : T(0));
  sX[r][c] = r == c ? T(1) : T(0);
  // Column j of the factor, and with it step j of the forward substitution C X = I carried in sX (right-looking as well:
  // row j of X is final once pivot j is, and leaves the rows below it) — the two updates touch disjoint columns, so the
  // inverse costs no barrier of its own.
  for (int j = 0; j < kNB; ++j) {
    __syncthreads();
    const T d = sC[j][j];
    const T piv = (d > T(0) && d < T(INFINITY)) ? T(::sqrt(double(d))) : T(NAN);
    if (c == j && r > j) sC[r][j] = sC[r][j] / piv;
    if (r == j && c <= j) sX[j][c] = sX[j][c] / piv;
    __syncthreads();
    if (r > j) {
      if (c > j) {
        if (r >= c) sC[r][c] -= sC[r][j] * sC[c][j];
      } else {
        sX[r][c] -= sC[r][j] * sX[j][c];
      }
    }
    if (r == j && c == j) sC[j][j] = piv;
  }
  __syncthreads();
  if (r < nb && c < nb) {
    Z[r * N + c] = sX[r][c];
    if (c <= r) A[r * N + c] = sC[r][c];
  }
  if (threadIdx.x < 64) {   // sum log C_jj: lane j takes pivot j, the butterfly adds in a fixed order
    const double s = wave_sum((r == 0 && c < nb) ? ::log(double(sC[c][c])) : 0.0);
    if (threadIdx.x == 0) ws.logp[model * nt + k] = s;
  }
}

// acc = opA(A) [M x K] opB(B) [K x Nc] for one kT x kT output tile (M, Nc <= kT valid rows / columns, anything beyond reads as
// zero); opA(A)[i][q] = TA ? A[q lda + i] : A[i lda + q], opB(B)[q][j] = TB ? B[j ldb + q] : B[q ldb + j].  Wavefront w owns
// the 16 x 16 block (w >> 1, w & 1); the whole workgroup must call it.
template <typename T, bool TA, bool TB>
__device__ __forceinline__ typename Mma<T>::Acc gemm_tile(const T* A, int lda, const T* B, int ldb,
                                                           int M, int Nc, int K) {
  __shared__ T sA[kT][kT + 1];   // [i][q]
  __shared__ T sB[kT][kT + 1];   // [q][j]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = (wave >> 1) * 16, wj = (wave & 1) * 16;
  typename Mma<T>::Acc acc = {T(0), T(0), T(0), T(0)};
  for (int q0 = 0; q0 < K; q0 += kT) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kT * kT / kBlk; ++s) {
      const int idx = threadIdx.x + s * kBlk, slow = idx >> 5, fast = idx & 31;
      {
        const int i = TA ? fast : slow, q = TA ? slow : fast;
        const bool ok = i < M && q0 + q < K;
        sA[i][q] = ok ? (TA ? A[size_t(q0 + q) * lda + i] : A[size_t(i) * lda + q0 + q]) : T(0);
      }
      {
        const int j = TB ? slow : fast, q = TB ? fast : slow;
        const bool ok = j < Nc && q0 + q < K;
        sB[q][j] = ok ? (TB ? B[size_t(j) * ldb + q0 + q] : B[size_t(q0 + q) * ldb + j]) : T(0);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kT; q += 4)
      acc = Mma<T>::mma(sA[wi + (lane & 15)][q + (lane >> 4)], sB[q + (lane >> 4)][wj + (lane & 15)], acc);
  }
  return acc;
}

enum { kSet = 0, kSetNeg = 1, kSub = 2 };

// D (op)= acc on the valid M x Nc part of the tile; `mirror`: also to the transposed tile at Dm
template <typename T>
__device__ __forceinline__ void store_tile(typename Mma<T>::Acc acc, T* D, int ldd, int M, int Nc, int op, T* Dm = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (wave & 1) * 16 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = (wave >> 1) * 16 + Mma<T>::row(lane, r);
    if (i < M && j < Nc) {
      T* p = D + size_t(i) * ldd + j;
      const T v = op == kSet ? acc[r] : op == kSetNeg ? -acc[r] : *p - acc[r];
      *p = v;
      if (Dm) Dm[size_t(j) * ldd + i] = v;
    }
  }
}

// panel k: C[b,k] = A[b,k] Z[k,k]^T for b > k (in place), Z[k,b] = Z[k,k] W[k,b] for b < k (in place, `inv` models only)
template <typename T> __global__ __launch_bounds__(kBlk) void sst_panel_kernel(Ws<T> ws, int N, int k, int inv) {
  const int b = blockIdx.x, model = blockIdx.z;
  const int k0 = k * kNB, nb = min(kNB, N - k0), b0 = b * kT;
  T* A = ws.A[model];
  T* Z = ws.Z[model];
  const T* D = Z + size_t(k0) * N + k0;
  if (b > k) {
    const int mb = min(kT, N - b0);
    T* t = A + size_t(b0) * N + k0;
    store_tile<T>(gemm_tile<T, false, true>(t, N, D, N, mb, nb, nb), t, N, mb, nb, kSet);
  } else if (b < k && ((inv >> model) & 1)) {
    T* t = Z + size_t(k0) * N + b0;
    store_tile<T>(gemm_tile<T, false, false>(D, N, t, N, nb, kT, nb), t, N, nb, kT, kSet);
  }
}

// after panel k, rows i = k + 1 + blockIdx.y: A[i,j] -= C[i,k] C[j,k]^T (k < j <= i), W[i,j] -= C[i,k] Z[k,j] (j <= k; W[i,k] starts at 0)
template <typename T> __global__ __launch_bounds__(kBlk) void sst_trail_kernel(Ws<T> ws, int N, int k, int inv) {
  const int j = blockIdx.x, i = k + 1 + blockIdx.y, model = blockIdx.z;
  const int k0 = k * kNB, i0 = i * kT, j0 = j * kT, mi = min(kT, N - i0);
  T* A = ws.A[model];
  T* Z = ws.Z[model];
  const T* Cik = A + size_t(i0) * N + k0;
  if (j <= k) {
    if (!((inv >> model) & 1)) return;
    store_tile<T>(gemm_tile<T, false, false>(Cik, N, Z + size_t(k0) * N + j0, N, mi, kT, kNB), Z + size_t(i0) * N + j0, N, mi, kT,
                  j == k ? kSetNeg : kSub);
  } else if (j <= i) {
    const int mj = min(kT, N - j0);
    store_tile<T>(gemm_tile<T, false, true>(Cik, N, A + size_t(j0) * N + k0, N, mi, mj, kNB), A + size_t(i0) * N + j0, N, mi, mj, kSub);
  }
}

// JOB 0: G = Z^T Z (both models, `inv` ones) into A;  1: T = G M' into Z[0];  2: Y = T G into M.  0 and 2: lower tiles, mirrored.
template <typename T, int JOB> __global__ __launch_bounds__(kBlk) void sst_mm_kernel(Ws<T> ws, int N, int inv) {
  const int b = blockIdx.x, a = blockIdx.y, model = blockIdx.z;
  const int a0 = a * kT, b0 = b * kT, ma = min(kT, N - a0), mb = min(kT, N - b0);
  if (JOB != 1 && b > a) return;
  if (JOB == 0) {
    if (!((inv >> model) & 1)) return;
    const T* Z = ws.Z[model];
    T* G = ws.A[model];
    store_tile<T>(gemm_tile<T, true, false>(Z + size_t(a0) * N + a0, N, Z + size_t(a0) * N + b0, N, ma, mb, N - a0),
                  G + size_t(a0) * N + b0, N, ma, mb, kSet, a != b ? G + size_t(b0) * N + a0 : nullptr);
  } else if (JOB == 1) {
    store_tile<T>(gemm_tile<T, false, false>(ws.A[0] + size_t(a0) * N, N, ws.M + b0, N, ma, mb, N), ws.Z[0] + size_t(a0) * N + b0, N,
                  ma, mb, kSet);
  } else {
    store_tile<T>(gemm_tile<T, false, false>(ws.Z[0] + size_t(a0) * N, N, ws.A[0] + b0, N, ma, mb, N), ws.M + size_t(a0) * N + b0, N,
                  ma, mb, kSet, a != b ? ws.M + size_t(b0) * N + a0 : nullptr);
  }
}

// Row i of the pair vector: mu = w' q(G') per pair, the mode's gradient, and the row's sum of mu delta' in fp64.
template <typename T, int MODE>
__global__ __launch_bounds__(kBlk) void sst_pair_kernel(const T* __restrict__ g, const T* __restrict__ m, int n, T alpha, int np,
                                                        Ws<T> ws, T* __restrict__ grad) {
  constexpr bool INCL = MODE == MM_SST_INCLUSIVE;
  __shared__ T sh[4];
  __shared__ double shd[4];
  const int i = blockIdx.x, N = n - 1;
  T cx, cz;
  shifts(ws.maxp, np, sh, cx, cz);
  const T* __restrict__ Gx = ws.A[0];
  const T* __restrict__ Gz = ws.A[1];
  const T* __restrict__ Y = ws.M;
  const size_t dg = size_t(N) + 1, ri = size_t(i > 0 ? i - 1 : 0) * N;
  const bool in = i > 0;   // (node 0: its row and column of G are zero)
  const T gxii = in ? Gx[(i - 1) * dg] : T(0);
  const T gzii = in && INCL && grad ? Gz[(i - 1) * dg] : T(0);
  const T yii = in && MODE == MM_SST_EXCLUSIVE && grad ? Y[(i - 1) * dg] : T(0);
  const int base = poff(n, i) - i - 1;
  double part = 0.0;
  for (int j = i + 1 + threadIdx.x; j < n; j += kBlk) {
    const int p = base + j;
    T tx, tz;
    thetas<T, INCL>(g[p], m[p], alpha, tx, tz);
    const T wx = Num<T>::exp(tx - cx);
    const T qx = (gxii + Gx[(j - 1) * dg]) - T(2) * (in ? Gx[ri + (j - 1)] : T(0));
    const T mu = wx * qx;
    const T dl = (tz - cz) - (tx - cx);
    part += double(mu) * double(dl);
    if (grad) {
      T d;
      if constexpr (MODE == MM_SST_INCLUSIVE) {
        const T qz = (gzii + Gz[(j - 1) * dg]) - T(2) * (in ? Gz[ri + (j - 1)] : T(0));
        d = mu - Num<T>::exp(tz - cz) * qz;
      } else if constexpr (MODE == MM_SST_EXCLUSIVE) {
        const T qy = (yii + Y[(j - 1) * dg]) - T(2) * (in ? Y[ri + (j - 1)] : T(0));
        d = mu * dl - wx * qy;
      } else {
        d = mu * (tz - tx);
      }
      grad[p] = d;
    }
  }
  part = block_sum(part, shd);
  if (threadIdx.x == 0) ws.pairp[i] = part;
}

template <typename T>
__global__ __launch_bounds__(64) void sst_finish_kernel(const double* __restrict__ logp, int nt, const double* __restrict__ pairp,
                                                        int rows, T* __restrict__ loss_out) {
  double lx = 0.0, lz = 0.0, s = 0.0;
  for (int t = threadIdx.x; t < nt; t += 64) { lx += logp[t]; lz += logp[nt + t]; }
  for (int t = threadIdx.x; t < rows; t += 64) s += pairp[t];
  lx = wave_sum(lx);
  lz = wave_sum(lz);
  s = wave_sum(s);
  if (threadIdx.x == 0) loss_out[0] = T(2.0 * (lz - lx) - s);
}

template <typename T> Ws<T> carve(void* ws, int64_t n) {
  char* p = static_cast<char*>(ws);
  const size_t mb = mat_bytes(sizeof(T), n);
  Ws<T> w;
  w.A[0] = reinterpret_cast<T*>(p);
  w.A[1] = reinterpret_cast<T*>(p + mb);
  w.Z[0] = reinterpret_cast<T*>(p + 2 * mb);
  w.Z[1] = reinterpret_cast<T*>(p + 3 * mb);
  w.M = reinterpret_cast<T*>(p + 4 * mb);
  p += 5 * mb;
  w.maxp = reinterpret_cast<T*>(p);
  p += round256(sizeof(T) * 2 * kMaxP);
  w.logp = reinterpret_cast<double*>(p);
  p += round256(sizeof(double) * 2 * size_t(panels(n)));
  w.pairp = reinterpret_cast<double*>(p);
  return w;
}
inline size_t ws_bytes(size_t el, int64_t n) {
  if (n < 2) return 0;
  return 5 * mat_bytes(el, n) + round256(el * 2 * kMaxP) + round256(sizeof(double) * 2 * size_t(panels(n))) +
      round256(sizeof(double) * size_t(n - 1));
}

template <typename T, int MODE>
int launch(const T* g, const T* m, int64_t n64, T alpha, T* grad, T* loss_out, void* wsp, hipStream_t st) {
  constexpr bool INCL = MODE == MM_SST_INCLUSIVE;
  constexpr bool EXACT = MODE == MM_SST_EXCLUSIVE;
  const int n = int(n64), N = n - 1, nt = panels(n64), npairs = n * (n - 1) / 2;
  const int np = min(kMaxP, (npairs + kBlk - 1) / kBlk);
  const bool exact = EXACT && grad;
  const int inv = (INCL && grad) ? 3 : 1;   // bit per model: its inverse is needed
  const Ws<T> ws = carve<T>(wsp, n64);
  const dim3 wg(kBlk);
  sst_max_kernel<T, INCL><<<dim3(np), wg, 0, st>>>(g, m, npairs, alpha, ws.maxp);
  if (exact) sst_assemble_kernel<T, INCL, EXACT><<<dim3(N, 2), wg, 0, st>>>(g, m, n, alpha, np, ws);
  else sst_assemble_kernel<T, INCL, false><<<dim3(N, 2), wg, 0, st>>>(g, m, n, alpha, np, ws);
  for (int k = 0; k < nt; ++k) {
    sst_diag_kernel<T><<<dim3(1, 1, 2), dim3(kNB * kNB), 0, st>>>(ws, N, k, nt);
    if (nt > 1) sst_panel_kernel<T><<<dim3(nt, 1, 2), wg, 0, st>>>(ws, N, k, inv);
    if (k + 1 < nt) sst_trail_kernel<T><<<dim3(nt, nt - k - 1, 2), wg, 0, st>>>(ws, N, k, inv);
  }
  sst_mm_kernel<T, 0><<<dim3(nt, nt, 2), wg, 0, st>>>(ws, N, inv);
  if (exact) {
    sst_mm_kernel<T, 1><<<dim3(nt, nt, 1), wg, 0, st>>>(ws, N, inv);
    sst_mm_kernel<T, 2><<<dim3(nt, nt, 1), wg, 0, st>>>(ws, N, inv);
  }
  sst_pair_kernel<T, MODE><<<dim3(N), wg, 0, st>>>(g, m, n, alpha, np, ws, grad);
  sst_finish_kernel<T><<<dim3(1), dim3(64), 0, st>>>(ws.logp, nt, ws.pairp, N, loss_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MM_OK : int(e);
}

template <typename T>
int dispatch(int mode, const void* g, const void* m, int64_t n, double alpha, void* grad, void* loss_out, void* ws, hipStream_t st) {
  const T *gp = static_cast<const T*>(g), *mp = static_cast<const T*>(m);
  T *gr = static_cast<T*>(grad), *lo = static_cast<T*>(loss_out);
  switch (mode) {
    case MM_SST_INCLUSIVE: return launch<T, MM_SST_INCLUSIVE>(gp, mp, n, T(alpha), gr, lo, ws, st);
    case MM_SST_EXCLUSIVE: return launch<T, MM_SST_EXCLUSIVE>(gp, mp, n, T(alpha), gr, lo, ws, st);
    default: return launch<T, MM_SST_EXCLUSIVE_REFERENCE>(gp, mp, n, T(alpha), gr, lo, ws, st);
  }
}

}  // namespace sst
}  // namespace mm

using namespace mm::sst;

extern "C" {

size_t mm_sst_kl_ws_bytes(int dtype, int64_t n) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || n > kMaxNodes) return 0;
  return ws_bytes(dtype == MM_F64 ? 8 : 4, n);
}

int mm_sst_kl_loss(int dtype, int mode, const void* target, const void* m, int64_t n, double alpha, void* grad_out,
                   void* loss_out, void* ws, mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || mode < MM_SST_INCLUSIVE || mode > MM_SST_EXCLUSIVE_REFERENCE || n < 0 || !loss_out)
    return MM_ERR_ARG;
  if (n >= 2 && (!target || !m || !ws)) return MM_ERR_ARG;
  if (n > kMaxNodes) return MM_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n < 2) {   // no pair: the loss is 0 and the gradient has no entry
    const hipError_t e = mm::clear_async(loss_out, dtype == MM_F64 ? 8 : 4, st);
    return e == hipSuccess ? MM_OK : int(e);
  }
  return dtype == MM_F32 ? dispatch<float>(mode, target, m, n, alpha, grad_out, loss_out, ws, st)
                         : dispatch<double>(mode, target, m, n, alpha, grad_out, loss_out, ws, st);
}

}  // extern "C"
