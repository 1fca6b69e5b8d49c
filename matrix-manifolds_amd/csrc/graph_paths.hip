// All-pairs graph distances on the GPU — what data/graph.py (targets) and pyx/__init__.py (the evaluator's shortest-path
// trees) need before the first step, and what scipy's BFS / Dijkstra did on one CPU core (the reference: networkit in
// data/graph.py:15-87, its own BFS / Dijkstra in pyx/impl/precision.cpp:44-92).  Exact integers throughout.
//
// HOPS (unweighted; directed or not): every source at once, one BIT per source.
//   R_L[v] = { s : d(v -> s) <= L }      R_0[v] = {v}      R_L[v] = R_{L-1}[v]  u  U_{u in N(v)} R_{L-1}[u]
// (a shortest v -> s route of L hops leaves v through an OUT-neighbour u with d(u -> s) = L - 1), so the rows of the CSR's
// out-neighbours give D[v][s] = d(v -> s) row-major directly, directed graphs included — no transposed CSR.  Only what is new
// has to travel: with the frontier F_L[v] = R_L[v] \ R_{L-1}[v] the level is  F_L[v] = (U_u F_{L-1}[u]) \ R_{L-1}[v].
// One launch per level; a wavefront owns 64 consecutive 64-bit words of one row v: lane l ORs word w0 + l of the neighbours'
// frontier rows (each a contiguous 512-byte read), masks what v has reached, and the wave then walks its non-zero words —
// the word is broadcast and lane b tests bit b — so that dist[v][64 w + b] = L is written as whole 256-byte runs of the row.
// State: three bit matrices [n][ceil(n / 64)] (reached, two frontiers used alternately by the level's parity: other
// workgroups still read F_{L-1} while F_L is written).  No workgroup reads what another one writes in the same launch.
//
// COSTS (integer edge costs >= 0): blocked Floyd-Warshall over (min, +) in int32, 64 x 64 tiles, ceil(n / 64) rounds of
// {diagonal tile; its row and its column of tiles; the rest}.  256 threads, each owning a 4 x 4 register block; the A tile
// (i, k) and the B tile (k, j) are staged in LDS.  In the first two phases the tile itself is one of its operands: after step
// kk the owners of row / column kk + 1 publish it to LDS — the only part of the evolving tile that step kk + 1 reads (row and
// column kk do not change in step kk: d[kk][kk] = 0).  INF = 2^30 - 1: INF + INF fits an int32, min(c, .) keeps every entry
// <= INF, and rows / columns beyond n read as INF and are not stored.
//
// TARGETS: the work of GraphDataset.__init__ (data/dataset.py:16-19) straight from the int32 matrix — max over the upper
// triangle by a reduction kernel, then T(d) * T(d) / (T(dmax) * T(dmax)) with the maximum read from device memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mm_manifolds.h"
#include "clear.hpp"

namespace mm {
namespace graph_paths {

constexpr int64_t kMaxNodes = 46340;  // n * n < 2^31, as mm_graph_sort_rows
constexpr int kBlock = 256;
constexpr int kTile = 64;
constexpr int kInf = (1 << 30) - 1;

inline int64_t words_per_row(int64_t n) { return (n + 63) / 64; }

inline unsigned grid_for(size_t items, unsigned cap = 1u << 16) {
  const size_t blocks = (items + kBlock - 1) / kBlock;
  return unsigned(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

// ---- hops -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void hops_init_kernel(int n, int W, uint64_t* __restrict__ reached,
                                                            uint64_t* __restrict__ frontier0, int* __restrict__ dist) {
  // (n <= 46340: n * n < 2^31, and the grid's stride is at most 2^24, so 32-bit counters do not wrap)
  const unsigned stride = gridDim.x * kBlock, t0 = blockIdx.x * kBlock + threadIdx.x;
  const unsigned cells = unsigned(n) * unsigned(n), words = unsigned(n) * unsigned(W);
  for (unsigned k = t0; k < cells; k += stride) dist[k] = (k / n == k % n) ? 0 : -1;
  for (unsigned k = t0; k < words; k += stride) {
    const int v = int(k / W), w = int(k % W);
    const uint64_t bit = (v >> 6) == w ? uint64_t(1) << (v & 63) : uint64_t(0);
    reached[k] = bit;
    frontier0[k] = bit;
  }
}

__global__ __launch_bounds__(kBlock) void hops_level_kernel(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                             int n, int W, int chunks, const uint64_t* __restrict__ prev,
                                                             uint64_t* __restrict__ next, uint64_t* __restrict__ reached,
                                                             int* __restrict__ dist, int level, int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t task = int64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);  // wave-uniform: (row v, 64 words of it)
  if (task >= int64_t(n) * chunks) return;
  const int v = int(task / chunks), w0 = int(task % chunks) * 64, w = w0 + lane;
  const bool live = w < W;
  const uint64_t* col = prev + (live ? w : 0);
  uint64_t acc = 0;
  const int e0 = indptr[v], e1 = indptr[v + 1];
  for (int e = e0; e < e1; ++e) {
    const int u = indices[e];
    if (unsigned(u) < unsigned(n) && live) acc |= col[size_t(u) * W];
  }
  uint64_t fresh = 0;
  if (live) {
    const size_t k = size_t(v) * W + w;
    const uint64_t r = reached[k];
    fresh = acc & ~r;
    next[k] = fresh;
    if (fresh) reached[k] = r | fresh;
  }
  uint64_t todo = __ballot(fresh != 0);
  if (todo == 0) return;
  if (lane == 0) *flag = 1;
  int* row = dist + size_t(v) * n;
  while (todo) {  // wave-uniform walk over the lanes that found something
    const int k = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t word = __shfl((unsigned long long)fresh, k);
    const int s = (w0 + k) * 64 + lane;
    if (s < n && ((word >> lane) & 1)) row[s] = level;
  }
}

// ---- costs ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cost_init_kernel(int n, int* __restrict__ dist) {
  const unsigned stride = gridDim.x * kBlock, cells = unsigned(n) * unsigned(n);
  for (unsigned k = blockIdx.x * kBlock + threadIdx.x; k < cells; k += stride) dist[k] = (k / n == k % n) ? 0 : kInf;
}

// one wavefront per row: the cheapest of parallel edges wins (an integer vector atomic: exact, order-free)
__global__ __launch_bounds__(kBlock) void cost_edges_kernel(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                             const int* __restrict__ costs, int n, int* __restrict__ dist) {
  const int v = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (v >= n) return;
  const int e1 = indptr[v + 1];
  for (int e = indptr[v] + (threadIdx.x & 63); e < e1; e += 64) {
    const int u = indices[e], c = costs[e];
    if (unsigned(u) < unsigned(n) && u != v) atomicMin(&dist[size_t(v) * n + u], c < kInf ? c : kInf);
  }
}

__global__ __launch_bounds__(kBlock) void cost_finish_kernel(int n, int* __restrict__ dist) {
  const unsigned stride = gridDim.x * kBlock, cells = unsigned(n) * unsigned(n);
  for (unsigned k = blockIdx.x * kBlock + threadIdx.x; k < cells; k += stride)
    if (dist[k] >= kInf) dist[k] = -1;
}

// PHASE 1: the diagonal tile (k, k); 2: the tiles of row k (blockIdx.y = 0) and of column k (1); 3: every other tile.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void cost_tile_kernel(int* __restrict__ dist, int n, int k) {
  __shared__ int As[kTile][kTile + 1];                            // A[i][kk]: read down a column, one row per register row
  __shared__ __attribute__((aligned(16))) int Bs[kTile][kTile];   // B[kk][j]: read as one int4 per thread
  int ti, tj;
  if (PHASE == 1) {
    ti = tj = k;
  } else if (PHASE == 2) {
    if (int(blockIdx.x) == k) return;
    ti = blockIdx.y == 0 ? k : int(blockIdx.x);
    tj = blockIdx.y == 0 ? int(blockIdx.x) : k;
  } else {
    ti = blockIdx.y;
    tj = blockIdx.x;
    if (ti == k || tj == k) return;
  }
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  for (int idx = tid; idx < kTile * kTile; idx += kBlock) {
    const int r = idx >> 6, c = idx & 63;
    const int ar = ti * kTile + r, ac = k * kTile + c, br = k * kTile + r, bc = tj * kTile + c;
    As[r][c] = (ar < n && ac < n) ? dist[size_t(ar) * n + ac] : kInf;
    Bs[r][c] = (br < n && bc < n) ? dist[size_t(br) * n + bc] : kInf;
  }
  int c[4][4];
  const int i0 = ti * kTile + ty * 4, j0 = tj * kTile + tx * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) c[r][q] = (i0 + r < n && j0 + q < n) ? dist[size_t(i0 + r) * n + j0 + q] : kInf;
  __syncthreads();
  const bool evolve_b = PHASE != 3 && ti == k, evolve_a = PHASE != 3 && tj == k;   // the tile is its own B / A operand
#pragma unroll 4
  for (int kk = 0; kk < kTile; ++kk) {
    int a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = As[ty * 4 + r][kk];
    const int4 bv = *reinterpret_cast<const int4*>(&Bs[kk][tx * 4]);
    const int b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) c[r][q] = min(c[r][q], a[r] + b[q]);
    if (PHASE != 3) {
      const int nx = kk + 1;   // the row / column the next step reads
      if (nx < kTile) {
        if (evolve_b && (nx >> 2) == ty) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r == (nx & 3)) {
#pragma unroll
              for (int q = 0; q < 4; ++q) Bs[nx][tx * 4 + q] = c[r][q];
            }
        }
        if (evolve_a && (nx >> 2) == tx) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q == (nx & 3)) {
#pragma unroll
              for (int r = 0; r < 4; ++r) As[ty * 4 + r][nx] = c[r][q];
            }
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + r < n && j0 + q < n) dist[size_t(i0 + r) * n + j0 + q] = c[r][q];
}

// ---- targets ----------------------------------------------------------------------------------------------------------------
// stats[0] = max finite distance of the upper triangle, stats[1] = its number of -1 entries (cleared by the caller's launch)
__global__ __launch_bounds__(kBlock) void targets_stats_kernel(const int* __restrict__ dist, int n,
                                                                unsigned long long* __restrict__ stats) {
  __shared__ int smax[kBlock / 64];
  __shared__ unsigned long long scnt[kBlock / 64];
  const unsigned stride = gridDim.x * kBlock, cells = unsigned(n) * unsigned(n);
  int mx = 0;
  unsigned long long cnt = 0;
  for (unsigned k = blockIdx.x * kBlock + threadIdx.x; k < cells; k += stride) {
    if (k % n > k / n) {
      const int d = dist[k];
      mx = max(mx, d);
      cnt += d < 0 ? 1 : 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = max(mx, __shfl_xor(mx, off));
    cnt += __shfl_xor(cnt, off);
  }
  if ((threadIdx.x & 63) == 0) {
    smax[threadIdx.x >> 6] = mx;
    scnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) {
      mx = max(mx, smax[w]);
      cnt += scnt[w];
    }
    if (mx > 0) atomicMax(&stats[0], (unsigned long long)mx);
    if (cnt > 0) atomicAdd(&stats[1], cnt);
  }
}

template <typename T> __device__ __forceinline__ T mul_rn(T a, T b);
template <> __device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
template <> __device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
template <typename T> __device__ __forceinline__ T div_rn(T a, T b);
template <> __device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
template <> __device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }
template <typename T> __device__ __forceinline__ T infinity();
template <> __device__ __forceinline__ float infinity() { return __int_as_float(0x7f800000); }
template <> __device__ __forceinline__ double infinity() { return __longlong_as_double(0x7ff0000000000000ll); }

// one workgroup per 64 x 64 tile (bi <= bj) of the upper triangle: the condensed run and the dense tile are written along the
// rows as they are read; the mirrored dense tile goes through LDS so that it, too, is written along its rows
template <typename T>
__global__ __launch_bounds__(kBlock) void targets_scale_kernel(const int* __restrict__ dist, int n,
                                                                const unsigned long long* __restrict__ stats,
                                                                T* __restrict__ condensed, T* __restrict__ dense) {
  __shared__ T tile[kTile][kTile + 1];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  const T dmax = T((long long)stats[0]);
  const T denom = mul_rn(dmax, dmax);
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const int j = bj * kTile + c;
  for (int r = r0; r < kTile; r += kBlock / 64) {
    const int i = bi * kTile + r;
    T val = T(0);
    if (i < n && j < n && j > i) {
      const int d = dist[size_t(i) * n + j];
      const T td = T(d);
      val = d < 0 ? infinity<T>() : div_rn(mul_rn(td, td), denom);
      if (condensed) condensed[int64_t(i) * (2 * int64_t(n) - i - 1) / 2 + (j - i - 1)] = val;
    }
    tile[r][c] = val;   // (zero on and below the diagonal of a diagonal tile)
  }
  if (!dense) return;
  __syncthreads();
  for (int r = r0; r < kTile; r += kBlock / 64) {
    const int i = bi * kTile + r;
    if (i < n && j < n) {
      if (bi != bj) dense[size_t(i) * n + j] = tile[r][c];
      else dense[size_t(i) * n + j] = j > i ? tile[r][c] : j < i ? tile[c][r] : T(0);
    }
    // the mirrored tile (bj, bi): row bj * 64 + r, column bi * 64 + c
    const int mi = bj * kTile + r, mj = bi * kTile + c;
    if (bi != bj && mi < n && mj < n) dense[size_t(mi) * n + mj] = tile[c][r];
  }
}

inline int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MM_OK : int(e);
}

inline int cleared(void* p, size_t bytes, hipStream_t st) {
  const hipError_t e = mm::clear_async(p, bytes, st);
  return e == hipSuccess ? MM_OK : e == hipErrorInvalidValue ? int(MM_ERR_ARG) : int(e);
}

}  // namespace graph_paths
}  // namespace mm

using namespace mm::graph_paths;

extern "C" int64_t mm_graph_max_nodes(void) { return kMaxNodes; }

extern "C" size_t mm_graph_hops_ws_bytes(int64_t n) {
  if (n < 0 || n > kMaxNodes) return 0;
  return size_t(3) * size_t(n) * size_t(words_per_row(n)) * sizeof(uint64_t);
}

extern "C" int mm_graph_hops(const int* indptr, const int* indices, int64_t n, int level_begin, int level_count, int* dist,
                             int* new_bits, void* ws, size_t ws_bytes, mm_stream_t stream) {
  if (n < 0 || n > kMaxNodes || level_begin < 0 || level_count < 1) return MM_ERR_ARG;
  if (int64_t(level_begin) + int64_t(level_count) >= (int64_t(1) << 31)) return MM_ERR_ARG;
  if (n == 0) return MM_OK;
  if (!indptr || !indices || !dist || !new_bits || !ws) return MM_ERR_ARG;
  if (ws_bytes < mm_graph_hops_ws_bytes(n) || (reinterpret_cast<uintptr_t>(ws) & 7)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int W = int(words_per_row(n)), chunks = (W + 63) / 64;
  const size_t words = size_t(n) * W;
  uint64_t* reached = static_cast<uint64_t*>(ws);
  uint64_t* frontier[2] = {reached + words, reached + 2 * words};
  if (int rc = cleared(new_bits, size_t(level_count) * sizeof(int), st)) return rc;
  if (level_begin == 0) {
    hops_init_kernel<<<dim3(grid_for(size_t(n) * n)), dim3(kBlock), 0, st>>>(int(n), W, reached, frontier[0], dist);
    if (int rc = launched()) return rc;
  }
  const int64_t tasks = n * chunks;
  const unsigned blocks = unsigned((tasks + kBlock / 64 - 1) / (kBlock / 64));
  for (int j = 0; j < level_count; ++j) {
    const int level = level_begin + j + 1;
    hops_level_kernel<<<dim3(blocks), dim3(kBlock), 0, st>>>(indptr, indices, int(n), W, chunks, frontier[(level - 1) & 1],
                                                             frontier[level & 1], reached, dist, level, new_bits + j);
    if (int rc = launched()) return rc;
  }
  return MM_OK;
}

extern "C" int mm_graph_cost_paths(const int* indptr, const int* indices, const int* costs, int64_t n, int* dist,
                                   mm_stream_t stream) {
  if (n < 0 || n > kMaxNodes) return MM_ERR_ARG;
  if (n == 0) return MM_OK;
  if (!indptr || !indices || !costs || !dist) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned cells_grid = grid_for(size_t(n) * n);
  cost_init_kernel<<<dim3(cells_grid), dim3(kBlock), 0, st>>>(int(n), dist);
  if (int rc = launched()) return rc;
  cost_edges_kernel<<<dim3(unsigned((n + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st>>>(indptr, indices, costs,
                                                                                                   int(n), dist);
  if (int rc = launched()) return rc;
  const int tiles = int((n + kTile - 1) / kTile);
  for (int k = 0; k < tiles; ++k) {
    cost_tile_kernel<1><<<dim3(1), dim3(kBlock), 0, st>>>(dist, int(n), k);
    if (tiles > 1) {
      cost_tile_kernel<2><<<dim3(tiles, 2), dim3(kBlock), 0, st>>>(dist, int(n), k);
      cost_tile_kernel<3><<<dim3(tiles, tiles), dim3(kBlock), 0, st>>>(dist, int(n), k);
    }
    if (int rc = launched()) return rc;
  }
  cost_finish_kernel<<<dim3(cells_grid), dim3(kBlock), 0, st>>>(int(n), dist);
  return launched();
}

extern "C" int mm_graph_targets(int dtype, const int* dist, int64_t n, int64_t* stats, void* condensed, void* dense,
                                mm_stream_t stream) {
  if ((dtype != MM_F32 && dtype != MM_F64) || n < 0 || n > kMaxNodes || !stats || (n > 0 && !dist)) return MM_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(stats) & 7)) return MM_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = cleared(stats, 2 * sizeof(int64_t), st)) return rc;
  if (n == 0) return MM_OK;
  unsigned long long* ustats = reinterpret_cast<unsigned long long*>(stats);
  targets_stats_kernel<<<dim3(grid_for(size_t(n) * n, 2048)), dim3(kBlock), 0, st>>>(dist, int(n), ustats);
  if (int rc = launched()) return rc;
  if (!condensed && !dense) return MM_OK;
  const unsigned tiles = unsigned((n + kTile - 1) / kTile);
  if (dtype == MM_F32)
    targets_scale_kernel<float><<<dim3(tiles, tiles), dim3(kBlock), 0, st>>>(dist, int(n), ustats, static_cast<float*>(condensed),
                                                                             static_cast<float*>(dense));
  else
    targets_scale_kernel<double><<<dim3(tiles, tiles), dim3(kBlock), 0, st>>>(dist, int(n), ustats, static_cast<double*>(condensed),
                                                                              static_cast<double*>(dense));
  return launched();
}
