// det_common.hpp — what the bit-deterministic pair-gradient modes share (spd_det.hpp, vec_det.hpp): pair gradients WITHOUT float
// atomics, next to the atomic kernels of each family ("Scatter of pair gradients", option b).
//
// Form: BOTH ORDERS, COLUMN-OWNED.  A lane owns one column node c and walks ONE chunk of rows r != c in ascending order, r < c and
// r > c alike; the row operand is wave-uniform.  The pair function is symmetric in its arguments, so the column side of the atomic
// backward applied to EVERY r != c is the whole gradient of node c: there is no row-side sum — no reduction across lanes, no
// atomics — and the price is every pair twice.  A lane's chunk sums leave with plain stores into slab[chunk][entry][c] (coalesced
// per entry); the finalize kernel (one thread per node) adds a node's chunk records in chunk order, applies the family's map and
// writes grad_x.
//
// The loss term and sum dloss/dm d^2 are counted in the r < c visit only, reduced per workgroup in a fixed order (butterfly inside
// a wavefront, wavefronts in index order) and stored to ONE slot per workgroup; finalize adds the slots in fp64, lane t the slots
// t, t + 64, ... in index order, the 64 lane sums through the same butterfly, and writes {loss, sigmoid(scale_raw) sum dloss/dm d^2}.
// (The atomic modes' version, loss_finalize in loss.hpp, has a fixed number of slots and also leaves them clean.)
//
// These two blocks — the tail of each pair_kernel, the head of each finalize_kernel — and the cut of the row window stand in BOTH
// spd_det.hpp and vec_det.hpp, word for word, and are NOT functions of this header: as __forceinline__ device functions (by value,
// by reference, with and without __restrict__) they changed the instruction streams of the kernels that call them (a function's
// pointer parameters are generic where a kernel's are global: the null tests, the order of the loop's phis and of two additions
// came out differently), and the kernels are held to their instruction streams.  A change to one copy is a change to the other.
//
// THE CONTRACT: every order of summation is a pure function of the shape — (element size, bytes of a node's chunk record, n)
// through geometry() below: never of the row range, the device, an occupancy query or the environment.  The kWaves wavefronts of
// a workgroup own DIFFERENT columns (64 each) and walk the same rows: no partial sums of one column are shared between
// wavefronts, so nothing is folded through LDS but the loss record.  Rows that hold no live pair for a wavefront's columns are
// cut off the walk without moving a sum: a lane adds its live pairs in row order either way.  Every record and every slot is
// written by every launch, so the workspace may hold anything.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mm {
namespace det {

// ---- launch geometry: a pure function of (bytes of one node's record in one chunk, n, row quantum) --------------------------------
constexpr int kWaves = 4;                        // wavefronts of a workgroup; each owns 64 columns of its own
constexpr int kCols = 64 * kWaves;               // columns per workgroup
constexpr int kMinRows = 8;                      // rows per chunk at least: a chunk pays a column prologue and a record's stores per lane
constexpr int64_t kTargetWgs = 1024;             // the grid is sized towards this many workgroups (four per CU of an MI355X)
constexpr size_t kSlabCap = size_t(64) << 20;    // the slab is at most max(one record per node, this)

struct DetGeometry {
  int64_t groups, chunks, rows;   // column groups, row chunks, rows per chunk: (chunks - 1) rows < n <= chunks rows
  size_t slab_bytes, slot_bytes;
  size_t bytes() const { return slab_bytes + slot_bytes; }
};
// esz: bytes of an element (the slots are elements); entry_bytes: of one node's record in one chunk; rows per chunk are a multiple
// of row_quantum (1, or the unroll of the family's row walk).  n < 1: no group, and rows = kMinRows — no launch reads it.
inline DetGeometry geometry(size_t esz, size_t entry_bytes, int64_t n, int64_t row_quantum) {
  DetGeometry g{};
  if (n < 1) { g.groups = 0; g.chunks = 1; g.rows = kMinRows; g.slab_bytes = 0; g.slot_bytes = 0; return g; }
  g.groups = (n + kCols - 1) / kCols;
  int64_t want = (kTargetWgs + g.groups - 1) / g.groups;                     // falls as n grows
  const size_t record = entry_bytes * size_t(n);                             // one chunk's records of all nodes
  const int64_t cap = std::max<int64_t>(1, int64_t(kSlabCap / record));      // the slab stays within max(record, kSlabCap)
  want = std::max<int64_t>(1, std::min(want, cap));
  g.rows = std::max<int64_t>(kMinRows, ((n + want - 1) / want + row_quantum - 1) / row_quantum * row_quantum);
  g.chunks = (n + g.rows - 1) / g.rows;
  g.slab_bytes = (size_t(g.chunks) * record + 63) / 64 * 64;
  g.slot_bytes = (2 * size_t(g.groups) * size_t(g.chunks) * esz + 63) / 64 * 64;
  return g;
}

}  // namespace det
}  // namespace mm
