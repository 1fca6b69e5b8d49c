// Host-side check of the right-aligned column blocks of the SPD forward (csrc/spd_ws.hpp: fold_tile / fold_grid on the padded
// problem): with s = (bw - n mod bw) mod bw phantom nodes in front, the padded tiling — converted at the tile's origin exactly as
// spd_pdist_fwd_kernel converts it (real index = padded - s, a column is live iff 0 <= j < n) — visits every pair (i, j),
// rb <= i < re, i < j < n, exactly once; the pair offset is shift-invariant up to the constant s (2n - 1 + s) / 2; and the
// wavefront-tile counts of profiles/right_align.md hold (with the units the backward's walk WOULD have on the padded problem:
// that walk is not launched, see there).  No GPU involved: tests/test_spd_shift_host.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/mm_manifolds.h"
#include "../../matrix-manifolds_amd/csrc/spd_ws.hpp"
using namespace mm;

static long bad = 0, checked = 0;
#define FAIL(...) do { if (++bad < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

// fold_tile on the host: the tile of workgroup (x, y) — the device function reads blockIdx
struct HostTile { int i0, jbase; bool ok; };
static HostTile host_fold_tile(int TI, int BW, int n, int row_begin, int row_end, int bx, int by) {
  const int gy = (row_end - row_begin + TI - 1) / TI;
  const int nJB = (n + BW - 1) / BW;
  int y = by, x = bx;
  int cb0 = (row_begin + y * TI + 1) / BW;
  int cnt = nJB - cb0;
  if (x >= cnt) {
    x -= cnt;
    const int y2 = gy - 1 - y;
    if (y2 <= y) return {0, 0, false};
    y = y2;
    cb0 = (row_begin + y * TI + 1) / BW;
    cnt = nJB - cb0;
    if (x >= cnt) return {0, 0, false};
  }
  return {row_begin + y * TI, (cb0 + x) * BW, true};
}
template <int TI, int BW> static dim3 grid_of(int n, int rb, int re) { return fold_grid<TI, BW>(n, rb, re); }

// Wavefront-tiles of a forward launch that reach their row loop (spd_pdist_fwd_kernel: not below the diagonal, not beyond n), and
// the pairs they store into seen[]
template <int TI> static long forward_visit(int n, int rb, int re, int bw, int s, std::vector<unsigned char>* seen) {
  const int NCW = 4;   // wavefronts of a workgroup; the tile is NCW * bw columns wide
  long waves = 0;
  dim3 g = bw == 64 ? grid_of<TI, 256>(n + s, rb + s, re + s) : grid_of<TI, 512>(n + s, rb + s, re + s);
  for (unsigned by = 0; by < g.y; ++by) for (unsigned bx = 0; bx < g.x; ++bx) {
    const HostTile t = host_fold_tile(TI, NCW * bw, n + s, rb + s, re + s, int(bx), int(by));
    if (!t.ok) continue;
    const int i0 = t.i0 - s, i1 = i0 + TI < re ? i0 + TI : re;
    if (i0 < rb || i0 >= re) { FAIL("fwd n=%d s=%d rows [%d,%d): tile row %d", n, s, rb, re, i0); continue; }
    for (int w = 0; w < NCW; ++w) {
      const int wj0 = t.jbase - s + w * bw;
      if (wj0 + bw - 1 <= i0) continue;
      if (wj0 >= n) continue;
      ++waves;
      if (!seen) continue;
      for (int i = i0; i < i1; ++i) for (int l = 0; l < bw; ++l) {
        const int j = wj0 + l;
        if (!(unsigned(j) < unsigned(n)) || !(j > i)) continue;
        ++(*seen)[size_t(i) * n + j];
      }
    }
  }
  return waves;
}

static void expect_all_once(const std::vector<unsigned char>& seen, int n, int rb, int re, const char* what, int bw, int s) {
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
    const int want = (i >= rb && i < re && j > i) ? 1 : 0;
    ++checked;
    if (seen[size_t(i) * n + j] != want) { FAIL("%s n=%d bw=%d s=%d rows [%d,%d): pair (%d,%d) seen %d times", what, n, bw, s, rb, re, i, j, int(seen[size_t(i) * n + j])); return; }
  }
}

int main() {
  std::vector<int> sizes;
  for (int n = 2; n <= 300; ++n) sizes.push_back(n);
  for (int n : {511, 512, 513, 1023, 1025}) sizes.push_back(n);
  for (int n : sizes) for (int bw : {64, 128}) {
    const int s = (bw - n % bw) % bw;
    // the pair-offset identity: pair_off(n + s, i + s) = pair_off(n, i) + s (2n - 1 + s) / 2
    const int64_t shift_const = int64_t(s) * (2 * int64_t(n) - 1 + s) / 2;
    for (int i = 0; i <= n; ++i) { ++checked; if (pair_off(n + s, i + s) != pair_off(n, i) + shift_const) FAIL("pair_off n=%d s=%d i=%d", n, s, i); }
    if ((n + s) % bw != 0 || s < 0 || s >= bw) FAIL("shift n=%d bw=%d s=%d", n, bw, s);
    const int shards[5][2] = {{0, n}, {0, n / 3}, {n / 3, n}, {n - 2 > 0 ? n - 2 : 0, n}, {n / 3, (2 * n) / 3}};
    for (const auto& sd : shards) {
      const int rb = sd[0], re = sd[1];
      if (re <= rb) continue;
      for (int both = 0; both < 2; ++both) {
        const int ss = both ? s : 0;   // (the plain walk through the same enumeration: the enumeration itself is held to the truth)
        std::vector<unsigned char> seen(size_t(n) * n, 0);
        forward_visit<8>(n, rb, re, bw, ss, &seen);
        expect_all_once(seen, n, rb, re, "forward TI=8", bw, ss);
        std::fill(seen.begin(), seen.end(), 0);
        forward_visit<2>(n, rb, re, bw, ss, &seen);
        expect_all_once(seen, n, rb, re, "forward TI=2", bw, ss);
      }
    }
  }
  // the unit counts of the table in profiles/right_align.md: n, bw, s, backward units before -> after, forward wavefront-tiles
  const struct { int n, bw, s; long bu0, bu1, fw0, fw1; } rows[] = {
      {5000, 128, 120, 104800, 100120, 13105, 12520},
      {4158, 128, 66, 71709, 69597, 8968, 8712},
      {2274, 64, 30, 42558, 41508, 5325, 5220},
  };
  for (const auto& t : rows) {
    const int s = (t.bw - t.n % t.bw) % t.bw;
    const long bu0 = long(ColWalk(t.n, 0, t.n, t.bw).total()), bu1 = long(ColWalk(t.n + s, s, t.n + s, t.bw).total());
    const long fw0 = forward_visit<8>(t.n, 0, t.n, t.bw, 0, nullptr), fw1 = forward_visit<8>(t.n, 0, t.n, t.bw, s, nullptr);
    ++checked;
    printf("n=%d bw=%d s=%d backward units %ld -> %ld, forward wavefront-tiles %ld -> %ld\n", t.n, t.bw, s, bu0, bu1, fw0, fw1);
    if (s != t.s || bu0 != t.bu0 || bu1 != t.bu1 || fw0 != t.fw0 || fw1 != t.fw1) FAIL("unit counts n=%d", t.n);
  }
  {
    const int n = 16384, bw = 64, s = (bw - n % bw) % bw;
    if (s != 0) FAIL("n=16384 has a shift");
  }
  printf("checked %ld, bad = %ld\n", checked, bad);
  return bad != 0;
}
