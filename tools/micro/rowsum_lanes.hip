// Host-side check of the lane map of the SPD backward's row sums (csrc/smallmat.hpp: group_reduce_transposed / group_reduce_slot;
// csrc/spd_pair.hpp stages one LDS plane per 16-lane group and adds the four planes when a segment's row sums leave).
// The four DPP levels (lane bit 3: row_ror:8; bit 2: row_half_mirror; bits 1, 0: quad_perm) are emulated on an array of 64 lanes,
// level by level as wave_reduce_level<2 .. 5> applies them, and for NP = 3, 6, 10 (SPD(2), SPD(3), SPD(4)):
//   * every (lane group, entry) has exactly one writer lane (group_reduce_slot);
//   * the value that writer holds is the sum of the entry over the 16 lanes of its group;
//   * the four planes add up to the wavefront total.
// Values are small integers in double: every sum is exact whatever its order.  No GPU involved; built and run like walk_check.hip:
//   hipcc -O1 -std=c++17 tools/micro/rowsum_lanes.hip -o rowsum_lanes && ./rowsum_lanes
#include <cstdio>
#include <vector>
#include "../../include/mm_manifolds.h"
#include "../../matrix-manifolds_amd/csrc/smallmat.hpp"
using namespace mm;

// the lane a DPP level reads from (dpp_partner<LEVEL> in smallmat.hpp)
static int partner(int level, int lane) {
  const int row = lane & ~15, l = lane & 15;
  switch (level) {
    case 2: return row | ((l + 8) & 15);                     // row_ror:8
    case 3: return row | (l & 8) | (7 - (l & 7));            // row_half_mirror
    case 4: { const int p[4] = {2, 3, 0, 1}; return (lane & ~3) | p[lane & 3]; }   // quad_perm [2,3,0,1]
    default: { const int p[4] = {1, 0, 3, 2}; return (lane & ~3) | p[lane & 3]; }  // quad_perm [1,0,3,2]
  }
}

// wave_reduce_level<2 .. 5> on all 64 lanes at once: v[lane][k]
static std::vector<std::vector<double>> level_step(int level, const std::vector<std::vector<double>>& v) {
  const int n = int(v[0].size()), m = (n + 1) / 2;
  std::vector<std::vector<double>> o(64, std::vector<double>(m));
  for (int lane = 0; lane < 64; ++lane) {
    const bool up = (lane >> (5 - level)) & 1;
    const int p = partner(level, lane);
    for (int k = 0; k < n / 2; ++k) {
      const double keep = up ? v[lane][2 * k + 1] : v[lane][2 * k];
      const double recv = v[p][((p >> (5 - level)) & 1) ? 2 * k : 2 * k + 1];   // what the partner sends
      o[lane][k] = keep + recv;
    }
    if (n & 1) o[lane][m - 1] = v[lane][n - 1] + v[p][n - 1];
  }
  return o;
}

template <int NP> static long check() {
  long bad = 0;
  std::vector<std::vector<double>> v(64, std::vector<double>(NP));
  unsigned s = 12345u + NP;
  for (int lane = 0; lane < 64; ++lane)
    for (int k = 0; k < NP; ++k) { s = s * 1664525u + 1013904223u; v[lane][k] = double(int(s >> 20) - 2048); }
  auto r = v;
  for (int level = 2; level <= 5; ++level) r = level_step(level, r);
  if (r[0].size() != 1) { printf("NP=%d: %zu values left per lane\n", NP, r[0].size()); return 1; }
  double plane[4][NP];
  int writers[4][NP] = {};
  for (int lane = 0; lane < 64; ++lane) {
    bool writer;
    const int slot = group_reduce_slot<NP>(lane, writer);
    const int g = lane >> 4;
    if (slot < 0 || slot >= NP) { ++bad; printf("NP=%d lane %d: slot %d\n", NP, lane, slot); continue; }
    double sum = 0;
    for (int l = 16 * g; l < 16 * g + 16; ++l) sum += v[l][slot];
    // (duplicates too: every lane holds the group sum of the entry its slot names)
    if (r[lane][0] != sum) { if (++bad < 10) printf("NP=%d lane %d slot %d: holds %g, group sum %g\n", NP, lane, slot, r[lane][0], sum); }
    if (writer) { ++writers[g][slot]; plane[g][slot] = r[lane][0]; }
  }
  for (int g = 0; g < 4; ++g)
    for (int k = 0; k < NP; ++k)
      if (writers[g][k] != 1) { ++bad; printf("NP=%d group %d entry %d: %d writers\n", NP, g, k, writers[g][k]); }
  if (bad) return bad;
  for (int k = 0; k < NP; ++k) {
    double tot = 0;
    for (int lane = 0; lane < 64; ++lane) tot += v[lane][k];
    if (plane[0][k] + plane[1][k] + plane[2][k] + plane[3][k] != tot) { ++bad; printf("NP=%d entry %d: planes do not add up\n", NP, k); }
  }
  return bad;
}

int main() {
  const long bad = check<3>() + check<6>() + check<10>();
  printf("rowsum lane map: bad = %ld\n", bad);
  return bad != 0;
}
