"""Right-aligned column blocks of the SPD forward (csrc/spd_ws.hpp, fold_tile / fold_grid on the padded problem), on the
host: tools/micro/shift_check.hip enumerates — with the kernel's own fold_grid, the tile map and the same conversion
`real index = padded - s` — the pairs the shifted forward tiling visits, for every n in 2 ... 300 and 511, 512, 513, 1023, 1025,
wavefront widths 64 and 128, s = (bw - n mod bw) mod bw and five row shards, and requires

* every pair (i, j), rb <= i < re, i < j < n, exactly once, with tiles of 8 and of 2 rows;
* pair_off(n + s, i + s) = pair_off(n, i) + s (2n - 1 + s) / 2;
* the counts of profiles/right_align.md for n = 5000, 4158 and 2274: wavefront-tiles of the forward, and the units the backward's
  walk would have on the padded problem (that walk is not launched: measured, it gains nothing — see there).

No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = ['n=5000 bw=128 s=120 backward units 104800 -> 100120, forward wavefront-tiles 13105 -> 12520',
          'n=4158 bw=128 s=66 backward units 71709 -> 69597, forward wavefront-tiles 8968 -> 8712',
          'n=2274 bw=64 s=30 backward units 42558 -> 41508, forward wavefront-tiles 5325 -> 5220']


def test_shifted_tiling_visits_every_pair_once(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'shift_check')
    subprocess.run([hipcc, '-O1', '-std=c++17', '--offload-arch=gfx950', os.path.join(ROOT, 'tools', 'micro', 'shift_check.hip'), '-o', exe],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'bad = 0' in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
    for line in COUNTS:
        assert line in r.stdout, (line, r.stdout[-1000:])


def test_unit_counts_from_the_formulas():
    """The same counts from ColWalk's formulas in Python integers (no compiler needed): units of the walk before and after."""
    def total(n, rb, re, bw):
        re = max(min(re, n - 1), rb)
        ncb = (n + bw - 1) // bw
        c0 = min((rb + 1) // bw, ncb)
        c1 = min(max(re // bw, c0), ncb)
        if re == rb:
            return 0
        tri = (bw // 2) * (c1 * (c1 - 1) - c0 * (c0 - 1)) + (c1 - c0) * (bw - 1 - rb)
        return tri + (ncb - c1) * (re - rb)
    for n, bw, s, before, after in ((5000, 128, 120, 104800, 100120), (4158, 128, 66, 71709, 69597), (2274, 64, 30, 42558, 41508),
                                    (16384, 64, 0, None, None)):
        assert (bw - n % bw) % bw == s
        if before is None:
            assert total(n, 0, n, bw) == total(n + s, s, n + s, bw)
            continue
        assert total(n, 0, n, bw) == before and total(n + s, s, n + s, bw) == after
        # the identity the relabelling rests on
        for i in (0, 1, n // 2, n - 1, n):
            assert (i + s) * (2 * (n + s) - (i + s) - 1) // 2 == i * (2 * n - i - 1) // 2 + s * (2 * n - 1 + s) // 2
