"""Lane map of the SPD backward's row sums by lane groups, on the host: tools/micro/rowsum_lanes.hip emulates the four DPP levels
on 64 lanes and holds group_reduce_slot (csrc/smallmat.hpp) to them for NP = 3, 6, 10 — one writer per (lane group, entry), the
writer holds its group's sum, the four planes add up to the wavefront total.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_reduction_lane_map(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'rowsum_lanes')
    subprocess.run([hipcc, '-O1', '-std=c++17', '--offload-arch=gfx950', os.path.join(ROOT, 'tools', 'micro', 'rowsum_lanes.hip'), '-o', exe],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'bad = 0' in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
