"""CPU-only checks of the all-pairs graph distances (csrc/graph_paths.hip): the entry points are declared, exported and refuse bad
arguments before anything touches a GPU; the plain-Python oracle of tests/graph_paths_cases.py equals scipy on every case and the
case table has the properties it claims; the Python layer returns on the CPU exactly what the scipy route returns, honours
MM_GRAPH_APSP=scipy and refuses costs outside the precondition; no graph_paths kernel uses scratch.  Runs no kernel."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import graph_paths_cases as gc
from graphembed import _backend as B

NEW = ('mm_graph_max_nodes', 'mm_graph_hops_ws_bytes', 'mm_graph_hops', 'mm_graph_cost_paths', 'mm_graph_targets')
MAX_NODES = 46340


def _as_int(d):
    return np.where(np.isfinite(d), d, -1).astype(np.int32)


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert B.lib().raw('mm_abi_version')() == 4
    assert B.lib().raw('mm_graph_max_nodes')() == MAX_NODES and MAX_NODES**2 < 2**31 <= (MAX_NODES + 1)**2


def test_hops_workspace_formula():
    ws = B.lib().raw('mm_graph_hops_ws_bytes')
    for n in (0, 1, 2, 63, 64, 65, 128, 129, 257, 4039, 16384, MAX_NODES):
        assert ws(n) == 3 * n * ((n + 63) // 64) * 8, n   # three bit matrices [n][ceil(n / 64)] of 64-bit words
    assert ws(-1) == 0 and ws(MAX_NODES + 1) == 0 and ws(1 << 40) == 0


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_int64 * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    hops, costs, targets = (lib.raw(k) for k in ('mm_graph_hops', 'mm_graph_cost_paths', 'mm_graph_targets'))
    big = lib.raw('mm_graph_hops_ws_bytes')(10)

    def h(indptr=q, indices=q, n=10, lb=0, lc=1, dist=q, flags=q, ws=q, ws_bytes=big):
        return hops(indptr, indices, n, lb, lc, dist, flags, ws, ws_bytes, None)

    for name in ('indptr', 'indices', 'dist', 'flags', 'ws'):
        assert h(**{name: None}) == -1, name
    assert h(n=-1) == -1 and h(n=MAX_NODES + 1) == -1
    assert h(lb=-1) == -1 and h(lc=0) == -1 and h(lc=-3) == -1
    assert h(ws_bytes=big - 1) == -1 and h(ws_bytes=0) == -1
    assert h(lb=2**31 - 1, lc=1) == -1 and h(lb=2**31 - 9, lc=9) == -1 and h(lb=2**30, lc=2**30) == -1
    assert h(ws=ctypes.c_void_p(q.value + 4)) == -1                      # ws holds 64-bit words
    assert h(n=0, indptr=None, indices=None, dist=None, flags=None, ws=None, ws_bytes=0) == 0   # nothing to do

    def c(indptr=q, indices=q, cst=q, n=10, dist=q):
        return costs(indptr, indices, cst, n, dist, None)

    assert c(indptr=None) == -1 and c(indices=None) == -1 and c(cst=None) == -1 and c(dist=None) == -1
    assert c(n=-1) == -1 and c(n=MAX_NODES + 1) == -1
    assert c(n=0, indptr=None, indices=None, cst=None, dist=None) == 0

    def t(dtype=B.MM_F32, dist=q, n=10, stats=q, condensed=q, dense=q):
        return targets(dtype, dist, n, stats, condensed, dense, None)

    assert t(dtype=2) == -1 and t(dtype=-1) == -1 and t(dist=None) == -1 and t(stats=None) == -1
    assert t(n=-1) == -1 and t(n=MAX_NODES + 1) == -1 and t(stats=ctypes.c_void_p(q.value + 4)) == -1
    with pytest.raises(B.BackendError):
        lib.call('mm_graph_hops', q, q, 10, 0, 0, q, q, q, big, None)


@pytest.mark.parametrize('case', gc.ALL_CASES, ids=repr)
def test_oracle_equals_scipy(case):
    from scipy.sparse.csgraph import shortest_path
    m = case.scipy_matrix()
    want = shortest_path(m, method='D', unweighted=not case.weighted, directed=case.directed)
    got = case.oracle()
    assert got.dtype == np.int32 and got.shape == (case.n, case.n)
    assert np.array_equal(got, _as_int(want))
    if not case.weighted:   # scipy's BFS as well (what compute_graph_pdists calls)
        assert np.array_equal(got, _as_int(shortest_path(m, unweighted=True, directed=case.directed)))
    if not case.directed:
        assert np.array_equal(got, got.T)


def test_case_table_has_the_properties_it_claims():
    from graphembed.data import graph as G
    assert G.LEVEL_BATCH == gc.LEVEL_BATCH
    assert sorted({c.n for c in gc.ALL_CASES}) == sorted(gc.SIZES + (1025, ))
    for n in gc.SIZES:
        names = {c.name for c in gc.ALL_CASES if c.n == n}
        for shape in ('path', 'cycle', 'star', 'complete', 'tree', 'gnm', 'noedges', 'dicycle', 'cost19', 'cost-zero'):
            assert f'{shape}-{n}' in names, (shape, n)
        if n >= 63:
            for shape in ('components', 'digraph', 'loops', 'cost-detour', 'cost-parallel', 'cost-components'):
                assert f'{shape}-{n}' in names, (shape, n)
    for c in gc.ALL_CASES:
        d = c.oracle()
        assert (np.diag(d) == 0).all()
        if 'path' in c.tags and c.n >= 63:
            assert gc.diameter(d) == c.n - 1 > 2 * gc.LEVEL_BATCH            # several level batches
        if 'connected' in c.tags and 'directed' not in c.tags:
            assert (d >= 0).all(), c
        if 'disconnected' in c.tags:
            assert (d < 0).any() and (np.triu(d, 1) < 0).any(), c          # unreachable pairs, also where the targets look
        if 'multi' in c.tags:
            pairs = [(v, int(u)) for v in range(c.n) for u in c.indices[c.indptr[v]:c.indptr[v + 1]]]
            assert len(set(pairs)) < len(pairs) and any(v == u for v, u in pairs), c   # repeated neighbours and self-loops
        if c.weighted and c.costs.size:
            assert int(c.costs.min()) >= 0 and (c.n - 1) * int(c.costs.max()) < gc.COST_BOUND, c
        if 'zero' in c.tags:
            assert c.n < 63 or ((c.costs == 0).any() and (d[~np.eye(c.n, dtype=bool)] == 0).any())
        if 'detour' in c.tags:      # the direct edge (v, v + 20) costs 40, the ring gets there for 20
            hops = gc.bfs_all(c.indptr, c.indices, c.n)
            assert d[0][20] == 20 and hops[0][20] == 1
        if 'bound' in c.tags:
            worst = (c.n - 1) * int(c.costs.max())
            assert 0.99 * gc.COST_BOUND <= worst < gc.COST_BOUND and gc.diameter(d) == worst   # within 1 % of the bound, and reached
    big = gc.BY_NAME['cost19-1025']
    assert (big.n + 63) // 64 == 17
    assert any('directed' in c.tags and (c.oracle() < 0).any() for c in gc.HOP_CASES)


CPU_CASES = ('gnm-65', 'components-129', 'digraph-64', 'path-63', 'cost19-65', 'cost-digraph-64', 'cost-zero-63')


@pytest.mark.parametrize('name', CPU_CASES)
def test_python_layer_on_the_cpu_is_the_scipy_route(name, monkeypatch):
    """graph_distances / compute_graph_pdists / GraphDataset.from_graph on the CPU against scipy called as the parent commit called it"""
    import networkx as nx
    from scipy.sparse.csgraph import shortest_path
    from scipy.spatial.distance import squareform
    from graphembed.data import GraphDataset
    from graphembed.data import graph as G
    case = gc.BY_NAME[name]
    g = case.networkx()
    for env in (None, 'scipy'):
        if env:
            monkeypatch.setenv('MM_GRAPH_APSP', env)
        if case.weighted:
            a = nx.to_scipy_sparse_array(g, nodelist=range(case.n), weight='weight')
            want = shortest_path(a, method='D', unweighted=False, directed=g.is_directed())
            got = G.graph_distances(g, 'cpu', weight='weight')
        else:
            a = nx.to_scipy_sparse_array(g, nodelist=range(case.n))
            want = shortest_path(a, unweighted=True, directed=g.is_directed())
            got = G.graph_distances(g, 'cpu')
        assert got.dtype == torch.int32 and got.device.type == 'cpu'
        assert np.array_equal(got.numpy(), _as_int(want)) and np.array_equal(got.numpy(), case.oracle())
        if case.weighted:
            continue
        pd = G.compute_graph_pdists(g)
        assert pd.dtype == np.float64 and np.array_equal(pd, squareform(want, checks=False))
        if 'disconnected' in case.tags:
            assert np.isinf(pd).any()
            with pytest.raises(ValueError):
                GraphDataset.from_graph(g, 'cpu')
        else:
            for dtype in (torch.float32, torch.float64):
                ds = GraphDataset.from_graph(g, 'cpu', dtype)
                ref = GraphDataset(torch.from_numpy(pd).to(dtype))
                assert ds.condensed.dtype == dtype and torch.equal(ds.condensed, ref.condensed) and len(ds) == case.n


def test_compute_graph_pdists_caches_the_same_vector(tmp_path):
    from graphembed.data import graph as G
    g = gc.BY_NAME['tree-65'].networkx()
    pd = G.compute_graph_pdists(g, str(tmp_path))
    assert np.array_equal(np.load(tmp_path / G.CACHED_PDISTS_FILE), pd)


def test_switch_forces_scipy(monkeypatch):
    """MM_GRAPH_APSP=scipy: the GPU route is off whatever the machine has; otherwise it needs a GPU and the built library"""
    from graphembed.data import graph as G
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.delenv('MM_GRAPH_APSP', raising=False)
    assert G.gpu_apsp_enabled() == os.path.isfile(B.LIB_PATH)
    monkeypatch.setenv('MM_GRAPH_APSP', 'scipy')
    assert not G.gpu_apsp_enabled()
    monkeypatch.setenv('MM_GRAPH_APSP', 'gpu')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert not G.gpu_apsp_enabled()
    for doc in ('INTEGRATION.md', 'README.md'):   # documented next to the other MM_* switches
        assert 'MM_GRAPH_APSP' in open(os.path.join(ROOT, doc)).read(), doc


def test_python_layer_refuses_costs_outside_the_precondition():
    import networkx as nx
    from graphembed.data import graph as G
    from graphembed.pyx import FastPrecision

    def graph(cost, n=5):
        g = nx.path_graph(n)
        nx.set_edge_attributes(g, 1, 'weight')
        g[1][2]['weight'] = cost
        return g

    for bad in (-1, 2.5, float('nan'), 2**30, (2**30 - 1) // 4 + 1):
        with pytest.raises(ValueError):
            G.graph_distances(graph(bad), 'cpu', weight='weight')
    ok = (2**30 - 2) // 4
    d = G.graph_distances(graph(ok), 'cpu', weight='weight')
    assert int(d[1][2]) == ok and int(d[0][4]) == ok + 3
    indptr, indices, costs = G.weighted_csr(graph(7), 'weight')
    assert indptr.dtype == indices.dtype == costs.dtype == np.int32 and list(indptr) == [0, 1, 3, 5, 7, 8]
    assert list(indices) == [1, 0, 2, 1, 3, 2, 4, 3] and list(costs) == [1, 1, 7, 7, 1, 1, 1, 1]
    with pytest.raises(ValueError, match='weighted graphs need integer edge costs'):      # the evaluator's own message
        FastPrecision(graph(2.5), device='cpu')


def test_graph_paths_kernels_keep_everything_in_registers():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    if not (os.path.exists(os.path.join(kernel_meta.LLVM, 'llvm-objdump')) and os.path.exists(kernel_meta.LIB)):
        pytest.skip('needs the ROCm llvm tools and the built library')
    ks = {nm: k for nm, k in kernel_meta.kernels().items() if nm.startswith('graph_paths::')}
    want = {'graph_paths::hops_init_kernel', 'graph_paths::hops_level_kernel', 'graph_paths::cost_init_kernel',
            'graph_paths::cost_edges_kernel', 'graph_paths::cost_finish_kernel', 'graph_paths::cost_tile_kernel<1>',
            'graph_paths::cost_tile_kernel<2>', 'graph_paths::cost_tile_kernel<3>', 'graph_paths::targets_stats_kernel',
            'graph_paths::targets_scale_kernel<float>', 'graph_paths::targets_scale_kernel<double>'}
    assert set(ks) == want, sorted(ks)
    for nm, k in ks.items():
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
        if 'tile' in nm or 'scale' in nm:
            print(f'{nm}: LDS {k["lds"]} bytes, {k["vgpr"]} VGPRs')
            assert 0 < k['lds'] <= 64 * 1024, (nm, k)
