"""The all-pairs graph distances on the GPU (csrc/graph_paths.hip) against the plain-Python BFS / Dijkstra of
tests/graph_paths_cases.py: mm_graph_hops and mm_graph_cost_paths through the C ABI on every case (equality: the answers are
integers), the level batching of the hops entry, mm_graph_targets against GraphDataset on the CPU (equality: one correctly rounded
multiply and one correctly rounded divide per element on both sides), and the Python layer — FastPrecision and
GraphDataset.from_graph built on the device against the scipy route."""
import numpy as np
import pytest
import torch

import graph_paths_cases as gc
from graphembed import _backend as B

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the oracle's matrices are shared and read-only)


def _csr(case):
    indices = case.indices if case.indices.size else np.zeros(1, dtype=np.int32)   # (a pointer to something for the edgeless cases)
    costs = None
    if case.weighted:
        costs = _dev(case.costs if case.costs.size else np.zeros(1, dtype=np.int32))
    return _dev(case.indptr), _dev(indices), costs


def _hops(case, batch, extra=0, flags_out=None):
    """the hop matrix through mm_graph_hops issued `batch` levels per call until a call's last flag is 0, then `extra` more levels;
    ws and dist start as 0xFF bytes.  flags_out collects every flag in level order."""
    lib = B.lib()
    n = case.n
    indptr, indices, _ = _csr(case)
    nbytes = lib.raw('mm_graph_hops_ws_bytes')(n)
    ws = torch.full((max(nbytes // 8, 1), ), -1, dtype=torch.int64, device=DEV)
    dist = torch.full((n, n), -1, dtype=torch.int32, device=DEV)
    dist.view(torch.uint8).fill_(0xFF)
    st = B.stream_of(dist)
    level, flags_all = 0, []
    while True:
        flags = torch.full((batch, ), 7, dtype=torch.int32, device=DEV)
        lib.call('mm_graph_hops', B.ptr(indptr), B.ptr(indices), n, level, batch, B.ptr(dist), B.ptr(flags), B.ptr(ws), nbytes, st)
        level += batch
        f = flags.cpu().tolist()
        flags_all += f
        if f[-1] == 0:
            break
        assert level <= n + batch, 'the frontier must empty within n levels'
    if extra:
        before = dist.clone()
        flags = torch.full((extra, ), 7, dtype=torch.int32, device=DEV)
        lib.call('mm_graph_hops', B.ptr(indptr), B.ptr(indices), n, level, extra, B.ptr(dist), B.ptr(flags), B.ptr(ws), nbytes, st)
        assert flags.cpu().tolist() == [0] * extra
        assert torch.equal(dist, before)
    if flags_out is not None:
        flags_out.extend(flags_all)
    return dist


@pytest.mark.parametrize('case', gc.HOP_CASES, ids=repr)
def test_hops_equal_the_bfs_oracle(case):
    got = _hops(case, gc.LEVEL_BATCH)
    assert torch.equal(got.cpu(), torch.from_numpy(case.oracle().copy()))


@pytest.mark.parametrize('case', gc.COST_CASES, ids=repr)
def test_costs_equal_the_dijkstra_oracle(case):
    n = case.n
    indptr, indices, costs = _csr(case)
    dist = torch.empty(n, n, dtype=torch.int32, device=DEV)
    dist.view(torch.uint8).fill_(0xFF)
    B.lib().call('mm_graph_cost_paths', B.ptr(indptr), B.ptr(indices), B.ptr(costs), n, B.ptr(dist), B.stream_of(dist))
    assert torch.equal(dist.cpu(), torch.from_numpy(case.oracle().copy()))


@pytest.mark.parametrize('name', ('path-65', 'path-129', 'gnm-257', 'digraph-129', 'components-65', 'noedges-64', 'dicycle-63'))
def test_level_batching(name):
    """1, 3 and 64 levels per call give the same matrix; eight more levels after convergence change nothing and set no flag; the
    last flag that is set sits at the oracle's diameter"""
    case = gc.BY_NAME[name]
    want = torch.from_numpy(case.oracle().copy())
    diam = gc.diameter(case.oracle())
    for batch in (1, 3, 64):
        flags = []
        got = _hops(case, batch, extra=8, flags_out=flags)
        assert torch.equal(got.cpu(), want), batch
        assert flags[:diam] == [1] * diam and not any(flags[diam:]), (batch, diam, flags)   # level L is flags[L - 1]


TARGET_CASES = ('path-2', 'gnm-63', 'tree-65', 'cycle-129', 'gnm-257', 'dicycle-64', 'cost19-65', 'cost-bound-129')


def _targets(dist, dtype, condensed=True, dense=True):
    n = dist.shape[0]
    stats = torch.full((2, ), -5, dtype=torch.int64, device=DEV)
    cond = torch.full((n * (n - 1) // 2, ), float('nan'), dtype=dtype, device=DEV) if condensed else None
    dns = torch.full((n, n), float('nan'), dtype=dtype, device=DEV) if dense else None
    B.lib().call('mm_graph_targets', B.MM_F32 if dtype == torch.float32 else B.MM_F64, B.ptr(dist), n, B.ptr(stats), B.ptr(cond),
                 B.ptr(dns), B.stream_of(dist))
    return stats.cpu().tolist(), cond, dns


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64), ids=('f32', 'f64'))
@pytest.mark.parametrize('name', TARGET_CASES)
def test_targets_equal_graph_dataset(name, dtype):
    case = gc.BY_NAME[name]
    oracle = case.oracle()
    assert (oracle >= 0).all()
    want_c, want_d = gc.targets_reference(oracle, dtype)
    dist = _dev(oracle)
    stats, cond, dns = _targets(dist, dtype)
    upper = oracle[np.triu_indices(case.n, 1)]
    assert stats == [int(upper.max()) if upper.size else 0, 0]
    assert torch.equal(cond.cpu(), want_c)
    assert torch.equal(dns.cpu(), want_d)
    # either output alone
    _, cond1, none = _targets(dist, dtype, dense=False)
    _, none2, dns1 = _targets(dist, dtype, condensed=False)
    assert none is None and none2 is None and torch.equal(cond1, cond) and torch.equal(dns1, dns)


@pytest.mark.parametrize('dtype', (torch.float32, torch.float64), ids=('f32', 'f64'))
@pytest.mark.parametrize('name', ('components-129', 'digraph-65', 'cost-components-65'))
def test_targets_of_a_disconnected_graph(name, dtype):
    case = gc.BY_NAME[name]
    oracle = case.oracle()
    iu = np.triu_indices(case.n, 1)
    upper = oracle[iu]
    assert (upper < 0).any() and (upper > 0).any()
    stats, cond, dns = _targets(_dev(oracle), dtype)
    assert stats == [int(upper.max()), int((upper < 0).sum())]
    t = torch.from_numpy(upper.astype(np.float64)).to(dtype)
    m = torch.tensor(float(upper.max()), dtype=torch.float64).to(dtype)
    want = torch.where(torch.from_numpy(upper < 0), torch.tensor(float('inf'), dtype=dtype), t * t / (m * m))
    assert torch.equal(cond.cpu(), want)
    dense = torch.zeros(case.n, case.n, dtype=dtype)
    dense[iu[0], iu[1]] = want
    dense = dense + dense.T
    assert torch.equal(dns.cpu(), dense)


def _fast_precision_pair(g, monkeypatch):
    from graphembed.pyx import FastPrecision
    monkeypatch.delenv('MM_GRAPH_APSP', raising=False)
    ours = FastPrecision(g, device=DEV)
    monkeypatch.setenv('MM_GRAPH_APSP', 'scipy')
    ref = FastPrecision(g, device=DEV)
    monkeypatch.delenv('MM_GRAPH_APSP', raising=False)
    return ours, ref


@pytest.mark.parametrize('name', ('gnm-129', 'cost19-65'))
def test_fast_precision_on_the_device_equals_the_scipy_route(name, monkeypatch):
    """Everything the evaluator keeps is EQUAL on both routes — hops, num_layers, nodes_per_layer, the CSR — and so is the mean
    average precision (a deterministic kernel).  The layer F1 scores cannot be compared by equality: mm_graph_layer_f1 (not touched
    here) sums them with fp64 atomics in whatever order the workgroups arrive, and ONE evaluator gives a different last bit from call
    to call — measured on the MI355X on these two cases: 6 calls of the scipy-route instance gave 6 distinct results, spread
    4.4e-16 ... 7.2e-16; device route against scipy route 5.6e-16 ... 8.3e-16, the same size.  With every input of that kernel equal
    bit for bit, the scores may differ by the reordering of a sum only: each is a sum of at most n^2 terms in [0, 1] over a count,
    two orders of such a sum differ by at most 2 (n^2 - 1) u times the sum (u = 2^-53), and the variance m2 / cnt - mean^2 by three
    such terms; 8 n^2 u covers both (1.5e-11 at n = 129)."""
    case = gc.BY_NAME[name]
    g = case.networkx()
    ours, ref = _fast_precision_pair(g, monkeypatch)
    assert ours.weighted == ref.weighted == case.weighted
    assert ours.hops.is_cuda and ours.hops.dtype == ref.hops.dtype == torch.int32 and torch.equal(ours.hops, ref.hops)
    assert ours.num_layers == ref.num_layers and ours.nodes_per_layer() == ref.nodes_per_layer()
    assert torch.equal(ours.indptr, ref.indptr) and torch.equal(ours.indices, ref.indices) and ours.n == ref.n
    pd = torch.rand(case.n * (case.n - 1) // 2, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    assert ours.mean_average_precision(pd) == ref.mean_average_precision(pd)
    bound = 8 * case.n**2 * 2.0**-53
    for a, b in zip(ours.layer_mean_f1_scores(pd), ref.layer_mean_f1_scores(pd)):
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
        diff = float(np.nanmax(np.abs(a - b)))
        print(f'{name}: layer F1 device route vs scipy route, max difference {diff:.2e} (bound {bound:.2e})')
        assert diff <= bound


def test_fast_precision_keeps_its_error_texts(monkeypatch):
    from graphembed.pyx import FastPrecision
    monkeypatch.delenv('MM_GRAPH_APSP', raising=False)
    with pytest.raises(ValueError, match='FastPrecision needs a connected graph'):
        FastPrecision(gc.BY_NAME['components-65'].networkx(), device=DEV)
    with pytest.raises(ValueError, match='FastPrecision needs a connected graph'):
        FastPrecision(gc.BY_NAME['cost-components-65'].networkx(), device=DEV)


def test_python_layer_on_the_device(monkeypatch):
    """graph_distances (hops and costs), compute_graph_pdists and GraphDataset.from_graph on the device against the scipy route"""
    from graphembed.data import GraphDataset
    from graphembed.data import graph as G
    monkeypatch.delenv('MM_GRAPH_APSP', raising=False)
    assert G.gpu_apsp_enabled()
    for name in ('path-129', 'digraph-129', 'cost-digraph-65', 'cost-parallel-129'):
        case = gc.BY_NAME[name]
        d = G.graph_distances(case.networkx(), DEV, weight='weight' if case.weighted else None)
        assert d.is_cuda and d.dtype == torch.int32 and torch.equal(d.cpu(), torch.from_numpy(case.oracle().copy())), name
    case = gc.BY_NAME['gnm-129']
    g = case.networkx()
    pd = G.compute_graph_pdists(g)
    monkeypatch.setenv('MM_GRAPH_APSP', 'scipy')
    pd_ref = G.compute_graph_pdists(g)
    monkeypatch.delenv('MM_GRAPH_APSP', raising=False)
    assert pd.dtype == pd_ref.dtype == np.float64 and np.array_equal(pd, pd_ref)
    idx = torch.randperm(case.n, generator=torch.Generator().manual_seed(3))[:17]
    for dtype in (torch.float32, torch.float64):
        ds = GraphDataset.from_graph(g, DEV, dtype)
        ref = GraphDataset(torch.from_numpy(pd_ref).to(dtype))
        assert ds.condensed.is_cuda and ds.condensed.dtype == dtype and len(ds) == case.n
        assert torch.equal(ds.condensed.cpu(), ref.condensed)
        assert torch.equal(ds[idx].cpu(), ref[idx])
    with pytest.raises(ValueError):
        GraphDataset.from_graph(gc.BY_NAME['components-65'].networkx(), DEV)
