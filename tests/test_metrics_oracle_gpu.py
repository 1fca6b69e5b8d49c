"""The evaluation kernels — mm_graph_sort_rows, mm_graph_average_precision, mm_graph_layer_f1 (both capacities, both
aggregations) — and the Python routes over them, held per node and per tree to the exact oracle of tests/metrics_cases.py
under its derived rule.  Calls go through the C ABI as a caller makes them; outputs and scratch are pre-filled with NaN / 0x7F
so that an unwritten element shows.  Orders, ranks and counts are compared for equality, sums under
|sum - oracle| <= (N + 8) 2^-52 sum|term|.  Every comparison prints err / bound; the largest per kernel and dtype is printed
when the module ends (profiles/metrics_oracle.md records them)."""
import functools

import numpy as np
import pytest
import torch

import metrics_cases as mc

pytestmark = pytest.mark.gpu

TORCH_DT = {'f32': torch.float32, 'f64': torch.float64}
MM_ERR_UNSUPPORTED = -2
FILL32 = 0x7F7F7F7F
SMALL = tuple(c for c in mc.CASES if c[1] <= mc.ALL_TREE_MAX_N)
cases = pytest.mark.parametrize('case', mc.CASES, ids=mc.case_id)
small_cases = pytest.mark.parametrize('case', SMALL, ids=mc.case_id)
dtypes = pytest.mark.parametrize('dt', mc.DTYPES)


@pytest.fixture(scope='module', autouse=True)
def ratios():
    yield
    for (kernel, dt), worst in sorted(mc.RATIOS.items()):
        print(f'\nORACLE-RATIO {kernel} {dt} {worst:.3g}', end='')
    print()


def B():
    from graphembed import _backend
    return _backend


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def dense_dev(case, dt):
    d = dev(mc.dense(case, dt))
    assert d.dtype == TORCH_DT[dt]
    return d


def sort_rows(d):
    b, n = B(), d.shape[0]
    nbytes = b.lib().raw('mm_graph_sort_rows_ws_bytes')(b.dtype_code(d), n)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x7F, dtype=torch.uint8, device='cuda')
    order = torch.full((n, n), FILL32, dtype=torch.int32, device='cuda')
    b.lib().call('mm_graph_sort_rows', b.dtype_code(d), b.ptr(d), n, b.ptr(order), b.ptr(ws), nbytes, b.stream_of(d))
    return order


@functools.lru_cache(maxsize=None)
def gpu_order(case, dt):
    """The library's own sort of the case, checked once against the oracle wherever the oracle holds the row."""
    d = dense_dev(case, dt)
    before = d.clone()
    order = sort_rows(d)
    assert torch.equal(d.view(torch.uint8), before.view(torch.uint8)), 'the sort wrote into its input'
    want = mc.orders(case)
    rows = sorted(want)
    got = order[torch.tensor(rows, device='cuda')].cpu().numpy()
    for k, u in enumerate(rows):
        assert np.array_equal(got[k], want[u]), (case, dt, u, np.flatnonzero(got[k] != want[u])[:8])
    return order


# ------------------------------------------------------------------------------------------------------------------- the sort
@cases
@dtypes
def test_sort_rows_is_the_stable_order(case, dt):
    order = gpu_order(case, dt)
    n = case[1]                                          # every row is a permutation (the rows the oracle does not hold too)
    assert torch.equal(torch.sort(order, dim=1).values, torch.arange(n, dtype=torch.int32, device='cuda').expand(n, n))


def test_sort_rows_refuses_one_node_past_its_range():
    b = B()
    n = mc.SORT_REFUSED_N
    dummy = torch.zeros(64, dtype=torch.float64, device='cuda')
    for code in (0, 1):
        assert b.lib().raw('mm_graph_sort_rows_ws_bytes')(code, n) == 0
        assert b.lib().raw('mm_graph_sort_rows_ws_bytes')(code, n - 1) > 0
        rc = b.lib().raw('mm_graph_sort_rows')(code, b.ptr(dummy), n, b.ptr(dummy), b.ptr(dummy), 1 << 40, b.stream_of(dummy))
        assert rc == MM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(dummy.any())


# ---------------------------------------------------------------------------------------------------------- average precision
def abi_average_precision(d, indptr, indices):
    """-> (ap [n], rank scratch [nnz], the guard element behind it)."""
    b, n = B(), d.shape[0]
    ap = torch.full((n,), float('nan'), dtype=d.dtype, device='cuda')
    scratch = torch.full((indices.numel() + 1,), FILL32, dtype=torch.int32, device='cuda')
    b.lib().call('mm_graph_average_precision', b.dtype_code(d), b.ptr(d), n, b.ptr(indptr), b.ptr(indices), b.ptr(scratch),
                 b.ptr(ap), b.stream_of(d))
    return ap, scratch[:-1], int(scratch[-1])


def ap_bound(orc, dt):
    bnd = mc.bound(orc['deg'], orc['sum'])
    return bnd + (mc.L(2.0) ** -24 * orc['sum'] if dt == 'f32' else 0)


@small_cases
@dtypes
def test_average_precision_per_node(case, dt):
    indptr, indices = (dev(a) for a in mc.csr(case))
    ap, rank, guard = abi_average_precision(dense_dev(case, dt), indptr, indices)
    orc = mc.ap_oracle(case)
    assert guard == FILL32
    assert np.array_equal(rank.cpu().numpy(), orc['ranks'])
    got = ap.cpu().numpy().astype(mc.L)
    assert (got[orc['deg'] == 0] == 0).all()             # exactly 0, and written
    mc.hold('average_precision', dt, got * orc['deg'].astype(mc.L), orc['sum'], ap_bound(orc, dt), mc.case_id(case))
    if case[2] in mc.NAN_REGIMES:
        assert ((got >= 0) & (got <= 1)).all()


# ------------------------------------------------------------------------------------------------------------------ layer F1
def layer_f1(order, hops, indptr, lo, hi, per_tree, nl, acc):
    b = B()
    b.lib().call('mm_graph_layer_f1', b.ptr(order), b.ptr(hops), order.shape[0], b.ptr(indptr), lo, hi, per_tree, nl,
                 b.ptr(acc[0]), b.ptr(acc[1]), b.ptr(acc[2]), b.stream_of(order))


def new_acc(shape_front, width):
    """Zeroed accumulators [.., 3, width] with a NaN guard column behind each."""
    acc = torch.zeros(*shape_front, 3, width + 1, dtype=torch.float64, device='cuda')
    acc[..., width] = float('nan')
    return acc


def check_acc(kernel, dt, acc, want, what):
    m1, m2, cnt, nterms = want
    width = len(m1)
    got = acc.cpu().numpy()
    assert np.isnan(got[:, width]).all(), 'wrote behind num_layers - 1'
    assert np.array_equal(got[2, :width], cnt.astype(np.float64)), (what, got[2, :width], cnt)
    mc.hold(kernel, dt, got[0, :width], m1, mc.bound(nterms, m1), what + ' sum f1')
    mc.hold(kernel, dt, got[1, :width], m2, mc.bound(nterms, m2), what + ' sum f1^2')


def kernel_name(case):
    return 'layer_f1<256>' if mc.num_layers(case) <= 256 else 'layer_f1<2048>'


@cases
@dtypes
@pytest.mark.parametrize('per_tree', (0, 1))
def test_layer_f1_one_tree_at_a_time(case, dt, per_tree):
    """The kernel uses indptr only for the root's degree: with exactly one root of degree 1 and min_degree = max_degree = 1
    the accumulators are that one tree's."""
    n, nl = case[1], mc.num_layers(case)
    order, hops = gpu_order(case, dt), dev(mc.layers(case))
    roots = mc.tree_roots(case)
    acc = new_acc((len(roots),), nl - 1) if nl > 1 else None
    for k, u in enumerate(roots):
        indptr = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
        indptr[u + 1:] = 1
        layer_f1(order, hops, indptr, 1, 1, per_tree, nl, acc[k])
    for k, u in enumerate(roots):
        check_acc(kernel_name(case), dt, acc[k], mc.accumulators(case, [u], per_tree), f'{mc.case_id(case)} tree {u}')


@small_cases
@dtypes
def test_layer_f1_all_trees(case, dt):
    """The real degrees: the defaults, a filter that binds exactly on one degree, a filter that excludes every root."""
    nl = mc.num_layers(case)
    order, hops, indptr = gpu_order(case, dt), dev(mc.layers(case)), dev(mc.csr(case)[0])
    for name, lo, hi in mc.filter_cases(case) + (('all', 0, 2 ** 31 - 1),):
        roots = mc.selected_roots(case, lo, hi)
        assert (name != 'none' or not roots) and (name != 'all' or len(roots) == case[1])
        for per_tree in (0, 1):
            acc = new_acc((), nl - 1)
            layer_f1(order, hops, indptr, lo, hi, per_tree, nl, acc)
            check_acc(kernel_name(case), dt, acc, mc.accumulators(case, roots, per_tree),
                      f'{mc.case_id(case)} {name} per_tree={per_tree}')


def test_layer_f1_refuses_one_layer_past_its_capacity():
    b = B()
    nl, n = mc.REFUSED_NUM_LAYERS, 4
    order = torch.arange(n, dtype=torch.int32, device='cuda').repeat(n, 1).contiguous()
    hops = torch.ones(n, n, dtype=torch.int32, device='cuda')
    indptr = torch.arange(n + 1, dtype=torch.int32, device='cuda')
    acc = torch.full((3, nl - 1), float('nan'), dtype=torch.float64, device='cuda')
    rc = b.lib().raw('mm_graph_layer_f1')(b.ptr(order), b.ptr(hops), n, b.ptr(indptr), 0, 2 ** 31 - 1, 0, nl, b.ptr(acc[0]),
                                          b.ptr(acc[1]), b.ptr(acc[2]), b.stream_of(order))
    assert rc == MM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(acc).all())
    acc.zero_()                                           # the last supported count runs
    layer_f1(order, hops, indptr, 0, 2 ** 31 - 1, 0, nl - 1, acc)
    torch.cuda.synchronize()
    assert acc[2].sum().item() == n * (n - 1)


# ------------------------------------------------------------------------------------------------------------- Python routes
@functools.lru_cache(maxsize=None)
def evaluator(case):
    import networkx as nx
    from graphembed.pyx import FastPrecision
    g = nx.Graph()
    g.add_nodes_from(range(case[1]))
    g.add_edges_from(mc.edges(case))
    fp = FastPrecision(g)
    assert fp.num_layers == mc.num_layers(case) and np.array_equal(fp.hops.cpu().numpy(), mc.layers(case))
    assert np.array_equal(fp.indptr.cpu().numpy(), mc.csr(case)[0]) and np.array_equal(fp.indices.cpu().numpy(), mc.csr(case)[1])
    return g, fp


graph_cases = pytest.mark.parametrize('case', mc.GRAPH_CASES, ids=mc.case_id)


@graph_cases
@dtypes
def test_python_map_routes(case, dt):
    from graphembed.metrics import mean_average_precision, node_average_precision
    g, fp = evaluator(case)
    pd = torch.from_numpy(mc.pdists(case, dt).copy())
    orc = mc.ap_oracle(case)
    n = case[1]
    want = mc.exact_sum(orc['ap']) / n
    bnd = (int(orc['deg'].max()) + 8 + n + 8) * mc.L(mc.U52) * want + (mc.L(2.0) ** -24 * want if dt == 'f32' else 0)
    mc.hold('FastPrecision.mean_average_precision', dt, fp.mean_average_precision(pd), want, bnd, mc.case_id(case))
    mc.hold('metrics.mean_average_precision', dt, mean_average_precision(pd.cuda(), g), want, bnd, mc.case_id(case))
    mc.hold('metrics.mean_average_precision', dt, mean_average_precision(dev(mc.dense(case, dt)), g), want, bnd,
            mc.case_id(case) + ' dense')
    ap, _, _ = abi_average_precision(dense_dev(case, dt), fp.indptr, fp.indices)
    node = node_average_precision(pd.cuda(), fp.indptr, fp.indices)
    assert node.dtype == ap.dtype and torch.equal(node.view(torch.uint8), ap.view(torch.uint8))


def check_scores(dt, got, want, what):
    means, var = got
    m1, m2, cnt, nterms = want
    assert len(means) == len(var) == len(m1)
    empty = cnt == 0
    assert np.array_equal(np.isnan(means), empty) and np.array_equal(np.isnan(var), empty), what
    ok = ~empty
    wmean = m1[ok] / cnt[ok]
    mc.hold('FastPrecision.layer_f1 means', dt, means[ok], wmean, mc.bound(nterms[ok], wmean), what)
    mc.hold('FastPrecision.layer_f1 variance', dt, var[ok], m2[ok] / cnt[ok] - wmean * wmean,
            4 * (nterms[ok] + 8) * mc.L(mc.U52), what)


@graph_cases
@dtypes
def test_python_layer_f1_routes(case, dt):
    g, fp = evaluator(case)
    pd = torch.from_numpy(mc.pdists(case, dt).copy())
    n = case[1]
    for name, lo, hi in mc.filter_cases(case):
        kw = {} if name == 'default' else dict(min_degree=lo, max_degree=hi)
        check_scores(dt, fp.layer_mean_f1_scores(pd, **kw), mc.accumulators(case, mc.selected_roots(case, lo, hi), 0),
                     f'{mc.case_id(case)} {name}')
    check_scores(dt, fp.layer_mean_average_f1_scores(pd), mc.accumulators(case, range(n), 1), f'{mc.case_id(case)} per tree')


@pytest.mark.parametrize('case', [c for c in mc.GRAPH_CASES if c[2] == 'bfs'], ids=mc.case_id)
@dtypes
def test_python_two_distance_sets(case, dt):
    """num_pdists_sets = 2: the second set is the `distinct` regime of the same size, on the same trees."""
    g, fp = evaluator(case)
    n = case[1]
    other = ('regime', n, 'distinct')
    pd = torch.from_numpy(np.concatenate([mc.pdists(case, dt), mc.pdists(other, dt)]))
    for per_tree in (0, 1):
        a, b = (mc.accumulators(case, range(n), per_tree, dist_case=dc) for dc in (None, other))
        want = tuple(x + y for x, y in zip(a, b))
        got = fp.layer_mean_average_f1_scores(pd, 2) if per_tree else fp.layer_mean_f1_scores(pd, 2, 0, 2 ** 31 - 1)
        check_scores(dt, got, want, f'{mc.case_id(case)} two sets per_tree={per_tree}')
