"""The oracle of tests/metrics_cases.py held to everything that already states the metrics on the host — the numpy
restatement (oracle/ref_port.py), the reference's recorded MAPs (tests/golden/metrics.npz), the hand-derived fractions of
tests/test_layer_f1_known_answers.py, numpy's and torch's stable sorts — and the case table held to the constants the kernels
are built around, parsed out of the sources.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import metrics_cases as mc
from conftest import ROOT, load_golden

CSRC = os.path.join(ROOT, 'matrix-manifolds_amd', 'csrc')
SMALL = tuple(c for c in mc.CASES if c[1] <= mc.ALL_TREE_MAX_N)
FINITE = tuple(c for c in SMALL if c[2] not in mc.NAN_REGIMES and c[1] >= 2)


# ----------------------------------------------------------------------------------------------------------------- the order
@pytest.mark.parametrize('case', [c for c in mc.CASES if c[0] == 'regime'], ids=mc.case_id)
def test_stable_order_is_the_stable_sort_of_numpy_and_torch(case):
    for dt in mc.DTYPES:
        d = mc.dense(case, dt)
        if case[2] in mc.NAN_REGIMES:
            assert np.isnan(d).any() and (case[2] != 'nan_scattered' or (np.signbit(d) & np.isnan(d)).any())
        rows = range(0, case[1], 7) if case[1] > 300 else range(case[1])
        for u in rows:
            mine = mc.stable_order(d[u])
            assert mine == np.argsort(d[u], kind='stable').tolist()
            assert mine == torch.sort(torch.from_numpy(d[u].copy()), stable=True).indices.tolist()
            assert mine == mc.orders(case)[u].tolist()          # fp32 and fp64 inputs: one order


def test_stable_order_by_hand():
    nan, mnan = np.float32(np.nan), np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    row = np.array([mnan, 1.0, 0.0, nan, -0.0, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32)
    assert mc.stable_order(row) == [6, 8, 2, 4, 1, 7, 5, 0, 3]
    sub = np.array([3, 2, 2, 1], dtype=np.uint32).view(np.float32)          # subnormals one bit apart do not tie
    assert mc.stable_order(sub) == [3, 1, 2, 0]
    assert mc.ranks(np.array([[0, 2, nan, 1]] * 4, dtype=np.float32), 0).tolist() == [0, 2, 3, 1]


# ---------------------------------------------------------------------------------------------------------- average precision
def _neighbours(case):
    return [set(r) for r in mc.adjacency(case)]


@pytest.mark.parametrize('case', [c for c in FINITE if c[0] != 'degree' and c[2] != 'zeros'], ids=mc.case_id)
def test_ap_oracle_vs_numpy_restatement(case):
    """Every case the restatement can express: it needs every degree > 0 and takes the root to sort first, which a zero
    distance to a node of smaller index breaks (`zeros`)."""
    from oracle import ref_port as rp
    want = rp.mean_average_precision(mc.dense(case, 'f64'), _neighbours(case))
    got = float(mc.exact_sum(mc.ap_oracle(case)['ap']) / case[1])
    assert abs(got - want) <= 1e-13, (got, want)


def test_ap_terms_is_what_ap_oracle_sums():
    for case in (('size', 64, 'mixed'), ('regime', 257, 'nan_scattered'), ('degree', 514, 'mixed')):
        indptr, indices = mc.csr(case)
        terms, edge_ranks = mc.ap_terms(mc.dense(case), indptr, indices)
        orc = mc.ap_oracle(case)
        assert terms == orc['terms'] and np.array_equal(edge_ranks, orc['ranks'])
    assert mc.ap_oracle(('degree', 514, 'mixed'))['deg'][:6].tolist() == [0, 1, 255, 256, 257, 513]
    assert mc.ap_oracle(('degree', 514, 'mixed'))['ap'][0] == 0
    star = mc.ap_oracle(('degree', 514, 'mixed'))                # every other node is a neighbour: k_v = r_v
    assert star['sum'][5] == 513


@pytest.mark.parametrize('tag', [f'er{n}_{p}_{s}' for n, p in ((50, 0.1), (100, 0.05), (100, 0.5), (300, 0.02)) for s in (0, 1)])
def test_ap_oracle_vs_recorded_reference(tag):
    G = load_golden('metrics')
    n = int(G[f'{tag}/n'])
    nb = [[] for _ in range(n)]
    for a, b in np.asarray(G[f'{tag}/edges']).tolist():
        nb[a].append(b), nb[b].append(a)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in nb])])
    indices = np.array([w for r in nb for w in sorted(r)])
    d = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    d[iu] = np.asarray(G[f'{tag}/pdists'], dtype=np.float64)
    d.T[iu] = d[iu]
    terms, _ = mc.ap_terms(d, indptr, indices)
    aps = [sum(t, Fraction(0)) / len(t) for t in terms if t]      # (the reference averages over the nodes it scores)
    assert len(aps) == n
    assert abs(float(sum(aps, Fraction(0)) / n) - float(G[f'{tag}/map'])) <= 1e-12


@pytest.mark.parametrize('case', [c for c in mc.CASES if c[2] in mc.NAN_REGIMES], ids=mc.case_id)
def test_nan_rows_score_between_zero_and_one(case):
    orc = mc.ap_oracle(case)
    assert ((orc['ap'] >= 0) & (orc['ap'] <= 1)).all()
    if case[2] == 'nan_rows':
        d = mc.dense(case)
        for u in (0, 5, case[1] - 1):
            assert np.isnan(np.delete(d[u], u)).all()
            nb = np.array(mc.adjacency(case)[u])                 # all NaN: the rank is the index order
            want = [int((np.arange(case[1]) < v).sum()) + (0 if v < u else -1) + 1 for v in nb]
            e0 = mc.csr(case)[0][u]
            assert orc['ranks'][e0:e0 + len(nb)].tolist() == want
    if case[2] == 'nan_one':                                     # the one NaN neighbour ranks last: behind every number
        indptr, indices = mc.csr(case)
        row = mc.dense(case)[0]
        assert np.isnan(row[indices[indptr[0]]]) and orc['ranks'][indptr[0]] >= case[1] - int(np.isnan(row).sum())


# ------------------------------------------------------------------------------------------------------------------ layer F1
def _close(got, want, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all()
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= tol).all(), np.abs(got[ok] - want[ok]).max()


def _means(case, roots, per_tree):
    m1, m2, cnt, _ = mc.accumulators(case, roots, per_tree)
    with np.errstate(invalid='ignore', divide='ignore'):
        means = m1 / cnt
        return means, m2 / cnt - means * means


@pytest.mark.parametrize('case', FINITE, ids=mc.case_id)
def test_f1_oracle_vs_numpy_restatement(case):
    """Every case the restatement can express: numbers (inf included) as distances.  Its width is max(layer), ours
    num_layers - 1: the same wherever the top layer is occupied."""
    from oracle import ref_port as rp
    d, lay = mc.dense(case, 'f64'), mc.layers(case).astype(np.int64)
    top = int(lay.max())
    assert top == mc.num_layers(case) - 1 or case[1] < 64
    deg = np.diff(mc.csr(case)[0])
    per_tree = case[1] % 2                                       # the restatement is slow: one aggregation per case
    name, lo, hi = mc.filter_cases(case)[0]
    for roots, kw in ((range(case[1]), dict()), (mc.selected_roots(case, lo, hi), dict(degrees=deg, min_degree=lo, max_degree=hi))):
        if case[1] > 258 and kw:
            continue
        want = rp.layer_f1_scores(d, lay, per_tree_average=bool(per_tree), **kw)
        got = _means(case, roots, per_tree)
        assert np.isnan(np.asarray(got[0][top:], dtype=np.float64)).all()
        _close(got[0][:top], want[0])
        _close(got[1][:top], want[1])


def test_f1_oracle_vs_hand_derived_fractions():
    import test_layer_f1_known_answers as ka
    for name, kc in ka.CASES.items():
        g = ka.graph_of(kc)
        n = g.number_of_nodes()
        adj = [sorted(g.neighbors(u)) for u in range(n)]
        lay = mc._hops(adj)
        d = np.zeros((n, n))
        iu = np.triu_indices(n, 1)
        d[iu] = kc['pdists']
        d.T[iu] = d[iu]
        trees = {u: mc.tree_f1(mc.stable_order(d[u]), lay[u], u) for u in range(n)}
        width = int(lay.max())

        def moments(roots, per_tree):
            out = []
            for l in range(1, width + 1):
                vals = [trees[u][l] for u in roots if l in trees[u]]
                vals = [sum(v, Fraction(0)) / len(v) for v in vals] if per_tree else [x for v in vals for x in v]
                out.append(ka.moments(vals))
            return out
        assert moments(range(n), False) == kc['all_nodes']
        assert moments(range(n), True) == kc['per_tree']
        if 'leaves_only' in kc:
            assert moments([u for u in range(n) if len(adj[u]) == 1], False) == kc['leaves_only']


@pytest.mark.parametrize('case', mc.CASES, ids=mc.case_id)
def test_bulk_walk_is_the_fenwick_walk(case):
    """tree_walk (cumulative histograms, what the all-tree sums use) == tree_f1 (the Fenwick definition), ratio by ratio."""
    if case[1] < 2:
        return
    lay = mc.layers(case)
    roots = mc.tree_roots(case) if case[1] > 64 else range(case[1])
    for u in sorted({0, 1, case[1] // 2, case[1] - 2, case[1] - 1} & set(roots)):
        row = mc.orders(case)[u]
        a, num, den = mc.tree_walk(row, lay[u], u)
        want = mc.tree_f1(row, lay[u], u)
        got = {}
        for l, p, q in zip(a.tolist(), num.tolist(), den.tolist()):
            got.setdefault(l, []).append(Fraction(p, q))
        assert got == want
        sums = mc.f1_oracle(case)[u]
        for l, fr in want.items():
            assert sums[l][2] == len(fr)
            assert abs(sums[l][0] - mc.ld(sum(fr, Fraction(0)))) <= 2.0 ** -60 * len(fr)
            assert abs(sums[l][1] - mc.ld(sum((x * x for x in fr), Fraction(0)))) <= 2.0 ** -60 * len(fr)


def test_exact_sum_keeps_what_a_double_drops():
    assert np.finfo(mc.L).eps <= 2.0 ** -63, 'the oracle needs an extended long double'
    xs = np.array([mc.L(1), mc.L(2.0) ** -60, -mc.L(1), mc.L(2.0) ** -62], dtype=mc.L)
    assert mc.exact_sum(xs) == mc.L(2.0) ** -60 + mc.L(2.0) ** -62
    third = mc.ld(Fraction(1, 3))
    assert abs(mc.exact_sum([third] * 3) - 1) <= 2.0 ** -62


# ------------------------------------------------------------------------------------------------------------- the constants
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_case_table_straddles_every_constant_of_the_kernels():
    metrics, sort = _src('metrics.hip'), _src('metrics_sort.hip')
    block = int(re.search(r'constexpr int kApBlock = (\d+);', metrics).group(1))
    caps = sorted(int(c) for c in set(re.findall(r'layer_f1_kernel<(\d+)><<<', metrics)))
    small_cap = int(re.search(r'if \(num_layers <= (\d+)\)\s*layer_f1_kernel<(\d+)>', metrics).group(1))
    refused = int(re.search(r'if \(num_layers > (\d+)\) return MM_ERR_UNSUPPORTED', metrics).group(1))
    sort_limits = {int(x) for x in re.findall(r'n > (\d+)\) return', sort)}
    assert len(caps) == 2 and caps[0] == small_cap and caps[1] == refused and len(sort_limits) == 1
    sort_limit = sort_limits.pop()

    def straddled(values, c):
        return {c - 1, c, c + 1} <= set(values)
    ns = [c[1] for c in mc.CASES]
    degs = mc.ap_oracle(('degree', mc.DEGREE_N, 'mixed'))['deg'].tolist()
    nl = [mc.num_layers(c) for c in mc.CASES]
    assert straddled(ns, block) and straddled(degs, block)   # the strided loops of the AP kernel
    for k in (1, 2):                                        # the chunks of the F1 walk: n - 1 live positions
        assert straddled([n - 1 for n in ns], k * block)
    assert {2 * block, 2 * block + 1} <= set(ns)             # (a third pass of the AP loop: one node, none)
    assert straddled(nl, small_cap)                          # 255 | 256 -> <256>, 257 -> <2048>
    assert refused in nl and mc.REFUSED_NUM_LAYERS == refused + 1 and max(nl) == refused
    assert mc.SORT_REFUSED_N == sort_limit + 1 and max(ns) <= sort_limit
    for c in mc.CASES:                                       # the instantiation a case takes holds its top layer
        assert int(mc.layers(c).max()) <= mc.num_layers(c) - 1


def test_case_table_is_the_stated_one():
    assert len(mc.CASES) == len(set(mc.CASES)) == 11 + 1 + 4 + 8 + 18
    assert {mc.num_layers(c) for c in mc.CASES if c[0] in ('size', 'regime', 'degree')} == {7}
    for c in mc.CASES:
        if c[0] in ('size', 'regime') and c[1] >= 64:
            assert set(np.unique(mc.layers(c))) == set(range(7))
    assert set(np.unique(mc.layers(('shape', 513, 'gaps')))) == {0} | set(mc.GAP_LAYERS)
    own = mc.layers(('shape', 257, 'own'))
    assert all(sorted(own[u].tolist()) == list(range(257)) for u in range(257))
    for c in mc.GRAPH_CASES:                                 # symmetric, connected, hop layers
        adj = mc.adjacency(c)
        assert all(u in adj[w] for u in range(c[1]) for w in adj[u])
        assert np.array_equal(mc.layers(c), mc._hops(adj))
    sub = mc.pdists(('regime', 257, 'subnormal'))
    assert sub.dtype == np.float32 and ((sub > 0) & (sub < np.finfo(np.float32).tiny)).all() and len(np.unique(sub)) == 8
    zeros = mc.pdists(('regime', 257, 'zeros'))
    assert (np.signbit(zeros) & (zeros == 0)).any() and (~np.signbit(zeros) & (zeros == 0)).any()
    for dt in mc.DTYPES:                                     # the NaN carry the stated bits, both signs
        pd = mc.pdists(('regime', 513, 'nan_scattered'), dt)
        bits = pd.view(np.uint32 if dt == 'f32' else np.uint64)[np.isnan(pd)]
        assert set(bits.tolist()) == set(mc.NAN_BITS[dt])
    for c in mc.CASES:                                       # every filter case selects what its name says
        if 2 <= c[1] <= mc.ALL_TREE_MAX_N:
            (_, lo, hi), (_, nlo, nhi), _ = mc.filter_cases(c)
            assert len(mc.selected_roots(c, lo, hi)) >= 1 and mc.selected_roots(c, nlo, nhi) == []
    assert len(mc.selected_roots(('degree', 514, 'mixed'), *mc.filter_cases(('degree', 514, 'mixed'))[0][1:])) == 1
