"""Cases, inputs, exact oracle and tolerance rule of the evaluation kernels (csrc/metrics.hip: average_precision_kernel,
layer_f1_kernel<256 / 2048>; csrc/metrics_sort.hip: the segmented row sort), shared by tests/test_metrics_cases_host.py
and tests/test_metrics_oracle_gpu.py.  Host code only (numpy, integers, fractions): nothing here runs a kernel.

THE ORDER.  One total order on (distance, node): numbers ascending with -0.0 == +0.0, then every NaN of either sign and
any payload, ties by node index.  `stable_order(row)` lists the nodes of a row in that order; it is what
numpy.argsort(kind='stable') and torch.sort(stable=True) give, and it is the contract of mm_graph_average_precision and
mm_graph_sort_rows (include/mm_manifolds.h).

THE ORACLE.  Integers and exact ratios.
  ranks(dense, u)                  position (1 = closest) of every node in stable_order(dense[u]) with u removed
  ap_terms(dense, indptr, indices) per node the list of Fraction(k_v, r_v): r_v = rank of neighbour v, k_v = neighbours of
                                   rank <= r_v;  AP(u) = sum / deg(u)
  tree_f1(order_row, layer_row, u) per layer the list of f1 = 2 nb / (i + R) of the tree rooted at u:  i = position of v,
                                   nb = 1 + #{earlier, layer <= layer(v)},  R = #{layers 1 .. layer(v)-1} + #{earlier on
                                   layer(v)} + 1  (= 2 p r / (p + r) with p = nb / i, r = nb / R); a Fenwick tree over layers
Sums: every exact ratio is divided once in numpy.longdouble and the quotients are added with math.fsum (each quotient
split into two doubles, so nothing is lost in the conversion; `exact_sum`).

THE TOLERANCE RULE (derived, not measured).  The kernels form each term in a handful of correctly rounded fp64 operations
(f1: two quotients, two products, a sum, a quotient -> at most 7 roundings of 2^-53; its square: 15) and add N of them in an
unspecified order (N - 1 roundings), so
    |sum - oracle| <= (N + 8) 2^-52 sum|term|
for  deg AP(u) with N = deg;  a tree's per-layer sum f1 and sum f1^2 with N = the layer's count;  the all-tree accumulators
with N = the total number of f1 terms that entered the layer (for the per-tree aggregation a tree's mean carries
(n_t + 7) 2^-53, its square (2 n_t + 15) 2^-53, adding T of them T - 1 more: below (N + 8) 2^-52 as N >= n_t + T - 1).
fp32 AP adds the one rounding of the result: + 2^-24 AP.  Python routes: a layer mean is the accumulator over an exact
count (one more rounding, inside the 8); the variance is a difference of two numbers <= 1, its bound is absolute,
4 (N + 8) 2^-52; MAP is the fp64 mean of n node scores: (max deg + 8 + n + 8) 2^-52 MAP (+ 2^-24 MAP in fp32).
Counts, ranks and sort orders are compared for equality.

THE CASE TABLE (a stated list; every case in fp32 and fp64, the same numbers: inputs are fp32-representable).
  ('size', n, 'mixed')     n in SIZES = 1, 2, 3, 64, 255, 256, 257, 258, 512, 513, 514: the 256-thread strided loops of the AP
                           kernel and the 256-position chunk of the F1 walk (n - 1 around 256 and 512); layers random in 1..6
  ('degree', 514, 'mixed') hand-built CSR with degrees 0, 1, 255, 256, 257, n - 1 (nodes 0..5) and 1..7 elsewhere
  ('path', n, 'distinct')  path graphs with the real hop matrix, n = 255, 256, 257 (num_layers = n: capacity 256 | 2048) and
                           2048 (the last supported; per tree only, roots 0, 1023, 2047); num_layers = 2049 is refused
  ('shape', n, s)          n in 257, 513; s = bfs (hop layers of a connected Erdos-Renyi graph), gaps (layers from {1, 4, 9, 200}),
                           one (every node on layer 1), own (every node on its own layer)
  ('regime', n, r)         n in 257, 513; r = distinct, four, equal, inf, zeros (-0.0 / +0.0 / 0.5), subnormal (fp32 subnormals
                           one bit apart), nan_scattered (NaN of both signs, explicit bit patterns), nan_one (one neighbour NaN),
                           nan_rows (whole rows NaN)
Inputs come from seeds crc32(repr(case))."""
import functools
import math
import zlib
from fractions import Fraction

import numpy as np

L = np.longdouble
U52 = 2.0 ** -52
SIZES = (1, 2, 3, 64, 255, 256, 257, 258, 512, 513, 514)
DEGREE_N = 514
PATH_NS = (255, 256, 257, 2048)
REFUSED_NUM_LAYERS = 2049
SORT_REFUSED_N = 46341
SHAPES = ('bfs', 'gaps', 'one', 'own')
REGIMES = ('distinct', 'four', 'equal', 'inf', 'zeros', 'subnormal', 'nan_scattered', 'nan_one', 'nan_rows')
NAN_REGIMES = ('nan_scattered', 'nan_one', 'nan_rows')
GAP_LAYERS = (1, 4, 9, 200)
NAN_BITS = {'f32': (0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFF800001, 0x7FA00000),
            'f64': (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF0000000000001, 0x7FF4000000000000)}
NP_DT = {'f32': np.float32, 'f64': np.float64}
DTYPES = ('f32', 'f64')

CASES = (tuple(('size', n, 'mixed') for n in SIZES) + (('degree', DEGREE_N, 'mixed'),)
         + tuple(('path', n, 'distinct') for n in PATH_NS)
         + tuple(('shape', n, s) for n in (257, 513) for s in SHAPES)
         + tuple(('regime', n, r) for n in (257, 513) for r in REGIMES))
ALL_TREE_MAX_N = 514                                  # the all-tree comparison stops here; path 2048 is held per tree
GRAPH_CASES = tuple(c for c in CASES if (c[0] == 'path' and c[1] <= 257) or c[2] == 'bfs')   # real graphs: the Python routes

RATIOS = {}   # (kernel, dtype) -> largest err / bound seen


def case_id(case):
    return '-'.join(str(x) for x in case)


def rng_of(case, what=''):
    return np.random.RandomState(zlib.crc32(repr((case, what)).encode()) % (2 ** 32))


# ------------------------------------------------------------------------------------------------------------------ graphs
def _bfs_graph(case):
    """Adjacency sets of a connected Erdos-Renyi graph (p = 3 / n; components are joined by one edge each)."""
    n = case[1]
    rng = rng_of(case, 'graph')
    adj = [set() for _ in range(n)]
    iu = np.triu_indices(n, 1)
    pick = rng.rand(len(iu[0])) < 3.0 / n
    for a, b in zip(iu[0][pick].tolist(), iu[1][pick].tolist()):
        adj[a].add(b), adj[b].add(a)
    seen = _reach(adj, 0)
    for v in range(n):
        if v not in seen:                  # hang the component of v on the reached part
            a = sorted(seen)[int(rng.randint(len(seen)))]
            adj[a].add(v), adj[v].add(a)
            seen |= _reach(adj, v)
    return adj


def _reach(adj, s):
    seen, todo = {s}, [s]
    while todo:
        for w in adj[todo.pop()]:
            if w not in seen:
                seen.add(w), todo.append(w)
    return seen


@functools.lru_cache(maxsize=None)
def adjacency(case):
    """Neighbour lists (sorted) of the case's graph.  Only the `degree` case is not symmetric (the kernels read rows)."""
    kind, n, var = case
    if kind == 'path':
        return tuple(tuple(w for w in (u - 1, u + 1) if 0 <= w < n) for u in range(n))
    if var == 'bfs':
        return tuple(tuple(sorted(s)) for s in _bfs_graph(case))
    rng = rng_of(case, 'graph')
    if kind == 'degree':
        degs = [0, 1, 255, 256, 257, n - 1] + [u % 7 + 1 for u in range(6, n)]
        out = []
        for u, d in enumerate(degs):
            others = np.array([w for w in range(n) if w != u])
            out.append(tuple(sorted(rng.permutation(others)[:d].tolist())))
        return tuple(out)
    adj = [set() for _ in range(n)]                      # a ring plus about two random chords per node
    for u in range(n):
        for w in ((u + 1) % n,) + tuple(rng.randint(0, n, size=2).tolist() if n > 3 else ()):
            if w != u:
                adj[u].add(w), adj[w].add(u)
    return tuple(tuple(sorted(s)) for s in adj)


def edges(case):
    return [(u, w) for u, nb in enumerate(adjacency(case)) for w in nb if u < w]


@functools.lru_cache(maxsize=None)
def csr(case):
    nb = adjacency(case)
    indptr = np.zeros(len(nb) + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(r) for r in nb])
    return indptr, np.array([w for r in nb for w in r], dtype=np.int32)


def _hops(adj):
    n = len(adj)
    out = np.zeros((n, n), dtype=np.int32)
    for s in range(n):
        dist, front, d = {s: 0}, [s], 0
        while front:
            d += 1
            nxt = []
            for v in front:
                for w in adj[v]:
                    if w not in dist:
                        dist[w] = d
                        nxt.append(w)
            front = nxt
        assert len(dist) == n
        out[s, list(dist)] = list(dist.values())
    return out


@functools.lru_cache(maxsize=None)
def layers(case):
    """int32 [n, n]: the layer of v in the tree rooted at u (0 for u itself only)."""
    kind, n, var = case
    if kind == 'path':
        i = np.arange(n, dtype=np.int32)
        lay = np.abs(i[:, None] - i[None, :])
    elif var == 'bfs':
        lay = _hops(adjacency(case))
    else:
        rng = rng_of(case, 'layers')
        if var == 'gaps':
            lay = np.array(GAP_LAYERS, dtype=np.int32)[rng.randint(0, 4, size=(n, n))]
        elif var == 'one':
            lay = np.ones((n, n), dtype=np.int32)
        elif var == 'own':
            lay = np.zeros((n, n), dtype=np.int32)
            for u in range(n):
                lay[u, np.arange(n) != u] = rng.permutation(n - 1) + 1
        else:
            lay = rng.randint(1, 7, size=(n, n)).astype(np.int32)
        lay[np.arange(n), np.arange(n)] = 0
    lay = np.ascontiguousarray(lay, dtype=np.int32)
    lay.setflags(write=False)
    return lay


def num_layers(case):
    kind, n, var = case
    if kind == 'path':
        return n
    if var == 'bfs':
        return int(layers(case).max()) + 1
    return {'gaps': GAP_LAYERS[-1] + 1, 'one': 2, 'own': n}.get(var, 7)


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def pdists(case, dtype='f32'):
    """The condensed distance vector of a case (pair order (0,1), (0,2), ..), in fp32-representable numbers; the NaN of
    `nan_scattered` carry the explicit bit patterns NAN_BITS[dtype]."""
    kind, n, var = case
    m = n * (n - 1) // 2
    rng = rng_of(case, 'pdists')
    iu = np.triu_indices(n, 1)
    if var == 'distinct':
        pd = ((rng.permutation(m) + 1) * 2.0 ** -12).astype(np.float32)
    elif var == 'four':
        pd = (0.5 * (1 + rng.randint(0, 4, size=m))).astype(np.float32)
    elif var == 'equal':
        pd = np.full(m, 1.25, dtype=np.float32)
    elif var == 'zeros':
        pd = np.array([-0.0, 0.0, 0.5], dtype=np.float32)[rng.randint(0, 3, size=m)]
    elif var == 'subnormal':
        pd = rng.randint(1, 9, size=m).astype(np.uint32).view(np.float32)
    else:    # mixed: about n / 2 values, so every row has ties and distinct values
        pd = (np.floor(rng.rand(m) * max(n // 2, 2)) / 8.0 + 0.125).astype(np.float32)
    if var == 'inf':
        pd[rng.rand(m) < 0.1] = np.inf
    nan = np.zeros(m, dtype=bool)
    if var == 'nan_scattered':
        nan = rng.rand(m) < 0.1
    elif var == 'nan_one':       # the first neighbour of every third node
        nb = adjacency(case)
        for u in range(0, n, 3):
            a, b = min(u, nb[u][0]), max(u, nb[u][0])
            nan[a * n - a * (a + 1) // 2 + b - a - 1] = True
    elif var == 'nan_rows':
        rows = (0, 5, n - 1)
        nan = np.isin(iu[0], rows) | np.isin(iu[1], rows)
    out = pd.astype(NP_DT[dtype])
    if nan.any():
        bits = np.array(NAN_BITS[dtype], dtype=np.uint32 if dtype == 'f32' else np.uint64)
        out.view(bits.dtype)[nan] = bits[np.arange(int(nan.sum())) % len(bits)]
        assert np.isnan(out[nan]).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def dense(case, dtype='f32'):
    """The symmetric zero-diagonal [n, n] matrix of pdists(case, dtype), bit patterns kept."""
    n = case[1]
    pd = pdists(case, dtype)
    out = np.zeros((n, n), dtype=pd.dtype)
    iu = np.triu_indices(n, 1)
    out[iu] = pd
    out.T[iu] = pd
    out.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------------------------- the order
def stable_order(row):
    """The nodes of a row in the total order: numbers ascending (-0.0 == +0.0), then every NaN, ties by index."""
    vals = np.asarray(row).tolist()
    keys = [(True, 0.0) if v != v else (False, v) for v in vals]
    return sorted(range(len(vals)), key=keys.__getitem__)       # (sorted is stable: equal keys stay in index order)


def tree_roots(case):
    """Roots whose trees are held one at a time: every root up to 258 nodes, five beyond, three on the 2048-node path."""
    n = case[1]
    if n == 2048:
        return (0, 1023, 2047)
    return tuple(range(n)) if n <= 258 else tuple(sorted({0, 1, n // 2, n - 2, n - 1}))


@functools.lru_cache(maxsize=None)
def orders(case):
    """{u: stable_order of row u} — every row up to ALL_TREE_MAX_N nodes, the tree_roots beyond."""
    n = case[1]
    d = dense(case)
    rows = range(n) if n <= ALL_TREE_MAX_N else tree_roots(case)
    return {u: np.array(stable_order(d[u]), dtype=np.int32) for u in rows}


def order_matrix(case):
    o = orders(case)
    return np.stack([o[u] for u in range(case[1])])


# ------------------------------------------------------------------------------------------------------------ average precision
def ranks(dense_, u):
    """rank[v] = position (1 = closest) of v in stable_order(dense_[u]) with u removed; rank[u] = 0."""
    out = np.zeros(len(dense_), dtype=np.int64)
    pos = 0
    for v in stable_order(dense_[u]):
        if v != u:
            pos += 1
            out[v] = pos
    return out


def ap_terms(dense_, indptr, indices):
    """Per node the list of Fraction(k_v, r_v) over its neighbours in CSR order, and the ranks r_v per CSR entry."""
    terms, edge_ranks = [], np.zeros(len(indices), dtype=np.int64)
    for u in range(len(indptr) - 1):
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        if e0 == e1:
            terms.append([])
            continue
        r = ranks(dense_, u)[indices[e0:e1]]
        edge_ranks[e0:e1] = r
        k = {rv: i + 1 for i, rv in enumerate(sorted(r.tolist()))}
        terms.append([Fraction(k[rv], rv) for rv in r.tolist()])
    return terms, edge_ranks


def exact_sum(xs):
    """Sum of longdouble values through math.fsum: every value goes in as two doubles (head and tail), the sum comes back as
    two (fsum, and fsum of what it left)."""
    xs = np.asarray(xs, dtype=L).reshape(-1)
    if len(xs) == 0:
        return L(0)
    if len(xs) == 1:
        return xs[0]
    hi = xs.astype(np.float64)
    parts = hi.tolist() + (xs - hi).astype(np.float64).tolist()
    s = math.fsum(parts)
    return L(s) + L(math.fsum(parts + [-s]))


def ld(fr):
    """An exact ratio divided once in longdouble."""
    return L(fr.numerator) / L(fr.denominator)


@functools.lru_cache(maxsize=None)
def ap_oracle(case):
    """{'ranks': int64 [nnz], 'sum': longdouble [n] = deg AP(u), 'ap': longdouble [n], 'deg': int [n]}."""
    indptr, indices = csr(case)
    n = case[1]
    terms, edge_ranks = [], np.zeros(len(indices), dtype=np.int64)
    o = orders(case)
    for u in range(n):     # ap_terms with the case's cached orders
        e0, e1 = int(indptr[u]), int(indptr[u + 1])
        rank = np.zeros(n, dtype=np.int64)
        seq = o[u][o[u] != u]
        rank[seq] = np.arange(1, n)
        r = rank[indices[e0:e1]]
        edge_ranks[e0:e1] = r
        k = {rv: i + 1 for i, rv in enumerate(sorted(r.tolist()))}
        terms.append([Fraction(k[rv], rv) for rv in r.tolist()])
    sums = np.array([exact_sum([ld(t) for t in ts]) for ts in terms], dtype=L)
    deg = np.diff(indptr).astype(np.int64)
    ap = np.where(deg > 0, sums / np.maximum(deg, 1).astype(L), L(0))
    return {'ranks': edge_ranks, 'sum': sums, 'ap': ap, 'deg': deg, 'terms': terms}


# ------------------------------------------------------------------------------------------------------------------ layer F1
def tree_f1(order_row, layer_row, u):
    """{layer: [Fraction f1, ..]} of the tree rooted at u: order_row = the nodes by embedding distance (u anywhere in it),
    layer_row[v] = the layer of v.  O(n log n): a Fenwick tree over the layers counts the earlier nodes on layers <= l."""
    layer_row = [int(x) for x in layer_row]
    top = max(layer_row) + 1
    fen = [0] * (top + 1)
    hist = [0] * (top + 1)
    for v, l in enumerate(layer_row):
        if v != u:
            hist[l] += 1
    strict_before, run = [0] * (top + 1), 0     # nodes on layers 1 .. l-1
    for l in range(1, top + 1):
        strict_before[l] = run
        run += hist[l]
    on_layer = [0] * (top + 1)
    out, i = {}, 0
    for v in order_row:
        v = int(v)
        if v == u:
            continue
        i += 1
        l = layer_row[v]
        q, nb = l + 1, 1
        while q > 0:
            nb += fen[q]
            q -= q & -q
        r = strict_before[l] + on_layer[l] + 1
        out.setdefault(l, []).append(Fraction(2 * nb, i + r))
        on_layer[l] += 1
        q = l + 1
        while q <= top:
            fen[q] += 1
            q += q & -q
    return out


def tree_walk(order_row, layer_row, u):
    """(layer, numerator, denominator) int64 arrays of the same ratios in walk order, counted with cumulative per-layer
    histograms (O(n L), vectorised): the bulk route of the all-tree sums; the host tests hold it to tree_f1."""
    order_row = np.asarray(order_row)
    seq = order_row[order_row != u]
    a = np.asarray(layer_row)[seq].astype(np.int64)
    m, top = len(a), int(a.max()) + 1 if len(a) else 1
    idx = np.arange(m)
    seen = np.zeros((m + 1, top), dtype=np.int64)
    seen[idx + 1, a] = 1
    seen = np.cumsum(seen, axis=0)                  # seen[i, l] = nodes among the first i on layer l
    nb = 1 + np.cumsum(seen[:m], axis=1)[idx, a]
    hist = seen[m].copy()
    hist[0] = 0
    strict_before = np.concatenate([[0], np.cumsum(hist)[:-1]])
    r = strict_before[a] + seen[idx, a] + 1
    return a, 2 * nb, idx + 1 + r


def layer_sums(lay, num, den):
    """{layer: (sum f1, sum f1^2, count)} in longdouble, each ratio divided once."""
    f1 = num.astype(L) / den.astype(L)
    f2 = (num * num).astype(L) / (den * den).astype(L)
    out = {}
    srt = np.argsort(lay, kind='stable')
    cuts = np.flatnonzero(np.diff(lay[srt])) + 1
    for grp in np.split(srt, cuts):
        if len(grp):
            out[int(lay[grp[0]])] = (exact_sum(f1[grp]), exact_sum(f2[grp]), len(grp))
    return out


@functools.lru_cache(maxsize=None)
def f1_oracle(case, dist_case=None):
    """{u: {layer: (sum f1, sum f1^2, count)}} for every tree the case holds (all up to ALL_TREE_MAX_N nodes); `dist_case`
    lends the distances of another case of the same size (a second distance set on the same trees)."""
    lay = layers(case)
    return {u: layer_sums(*tree_walk(row, lay[u], u)) for u, row in orders(dist_case or case).items()}


def accumulators(case, roots, per_tree, dist_case=None):
    """The accumulators over the trees `roots`: m1, m2, counts (longdouble) and the number of f1 terms N per layer.  The
    terms are positive, so the sum of |term| that the bound scales with is m1 (m2) itself."""
    width = num_layers(case) - 1
    tab = f1_oracle(case, dist_case)
    per_layer = [[] for _ in range(width)]
    for u in roots:
        for l, s in tab[u].items():
            per_layer[l - 1].append(s)
    m1, m2, cnt = np.zeros(width, dtype=L), np.zeros(width, dtype=L), np.zeros(width, dtype=L)
    nterms = np.zeros(width, dtype=np.int64)
    for k, items in enumerate(per_layer):
        if not items:
            continue
        nterms[k] = sum(c for _, _, c in items)
        if per_tree:
            means = np.array([s1 / L(c) for s1, _, c in items], dtype=L)
            m1[k], m2[k], cnt[k] = exact_sum(means), exact_sum(means * means), len(items)
        else:
            m1[k], m2[k], cnt[k] = exact_sum([s1 for s1, _, _ in items]), exact_sum([s2 for _, s2, _ in items]), nterms[k]
    return m1, m2, cnt, nterms


def selected_roots(case, min_degree, max_degree):
    deg = np.diff(csr(case)[0])
    return [u for u in range(case[1]) if min_degree <= deg[u] <= max_degree]


def filter_cases(case):
    """(name, min_degree, max_degree): a filter that binds exactly on one root's degree, one that excludes every root, the
    defaults of FastPrecision.layer_mean_f1_scores."""
    deg = np.diff(csr(case)[0])
    vals, counts = np.unique(deg, return_counts=True)
    d = int(vals[len(vals) - 1 - np.argmin(counts[::-1])])            # the rarest degree (the largest of them)
    return (('exact', d, d), ('none', int(deg.max()) + 1, int(deg.max()) + 1), ('default', 1, 99999))


# ------------------------------------------------------------------------------------------------------------- the rule
def bound(nterms, abs_sum):
    return (np.asarray(nterms, dtype=L) + 8) * L(U52) * np.abs(np.asarray(abs_sum, dtype=L))


def hold(kernel, dtype, got, want, bnd, what):
    """Assert |got - want| <= bnd elementwise (NaN anywhere fails), print err / bound and keep the largest per kernel."""
    got, want, bnd = (np.atleast_1d(np.asarray(x, dtype=L)) for x in (got, want, bnd))
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, L(0), err / bnd)
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if len(ratio) else 0.0
    RATIOS[(kernel, dtype)] = max(RATIOS.get((kernel, dtype), 0.0), worst)
    print(f'{kernel} {dtype} {what}: err / bound = {worst:.3g}')
    assert worst <= 1.0, f'{kernel} {dtype} {what}: err / bound = {worst:.3g} at {int(np.argmax(ratio))}'
