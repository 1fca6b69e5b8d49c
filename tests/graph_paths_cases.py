"""Case table and oracle of the all-pairs graph distances (csrc/graph_paths.hip; tests/test_graph_paths_host.py and
tests/test_graph_paths_gpu.py).

A case is a CSR adjacency (row v = out-neighbours of v, int32), optionally with integer edge costs, generated from a fixed seed.
The oracle is a plain-Python BFS (`deque`) / Dijkstra (`heapq`) over the same CSR on Python ints: out[v][s] = d(v -> s), -1
where s cannot be reached.  Sizes sit at the edges of the 64-bit word and of the 64 x 64 tile: n = 1, 2, 63, 64, 65, 128, 129,
257, and one sparse graph of n = 1025 (17 tile rounds)."""
import heapq
from collections import deque

import numpy as np

SIZES = (1, 2, 63, 64, 65, 128, 129, 257)
LEVEL_BATCH = 8                     # graphembed.data.graph.LEVEL_BATCH, restated (the host test compares them)
COST_BOUND = 2**30                  # (n - 1) * max cost stays below it


class Case:
    def __init__(self, name, n, edges, directed, costs=None, tags=()):
        """edges: list of (u, v) — stored as given (u -> v) for a directed case, in both directions otherwise; repeated entries and
        self-loops are kept as they are.  costs: one per entry of `edges`."""
        self.name, self.n, self.directed, self.tags = name, n, directed, set(tags)
        rows = [[] for _ in range(n)]
        for k, (u, v) in enumerate(edges):
            c = None if costs is None else int(costs[k])
            rows[u].append((v, c))
            if not directed and u != v:
                rows[v].append((u, c))
        indptr, indices, cst = [0], [], []
        for r in rows:
            for v, c in r:   # (insertion order: repeated neighbours stay repeated, nothing is sorted)
                indices.append(v)
                cst.append(c)
            indptr.append(len(indices))
        self.indptr = np.asarray(indptr, dtype=np.int32)
        self.indices = np.asarray(indices, dtype=np.int32)
        self.costs = None if costs is None else np.asarray(cst, dtype=np.int32)
        self._oracle = None

    @property
    def weighted(self):
        return self.costs is not None

    def oracle(self):
        """[n][n] int32, computed once and shared (read-only)"""
        if self._oracle is None:
            d = dijkstra_all(self.indptr, self.indices, self.costs, self.n) if self.weighted else bfs_all(self.indptr, self.indices, self.n)
            d.setflags(write=False)
            self._oracle = d
        return self._oracle

    def scipy_matrix(self):
        """csr_array for scipy.sparse.csgraph.shortest_path: parallel edges reduced to the cheapest, self-loops dropped (scipy sums
        duplicates on conversion, which is not what a multigraph means); stored zeros are zero-cost edges"""
        import scipy.sparse as sp
        best = {}
        for v in range(self.n):
            for e in range(self.indptr[v], self.indptr[v + 1]):
                u = int(self.indices[e])
                c = 1 if self.costs is None else int(self.costs[e])
                if u != v:
                    best[(v, u)] = min(best.get((v, u), c), c)
        r = np.asarray([k[0] for k in best], dtype=np.int32)
        c = np.asarray([k[1] for k in best], dtype=np.int32)
        d = np.asarray(list(best.values()), dtype=np.float64)
        return sp.csr_array((d, (r, c)), shape=(self.n, self.n))

    def networkx(self, weight='weight'):
        """the same graph as a networkx (Di)Graph with nodes 0..n-1 (parallel edges reduced to the cheapest, self-loops dropped)"""
        import networkx as nx
        g = nx.DiGraph() if self.directed else nx.Graph()
        g.add_nodes_from(range(self.n))
        m = self.scipy_matrix().tocoo()
        for u, v, c in zip(m.row, m.col, m.data):
            if self.weighted:
                g.add_edge(int(u), int(v), **{weight: int(c)})
            else:
                g.add_edge(int(u), int(v))
        return g

    def __repr__(self):
        return self.name


def bfs_all(indptr, indices, n):
    out = np.full((n, n), -1, dtype=np.int32)
    ip, ix = [int(x) for x in indptr], [int(x) for x in indices]
    # out[v][s] = d(v -> s): a BFS from v along out-edges fills row v
    for v in range(n):
        dist = [-1] * n
        dist[v] = 0
        q = deque([v])
        while q:
            a = q.popleft()
            for e in range(ip[a], ip[a + 1]):
                b = ix[e]
                if dist[b] < 0:
                    dist[b] = dist[a] + 1
                    q.append(b)
        out[v] = dist
    return out


def dijkstra_all(indptr, indices, costs, n):
    out = np.full((n, n), -1, dtype=np.int32)
    ip, ix, cs = [int(x) for x in indptr], [int(x) for x in indices], [int(x) for x in costs]
    for v in range(n):
        dist = [None] * n
        dist[v] = 0
        heap = [(0, v)]
        while heap:
            da, a = heapq.heappop(heap)
            if da > dist[a]:
                continue
            for e in range(ip[a], ip[a + 1]):
                b, nd = ix[e], da + cs[e]
                if dist[b] is None or nd < dist[b]:
                    dist[b] = nd
                    heapq.heappush(heap, (nd, b))
        out[v] = [-1 if d is None else d for d in dist]
    return out


def _rng(*key):
    return np.random.default_rng(int.from_bytes(repr(key).encode(), 'little') % (2**32))


def _tree_edges(n, rng):
    return [(int(rng.integers(0, v)), v) for v in range(1, n)]


def _gnm(n, m, rng, directed=False):
    seen, out = set(), []
    m = min(m, n * (n - 1) // (1 if directed else 2))
    while len(out) < m:
        u, v = (int(x) for x in rng.integers(0, n, 2))
        if u == v:
            continue
        key = (u, v) if directed or u < v else (v, u)
        if key not in seen:
            seen.add(key)
            out.append((u, v))
    return out


def _hop_cases():
    cases = []
    for n in SIZES:
        rng = _rng('hops', n)
        cases.append(Case(f'path-{n}', n, [(v, v + 1) for v in range(n - 1)], False, tags=('path', 'connected')))
        cases.append(Case(f'cycle-{n}', n, [(v, (v + 1) % n) for v in range(n)] if n > 2 else [(v, v + 1) for v in range(n - 1)], False,
                          tags=('connected', )))
        cases.append(Case(f'star-{n}', n, [(0, v) for v in range(1, n)], False, tags=('connected', )))
        cases.append(Case(f'complete-{n}', n, [(u, v) for u in range(n) for v in range(u + 1, n)], False, tags=('connected', )))
        cases.append(Case(f'tree-{n}', n, _tree_edges(n, rng), False, tags=('connected', 'tree')))
        cases.append(Case(f'gnm-{n}', n, _tree_edges(n, rng) + _gnm(n, n, rng), False, tags=('connected', )))   # a tree plus n more: connected
        cases.append(Case(f'noedges-{n}', n, [], False, tags=('disconnected', ) if n > 1 else ()))
        cases.append(Case(f'dicycle-{n}', n, [(v, (v + 1) % n) for v in range(n)] if n > 1 else [], True, tags=('directed', 'connected')))
        if n >= 63:
            h = n // 2   # two components (trees plus a few edges) and the isolated node n - 1
            a = _tree_edges(h, rng) + _gnm(h, h // 2, rng)
            b = [(u + h, v + h) for u, v in _tree_edges(n - 1 - h, rng)]
            cases.append(Case(f'components-{n}', n, a + b, False, tags=('disconnected', )))
            cases.append(Case(f'digraph-{n}', n, _gnm(n, 2 * n, rng, directed=True), True, tags=('directed', 'disconnected')))
            t = _tree_edges(n, rng)   # self-loops on every third node, every tree edge listed two or three times
            cases.append(Case(f'loops-{n}', n, [(v, v) for v in range(0, n, 3)] + t + t[::2] + t, False, tags=('connected', 'multi')))
    rng = _rng('hops', 1025)
    cases.append(Case('gnm-1025', 1025, _tree_edges(1025, rng) + _gnm(1025, 2048, rng), False, tags=('connected', 'large')))
    return cases


def _cost_cases():
    cases = []
    for n in SIZES:
        rng = _rng('costs', n)
        e = _tree_edges(n, rng) + _gnm(n, 2 * n, rng)
        cases.append(Case(f'cost19-{n}', n, e, False, costs=rng.integers(1, 10, len(e)), tags=('connected', )))
        cases.append(Case(f'cost-zero-{n}', n, e, False, costs=rng.integers(0, 3, len(e)), tags=('connected', 'zero')))
        ed = _gnm(n, 3 * n, rng, directed=True)
        cases.append(Case(f'cost-digraph-{n}', n, ed, True, costs=rng.integers(1, 10, len(ed)), tags=('directed', )))
        if n >= 63:
            # a ring of cost 1 and chords of cost 40: the cheapest route to a chord's end walks round the ring in up to 39 hops
            ring = [(v, (v + 1) % n) for v in range(n)]
            chords = [(v, (v + 20) % n) for v in range(0, n, 7)]
            cases.append(Case(f'cost-detour-{n}', n, ring + chords, False, costs=[1] * len(ring) + [40] * len(chords),
                              tags=('connected', 'detour')))
            # every tree edge three times at costs 9, 2, 5 (the cheapest in the middle), self-loops of cost 7
            t = _tree_edges(n, rng)
            cases.append(Case(f'cost-parallel-{n}', n, t + t + t + [(v, v) for v in range(0, n, 5)], False,
                              costs=[9] * len(t) + [2] * len(t) + [5] * len(t) + [7] * len(range(0, n, 5)), tags=('connected', 'multi')))
            h = n // 2
            a, b = _tree_edges(h, rng), [(u + h, v + h) for u, v in _tree_edges(n - 1 - h, rng)]
            cases.append(Case(f'cost-components-{n}', n, a + b, False, costs=rng.integers(1, 10, len(a) + len(b)),
                              tags=('disconnected', )))
    # (n - 1) * max cost just under 2^30: a path of 129 nodes whose edges all cost the largest value the bound admits — the
    # end-to-end distance is (n - 1) * max cost itself
    n = 129
    big = (COST_BOUND - 2) // (n - 1)
    path = [(v, v + 1) for v in range(n - 1)]
    cases.append(Case('cost-bound-129', n, path, False, costs=[big] * len(path), tags=('connected', 'bound')))
    rng = _rng('costs', 1025)
    e = _tree_edges(1025, rng) + _gnm(1025, 2048, rng)
    cases.append(Case('cost19-1025', 1025, e, False, costs=rng.integers(1, 10, len(e)), tags=('connected', 'large')))
    return cases


HOP_CASES = _hop_cases()
COST_CASES = _cost_cases()
ALL_CASES = HOP_CASES + COST_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def diameter(d):
    """largest finite entry of a distance matrix"""
    return int(np.asarray(d).max()) if np.asarray(d).size else 0


def targets_reference(dist, torch_dtype):
    """(condensed, dense) as GraphDataset computes them on the CPU from the upper triangle of an oracle matrix without -1 entries"""
    import torch
    from scipy.spatial.distance import squareform
    from graphembed.data.dataset import GraphDataset
    pd = squareform(np.asarray(dist, dtype=np.float64), checks=False)
    ds = GraphDataset(torch.from_numpy(pd).to(torch_dtype))
    return ds.condensed, ds.pdists
