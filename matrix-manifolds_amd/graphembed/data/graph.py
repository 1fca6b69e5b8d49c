"""Graph loading and all-pairs shortest paths — counterpart of
graphembed/graphembed/data/graph.py:15-87 (edge lists / .npy).  The distances come from the GPU
(csrc/graph_paths.hip, `graph_distances`) where there is one and from scipy's BFS / Dijkstra elsewhere
or under MM_GRAPH_APSP=scipy; the reference's networkit is not a dependency here."""
import gzip
import os

import numpy as np
import torch

CACHED_PDISTS_FILE = 'cached_pdists.npy'


COST_SENTINEL = 2**30 - 1   # the "no route" value inside mm_graph_cost_paths: finite distances stay below it
LEVEL_BATCH = 8             # hop levels issued per call of mm_graph_hops, between two looks at the last flag


def gpu_apsp_enabled():
    """True when all-pairs distances go through csrc/graph_paths.hip: a GPU and the built library are there and
    MM_GRAPH_APSP is not `scipy` (the switch that forces scipy's BFS / Dijkstra, the only route on a machine without a GPU)."""
    from graphembed import _backend as B
    if os.environ.get('MM_GRAPH_APSP', '').lower() == 'scipy':
        return False
    return torch.cuda.is_available() and os.path.isfile(B.LIB_PATH)


def weighted_csr(g, weight):
    """(indptr, indices, costs) of a networkx graph with nodes 0..n-1, as numpy int32 arrays: row v lists the out-neighbours of
    v in ascending order (the layout of metrics.graph_csr) and the cost of each edge (1 where the attribute is missing, as
    networkx's own matrices have it).  ValueError for costs that are negative, not integers, or beyond (n - 1) * max cost <
    2^30 - 1 — the precondition of mm_graph_cost_paths."""
    n = g.number_of_nodes()
    indptr = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for u in range(n):
        nb = sorted((v, d.get(weight, 1)) for v, d in g[u].items())
        cols.extend(v for v, _ in nb)
        vals.extend(c for _, c in nb)
        indptr[u + 1] = indptr[u] + len(nb)
    vals = np.asarray(vals, dtype=np.float64)
    if vals.size:
        if not np.all(np.isfinite(vals)) or not np.all(np.equal(np.mod(vals, 1), 0)):
            raise ValueError('graph distances on the GPU need integer edge costs')
        if vals.min() < 0:
            raise ValueError('graph distances need edge costs >= 0')
        if max(n - 1, 1) * int(vals.max()) >= COST_SENTINEL:
            raise ValueError(f'edge costs too large: (n - 1) * max cost = {max(n - 1, 1) * int(vals.max())} must stay below '
                             f'2^30 - 1 = {COST_SENTINEL}')
    return indptr.astype(np.int32), np.asarray(cols, dtype=np.int32), vals.astype(np.int32)


def _scipy_distances(g, weight):
    import networkx as nx
    from scipy.sparse.csgraph import shortest_path
    n = g.number_of_nodes()
    if weight is None:
        a = nx.to_scipy_sparse_array(g, nodelist=range(n))
        return shortest_path(a, unweighted=True, directed=g.is_directed())
    a = nx.to_scipy_sparse_array(g, nodelist=range(n), weight=weight)
    return shortest_path(a, method='D', unweighted=False, directed=g.is_directed())


def graph_distances(g, device=None, weight=None):
    """All-pairs shortest-path distances of a networkx graph with nodes 0..n-1 as an int32 [n, n] tensor on `device`:
    out[v][s] = d(v -> s), -1 where s cannot be reached.  weight=None counts hops; otherwise `weight` names the edge attribute
    that holds the integer costs (>= 0, (n - 1) * max cost < 2^30 - 1; ValueError otherwise).  On a cuda device the matrix is
    computed there (mm_graph_hops: bit-parallel BFS from every source at once; mm_graph_cost_paths: blocked Floyd-Warshall) and
    never leaves it; on the CPU, without the library or under MM_GRAPH_APSP=scipy it is scipy's, the same integers."""
    if device is None:
        device = 'cuda' if gpu_apsp_enabled() else 'cpu'
    device = torch.device(device)
    n = g.number_of_nodes()
    if weight is not None:
        indptr, indices, costs = weighted_csr(g, weight)    # (validates the costs on either route)
    if device.type != 'cuda' or not gpu_apsp_enabled():
        d = _scipy_distances(g, weight)
        return torch.from_numpy(np.where(np.isfinite(d), d, -1).astype(np.int32)).to(device)
    from graphembed import _backend as B
    from graphembed.metrics import graph_csr
    lib = B.lib()
    if n > lib.raw('mm_graph_max_nodes')():
        raise B.BackendError(f'graphs of {n} nodes exceed the all-pairs kernels\' range')
    with B.on_device(device):
        dist = torch.empty(n, n, dtype=torch.int32, device=device)
        if n == 0:
            return dist
        st = B.stream_of(dist)
        if weight is not None:
            indptr, indices, costs = (torch.from_numpy(a).to(device) for a in (indptr, indices, costs))
            lib.call('mm_graph_cost_paths', B.ptr(indptr), B.ptr(indices), B.ptr(costs), n, B.ptr(dist), st)
            return dist
        indptr, indices = graph_csr(g, device)
        if indices.numel() == 0:
            indices = torch.zeros(1, dtype=torch.int32, device=device)
        nbytes = lib.raw('mm_graph_hops_ws_bytes')(n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        flags = torch.empty(LEVEL_BATCH, dtype=torch.int32, device=device)
        level = 0
        while True:   # a level that finds nothing ends the search; no route is longer than n - 1 hops
            lib.call('mm_graph_hops', B.ptr(indptr), B.ptr(indices), n, level, LEVEL_BATCH, B.ptr(dist), B.ptr(flags), B.ptr(ws),
                     nbytes, st)
            level += LEVEL_BATCH
            if int(flags[-1].item()) == 0 or level >= n:
                return dist


def compute_graph_pdists(g, cache_dir=None):
    from scipy.spatial.distance import squareform
    if gpu_apsp_enabled():
        d = graph_distances(g, 'cuda').cpu().numpy().astype(np.float64)
        d[d < 0] = np.inf
    else:
        d = _scipy_distances(g, None)
    pd = squareform(d, checks=False)
    if cache_dir:
        np.save(os.path.join(cache_dir, CACHED_PDISTS_FILE), pd)
    return pd


def load_graph_pdists(f, cache_dir=None, flip_probability=None):
    """Returns (condensed shortest-path distances as a tensor, networkx graph or None)."""
    import networkx as nx
    if flip_probability is not None:
        raise NotImplementedError('noisy-graph generation is outside the accelerated path')
    f = os.path.abspath(os.path.realpath(f))
    if f.endswith('.npy'):
        return torch.from_numpy(np.load(f)).to(torch.get_default_dtype()), None
    directed = f.endswith('.dir-edges') or f.endswith('.dir-edges.gz')
    opener = gzip.open if f.endswith('.gz') else open
    with opener(f, 'rt') as fh:
        g = nx.parse_edgelist((l for l in fh if l.strip() and not l.startswith('#')),
                              create_using=nx.DiGraph if directed else nx.Graph, data=False)
    g = nx.convert_node_labels_to_integers(g)
    assert g.is_directed() or nx.number_connected_components(g) == 1
    cache = None
    if cache_dir is not None:
        cache = os.path.join(cache_dir, os.path.basename(f))
        cached = os.path.join(cache, CACHED_PDISTS_FILE)
        if os.path.isfile(cached):
            return torch.from_numpy(np.load(cached)).to(torch.get_default_dtype()), g
        os.makedirs(cache, exist_ok=True)
    pd = compute_graph_pdists(g, cache)
    return torch.from_numpy(pd).to(torch.get_default_dtype()), g
