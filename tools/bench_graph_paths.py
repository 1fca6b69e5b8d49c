#!/usr/bin/env python3
"""All-pairs graph distances: the scipy route against the GPU route (csrc/graph_paths.hip), same process, same box.

Graphs: G(4039, 88 234) and G(16 384, 760 000), fixed seeds; hops and integer costs 1 ... 9 timed separately.  Rows:
  scipy      scipy.sparse.csgraph.shortest_path from the sparse adjacency (BFS for hops, Dijkstra for costs) — the route of
             compute_graph_pdists / FastPrecision without a GPU
  gpu e2e    from the networkx graph to device-resident targets: CSR on the host, upload, mm_graph_hops in batches or
             mm_graph_cost_paths, mm_graph_targets (condensed fp32) — ends in a device synchronise
  kernels    the C-ABI calls alone on a resident CSR (device events around them)
Median of --reps after one warm-up.  The Floyd-Warshall row also reports 2 n^3 integer operations over its kernel time.

    python tools/bench_graph_paths.py [--sizes small,large] [--reps 5] [--scipy-large] [--out FILE.json]
Prints a markdown table and one JSON line; scipy on the large graph takes minutes per run and is off unless --scipy-large."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

GRAPHS = {'small': (4039, 88234, 11), 'large': (16384, 760000, 12)}


def make_graph(n, m, seed):
    g = nx.gnm_random_graph(n, m, seed=seed)
    rng = np.random.default_rng(seed)
    for (u, v), c in zip(g.edges(), rng.integers(1, 10, g.number_of_edges())):
        g[u][v]['weight'] = int(c)
    return g


def median_of(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def scipy_route(g, weighted):
    from scipy.sparse.csgraph import shortest_path
    n = g.number_of_nodes()
    if weighted:
        a = nx.to_scipy_sparse_array(g, nodelist=range(n), weight='weight')
        return shortest_path(a, method='D', unweighted=False, directed=False)
    a = nx.to_scipy_sparse_array(g, nodelist=range(n))
    return shortest_path(a, unweighted=True, directed=False)


def gpu_route(g, weighted):
    """networkx graph -> distances and condensed fp32 targets on the device; returns (dist, condensed, stats)"""
    from graphembed import _backend as B
    from graphembed.data.graph import graph_distances
    dist = graph_distances(g, 'cuda', weight='weight' if weighted else None)
    n = dist.shape[0]
    stats = torch.empty(2, dtype=torch.int64, device='cuda')
    cond = torch.empty(n * (n - 1) // 2, dtype=torch.float32, device='cuda')
    B.lib().call('mm_graph_targets', B.MM_F32, B.ptr(dist), n, B.ptr(stats), B.ptr(cond), None, B.stream_of(dist))
    torch.cuda.synchronize()
    return dist, cond, stats


def kernel_times(g, weighted, reps):
    """(distance entry, targets entry) in seconds: device events around the C-ABI calls on a resident CSR"""
    from graphembed import _backend as B
    from graphembed.data.graph import LEVEL_BATCH, weighted_csr
    lib = B.lib()
    n = g.number_of_nodes()
    indptr, indices, costs = (torch.from_numpy(a).cuda() for a in weighted_csr(g, 'weight'))
    dist = torch.empty(n, n, dtype=torch.int32, device='cuda')
    nbytes = lib.raw('mm_graph_hops_ws_bytes')(n)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device='cuda')
    flags = torch.empty(LEVEL_BATCH, dtype=torch.int32, device='cuda')
    stats = torch.empty(2, dtype=torch.int64, device='cuda')
    cond = torch.empty(n * (n - 1) // 2, dtype=torch.float32, device='cuda')
    st = B.stream_of(dist)

    def distances():
        if weighted:
            lib.call('mm_graph_cost_paths', B.ptr(indptr), B.ptr(indices), B.ptr(costs), n, B.ptr(dist), st)
            return
        level = 0
        while True:   # (the flag read between batches is part of the route: it is what decides the number of launches)
            lib.call('mm_graph_hops', B.ptr(indptr), B.ptr(indices), n, level, LEVEL_BATCH, B.ptr(dist), B.ptr(flags), B.ptr(ws),
                     nbytes, st)
            level += LEVEL_BATCH
            if int(flags[-1].item()) == 0 or level >= n:
                return

    def targets():
        lib.call('mm_graph_targets', B.MM_F32, B.ptr(dist), n, B.ptr(stats), B.ptr(cond), None, st)

    out = []
    for fn in (distances, targets):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        out.append(statistics.median(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='small,large')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scipy-large', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_graph_paths.py measures the GPU route: no GPU here')
    from bench_configs import host_calibration
    rows, result = [], {'_host': host_calibration()}
    for size in a.sizes.split(','):
        n, m, seed = GRAPHS[size]
        g = make_graph(n, m, seed)
        for weighted in (False, True):
            kind = 'costs 1-9' if weighted else 'hops'
            do_scipy = size != 'large' or a.scipy_large
            t_scipy = median_of(lambda: scipy_route(g, weighted), a.reps) if do_scipy else None
            t_e2e = median_of(lambda: gpu_route(g, weighted), a.reps)
            t_dist, t_targets = kernel_times(g, weighted, a.reps)
            if do_scipy:   # the answers at the timed size
                want = scipy_route(g, weighted)
                got = gpu_route(g, weighted)[0].cpu().numpy()
                assert np.array_equal(got, np.where(np.isfinite(want), want, -1).astype(np.int32)), (size, kind)
            row = {'graph': size, 'n': n, 'edges': m, 'kind': kind, 'scipy_s': t_scipy, 'gpu_e2e_s': t_e2e, 'dist_kernels_s': t_dist,
                   'targets_kernels_s': t_targets}
            if weighted:
                row['fw_int_ops_per_s'] = 2.0 * n**3 / t_dist
            rows.append(row)
            print(json.dumps(row), flush=True)
    result['rows'] = rows
    fmt = lambda v: 'not measured' if v is None else f'{v:.4g} s'   # noqa: E731
    print('\n| Graph | n | Edges | Distances | scipy | GPU end to end | distance kernels | target kernels | speed-up (scipy / e2e) |')
    print('|---|---|---|---|---|---|---|---|---|')
    for r in rows:
        sp = 'n/a' if r['scipy_s'] is None else f"{r['scipy_s'] / r['gpu_e2e_s']:.1f} x"
        print(f"| {r['graph']} | {r['n']} | {r['edges']} | {r['kind']} | {fmt(r['scipy_s'])} | {fmt(r['gpu_e2e_s'])} | "
              f"{fmt(r['dist_kernels_s'])} | {fmt(r['targets_kernels_s'])} | {sp} |")
    for r in rows:
        if 'fw_int_ops_per_s' in r:
            print(f"Floyd-Warshall n = {r['n']}: 2 n^3 = {2.0 * r['n']**3:.3g} integer operations in {r['dist_kernels_s']:.4g} s = "
                  f"{r['fw_int_ops_per_s']:.3g} op/s")
    h = result['_host']
    print(f"Host of this run: one eager torch launch {h['launch_us']:.1f} us, one C-ABI call {h['cabi_us']:.2f} us, 1000 python "
          f"iterations {h['python_us']:.0f} us ({h['host_cpus']} CPUs)")
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
