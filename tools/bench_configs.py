#!/usr/bin/env python3
"""Secondary measurements: fwd+bwd time of the hot path on every BASELINE.json configuration
(synthetic inputs of the named sizes).  Prints one JSON object.
Usage: python tools/bench_configs.py [--only NAME]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
from graphembed import manifolds as M  # noqa: E402
from graphembed._backend import unit_seed  # noqa: E402
from graphembed.modules import ManifoldEmbedding  # noqa: E402
from graphembed.objectives import StochasticNeighborLoss, StochasticTreeLoss, StressLoss  # noqa: E402
from graphembed.optim import RiemannianAdam, RiemannianSGD  # noqa: E402


def timeit(fn, iters=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def pdist_case(man, n, dtype, **kw):
    torch.manual_seed(42)
    x = man.rand(n, out=torch.empty(0, dtype=dtype, device='cuda'), **kw).requires_grad_()
    P = n * (n - 1) // 2
    g = torch.randn(P, dtype=dtype, device='cuda')
    fwd = timeit(lambda: man.pdist(x, squared=True))

    def both():
        d2 = man.pdist(x, squared=True)
        torch.autograd.grad(d2, x, g)
    tot = timeit(both)
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'fwd_us': fwd, 'fwd_bwd_us': tot,
            'pairs_per_s': P / (tot * 1e-6), 'GBps_8B_per_pair': P * 2 * x.element_size() / (tot * 1e-6) / 1e9}


def native_case(mans, n, dtype, loss='stress'):
    """full training step through ONE C-ABI call (mm_train_step_run / NativeTrainStep), replayed as a hipGraph — for a
    single SPD factor two launches per step: pair kernel + fused finalize / update / tables (bench.TrainStepWorkload)"""
    import bench
    wl = bench.TrainStepWorkload(mans, n, dtype, torch.device('cuda', 0), loss=loss)
    graph, _ = bench.graph_of(wl.kernels, bench.Fence(1))
    t = timeit(graph.replay, iters=40, warm=200)
    P = n * (n - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def step_case(mans, n, dtype, fused=False, graph=False, pair_kernel=True, adam=False, sne=None, sst=None, native=True, batch=None,
              exact=True, torch_ops=None, iters=20, warm=5):
    """full training step: compute_dists + stress loss + backward + fused RSGD (momentum 0); `sne` = 'incl' / 'excl': the
    stochastic-neighbour KL loss instead (alpha = 1), on its kernels or, `native=False`, in its torch-op form; `sst`: the
    spanning-tree KL loss likewise ('excl' with the reference's gradient, the class's default); `batch`: a fixed index batch of
    that many nodes through BatchedObjective (the reference's batch_size) instead of the full batch; `exact=False`: the manifold's
    retraction (the fused step kernel where exp has none); `torch_ops`: a function x -> pair vector of squared distances in
    torch ops that stands in for the manifold's pdist (the yardstick of a factor the reference cannot train; not with `fused` or
    `batch`)"""
    assert torch_ops is None or not (fused or batch), 'torch_ops replaces the unfused full-batch pdist'
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, mans)
            emb.pair_kernel = pair_kernel  # products: the single mixed-manifold pair kernel
    finally:
        torch.set_default_dtype(torch.float32)
    P = n * (n - 1) // 2
    target = torch.rand(P, dtype=dtype, device='cuda') * 0.99 + 0.01
    fn = StressLoss() if sne is None else StochasticNeighborLoss(inclusive=sne == 'incl', native=native)
    if sst is not None:
        fn = StochasticTreeLoss(inclusive=sst == 'incl', native=native)
    kw = {} if sne is None and sst is None else {'alpha': 1.0}
    if batch is not None:
        from graphembed.data import GraphDataset
        from graphembed.modules import BatchedObjective
        obj = BatchedObjective(fn, GraphDataset(target), emb)
        obj.check_indices = False   # a slice of a randperm
        idx = torch.randperm(n, device='cuda')[:batch].clone()
        P = batch * (batch - 1) // 2
    if adam:  # the optimizer of the paper grid (experiments/run_grid.py:24-36)
        opt = RiemannianAdam(list(emb.xs), lr=1e-3, exact=exact, max_grad_norm=20)
        opt_s = RiemannianAdam(list(emb.scales), lr=1e-4, max_grad_norm=500)
    else:
        opt = RiemannianSGD(list(emb.xs), lr=1e-3, exact=exact, max_grad_norm=20)
        opt_s = RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)

    def step():
        opt.zero_grad(set_to_none=True)
        opt_s.zero_grad(set_to_none=True)
        if batch is not None:
            loss = obj(idx, epoch=0, **kw)
        else:
            if fused:
                loss = emb.fused_objective(fn, target, None)
            elif torch_ops is not None:
                loss = fn(target, torch.nn.functional.softplus(emb.scales[0]) * torch_ops(emb.xs[0]), **kw)
            else:
                loss = fn(target, emb.compute_dists(None), **kw)
        loss.backward(unit_seed(loss))
        opt.step()
        opt_s.step()
    if graph:  # whole training step replayed as one hipGraph (static shapes, no host sync inside)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        t = timeit(gr.replay, iters, warm)
    else:
        t = timeit(step, iters, warm)
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


class _SoPdistTorchOps(torch.autograd.Function):
    """SpecialOrthogonal.pdist(x, squared=True) in torch ops on the GPU — the formulas of csrc/so_pair.hpp on the gathered pairs:
    D = x_j - x_i = U S V^T (torch.linalg.svd), d2 = sum 4 asin^2(S / 2), d d2 / dx_j = U diag(S psi') V^T.  (Written out: autograd
    through the SVD divides by differences of singular values, and every rotation plane appears twice.)"""

    @staticmethod
    def forward(ctx, x):
        n = x.shape[0]
        ij = torch.triu_indices(n, n, 1, device=x.device)
        xd = x.detach()
        U, S, Vh = torch.linalg.svd(xd[ij[1]] - xd[ij[0]])
        s = (S / 2).clamp(max=1)
        half = torch.asin(s)
        dpsi = 2 * torch.where(s > 1e-20, half / s.clamp_min(1e-20), torch.ones_like(s)) / (1 - s * s).clamp_min(1e-12).sqrt()
        ctx.save_for_backward(ij, (U * (S * dpsi).unsqueeze(-2)) @ Vh)
        ctx.n = n
        return (4 * half * half).sum(-1)

    @staticmethod
    def backward(ctx, g):
        ij, dD = ctx.saved_tensors
        gj = g.reshape(-1, 1, 1) * dD
        return torch.zeros(ctx.n, *dD.shape[1:], dtype=dD.dtype, device=dD.device).index_add_(0, ij[1], gj).index_add_(0, ij[0], -gj)


def stereo_pdist_case(m, n, dtype):
    """one constant-curvature factor (graphembed.manifolds.Stereographic): pdist forward | forward + backward (points and curvature)"""
    man = M.Stereographic(m).to(device='cuda', dtype=dtype)
    torch.manual_seed(42)
    x = man.rand(n, out=torch.empty(0, dtype=dtype, device='cuda')).requires_grad_()
    P = n * (n - 1) // 2
    g = torch.randn(P, dtype=dtype, device='cuda')
    fwd = timeit(lambda: man.pdist(x, squared=True))

    def both():
        d2 = man.pdist(x, squared=True)
        torch.autograd.grad(d2, (x, man.c), g)
    tot = timeit(both)
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'fwd_us': fwd, 'fwd_bwd_us': tot, 'pairs_per_s': P / (tot * 1e-6)}


def stereo_step_case(ds, n, dtype, graph=False, fused=False, quotient=False):
    """training step of a product of constant-curvature factors (StereographicProductEmbedding): objective (stress, or the
    quotient loss at epoch 1) + backward + fused RSGD step of the points + SGD step of the curvatures + stabilize.  `fused`: the
    multi-factor pair kernel (mm_stereo_product_loss, one pair pass for all factors); otherwise the per-factor route
    (`pair_kernel = False`: one pdist forward and backward per factor, the loss as element-wise torch passes)"""
    from graphembed.modules import StereographicProductEmbedding
    from graphembed.objectives import QuotientLoss
    torch.manual_seed(0)
    emb = StereographicProductEmbedding(n, ds).to(device='cuda', dtype=dtype)
    emb.pair_kernel = fused
    P = n * (n - 1) // 2
    target = torch.rand(P, dtype=dtype, device='cuda') * 0.99 + 0.01
    fn = QuotientLoss() if quotient else StressLoss()
    kw = dict(epoch=1, alpha=1.0) if quotient else {}
    opt = RiemannianSGD([dict(params=list(emb.xs), lr=1e-3, exact=True, max_grad_norm=20),
                         dict(params=list(emb.curvature_params), lr=1e-4, exact=False, max_grad_norm=None)], lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = emb.fused_objective(fn, target, None, **kw) if fused else fn(target, emb.compute_dists(None), **kw)
        loss.backward(unit_seed(loss))
        opt.step()
        emb.stabilize()
    if graph:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        t = timeit(gr.replay)
    else:
        t = timeit(step)
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def stereo_minibatch_case(ds, n, bs, dtype, graph=False, in_kernel=True):
    """node-minibatch training step of a product of constant-curvature factors as the reference's product grid runs it
    (experiments/products/run_prod_grid.py: RiemannianAdam, the points exact, the curvatures a group of their own; stabilize):
    objective over the batch + backward + Adam + stabilize.  `in_kernel`: the index vector inside the pair kernel
    (mm_stereo_product_loss_subset) and one mm_stereo_radam_step per factor; otherwise the route before them - the dataset's
    target gather, `take_rows`, mm_stereo_product_loss, scatter-add backward, and Adam composed from the class's maps"""
    from graphembed.data import GraphDataset
    from graphembed.modules import BatchedObjective, StereographicProductEmbedding
    torch.manual_seed(0)
    emb = StereographicProductEmbedding(n, ds).to(device='cuda', dtype=dtype)
    data = GraphDataset(torch.rand(n * (n - 1) // 2, dtype=dtype, device='cuda') * 0.99 + 0.01)
    if not in_kernel:
        class Gathered:   # the same targets without the dense matrix on offer
            __getitem__ = staticmethod(data.__getitem__)
        data = Gathered()
        for man in emb.manifolds:
            man.radam_step = None   # RiemannianAdam then composes the update from egrad2rgrad / norm / exp / transp
    obj = BatchedObjective(StressLoss(), data, emb)
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=0.05, exact=True), dict(params=list(emb.curvature_params), lr=0.05)])
    perm = torch.randperm(n, device='cuda')
    idx = perm[:bs].clone()
    state = {'i': 0}

    def step():
        opt.zero_grad(set_to_none=True)
        loss = obj(idx)
        loss.backward(unit_seed(loss))
        opt.step()
        emb.stabilize()

    def advance():
        i = state['i']
        idx.copy_(perm[i:i + bs])
        state['i'] = (i + bs) % max(n - bs, 1)
    if graph:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        run = gr.replay
    else:
        run = step

    def timed():
        advance()
        run()
    t = timeit(timed, iters=50)
    P = bs * (bs - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def grass_minibatch_case(N, p, n, bs, dtype, graph=False, in_kernel=True):
    """node-minibatch training step of a Grassmann embedding as the reference's grid runs it (experiments/run_grid.py:24-36,
    123-134: RiemannianAdam(lr=0.01, exact=True, max_grad_norm=100), batch_size=512): objective over the batch + backward +
    Adam on the points and on the scale.  `in_kernel`: the index vector inside the pair kernel (mm_grass_pdist_loss_subset) and
    one mm_mat_radam_step; otherwise the route before them - the dataset's target gather, `take_rows`, mm_grass_pdist_loss,
    scatter-add backward, and Adam composed from egrad2rgrad / norm / exp / transp"""
    from graphembed.data import GraphDataset
    from graphembed.modules import BatchedObjective
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, [M.Grassmann(N, p)])
    finally:
        torch.set_default_dtype(torch.float32)
    data = GraphDataset(torch.rand(n * (n - 1) // 2, dtype=dtype, device='cuda') * 0.99 + 0.01)
    if not in_kernel:
        class Gathered:   # the same targets without the dense matrix on offer
            __getitem__ = staticmethod(data.__getitem__)
        data = Gathered()
        emb.manifolds[0].radam_step = None   # RiemannianAdam then composes the update
    obj = BatchedObjective(StressLoss(), data, emb)
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=0.01, exact=True, max_grad_norm=100), dict(params=list(emb.scales), lr=0.01)])
    perm = torch.randperm(n, device='cuda')
    idx = perm[:bs].clone()
    state = {'i': 0}

    def step():
        opt.zero_grad(set_to_none=True)
        loss = obj(idx)
        loss.backward(unit_seed(loss))
        opt.step()

    def advance():
        i = state['i']
        idx.copy_(perm[i:i + bs])
        state['i'] = (i + bs) % max(n - bs, 1)
    if graph:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        run = gr.replay
    else:
        run = step

    def timed():
        advance()
        run()
    t = timeit(timed, iters=50)
    P = bs * (bs - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def so_minibatch_case(N, n, bs, dtype, graph=False, in_kernel=True, sne=False):
    """node-minibatch training step of an SO(N) embedding with the reference grid's optimizer settings (experiments/run_grid.py:
    RiemannianAdam(lr=0.01, max_grad_norm=100), batch_size=512) and the retraction (`exact` stays on the optimizers' generic
    route for SO(n)): objective over the batch + backward + Adam on the points (mm_mat_radam_step either way) and on the scale.
    `in_kernel`: the index vector inside the pair kernels of csrc/so.hip (SUB); otherwise the route before them - the dataset's
    target gather, `take_rows`, the full-batch kernels on the gathered rows, zero fill and index_add in the backward.  `sne`: the
    StochasticNeighborLoss on the pair vector of compute_dists (mm_so_pdist_fwd_subset / _bwd_subset) instead of the fused stress
    objective (mm_so_pdist_loss_subset)"""
    from graphembed.data import GraphDataset
    from graphembed.modules import BatchedObjective
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, [M.SpecialOrthogonal(N)])
    finally:
        torch.set_default_dtype(torch.float32)
    data = GraphDataset(torch.rand(n * (n - 1) // 2, dtype=dtype, device='cuda') * 0.99 + 0.01)
    if not in_kernel:
        class Gathered:   # the same targets without the dense matrix on offer
            __getitem__ = staticmethod(data.__getitem__)
        data = Gathered()
        emb.manifolds[0].pdist_subset = None   # compute_dists then gathers its rows
    obj = BatchedObjective(StochasticNeighborLoss() if sne else StressLoss(), data, emb)
    kw = dict(alpha=1.0) if sne else {}
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=0.01, exact=False, max_grad_norm=100), dict(params=list(emb.scales), lr=0.01)])
    perm = torch.randperm(n, device='cuda')
    idx = perm[:bs].clone()
    state = {'i': 0}

    def step():
        opt.zero_grad(set_to_none=True)
        loss = obj(idx, **kw)
        loss.backward(unit_seed(loss))
        opt.step()

    def advance():
        i = state['i']
        idx.copy_(perm[i:i + bs])
        state['i'] = (i + bs) % max(n - bs, 1)
    if graph:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        run = gr.replay
    else:
        run = step

    def timed():
        advance()
        run()
    t = timeit(timed, iters=50)
    P = bs * (bs - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def stein_minibatch_case(d, n, bs, dtype, graph=False, in_kernel=True):
    """node-minibatch training step of a Stein-divergence SPD(d) embedding (the `spdstein` factor of the reference grid) with the
    grid's optimizer settings, as so_minibatch_case: fused stress objective over the batch + backward + Adam on the points
    (mm_spd_radam_step either way) and on the scale.  `in_kernel`: the index vector inside the Stein pair kernel
    (mm_spd_stein_pdiv_loss_subset); otherwise the route before it - the dataset's target gather, `take_rows`, the Stein forward
    and backward kernels on the gathered rows around mm_product_loss, zero fill and index_add in the backward"""
    from graphembed.data import GraphDataset
    from graphembed.modules import BatchedObjective
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, [M.SymmetricPositiveDefinite(d, use_stein_div=True)])
    finally:
        torch.set_default_dtype(torch.float32)
    data = GraphDataset(torch.rand(n * (n - 1) // 2, dtype=dtype, device='cuda') * 0.01 + 0.001)
    if not in_kernel:
        class Gathered:   # the same targets without the dense matrix on offer
            __getitem__ = staticmethod(data.__getitem__)
        data = Gathered()
        man = emb.manifolds[0]
        man.pdist_loss = man.pdist_loss_subset = man.pdist_subset = None   # the manifold as it was before the fused Stein kernels
    obj = BatchedObjective(StressLoss(), data, emb)
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=0.01, exact=False, max_grad_norm=100), dict(params=list(emb.scales), lr=0.01)])
    perm = torch.randperm(n, device='cuda')
    idx = perm[:bs].clone()
    state = {'i': 0}

    def step():
        opt.zero_grad(set_to_none=True)
        loss = obj(idx)
        loss.backward(unit_seed(loss))
        opt.step()

    def advance():
        i = state['i']
        idx.copy_(perm[i:i + bs])
        state['i'] = (i + bs) % max(n - bs, 1)
    if graph:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        run = gr.replay
    else:
        run = step

    def timed():
        advance()
        run()
    t = timeit(timed, iters=50)
    P = bs * (bs - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def _stein3():
    return M.SymmetricPositiveDefinite(3, use_stein_div=True)


CASES = {
    'c3_spd3_stein_step_n5000_f32': lambda: step_case([_stein3()], 5000, torch.float32),
    'c3_spd3_stein_step_n5000_f32_fused': lambda: step_case([_stein3()], 5000, torch.float32, fused=True),
    'c3_spd3_stein_step_n5000_f32_fused_graph': lambda: step_case([_stein3()], 5000, torch.float32, fused=True, graph=True),
    'c3_spd3_stein_minibatch512_step_f32': lambda: stein_minibatch_case(3, 5000, 512, torch.float32),
    'c3_spd3_stein_minibatch512_step_f32_graph': lambda: stein_minibatch_case(3, 5000, 512, torch.float32, graph=True),
    'c3_spd3_stein_minibatch512_step_f32_gathered': lambda: stein_minibatch_case(3, 5000, 512, torch.float32, in_kernel=False),
    'c3_spd3_stein_minibatch512_step_f32_gathered_graph': lambda: stein_minibatch_case(3, 5000, 512, torch.float32, graph=True, in_kernel=False),
    'c1_tree40_euclidean10_f64': lambda: pdist_case(M.Euclidean(10), 40, torch.float64),
    'c2_facebook_lorentz11_f32_gram': lambda: pdist_case(M.Lorentz(11), 4039, torch.float32),
    'c2_facebook_lorentz11_f32_valu': lambda: pdist_case(_valu(M.Lorentz(11)), 4039, torch.float32),
    'c2_facebook_lorentz11_f64_gram': lambda: pdist_case(M.Lorentz(11), 4039, torch.float64),
    'c2_facebook_lorentz11_f64_valu': lambda: pdist_case(_valu(M.Lorentz(11)), 4039, torch.float64),
    # the bit-deterministic mode of the vector manifolds (csrc/vec_det.hpp) beside its atomic twins: measure each pair in ONE run on
    # one box (profiles/vec_deterministic.md)
    'c2_facebook_lorentz11_f32_deterministic': lambda: pdist_case(M.Lorentz(11, deterministic=True), 4039, torch.float32),
    'c2_facebook_lorentz11_f64_deterministic': lambda: pdist_case(M.Lorentz(11, deterministic=True), 4039, torch.float64),
    'c2_facebook_lorentz11_step_f32_fused_graph_deterministic': lambda: step_case([M.Lorentz(11, deterministic=True)], 4039, torch.float32, fused=True, graph=True),
    'c2_facebook_lorentz11_step_f32': lambda: step_case([M.Lorentz(11)], 4039, torch.float32),
    'c2_facebook_lorentz11_step_f32_fused': lambda: step_case([M.Lorentz(11)], 4039, torch.float32, fused=True),
    'c2_facebook_lorentz11_step_f32_fused_graph': lambda: step_case([M.Lorentz(11)], 4039, torch.float32, fused=True, graph=True),
    'c3_grqc_spd3_n5000_f32': lambda: pdist_case(M.SymmetricPositiveDefinite(3), 5000, torch.float32),
    # the bit-deterministic mode (csrc/spd_det.hpp) beside its atomic twins: measure each pair in ONE run on one box
    # (profiles/spd_deterministic.md)
    'c3_grqc_spd3_n5000_f32_deterministic': lambda: pdist_case(M.SymmetricPositiveDefinite(3, deterministic=True), 5000, torch.float32),
    'c3_grqc_spd3_n4158_f32': lambda: pdist_case(M.SymmetricPositiveDefinite(3), 4158, torch.float32),
    'c3_grqc_spd3_n5000_f64': lambda: pdist_case(M.SymmetricPositiveDefinite(3), 5000, torch.float64),
    # "mid-training" spread: ||log X|| = 0.35 -> pair distances ~0.5 (targets are normalised to max 1)
    'c3_grqc_spd3_n5000_f32_mid': lambda: pdist_case(M.SymmetricPositiveDefinite(3), 5000, torch.float32, ir=0.35),
    'c3_grqc_spd3_n5000_f64_mid': lambda: pdist_case(M.SymmetricPositiveDefinite(3), 5000, torch.float64, ir=0.35),
    'c3_spd3_stein_n5000_f32': lambda: pdist_case(M.SymmetricPositiveDefinite(3, use_stein_div=True), 5000, torch.float32),
    'c3_spd2_n5000_f32': lambda: pdist_case(M.SymmetricPositiveDefinite(2), 5000, torch.float32),
    'c4_csphd_product_step_f32': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32),
    'c4_csphd_product_step_f32_fused': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, fused=True),
    'c4_csphd_product_step_f32_fused_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, fused=True, graph=True),
    'c4_csphd_product_step_f32_fused_graph_unroll4': lambda: unrolled_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, 4),
    'c2_facebook_lorentz11_step_f32_fused_graph_unroll4': lambda: unrolled_case([M.Lorentz(11)], 4039, torch.float32, 4),
    'c4_csphd_product_step_f32_perfactor': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, fused=True, pair_kernel=False),
    'c4_csphd_product_step_f32_perfactor_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, fused=True, graph=True, pair_kernel=False),
    'c4_csphd_product_step_f64_fused_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float64, fused=True, graph=True),
    'c4_product_n5000_step_f32_fused_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 5000, torch.float32, fused=True, graph=True),
    'c4_product_n5000_step_f32_perfactor_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 5000, torch.float32, fused=True, graph=True, pair_kernel=False),
    'c4_product_n2500_step_f32_fused_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 2500, torch.float32, fused=True, graph=True),
    'c4_product_n2500_step_f32_perfactor_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 2500, torch.float32, fused=True, graph=True, pair_kernel=False),
    'c4_csphd_product_step_f32_fused_radam_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, fused=True, graph=True, adam=True),
    'c3_spd3_step_n5000_f32_fused_radam_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, fused=True, graph=True, adam=True),
    'c3_spd3_step_n5000_f32_fused_radam': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, fused=True, adam=True),
    'c4_csphd_product_step_f32_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, graph=True),
    'c4_csphd_product_step_f64': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float64),
    'c5_wormnet_spd4_n2274_f32': lambda: pdist_case(M.SymmetricPositiveDefinite(4), 2274, torch.float32),
    'c5_wormnet_spd4_n2274_f32_deterministic': lambda: pdist_case(M.SymmetricPositiveDefinite(4, deterministic=True), 2274, torch.float32),
    'c5_wormnet_spd4_n16384_f32': lambda: pdist_case(M.SymmetricPositiveDefinite(4), 16384, torch.float32),
    'c3_spd3_step_n5000_f32': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32),
    'c3_spd3_step_n5000_f32_fused': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, fused=True),
    'c3_spd3_step_n5000_f32_fused_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, fused=True, graph=True),
    'c3_spd3_step_n5000_f32_fused_graph_deterministic': lambda: step_case([M.SymmetricPositiveDefinite(3, deterministic=True)], 5000, torch.float32, fused=True, graph=True),
    'c3_spd3_step_n5000_f32_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, graph=True),
    'c3_spd3_step_n5000_f32_native_graph': lambda: native_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32),
    'c3_spd3_step_n5000_f64_native_graph': lambda: native_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64),
    'c4_csphd_product_step_f32_native_graph': lambda: native_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32),
    'c2_facebook_lorentz11_step_f32_native_graph': lambda: native_case([M.Lorentz(11)], 4039, torch.float32),
    'c5_spd4_step_n16384_f32_native_graph': lambda: native_case([M.SymmetricPositiveDefinite(4)], 16384, torch.float32, loss='quotient'),
    'c5_spd4_step_n2274_f32_native_graph': lambda: native_case([M.SymmetricPositiveDefinite(4)], 2274, torch.float32, loss='quotient'),
    'c5_spd4_step_n2274_f32_fused': lambda: step_case([M.SymmetricPositiveDefinite(4)], 2274, torch.float32, fused=True),
    'c3_spd3_minibatch512_step_f32': lambda: minibatch_case([M.SymmetricPositiveDefinite(3)], 5000, 512, torch.float32),
    'c3_spd3_minibatch512_step_f32_graph': lambda: minibatch_case([M.SymmetricPositiveDefinite(3)], 5000, 512, torch.float32, graph=True),
    'c4_csphd_minibatch512_step_f32_graph': lambda: minibatch_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, 512, torch.float32, graph=True),
    'c4_csphd_minibatch512_step_f32_radam_graph': lambda: minibatch_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, 512, torch.float32, graph=True, adam=True),
    'c3_spd3_minibatch512_step_f32_radam_graph': lambda: minibatch_case([M.SymmetricPositiveDefinite(3)], 5000, 512, torch.float32, graph=True, adam=True),
    'c4_csphd_minibatch512_step_f32': lambda: minibatch_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, 512, torch.float32),
    'c2_lorentz11_minibatch512_step_f32': lambda: minibatch_case([M.Lorentz(11)], 4039, 512, torch.float32),
    # round 4: node minibatches inside the single factors' own pair kernels (SPD(4...9), vectors wider than 16)
    'c5_spd4_minibatch512_step_n16384_f32_graph': lambda: minibatch_case([M.SymmetricPositiveDefinite(4)], 16384, 512, torch.float32, graph=True),
    'c5_spd4_minibatch512_step_n16384_f32_native_graph': lambda: native_minibatch_case([M.SymmetricPositiveDefinite(4)], 16384, 512, torch.float32),
    'c5_spd4_minibatch512_step_n2274_f32_native_graph': lambda: native_minibatch_case([M.SymmetricPositiveDefinite(4)], 2274, 512, torch.float32),
    'c5_spd4_minibatch512_step_n2274_f32_radam_native_graph': lambda: native_minibatch_case([M.SymmetricPositiveDefinite(4)], 2274, 512, torch.float32, adam=True),
    'c3_spd3_minibatch512_step_f32_native_graph': lambda: native_minibatch_case([M.SymmetricPositiveDefinite(3)], 5000, 512, torch.float32),
    'spd6_minibatch512_step_n2274_f32_native_graph': lambda: native_minibatch_case([M.SymmetricPositiveDefinite(6)], 2274, 512, torch.float32),
    'lorentz24_minibatch512_step_n4039_f32_native_graph': lambda: native_minibatch_case([M.Lorentz(24)], 4039, 512, torch.float32),
    'sphere6_n5000_f32': lambda: pdist_case(M.Sphere(6), 5000, torch.float32),
    'euclidean10_n5000_f32': lambda: pdist_case(M.Euclidean(10), 5000, torch.float32),
    'sphere6_n5000_f32_deterministic': lambda: pdist_case(M.Sphere(6, deterministic=True), 5000, torch.float32),
    'euclidean10_n5000_f32_deterministic': lambda: pdist_case(M.Euclidean(10, deterministic=True), 5000, torch.float32),
    # Lorentz(24) at batch 512 of 4039, replayed: the index vector inside the pair kernel | `gather`: rows and targets gathered, the
    # full-batch kernel on them, the gradient rows scattered back — in either mode
    'lorentz24_minibatch512_step_n4039_f32_graph': lambda: minibatch_case([M.Lorentz(24)], 4039, 512, torch.float32, graph=True),
    'lorentz24_minibatch512_step_n4039_f32_graph_gather': lambda: minibatch_case([M.Lorentz(24)], 4039, 512, torch.float32, graph=True, gather=True),
    'lorentz24_minibatch512_step_n4039_f32_graph_deterministic': lambda: minibatch_case([M.Lorentz(24, deterministic=True)], 4039, 512, torch.float32, graph=True),
    'lorentz24_minibatch512_step_n4039_f32_graph_deterministic_gather': lambda: minibatch_case([M.Lorentz(24, deterministic=True)], 4039, 512, torch.float32, graph=True, gather=True),
    'grassmann52_n2000_f32': lambda: pdist_case(M.Grassmann(5, 2), 2000, torch.float32),
    # Grassmann training steps: per-factor objective (pdist forward, loss, pdist backward) | one pair kernel (mm_grass_pdist_loss);
    # the optimizer update is one launch in all of them (mm_mat_rsgd_step)
    'grassmann52_step_n2000_f32': lambda: step_case([M.Grassmann(5, 2)], 2000, torch.float32),
    'grassmann52_step_n2000_f32_fused': lambda: step_case([M.Grassmann(5, 2)], 2000, torch.float32, fused=True),
    'grassmann52_step_n2000_f32_fused_graph': lambda: step_case([M.Grassmann(5, 2)], 2000, torch.float32, fused=True, graph=True),
    'grassmann94_step_n2000_f32': lambda: step_case([M.Grassmann(9, 4)], 2000, torch.float32),
    'grassmann94_step_n2000_f32_fused': lambda: step_case([M.Grassmann(9, 4)], 2000, torch.float32, fused=True),
    'grassmann94_step_n2000_f32_fused_graph': lambda: step_case([M.Grassmann(9, 4)], 2000, torch.float32, fused=True, graph=True),
    # SO(3) (csrc/so.hip): pdist fwd + bwd; training steps with the retraction (the fused St(n, n) step kernel) on the fused objective,
    # and the same step with the objective in torch ops on the GPU (batched torch.linalg.svd over the gathered pairs) - the only
    # yardstick there is: the reference's own dist has no derivative
    'so3_n2000_f32': lambda: pdist_case(M.SpecialOrthogonal(3), 2000, torch.float32),
    'so3_step_n2000_f32': lambda: step_case([M.SpecialOrthogonal(3)], 2000, torch.float32, exact=False),
    'so3_step_n2000_f32_fused': lambda: step_case([M.SpecialOrthogonal(3)], 2000, torch.float32, fused=True, exact=False),
    'so3_step_n2000_f32_fused_graph': lambda: step_case([M.SpecialOrthogonal(3)], 2000, torch.float32, fused=True, graph=True, exact=False),
    'so3_step_n2000_f32_torch_ops': lambda: step_case([M.SpecialOrthogonal(3)], 2000, torch.float32, exact=False,
                                                      torch_ops=_SoPdistTorchOps.apply, iters=3, warm=1),
    # SO(3) node minibatches with Adam (retraction); `_gathered`: the route before the SUB kernels of csrc/so.hip; `_sne`: the pair-vector route
    'so3_minibatch512_radam_step_n2000_f32': lambda: so_minibatch_case(3, 2000, 512, torch.float32),
    'so3_minibatch512_radam_step_n2000_f32_graph': lambda: so_minibatch_case(3, 2000, 512, torch.float32, graph=True),
    'so3_minibatch512_radam_step_n2000_f32_gathered': lambda: so_minibatch_case(3, 2000, 512, torch.float32, in_kernel=False),
    'so3_minibatch512_radam_step_n2000_f32_gathered_graph': lambda: so_minibatch_case(3, 2000, 512, torch.float32, graph=True, in_kernel=False),
    'so3_minibatch512_sne_radam_step_n2000_f32': lambda: so_minibatch_case(3, 2000, 512, torch.float32, sne=True),
    'so3_minibatch512_sne_radam_step_n2000_f32_graph': lambda: so_minibatch_case(3, 2000, 512, torch.float32, graph=True, sne=True),
    'so3_minibatch512_sne_radam_step_n2000_f32_gathered': lambda: so_minibatch_case(3, 2000, 512, torch.float32, in_kernel=False, sne=True),
    'so3_minibatch512_sne_radam_step_n2000_f32_gathered_graph': lambda: so_minibatch_case(3, 2000, 512, torch.float32, graph=True, in_kernel=False, sne=True),
    # node minibatches with Adam, the reference grid's recipe; `_gathered`: the route before mm_grass_pdist_loss_subset / mm_mat_radam_step
    'grassmann52_minibatch512_radam_step_n2000_f32': lambda: grass_minibatch_case(5, 2, 2000, 512, torch.float32),
    'grassmann52_minibatch512_radam_step_n2000_f32_graph': lambda: grass_minibatch_case(5, 2, 2000, 512, torch.float32, graph=True),
    'grassmann52_minibatch512_radam_step_n2000_f32_gathered': lambda: grass_minibatch_case(5, 2, 2000, 512, torch.float32, in_kernel=False),
    'grassmann52_minibatch512_radam_step_n2000_f32_gathered_graph': lambda: grass_minibatch_case(5, 2, 2000, 512, torch.float32, graph=True, in_kernel=False),
    'grassmann94_minibatch512_radam_step_n2000_f32': lambda: grass_minibatch_case(9, 4, 2000, 512, torch.float32),
    'grassmann94_minibatch512_radam_step_n2000_f32_graph': lambda: grass_minibatch_case(9, 4, 2000, 512, torch.float32, graph=True),
    'grassmann94_minibatch512_radam_step_n2000_f32_gathered': lambda: grass_minibatch_case(9, 4, 2000, 512, torch.float32, in_kernel=False),
    'grassmann94_minibatch512_radam_step_n2000_f32_gathered_graph': lambda: grass_minibatch_case(9, 4, 2000, 512, torch.float32, graph=True, in_kernel=False),
    # stochastic-neighbour KL loss (StochasticNeighborLoss: pdist forward, mm_sne_kl_loss, pdist backward) | its torch-op form
    'c3_spd3_sne_incl_step_n5000_f32': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sne='incl'),
    'c3_spd3_sne_incl_step_n5000_f32_torchops': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sne='incl', native=False),
    'c3_spd3_sne_incl_step_n5000_f32_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sne='incl', graph=True),
    'c3_spd3_sne_excl_step_n5000_f32': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sne='excl'),
    'c3_spd3_sne_excl_step_n5000_f32_torchops': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sne='excl', native=False),
    'c3_spd3_sne_excl_step_n5000_f32_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sne='excl', graph=True),
    # constant curvature with learnable curvature (csrc/stereo.hip); the Lorentz rows of the same n, m and dtype are the yardstick
    'stereo10_n4039_f32': lambda: stereo_pdist_case(10, 4039, torch.float32),
    'stereo10_n4039_f64': lambda: stereo_pdist_case(10, 4039, torch.float64),
    'lorentz10_n4039_f32_valu': lambda: pdist_case(_valu(M.Lorentz(10)), 4039, torch.float32),
    'lorentz10_n4039_f64_valu': lambda: pdist_case(_valu(M.Lorentz(10)), 4039, torch.float64),
    'stereo10_step_n4039_f32': lambda: stereo_step_case([10], 4039, torch.float32),
    'stereo10_step_n4039_f32_graph': lambda: stereo_step_case([10], 4039, torch.float32, graph=True),
    'lorentz10_step_n4039_f32': lambda: step_case([M.Lorentz(10)], 4039, torch.float32),
    'stereo5_n1025_f32': lambda: stereo_pdist_case(5, 1025, torch.float32),
    'lorentz5_n1025_f32_valu': lambda: pdist_case(_valu(M.Lorentz(5)), 1025, torch.float32),
    'stereo5x5_step_n1025_f32': lambda: stereo_step_case([5, 5], 1025, torch.float32),
    'stereo5x5_step_n1025_f32_graph': lambda: stereo_step_case([5, 5], 1025, torch.float32, graph=True),
    # the same steps through the fused multi-factor objective kernel (mm_stereo_product_loss), and their per-factor twins
    'stereo5x5_step_n1025_f32_fused': lambda: stereo_step_case([5, 5], 1025, torch.float32, fused=True),
    'stereo5x5_step_n1025_f32_fused_graph': lambda: stereo_step_case([5, 5], 1025, torch.float32, fused=True, graph=True),
    'stereo2x8_step_n4039_f32': lambda: stereo_step_case([2] * 8, 4039, torch.float32),
    'stereo2x8_step_n4039_f32_fused': lambda: stereo_step_case([2] * 8, 4039, torch.float32, fused=True),
    'stereo5x5_quotient_step_n1025_f32': lambda: stereo_step_case([5, 5], 1025, torch.float32, quotient=True),
    'stereo5x5_quotient_step_n1025_f32_fused': lambda: stereo_step_case([5, 5], 1025, torch.float32, fused=True, quotient=True),
    'lorentz5x5_step_n1025_f32': lambda: step_case([M.Lorentz(5), M.Lorentz(5)], 1025, torch.float32),
    # node minibatches with RiemannianAdam, the regime of the reference's product grid: the index vector inside the pair kernel and
    # the fused Adam step, and their twins on the route before them (`_gathered`: take_rows + Adam composed from the maps)
    'stereo5x5_minibatch512_radam_step_n4039_f32': lambda: stereo_minibatch_case([5, 5], 4039, 512, torch.float32),
    'stereo5x5_minibatch512_radam_step_n4039_f32_graph': lambda: stereo_minibatch_case([5, 5], 4039, 512, torch.float32, graph=True),
    'stereo5x5_minibatch512_radam_step_n4039_f32_gathered': lambda: stereo_minibatch_case([5, 5], 4039, 512, torch.float32, in_kernel=False),
    'stereo5x5_minibatch512_radam_step_n4039_f32_gathered_graph': lambda: stereo_minibatch_case([5, 5], 4039, 512, torch.float32, graph=True, in_kernel=False),
    'stereo2x8_minibatch4096_radam_step_n8192_f32': lambda: stereo_minibatch_case([2] * 8, 8192, 4096, torch.float32),
    'stereo2x8_minibatch4096_radam_step_n8192_f32_graph': lambda: stereo_minibatch_case([2] * 8, 8192, 4096, torch.float32, graph=True),
    'stereo2x8_minibatch4096_radam_step_n8192_f32_gathered': lambda: stereo_minibatch_case([2] * 8, 8192, 4096, torch.float32, in_kernel=False),
    'stereo2x8_minibatch4096_radam_step_n8192_f32_gathered_graph': lambda: stereo_minibatch_case([2] * 8, 8192, 4096, torch.float32, graph=True, in_kernel=False),
    'c4_csphd_sne_incl_step_f32_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, sne='incl', graph=True),
    # spanning-tree KL loss (StochasticTreeLoss: pdist forward over a 512-node index batch, mm_sst_kl_loss, pdist backward) | its torch-op form
    'c3_spd3_sst_incl_minibatch512_step_n5000_f32': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sst='incl', batch=512),
    'c3_spd3_sst_incl_minibatch512_step_n5000_f32_torchops': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sst='incl', batch=512, native=False),
    'c3_spd3_sst_incl_minibatch512_step_n5000_f32_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sst='incl', batch=512, graph=True),
    'c3_spd3_sst_incl_minibatch512_step_n5000_f64': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64, sst='incl', batch=512),
    'c3_spd3_sst_incl_minibatch512_step_n5000_f64_torchops': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64, sst='incl', batch=512, native=False),
    'c3_spd3_sst_incl_minibatch512_step_n5000_f64_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64, sst='incl', batch=512, graph=True),
    'c3_spd3_sst_excl_minibatch512_step_n5000_f32': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sst='excl', batch=512),
    'c3_spd3_sst_excl_minibatch512_step_n5000_f32_torchops': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sst='excl', batch=512, native=False),
    'c3_spd3_sst_excl_minibatch512_step_n5000_f32_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float32, sst='excl', batch=512, graph=True),
    'c3_spd3_sst_excl_minibatch512_step_n5000_f64': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64, sst='excl', batch=512),
    'c3_spd3_sst_excl_minibatch512_step_n5000_f64_torchops': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64, sst='excl', batch=512, native=False),
    'c3_spd3_sst_excl_minibatch512_step_n5000_f64_graph': lambda: step_case([M.SymmetricPositiveDefinite(3)], 5000, torch.float64, sst='excl', batch=512, graph=True),
    'c4_csphd_sst_incl_step_f32_graph': lambda: step_case([M.Lorentz(6), M.Sphere(6), M.SymmetricPositiveDefinite(2)], 1025, torch.float32, sst='incl', graph=True),
}


def unrolled_case(mans, n, dtype, unroll):
    """full-batch fused training step, `unroll` steps per recorded graph (GraphedTrainStep(unroll=)); time per STEP"""
    from graphembed.graphed import GraphedTrainStep
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, mans)
    finally:
        torch.set_default_dtype(torch.float32)
    P = n * (n - 1) // 2
    target = torch.rand(P, dtype=dtype, device='cuda') * 0.99 + 0.01
    fn = StressLoss()
    opts = [RiemannianSGD(list(emb.xs), lr=1e-3, exact=True, max_grad_norm=20),
            RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)]
    step = GraphedTrainStep(lambda: emb.fused_objective(fn, target, None), opts, warmup=2, unroll=unroll).capture()
    t = timeit(step) / unroll
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def minibatch_case(mans, n, bs, dtype, graph=False, adam=False, gather=False):
    """node-minibatch training step as train.py:198-222 runs it (batch_size=512 in the paper grid): targets of the
    induced sub-graph from the dense matrix, embedding rows gathered, fused loss, scatter-add backward, RSGD; `gather`: keep
    the batch out of the pair kernels' index-vector forms (rows and targets gathered, gradient rows scattered back)"""
    from graphembed.data import GraphDataset
    from graphembed.modules import BatchedObjective
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, mans)
            emb.pair_kernel = not gather
            ds = GraphDataset(torch.rand(n * (n - 1) // 2) * 0.99 + 0.01)
    finally:
        torch.set_default_dtype(torch.float32)
    obj = BatchedObjective(StressLoss(), ds, emb)
    if adam:
        opt = RiemannianAdam(list(emb.xs), lr=1e-3, exact=True, max_grad_norm=20)
        opt_s = RiemannianAdam(list(emb.scales), lr=1e-4, max_grad_norm=500)
    else:
        opt = RiemannianSGD(list(emb.xs), lr=1e-3, exact=True, max_grad_norm=20)
        opt_s = RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)
    perm = torch.randperm(n, device='cuda')
    state = {'i': 0}

    def step():
        i = state['i']
        idx = perm[i:i + bs]
        state['i'] = (i + bs) % (n - bs)
        opt.zero_grad()
        opt_s.zero_grad()
        obj(idx).backward()
        opt.step()
        opt_s.step()
    if graph:  # static index buffer, refreshed in place before every replay
        from graphembed.graphed import GraphedTrainStep
        idx_static = perm[:bs].clone()
        gstep = GraphedTrainStep(lambda: obj(idx_static), [opt, opt_s]).capture()

        def step():  # noqa: F811
            i = state['i']
            idx_static.copy_(perm[i:i + bs])
            state['i'] = (i + bs) % (n - bs)
            gstep()
    t = timeit(step, iters=50)
    P = bs * (bs - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def native_minibatch_case(mans, n, bs, dtype, adam=False):
    """node-minibatch training step through ONE C-ABI call (mm_train_step_run with batch_idx), replayed as a hipGraph with the
    index vector refreshed in place: for a single SPD(d <= 5) factor two launches per step — the pair kernel over the batch (index
    vector inside) and the per-point finalize / optimizer / tables kernel over all n points (the launch count is read off the rocprofv3 kernel trace of this case: tools/gpu_r04_b.sh)."""
    from graphembed.data import GraphDataset
    from graphembed.native_step import NativeTrainStep
    torch.manual_seed(0)
    torch.set_default_dtype(dtype)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, mans)
            ds = GraphDataset(torch.rand(n * (n - 1) // 2) * 0.99 + 0.01)
    finally:
        torch.set_default_dtype(torch.float32)
    if adam:
        opts = [RiemannianAdam(list(emb.xs), lr=1e-3, exact=True, max_grad_norm=20), RiemannianAdam(list(emb.scales), lr=1e-4, max_grad_norm=500)]
    else:
        opts = [RiemannianSGD(list(emb.xs), lr=1e-3, exact=True, max_grad_norm=20), RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)]
    step = NativeTrainStep(emb, StressLoss(), None, opts, dense=ds.pdists)
    perm = torch.randperm(n, device='cuda')
    idx_static = perm[:bs].clone()
    for _ in range(3):
        step(indices=idx_static)            # (the second step on: the tables of the new points are the step kernel's own)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(indices=idx_static)
    torch.cuda.current_stream().wait_stream(side)
    state = {'i': 0}

    def run():
        i = state['i']
        idx_static.copy_(perm[i:i + bs])
        state['i'] = (i + bs) % (n - bs)
        g.replay()
    t = timeit(run, iters=50)
    P = bs * (bs - 1) // 2
    return {'n': n, 'pairs': P, 'dtype': str(dtype).split('.')[-1], 'step_us': t, 'pairs_per_s': P / (t * 1e-6)}


def _valu(man):
    man.use_gram = False
    return man


def host_calibration():
    """How fast THIS box's host dispatches work — the yardstick for every eager (non-graph) row, which is host-bound: the same
    tree measured 1.3 - 1.6 x apart in its eager rows on two boxes while every graph-replayed row agreed to 3 % (round 5's
    table against round 4's; advisor, round 5).  `launch_us`: a trivial in-place torch kernel enqueued in a loop (framework
    dispatch + hipLaunchKernel, no synchronisation inside); `cabi_us`: an argument-check-only C-ABI call through ctypes;
    `python_us`: 1000 iterations of a pure-python arithmetic loop."""
    import time
    from graphembed import _backend as B
    t = torch.zeros(64, device='cuda')
    for _ in range(200):
        t.add_(1.0)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(2000):
            t.add_(1.0)
        best = min(best, (time.perf_counter() - t0) / 2000 * 1e6)
        torch.cuda.synchronize()
    fn = B.lib().raw('mm_pair_offset')
    t0 = time.perf_counter()
    for _ in range(20000):
        fn(5000, 17)
    cabi = (time.perf_counter() - t0) / 20000 * 1e6
    t0 = time.perf_counter()
    acc = 0
    for i in range(200000):
        acc += i * i % 7
    py = (time.perf_counter() - t0) / 200 * 1e6
    return {'launch_us': best, 'cabi_us': cabi, 'python_us': py, 'host_cpus': os.cpu_count()}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    out = {'_host': host_calibration()}
    for name, fn in CASES.items():
        if a.only and a.only not in name:
            continue
        out[name] = fn()
    print(json.dumps(out, indent=1))
