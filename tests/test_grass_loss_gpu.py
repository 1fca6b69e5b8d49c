"""The fused Grassmann objective (mm_grass_pdist_loss through Grassmann.pdist_loss / ManifoldEmbedding.fused_objective)
against the fp64 oracle of oracle/ref_port.py, with the measured tolerance rule of tests/grass_cases.py: the route the
package took before (compute_dists -> objective -> autograd, on the GPU, same inputs) is the yardstick.  That yardstick shares
the device code under test; the absolute check of both routes is tests/test_mat_oracle_gpu.py (pdist forward / backward at all 26
shapes of mat_cases.SHAPES, the fused objective at (2,1) (3,3) (4,4) (6,4) (7,3) (8,4) (9,1), fp32 and fp64)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grass_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

# n: wavefront (64), row-tile (16) and multi-block boundaries; (3,2) and (4,3) have a principal angle of exactly 0
SHAPES = [(N, p, n) for (N, p) in ((5, 2), (6, 3)) for n in (2, 3, 64, 65, 129, 257)] + \
         [(N, p, n) for (N, p) in ((4, 1), (9, 4), (3, 2), (4, 3)) for n in (65, 257)]


def _unfused(emb, fn, kw, target, i=None):
    """loss, grad_x, grad_scale of compute_dists -> objective -> autograd."""
    params = [emb.xs[0], emb.scales[0]]
    loss = fn(target, emb.compute_dists(i), **kw)
    gx, gs = torch.autograd.grad(loss, params)
    return loss.detach(), gx, gs


def _fused(emb, fn, kw, target, i=None, rows=None):
    params = [emb.xs[0], emb.scales[0]]
    loss = emb.fused_objective(fn, target, i, rows=rows, **kw)
    assert loss is not None
    gx, gs = torch.autograd.grad(loss, params)
    return loss.detach(), gx, gs


@pytest.mark.parametrize('loss_name', ['stress', 'quotient'])
@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p,n', SHAPES)
def test_fused_objective_vs_fp64_oracle(N, p, n, dname, loss_name):
    dt = gc.DT[dname]
    fn, kw = gc.objective(loss_name)
    failures = []
    for regime in gc.REGIMES[dname]:
        want = gc.objective_oracle(regime, n, N, p, loss_name)
        emb = gc.embedding(n, N, p, dt, gc.frames(regime, n, N, p))
        target = gc.targets(n).to(dt).cuda()
        old = _unfused(emb, fn, kw, target)
        new = _fused(emb, fn, kw, target)
        tag = f'objective {N}x{p} n={n} {dname} {loss_name} {regime}'
        for what, o, g, w in zip(('loss', 'grad_x', 'grad_scale'), old, new, want):
            assert torch.isfinite(g).all(), (tag, what)
            gc.check(tag, what, o, g, w, dt, failures)
    assert not failures, '\n'.join(failures)


def test_cases_cover_every_form_of_the_table():
    """mm_grass_pdist_loss_form over every supported (dtype, N, p): the shapes above reach each form the table holds."""
    from graphembed import _backend as B
    form = B.lib().raw('mm_grass_pdist_loss_form')
    table = {(d, N, p): form(d, N, p) for d in (0, 1) for N in range(1, 10) for p in range(1, min(N, 4) + 1)}
    assert set(table.values()) <= {0, 1}, table
    hit = {table[(d, N, p)] for d in (0, 1) for (N, p, _) in SHAPES}
    assert hit == set(table.values()), (hit, {k: v for k, v in table.items() if v == 0})


@pytest.mark.parametrize('loss_name', ['stress', 'quotient'])
@pytest.mark.parametrize('N,p', [(5, 2), (9, 4)])
def test_row_shards_sum_to_the_full_call(N, p, loss_name):
    n, dt = 257, torch.float64
    fn, kw = gc.objective(loss_name)
    emb = gc.embedding(n, N, p, dt, gc.frames('uniform', n, N, p))
    target = gc.targets(n).to(dt).cuda()
    full = _fused(emb, fn, kw, target)
    off = lambda r: r * (2 * n - r - 1) // 2   # noqa: E731
    parts = [_fused(emb, fn, kw, target[off(rb):off(re)], rows=(rb, re)) for rb, re in ((0, 1), (1, 70), (70, 257), (70, 70))]
    empty = parts[-1]
    assert float(empty[0]) == 0.0 and float(empty[2]) == 0.0 and not empty[1].any()
    for k, what in enumerate(('loss', 'grad_x', 'grad_scale')):
        total = sum(part[k] for part in parts)
        floor = 64 * gc.eps_of(dt) * float(full[k].abs().max())
        err = float((total - full[k]).abs().max())
        print(f'shards {N}x{p} {loss_name} {what}: err {err:.3e} floor {floor:.3e}')
        assert err <= floor, (what, err, floor)


def test_one_objective_is_one_pair_kernel_call():
    """One fused_objective of a Grassmann embedding = one mm_grass_pdist_loss: no forward / backward pdist kernels, no
    product-loss kernel, and no tensor of pair length is written (the peak of device memory stays below one pair vector)."""
    N, p, n, dt = 5, 2, 513, torch.float32
    fn, kw = gc.objective('quotient')
    emb = gc.embedding(n, N, p, dt, gc.frames('uniform', n, N, p))
    target = gc.targets(n).to(dt).cuda()
    _fused(emb, fn, kw, target)   # (warm: library handles, the allocator's pools)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with gc.CallSpy() as spy:
        loss = emb.fused_objective(fn, target, None, **kw)
        loss.backward()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    assert spy.calls.count('mm_grass_pdist_loss') == 1, spy.calls
    assert not {'mm_grass_pdist_fwd', 'mm_grass_pdist_bwd', 'mm_product_loss'} & set(spy.calls), spy.calls
    assert grew < target.numel() * target.element_size(), (grew, target.numel() * target.element_size())
    assert emb.xs[0].grad is not None and emb.scales[0].grad is not None


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_node_minibatch(dname):
    """64 distinct nodes of 257 through fused_objective: the oracle on the gathered points; rows outside the batch get zeros."""
    N, p, n, bs = 5, 2, 257, 64
    dt = gc.DT[dname]
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(11))[:bs]
    x = gc.frames('uniform', n, N, p)
    target64 = gc.targets(bs)
    failures = []
    for loss_name in ('stress', 'quotient'):
        fn, kw = gc.objective(loss_name)
        xs = x[idx].clone().requires_grad_(True)
        s = torch.tensor(gc.SCALE_RAW, dtype=torch.float64, requires_grad=True)
        wl = gc.oracle_loss(loss_name, target64, gc.ref.compute_dists([gc.ref.Grassmann(N, p)], [xs], [s]))
        wgx_b, wgs = torch.autograd.grad(wl, [xs, s])
        wgx = torch.zeros_like(x).index_add_(0, idx, wgx_b)
        emb = gc.embedding(n, N, p, dt, x)
        target = target64.to(dt).cuda()
        old = _unfused(emb, fn, kw, target, idx)
        with gc.CallSpy() as spy:
            new = _fused(emb, fn, kw, target, idx)
        assert spy.calls.count('mm_grass_pdist_loss') == 1, spy.calls
        outside = torch.ones(n, dtype=torch.bool)
        outside[idx] = False
        assert not new[1][outside.cuda()].any()
        tag = f'minibatch {N}x{p} {dname} {loss_name}'
        for what, o, g, w in zip(('loss', 'grad_x', 'grad_scale'), old, new, (wl.detach(), wgx, wgs)):
            gc.check(tag, what, o, g, w, dt, failures)
    assert not failures, '\n'.join(failures)
