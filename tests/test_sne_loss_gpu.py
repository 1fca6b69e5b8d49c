"""The stochastic-neighbour KL kernels (csrc/sne_loss.hip, mm_sne_kl_loss) on the GPU: against the long-double oracle of
tests/sne_cases.py under the project's tolerance rule (e_kernel <= 2 e_ref + 64 eps scale, e_ref the recorded reference's own
error in the same dtype), bitwise reproducibility, the C ABI without a gradient buffer, and end to end through
ManifoldEmbedding + BatchedObjective and a captured training step.

Measured on the MI355X, largest e_kernel / max(e_ref, floor) per regime (the rule allows 2 where e_ref dominates, 1 at the floor;
fp32 loss, gradient | fp64 loss, gradient): near 0.11, 0.06 | 0.09, 0.05; mid 0.02, 0.07 | 0.03, 0.07; far 0.09, 0.16 | 0.18, 0.12;
outlier 0.07, 0.35 | 0.23, 0.17 (profiles/sne_loss.md)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sne_cases as S  # noqa: E402
import step_cases as sc  # noqa: E402
from grass_cases import CallSpy  # noqa: E402
from oracle import ref_port as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
BIG = 1025   # 17 blocks of 64 nodes, the last one ragged


def _inputs(n, regime, dname):
    g, m = S.inputs(n, regime)
    return (torch.from_numpy(g.astype(np.float64)).to(device='cuda', dtype=DT[dname]),
            torch.from_numpy(m).to(device='cuda', dtype=DT[dname]))


def _kernel(n, regime, mode, dname):
    """(loss, grad) of the kernel route as numpy arrays."""
    from graphembed.objectives import StochasticNeighborLoss
    g, m = _inputs(n, regime, dname)
    m.requires_grad_()
    loss = StochasticNeighborLoss(inclusive=mode == 'incl')(g, m, alpha=S.ALPHA)
    assert loss.dtype == DT[dname] and loss.is_cuda and loss.dim() == 0
    gr, = torch.autograd.grad(loss, m)
    return loss.detach().cpu().numpy(), gr.cpu().numpy()


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('n,regime', S.CASES, ids=[f'n{n}-{r}' for n, r in S.CASES])
def test_kernels_against_the_oracle(n, regime, dname):
    failures = []
    for mode in S.MODES:
        loss, grad = _kernel(n, regime, mode, dname)
        S.check(n, regime, mode, dname, 'loss', loss, failures)     # (a value that is not finite fails the check)
        S.check(n, regime, mode, dname, 'grad', grad, failures)
    S.print_ratios()
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('regime', ['mid', 'outlier'])
def test_kernels_against_the_oracle_over_many_blocks(regime, dname):
    """n = 1025 has no recorded reference: it is held to the largest recorded e_ref / scale of its regime and mode."""
    failures = []
    for mode in S.MODES:
        loss, grad = _kernel(BIG, regime, mode, dname)
        S.check(BIG, regime, mode, dname, 'loss', loss, failures)
        S.check(BIG, regime, mode, dname, 'grad', grad, failures)
    S.print_ratios()
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('mode', S.MODES)
def test_two_nodes(mode, dname):
    """One pair: loss and gradient are 0 up to 4 eps max|theta|; fewer than two nodes: exactly 0 and no gradient entry."""
    from graphembed.objectives import StochasticNeighborLoss
    fn = StochasticNeighborLoss(inclusive=mode == 'incl')
    dt = DT[dname]
    g = torch.tensor([3.0], dtype=dt, device='cuda')
    m = torch.tensor([2.7], dtype=dt, device='cuda', requires_grad=True)
    loss = fn(g, m, alpha=S.ALPHA)
    gr, = torch.autograd.grad(loss, m)
    bound = 4 * S.EPS[dname] * max(S.ALPHA * 3.0, 2.7)
    print(float(loss), float(gr), bound)
    assert abs(float(loss)) <= bound and abs(float(gr)) <= bound
    e = torch.empty(0, dtype=dt, device='cuda', requires_grad=True)
    loss = fn(torch.empty(0, dtype=dt, device='cuda'), e, alpha=S.ALPHA)
    gr, = torch.autograd.grad(loss, e)
    assert float(loss) == 0.0 and gr.numel() == 0


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('n,regime', [(257, 'mid'), (BIG, 'outlier')])
def test_two_calls_give_the_same_bits(n, regime, dname):
    for mode in S.MODES:
        l1, g1 = _kernel(n, regime, mode, dname)
        l2, g2 = _kernel(n, regime, mode, dname)
        assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes(), (mode, float(l1), float(l2))


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_c_abi_without_a_gradient_buffer(dname):
    from graphembed import _backend as B
    lib = B.lib()
    n = 129
    g, m = _inputs(n, 'mid', dname)
    dt = B.dtype_code(m)
    ws = torch.empty(lib.raw('mm_sne_kl_ws_bytes')(dt, n), dtype=torch.uint8, device='cuda')
    for mode in (B.SNE_INCLUSIVE, B.SNE_EXCLUSIVE):
        out = torch.full((2, ), float('nan'), dtype=m.dtype, device='cuda')
        grad = torch.empty_like(m)
        ws.fill_(0xff)   # (the workspace needs no clearing)
        lib.call('mm_sne_kl_loss', dt, mode, B.ptr(g), B.ptr(m), n, S.ALPHA, B.ptr(grad), B.ptr(out[0:]), B.ptr(ws), B.stream_of(m))
        ws.fill_(0x00)
        lib.call('mm_sne_kl_loss', dt, mode, B.ptr(g), B.ptr(m), n, S.ALPHA, None, B.ptr(out[1:]), B.ptr(ws), B.stream_of(m))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.isfinite(o).all() and o[0:1].tobytes() == o[1:2].tobytes(), o
    # fewer than two nodes: MM_OK, a zero loss, nothing else touched
    out = torch.full((1, ), float('nan'), dtype=m.dtype, device='cuda')
    for k in (0, 1):
        assert lib.raw('mm_sne_kl_loss')(dt, 0, None, None, k, S.ALPHA, None, ctypes.c_void_p(out.data_ptr()), None,
                                         B.stream_of(m)) == 0
        assert float(out) == 0.0
        out.fill_(float('nan'))


# ------------------------------------------------------------------------------------------------------------- end to end
def _embedding(factors, n, dname, seed):
    """(embedding on the GPU, its initial points in fp64 on the CPU, raw scales)."""
    from graphembed import manifolds as M
    from graphembed.modules import ManifoldEmbedding
    mk = {'spd': M.SymmetricPositiveDefinite, 'lorentz': M.Lorentz, 'sphere': M.Sphere, 'euclidean': M.Euclidean}
    gen = torch.Generator().manual_seed(seed)
    xs = [sc.points(f, n, 'perturb', 0.3, gen, dname) for f in factors]
    scales = [float(np.float32(v)) for v in [0.5, 0.3, 0.7][:len(factors)]]
    torch.set_default_dtype(DT[dname])
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, [mk[k](d) for k, d in factors])
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for p, x in zip(emb.xs, xs):
            p.copy_(torch.from_numpy(x).to(device='cuda', dtype=DT[dname]))
        for p, s in zip(emb.scales, scales):
            p.fill_(s)
    return emb, xs, scales


def _dataset(n, dname, seed):
    from graphembed.data import GraphDataset
    gen = torch.Generator().manual_seed(seed)
    hops = torch.randint(1, 7, (n * (n - 1) // 2, ), generator=gen).to(DT[dname])
    return GraphDataset(hops.cuda())


def _expected(factors, xs, scales, gd, idx, inclusive, alpha):
    """Loss, point gradients (dense: zero rows outside a minibatch) and scale gradients of the torch-op form in fp64 on the CPU
    over oracle.ref_port distances."""
    from graphembed.objectives import StochasticNeighborLoss
    from oracle import step as ostep
    mans = [ostep.manifold(f) for f in factors]
    xt = [torch.from_numpy(x).clone().requires_grad_() for x in xs]
    st = [torch.tensor(s, dtype=torch.float64, requires_grad=True) for s in scales]
    md = ref.compute_dists(mans, xt, st, idx)
    loss = StochasticNeighborLoss(inclusive=inclusive, native=False)(gd, md, alpha=alpha)
    grads = torch.autograd.grad(loss, xt + st)
    gx = [ref.sym(g) if f[0] == 'spd' else g for f, g in zip(factors, grads[:len(xt)])]
    return loss.detach(), gx, grads[len(xt):]


def _compare(factors, dname, loss, emb, want):
    wl, wgx, wgs = want
    tol = sc.TOL
    el = abs(float(loss) - float(wl))
    print(f'loss {float(loss):.9g} want {float(wl):.9g} err {el:.3e} allowed {tol["loss"][dname] * abs(float(wl)):.3e}')
    assert el <= tol['loss'][dname] * abs(float(wl))
    for f, p, w in zip(factors, emb.xs, wgx):
        key = 'grad_spd' if f[0] == 'spd' else 'grad_vec'
        e = float((p.grad.double().cpu() - w).abs().max())
        allowed = tol[key][dname] * float(w.abs().max())
        print(f'grad/{f[0]}{f[1]} err {e:.3e} allowed {allowed:.3e}')
        assert e <= allowed, (f, e, allowed)
    for f, p, w in zip(factors, emb.scales, wgs):
        e = abs(float(p.grad) - float(w))
        allowed = tol['scale_grad'][dname] * max(abs(float(w)), 1e-3 * abs(float(wl)))
        print(f'scale_grad/{f[0]}{f[1]} err {e:.3e} allowed {allowed:.3e}')
        assert e <= allowed, (f, e, allowed)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('inclusive', [True, False])
def test_spd3_full_batch_through_the_batched_objective(inclusive, dname):
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StochasticNeighborLoss
    factors, n, alpha = [('spd', 3)], 65, 1.3
    emb, xs, scales = _embedding(factors, n, dname, seed=11)
    ds = _dataset(n, dname, seed=12)
    fn = StochasticNeighborLoss(inclusive=inclusive)
    assert emb.fused_objective(fn, ds[None], None, epoch=0, alpha=alpha) is None   # no fused_spec: the last line of BatchedObjective
    with CallSpy() as spy:
        loss = BatchedObjective(fn, ds, emb)(None, epoch=0, alpha=alpha)
        loss.backward()
    assert spy.calls.count('mm_sne_kl_loss') == 1, spy.calls
    _compare(factors, dname, loss, emb, _expected(factors, xs, scales, ds.condensed.double().cpu(), None, inclusive, alpha))


@pytest.mark.parametrize('inclusive', [True, False])
def test_product_node_minibatch_through_the_batched_objective(inclusive):
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StochasticNeighborLoss
    factors, n, alpha, dname = sc.CSPHD, 65, 0.9, 'f32'
    emb, xs, scales = _embedding(factors, n, dname, seed=21)
    ds = _dataset(n, dname, seed=22)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(23))[:33]
    with CallSpy() as spy:
        loss = BatchedObjective(StochasticNeighborLoss(inclusive=inclusive), ds, emb)(idx, epoch=0, alpha=alpha)
        loss.backward()
    assert spy.calls.count('mm_sne_kl_loss') == 1, spy.calls
    dense = ds.pdists.double().cpu()
    a, b = np.triu_indices(idx.numel(), 1)
    gd = dense[idx[a], idx[b]]
    _compare(factors, dname, loss, emb, _expected(factors, xs, scales, gd, idx, inclusive, alpha))


def test_captured_training_step_equals_eager_steps():
    """GraphedTrainStep over the SPD(3) step with RiemannianSGD: 3 warm-up steps + 5 replays against 8 eager steps."""
    from graphembed.graphed import GraphedTrainStep
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StochasticNeighborLoss
    from graphembed.optim import RiemannianSGD
    factors, n, alpha, dname = [('spd', 3)], 65, 1.3, 'f32'
    ds = _dataset(n, dname, seed=32)
    runs = []
    for graphed in (False, True):
        emb, xs, _ = _embedding(factors, n, dname, seed=31)
        obj = BatchedObjective(StochasticNeighborLoss(inclusive=True), ds, emb)
        opts = [RiemannianSGD(list(emb.xs), lr=0.05, max_grad_norm=None, exact=True),
                RiemannianSGD(list(emb.scales), lr=0.01, max_grad_norm=None)]
        step = GraphedTrainStep(lambda: obj(None, epoch=0, alpha=alpha), opts, warmup=3)
        if graphed:
            step.capture()
            losses = [float(v) for v in step.warmup_losses] + [float(step()) for _ in range(5)]
        else:
            losses = [float(step._eager_step()) for _ in range(8)]
        torch.cuda.synchronize()
        runs.append((losses, emb.xs[0].detach().double().cpu(), float(emb.scales[0]), torch.from_numpy(xs[0])))
    (le, xe, se, x0), (lg, xg, sg, _) = runs
    print('eager ', le)
    print('graph ', lg)
    assert all(np.isfinite(le)) and le[-1] != le[0]   # (the steps do move the points)
    for a, b in zip(le, lg):
        assert abs(a - b) <= sc.TOL['loss'][dname] * abs(a), (le, lg)
    # the single-step rule of tests/step_cases.py (TOL['disp'] of the displacement + 8 ulp of max|x| for the rounding of the
    # stored point) summed over the K = 8 steps: the displacements add up to at least `moved`, the roundings to 8 K ulp
    K = 8
    moved = float((xe - x0).abs().max())
    allowed = sc.TOL['disp'][dname] * moved + 8 * K * sc.ULP[dname] * float(xe.abs().max())
    err = float((xg - xe).abs().max())
    print(f'moved {moved:.3e} err {err:.3e} allowed {allowed:.3e}')
    assert moved > 0 and err <= allowed
    assert abs(sg - se) <= sc.TOL['disp'][dname] * abs(se - 0.5) + 8 * K * sc.ULP[dname] * abs(se)
