"""The fused RiemannianSGD kernels of Grassmann / Stiefel points (mm_mat_rsgd_step, mm_mat_rsgd_momentum_step through
_MatrixManifold.rsgd_step / rsgd_momentum_step and RiemannianSGD) against oracle/ref_port.rsgd_step in fp64, with the
measured tolerance rule of tests/grass_cases.py: the yardstick is the explicit egrad2rgrad / norm / clip / retr|exp /
transp sequence of per-operation launches on the GPU, same inputs.  That yardstick shares the device code under test; the
absolute check is tests/test_mat_oracle_gpu.py (every per-operation map at all 26 shapes of mat_cases.SHAPES, both kinds, and the
fused step at (2,1) (3,3) (4,4) (6,4) (7,3) (8,4) (9,1), fp32 and fp64, under the rule of tests/mat_cases.py)."""
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

LR = 0.05
# (kind, retraction, exact)
VARIANTS = {'grassmann_svd': ('grassmann', 'svd', False), 'grassmann_qr': ('grassmann', 'qr', False),
            'grassmann_exp': ('grassmann', 'svd', True), 'stiefel_svd': ('stiefel', 'svd', False),
            'stiefel_qr': ('stiefel', 'qr', False)}
SHAPES = [(5, 2), (9, 4), (4, 1)]


def _oracle_manifold(kind, retr, N, p):
    man = gc.ref.make(kind, N, p)
    if retr == 'qr':   # grassmann.py:71-74 / stiefel.py:62-63
        man.retr = (lambda x, u: torch.linalg.qr(x + u)[0]) if kind == 'grassmann' else man.retr_qr
    return man


def _device_manifold(kind, retr, N, p):
    import graphembed.manifolds as M
    return (M.Grassmann if kind == 'grassmann' else M.Stiefel)(N, p, retr=retr)


def _egrad(cnt, N, p, k=0):
    g = torch.Generator().manual_seed(gc._seed('egrad', cnt, N, p, k))
    return torch.randn(cnt, N, p, dtype=torch.float64, generator=g)


def _median_norm(oman, x, g):
    return float(oman.norm(x, oman.egrad2rgrad(x, g)).median())


def _old_rgrad(man, x, g, clip):
    rgrad = man.egrad2rgrad(x, g)
    if clip is not None:
        rgrad = rgrad * torch.clamp(clip / man.norm(x, rgrad, keepdim=True), max=1.0)
    return rgrad


def _old_step(man, x, g, clip, exact, lr=LR):
    """optim/rsgd.py:63-68,82 as separate launches."""
    with torch.no_grad():
        return (man.exp if exact else man.retr)(x, -lr * _old_rgrad(man, x, g, clip))


def _old_momentum_step(man, x, g, buf, clip, exact, momentum, dampening):
    """optim/rsgd.py:70-80 as separate launches; returns (new points, transported buffer)."""
    with torch.no_grad():
        buf = buf * momentum + (1 - dampening) * _old_rgrad(man, x, g, clip)
        new = (man.exp if exact else man.retr)(x, -LR * buf)
        return new, man.transp(x, new, buf)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', SHAPES)
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_rsgd_step_vs_fp64_oracle(variant, N, p, dname):
    kind, retr, exact = VARIANTS[variant]
    dt = gc.DT[dname]
    oman, man = _oracle_manifold(kind, retr, N, p), _device_manifold(kind, retr, N, p)
    failures = []
    for cnt in (1, 63, 64, 65, 130):
        x, g = gc.frames('uniform', cnt, N, p), _egrad(cnt, N, p)
        # the median norm: both branches of the clip in one launch
        for clip in (None, _median_norm(oman, x, g)):
            want, _ = gc.ref.rsgd_step(oman, x, g, lr=LR, max_grad_norm=clip, exact=exact)
            xd, gd = x.to(dt).cuda(), g.to(dt).cuda()
            old = _old_step(man, xd, gd, clip, exact)
            with gc.CallSpy() as spy:
                new = man.rsgd_step(xd, gd, lr=LR, max_grad_norm=clip, exact=exact)
            assert spy.calls == ['mm_mat_rsgd_step'], spy.calls
            assert new is not None and new.data_ptr() != xd.data_ptr() and torch.isfinite(new).all()
            gc.check(f'rsgd {variant} {N}x{p} {dname} cnt={cnt} clip={clip is not None}', 'x_new', old, new, want, dt, failures)
            inplace = xd.clone()
            assert man.rsgd_step(inplace, gd, lr=LR, max_grad_norm=clip, exact=exact, inplace=True) is inplace
            assert torch.equal(inplace, new)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', SHAPES)
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_rsgd_momentum_two_steps_vs_fp64_oracle(variant, N, p, dname):
    kind, retr, exact = VARIANTS[variant]
    dt = gc.DT[dname]
    momentum, dampening = 0.9, 0.1
    oman, man = _oracle_manifold(kind, retr, N, p), _device_manifold(kind, retr, N, p)
    failures = []
    for cnt in (1, 65, 130):
        x0 = gc.frames('uniform', cnt, N, p)
        g0, g1 = _egrad(cnt, N, p, 0), _egrad(cnt, N, p, 1)
        clip = _median_norm(oman, x0, g0)
        wx, wbuf = x0, None   # (the optimizer seeds the buffer with a copy of the first gradient: rsgd.py:53-54)
        ox, obuf = x0.to(dt).cuda(), g0.to(dt).cuda().clone()
        nx, nbuf = ox.clone(), obuf.clone()
        for k, g in enumerate((g0, g1)):
            wx, wbuf = gc.ref.rsgd_step(oman, wx, g, lr=LR, momentum=momentum, dampening=dampening, max_grad_norm=clip,
                                        exact=exact, momentum_buffer=wbuf)
            gd = g.to(dt).cuda()
            ox, obuf = _old_momentum_step(man, ox, gd, obuf, clip, exact, momentum, dampening)
            with gc.CallSpy() as spy:
                nx = man.rsgd_momentum_step(nx, gd, nbuf, lr=LR, momentum=momentum, dampening=dampening, max_grad_norm=clip,
                                            exact=exact)
            assert spy.calls == ['mm_mat_rsgd_momentum_step'], spy.calls
            assert nx is not None and torch.isfinite(nx).all() and torch.isfinite(nbuf).all()
            tag = f'momentum {variant} {N}x{p} {dname} cnt={cnt} step={k + 1}'
            gc.check(tag, 'x_new', ox, nx, wx, dt, failures)
            gc.check(tag, 'buffer', obuf, nbuf, wbuf, dt, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('retr', ['svd', 'qr'])
def test_optimizer_step_is_one_launch(retr, momentum):
    """RiemannianSGD.step() on a Grassmann parameter: exactly one fused kernel, no per-operation map."""
    from graphembed.modules import ManifoldParameter
    from graphembed.optim import RiemannianSGD
    N, p, cnt = 5, 2, 65
    man = _device_manifold('grassmann', retr, N, p)
    x = gc.frames('uniform', cnt, N, p)
    par = ManifoldParameter(x.float().cuda(), manifold=man)
    opt = RiemannianSGD([par], lr=LR, momentum=momentum, dampening=0.1, max_grad_norm=1.0)
    name = 'mm_mat_rsgd_momentum_step' if momentum else 'mm_mat_rsgd_step'
    wx, wbuf = x, None
    for k in range(2):
        g = _egrad(cnt, N, p, k)
        par.grad = g.float().cuda()
        with gc.CallSpy() as spy:
            opt.step()
        assert spy.calls == [name], spy.calls
        wx, wbuf = gc.ref.rsgd_step(_oracle_manifold('grassmann', retr, N, p), wx, g, lr=LR, momentum=momentum, dampening=0.1,
                                    max_grad_norm=1.0, momentum_buffer=wbuf)
    # The arithmetic is held to the oracle by the tests above; this asks only whether the optimizer hands the kernel its own
    # state.  A misplaced gradient or buffer moves a point by lr |rgrad| ~ 5e-2, the fp32 rounding of two steps on entries
    # of size <= 1 is ~1e-6: 1e-4 separates the two.
    assert gc.deviation(par, wx) <= 1e-4


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_graphed_train_step_replays(dname):
    """Three replays of a captured Grassmann training step (fused objective + fused optimizer kernel) against three fp64
    oracle steps from the same start; the yardstick is three eager steps of per-operation launches."""
    from graphembed.graphed import GraphedTrainStep
    from graphembed.optim import RiemannianSGD
    N, p, n, lr, clip = 5, 2, 129, 1e-2, 1.0
    dt = gc.DT[dname]
    fn, kw = gc.objective('quotient')
    emb = gc.embedding(n, N, p, dt, gc.frames('spread', n, N, p))
    emb.burnin(True)   # the scale stays put: the step is the points'
    target = gc.targets(n).to(dt).cuda()
    opt = RiemannianSGD(list(emb.xs), lr=lr, max_grad_norm=clip)
    step = GraphedTrainStep(lambda: emb.fused_objective(fn, target, None, **kw), [opt], warmup=1)
    with gc.CallSpy() as spy:
        step.capture()
    assert spy.calls.count('mm_grass_pdist_loss') == 2 and spy.calls.count('mm_mat_rsgd_step') == 2, spy.calls   # warm-up + recording
    assert 'mm_mat_map' not in spy.calls and 'mm_grass_pdist_bwd' not in spy.calls, spy.calls
    torch.cuda.synchronize()
    start = emb.xs[0].detach().clone()
    # yardstick: three eager steps, every operation its own launch
    old = gc.embedding(n, N, p, dt, start.double().cpu())
    man = old.manifolds[0]
    for _ in range(3):
        old_loss = fn(target, old.compute_dists(None), **kw)
        g, = torch.autograd.grad(old_loss, [old.xs[0]])
        with torch.no_grad():
            old.xs[0].copy_(_old_step(man, old.xs[0].detach(), g, clip, False, lr))
    # oracle: three fp64 steps
    oman = gc.ref.Grassmann(N, p)
    wx = start.double().cpu()
    s = torch.tensor(gc.SCALE_RAW, dtype=torch.float64)
    losses = []
    for _ in range(3):
        xr = wx.clone().requires_grad_(True)
        wl = gc.oracle_loss('quotient', gc.targets(n), gc.ref.compute_dists([oman], [xr], [s]))
        g, = torch.autograd.grad(wl, [xr])
        losses.append(float(wl))
        wx, _ = gc.ref.rsgd_step(oman, wx, g, lr=lr, max_grad_norm=clip)
    with gc.CallSpy() as spy:
        for _ in range(3):
            last = step()
    assert spy.calls == [], spy.calls   # replays launch the graph, nothing else
    torch.cuda.synchronize()
    failures = []
    gc.check(f'graphed {N}x{p} n={n} {dname}', 'x after 3 steps', old.xs[0], emb.xs[0], wx, dt, failures)
    gc.check(f'graphed {N}x{p} n={n} {dname}', 'loss of step 3', old_loss, last, torch.tensor(losses[-1], dtype=torch.float64), dt,
             failures)
    assert not failures, '\n'.join(failures)
