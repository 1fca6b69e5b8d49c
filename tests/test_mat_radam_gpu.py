"""The fused RiemannianAdam step of Grassmann / Stiefel points (mm_mat_radam_step, csrc/mat_step.hip; _MatrixManifold.radam_step,
picked up by RiemannianAdam) against oracle/ref_port.radam_step in fp64 under the absolute rule of tests/mat_cases.py, on the cases
of tests/grass_subset_cases.py: three consecutive steps from empty state, the optimizer's wiring (fused, and composed in a child
process under MM_RADAM_UNFUSED=1), and two minibatch training steps, eager and as a captured graph.  Every comparison prints
err / bound (-rA); the worst ratios are in profiles/grass_minibatch.md."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grass_subset_cases as C  # noqa: E402
from grass_cases import CallSpy  # noqa: E402

pytestmark = pytest.mark.gpu
mc, gc = C.mc, C.gc
EPS = 1e-8   # graphembed.utils.EPS, the reference's constant for both precisions


def device_manifold(kind, retr, N, p):
    import graphembed.manifolds as M
    return (M.Grassmann if kind == 'grassmann' else M.Stiefel)(N, p, retr=retr)


def three_steps(man, x, gs, nc, clip, exact, inplace):
    """[(x_k, exp_avg_k, exp_avg_sq_k, step_k)] of three man.radam_step calls from empty state"""
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    step, ticket = torch.ones((), dtype=torch.float64, device=x.device), torch.zeros(1, dtype=torch.int32, device=x.device)
    x = x.clone()
    out = []
    for g in gs:
        with CallSpy() as spy:
            new = man.radam_step(x, g, m, v, step, ticket, lr=C.RADAM_LR, betas=C.BETAS, nc=nc, eps=EPS, max_grad_norm=clip, exact=exact,
                                 inplace=inplace)
        assert spy.calls == ['mm_mat_radam_step'], spy.calls
        assert new is not None and (new is x) == inplace and int(ticket) == 0
        x = new
        out.append((x.clone(), m.clone(), v.clone(), float(step)))
    return out


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', C.RADAM_SHAPES + C.RADAM_STIEFEL_ONLY, ids=lambda v: str(v))
@pytest.mark.parametrize('variant', sorted(C.VARIANTS))
def test_three_steps_against_the_oracle(variant, N, p, dname):
    """Grassmann at N = p (a single point, tangent space {0}) asserts finite output and x_new^T x_new = I to 64 eps only.  With
    `exact` the entry point moves with the instance's retraction there: exp keeps x^T x only along tangents, and the direction
    at N = p is normalised rounding noise (the reference's own fp64 step leaves x^T x - I at 2.2e-02 on Gr(3,3) and 1.1e-02 on
    Gr(4,4) after these three steps)."""
    kind, retr, exact = C.VARIANTS[variant]
    dt = gc.DT[dname]
    man = device_manifold(kind, retr, N, p)
    failures = []
    for cnt in C.RADAM_CNT:
        x = C.points('uniform', cnt, N, p).to(dt).cuda()
        gs = [g.to(dt).cuda() for g in C.radam_grads(cnt, N, p)]
        clip = C.radam_clip(kind, cnt, N, p)
        for nc in (False, True):
            got = three_steps(man, x, gs, nc, clip, exact, False)
            again = three_steps(man, x, gs, nc, clip, exact, True)
            for k, (a, b) in enumerate(zip(got, again)):
                assert all(torch.equal(s, t) for s, t in zip(a[:3], b[:3])), f'the in-place call differs at step {k + 1}'
                assert a[3] == b[3] == 2.0 + k, (k, a[3])                      # the device step counter
                assert torch.equal(a[2], a[2][:, :1, :1].expand_as(a[2])), 'one scalar per point, stored over its entries'
            if kind == 'grassmann' and N == p:
                # Gr(N,N) is a single point: its Riemannian gradient is rounding noise and Adam normalises that noise to size lr
                eye = torch.eye(p, dtype=dt, device='cuda')
                off = [float((xk.transpose(1, 2) @ xk - eye).abs().max()) for xk, _, _, _ in got]
                print(f'radam {variant} {N}x{p} cnt={cnt} nc={nc} {dname}: max |x^T x - I| after steps 1..3 '
                      + ' '.join(f'{o:.3e}' for o in off) + f' / {64 * gc.eps_of(dt):.3e}')
                for xk, mk, vk, _ in got:
                    assert bool(torch.isfinite(xk).all() and torch.isfinite(mk).all() and torch.isfinite(vk).all())
                if not max(off) <= 64 * gc.eps_of(dt):
                    failures.append(f'radam {variant} {N}x{p} cnt={cnt} nc={nc} {dname}: max |x^T x - I| {max(off):.3e} > 64 eps')
                continue
            q = C.radam_quantities(variant, cnt, N, p, nc)
            tag = f'radam {variant} {N}x{p} cnt={cnt} nc={nc}'
            for k, (xk, mk, vk, _) in enumerate(got):
                C.check(tag, f'radam_x@{k + 1}', xk, q[f'x{k + 1}'], dname, failures)
                C.check(tag, f'radam_exp_avg@{k + 1}', mk, q[f'exp_avg{k + 1}'], dname, failures)
                C.check(tag, f'radam_exp_avg_sq@{k + 1}', vk, q[f'exp_avg_sq{k + 1}'], dname, failures)
    assert not failures, '\n'.join(failures)


# ---- the optimizer -----------------------------------------------------------------------------------------------------------------
WIRING = dict(cnt=65, N=5, p=2, lr=0.01, clip=100.0)


def wiring_run(dname):
    """three RiemannianAdam steps (the reference grid's groups) on a Gr(5,2) embedding with given gradients; returns the entry
    points recorded and the points and moments after each step"""
    from graphembed.optim import RiemannianAdam
    w = WIRING
    dt = gc.DT[dname]
    emb = gc.embedding(w['cnt'], w['N'], w['p'], dt, C.points('uniform', w['cnt'], w['N'], w['p']).double())
    opt = RiemannianAdam([dict(params=emb.xs, lr=w['lr'], exact=True, max_grad_norm=w['clip']), dict(params=emb.scales, lr=w['lr'])])
    trace = []
    with CallSpy() as spy:
        for g in C.radam_grads(w['cnt'], w['N'], w['p']):
            emb.xs[0].grad = g.to(dt).cuda()
            emb.scales[0].grad = torch.full_like(emb.scales[0], 0.25)
            opt.step()
            st = opt.state[emb.xs[0]]
            trace.append((emb.xs[0].detach().clone().cpu(), st['exp_avg'].clone().cpu(), st['exp_avg_sq'].clone().cpu()))
    assert float(opt.state[emb.xs[0]]['step']) == 4.0 and float(emb.scales[0]) != gc.SCALE_RAW
    return spy.calls, trace


def hold_wiring(tag, trace, dname, failures):
    w = WIRING
    q = C.radam_quantities('grassmann_exp', w['cnt'], w['N'], w['p'], False, w['lr'], w['clip'])
    for k, (xk, mk, vk) in enumerate(trace):
        C.check(tag, f'wiring_x@{k + 1}', xk, q[f'x{k + 1}'], dname, failures)
        C.check(tag, f'wiring_exp_avg@{k + 1}', mk, q[f'exp_avg{k + 1}'], dname, failures)
        C.check(tag, f'wiring_exp_avg_sq@{k + 1}', vk, q[f'exp_avg_sq{k + 1}'], dname, failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_the_optimizer_takes_the_fused_step(dname):
    """(fails without _MatrixManifold.radam_step: the update is then composed from mm_mat_map launches)"""
    calls, trace = wiring_run(dname)
    assert calls.count('mm_mat_radam_step') == 3 and 'mm_mat_map' not in calls, calls
    failures = []
    hold_wiring(f'fused optimizer {dname}', trace, dname, failures)
    assert not failures, '\n'.join(failures)


def test_the_composed_route_is_still_there_and_agrees(tmp_path):
    """MM_RADAM_UNFUSED=1 is read at import: a fresh child process runs the same three steps composed from the manifold's maps"""
    out = tmp_path / 'unfused.pt'
    env = dict(os.environ, MM_RADAM_UNFUSED='1')
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), 'unfused', str(out)], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = torch.load(out)
    failures = []
    for dname in ('f32', 'f64'):
        calls, trace = got[dname]
        assert 'mm_mat_radam_step' not in calls and calls.count('mm_mat_map') >= 3 * 3, calls
        hold_wiring(f'composed optimizer {dname}', trace, dname, failures)
    assert not failures, '\n'.join(failures)


# ---- two minibatch training steps --------------------------------------------------------------------------------------------------
def _training(dname):
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    from graphembed.optim import RiemannianAdam
    from test_grass_subset_gpu import _dataset
    t = C.TRAIN
    dt = gc.DT[dname]
    emb = gc.embedding(C.N_TOTAL, t['N'], t['p'], dt, C.points(t['regime'], C.N_TOTAL, t['N'], t['p']).double())
    emb.burnin(True)   # the scale stays put: the step is the points'
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=t['lr'], exact=True, max_grad_norm=t['clip'])])
    return emb, opt, BatchedObjective(StressLoss(), _dataset(C.raw_dense(C.N_TOTAL).to(dt).cuda()), emb)


def _after(emb, opt):
    st = opt.state[emb.xs[0]]
    assert float(st['step']) == 3.0
    return emb.xs[0].detach(), st['exp_avg'], st['exp_avg_sq']


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_two_minibatch_steps_eager_and_replayed(dname):
    from graphembed.graphed import GraphedTrainStep
    b1, b2 = (b.cuda() for b in C.train_batches())
    q = C.train_quantities()
    failures = []
    # eager
    emb, opt, objective = _training(dname)
    with CallSpy() as eager:
        for b in (b1, b2):
            opt.zero_grad(set_to_none=True)
            objective(b).backward()
            opt.step()
    assert eager.calls == ['mm_grass_pdist_loss_subset', 'mm_mat_radam_step'] * 2, eager.calls
    for name, got in zip(('x', 'exp_avg', 'exp_avg_sq'), _after(emb, opt)):
        C.check(f'training eager {dname}', f'train_{name}', got, q[name], dname, failures)
    # the first step as the warm-up of a capture, the second as a replay with the batch copied into the captured tensor
    emb, opt, objective = _training(dname)
    buf = b1.clone()
    step = GraphedTrainStep(lambda: objective(buf), [opt], warmup=1)
    with CallSpy() as graphed:
        step.capture()
    assert graphed.calls == eager.calls, graphed.calls   # warm-up + recording
    buf.copy_(b2)
    with CallSpy() as replay:
        step()
    assert replay.calls == []
    torch.cuda.synchronize()
    for name, got in zip(('x', 'exp_avg', 'exp_avg_sq'), _after(emb, opt)):
        C.check(f'training replayed {dname}', f'train_{name}', got, q[name], dname, failures)
    assert not failures, '\n'.join(failures)


if __name__ == '__main__':
    if sys.argv[1] == 'unfused':
        assert os.environ.get('MM_RADAM_UNFUSED') == '1'
        torch.save({dname: wiring_run(dname) for dname in ('f32', 'f64')}, sys.argv[2])
