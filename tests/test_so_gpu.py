"""The SO(n) kernels of csrc/so.hip on the GPU, n = 2 .. 4, fp32 and fp64, through the C ABI and through
graphembed.manifolds.SpecialOrthogonal, held to the long-double oracle and the tolerance rule of tests/so_cases.py (every printed
line is err / bound; -rA shows them).

Worst err / bound measured on an MI355X: profiles/so.md."""
import pytest
import torch

import grass_cases as gc
import so_cases as sc
from so_cases import CNT, PREFIXES, Quantity

pytestmark = pytest.mark.gpu

DNAMES = ('f32', 'f64')


def _man(N, retr='svd'):
    import graphembed.manifolds as M
    return M.SpecialOrthogonal(N, retr=retr)


def _dev(t, dname):
    return t.to(sc.DT[dname]).cuda()


def _head(q, cnt):
    """the Quantity of the first cnt entries (the bound is that of the whole case)"""
    return Quantity(q.want[:cnt], q.cond, q.port32, q.scale)


def _names(regime, squared):
    return ('val', 'grad_x', 'grad_y') if squared or regime == 'spread' else ('val', )


def _abi():
    from graphembed import _backend as B
    return B, B.lib()


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_elementwise_dist(N, dname):
    """cnt = 130 and the prefixes 1, 63, 64, 65, squared and not: autograd's two launches, and the one-launch form of the C ABI"""
    B, lib = _abi()
    man, failures = _man(N), []
    for regime in sc.REGIMES:
        x = sc.points(regime, CNT, N)
        xd, yd = _dev(x, dname), _dev(torch.roll(x, 1, 0), dname)
        for squared in (True, False):
            q = sc.dist_quantities(regime, N, squared)
            what = 'd2' if squared else 'd'
            for cnt in (CNT, ) + PREFIXES:
                tag = f'so dist {N} {regime} cnt={cnt}'
                xs, ys = xd[:cnt].clone().requires_grad_(True), yd[:cnt].clone().requires_grad_(True)
                d = man.dist(xs, ys, squared=squared)
                (d * _dev(sc.upstream(CNT)[:cnt], dname)).sum().backward()
                got = {'val': d, 'grad_x': xs.grad, 'grad_y': ys.grad}
                for name in _names(regime, squared):
                    sc.check(tag, f'so_dist_{what}_{name}', got[name], _head(q[name], cnt), dname, failures)
                assert all(bool(torch.isfinite(t).all()) for t in got.values()), tag
            out, gx, gy = torch.empty(CNT, dtype=xd.dtype, device='cuda'), torch.empty_like(xd), torch.empty_like(yd)
            g = _dev(sc.upstream(CNT), dname)
            lib.call('mm_so_dist', B.dtype_code(xd), B.ptr(xd), B.ptr(yd), B.ptr(g), CNT, N, int(squared), B.ptr(out), B.ptr(gx),
                     B.ptr(gy), B.stream_of(xd))
            got = {'val': out, 'grad_x': gx, 'grad_y': gy}
            for name in _names(regime, squared):
                sc.check(f'so dist {N} {regime} one launch', f'so_dist_{what}_{name}@abi', got[name], q[name], dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_log_exp_and_the_gradient_identity(N, dname):
    B, lib = _abi()
    man, failures = _man(N), []
    for regime in sc.REGIMES:
        x, u = sc.points(regime, CNT, N), sc.tangents(regime, CNT, N)
        xd, yd, ud = _dev(x, dname), _dev(torch.roll(x, 1, 0), dname), _dev(u, dname)
        q = sc.map_quantities(regime, N)
        for cnt in (CNT, ) + PREFIXES:
            tag = f'so map {N} {regime} cnt={cnt}'
            with torch.no_grad():
                sc.check(tag, 'so_map_log', man.log(xd[:cnt], yd[:cnt]), _head(q['log'], cnt), dname, failures)
                sc.check(tag, 'so_map_exp', man.exp(xd[:cnt], ud[:cnt]), _head(q['exp'], cnt), dname, failures)
        for op, name, second in ((B.SO_LOG, 'log', yd), (B.SO_EXP, 'exp', ud)):
            out = torch.empty_like(xd)
            lib.call('mm_so_map', B.dtype_code(xd), op, B.ptr(xd), B.ptr(second), CNT, N, B.ptr(out), B.stream_of(xd))
            sc.check(f'so map {N} {regime}', f'so_map_{name}@abi', out, q[name], dname, failures)
        # proju(y, d d2 / dy) = -2 log_y(x): the same tangent vector from two kernels, held to the gradient's bound.  The identity
        # is exact on SO(n) only — the inputs are orthogonal to fp32 rounding — so the kernels' residual is held to the oracle's.
        qg = sc.dist_quantities(regime, N, True)['grad_y']
        g = _dev(sc.upstream(CNT), dname)
        gx, gy = torch.empty_like(xd), torch.empty_like(yd)
        lib.call('mm_so_dist', B.dtype_code(xd), B.ptr(xd), B.ptr(yd), B.ptr(g), CNT, N, 1, None, B.ptr(gx), B.ptr(gy), B.stream_of(xd))
        with torch.no_grad():
            resid = man.proju(yd, gy) + 2 * g.reshape(-1, 1, 1) * man.log(yd, xd)
        err = float((resid.double().cpu() - sc.identity_residual(regime, N)).abs().max())
        bnd = qg.bound(dname)
        print(f'so identity {N} {regime} {dname}: |proju(y, grad_y) + 2 g log_y(x)| {err:.3e} / bound {bnd:.3e} = {err / bnd:.3f}')
        key = ('so_identity', dname)
        if err / bnd > sc.RATIOS.get(key, (-1.0, ''))[0]:
            sc.RATIOS[key] = (err / bnd, f'{N} {regime}')
        if not err <= bnd:
            failures.append(f'identity {N} {regime} {dname}: {err:.3e} > {bnd:.3e}')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_cut_locus_is_finite(N, dname):
    """a plane angle within 1e-3 of pi and a pair in different components of O(n): d2 under the rule, everything finite,
    exp outputs orthogonal"""
    man, failures = _man(N), []
    x, y, u = sc.cut_pairs(N)
    xd, yd, ud = (_dev(t, dname).requires_grad_(k < 2) for k, t in enumerate((x, y, u)))
    d2 = man.dist(xd, yd, squared=True)
    sc.check(f'so cut {N}', 'so_cut_d2', d2, sc.cut_quantities(N)['val'], dname, failures)
    d2.sum().backward()
    d = man.dist(xd.detach().requires_grad_(True), yd.detach(), squared=False)
    d.sum().backward()
    with torch.no_grad():
        lg, ex = man.log(xd, yd), man.exp(xd, ud)
        pd = man.pdist(torch.cat([xd, yd]), squared=True)
    for name, t in (('d2', d2), ('grad_x', xd.grad), ('grad_y', yd.grad), ('d', d), ('log', lg), ('exp', ex), ('pdist', pd)):
        assert bool(torch.isfinite(t).all()), (N, dname, name)
    defect, bnd = sc.orth_defect(ex), sc.orth_bound(x, dname)
    print(f'so cut {N} {dname}: |exp^T exp - I| {defect:.3e} / bound {bnd:.3e}')
    assert defect <= bnd, (defect, bnd)
    assert not failures, '\n'.join(failures)


def _pdist_run(man, xd, squared, rows, dname):
    xs = xd.clone().requires_grad_(True)
    d = man.pdist(xs, squared=squared, rows=rows)
    (d * _dev(sc.upstream(d.numel()), dname)).sum().backward()
    return d.detach(), xs.grad


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_pdist_forward_and_backward(N, dname):
    """n in {2, 3, 65, 129, 130}: below a tile, the tile edges, more than one block of columns"""
    man, failures = _man(N), []
    for regime in sc.REGIMES:
        for n in sc.PDIST_N:
            xd = _dev(sc.points(regime, n, N), dname)
            for squared in (True, False):
                q = sc.pdist_quantities(regime, n, N, squared)
                val, grad = _pdist_run(man, xd, squared, None, dname)
                what = 'd2' if squared else 'd'
                sc.check(f'so pdist {N} {regime} n={n}', f'so_pdist_{what}_val', val, q[(None, 'val')], dname, failures)
                if squared or regime == 'spread':
                    sc.check(f'so pdist {N} {regime} n={n}', f'so_pdist_{what}_grad', grad, q[(None, 'grad')], dname, failures)
                assert bool(torch.isfinite(grad).all()), (regime, n, squared)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_row_ranges_shard_the_pair_list(N, dname):
    """four non-empty row ranges and an empty one at n = 129; the four tile [0, 129) and must sum to the whole"""
    B, lib = _abi()
    man, failures, n = _man(N), [], 129
    for regime in sc.REGIMES:
        xd = _dev(sc.points(regime, n, N), dname)
        q = sc.pdist_quantities(regime, n, N, True, sc.ROWS_129)
        for rows in sc.ROWS_129:
            val, grad = _pdist_run(man, xd, True, rows, dname)
            if sc.pair_slice(n, rows)[0] == sc.pair_slice(n, rows)[1]:
                assert val.numel() == 0 and float(grad.abs().max()) == 0, rows
                continue
            sc.check(f'so pdist {N} {regime} n={n} rows={rows}', 'so_pdist_rows_val', val, q[(rows, 'val')], dname, failures)
            sc.check(f'so pdist {N} {regime} n={n} rows={rows}', 'so_pdist_rows_grad', grad, q[(rows, 'grad')], dname, failures)
        # the shards of ONE upstream vector: values concatenate and gradients add up to the full range's, both under its bounds
        whole = sc.pdist_quantities(regime, n, N, True)
        g = _dev(sc.upstream(n * (n - 1) // 2), dname)
        vals, total = [], torch.zeros_like(xd)
        dt = B.dtype_code(xd)
        ws = torch.empty(lib.raw('mm_so_pdist_ws_bytes')(dt, n, N), dtype=torch.uint8, device='cuda')
        for rows in sc.ROWS_129:
            lo, hi = sc.pair_slice(n, rows)
            out, grad = torch.empty(hi - lo, dtype=xd.dtype, device='cuda'), torch.empty_like(xd)
            gs = g[lo:hi].contiguous()
            lib.call('mm_so_pdist_fwd', dt, B.ptr(xd), n, N, rows[0], rows[1], 1, B.ptr(out) if hi > lo else None, B.stream_of(xd))
            ws.fill_(0xFF)   # a dirty workspace changes nothing
            lib.call('mm_so_pdist_bwd', dt, B.ptr(xd), B.ptr(gs) if hi > lo else None, n, N, rows[0], rows[1], 1, B.ptr(grad),
                     B.ptr(ws), B.stream_of(xd))
            if hi > lo:
                vals.append(out)
            total += grad
        sc.check(f'so pdist {N} {regime} n={n} shards', 'so_pdist_rows_val@sum', torch.cat(vals), whole[(None, 'val')], dname, failures)
        sc.check(f'so pdist {N} {regime} n={n} shards', 'so_pdist_rows_grad@sum', total, whole[(None, 'grad')], dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_coincident_points(N, dname):
    """point 7 := point 3: zero distance, a finite gradient, no NaN in the fused loss"""
    man, failures, n = _man(N), [], 65
    xd = _dev(sc.points('spread', n, N, True), dname)
    q = sc.pdist_quantities('spread', n, N, True, (None, ), True)
    val, grad = _pdist_run(man, xd, True, None, dname)
    sc.check(f'so pdist {N} spread n={n} coincident', 'so_pdist_coincident_val', val, q[(None, 'val')], dname, failures)
    sc.check(f'so pdist {N} spread n={n} coincident', 'so_pdist_coincident_grad', grad, q[(None, 'grad')], dname, failures)
    k = sc.pair_slice(n, (3, 4))[0] + 7 - 3 - 1
    assert float(val[k]) == 0.0
    val1, grad1 = _pdist_run(man, xd, False, None, dname)
    assert float(val1[k]) == 0.0 and bool(torch.isfinite(grad1).all()) and bool(torch.isfinite(grad).all())
    a, b = xd[3:4].clone().requires_grad_(True), xd[7:8].clone().requires_grad_(True)
    for squared in (True, False):   # element-wise too: D = 0 gives d = 0 and a zero gradient
        d = man.dist(a, b, squared=squared)
        ga, gb = torch.autograd.grad(d.sum(), [a, b])
        assert float(d.detach()) == 0.0 and float(ga.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0
    for loss_name in sc.LOSSES:
        fn, kw = gc.objective(loss_name)
        xs, s = xd.clone().requires_grad_(True), torch.tensor([sc.SCALE_RAW], dtype=xd.dtype, device='cuda', requires_grad=True)
        loss = man.pdist_loss(xs, s, _dev(sc.targets(n), dname), fn.fused_spec(**kw))
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(xs.grad).all()) and bool(torch.isfinite(s.grad).all()), loss_name
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('loss_name', sc.LOSSES)
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', sc.DIMS)
def test_fused_objective(N, dname, loss_name):
    """pdist_loss at n = 65 and 130: loss, point gradient, scale gradient — through the C ABI on a dirty workspace and through
    autograd"""
    B, lib = _abi()
    man, failures = _man(N), []
    fn, kw = gc.objective(loss_name)
    lkind, alpha, eps, terms = fn.fused_spec(**kw)[:4]
    for regime in sc.REGIMES:
        for n in (65, 130):
            q = sc.loss_quantities(regime, n, N, loss_name)
            tag = f'so objective {N} {regime} {loss_name} n={n}'
            xd, tg = _dev(sc.points(regime, n, N), dname), _dev(sc.targets(n), dname)
            xs = xd.clone().requires_grad_(True)
            s = torch.tensor([sc.SCALE_RAW], dtype=xd.dtype, device='cuda', requires_grad=True)
            loss = man.pdist_loss(xs, s, tg, fn.fused_spec(**kw))
            loss.backward()
            for name, got in (('loss', loss.reshape(1)), ('grad_x', xs.grad), ('grad_scale', s.grad)):
                sc.check(tag, f'so_loss_{name}', got, q[name], dname, failures)
            dt = B.dtype_code(xd)
            ws = torch.empty(lib.raw('mm_so_pdist_loss_ws_bytes')(dt, n, N), dtype=torch.uint8, device='cuda').fill_(0xFF)
            out, grad = torch.empty(2, dtype=xd.dtype, device='cuda'), torch.empty_like(xd)
            lib.call('mm_so_pdist_loss', dt, B.LOSS_STRESS if lkind == 'stress' else B.LOSS_QUOTIENT, B.ptr(xd), B.ptr(tg),
                     B.ptr(s.detach()), n, N, 0, n, alpha, eps, terms, None, B.ptr(out), B.ptr(grad), B.ptr(ws), B.stream_of(xd))
            for name, got in (('loss', out[:1]), ('grad_x', grad), ('grad_scale', out[1:])):
                sc.check(tag, f'so_loss_{name}@abi', got, q[name], dname, failures)
    assert not failures, '\n'.join(failures)


# ---- end to end: ManifoldEmbedding(65, [SpecialOrthogonal(3)]) with StressLoss ---------------------------------------------------
E2E_N, E2E_DIM = 65, 3


def _embedding(dname, x, retr='svd'):
    from graphembed.modules import ManifoldEmbedding
    dt = sc.DT[dname]
    torch.set_default_dtype(dt)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(E2E_N, [_man(E2E_DIM, retr)])
    finally:
        torch.set_default_dtype(torch.float32)
    assert emb.xs[0].shape == (E2E_N, E2E_DIM, E2E_DIM) and emb.xs[0].dtype == dt
    assert sc.orth_defect(emb.xs[0]) <= 64 * sc.U32 and float((torch.linalg.det(emb.xs[0].detach()) - 1).abs().max()) <= 1e-5
    with torch.no_grad():
        emb.xs[0].copy_(x.to(dt).cuda())
        emb.scales[0].fill_(sc.SCALE_RAW)
    return emb


def _optimizer(name, emb, exact=False):
    from graphembed.optim import RiemannianAdam, RiemannianSGD
    if name == 'rsgd':
        return RiemannianSGD(list(emb.xs), lr=sc.LR, exact=exact)
    return RiemannianAdam(list(emb.xs), lr=sc.LR, exact=exact)


@pytest.mark.parametrize('exact', (False, True))
@pytest.mark.parametrize('optimizer', ('rsgd', 'radam'))
@pytest.mark.parametrize('dname', DNAMES)
def test_embedding_trains_one_step(dname, optimizer, exact):
    """fused objective, backward and one optimizer step against the oracle's step; `exact` takes the optimizers' generic route
    over the new exp, the retraction the fused St(n, n) step kernel"""
    from graphembed.objectives import StressLoss
    failures = []
    for regime in sc.REGIMES:
        tag = f'so e2e {regime} {optimizer}{" exact" if exact else ""}'
        emb = _embedding(dname, sc.points(regime, E2E_N, E2E_DIM))
        opt = _optimizer(optimizer, emb, exact)
        with gc.CallSpy() as spy:
            loss = emb.fused_objective(StressLoss(), _dev(sc.targets(E2E_N), dname), None)
            loss.backward()
            grad = emb.xs[0].grad.clone()
            opt.step()
        assert spy.calls.count('mm_so_pdist_loss') == 1 and 'mm_so_pdist_bwd' not in spy.calls, spy.calls
        fused = 'mm_mat_rsgd_step' if optimizer == 'rsgd' else 'mm_mat_radam_step'
        if exact:
            assert fused not in spy.calls and 'mm_so_map' in spy.calls, spy.calls
        else:
            assert fused in spy.calls and 'mm_so_map' not in spy.calls, spy.calls
        q = sc.loss_quantities(regime, E2E_N, E2E_DIM, 'stress')
        sc.check(tag, 'so_e2e_loss', loss.reshape(1), q['loss'], dname, failures)
        sc.check(tag, 'so_e2e_grad', grad, q['grad_x'], dname, failures)
        sc.check(tag, 'so_e2e_x_new', emb.xs[0], sc.step_quantities(regime, E2E_N, E2E_DIM, optimizer, exact)['x_new'], dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('optimizer', ('rsgd', 'radam'))
@pytest.mark.parametrize('dname', DNAMES)
def test_three_steps_stay_on_the_group(dname, optimizer):
    """after three steps x^T x - I is within the rule's fp32 scale (16 2^-24, entries <= 1) and det = +1"""
    from graphembed.objectives import StressLoss
    emb = _embedding(dname, sc.points('spread', E2E_N, E2E_DIM))
    opt = _optimizer(optimizer, emb)
    tg = _dev(sc.targets(E2E_N), dname)
    for _ in range(3):
        opt.zero_grad()
        emb.fused_objective(StressLoss(), tg, None).backward()
        opt.step()
    x = emb.xs[0].detach()
    defect = sc.orth_defect(x)
    det = float((torch.linalg.det(x.double()) - 1).abs().max())
    print(f'so e2e {optimizer} {dname}: |x^T x - I| {defect:.3e}, |det - 1| {det:.3e} after three steps')
    assert defect <= 16 * sc.U32 and det <= E2E_DIM * 16 * sc.U32
    assert float((x - _dev(sc.points('spread', E2E_N, E2E_DIM), dname)).abs().max()) > 1e-3   # (and the points moved)


@pytest.mark.parametrize('dname', DNAMES)
def test_graphed_step_equals_the_eager_step(dname):
    """one captured and replayed step against the same step run eagerly, both against the oracle's step: the tolerance of the
    Grassmann step tests (grass_cases.check: e_new <= 2 e_old + 64 eps max|oracle| — the atomics' summation order)"""
    from graphembed.graphed import GraphedTrainStep
    from graphembed.objectives import StressLoss
    emb = _embedding(dname, sc.points('spread', E2E_N, E2E_DIM))
    emb.burnin(True)
    tg = _dev(sc.targets(E2E_N), dname)
    step = GraphedTrainStep(lambda: emb.fused_objective(StressLoss(), tg, None), [_optimizer('rsgd', emb)], warmup=1)
    with gc.CallSpy() as spy:
        step.capture()
    assert spy.calls.count('mm_so_pdist_loss') == 2 and spy.calls.count('mm_mat_rsgd_step') == 2, spy.calls   # warm-up + recording
    torch.cuda.synchronize()
    start = emb.xs[0].detach().clone()
    eager = _embedding(dname, start.double().cpu())
    opt = _optimizer('rsgd', eager)
    eager_loss = eager.fused_objective(StressLoss(), tg, None)
    eager_loss.backward()
    opt.step()
    want_loss, _, want_x = sc.oracle_step(start.double().cpu(), E2E_N, 'rsgd')
    with gc.CallSpy() as spy:
        last = step()
    assert spy.calls == [], spy.calls   # a replay launches the graph, nothing else
    torch.cuda.synchronize()
    failures = []
    gc.check(f'so graphed {dname}', 'x after the step', eager.xs[0], emb.xs[0], want_x, sc.DT[dname], failures)
    gc.check(f'so graphed {dname}', 'loss of the step', eager_loss.detach().reshape(1), last.reshape(1), want_loss, sc.DT[dname], failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('N', sc.DIMS)
def test_plain_stiefel_nn_polar_retraction_is_orthogonal_to_rounding(N):
    """Stiefel(n, n) itself (no SO class): the polar retraction of St(n, n) ends with a Newton-Schulz step (retr_op,
    csrc/mat_common.hpp), so the per-point map and the fused RSGD step return o^T o - I within 16 2^-24 in fp32 — the allowance of
    the three-step test above; without the step the polar factor carries ~17 eps (1.0e-6).  The result itself is held to the fp64
    port by tests/test_mat_oracle_gpu.py at (2,2), (3,3), (4,4); rectangular St(N, p) does not take the step."""
    import graphembed.manifolds as M
    import mat_cases as mc
    man = M.Stiefel(N, N)
    x, _, _, t, _ = mc.map_inputs('stiefel', 'uniform', N, N)
    xd, td = x.cuda(), t.cuda()
    with torch.no_grad():
        mapped = man.retr(xd, td)
    stepped = man.rsgd_step(xd, -td / sc.LR, lr=sc.LR)   # proju of a tangent is itself: the same move through mm_mat_rsgd_step
    assert stepped is not None
    for name, o in (('retr', mapped), ('rsgd_step', stepped)):
        defect = sc.orth_defect(o)
        print(f'stiefel {N}x{N} {name}: |o^T o - I| {defect:.3e} / {16 * sc.U32:.3e}')
        assert defect <= 16 * sc.U32, (name, defect)


def test_mixed_dtypes_are_refused():
    """one fp32 and one fp64 argument would both reach the kernel under the first one's dtype code"""
    man = _man(3)
    x = sc.points('spread', 4, 3).cuda()
    for call in (man.dist, man.log, man.exp):
        with pytest.raises(TypeError):
            call(x, x.double())


def test_print_worst_ratios():
    """(last in the file) the worst err / bound per quantity and dtype seen by the tests above: the table of profiles/so.md"""
    for (what, dname), (ratio, tag) in sorted(sc.RATIOS.items()):
        if what.startswith('so_'):
            print(f'{what:28s} {dname}: {ratio:.3f}  ({tag})')
            assert ratio <= 1.0, (what, dname, tag)
