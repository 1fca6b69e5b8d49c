"""The Stein-divergence fused objective and node-minibatch kernels on the GPU (csrc/spd_stein_loss.hpp; mm_spd_stein_pdiv_loss,
_loss_subset, _fwd_subset, _bwd_subset and the routes through SymmetricPositiveDefinite(use_stein_div=True), ManifoldEmbedding and
BatchedObjective) against the fp64 oracle of tests/stein_cases.py under grass_cases.check: e_new <= 2 e_old + 64 eps max|oracle|,
e_old the route the package took before these kernels (forward kernel, loss in torch ops, backward kernel — on gathered rows for a
batch), run on the same GPU in the same test.  The ratios are printed (-rA); the worst are in profiles/stein_loss.md."""
import pytest
import torch

import grass_cases as gc
import grass_subset_cases as gsc
import stein_cases as C
from grass_cases import CallSpy

pytestmark = pytest.mark.gpu
DNAMES = ('f32', 'f64')
NAMES = ('loss', 'grad_x', 'grad_scale')


def _B():
    from graphembed import _backend as B
    return B


def dev(t, dname):
    return t.to(C.DT[dname]).cuda().contiguous()


def workspace(dname, n, d, fill=None):
    B = _B()
    ws = torch.empty(B.lib().raw('mm_spd_pdist_ws_bytes')(B.MM_F32 if dname == 'f32' else B.MM_F64, n, d), dtype=torch.uint8, device='cuda')
    if fill is not None:
        ws.fill_(fill)
    return ws


def manifold(d):
    import graphembed.manifolds as M
    return M.SymmetricPositiveDefinite(d, use_stein_div=True, wmin=C.WMIN)


def raw_loss(dname, x, tg, loss_name, rows=None, scale=True, dyn=False, ws=None, idx=None):
    """mm_spd_stein_pdiv_loss (idx None: `tg` the target pair vector of the rows) or _loss_subset (`tg` the dense matrix); outputs
    pre-filled with NaN; returns (loss [1], grad_x, grad_scale [1])"""
    B = _B()
    xc, tc = (x if x.is_cuda else dev(x, dname)), dev(tg, dname)
    n, d = xc.shape[0], xc.shape[-1]
    m = n if idx is None else idx.numel()
    rb, re = (0, m) if rows is None else rows
    kind, alpha, eps, terms = C.loss_spec(loss_name)
    out = torch.full((2, ), float('nan'), dtype=xc.dtype, device='cuda')
    grad = torch.full_like(xc, float('nan'))
    sc = torch.tensor([C.SCALE_RAW], dtype=xc.dtype, device='cuda') if scale else None
    params = None
    if dyn:   # the by-value pair is garbage: the device array must win
        params, alpha, eps = torch.tensor([alpha, eps], dtype=torch.float64, device='cuda'), 123.0, 456.0
    ws = workspace(dname, n, d) if ws is None else ws
    if idx is None:
        B.lib().call('mm_spd_stein_pdiv_loss', B.dtype_code(xc), kind, B.ptr(xc), B.ptr(tc), B.ptr(sc), n, d, rb, re, alpha, eps, terms,
                     B.ptr(params), C.WMIN, B.ptr(out), B.ptr(grad), B.ptr(ws), 0, B.stream_of(xc))
    else:
        ic = idx.cuda()
        B.lib().call('mm_spd_stein_pdiv_loss_subset', B.dtype_code(xc), kind, B.ptr(xc), B.ptr(tc), B.ptr(sc), n, d, B.ptr(ic), m, rb, re,
                     alpha, eps, terms, B.ptr(params), C.WMIN, B.ptr(out), B.ptr(grad), B.ptr(ws), 0, B.stream_of(xc))
    torch.cuda.synchronize()
    return out[0:1].clone(), grad, out[1:2].clone()


def old_route(dname, x, tg_pairs, loss_name, idx=None, scale=True):
    """the route before the fused kernels: Stein forward kernel (on the gathered rows of a batch), the loss in torch ops, autograd
    through the Stein backward kernel"""
    xc = dev(x, dname).requires_grad_()
    s = torch.tensor(C.SCALE_RAW, dtype=xc.dtype, device='cuda', requires_grad=True)
    xb = xc if idx is None else xc[idx.cuda()]
    sp = torch.nn.functional.softplus(s) if scale else 1.0
    md = sp * manifold(x.shape[-1]).stein_pdiv(xb, squared=True)
    fn, kw = gc.objective(loss_name)
    loss = fn(dev(tg_pairs, dname), md, **kw)
    if scale:
        gx, gs = torch.autograd.grad(loss, [xc, s])
    else:
        (gx, ), gs = torch.autograd.grad(loss, [xc]), torch.zeros((), dtype=xc.dtype, device='cuda')
    return loss.detach().reshape(1), gx, gs.reshape(1)


def hold(tag, old, new, want, dname, failures):
    for name, o, g, w in zip(NAMES, old, new, want):
        C.check(tag, name, o, g, w, C.DT[dname], failures)


def outside_is_plus_zero(grad, idx):
    outside = torch.ones(grad.shape[0], dtype=torch.bool, device=grad.device)
    outside[idx.to(grad.device)] = False
    g = grad[outside]
    return bool((g == 0).all()) and not bool(torch.signbit(g).any())


# ---- 1. the full-batch objective ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', DNAMES)
def test_loss_every_size(dname):
    """D = 2 ... 9 (every instantiation), stress, n = 65, `spread`"""
    failures = []
    for d in C.DIMS_ALL:
        x, tg = C.points('spread', 65, d), C.targets('spread', 65, d)
        new = raw_loss(dname, x, tg, 'stress')
        assert all(bool(torch.isfinite(t).all()) for t in new)
        hold(f'stein loss d={d} {dname}', old_route(dname, x, tg, 'stress'), new, C.full_oracle('spread', 65, d, 'stress'), dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('d', C.DIMS)
@pytest.mark.parametrize('dname', DNAMES)
def test_loss_shapes_regimes_and_losses(dname, d):
    """n = 2, 3, 33, 65, 130, 257: the 32-row tile, the 64-column block, several blocks and the ragged last one"""
    failures = []
    for regime in C.REGIMES:
        for loss_name in C.LOSSES:
            for n in C.SIZES:
                x, tg = C.points(regime, n, d), C.targets(regime, n, d)
                new = raw_loss(dname, x, tg, loss_name)
                assert all(bool(torch.isfinite(t).all()) for t in new)
                hold(f'stein loss {regime} {loss_name} d={d} n={n} {dname}', old_route(dname, x, tg, loss_name), new,
                     C.full_oracle(regime, n, d, loss_name), dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
def test_scale_null_device_params_and_a_dirty_workspace(dname):
    d, failures = 3, []
    x, tg = C.points('spread', 65, d), C.targets('spread', 65, d)
    # scale_raw null: scale 1, no scale gradient
    xf = x.clone().requires_grad_(True)
    md = C.ref.SPD(d, wmin=C.WMIN).stein_pdiv(xf, squared=True)
    loss = C.ref.stress_loss(tg, md)
    gx, = torch.autograd.grad(loss, [xf])
    want = (loss.detach().reshape(1), 0.5 * (gx + gx.transpose(1, 2)), torch.zeros(1, dtype=torch.float64))
    new = raw_loss(dname, x, tg, 'stress', scale=False)
    assert float(new[2]) == 0.0
    hold(f'stein loss no scale {dname}', old_route(dname, x, tg, 'stress', scale=False), new, want, dname, failures)
    # {alpha, eps} on the device against by value: the same numbers (the atomics' order aside)
    by_value = raw_loss(dname, x, tg, 'quotient')
    on_device = raw_loss(dname, x, tg, 'quotient', dyn=True)
    hold(f'stein loss device params {dname}', by_value, on_device, C.full_oracle('spread', 65, d, 'quotient'), dname, failures)
    # a workspace left by a call of another size, and one full of 0xff bytes: every call prepares it itself
    ws = workspace(dname, 130, d, fill=0xff)
    raw_loss(dname, C.points('spread', 130, d), C.targets('spread', 130, d), 'quotient', ws=ws)
    dirty = raw_loss(dname, x, tg, 'quotient', ws=ws)
    hold(f'stein loss dirty workspace {dname}', by_value, dirty, C.full_oracle('spread', 65, d, 'quotient'), dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', DNAMES)
def test_row_shards_sum_to_the_whole(dname, loss_name):
    B = _B()
    d, n = 3, 130
    x, tg = C.points('spread', n, d), C.targets('spread', n, d)
    whole = raw_loss(dname, x, tg, loss_name)
    parts = [torch.zeros_like(t) for t in whole]
    for r in range(3):
        rb, re = B.shard_rows(n, 3, r)
        lo, hi = B.pair_offset(n, rb), B.pair_offset(n, re)
        part = raw_loss(dname, x, tg[lo:hi], loss_name, rows=(rb, re))
        for acc, t in zip(parts, part):
            acc += t
    eps = gc.eps_of(C.DT[dname])
    for name, a, b in zip(NAMES, parts, whole):
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f'stein shards {loss_name} {dname} {name}: {err:.3e} of {scale:.3e}')
        assert err <= 64 * eps * scale, (name, err, scale)
    empty = raw_loss(dname, x, tg[:0], loss_name, rows=(40, 40))
    assert all(float(t.abs().max()) == 0.0 for t in empty)
    last = raw_loss(dname, x, tg[:0], loss_name, rows=(n - 1, n))   # the last row has no pair
    assert all(float(t.abs().max()) == 0.0 for t in last)


@pytest.mark.parametrize('dname', DNAMES)
def test_coincident_points(dname):
    """two equal rows: S = 0 there, the clamp binds in the value and is transparent in the gradient; everything finite"""
    failures = []
    x = C.coincident_points()
    tg = C.targets('spread', 65, 3)
    for loss_name in C.LOSSES:
        new = raw_loss(dname, x, tg, loss_name)
        assert all(bool(torch.isfinite(t).all()) for t in new)
        hold(f'stein loss coincident {loss_name} {dname}', old_route(dname, x, tg, loss_name), new, C.objective_of(x, tg, loss_name), dname,
             failures)
    assert not failures, '\n'.join(failures)


# ---- 2. node minibatches: the raw entries ---------------------------------------------------------------------------------------------
def batch_targets(regime, d, bs):
    idx = C.batch_idx(bs)
    i, j = C.ref.triu_pairs(bs)
    return C.dense(regime, d, bs)[idx[i], idx[j]]


def perturbed(x, idx):
    """the table with every row OUTSIDE the batch replaced by another valid SPD matrix"""
    y = x.clone()
    outside = torch.ones(x.shape[0], dtype=torch.bool)
    outside[idx] = False
    y[outside] = 3.0 * x[outside].flip(0) + 0.5 * torch.eye(x.shape[-1], dtype=x.dtype)
    return y


@pytest.mark.parametrize('d', C.DIMS)
@pytest.mark.parametrize('dname', DNAMES)
def test_loss_subset(dname, d):
    failures = []
    for regime in C.REGIMES:
        x = C.points(regime, C.N_TOTAL, d)
        for bs in C.BATCHES:
            idx = C.batch_idx(bs)
            for loss_name in C.LOSSES:
                tag = f'stein subset {regime} {loss_name} d={d} bs={bs} {dname}'
                want = C.batch_oracle(regime, d, bs, loss_name)
                old = old_route(dname, x, batch_targets(regime, d, bs), loss_name, idx)
                new = raw_loss(dname, x, C.dense(regime, d, bs), loss_name, idx=idx)
                assert all(bool(torch.isfinite(t).all()) for t in new) and outside_is_plus_zero(new[1], idx), tag
                hold(tag, old, new, want, dname, failures)
                # the transposed targets are another problem (the matrix is not symmetric): the kernel reads dense[idx[a]][idx[b]]
                if bs == 65 and loss_name == 'stress':
                    swapped = raw_loss(dname, x, C.dense(regime, d, bs).T.contiguous(), loss_name, idx=idx)
                    assert abs(float(swapped[0]) - float(want[0])) > 1e-3 * abs(float(want[0]))
                # rows outside the batch do not matter
                if bs in (3, 65):
                    other = raw_loss(dname, perturbed(x, idx), C.dense(regime, d, bs), loss_name, idx=idx)
                    assert outside_is_plus_zero(other[1], idx), tag
                    hold(tag + ' (other rows outside)', old, other, want, dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
def test_loss_subset_row_shards_and_tiny_batches(dname):
    d, bs, regime = 3, 130, 'spread'
    x, idx, dm = C.points(regime, C.N_TOTAL, d), C.batch_idx(130), C.dense(regime, d, 130)
    eps = gc.eps_of(C.DT[dname])
    for loss_name in C.LOSSES:
        whole = raw_loss(dname, x, dm, loss_name, idx=idx)
        parts = [torch.zeros_like(t) for t in whole]
        for rows in gsc.COVER:
            for acc, t in zip(parts, raw_loss(dname, x, dm, loss_name, idx=idx, rows=rows)):
                acc += t
        for name, a, b in zip(NAMES, parts, whole):
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            print(f'stein subset shards {loss_name} {dname} {name}: {err:.3e} of {scale:.3e}')
            assert err <= 64 * eps * scale, (name, err, scale)
        for tiny in (idx[:0], idx[:1]):
            got = raw_loss(dname, x, dm, loss_name, idx=tiny)
            assert all(float(t.abs().max()) == 0.0 for t in got) and not bool(torch.signbit(got[1]).any())


def raw_pdiv_subset(dname, x, idx, squared, upstream=None, rows=None):
    """(pair vector, gradient of sum(upstream * value) or None) from mm_spd_stein_pdiv_fwd_subset / _bwd_subset"""
    B = _B()
    xc, ic = dev(x, dname), idx.cuda()
    n, d, bs = xc.shape[0], xc.shape[-1], idx.numel()
    rb, re = (0, bs) if rows is None else rows
    npairs = B.pair_offset(bs, re) - B.pair_offset(bs, rb) if bs >= 2 else 0
    out = torch.full((npairs, ), float('nan'), dtype=xc.dtype, device='cuda')
    ws = workspace(dname, n, d)
    B.lib().call('mm_spd_stein_pdiv_fwd_subset', B.dtype_code(xc), B.ptr(xc), n, d, B.ptr(ic), bs, rb, re, int(squared), C.WMIN,
                 B.ptr(out), B.ptr(ws), 0, B.stream_of(xc))
    grad = None
    if upstream is not None:
        grad = torch.full_like(xc, float('nan'))
        g = dev(upstream, dname)
        B.lib().call('mm_spd_stein_pdiv_bwd_subset', B.dtype_code(xc), B.ptr(xc), B.ptr(g), n, d, B.ptr(ic), bs, rb, re, int(squared),
                     C.WMIN, B.ptr(grad), B.ptr(ws), B.MM_WS_PREPARED, B.stream_of(xc))
    torch.cuda.synchronize()
    return out, grad


def old_pdiv(dname, x, idx, squared, upstream):
    xc = dev(x, dname).requires_grad_()
    v = manifold(x.shape[-1]).stein_pdiv(xc[idx.cuda()], squared=squared)
    gx, = torch.autograd.grad((v * dev(upstream, dname)).sum(), [xc])
    return v.detach(), gx


@pytest.mark.parametrize('d', C.DIMS)
@pytest.mark.parametrize('dname', DNAMES)
def test_pair_vector_of_a_batch(dname, d):
    failures = []
    x = C.points('spread', C.N_TOTAL, d)
    for bs in C.BATCHES:
        idx = C.batch_idx(bs)
        up = C.upstream(bs * (bs - 1) // 2)
        for squared in (True, False):
            tag = f'stein pdiv subset d={d} bs={bs} {"d2" if squared else "d"} {dname}'
            want_v, want_g = C.pdiv_oracle(x, idx, squared)
            old_v, old_g = old_pdiv(dname, x, idx, squared, up)
            new_v, new_g = raw_pdiv_subset(dname, x, idx, squared, up)
            assert outside_is_plus_zero(new_g, idx), tag
            C.check(tag, 'value', old_v, new_v, want_v, C.DT[dname], failures)
            C.check(tag, 'grad', old_g, new_g, want_g, C.DT[dname], failures)
            if bs == 65:   # rows outside the batch do not matter: the values bit for bit (no atomics), the gradient under the rule
                other_v, other_g = raw_pdiv_subset(dname, perturbed(x, idx), idx, squared, up)
                assert torch.equal(other_v, new_v) and outside_is_plus_zero(other_g, idx), tag
                C.check(tag + ' (other rows outside)', 'grad', old_g, other_g, want_g, C.DT[dname], failures)
    # row shards of the batch: the forward's slices bit for bit
    idx = C.batch_idx(130)
    whole, _ = raw_pdiv_subset(dname, x, idx, True)
    parts = [raw_pdiv_subset(dname, x, idx, True, rows=rows)[0] for rows in gsc.COVER]
    assert torch.equal(torch.cat(parts), whole)
    for tiny in (idx[:0], idx[:1]):
        v, g = raw_pdiv_subset(dname, x, tiny, True, torch.zeros(0, dtype=torch.float64))
        assert v.numel() == 0 and float(g.abs().max()) == 0.0
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
def test_a_repeated_node_accumulates(dname):
    """positions 7 and 40 name one node: its gradients accumulate, the pair of the node with itself is the clamp's value and adds
    nothing (squared: the form compute_dists uses)"""
    failures = []
    d, bs = 3, 65
    x = C.points('spread', C.N_TOTAL, d)
    idx = C.batch_idx(bs).clone()
    idx[40] = idx[7]
    up = C.upstream(bs * (bs - 1) // 2)
    want_v, want_g = C.pdiv_oracle(x, idx, True)
    k = _B().pair_offset(bs, 7) + 40 - 7 - 1
    assert float(want_v[k]) == C.WMIN
    old_v, old_g = old_pdiv(dname, x, idx, True, up)
    new_v, new_g = raw_pdiv_subset(dname, x, idx, True, up)
    assert bool(torch.isfinite(new_v).all()) and bool(torch.isfinite(new_g).all()) and outside_is_plus_zero(new_g, idx)
    C.check(f'stein pdiv subset repeated node {dname}', 'value', old_v, new_v, want_v, C.DT[dname], failures)
    C.check(f'stein pdiv subset repeated node {dname}', 'grad', old_g, new_g, want_g, C.DT[dname], failures)
    assert not failures, '\n'.join(failures)


# ---- 3. routes -------------------------------------------------------------------------------------------------------------------
def embedding(dname, x, manifolds=None):
    from graphembed.modules import ManifoldEmbedding
    dt = C.DT[dname]
    torch.set_default_dtype(dt)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(x.shape[0], manifolds if manifolds is not None else [manifold(x.shape[-1])])
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        emb.xs[-1].copy_(x.to(dt).cuda())
        for s in emb.scales:
            s.fill_(C.SCALE_RAW)
    return emb


def _dataset(dense):
    from graphembed.data import GraphDataset
    ds = GraphDataset(torch.ones(3, dtype=dense.dtype, device=dense.device))
    ds._dense = dense
    return ds


class _TakeRowsSpy:
    def __init__(self, monkeypatch):
        from graphembed import modules
        self.count, orig = 0, modules.take_rows

        def spy(x, i, validated=False):
            self.count += i is not None
            return orig(x, i, validated=validated)
        monkeypatch.setattr(modules, 'take_rows', spy)


OLD_STEIN = {'mm_spd_stein_pdiv_fwd', 'mm_spd_stein_pdiv_bwd', 'mm_product_loss'}


@pytest.mark.parametrize('dname', DNAMES)
def test_fused_objective_is_one_call(dname):
    """(fails without the feature: the objective is then mm_spd_stein_pdiv_fwd, mm_product_loss, mm_spd_stein_pdiv_bwd)"""
    from graphembed.objectives import StressLoss
    failures = []
    x, tg = C.points('spread', 65, 3), C.targets('spread', 65, 3)
    emb = embedding(dname, x)
    with CallSpy() as spy:
        loss = emb.fused_objective(StressLoss(), dev(tg, dname), None)
        loss.backward()
    assert spy.calls == ['mm_spd_stein_pdiv_loss'], spy.calls
    new = (loss.detach().reshape(1), emb.xs[0].grad, emb.scales[0].grad.reshape(1))
    hold(f'stein routed full batch {dname}', old_route(dname, x, tg, 'stress'), new, C.full_oracle('spread', 65, 3, 'stress'), dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', DNAMES)
def test_batched_objective_takes_the_in_kernel_route(dname, loss_name, monkeypatch):
    """(fails without mm_spd_stein_pdiv_loss_subset: the step then gathers — take_rows, the dataset's target gather)"""
    from graphembed.modules import BatchedObjective
    d, regime, bs, failures = 3, 'spread', 65, []
    x, idx = C.points(regime, C.N_TOTAL, d), C.batch_idx(bs).cuda()
    emb = embedding(dname, x)
    fn, kw = gc.objective(loss_name)
    objective = BatchedObjective(fn, _dataset(dev(C.dense(regime, d, bs), dname)), emb)
    want = C.batch_oracle(regime, d, bs, loss_name)
    old = old_route(dname, x, batch_targets(regime, d, bs), loss_name, idx.cpu())
    rows_spy = _TakeRowsSpy(monkeypatch)
    for where, indices in (('host', idx.cpu()), ('device', idx)):
        emb.zero_grad(set_to_none=True)
        with CallSpy() as spy:
            loss = objective(indices, **kw)
            loss.backward()
        assert spy.calls == ['mm_spd_stein_pdiv_loss_subset'] and rows_spy.count == 0, (spy.calls, rows_spy.count)
        new = (loss.detach().reshape(1), emb.xs[0].grad, emb.scales[0].grad.reshape(1))
        hold(f'stein routed batch ({where} indices) {loss_name} {dname}', old, new, want, dname, failures)
        assert outside_is_plus_zero(emb.xs[0].grad, idx)
    assert ('stein', C.DT[dname], emb.xs[0].device, C.N_TOTAL, d) in emb._pair_ws   # kept for the embedding's lifetime
    # repeated host-side indices: the gathered route, as before
    rep = idx.cpu().clone()
    rep[1] = rep[0]
    with CallSpy() as spy:
        loss = objective(rep, **kw)
    assert 'mm_spd_stein_pdiv_loss_subset' not in spy.calls and rows_spy.count == 1, spy.calls
    assert bool(torch.isfinite(loss))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
def test_the_pair_vector_objectives_take_the_in_kernel_route(dname, monkeypatch):
    """StochasticNeighborLoss consumes compute_dists(idx): forward and backward of the pair vector read the full table through the
    index vector (fails without mm_spd_stein_pdiv_fwd_subset: compute_dists then gathers and calls mm_spd_stein_pdiv_fwd)"""
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StochasticNeighborLoss
    d, bs = 3, 65
    x, idx = C.points('spread', C.N_TOTAL, d), C.batch_idx(bs).cuda()
    emb = embedding(dname, x)
    objective = BatchedObjective(StochasticNeighborLoss(), _dataset(dev(C.dense('spread', d, bs), dname)), emb)
    rows_spy = _TakeRowsSpy(monkeypatch)
    for indices in (idx.cpu(), idx):
        emb.zero_grad(set_to_none=True)
        with CallSpy() as spy:
            loss = objective(indices, alpha=1.3)
            forward = list(spy.calls)
            loss.backward()
        assert forward.count('mm_spd_stein_pdiv_fwd_subset') == 1 and 'mm_spd_stein_pdiv_bwd_subset' in spy.calls[len(forward):], spy.calls
        assert not OLD_STEIN & set(spy.calls) and rows_spy.count == 0, spy.calls
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(emb.xs[0].grad).all()) and outside_is_plus_zero(emb.xs[0].grad, idx)
    # the distances themselves against the raw entry, and all nodes: the full-batch kernel, as before
    with CallSpy() as spy:
        d2 = emb.compute_dists(idx)
    assert spy.calls == ['mm_spd_stein_pdiv_fwd_subset'], spy.calls
    raw, _ = raw_pdiv_subset(dname, x, idx.cpu(), True)
    assert torch.equal(d2.detach(), torch.nn.functional.softplus(emb.scales[0].detach()) * raw)
    with CallSpy() as spy:
        emb.compute_dists(None)
    assert spy.calls == ['mm_spd_stein_pdiv_fwd'], spy.calls


# the calls these two objectives issued before the Stein hooks existed, recorded on the parent commit (MI355X, this test's code)
PLAIN_SPD_CALLS = ['mm_spd_pdist_loss']
PRODUCT_WITH_STEIN_CALLS = ['mm_vec_pdist_fwd', 'mm_spd_stein_pdiv_fwd', 'mm_product_loss', 'mm_vec_pdist_bwd_gram', 'mm_spd_stein_pdiv_bwd']


def test_other_embeddings_issue_the_calls_they_issued_before():
    import graphembed.manifolds as M
    from graphembed.objectives import StressLoss
    x, tg = C.points('spread', 65, 3), C.targets('spread', 65, 3)
    emb = embedding('f32', x, [M.SymmetricPositiveDefinite(3)])
    with CallSpy() as spy:
        emb.fused_objective(StressLoss(), dev(tg, 'f32'), None).backward()
    print('plain SPD:', spy.calls)
    assert spy.calls == PLAIN_SPD_CALLS, spy.calls
    emb = embedding('f32', x, [M.Euclidean(4), manifold(3)])
    with CallSpy() as spy:
        emb.fused_objective(StressLoss(), dev(tg, 'f32'), None).backward()
    print('Euclidean x Stein:', spy.calls)
    # (with the C++ autograd nodes loaded the vector factor's two calls are issued from C++, past the spy — then as before)
    want = PRODUCT_WITH_STEIN_CALLS if _B().autograd_ext() is None else [c for c in PRODUCT_WITH_STEIN_CALLS if not c.startswith('mm_vec_')]
    assert spy.calls == want, spy.calls


# ---- 4. one training step --------------------------------------------------------------------------------------------------------
def _optimizer(name, emb):
    from graphembed.optim import RiemannianAdam, RiemannianSGD
    if name == 'rsgd':
        return RiemannianSGD(list(emb.xs), lr=C.STEP['lr'])
    return RiemannianAdam(list(emb.xs), lr=C.STEP['lr'], betas=(0.9, 0.999))


def _step_case(batch):
    """(x, target pairs fp64, idx or None, dense fp32 or None) of the step tests"""
    d, n, bs = C.STEP['d'], C.STEP['n'], C.STEP['bs']
    x = C.points('spread', n, d)
    if not batch:
        return x, C.targets('spread', n, d), None, None
    idx = gsc.batch_idx(n, bs)
    i, j = C.ref.triu_pairs(bs)
    dm = (gsc.raw_dense(n).double() * C.model_dists(x, idx).median()).float()
    return x, dm[idx[i], idx[j]].double(), idx, dm


@pytest.mark.parametrize('batch', (False, True), ids=('full', 'batch33'))
@pytest.mark.parametrize('optimizer', ('rsgd', 'radam'))
@pytest.mark.parametrize('dname', DNAMES)
def test_one_training_step(dname, optimizer, batch):
    """fused objective, backward and one optimizer step against ref.rsgd_step / ref.radam_step on ref_port.SPD(3) with the oracle's
    gradient; e_old: the same step with the unfused objective"""
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    failures = []
    x, tgp, idx, dm = _step_case(batch)
    want_loss, want_g, _ = C.objective_of(x, tgp, 'stress', idx)
    want_x = C.step_oracle(x, want_g, optimizer)
    # the unfused step
    old = embedding(dname, x)
    opt = _optimizer(optimizer, old)
    xb = old.xs[0] if idx is None else old.xs[0][idx.cuda()]
    md = torch.nn.functional.softplus(old.scales[0]) * old.manifolds[0].stein_pdiv(xb, squared=True)
    old_loss = StressLoss()(dev(tgp, dname), md)
    old_loss.backward()
    old_grad = old.xs[0].grad.clone()
    opt.step()
    # the fused step
    emb = embedding(dname, x)
    opt = _optimizer(optimizer, emb)
    with CallSpy() as spy:
        if idx is None:
            loss = emb.fused_objective(StressLoss(), dev(tgp, dname), None)
        else:
            loss = BatchedObjective(StressLoss(), _dataset(dev(dm, dname)), emb)(idx.cuda())
        loss.backward()
        grad = emb.xs[0].grad.clone()
        opt.step()
    assert spy.calls[0] == ('mm_spd_stein_pdiv_loss' if idx is None else 'mm_spd_stein_pdiv_loss_subset'), spy.calls
    assert not OLD_STEIN & set(spy.calls), spy.calls
    assert spy.calls[1:] == ['mm_spd_rsgd_step' if optimizer == 'rsgd' else 'mm_spd_radam_step'], spy.calls
    tag = f'stein step {optimizer} {"batch" if batch else "full"} {dname}'
    C.check(tag, 'loss', old_loss.detach().reshape(1), loss.detach().reshape(1), want_loss, C.DT[dname], failures)
    C.check(tag, 'grad_x', old_grad, grad, want_g, C.DT[dname], failures)
    C.check(tag, 'x_new', old.xs[0], emb.xs[0], want_x, C.DT[dname], failures)
    assert float((emb.xs[0].detach().double().cpu() - x).abs().max()) > 1e-4   # (and the points moved)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('batch', (False, True), ids=('full', 'batch33'))
@pytest.mark.parametrize('dname', DNAMES)
def test_captured_step_equals_the_eager_step(dname, batch):
    """fused Stein objective + RSGD captured once and replayed once against the same step run eagerly, both against the oracle's
    step; a replay issues no library call.  The minibatch step reads a device-side index buffer."""
    from graphembed.graphed import GraphedTrainStep
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    x, tgp, idx, dm = _step_case(batch)

    def build(points):
        emb = embedding(dname, points)
        emb.burnin(True)
        if idx is None:
            tg = dev(tgp, dname)
            return emb, (lambda: emb.fused_objective(StressLoss(), tg, None))
        buf = idx.cuda().clone()
        objective = BatchedObjective(StressLoss(), _dataset(dev(dm, dname)), emb)
        return emb, (lambda: objective(buf))
    emb, closure = build(x)
    step = GraphedTrainStep(closure, [_optimizer('rsgd', emb)], warmup=1)
    entry = 'mm_spd_stein_pdiv_loss' if idx is None else 'mm_spd_stein_pdiv_loss_subset'
    with CallSpy() as spy:
        step.capture()
    assert spy.calls.count(entry) == 2 and spy.calls.count('mm_spd_rsgd_step') == 2 and not OLD_STEIN & set(spy.calls), spy.calls
    torch.cuda.synchronize()
    start = emb.xs[0].detach().double().cpu()
    eager, eager_closure = build(start)
    opt = _optimizer('rsgd', eager)
    eager_loss = eager_closure()
    eager_loss.backward()
    opt.step()
    want_loss, want_g, _ = C.objective_of(start, tgp, 'stress', idx)
    want_x = C.step_oracle(start, want_g, 'rsgd')
    with CallSpy() as spy:
        last = step()
    assert spy.calls == [], spy.calls
    torch.cuda.synchronize()
    failures = []
    tag = f'stein captured {"batch" if batch else "full"} {dname}'
    C.check(tag, 'x after the step', eager.xs[0], emb.xs[0], want_x, C.DT[dname], failures)
    C.check(tag, 'loss of the step', eager_loss.detach().reshape(1), last.reshape(1), want_loss, C.DT[dname], failures)
    assert not failures, '\n'.join(failures)


def test_print_worst_ratios():
    """(last in the file) the worst e_new / max(e_old, floor) per test tag: the table of profiles/stein_loss.md"""
    worst = sorted(((r, t) for t, r in gc.RATIOS.items() if t.startswith('stein')), reverse=True)[:12]
    for r, t in worst:
        print(f'{r:8.3f}  {t}')
