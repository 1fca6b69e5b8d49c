"""The SO(n) node-minibatch kernels on the GPU (csrc/so.hip with SUB: mm_so_pdist_fwd_subset, mm_so_pdist_bwd_subset,
mm_so_pdist_loss_subset; SpecialOrthogonal.pdist_subset / pdist_loss_subset and the routes through ManifoldEmbedding.compute_dists,
fused_objective and BatchedObjective), n = 2 .. 4, fp32 and fp64, against the long-double oracle under the absolute rule of
tests/mat_cases.py on the cases of tests/so_subset_cases.py (which tests/test_so_subset_host.py holds to bound_f32 <= 1e-3 S on the
CPU).  Every comparison prints err / bound (-rA); the worst ratios are in profiles/so_minibatch.md."""
import pytest
import torch

import grass_cases as gc
import so_subset_cases as C
from grass_cases import CallSpy
from graphembed import _backend as B

pytestmark = pytest.mark.gpu
sc = C.sc
DNAMES = ('f32', 'f64')

_WS = {}


def _ws(dt, n, N, loss):
    """ONE workspace per table shape for the whole session, first filled with ones: every call clears it itself"""
    key = (dt, n, N, loss)
    if key not in _WS:
        sizer = 'mm_so_pdist_loss_ws_bytes' if loss else 'mm_so_pdist_ws_bytes'
        nbytes = B.lib().raw(sizer)(B.MM_F64 if dt == torch.float64 else B.MM_F32, n, N)
        _WS[key] = torch.ones(nbytes // torch.empty(0, dtype=dt).element_size(), dtype=dt, device='cuda')
    return _WS[key]


def _nan(*shape, dt):
    return torch.full(shape, float('nan'), dtype=dt, device='cuda')


def _sr(x):
    return torch.tensor([sc.SCALE_RAW], dtype=x.dtype, device=x.device)


def abi_loss(x, dense, idx, loss_name, rows=None, bs=None, grad=None):
    """(loss, grad_x, grad_scale) of one mm_so_pdist_loss_subset call; the outputs are pre-filled with NaN"""
    n_total, N = x.shape[0], x.shape[-1]
    bs = idx.numel() if bs is None else bs
    rb, re = (0, bs) if rows is None else rows
    kind, alpha, eps, terms = C.loss_spec(loss_name)
    out = _nan(2, dt=x.dtype)
    grad = torch.full_like(x, float('nan')) if grad is None else grad
    B.lib().call('mm_so_pdist_loss_subset', B.dtype_code(x), kind, B.ptr(x), B.ptr(dense), B.ptr(_sr(x)), n_total, N,
                 None if idx is None else B.ptr(idx), bs, rb, re, alpha, eps, terms, None, B.ptr(out), B.ptr(grad),
                 B.ptr(_ws(x.dtype, n_total, N, True)), B.stream_of(x))
    return out[:1], grad, out[1:]


def abi_fwd(x, idx, squared, rows=None, bs=None, out=None):
    n_total, N = x.shape[0], x.shape[-1]
    bs = idx.numel() if bs is None else bs
    rb, re = (0, bs) if rows is None else rows
    lo, hi = C.pair_slice(bs, (rb, re)) if bs >= 2 else (0, 0)
    out = _nan(hi - lo, dt=x.dtype) if out is None else out
    B.lib().call('mm_so_pdist_fwd_subset', B.dtype_code(x), B.ptr(x), n_total, N, None if idx is None else B.ptr(idx), bs, rb, re,
                 int(squared), B.ptr(out) if out.numel() else None, B.stream_of(x))
    return out


def abi_bwd(x, g, idx, squared, rows=None, bs=None, grad=None):
    n_total, N = x.shape[0], x.shape[-1]
    bs = idx.numel() if bs is None else bs
    rb, re = (0, bs) if rows is None else rows
    grad = torch.full_like(x, float('nan')) if grad is None else grad
    B.lib().call('mm_so_pdist_bwd_subset', B.dtype_code(x), B.ptr(x), None if g is None or not g.numel() else B.ptr(g), n_total, N,
                 None if idx is None else B.ptr(idx), bs, rb, re, int(squared), B.ptr(grad), B.ptr(_ws(x.dtype, n_total, N, False)),
                 B.stream_of(x))
    return grad


def table(regime, N, dname):
    return C.points(regime, C.N_TOTAL, N).to(sc.DT[dname]).cuda()


def inputs(regime, N, bs, dname):
    dt = sc.DT[dname]
    return table(regime, N, dname), C.dense(regime, N, bs).to(dt).cuda(), C.batch_idx(bs).cuda()


def upstream(k, dname):
    return C.upstream(k).to(sc.DT[dname]).cuda()


def hold(tag, got, q, rows, dname, failures):
    for name, g in zip(('loss', 'grad_x', 'grad_scale'), got):
        C.check(tag, f'so_subset_{name}', g, C.held(q[(rows, name)]), dname, failures)


def outside_is_plus_zero(grad, idx):
    mask = torch.ones(grad.shape[0], dtype=torch.bool, device=grad.device)
    mask[idx] = False
    rest = grad[mask]
    return rest.numel() > 0 and bool((rest == 0).all()) and not bool(torch.signbit(rest).any())


# ---- 1. every case against the oracle through the C ABI ----------------------------------------------------------------------------
@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_objective_cases_against_the_oracle(N, dname, loss_name):
    failures = []
    for regime in C.REGIMES:
        for bs in C.BATCHES:
            x, dense, idx = inputs(regime, N, bs, dname)
            got = abi_loss(x, dense, idx, loss_name)
            tag = f'so subset {N} {regime} bs={bs} {loss_name}'
            hold(tag, got, C.loss_quantities(regime, N, bs, loss_name), None, dname, failures)
            assert outside_is_plus_zero(got[1], idx), tag
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_pair_vector_cases_against_the_oracle(N, dname):
    failures = []
    for regime in C.REGIMES:
        for bs in C.BATCHES:
            x, _, idx = inputs(regime, N, bs, dname)
            for squared in (True, False):
                q = C.pdist_quantities(regime, N, bs, squared)
                val = abi_fwd(x, idx, squared)
                grad = abi_bwd(x, upstream(val.numel(), dname), idx, squared)
                tag, what = f'so subset pdist {N} {regime} bs={bs}', 'd2' if squared else 'd'
                got = {'val': val, 'grad': grad}
                for name in C.pdist_compared(regime, squared):
                    C.check(tag, f'so_subset_pdist_{what}_{name}', got[name], C.held(q[name]), dname, failures)
                assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(grad).all()), (tag, squared)
                assert outside_is_plus_zero(grad, idx), (tag, squared)
    assert not failures, '\n'.join(failures)


# ---- 2. row shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_row_shards_of_the_objective(N, dname, loss_name):
    """every range of SHARDS against the oracle of its pairs; the parts of COVER sum to the whole within the summed bounds"""
    bs, failures = 130, []
    for regime in C.REGIMES:
        x, dense, idx = inputs(regime, N, bs, dname)
        q = C.loss_quantities(regime, N, bs, loss_name)
        parts = {}
        for rows in C.SHARDS:
            got = abi_loss(x, dense, idx, loss_name, rows)
            tag = f'so subset shard {N} {regime} rows={rows} {loss_name}'
            assert outside_is_plus_zero(got[1], idx), tag
            if (rows, 'loss') in q:
                hold(tag, got, q, rows, dname, failures)
            else:   # no pair in the range: a zero gradient and {0, 0}
                assert all(torch.equal(g, torch.zeros_like(g)) for g in got), tag
            parts[rows] = got
        for k, name in enumerate(('loss', 'grad_x', 'grad_scale')):
            total = sum(parts[r][k].double().cpu() for r in C.COVER)
            bound = sum(C.held(q[(r, name)]).bound(dname) for r in C.COVER if (r, name) in q)
            err = float((total - q[(None, name)].want).abs().max())
            print(f'so subset cover {N} {regime} {loss_name} {name} {dname}: err {err:.3e} / summed bounds {bound:.3e}')
            if not err <= bound:
                failures.append(f'cover {N} {regime} {loss_name} {name}: {err:.3e} > {bound:.3e}')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_row_shards_of_the_pair_vector(N, dname):
    """the shards of ONE upstream vector over COVER: values concatenate to the full range's bit for bit (a pair is the same
    arithmetic in every tile), gradients add up to the full range's under its bound; ranges without a pair write nothing / zeros"""
    bs, failures = 130, []
    for regime in C.REGIMES:
        x, _, idx = inputs(regime, N, bs, dname)
        for squared in (True, False):
            q = C.pdist_quantities(regime, N, bs, squared)
            whole = abi_fwd(x, idx, squared)
            g = upstream(whole.numel(), dname)
            vals, total = [], torch.zeros_like(x)
            for rows in C.COVER + ((5, 5), ):
                lo, hi = C.pair_slice(bs, rows)
                vals.append(abi_fwd(x, idx, squared, rows))
                grad = abi_bwd(x, g[lo:hi].contiguous(), idx, squared, rows)
                assert vals[-1].numel() == hi - lo and outside_is_plus_zero(grad, idx), rows
                if lo == hi:
                    assert torch.equal(grad, torch.zeros_like(grad)), rows
                total += grad
            assert torch.equal(torch.cat(vals), whole), (regime, squared)
            if 'grad' in C.pdist_compared(regime, squared):
                C.check(f'so subset pdist {N} {regime} shards', f'so_subset_pdist_{"d2" if squared else "d"}_grad@sum', total,
                        C.held(q['grad']), dname, failures)
    assert not failures, '\n'.join(failures)


# ---- 3. the full-batch kernels on the gathered rows --------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_the_full_batch_kernels_on_the_gathered_batch_are_held_to_the_same_quantities(N, dname):
    """(not bitwise: both sum through float atomics)"""
    import graphembed.manifolds as M
    man, failures = M.SpecialOrthogonal(N), []
    for regime in C.REGIMES:
        for bs in (65, 130):
            x, dense, idx = inputs(regime, N, bs, dname)
            i, j = (t.cuda() for t in torch.triu_indices(bs, bs, 1))
            xb, tg = x[idx].contiguous(), dense[idx[i], idx[j]].contiguous()
            for loss_name in C.LOSSES:
                kind, alpha, eps, terms = C.loss_spec(loss_name)
                out, grad = _nan(2, dt=x.dtype), torch.full_like(xb, float('nan'))
                B.lib().call('mm_so_pdist_loss', B.dtype_code(x), kind, B.ptr(xb), B.ptr(tg), B.ptr(_sr(x)), bs, N, 0, bs, alpha, eps, terms,
                             None, B.ptr(out), B.ptr(grad), B.ptr(_ws(x.dtype, bs, N, True)), B.stream_of(x))
                full = torch.zeros_like(x)
                full[idx] = grad
                hold(f'so gathered {N} {regime} bs={bs} {loss_name}', (out[:1], full, out[1:]), C.loss_quantities(regime, N, bs, loss_name),
                     None, dname, failures)
            for squared in (True, False):
                q = C.pdist_quantities(regime, N, bs, squared)
                xs = xb.clone().requires_grad_(True)
                val = man.pdist(xs, squared=squared)
                (val * upstream(val.numel(), dname)).sum().backward()
                full = torch.zeros_like(x)
                full[idx] = xs.grad
                got = {'val': val.detach(), 'grad': full}
                for name in C.pdist_compared(regime, squared):
                    C.check(f'so gathered pdist {N} {regime} bs={bs}', f'so_subset_pdist_{"d2" if squared else "d"}_{name}', got[name],
                            C.held(q[name]), dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_the_identity_batch_is_the_full_batch_forward_bit_for_bit(N, dname):
    """idx = 0 .. n_total - 1: the SUB = true and the SUB = false forward walk the same pairs of the same points with the same
    arithmetic, one store per pair and no atomics.  n_total = 300: a second 256-wide column block, ragged; the row range
    (17, 200) starts and ends inside a 16-row tile"""
    n_total = 300
    x = C.points('spread', n_total, N).to(sc.DT[dname]).cuda()
    idx = torch.arange(n_total, dtype=torch.int64, device='cuda')
    for squared in (True, False):
        for rows in ((0, n_total), (17, 200)):
            lo, hi = C.pair_slice(n_total, rows)
            full = _nan(hi - lo, dt=x.dtype)
            B.lib().call('mm_so_pdist_fwd', B.dtype_code(x), B.ptr(x), n_total, N, rows[0], rows[1], int(squared), B.ptr(full),
                         B.stream_of(x))
            sub = abi_fwd(x, idx, squared, rows)
            assert bool(torch.isfinite(full).all()) and torch.equal(sub, full), (squared, rows)


# ---- 4. index hygiene ----------------------------------------------------------------------------------------------------------------
def _guarded(shape, dt, pad=64):
    """a NaN-filled buffer of `shape` with NaN guard rows before and after it: (whole, view)"""
    whole = _nan(shape[0] + 2 * pad, *shape[1:], dt=dt)
    return whole, whole[pad:pad + shape[0]]


def _guards_untouched(whole, pad=64):
    return bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[-pad:]).all())


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_index_hygiene(N, dname):
    """the kernels read the low 32-bit word of an index and clamp the node id into the table"""
    regime, bs, failures = 'spread', 65, []
    x, dense, idx = inputs(regime, N, bs, dname)
    high = torch.arange(bs, dtype=torch.int64, device='cuda') % 5 - 2     # -2 .. 2: negative and positive high words
    poisoned = (idx + (high << 32)).contiguous()
    assert torch.equal(poisoned & 0xffffffff, idx) and not torch.equal(poisoned, idx)
    hold(f'so subset poisoned high words {N}', abi_loss(x, dense, poisoned, 'stress'), C.loss_quantities(regime, N, bs, 'stress'), None,
         dname, failures)
    q = C.pdist_quantities(regime, N, bs, True)
    val = abi_fwd(x, poisoned, True)
    C.check(f'so subset poisoned high words {N}', 'so_subset_pdist_d2_val', val, q['val'], dname, failures)
    C.check(f'so subset poisoned high words {N}', 'so_subset_pdist_d2_grad', abi_bwd(x, upstream(val.numel(), dname), poisoned, True),
            q['grad'], dname, failures)
    # low words outside the table: clamped (wrong numbers for that batch, never an access outside the buffers)
    wild = idx.clone()
    wild[3], wild[4], wild[5] = C.N_TOTAL + 5, -7, 0x7fffffff
    whole, grad = _guarded(x.shape, x.dtype)
    got = abi_loss(x, dense, wild, 'quotient', grad=grad)
    assert all(bool(torch.isfinite(g).all()) for g in got) and _guards_untouched(whole)
    whole, out = _guarded((bs * (bs - 1) // 2, ), x.dtype)
    abi_fwd(x, wild, False, out=out)
    assert bool(torch.isfinite(out).all()) and _guards_untouched(whole)
    whole, grad = _guarded(x.shape, x.dtype)
    abi_bwd(x, upstream(out.numel(), dname), wild, False, grad=grad)
    assert bool(torch.isfinite(grad).all()) and _guards_untouched(whole)
    assert not failures, '\n'.join(failures)


# ---- 5. a repeated node in the pair-vector route -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('N', C.DIMS)
def test_a_repeated_node_accumulates(N, dname):
    """positions 7 and 40 name the same node: that pair is exactly 0 in both forms, its gradient is zero, and the node's row
    collects the contributions of both positions"""
    failures = []
    x = table(C.REPEAT['regime'], N, dname)
    idx = C.batch_idx(C.REPEAT['bs'], True).cuda()
    for squared in (True, False):
        q = C.pdist_quantities(C.REPEAT['regime'], N, C.REPEAT['bs'], squared, True)
        val = abi_fwd(x, idx, squared)
        grad = abi_bwd(x, upstream(val.numel(), dname), idx, squared)
        assert float(val[C.repeat_pair()]) == 0.0
        what = 'd2' if squared else 'd'
        C.check(f'so subset pdist {N} repeated node', f'so_subset_repeat_{what}_val', val, q['val'], dname, failures)
        C.check(f'so subset pdist {N} repeated node', f'so_subset_repeat_{what}_grad', grad, q['grad'], dname, failures)
        assert outside_is_plus_zero(grad, idx)
    assert not failures, '\n'.join(failures)


# ---- 6. nothing to do ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', DNAMES)
def test_batches_and_ranges_without_pairs(dname):
    N = 3
    x, dense, idx = inputs('spread', N, 65, dname)
    zero = torch.zeros_like(x)
    for bs, rows, ix in ((0, None, None), (1, None, idx), (65, (5, 5), idx), (65, (64, 65), idx), (65, (65, 65), None)):
        out = _nan(8, dt=x.dtype)
        for squared in (True, False):
            abi_fwd(x, ix, squared, rows, bs, out=out)
            assert bool(torch.isnan(out).all()), (bs, rows)                       # the forward writes nothing
            grad = abi_bwd(x, None, ix, squared, rows, bs)
            assert torch.equal(grad, zero) and not bool(torch.signbit(grad).any()), (bs, rows)
        for loss_name in C.LOSSES:
            loss, grad, gs = abi_loss(x, dense if ix is not None else None, ix, loss_name, rows, bs)
            assert torch.equal(grad, zero) and float(loss) == 0.0 and float(gs) == 0.0, (bs, rows, loss_name)


# ---- 7. routes -----------------------------------------------------------------------------------------------------------------------
def _embedding(dname, N, x):
    import graphembed.manifolds as M
    from graphembed.modules import ManifoldEmbedding
    dt = sc.DT[dname]
    torch.set_default_dtype(dt)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(C.N_TOTAL, [M.SpecialOrthogonal(N)])
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        emb.xs[0].copy_(x.to(dt).cuda())
        emb.scales[0].fill_(sc.SCALE_RAW)
    return emb


def _dataset(dense):
    """a GraphDataset on the GPU whose dense matrix is the case's (asymmetric) one"""
    from graphembed.data import GraphDataset
    ds = GraphDataset(torch.ones(3, dtype=dense.dtype, device=dense.device))
    ds._dense = dense
    return ds


class _TakeRowsSpy:
    """counts the row gathers of graphembed.modules (take_rows with an index vector)"""

    def __init__(self, monkeypatch):
        from graphembed import modules
        self.count, orig = 0, modules.take_rows

        def spy(x, i, validated=False):
            self.count += i is not None
            return orig(x, i, validated=validated)
        monkeypatch.setattr(modules, 'take_rows', spy)


@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', DNAMES)
def test_batched_objective_takes_the_in_kernel_route(dname, loss_name, monkeypatch):
    """(fails without mm_so_pdist_loss_subset: the step then gathers — take_rows, mm_pair_gather, mm_so_pdist_loss)"""
    from graphembed.modules import BatchedObjective
    N, regime, bs, failures = 3, 'spread', 65, []
    x, dense, idx = inputs(regime, N, bs, dname)
    emb = _embedding(dname, N, C.points(regime, C.N_TOTAL, N))
    fn, kw = gc.objective(loss_name)
    objective = BatchedObjective(fn, _dataset(dense), emb)
    q = C.loss_quantities(regime, N, bs, loss_name)
    rows_spy = _TakeRowsSpy(monkeypatch)
    for where, indices in (('host', idx.cpu()), ('device', idx)):
        emb.zero_grad(set_to_none=True)
        with CallSpy() as spy:
            loss = objective(indices, **kw)
            loss.backward()
        assert spy.calls == ['mm_so_pdist_loss_subset'] and rows_spy.count == 0, (spy.calls, rows_spy.count)
        hold(f'so subset routed ({where} indices) {N} {regime} bs={bs} {loss_name}',
             (loss.reshape(1), emb.xs[0].grad, emb.scales[0].grad.reshape(1)), q, None, dname, failures)
        assert outside_is_plus_zero(emb.xs[0].grad, idx)
    assert ('so loss', sc.DT[dname], emb.xs[0].device, C.N_TOTAL, N) in emb._pair_ws   # kept for the embedding's lifetime
    # repeated host-side indices: the gather route, as before
    rep = idx.cpu().clone()
    rep[1] = rep[0]
    with CallSpy() as spy:
        loss = objective(rep, **kw)
    assert 'mm_so_pdist_loss_subset' not in spy.calls and 'mm_so_pdist_loss' in spy.calls and rows_spy.count == 1, spy.calls
    assert bool(torch.isfinite(loss))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', DNAMES)
def test_the_pair_vector_objectives_take_the_in_kernel_route(dname, monkeypatch):
    """StochasticNeighborLoss consumes compute_dists(idx): forward and backward of the pair vector read the full table through
    the index vector (fails without mm_so_pdist_fwd_subset: compute_dists then gathers and calls mm_so_pdist_fwd)"""
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StochasticNeighborLoss
    s, failures = C.SNE, []
    N, bs = s['N'], s['bs']
    dt = sc.DT[dname]
    idx = C.batch_idx(bs).cuda()
    emb = _embedding(dname, N, C.points(s['regime'], C.N_TOTAL, N))
    objective = BatchedObjective(StochasticNeighborLoss(), _dataset(C.gsc.raw_dense(C.N_TOTAL).to(dt).cuda()), emb)
    q = C.sne_quantities()
    rows_spy = _TakeRowsSpy(monkeypatch)
    for where, indices in (('host', idx.cpu()), ('device', idx)):
        emb.zero_grad(set_to_none=True)
        with CallSpy() as spy:
            loss = objective(indices, alpha=s['alpha'])
            forward = list(spy.calls)
            loss.backward()
        assert forward.count('mm_so_pdist_fwd_subset') == 1 and spy.calls[len(forward):] == ['mm_so_pdist_bwd_subset'], spy.calls
        assert not {'mm_so_pdist_fwd', 'mm_so_pdist_bwd', 'mm_so_pdist_loss'} & set(spy.calls) and rows_spy.count == 0, spy.calls
        tag = f'so subset sne ({where} indices) {dname}'
        for name, got in (('loss', loss.reshape(1)), ('grad_x', emb.xs[0].grad), ('grad_scale', emb.scales[0].grad.reshape(1))):
            C.check(tag, f'so_subset_sne_{name}', got, q[name], dname, failures)
        assert outside_is_plus_zero(emb.xs[0].grad, idx)
    # compute_dists itself, with a repeated host-side node: no distinctness gate on this route
    rep = C.batch_idx(C.REPEAT['bs'], True)
    with CallSpy() as spy:
        d2 = emb.compute_dists(rep)
    assert spy.calls == ['mm_so_pdist_fwd_subset'] and rows_spy.count == 0, spy.calls
    raw = abi_fwd(emb.xs[0].detach(), rep.cuda(), True)     # (held to the oracle by test_a_repeated_node_accumulates)
    assert torch.equal(d2.detach(), torch.nn.functional.softplus(emb.scales[0].detach()) * raw)
    assert float(d2[C.repeat_pair()]) == 0.0
    with CallSpy() as spy:   # all nodes: the full-batch kernel, as before
        emb.compute_dists(None)
    assert spy.calls == ['mm_so_pdist_fwd'], spy.calls
    assert not failures, '\n'.join(failures)


# ---- 8. two minibatch training steps -----------------------------------------------------------------------------------------------
def _training(dname):
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    from graphembed.optim import RiemannianAdam
    t = C.TRAIN
    dt = sc.DT[dname]
    emb = _embedding(dname, t['N'], C.points(t['regime'], C.N_TOTAL, t['N']))
    emb.burnin(True)   # the scale stays put: the step is the points'
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=t['lr'], betas=C.BETAS, exact=False, max_grad_norm=t['clip'])])
    return emb, opt, BatchedObjective(StressLoss(), _dataset(C.gsc.raw_dense(C.N_TOTAL).to(dt).cuda()), emb)


def _after(emb, opt):
    st = opt.state[emb.xs[0]]
    assert float(st['step']) == 3.0
    return emb.xs[0].detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()


@pytest.mark.parametrize('dname', DNAMES)
def test_two_minibatch_steps_eager_and_replayed(dname):
    """fused objective -> RiemannianAdam (retraction) on two batches that share 30 nodes: points and both moments against
    oracle/ref_port.py's radam_step; then the same two steps with the first as the warm-up of a capture and the second as a replay
    of the recorded step after the device index buffer has been refilled"""
    from graphembed.graphed import GraphedTrainStep
    b1, b2 = (b.cuda() for b in C.train_batches())
    q = C.train_quantities()
    failures = []
    emb, opt, objective = _training(dname)
    with CallSpy() as eager:
        for b in (b1, b2):
            opt.zero_grad(set_to_none=True)
            objective(b).backward()
            opt.step()
    assert eager.calls == ['mm_so_pdist_loss_subset', 'mm_mat_radam_step'] * 2, eager.calls
    eager_state = _after(emb, opt)
    for name, got in zip(('x', 'exp_avg', 'exp_avg_sq'), eager_state):
        C.check(f'so subset training eager {dname}', f'so_subset_train_{name}', got, q[name], dname, failures)
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
    for name, old, got in zip(('x', 'exp_avg', 'exp_avg_sq'), eager_state, _after(emb, opt)):
        C.check(f'so subset training replayed {dname}', f'so_subset_train_{name}', got, q[name], dname, failures)
        gc.check(f'so subset training replayed {dname}', name, old, got, q[name].want, sc.DT[dname], failures)
    assert not failures, '\n'.join(failures)


def test_print_worst_ratios():
    """(last in the file) the worst err / bound per quantity and dtype seen by the tests above: the table of profiles/so_minibatch.md"""
    for (what, dname), (ratio, tag) in sorted(C.sc.RATIOS.items()):
        if what.startswith('so_subset'):
            print(f'{what:32s} {dname}: {ratio:.3f}  ({tag})')
            assert ratio <= 1.0, (what, dname, tag)
