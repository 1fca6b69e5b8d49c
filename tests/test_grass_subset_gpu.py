"""The Grassmann node-minibatch objective (mm_grass_pdist_loss_subset, csrc/grass_loss_subset.hip; Grassmann.pdist_loss_subset
and the route through ManifoldEmbedding.fused_objective / BatchedObjective) against oracle/ref_port.py in fp64 under the absolute
rule of tests/mat_cases.py, on the cases of tests/grass_subset_cases.py (which tests/test_grass_subset_host.py holds to
bound_f32 <= 1e-3 S on the CPU).  Every comparison prints err / bound (-rA); the worst ratios are in profiles/grass_minibatch.md."""
import pytest
import torch

import grass_subset_cases as C
from grass_cases import CallSpy
from graphembed import _backend as B

pytestmark = pytest.mark.gpu
mc, gc = C.mc, C.gc

_WS = {}


def _ws(dt, n_total, N, p):
    """ONE workspace per table shape for the whole session, first filled with ones: the call clears it itself"""
    key = (dt, n_total, N, p)
    if key not in _WS:
        nbytes = B.lib().raw('mm_grass_pdist_loss_ws_bytes')(B.MM_F64 if dt == torch.float64 else B.MM_F32, n_total, N, p)
        _WS[key] = torch.full((nbytes, ), 0x3f, dtype=torch.uint8, device='cuda')
    return _WS[key]


def abi_subset(x, dense, idx, N, p, loss_name, rows=None, bs=None):
    """(loss, grad_x, grad_scale) of one mm_grass_pdist_loss_subset call; the outputs are pre-filled with NaN"""
    n_total = x.shape[0]
    bs = idx.numel() if bs is None else bs
    rb, re = (0, bs) if rows is None else rows
    kind, alpha, eps, terms = C.loss_spec(loss_name)
    sr = torch.tensor([gc.SCALE_RAW], dtype=x.dtype, device=x.device)
    out, grad = torch.full((2, ), float('nan'), dtype=x.dtype, device=x.device), torch.full_like(x, float('nan'))
    B.lib().call('mm_grass_pdist_loss_subset', B.dtype_code(x), kind, B.ptr(x), B.ptr(dense), B.ptr(sr), n_total, N, p, B.ptr(idx), bs,
                 rb, re, alpha, eps, terms, None, B.ptr(out), B.ptr(grad), B.ptr(_ws(x.dtype, n_total, N, p)), B.stream_of(x))
    return out[:1], grad, out[1:]


def inputs(regime, N, p, bs, dname, n_total=C.N_TOTAL, perm=False):
    dt = gc.DT[dname]
    return (C.points(regime, n_total, N, p).to(dt).cuda(), C.dense(regime, N, p, bs, n_total, perm).to(dt).cuda(),
            C.batch_idx(n_total, bs, perm).cuda())


def hold(tag, got, q, rows, regime, N, p, dname, failures):
    """the compared quantities under the rule, the others finite"""
    for name, g in zip(('loss', 'grad_x', 'grad_scale'), got):
        if name in C.subset_compared(regime, N, p):
            C.check(tag, f'subset_{name}', g, q[(rows, name)], dname, failures)
        else:
            assert bool(torch.isfinite(g).all()), (tag, name)


def outside_is_zero(grad, idx):
    mask = torch.ones(grad.shape[0], dtype=torch.bool, device=grad.device)
    mask[idx] = False
    return torch.equal(grad[mask], torch.zeros_like(grad[mask]))


SHAPE_IDS = [f'{N}x{p}' for N, p in C.SHAPES]


@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', C.SHAPES, ids=SHAPE_IDS)
def test_cases_against_the_oracle(N, p, dname, loss_name):
    failures = []
    for regime in mc.regimes(N, p):
        for bs in C.BATCHES:
            x, dense, idx = inputs(regime, N, p, bs, dname)
            got = abi_subset(x, dense, idx, N, p, loss_name)
            tag = f'subset {N}x{p} {regime} bs={bs} {loss_name}'
            hold(tag, got, C.subset_quantities(regime, N, p, bs, loss_name, C.ranges_of(bs)), None, regime, N, p, dname, failures)
            assert outside_is_zero(got[1], idx), tag
    # the whole table in a permuted order
    regime = 'spread'
    x, dense, idx = inputs(regime, N, p, 65, dname, 65, True)
    got = abi_subset(x, dense, idx, N, p, loss_name)
    hold(f'subset {N}x{p} {regime} n_total=bs=65 {loss_name}', got, C.subset_quantities(regime, N, p, 65, loss_name, (None, ), 65, True),
         None, regime, N, p, dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', C.SHAPES, ids=SHAPE_IDS)
def test_row_shards(N, p, dname, loss_name):
    """every range of SHARDS against the oracle of its pairs; the parts of COVER sum to the whole within the summed bounds"""
    bs, failures = 130, []
    for regime in mc.regimes(N, p):
        x, dense, idx = inputs(regime, N, p, bs, dname)
        q = C.subset_quantities(regime, N, p, bs, loss_name, C.SHARDS)
        parts = {}
        for rows in C.SHARDS:
            got = abi_subset(x, dense, idx, N, p, loss_name, rows)
            tag = f'shard {N}x{p} {regime} rows={rows} {loss_name}'
            assert outside_is_zero(got[1], idx), tag
            if (rows, 'loss') in q:
                hold(tag, got, q, rows, regime, N, p, dname, failures)
            else:   # no pair in the range: a zero gradient and {0, 0}
                assert all(torch.equal(g, torch.zeros_like(g)) for g in got), tag
            parts[rows] = got
        for k, name in enumerate(('loss', 'grad_x', 'grad_scale')):
            if name not in C.subset_compared(regime, N, p):
                continue
            total = sum(parts[r][k].double().cpu() for r in C.COVER)
            bound = sum(q[(r, name)].bound(dname) for r in C.COVER if (r, name) in q)
            err = float((total - q[(None, name)].want).abs().max())
            print(f'cover {N}x{p} {regime} {loss_name} {name} {dname}: err {err:.3e} / summed bounds {bound:.3e}')
            if not err <= bound:
                failures.append(f'cover {N}x{p} {regime} {loss_name} {name}: {err:.3e} > {bound:.3e}')
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', C.SHAPES, ids=SHAPE_IDS)
def test_the_full_batch_kernel_on_the_gathered_batch_is_held_to_the_same_quantity(N, p, dname, loss_name):
    """(not bitwise: both kernels sum through float atomics)"""
    failures = []
    kind, alpha, eps, terms = C.loss_spec(loss_name)
    for regime in mc.regimes(N, p):
        for bs in (65, 130):
            x, dense, idx = inputs(regime, N, p, bs, dname)
            i, j = (t.cuda() for t in C.ref.triu_pairs(bs))
            xb, tg = x[idx].contiguous(), dense[idx[i], idx[j]].contiguous()
            sr = torch.tensor([gc.SCALE_RAW], dtype=x.dtype, device='cuda')
            out, grad = torch.full((2, ), float('nan'), dtype=x.dtype, device='cuda'), torch.full_like(xb, float('nan'))
            B.lib().call('mm_grass_pdist_loss', B.dtype_code(x), kind, B.ptr(xb), B.ptr(tg), B.ptr(sr), bs, N, p, 0, bs, alpha, eps, terms,
                         None, B.ptr(out), B.ptr(grad), B.ptr(_ws(x.dtype, bs, N, p)), B.stream_of(x))
            full = torch.zeros_like(x)
            full[idx] = grad
            hold(f'gathered {N}x{p} {regime} bs={bs} {loss_name}', (out[:1], full, out[1:]),
                 C.subset_quantities(regime, N, p, bs, loss_name, C.ranges_of(bs)), None, regime, N, p, dname, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('N,p', C.SHAPES, ids=SHAPE_IDS)
def test_index_hygiene(N, p, dname):
    """the kernel reads the low 32-bit word of an index and clamps the node id into the table"""
    regime, bs, loss_name, failures = 'spread', 65, 'stress', []
    x, dense, idx = inputs(regime, N, p, bs, dname)
    q = C.subset_quantities(regime, N, p, bs, loss_name, C.ranges_of(bs))
    high = torch.arange(bs, dtype=torch.int64, device='cuda') % 5 - 2     # -2 .. 2: negative and positive high words
    poisoned = (idx + (high << 32)).contiguous()
    assert torch.equal(poisoned & 0xffffffff, idx) and not torch.equal(poisoned, idx)
    hold(f'poisoned high words {N}x{p}', abi_subset(x, dense, poisoned, N, p, loss_name), q, None, regime, N, p, dname, failures)
    # low words outside the table: clamped (wrong numbers for that batch, never an access outside the buffers)
    wild = idx.clone()
    wild[3], wild[4], wild[5] = C.N_TOTAL + 5, -7, 0x7fffffff
    got = abi_subset(x, dense, wild, N, p, loss_name)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert not failures, '\n'.join(failures)


def _dataset(dense):
    """a GraphDataset on the GPU whose dense matrix is the case's (asymmetric) one"""
    from graphembed.data import GraphDataset
    ds = GraphDataset(torch.ones(3, dtype=dense.dtype, device=dense.device))
    ds._dense = dense
    return ds


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_batched_objective_takes_the_in_kernel_route(dname):
    """(fails without mm_grass_pdist_loss_subset: the step then gathers — take_rows, mm_pair_gather, mm_grass_pdist_loss)"""
    from graphembed.modules import BatchedObjective
    N, p, regime, bs, failures = 6, 3, 'spread', 65, []
    dt = gc.DT[dname]
    x, dense, idx = inputs(regime, N, p, bs, dname)
    emb = gc.embedding(C.N_TOTAL, N, p, dt, C.points(regime, C.N_TOTAL, N, p).double())
    fn, kw = gc.objective('quotient')
    objective = BatchedObjective(fn, _dataset(dense), emb)
    q = C.subset_quantities(regime, N, p, bs, 'quotient', C.ranges_of(bs))
    for where, indices in (('host', idx.cpu()), ('device', idx)):
        emb.zero_grad(set_to_none=True)
        with CallSpy() as spy:
            loss = objective(indices, **kw)
        assert spy.calls == ['mm_grass_pdist_loss_subset'], spy.calls
        loss.backward()
        hold(f'routed ({where} indices) {N}x{p} {regime} bs={bs}', (loss.reshape(1), emb.xs[0].grad, emb.scales[0].grad.reshape(1)), q, None,
             regime, N, p, dname, failures)
        assert outside_is_zero(emb.xs[0].grad, idx)
    assert ('grass', dt, emb.xs[0].device, C.N_TOTAL, N, p) in emb._pair_ws   # kept for the embedding's lifetime
    # repeated host-side indices: the gather route, as before
    rep = idx.cpu().clone()
    rep[1] = rep[0]
    with CallSpy() as spy:
        loss = objective(rep, **kw)
    assert 'mm_grass_pdist_loss_subset' not in spy.calls and 'mm_grass_pdist_loss' in spy.calls, spy.calls
    assert bool(torch.isfinite(loss))
    assert not failures, '\n'.join(failures)
