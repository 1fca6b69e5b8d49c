"""The node-minibatch form of the affine-invariant SPD pair kernel on the GPU (csrc/spd_pair.hpp: spd_pdist_bwd_kernel<..., SUB =
true>; mm_spd_pdist_loss_subset through graphembed.modules._SingleSubsetLoss and through the C ABI) against the fp64 oracle of
tests/spd_subset_cases.py, whose docstring states the cases, the rule (e_sub <= 2 e_full + 64 eps S, e_full the deviation from
the same oracle of the gathered full-batch route on the same GPU in the same test) and the teeth: per case the allowance granted
to grad_x must stay below half of what ONE transposed target moves it by, so a pass cannot contain a wrong pair.  Every figure
is printed before it is judged (-rA); the last test prints the worst per quantity, dtype and sweep: profiles/spd_subset.md."""
import pytest
import torch

import grass_cases as gc
import spd_subset_cases as C

pytestmark = pytest.mark.gpu
ENTRY = 'mm_spd_pdist_loss_subset'


def _B():
    from graphembed import _backend as B
    return B


def _spd(D):
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    man = SPD(D)
    assert (man.wmin, man.wmax) == (C.WMIN, C.WMAX)
    return man


def dev(t, dname):
    return t.to(C.DT[dname]).cuda().contiguous()


def _spec(loss_name):
    fn, kw = gc.objective(loss_name)
    return fn.fused_spec(**kw)


def _leaves(x, dname):
    return x.detach().clone().requires_grad_(), torch.tensor(C.SCALE_RAW, dtype=C.DT[dname], device='cuda', requires_grad=True)


def in_kernel(dname, D, x, dm, idx, loss_name, rows=None):
    """(loss [1], grad_x [N_TOTAL, D, D], grad_scale [1]) of _SingleSubsetLoss: exactly one library call, the SUB kernel's entry"""
    from graphembed.modules import _SingleSubsetLoss
    xl, s = _leaves(x, dname)
    with gc.CallSpy() as spy:
        loss = _SingleSubsetLoss.apply(_spec(loss_name), rows, _spd(D), (_B().FACTOR_SPD, D), None, idx, dm, xl, s)
        gx, gs = torch.autograd.grad(loss, [xl, s])
    assert spy.calls == [ENTRY] and not any('gather' in name for name in spy.calls), spy.calls
    return loss.detach().reshape(1), gx, gs.reshape(1)


def established(dname, D, x, dm, idx, loss_name, rows=None):
    """the same objective on the route the full-batch tests hold: gather x[idx], the pair-vector targets dm[idx[a], idx[b]], the
    full-batch fused kernel over `rows`, the gradient rows scattered into zeros (autograd's index backward)"""
    bs = idx.numel()
    xl, s = _leaves(x, dname)
    a, b = torch.triu_indices(bs, bs, 1, device=idx.device)
    lo, hi = C.pair_slice(bs, rows)
    tg = dm[idx[a[lo:hi]], idx[b[lo:hi]]].contiguous()
    with gc.CallSpy() as spy:
        loss = _spd(D).pdist_loss(xl[idx], s, tg, _spec(loss_name), rows=rows)
        gx, gs = torch.autograd.grad(loss, [xl, s])
    assert spy.calls == ['mm_spd_pdist_loss'], spy.calls
    return loss.detach().reshape(1), gx, gs.reshape(1)


def outside_is_zero(grad, idx):
    outside = torch.ones(grad.shape[0], dtype=torch.bool, device=grad.device)
    outside[idx] = False
    return bool((grad[outside] == 0).all())


def finite(res):
    return all(bool(torch.isfinite(t).all()) for t in res)


def all_zero(res):
    return all(float(t.abs().max()) == 0.0 for t in res)


def judge(sweep, tag, dname, c, full, sub, idx, failures, want=None, effect=None):
    """everything a result of the SUB kernel is held to; returns the allowances the rule granted"""
    want = C.oracle(c) if want is None else want
    assert finite(sub) and outside_is_zero(sub[1], idx), tag
    granted = C.hold(sweep, tag, dname, full, sub, want, failures)
    effect = C.one_pair_effect(c) if effect is None else effect
    line = f'{tag} {dname}: allowance of grad_x {granted["grad_x"]:.3e}, one transposed target moves it by {effect:.3e}'
    print(line)
    if not granted['grad_x'] < 0.5 * effect:
        failures.append(line + ': the rule could hide a wrong pair')
    return granted


def run_case(sweep, c, dname, failures):
    x, dm, idx = dev(C.points(c.regime, c.D), dname), dev(C.dense(c.regime, c.D, c.bs), dname), C.batch_idx(c.bs).cuda()
    sub = in_kernel(dname, c.D, x, dm, idx, c.loss, c.rows)
    if not C.n_pairs(c):     # a range without a pair: a zero loss record and an all-zero gradient
        assert all_zero(sub) and all_zero(C.oracle(c)[:3]), C.case_id(c)
        return sub, None
    full = established(dname, c.D, x, dm, idx, c.loss, c.rows)
    return sub, judge(sweep, C.case_id(c), dname, c, full, sub, idx, failures)


# ---- 1. every instantiation, in every regime ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', C.DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_every_instantiation(dname, D):
    """stress and quotient kernel of this (dtype, D) in `init` (close pairs), `mid` and `wide` (the far-pair paths), bs = 130"""
    failures = []
    cases = [c for c in C.instantiation_cases() if c.D == D]
    assert len(cases) == 6
    for c in cases:
        run_case('instantiations', c, dname, failures)
    assert not failures, '\n'.join(failures)


# ---- 2. batch sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', C.BATCH_DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_batch_sizes(dname, D):
    """one pair, three pairs, one column past a 64- and past a 128-column block, the whole table as a permutation"""
    failures = []
    cases = [c for c in C.batch_size_cases() if c.D == D]
    assert len(cases) == 10
    for c in cases:
        run_case('batch sizes', c, dname, failures)
    assert not failures, '\n'.join(failures)


# ---- 3. row shards of a batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss_name', C.LOSSES)
@pytest.mark.parametrize('D', C.SHARD_DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_row_shards(dname, D, loss_name):
    """every range of SHARDS against its own oracle; the ranges of COVER add up to the full range within the full range's allowance"""
    failures, results = [], {}
    for rows in C.SHARDS:
        results[rows] = run_case('row shards', C.Case('mid', D, C.BS, loss_name, rows), dname, failures)
    whole, granted = results[None]
    for k, name in enumerate(C.NAMES):
        total = sum(results[rows][0][k].double() for rows in C.COVER)
        err = float((total - whole[k].double()).abs().max())
        print(f'spd({D}) {loss_name} {dname} {name}: sum over COVER differs from the full range by {err:.3e}, allowance {granted[name]:.3e}')
        if not err <= granted[name]:
            failures.append(f'sum over COVER, {name}: {err:.3e} > {granted[name]:.3e}')
    assert not failures, '\n'.join(failures)


# ---- 4. what the masked lanes read ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', C.MASKED_DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_masked_lanes_read_nothing_that_counts(dname, D):
    """NaN in every entry of `dense` whose row or column node is outside the batch; then also on the diagonal and on the transposed
    side dense[idx[b]][idx[a]], a < b — what lanes at or below the diagonal and beyond the batch load and must mask"""
    failures = []
    x = dev(C.points('mid', D), dname)
    for bs in C.MASKED_SIZES:
        idx = C.batch_idx(bs)
        inb = torch.zeros(C.N_TOTAL, dtype=torch.bool)
        inb[idx] = True
        a, b = torch.triu_indices(bs, bs, 1)
        clean = C.dense('mid', D, bs)
        outside = clean.clone()
        outside[~inb, :] = float('nan')
        outside[:, ~inb] = float('nan')
        lower = outside.clone()
        lower.fill_diagonal_(float('nan'))
        lower[idx[b], idx[a]] = float('nan')
        assert torch.equal(lower[idx[a], idx[b]], clean[idx[a], idx[b]]) and int(torch.isnan(lower).sum()) == C.N_TOTAL**2 - a.numel()
        for loss_name in C.LOSSES:
            c = C.Case('mid', D, bs, loss_name, None)
            full = established(dname, D, x, dev(clean, dname), idx.cuda(), loss_name)
            for what, dm in (('NaN outside the batch', outside), ('NaN everywhere but the targets', lower)):
                sub = in_kernel(dname, D, x, dev(dm, dname), idx.cuda(), loss_name)
                judge('masked lanes', f'{C.case_id(c)} ({what})', dname, c, full, sub, idx.cuda(), failures)
    assert not failures, '\n'.join(failures)


# ---- 5. the C ABI: workspaces ------------------------------------------------------------------------------------------------------------
def workspace(dname, D, fill):
    B = _B()
    nbytes = B.lib().raw('mm_spd_pdist_ws_bytes')(B.MM_F32 if dname == 'f32' else B.MM_F64, C.N_TOTAL, D)
    return torch.full((nbytes, ), fill, dtype=torch.uint8, device='cuda')


def raw_call(x, dm, idx, loss_name, ws, flags=0, prepare=False):
    """mm_spd_pdist_loss_subset itself (outputs pre-filled with NaN), optionally behind mm_spd_prepare"""
    B = _B()
    D = x.shape[-1]
    kind, alpha, eps, terms = C.loss_spec(loss_name)
    out = torch.full((2, ), float('nan'), dtype=x.dtype, device='cuda')
    grad = torch.full_like(x, float('nan'))
    sc = torch.tensor([C.SCALE_RAW], dtype=x.dtype, device='cuda')
    with B.on_device(x.device):
        if prepare:
            B.lib().call('mm_spd_prepare', B.dtype_code(x), B.ptr(x), C.N_TOTAL, D, B.ptr(ws), B.stream_of(x))
        B.lib().call(ENTRY, B.dtype_code(x), kind, B.ptr(x), B.ptr(dm), B.ptr(sc), C.N_TOTAL, D, B.ptr(idx), idx.numel(), 0, idx.numel(),
                     alpha, eps, terms, None, C.WMIN, C.WMAX, B.ptr(out), B.ptr(grad), B.ptr(ws), flags, B.stream_of(x))
    torch.cuda.synchronize()
    return out[0:1].clone(), grad, out[1:2].clone()


@pytest.mark.parametrize('D', C.ABI_DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_workspaces_through_the_c_abi(dname, D):
    """a workspace of 0xFF bytes against a zeroed one; mm_spd_prepare + MM_WS_PREPARED against flags = 0; ONE workspace serving
    batch A, a disjoint batch B of the same size (the same walk: the share table's entry hits) and A again"""
    B = _B()
    failures = []
    x = dev(C.points('mid', D), dname)
    dm = dev(C.dense('mid', D, C.ABI_BS, with_second=True), dname)
    batches = {'A': C.batch_idx(C.ABI_BS), 'B': C.second_batch()}
    for loss_name in C.LOSSES:
        c = C.Case('mid', D, C.ABI_BS, loss_name, None)
        both = C.dense('mid', D, C.ABI_BS, True)
        want = {'A': C.oracle(c), 'B': C.objective_of('mid', D, both, batches['B'], loss_name)}
        effect = {k: C.pair_effect_of('mid', D, both, batches[k], loss_name) for k in batches}
        idx = {k: v.cuda() for k, v in batches.items()}
        full = {k: established(dname, D, x, dm, idx[k], loss_name) for k in batches}

        def held(what, k, sub):
            judge('workspaces', f'{C.case_id(c)} ({what})', dname, c, full[k], sub, idx[k], failures, want[k], effect[k])
        held('zeroed workspace', 'A', raw_call(x, dm, idx['A'], loss_name, workspace(dname, D, 0)))
        held('0xFF workspace', 'A', raw_call(x, dm, idx['A'], loss_name, workspace(dname, D, 0xFF)))
        held('mm_spd_prepare, MM_WS_PREPARED', 'A',
             raw_call(x, dm, idx['A'], loss_name, workspace(dname, D, 0xFF), flags=B.MM_WS_PREPARED, prepare=True))
        ws = workspace(dname, D, 0)
        for step, k in enumerate('ABA'):
            sub = raw_call(x, dm, idx[k], loss_name, ws)
            held(f'one workspace, call {step + 1}: batch {k}', k, sub)
            other = idx['B' if k == 'A' else 'A']
            assert bool((sub[1][other] == 0).all()), (loss_name, step, k)
    assert not failures, '\n'.join(failures)


# ---- last: the figures -------------------------------------------------------------------------------------------------------------------
def test_print_worst_ratios():
    """(last in the file) per sweep, dtype and quantity the worst e_sub / allowance, e_sub / S and e_full / S of this session"""
    worst = {}
    for sweep, dname, name, r_allow, r_sub, r_full, tag in C.RECORDS:
        w = worst.setdefault((sweep, dname, name), [0.0, 0.0, 0.0, 0])
        w[0], w[1], w[2], w[3] = max(w[0], r_allow), max(w[1], r_sub), max(w[2], r_full), w[3] + 1
    print('sweep | dtype | quantity | calls | e_sub / allowance | e_sub / S | e_full / S')
    for (sweep, dname, name), (r_allow, r_sub, r_full, count) in sorted(worst.items()):
        print(f'{sweep} | {dname} | {name} | {count} | {r_allow:.3f} | {r_sub:.2e} | {r_full:.2e}')
