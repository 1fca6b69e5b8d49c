"""The fused objective of a product of constant-curvature factors (mm_stereo_product_*, csrc/stereo.hip) against the long-double
oracle of tests/stereo_product_cases.py: every case x objective setting x {f64, f32} through the C ABI, the Python classes
(which must agree bitwise), shards, degenerate sizes, the route BatchedObjective takes, training and graph capture.

Tolerance rule (stereo_cases.bound): fp64 <= 1e-11 of the scale; fp32 <= twice the recorded reference-fp32's own deviation from
the same oracle on the same case, setting and quantity, never asked below 16 * 2^-24 of the scale.  Scales: sum |loss terms|,
max |grad_x_k|, sum |g dF/dc_raw| of the factor, max m."""
import functools

import numpy as np
import pytest
import torch

import stereo_cases as S
import stereo_product_cases as P
from grass_cases import CallSpy
from graphembed import _backend as B
from test_stereo_gpu import DT, NP, check, cuda, dev, train_setup

pytestmark = pytest.mark.gpu

PER_FACTOR = ('mm_stereo_pdist_fwd', 'mm_stereo_pdist_bwd')


def abi_fwd(xs, cs, modes, rows):
    n = xs[0].shape[0]
    lo, hi = S.pair_slice(n, rows)
    out = torch.full((hi - lo, ), float('nan'), dtype=xs[0].dtype, device=xs[0].device)
    fs = B.stereo_factors([(x, c, None, None, S.C_MIN, x.shape[1], md) for x, c, md in zip(xs, cs, modes)])
    B.lib().call('mm_stereo_product_pdist_fwd', B.dtype_code(xs[0]), fs, len(xs), n, rows[0], rows[1], B.ptr(out), B.stream_of(xs[0]))
    return out


def abi_loss(xs, cs, modes, setting, target, rows):
    """(loss [1], [grad_x_k], [grad_c_k]); the workspace goes in dirty (0xFF), the outputs NaN-filled"""
    n = xs[0].shape[0]
    dt = B.dtype_code(xs[0])
    kind, alpha, eps, terms = P.spec_of(setting)
    gxs = [torch.full_like(x, float('nan')) for x in xs]
    gcs = [torch.full((1, ), float('nan'), dtype=x.dtype, device=x.device) for x in xs]
    loss = torch.full((1, ), float('nan'), dtype=xs[0].dtype, device=xs[0].device)
    ms = (B._c.c_int32 * len(xs))(*[x.shape[1] for x in xs])
    ws = torch.empty(B.lib().raw('mm_stereo_product_ws_bytes')(dt, n, len(xs), ms), dtype=torch.uint8, device=xs[0].device)
    ws.fill_(0xFF)
    fs = B.stereo_factors([(x, c, gx, gc, S.C_MIN, x.shape[1], md) for x, c, gx, gc, md in zip(xs, cs, gxs, gcs, modes)])
    B.lib().call('mm_stereo_product_loss', dt, kind, fs, len(xs), B.ptr(target), n, rows[0], rows[1], alpha, eps, terms, None,
                 B.ptr(loss), B.ptr(ws), B.stream_of(xs[0]))
    return loss, gxs, gcs


def device_inputs(case, dname):
    xs, craws = P.make_inputs(case)
    return [cuda(x, dname) for x in xs], [cuda(np.array([c]), dname) for c in craws]


def manifolds(case, dname):
    from graphembed.manifolds import Stereographic
    return [Stereographic(d, c_init=c, c_min=S.C_MIN, keep_sign_fixed=f).to(device=dev(), dtype=DT[dname])
            for d, c, f in zip(case[1], case[2], case[3])]


def compare(failures, tag, dname, o, R, case, name, loss, gxs, gcs):
    """loss, grad_x and grad_c of every factor against the oracle record `o` under the tolerance rule"""
    ref = (lambda what: R[P.key(case, name, what, 'f32')]) if dname == 'f32' and case is not None else (lambda what: None)
    if loss is not None:
        check(failures, f'{tag} loss', dname, float(loss), o['loss'], o['loss_scale'], ref('loss'))
    for k, (gx, gc) in enumerate(zip(gxs, gcs)):
        check(failures, f'{tag} grad_x[{k}]', dname, gx.cpu().numpy(), o['gx'][k], np.abs(o['gx'][k]).max(), ref(f'gx{k}'))
        r = ref(f'gc{k}')
        check(failures, f'{tag} grad_c[{k}]', dname, float(gc), o['gc'][k], o['gcs'][k], None if r is None else r[0])


@pytest.mark.parametrize('name', P.SETTING_IDS)
@pytest.mark.parametrize('case', P.CASES, ids=P.CASE_IDS)
def test_case_against_the_oracle(case, name):
    setting = P.SETTINGS[P.SETTING_IDS.index(name)]
    R = S.recorded()
    n = case[0]
    rows = P.rows_of(case)
    lo, hi = S.pair_slice(n, rows)
    o = P.oracle(case, name)
    tag = f'{P.case_id(case)} {name}'
    failures = []
    for dname in ('f64', 'f32'):
        xs, cs = device_inputs(case, dname)
        modes = P.modes_of(case)
        got = abi_fwd(xs, cs, modes, rows)
        target = cuda(o['target'], dname)
        loss, gxs, gcs = abi_loss(xs, cs, modes, setting, target, rows)
        if setting[1] == 0:
            assert bool(torch.isnan(loss).all()), 'MM_LOSS_NONE writes no loss'
            loss = None
        if hi == lo:   # the last row or an empty range: no pair
            assert got.shape == (0, ) and all(not g.any() for g in gxs) and all(not g.any() for g in gcs), 'a range without pairs leaves zeros'
            assert loss is None or float(loss) == 0.0
            continue
        ref32 = R[f'prod/{P.case_id(P.base_of(case))}/dists_f32'][lo:hi] if dname == 'f32' else None
        check(failures, f'{tag} pair vector', dname, got.cpu().numpy(), o['m'], o['m_max'], ref32)
        compare(failures, tag, dname, o, R, case, name, loss, gxs, gcs)
    assert not failures, '\n'.join(failures)


REPRO = [P.CASES[3], P.CASES[8], P.CASES[9], P.CASES[10], P.CASES[13], P.CASES[16]]


@pytest.mark.parametrize('case', REPRO, ids=P.case_id)
def test_calls_are_reproducible_and_the_classes_agree_bitwise(case):
    from graphembed.manifolds.stereographic import product_loss, product_pdist
    n = case[0]
    rows = P.rows_of(case)
    for dname in ('f32', 'f64'):
        xs, cs = device_inputs(case, dname)
        modes = P.modes_of(case)
        mans = manifolds(case, dname)
        fwd = abi_fwd(xs, cs, modes, rows)
        assert torch.equal(fwd, abi_fwd(xs, cs, modes, rows))
        for name in ('up', 'stress', 'q3b'):
            setting = P.SETTINGS[P.SETTING_IDS.index(name)]
            target = cuda(P.oracle(case, name)['target'], dname)
            a, b = abi_loss(xs, cs, modes, setting, target, rows), abi_loss(xs, cs, modes, setting, target, rows)
            assert all(torch.equal(u, v) for u, v in zip(a[1] + a[2], b[1] + b[2])), 'two calls differ'
            assert name == 'up' or torch.equal(a[0], b[0])
            leaves = [x.clone().requires_grad_() for x in xs]
            for man in mans:
                man.c.grad = None
            r = None if case[5] is None else rows
            if name == 'up':
                d = product_pdist(mans, leaves, rows=r)
                assert torch.equal(d.detach(), fwd), 'the class and the C ABI disagree (forward)'
                (d * target).sum().backward()
            else:
                kind, alpha, eps, terms = P.spec_of(setting)
                loss = product_loss(mans, leaves, target, ('stress' if kind == 1 else 'quotient', alpha, eps, terms), rows=r)
                assert torch.equal(loss.detach().reshape(1), a[0]), 'the class and the C ABI disagree (loss)'
                loss.backward()
            for x, man, gx, gc in zip(leaves, mans, a[1], a[2]):
                assert torch.equal(x.grad, gx) and torch.equal(man.c.grad.to(gc.dtype), gc), 'the class and the C ABI disagree (backward)'


@pytest.mark.parametrize('name', ['up', 'stress', 'q3', 'q3b'])
def test_shards_sum_to_the_full_launch(name):
    """n = 129, ds = [5, 8]: the row ranges of the case list, completed to a partition of the rows, sum to the full launch; the
    ranges without a pair ([128, 129) and an empty one) leave exact zeros."""
    case = P.CASES[14]
    assert case[0] == 129 and case[5] is None
    setting = P.SETTINGS[P.SETTING_IDS.index(name)]
    R = S.recorded()
    o = P.oracle(case, name)
    cuts = [0, 1, 43, 86, 127, 128, 129]
    assert all(r in list(zip(cuts[:-1], cuts[1:])) for r in S._rows(129)[1:5])
    failures = []
    for dname in ('f64', 'f32'):
        xs, cs = device_inputs(case, dname)
        modes = P.modes_of(case)
        target = cuda(o['target'], dname)
        full = abi_loss(xs, cs, modes, setting, target, (0, 129))
        sums = [torch.zeros_like(t) for t in [full[0]] + full[1] + full[2]]
        fw = []
        for rb, re in list(zip(cuts[:-1], cuts[1:])) + [(5, 5)]:
            lo, hi = S.pair_slice(129, (rb, re))
            part = abi_loss(xs, cs, modes, setting, target[lo:hi].contiguous(), (rb, re))
            if hi == lo:
                assert all(not t.any() for t in part[1] + part[2]) and (name == 'up' or float(part[0]) == 0.0)
            for s, t in zip(sums, ([part[0]] if name != 'up' else [torch.zeros_like(part[0])]) + part[1] + part[2]):
                s += t
            fw.append(abi_fwd(xs, cs, modes, (rb, re)))
        assert torch.equal(torch.cat(fw), abi_fwd(xs, cs, modes, (0, 129)))
        for tag, res in (('shard sum', (sums[0], sums[1:3], sums[3:5])), ('full launch', full)):
            compare(failures, f'{name} {tag}', dname, o, R, case, name, None if name == 'up' else res[0], res[1], res[2])
    assert not failures, '\n'.join(failures)


def test_degenerate_node_counts():
    from graphembed.modules import StereographicProductEmbedding
    for dname in ('f32', 'f64'):
        for n in (0, 1):
            xs = [torch.zeros(n, 5, dtype=DT[dname], device=dev()), torch.zeros(n, 3, dtype=DT[dname], device=dev())]
            cs = [cuda(np.array([0.01]), dname), cuda(np.array([-0.3]), dname)]
            assert abi_fwd(xs, cs, [0, 0], (0, n)).shape == (0, )
            for name in ('up', 'stress', 'q3'):
                loss, gxs, gcs = abi_loss(xs, cs, [0, 0], P.SETTINGS[P.SETTING_IDS.index(name)], None, (0, n))
                assert all(not g.any() for g in gxs + gcs) and (name == 'up' or float(loss) == 0.0)
        emb = StereographicProductEmbedding(1, [5, 3]).to(device=dev(), dtype=DT[dname])
        d = emb.compute_dists()
        assert d.shape == (0, )
        d.sum().backward()
        assert all(not x.grad.any() for x in emb.xs) and all(float(c.grad) == 0.0 for c in emb.curvature_params)


@functools.lru_cache(maxsize=None)
def single_oracle(case, name):
    x, c_raw = S.make_inputs(case)
    mode = S.mode_of(case[2], case[3])
    m = S.pdist(x, c_raw, mode, True)
    target = (m * np.array(P.F, dtype=S.LD)[np.arange(len(m)) % 4]).astype(np.float32)
    setting = P.SETTINGS[P.SETTING_IDS.index(name)]
    terms, g = P.objective(m, target, setting)
    gx, gc, gcs = S.pdist_grads(x, c_raw, mode, True, g)
    return dict(m=m, target=S.upstream(len(m)) if name == 'up' else target, loss=terms.sum(), loss_scale=np.abs(terms).sum(), gx=[gx], gc=[gc], gcs=[gcs])


@pytest.mark.parametrize('name', ['up', 'stress', 'q3'])
def test_single_factor_against_the_oracle(name):
    """nf = 1 on a case of tests/stereo_cases.py: with an upstream g the recorded single-factor reference gives the fp32 bound; the
    objectives have no recorded fp32 counterpart there and are held to the fp64 rule."""
    case = (65, 8, 1.0, False, 'spread', None)
    x_np, c_raw = S.make_inputs(case)
    R = S.recorded()
    o = single_oracle(case, name)
    failures = []
    for dname in ('f64', 'f32') if name == 'up' else ('f64', ):
        xs, cs = [cuda(x_np, dname)], [cuda(np.array([c_raw]), dname)]
        got = abi_fwd(xs, cs, [0], (0, 65))
        loss, gxs, gcs = abi_loss(xs, cs, [0], P.SETTINGS[P.SETTING_IDS.index(name)], cuda(o['target'], dname), (0, 65))
        tag = S.case_id(case)
        f32 = dname == 'f32'
        check(failures, 'pair vector', dname, got.cpu().numpy(), o['m'], o['m'].max(), R[f'{tag}/pdist_sq_f32'] if f32 else None)
        check(failures, 'grad_x', dname, gxs[0].cpu().numpy(), o['gx'][0], np.abs(o['gx'][0]).max(), R[f'{tag}/gx_sq_f32'] if f32 else None)
        check(failures, 'grad_c', dname, float(gcs[0]), o['gc'][0], o['gcs'][0], R[f'{tag}/gc_sq_f32'][0] if f32 else None)
        if name != 'up':
            check(failures, 'loss', dname, float(loss), o['loss'], o['loss_scale'])
    assert not failures, '\n'.join(failures)


# ---- the route BatchedObjective takes ------------------------------------------------------------------------------------------
ROUTE_CASE = P.CASES[3]   # n = 65, ds = [5, 5], c = (0.01, -0.3)
BATCH = np.random.RandomState(11).permutation(65)[:23]


class Pairs:
    """the dataset protocol of BatchedObjective over the case's float32 targets"""

    def __init__(self, target, n, dname):
        self.n = n
        self.full = torch.from_numpy(target.astype(NP[dname]))
        self.dense = torch.zeros(n, n, dtype=self.full.dtype)
        a, b = torch.triu_indices(n, n, 1)
        self.dense[a, b] = self.full
        self.dense = self.dense + self.dense.T

    def __getitem__(self, i):
        if i is None:
            return self.full
        p, q = torch.triu_indices(len(i), len(i), 1)
        return self.dense[i[p], i[q]]


def route_embedding(dname, case=ROUTE_CASE):
    from graphembed.modules import StereographicProductEmbedding
    emb = StereographicProductEmbedding(case[0], list(case[1])).to(device=dev(), dtype=DT[dname])
    xs, craws = P.make_inputs(case)
    with torch.no_grad():
        for p, man, x, c in zip(emb.xs, emb.manifolds, xs, craws):
            p.copy_(cuda(x, dname))
            man.c.fill_(float(c))
    return emb


@functools.lru_cache(maxsize=None)
def batch_oracle(name):
    """the oracle of the node minibatch BATCH of ROUTE_CASE: its targets are the full case's targets of the same node pairs"""
    xs, craws = P.make_inputs(ROUTE_CASE)
    sub = [x[BATCH] for x in xs]
    m = sum(S.pdist(x, c, 0, True) for x, c in zip(sub, craws))
    target = Pairs(P.pairs_of(ROUTE_CASE)[1], 65, 'f32')[torch.from_numpy(BATCH)].numpy()
    terms, g = P.objective(m, target, P.SETTINGS[P.SETTING_IDS.index(name)])
    grads = [S.pdist_grads(x, c, 0, True, g) for x, c in zip(sub, craws)]
    return dict(loss=terms.sum(), loss_scale=np.abs(terms).sum(), gx=[a for a, _, _ in grads], gc=[b for _, b, _ in grads],
                gcs=[s for _, _, s in grads])


def run_objective(emb, objective, data, indices, **kw):
    from graphembed.modules import BatchedObjective
    emb.zero_grad()
    with CallSpy() as spy:
        loss = BatchedObjective(objective, data, emb)(indices, **kw)
        loss.backward()
    return loss.detach(), [x.grad.clone() for x in emb.xs], [c.grad.clone() for c in emb.curvature_params], spy.calls


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['stress', 'q3'])
def test_batched_objective_takes_the_fused_route(name, dname):
    from graphembed.objectives import QuotientLoss, StressLoss
    objective = StressLoss() if name == 'stress' else QuotientLoss()
    kw = dict(epoch=1, alpha=1.0)
    R = S.recorded()
    emb = route_embedding(dname)
    data = Pairs(P.pairs_of(ROUTE_CASE)[1], 65, dname)
    assert emb.pair_kernel is True
    assert emb.fused_objective(objective, data[None].to(dev()), None, **kw) is not None, 'no fused objective for the product'
    failures = []
    idx = torch.from_numpy(BATCH)
    for indices in (None, idx):
        loss, gxs, gcs, calls = run_objective(emb, objective, data, indices, **kw)
        assert calls.count('mm_stereo_product_loss') == 1 and not any(c.startswith('mm_stereo_pdist_') for c in calls), calls
        assert 'mm_stereo_product_pdist_fwd' not in calls
        emb.pair_kernel = False
        try:
            assert emb.fused_objective(objective, data[None].to(dev()), None, **kw) is None
            loss0, gxs0, gcs0, calls0 = run_objective(emb, objective, data, indices, **kw)
        finally:
            del emb.pair_kernel
        assert calls0.count('mm_stereo_pdist_fwd') == 2 and calls0.count('mm_stereo_pdist_bwd') == 2, calls0
        assert not any(c.startswith('mm_stereo_product_') for c in calls0), calls0
        if indices is None:
            o = P.oracle(ROUTE_CASE, name)
            compare(failures, f'{name} fused', dname, o, R, ROUTE_CASE, name, loss, gxs, gcs)
            # each route is within its bound of the oracle: the two differ by at most the sum of the two bounds
            for k in range(2):
                r = R[P.key(ROUTE_CASE, name, f'gx{k}', 'f32')] if dname == 'f32' else None
                b = S.bound(dname, 0.0 if r is None else S.deviation(r, o['gx'][k]), float(np.abs(o['gx'][k]).max()))
                assert float((gxs[k] - gxs0[k]).abs().max()) <= 2 * b, (k, float((gxs[k] - gxs0[k]).abs().max()), b)
                r = R[P.key(ROUTE_CASE, name, f'gc{k}', 'f32')] if dname == 'f32' else None
                b = S.bound(dname, 0.0 if r is None else S.deviation(r[0], o['gc'][k]), float(o['gcs'][k]))
                assert abs(float(gcs[k]) - float(gcs0[k])) <= 2 * b, (k, float(gcs[k]), float(gcs0[k]), b)
        else:
            rest = torch.ones(65, dtype=torch.bool)
            rest[idx] = False
            for gx in gxs + gxs0:
                assert not gx[rest.to(dev())].any(), 'gradients outside the minibatch are exactly zero'
                assert bool(gx[idx.to(dev())].any())
            if dname == 'f64':   # (no reference-fp32 record of the subset: the fp64 rule only)
                o = batch_oracle(name)
                compare(failures, f'{name} minibatch', dname, o, R, None, name, loss, [g[idx.to(dev())] for g in gxs], gcs)
                compare(failures, f'{name} minibatch per factor', dname, o, R, None, name, loss0, [g[idx.to(dev())] for g in gxs0], gcs0)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_sne_takes_one_product_forward_and_one_backward(dname):
    from graphembed.objectives import StochasticNeighborLoss
    emb = route_embedding(dname)
    data = Pairs(P.pairs_of(ROUTE_CASE)[1], 65, dname)
    assert emb.fused_objective(StochasticNeighborLoss(), data[None].to(dev()), None, epoch=1, alpha=1.0) is None
    for indices in (None, torch.from_numpy(BATCH)):
        loss, gxs, gcs, calls = run_objective(emb, StochasticNeighborLoss(), data, indices, epoch=1, alpha=1.0)
        assert calls.count('mm_stereo_product_pdist_fwd') == 1 and calls.count('mm_stereo_product_loss') == 1, calls
        assert not any(c.startswith('mm_stereo_pdist_') for c in calls), calls
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in gxs + gcs)
        emb.pair_kernel = False
        try:
            loss0, gxs0, gcs0, calls0 = run_objective(emb, StochasticNeighborLoss(), data, indices, epoch=1, alpha=1.0)
        finally:
            del emb.pair_kernel
        assert calls0.count('mm_stereo_pdist_fwd') == 2 and not any(c.startswith('mm_stereo_product_') for c in calls0), calls0
        for g, g0 in zip(gxs + gcs, gxs0 + gcs0):
            assert torch.allclose(g, g0, rtol=1e-3 if dname == 'f32' else 1e-9, atol=float(g0.abs().max()) * (1e-4 if dname == 'f32' else 1e-10))


# ---- training and capture ------------------------------------------------------------------------------------------------------
class Full:
    def __init__(self, target):
        self.target = target

    def __getitem__(self, i):
        assert i is None
        return self.target


def fused_step(emb, opt, objective, **kw):
    opt.zero_grad(set_to_none=True)
    loss = objective(None, **kw)
    loss.backward()
    opt.step()
    emb.stabilize()
    return loss.detach()


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_training_through_the_fused_route_follows_the_oracle_trace(dname):
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    R = S.recorded()
    emb, opt, target = train_setup(dname)
    objective = BatchedObjective(StressLoss(), Full(target), emb)
    want, _ = S.train_trace([R['train40/x0'], R['train40/x1']], [np.float32(0.01)] * 2, [0, 0], R['train40/target'], dname, 5)
    with CallSpy() as spy:
        trace = [float(fused_step(emb, opt, objective)) for _ in range(5)]
    assert spy.calls.count('mm_stereo_product_loss') == 5 and not any(c.startswith('mm_stereo_pdist_') for c in spy.calls)
    failures = []
    for e in range(5):
        check(failures, f'epoch {e} loss', dname, trace[e], want[e], want[e], R[f'train40/loss_{dname}'][e])
    assert not failures, '\n'.join(failures)
    assert all(b < a for a, b in zip(trace, trace[1:])), trace
    for man in emb.manifolds:
        assert float(man.c.detach()) != float(np.float32(0.01)), 'the curvature did not move'
    assert all(bool(torch.isfinite(x).all()) for x in emb.xs)


def captured_against_eager(make_objective, schedule):
    """One step captured once on a single stream and replayed three times against three eager steps; `schedule(objective, k)`
    gives the step's keyword arguments and, for the replay, is what runs between replays."""
    from graphembed.modules import BatchedObjective
    dname = 'f32'
    emb0, opt0, target0 = train_setup(dname)
    ob0 = make_objective()
    eager = BatchedObjective(ob0, Full(target0), emb0)
    for k in range(3):
        fused_step(emb0, opt0, eager, **schedule(ob0, k))
    emb, opt, target = train_setup(dname)
    ob = make_objective()
    objective = BatchedObjective(ob, Full(target), emb)
    params = list(emb.xs) + list(emb.curvature_params)
    start = [p.detach().clone() for p in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: allocator pools, lazy initialisation
        fused_step(emb, opt, objective, **schedule(ob, 0))
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for p, v in zip(params, start):
            p.copy_(v)
    kw = schedule(ob, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused_step(emb, opt, objective, **kw)
    with torch.no_grad():            # (capturing does not execute)
        for p, v in zip(params, start):
            p.copy_(v)
    for k in range(3):
        schedule(ob, k)
        graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(params, list(emb0.xs) + list(emb0.curvature_params)):
        scale = float(want.detach().abs().max())
        assert float((got.detach() - want.detach()).abs().max()) <= S.FLOOR32 * scale
    assert float(emb.manifolds[0].c.detach()) != float(start[2]), 'the curvature did not move'
    return emb, emb0


def test_captured_fused_step_follows_the_curvature_without_recapture():
    from graphembed.objectives import StressLoss
    captured_against_eager(StressLoss, lambda ob, k: {})


def test_captured_quotient_step_follows_the_epoch_schedule():
    """QuotientLoss.on_device: eps = 1 / (epoch + 1) is read from device memory, `set_epoch` between replays moves it."""
    from graphembed.objectives import QuotientLoss

    def make():
        ob = QuotientLoss()
        ob.on_device(dev())
        return ob

    def schedule(ob, k):
        epoch, alpha = 4 * k, 1.0 - 0.1 * k
        ob.set_epoch(epoch, alpha)
        return dict(epoch=epoch, alpha=alpha)

    emb, emb0 = captured_against_eager(make, schedule)
    # the schedule matters: three eager steps at the first epoch's values end elsewhere
    emb1, opt1, target1 = train_setup('f32')
    from graphembed.modules import BatchedObjective
    ob1 = make()
    frozen = BatchedObjective(ob1, Full(target1), emb1)
    for _ in range(3):
        fused_step(emb1, opt1, frozen, **schedule(ob1, 0))
    assert any(float((a.detach() - b.detach()).abs().max()) > 100 * S.FLOOR32 * float(b.detach().abs().max()) for a, b in zip(emb1.xs, emb0.xs))
