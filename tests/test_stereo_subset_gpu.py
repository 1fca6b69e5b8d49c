"""The in-kernel node minibatch of a product of constant-curvature factors (mm_stereo_product_loss_subset, csrc/stereo.hip): every
case of tests/stereo_subset_cases.py x objective setting x {f64, f32} through the C ABI, BITWISE against mm_stereo_product_loss on
the gathered tables and against the long-double oracle; shards, reproducibility, the Python class, the route BatchedObjective
takes.

Tolerance rule (stereo_cases.bound): fp64 <= 1e-11 of the scale; fp32 <= twice the recorded reference-fp32's own deviation from
the same oracle on the same case, setting and quantity, never asked below 16 * 2^-24 of the scale.  Scales as in
test_stereo_product_gpu.py: sum |loss terms|, max |grad_x_k|, sum |g dF/dc_raw| of the factor."""
import numpy as np
import pytest
import torch

import stereo_cases as S
import stereo_product_cases as P
import stereo_subset_cases as C
from grass_cases import CallSpy
from graphembed import _backend as B
from test_stereo_gpu import DT, NP, check, cuda, dev
from test_stereo_product_gpu import abi_loss, run_objective

pytestmark = pytest.mark.gpu

GUARD = 4096   # bytes behind the workspace that must stay untouched: the workspace is the BATCH's


def device_inputs(case, dname):
    """tables with NaN rows outside the batch, curvatures, idx, the dense targets (NaN outside the batch's pairs)"""
    xs, craws, idx = C.make_inputs(case)
    return ([cuda(C.poisoned(x, idx), dname) for x in xs], [cuda(np.array([c]), dname) for c in craws],
            torch.from_numpy(idx).to(dev()), cuda(C.dense_of(case), dname))


def abi_subset(xs, cs, modes, setting, dense, idx, rows):
    """(loss [1], [grad_x_k full-size], [grad_c_k]); outputs NaN-filled, the workspace 0xFF-filled and of the batch's size"""
    n_total, bs = xs[0].shape[0], idx.numel()
    dt = B.dtype_code(xs[0])
    kind, alpha, eps, terms = P.spec_of(setting)
    gxs = [torch.full_like(x, float('nan')) for x in xs]
    gcs = [torch.full((1, ), float('nan'), dtype=x.dtype, device=x.device) for x in xs]
    loss = torch.full((1, ), float('nan'), dtype=xs[0].dtype, device=xs[0].device)
    ms = (B._c.c_int32 * len(xs))(*[x.shape[1] for x in xs])
    size = B.lib().raw('mm_stereo_product_ws_bytes')(dt, bs, len(xs), ms)
    ws = torch.full((size + GUARD, ), 0xFF, dtype=torch.uint8, device=xs[0].device)
    fs = B.stereo_factors([(x, c, gx, gc, S.C_MIN, x.shape[1], md) for x, c, gx, gc, md in zip(xs, cs, gxs, gcs, modes)])
    B.lib().call('mm_stereo_product_loss_subset', dt, kind, fs, len(xs), B.ptr(dense), n_total, B.ptr(idx), bs, rows[0], rows[1], alpha,
                 eps, terms, None, B.ptr(loss), B.ptr(ws), B.stream_of(xs[0]))
    assert bool((ws[size:] == 0xFF).all()), 'the call wrote behind a workspace of the batch\'s size'
    return loss, gxs, gcs


def gathered_call(case, dname, setting, xs, cs, idx):
    """mm_stereo_product_loss on the contiguous gathered tables with the condensed targets of the same pairs"""
    bs = case[1]
    rows = C.rows_of(case)
    lo, hi = S.pair_slice(bs, rows)
    _, t = C.pairs_of(C.base_of(case))
    target = cuda(t[lo:hi], dname) if hi > lo else None
    return abi_loss([x[idx].contiguous() for x in xs], cs, C.modes_of(case), setting, target, rows)


def compare(failures, tag, dname, o, case, name, idx, loss, gxs, gcs):
    R = S.recorded()
    ref = (lambda what: R[C.key(case, name, what, 'f32')]) if dname == 'f32' and case is not None else (lambda what: None)
    check(failures, f'{tag} loss', dname, float(loss), o['loss'], o['loss_scale'], ref('loss'))
    for k, (gx, gc) in enumerate(zip(gxs, gcs)):
        check(failures, f'{tag} grad_x[{k}]', dname, gx[idx].cpu().numpy(), o['gx'][k][idx.cpu().numpy()], np.abs(o['gx'][k]).max(), ref(f'gx{k}'))
        r = ref(f'gc{k}')
        check(failures, f'{tag} grad_c[{k}]', dname, float(gc), o['gc'][k], o['gcs'][k], None if r is None else r[0])


@pytest.mark.parametrize('name', C.SETTING_IDS)
@pytest.mark.parametrize('case', C.CASES, ids=C.CASE_IDS)
def test_case_bitwise_against_the_gathered_call_and_against_the_oracle(case, name):
    setting = C.SETTINGS[C.SETTING_IDS.index(name)]
    n_total, bs = case[:2]
    lo, hi = S.pair_slice(bs, C.rows_of(case))
    o = C.oracle(case, name)
    tag = f'{C.case_id(case)} {name}'
    failures = []
    for dname in ('f64', 'f32'):
        xs, cs, idx, dense = device_inputs(case, dname)
        loss, gxs, gcs = abi_subset(xs, cs, C.modes_of(case), setting, dense, idx, C.rows_of(case))
        loss0, gxs0, gcs0 = gathered_call(case, dname, setting, xs, cs, idx)
        rest = torch.ones(n_total, dtype=torch.bool, device=dev())
        rest[idx] = False
        assert torch.equal(loss, loss0), (tag, dname, float(loss), float(loss0))
        for k, (gx, gx0, gc, gc0) in enumerate(zip(gxs, gxs0, gcs, gcs0)):
            assert torch.equal(gx[idx], gx0), (tag, dname, k, 'grad_x differs from the gathered call')
            assert torch.equal(gx[rest], torch.zeros_like(gx[rest])), (tag, dname, k, 'a row outside the batch is not zero')
            assert torch.equal(gc, gc0), (tag, dname, k, float(gc), float(gc0))
        if hi == lo:   # the last row or an empty range: no pair
            assert float(loss) == 0.0 and all(not g.any() for g in gxs + gcs), 'a range without pairs leaves zeros'
            continue
        compare(failures, tag, dname, o, case, name, idx, loss, gxs, gcs)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('name', ['stress', 'q3', 'q3b'])
def test_shards_of_the_batch_sum_to_the_whole(name):
    """bs = 129 of 257: the row ranges of the case list, completed to a partition of the batch's rows, sum to the full launch
    within the two bounds; the ranges without a pair leave exact zeros."""
    case = C.SHARD_BASE
    setting = C.SETTINGS[C.SETTING_IDS.index(name)]
    o = C.oracle(case, name)
    cuts = [0, 1, 43, 86, 127, 128, 129]
    assert all(r in list(zip(cuts[:-1], cuts[1:])) for r in S._rows(129)[1:5])
    failures = []
    for dname in ('f64', 'f32'):
        xs, cs, idx, dense = device_inputs(case, dname)
        modes = C.modes_of(case)
        full = abi_subset(xs, cs, modes, setting, dense, idx, (0, 129))
        sums = [torch.zeros_like(t) for t in [full[0]] + full[1] + full[2]]
        for rb, re in list(zip(cuts[:-1], cuts[1:])) + [(5, 5)]:
            part = abi_subset(xs, cs, modes, setting, dense, idx, (rb, re))
            if S.pair_slice(129, (rb, re))[0] == S.pair_slice(129, (rb, re))[1]:
                assert all(not t.any() for t in [part[0]] + part[1] + part[2])
            for s, t in zip(sums, [part[0]] + part[1] + part[2]):
                s += t
        for tag, res in (('shard sum', (sums[0], sums[1:3], sums[3:5])), ('full launch', full)):
            compare(failures, f'{name} {tag}', dname, o, case, name, idx, res[0], res[1], res[2])
    assert not failures, '\n'.join(failures)


REPRO = [C.CASES[1], C.CASES[3], C.CASES[7], C.CASES[9], C.CASES[10], C.CASES[13]]


@pytest.mark.parametrize('case', REPRO, ids=C.case_id)
def test_calls_are_reproducible_and_the_class_agrees_bitwise(case):
    from graphembed.manifolds import Stereographic
    from graphembed.manifolds.stereographic import product_loss_subset
    rows = C.rows_of(case)
    for dname in ('f32', 'f64'):
        xs, cs, idx, dense = device_inputs(case, dname)
        modes = C.modes_of(case)
        mans = [Stereographic(d, c_init=c, c_min=S.C_MIN, keep_sign_fixed=f).to(device=dev(), dtype=DT[dname])
                for d, c, f in zip(case[2], case[3], case[4])]
        cache = {}
        for name in ('stress', 'q3b'):
            setting = C.SETTINGS[C.SETTING_IDS.index(name)]
            a, b = abi_subset(xs, cs, modes, setting, dense, idx, rows), abi_subset(xs, cs, modes, setting, dense, idx, rows)
            assert all(torch.equal(u, v) for u, v in zip([a[0]] + a[1] + a[2], [b[0]] + b[1] + b[2])), 'two calls differ'
            leaves = [x.clone().requires_grad_() for x in xs]
            for man in mans:
                man.c.grad = None
            kind, alpha, eps, terms = P.spec_of(setting)
            loss = product_loss_subset(mans, leaves, idx, dense, ('stress' if kind == 1 else 'quotient', alpha, eps, terms), cache,
                                       rows=None if case[6] is None else rows)
            assert torch.equal(loss.detach().reshape(1), a[0]), 'the class and the C ABI disagree (loss)'
            loss.backward()
            for x, man, gx, gc in zip(leaves, mans, a[1], a[2]):
                assert torch.equal(x.grad, gx) and torch.equal(man.c.grad.to(gc.dtype), gc), 'the class and the C ABI disagree (backward)'
        assert len(cache) == 1, 'one cached workspace per (dtype, device, batch size)'


# ---- the route BatchedObjective takes ------------------------------------------------------------------------------------------
ROUTE_CASE = P.CASES[3]   # n = 65, ds = [5, 5], c = (0.01, -0.3)
BATCH = np.random.RandomState(11).permutation(65)[:23]


class Dense:
    """the dataset protocol of BatchedObjective over a dense target matrix; `pdists` (GraphDataset's attribute) only on request"""

    def __init__(self, dname, device=None, with_pdists=True, dtype=None):
        target = P.pairs_of(ROUTE_CASE)[1]
        full = torch.from_numpy(target.astype(NP[dname]))
        dense = torch.zeros(65, 65, dtype=full.dtype)
        a, b = torch.triu_indices(65, 65, 1)
        dense[a, b] = full
        self._dense = (dense + dense.T).to(device or dev())
        if dtype is not None:
            self._dense = self._dense.to(dtype)
        if with_pdists:
            self.pdists = self._dense

    def __getitem__(self, i):
        n = 65 if i is None else len(i)
        src = self._dense if i is None else self._dense[i.to(self._dense.device)][:, i.to(self._dense.device)]
        p, q = torch.triu_indices(n, n, 1)
        return src[p, q]


def route_embedding(dname):
    from graphembed.modules import StereographicProductEmbedding
    emb = StereographicProductEmbedding(65, [5, 5]).to(device=dev(), dtype=DT[dname])
    xs, craws = P.make_inputs(ROUTE_CASE)
    with torch.no_grad():
        for p, man, x, c in zip(emb.xs, emb.manifolds, xs, craws):
            p.copy_(cuda(x, dname))
            man.c.fill_(float(c))
    return emb


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['stress', 'q3'])
def test_batched_objective_keeps_the_minibatch_inside_the_kernel(name, dname):
    from graphembed.objectives import QuotientLoss, StochasticNeighborLoss, StressLoss
    objective = StressLoss() if name == 'stress' else QuotientLoss()
    kw = dict(epoch=1, alpha=1.0)
    emb = route_embedding(dname)
    idx = torch.from_numpy(BATCH)
    loss, gxs, gcs, calls = run_objective(emb, objective, Dense(dname), idx, **kw)
    assert calls.count('mm_stereo_product_loss_subset') == 1, calls
    assert 'mm_stereo_product_loss' not in calls and 'mm_pair_gather' not in calls and not any(c.startswith('mm_stereo_pdist_') for c in calls), calls
    # today's route (take_rows + mm_stereo_product_loss) over a dataset without `pdists`: the same numbers, bitwise
    loss0, gxs0, gcs0, calls0 = run_objective(emb, objective, Dense(dname, with_pdists=False), idx, **kw)
    assert calls0.count('mm_stereo_product_loss') == 1 and 'mm_stereo_product_loss_subset' not in calls0, calls0
    assert torch.equal(loss, loss0) and all(torch.equal(u, v) for u, v in zip(gxs + gcs, gxs0 + gcs0))
    rest = torch.ones(65, dtype=torch.bool)
    rest[idx] = False
    assert all(not g[rest.to(dev())].any() and bool(g[idx.to(dev())].any()) for g in gxs)
    # a device-side index vector takes the same route to the same numbers
    loss1, gxs1, gcs1, calls1 = run_objective(emb, objective, Dense(dname), idx.to(dev()), **kw)
    assert calls1.count('mm_stereo_product_loss_subset') == 1 and torch.equal(loss1, loss) and all(torch.equal(u, v) for u, v in zip(gxs1, gxs))

    def falls_back(data, ob=objective, **attrs):
        for k, v in attrs.items():
            setattr(emb, k, v)
        try:
            res = run_objective(emb, ob, data, idx, **kw)
        finally:
            for k in attrs:
                delattr(emb, k)
        assert 'mm_stereo_product_loss_subset' not in res[3], res[3]
        return res

    other = torch.float64 if dname == 'f32' else torch.float32
    for res in (falls_back(Dense(dname, device='cpu')), falls_back(Dense(dname, dtype=other))):
        assert res[3].count('mm_stereo_product_loss') == 1 and torch.equal(res[0], loss0)
    res = falls_back(Dense(dname), pair_kernel=False)
    assert res[3].count('mm_stereo_pdist_fwd') == 2 and not any(c.startswith('mm_stereo_product_') for c in res[3]), res[3]
    res = falls_back(Dense(dname), ob=StochasticNeighborLoss())
    assert res[3].count('mm_stereo_product_pdist_fwd') == 1 and res[3].count('mm_stereo_product_loss') == 1, res[3]
    # host-side indices: out of range raises like the reference's x[idx]; repeats go the gather route, which accumulates them
    with pytest.raises(IndexError):
        run_objective(emb, objective, Dense(dname), torch.tensor([1, 65, 3]), **kw)
    with pytest.raises(IndexError):
        run_objective(emb, objective, Dense(dname), torch.tensor([1, -66, 3]), **kw)
    twice = torch.tensor([4, 9, 4, 30])
    res = run_objective(emb, objective, Dense(dname), twice, **kw)
    assert 'mm_stereo_product_loss_subset' not in res[3] and res[3].count('mm_stereo_product_loss') == 1, res[3]
