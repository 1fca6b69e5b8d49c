"""The bit-deterministic SPD pair kernels on the GPU (csrc/spd_det.hpp; mm_spd_pdist_bwd_det / mm_spd_pdist_loss_det through the C
ABI and through graphembed) against the fp64 oracles of tests/spd_det_cases.py, whose docstring states the cases, the rule
(e_det <= 2 e_atomic + 64 eps S, e_atomic the deviation from the same oracle of the atomic entry on the same GPU in the same test)
and the teeth (the allowance granted to grad_x stays below half of what ONE replaced pair value moves it by).  Then what the mode
exists for: the same bits on every call — repeated, with det_ws full of NaN, prepared or not, eagerly or replayed — and the routes
that lead to it.  Every figure is printed before it is judged (-rA); the last test prints the worst per sweep, dtype and quantity:
profiles/spd_deterministic.md."""
import ctypes

import pytest
import torch

import grass_cases as gc
import spd_det_cases as C

pytestmark = pytest.mark.gpu
DET = {'bwd': 'mm_spd_pdist_bwd_det', 'loss': 'mm_spd_pdist_loss_det'}
ATOMIC = {'bwd': 'mm_spd_pdist_bwd', 'loss': 'mm_spd_pdist_loss'}


def _B():
    from graphembed import _backend as B
    return B


def dev(t, dname):
    return t.to(C.DT[dname]).cuda().contiguous()


def workspace(dname, D, n, fill=None):
    B = _B()
    nbytes = B.lib().raw('mm_spd_pdist_ws_bytes')(B.MM_F32 if dname == 'f32' else B.MM_F64, n, D)
    return torch.empty(nbytes, dtype=torch.uint8, device='cuda') if fill is None else torch.full((nbytes, ), fill, dtype=torch.uint8, device='cuda')


def det_workspace(dname, D, n, nan=True):
    """det_ws full of NaN (as floats of the case's dtype) or of 0xFF bytes"""
    B = _B()
    nbytes = B.lib().raw('mm_spd_pdist_det_ws_bytes')(B.MM_F32 if dname == 'f32' else B.MM_F64, n, D)
    esz = 4 if dname == 'f32' else 8
    assert nbytes % esz == 0
    return torch.full((nbytes // esz, ), float('nan'), dtype=C.DT[dname], device='cuda')


def raw_call(c, x, vec, det, ws=None, det_ws=None, flags=0, prepare=False):
    """the C entry of the case's kind in the deterministic (`det`) or the atomic mode, outputs pre-filled with NaN:
    (loss [1], grad_x [n, D, D], grad_scale [1]) — the bwd kinds return zeros for the loss record"""
    B = _B()
    dname = 'f32' if x.dtype == torch.float32 else 'f64'
    rb, re = (0, c.n) if c.rows is None else c.rows
    ws = workspace(dname, c.D, c.n, 0xFF) if ws is None else ws
    grad = torch.full_like(x, float('nan'))
    out = torch.full((2, ), float('nan'), dtype=x.dtype, device='cuda')
    extra = ()
    if det:
        det_ws = det_workspace(dname, c.D, c.n) if det_ws is None else det_ws
        extra = (B.ptr(det_ws), )
    with B.on_device(x.device):
        if prepare:
            B.lib().call('mm_spd_prepare', B.dtype_code(x), B.ptr(x), c.n, c.D, B.ptr(ws), B.stream_of(x))
        if c.kind in C.LOSS_KINDS:
            kind, alpha, eps, terms = C.S.loss_spec(c.kind)
            sc = torch.tensor([C.SCALE_RAW], dtype=x.dtype, device='cuda')
            B.lib().call((DET if det else ATOMIC)['loss'], B.dtype_code(x), kind, B.ptr(x), B.ptr(vec), B.ptr(sc), c.n, c.D, rb, re,
                         alpha, eps, terms, None, C.WMIN, C.WMAX, B.ptr(out), B.ptr(grad), B.ptr(ws), *extra, flags, B.stream_of(x))
        else:
            B.lib().call((DET if det else ATOMIC)['bwd'], B.dtype_code(x), B.ptr(x), B.ptr(vec), c.n, c.D, rb, re,
                         int(c.kind == 'bwd_sq'), C.WMIN, C.WMAX, B.ptr(grad), B.ptr(ws), *extra, flags, B.stream_of(x))
            out.zero_()
    torch.cuda.synchronize()
    return out[0:1].clone(), grad, out[1:2].clone()


def finite(res):
    return all(bool(torch.isfinite(t).all()) for t in res)


def all_zero(res):
    return all(float(t.abs().max()) == 0.0 for t in res if t.numel())


def judge(sweep, c, dname, atomic, det, failures):
    want = C.oracle(c)
    tag = C.case_id(c)
    assert finite(det), tag
    granted = C.hold(sweep, tag, dname, c, atomic, det, want, failures)
    effect = C.one_pair_effect(c)
    line = f'{tag} {dname}: allowance of grad_x {granted["grad_x"]:.3e}, one replaced pair value moves it by {effect:.3e}'
    print(line)
    if not granted['grad_x'] < 0.5 * effect:
        failures.append(line + ': the rule could hide a wrong pair')
    return granted


def run_case(sweep, c, dname, failures):
    x, vec = dev(C.points(c.regime, c.D, c.n), dname), dev(C.loaded(c), dname)
    det = raw_call(c, x, vec, True)
    if not C.n_pairs(c):      # a range without a pair: a zero loss record and an all-zero gradient
        assert all_zero(det) and all_zero(C.oracle(c)[:3]), C.case_id(c)
        return det, None
    atomic = raw_call(c, x, vec, False)
    return det, judge(sweep, c, dname, atomic, det, failures)


# ---- 1. every instantiation, in every regime -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', C.DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_every_instantiation(dname, D):
    """the four kernels of this (dtype, D) in `init` (close pairs), `mid` and `wide` (the far-pair paths), n = 130: 17 chunks"""
    failures = []
    cases = [c for c in C.instantiation_cases() if c.D == D]
    assert len(cases) == 12
    for c in cases:
        run_case('instantiations', c, dname, failures)
    assert not failures, '\n'.join(failures)


# ---- 2. sizes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', C.SIZE_DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_sizes(dname, D):
    """one pair, three pairs, a size at a chunk boundary and one past it, ragged last chunks, one column past a workgroup"""
    failures = []
    cases = [c for c in C.size_cases() if c.D == D]
    assert len(cases) == 24
    for c in cases:
        run_case('sizes', c, dname, failures)
    assert not failures, '\n'.join(failures)


def test_several_column_groups_times_several_chunks():
    """SPD(3) fp32 at n = 1025: 5 column groups x 129 chunks"""
    failures = []
    for c in C.large_cases():
        run_case('large', c, 'f32', failures)
    assert not failures, '\n'.join(failures)


# ---- 3. row shards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('D', C.SHARD_DIMS)
@pytest.mark.parametrize('dname', C.DNAMES)
def test_row_shards(dname, D, kind):
    """every range of SHARDS against the oracle's explicit pair list; the ranges of COVER add up to the full range within the rule"""
    failures, results = [], {}
    for rows in C.SHARDS:
        results[rows] = run_case('row shards', C.Case('mid', D, C.N_SHARD, kind, rows), dname, failures)
    whole, granted = results[None]
    for k, name in enumerate(C.NAMES):
        if name not in granted:
            continue
        total = sum(results[rows][0][k].double() for rows in C.COVER)
        err = float((total - whole[k].double()).abs().max())
        print(f'spd({D}) {kind} {dname} {name}: sum over COVER differs from the full range by {err:.3e}, allowance {granted[name]:.3e}')
        if not err <= granted[name]:
            failures.append(f'sum over COVER, {name}: {err:.3e} > {granted[name]:.3e}')
    assert not failures, '\n'.join(failures)


# ---- 4. the same bits ------------------------------------------------------------------------------------------------------------------------
def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('D', (2, 3, 4, 6))
@pytest.mark.parametrize('dname', C.DNAMES)
def test_bitwise(dname, D, kind):
    """torch.equal on grad_x and the loss record: five calls; det_ws full of NaN against one that keeps the previous call's
    records; an unprepared ws against mm_spd_prepare + MM_WS_PREPARED; det -> atomic -> det on ONE ws, where the atomic call
    finds clean accumulators (it agrees with an atomic call on a fresh workspace to the oracle rule's floor, 64 eps S)"""
    B = _B()
    for n in (C.N_INST, 257):
        c = C.Case('mid', D, n, kind, None)
        x, vec = dev(C.points(c.regime, c.D, c.n), dname), dev(C.loaded(c), dname)
        first = raw_call(c, x, vec, True)
        assert finite(first)
        kept = det_workspace(dname, D, n)
        for k in range(4):
            assert same(first, raw_call(c, x, vec, True, det_ws=kept if k % 2 else None)), (C.case_id(c), k)
        assert same(first, raw_call(c, x, vec, True, flags=B.MM_WS_PREPARED, prepare=True)), C.case_id(c)
        ws = workspace(dname, D, n, 0xFF)
        assert same(first, raw_call(c, x, vec, True, ws=ws)), C.case_id(c)
        after = raw_call(c, x, vec, False, ws=ws, flags=B.MM_WS_PREPARED)     # the tables of the det call, its untouched accumulators
        assert same(first, raw_call(c, x, vec, True, ws=ws, flags=B.MM_WS_PREPARED)), C.case_id(c)
        fresh = raw_call(c, x, vec, False)
        want = C.oracle(c)
        for k, name in enumerate(C.NAMES):
            if name in C.names_of(c):
                err = float((after[k].double() - fresh[k].double()).abs().max())
                floor = 64 * C.eps_of(C.DT[dname]) * want.S[name]
                print(f'{C.case_id(c)} {dname} {name}: atomic after det differs from atomic on a fresh workspace by {err:.3e}, floor {floor:.3e}')
                assert err <= floor, (C.case_id(c), name, err, floor)


@pytest.mark.parametrize('dname', C.DNAMES)
def test_status_word_of_a_non_pd_point(dname):
    B = _B()
    c = C.Case('mid', 3, 65, 'stress', None)
    x, vec = dev(C.points(c.regime, c.D, c.n), dname), dev(C.loaded(c), dname)
    x[7] = -x[7]
    x[40, 0, 0] = 0.0
    status = []
    for det in (True, False):
        ws = workspace(dname, c.D, c.n, 0xFF)
        raw_call(c, x, vec, det, ws=ws)
        st = ctypes.c_int(-1)
        B.lib().call('mm_spd_status', B.ptr(ws), c.n, ctypes.byref(st), None)
        status.append(st.value)
    assert status[0] == status[1] and status[0] >= 1, status


# ---- 5. the routes ---------------------------------------------------------------------------------------------------------------------------
def _embedding(D, n, dt, deterministic, manifolds=None):
    from graphembed import manifolds as M
    from graphembed.modules import ManifoldEmbedding
    torch.set_default_dtype(dt)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, manifolds or [M.SymmetricPositiveDefinite(D, deterministic=deterministic)])
    finally:
        torch.set_default_dtype(torch.float32)
    dname = 'f32' if dt == torch.float32 else 'f64'
    with torch.no_grad():
        emb.xs[0].copy_(dev(C.points('mid', D, n), dname))
        for s in emb.scales:
            s.fill_(C.SCALE_RAW)
    return emb


def _dataset(D, n, dt):
    from graphembed.data.dataset import GraphDataset
    return GraphDataset(C.targets('mid', D, n).to(dt).cuda().sqrt())


def _opts(emb):
    from graphembed.optim import RiemannianSGD
    return [RiemannianSGD(list(emb.xs), lr=2e-3, exact=True, max_grad_norm=20), RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)]


def _pdist_calls(spy):
    """the objective's entries among the calls (a minibatch also gathers its targets: mm_pair_gather; the mixed-manifold pair
    kernel a plain SPD(3) minibatch takes is mm_product_pairs_loss_subset)"""
    return [name for name in spy.calls if 'pdist' in name or 'pairs_loss' in name]


def _one_step(emb, objective, idx=None):
    for p in emb.parameters():
        p.grad = None
    with gc.CallSpy() as spy:
        loss = objective(idx) if idx is not None else objective(None)
        loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in emb.parameters())
    return _pdist_calls(spy), loss.detach().clone(), [p.grad.clone() for p in emb.parameters()]


@pytest.mark.parametrize('loss_name', C.LOSS_KINDS)
def test_routes(loss_name):
    from graphembed.modules import BatchedObjective
    D, n, dt = 3, 257, torch.float32
    fn, kw = gc.objective(loss_name)
    data = _dataset(D, n, dt)
    idx = C.S.batch_idx(65)
    # a deterministic manifold: full batch through fused_objective and through BatchedObjective, and a node minibatch of 65 of
    # 257 — nothing but the _det entries, and the same bits twice
    emb = _embedding(D, n, dt, True)
    runs = {'fused_objective': lambda i: emb.fused_objective(fn, data[None], None, **kw),
            'BatchedObjective': lambda i: BatchedObjective(fn, data, emb)(i, **kw)}
    for what, objective, i in (('fused_objective', runs['fused_objective'], None), ('BatchedObjective', runs['BatchedObjective'], None),
                               ('BatchedObjective, 65 of 257', runs['BatchedObjective'], idx)):
        a, b = _one_step(emb, objective, i), _one_step(emb, objective, i)
        assert a[0] == [DET['loss']] and b[0] == a[0], (what, a[0])
        assert torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2])), what
        if i is not None:
            outside = torch.ones(n, dtype=torch.bool, device='cuda')
            outside[i.cuda()] = False
            assert float(a[2][0][outside].abs().max()) == 0.0 and float(a[2][0][~outside].abs().max()) > 0
    # the unfused composition: pdist's backward through the deterministic entry, hosted by the Python autograd class
    man = emb.manifolds[0]
    xl = emb.xs[0].detach().clone().requires_grad_()
    with gc.CallSpy() as spy:
        d2 = man.pdist(xl, squared=True)
        (d2 * dev(C.upstream('mid', D, n), 'f32')).sum().backward()
    assert _pdist_calls(spy) == ['mm_spd_pdist_fwd', DET['bwd']], spy.calls
    # the default manifold keeps the old entries — full batch, minibatch inside the pair kernel, pdist under the C++ node
    plain = _embedding(D, n, dt, None)
    calls = _one_step(plain, lambda i: BatchedObjective(fn, data, plain)(i, **kw))[0]
    assert calls == [ATOMIC['loss']], calls
    calls = _one_step(plain, lambda i: BatchedObjective(fn, data, plain)(i, **kw), idx)[0]
    assert calls and not any(name.endswith('_det') for name in calls), calls
    xl = plain.xs[0].detach().clone().requires_grad_()
    with gc.CallSpy() as spy:
        plain.manifolds[0].pdist(xl, squared=True).sum().backward()
    assert not any(name.endswith('_det') for name in spy.calls), spy.calls
    if _B().autograd_ext() is not None:
        assert not _pdist_calls(spy), spy.calls      # both calls were issued by the C++ node
    # torch's switch flips a deterministic=None manifold, and back
    assert not torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        calls = _one_step(plain, lambda i: plain.fused_objective(fn, data[None], None, **kw))[0]
    finally:
        torch.use_deterministic_algorithms(False)
    assert calls == [DET['loss']], calls
    assert _one_step(plain, lambda i: plain.fused_objective(fn, data[None], None, **kw))[0] == [ATOMIC['loss']]


def test_product_with_a_deterministic_factor_takes_the_per_factor_kernels():
    from graphembed import manifolds as M
    D, n, dt = 2, 65, torch.float32
    fn, kw = gc.objective('stress')
    emb = _embedding(D, n, dt, True, manifolds=[M.SymmetricPositiveDefinite(D, deterministic=True), M.Euclidean(4)])
    with torch.no_grad():
        emb.xs[1].copy_(torch.randn(n, 4, generator=torch.Generator().manual_seed(3)).cuda())
    target = C.targets('mid', D, n).cuda()
    with gc.CallSpy() as spy:
        loss = emb.fused_objective(fn, target, None, **kw)
        loss.backward()
    assert 'mm_product_loss' in spy.calls and DET['bwd'] in spy.calls, spy.calls
    assert not any(name in spy.calls for name in ('mm_product_pairs_loss', ATOMIC['bwd'], ATOMIC['loss'])), spy.calls


def _train(D, dt, graphed, steps=20, n=65):
    from graphembed.graphed import GraphedTrainStep
    from graphembed.objectives import StressLoss
    emb = _embedding(D, n, dt, True)
    target = C.targets('mid', D, n).to(dt).cuda()
    opts = _opts(emb)
    fn = StressLoss()
    losses = []
    if graphed:
        step = GraphedTrainStep(lambda: emb.fused_objective(fn, target, None), opts, warmup=3).capture()
        losses = [v.clone() for v in step.warmup_losses] + [step().clone() for _ in range(steps - 3)]
    else:
        for _ in range(steps):
            for o in opts:
                o.zero_grad(set_to_none=True)
            loss = emb.fused_objective(fn, target, None)
            loss.backward()
            for o in opts:
                o.step()
            losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return emb.xs[0].detach().clone(), emb.scales[0].detach().clone(), torch.stack(losses)


@pytest.mark.parametrize('D,dt', [(3, torch.float32), (4, torch.float64)], ids=['spd3-f32', 'spd4-f64'])
def test_twenty_steps_end_in_the_same_bits(D, dt):
    """twenty RSGD steps from one initialisation, twice eagerly and twice as a GraphedTrainStep replay: points, scale and every
    loss torch.equal — between the repeats and between eager and replayed"""
    runs = {(g, k): _train(D, dt, g) for g in (False, True) for k in (0, 1)}
    ref = runs[(False, 0)]
    assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[2]).all())
    assert not torch.equal(ref[0], dev(C.points('mid', D, 65), 'f32' if dt == torch.float32 else 'f64'))
    for key, run in runs.items():
        for name, a, b in zip(('points', 'scale', 'losses'), ref, run):
            assert torch.equal(a, b), (key, name, float((a.double() - b.double()).abs().max()))


def test_native_train_step_refuses_a_deterministic_manifold():
    from graphembed.native_step import NativeTrainStep
    from graphembed.objectives import StressLoss
    D, n, dt = 3, 65, torch.float32
    target = C.targets('mid', D, n).cuda()
    emb = _embedding(D, n, dt, True)
    with pytest.raises(ValueError, match='deterministic'):
        NativeTrainStep(emb, StressLoss(), target, _opts(emb))
    plain = _embedding(D, n, dt, None)
    step = NativeTrainStep(plain, StressLoss(), target, _opts(plain))
    assert bool(torch.isfinite(step()))
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(ValueError, match='deterministic'):
            step()
    finally:
        torch.use_deterministic_algorithms(False)


# ---- last: the figures -------------------------------------------------------------------------------------------------------------------
def test_print_worst_ratios():
    """(last in the file) per sweep, dtype and quantity the worst e_det / allowance, e_det / S and e_atomic / S of this session"""
    worst = {}
    for sweep, dname, name, r_allow, r_det, r_atomic, tag in C.RECORDS:
        w = worst.setdefault((sweep, dname, name), [0.0, 0.0, 0.0, 0])
        w[0], w[1], w[2], w[3] = max(w[0], r_allow), max(w[1], r_det), max(w[2], r_atomic), w[3] + 1
    print('sweep | dtype | quantity | calls | e_det / allowance | e_det / S | e_atomic / S')
    for (sweep, dname, name), (r_allow, r_det, r_atomic, count) in sorted(worst.items()):
        print(f'{sweep} | {dname} | {name} | {count} | {r_allow:.3f} | {r_det:.2e} | {r_atomic:.2e}')
