"""The bit-deterministic vector pair kernels on the GPU (csrc/vec_det.hpp; mm_vec_pdist_bwd_det / mm_vec_pdist_loss_det /
mm_vec_pdist_loss_subset_det through the C ABI and through graphembed) against the fp64 oracle of tests/vec_det_cases.py, whose
docstring states the cases and the two rules every call is held to: the project's bounds (vec_cases.errors) and
e_det <= 2 e_atomic + 64 eps S, e_atomic the deviation from the same oracle of the default atomic entry in the same test.  Then
what the mode exists for: the same bits on every call — repeated, with det_ws full of NaN or of 0xFF bytes, under every
environment switch of the atomic kernels, eagerly or replayed, around an atomic call, a minibatch against the full batch of its
gathered rows — and the routes that lead to it.  Every figure is printed before it is judged (-rA); the last test prints the
worst per sweep, dtype and quantity: profiles/vec_deterministic.md.

Run as a script (`python tests/test_vec_det_gpu.py --digests`) it prints the SHA-256 digests of the results of DIGEST_CASES: the
library reads its environment switches once per process, so the environments of vec_cases.ENVS are fresh children."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import vec_det_cases as C  # noqa: E402

vc = C.vc
pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'f64': torch.float64}
DET = {'bwd': 'mm_vec_pdist_bwd_det', 'loss': 'mm_vec_pdist_loss_det', 'subset': 'mm_vec_pdist_loss_subset_det'}
ATOMIC = {'bwd': 'mm_vec_pdist_bwd', 'loss': 'mm_vec_pdist_loss', 'subset': 'mm_vec_pdist_loss_subset'}
ATOMIC_ALL = ('mm_vec_pdist_bwd', 'mm_vec_pdist_bwd_gram', 'mm_vec_pdist_loss', 'mm_vec_pdist_loss_subset', 'mm_product_pairs_loss',
              'mm_product_pairs_loss_subset')


def _B():
    from graphembed import _backend as B
    return B


def _dev(a, dt):
    return torch.from_numpy(np.array(a)).to(device='cuda', dtype=dt)      # (a copy: the table's arrays are read-only)


class Call:
    """The device buffers of one case and its call into the library, in either mode."""

    def __init__(self, c):
        B = _B()
        self.c, self.dt, self.inp = c, DT[c['dname']], C.inputs(c)
        self.dtc = B.MM_F32 if c['dname'] == 'f32' else B.MM_F64
        self.kind = vc.KIND_CODE[c['kind']]
        self.x = _dev(self.inp['x'], self.dt)
        self.n, self.rb, self.re = C.call_rows(c)
        self.scale = torch.tensor([self.inp['scale']], dtype=self.dt, device='cuda') if c['loss'] and c['scale'] else None
        self.idx = None if self.inp['idx'] is None else torch.from_numpy(self.inp['idx']).cuda()
        side = self.inp['dense'] if c['batch'] else (self.inp['g'] if c['entry'] == 'bwd' else self.inp['target'])
        self.side = _dev(side, self.dt)
        self.grad = torch.empty_like(self.x)
        self.out = torch.empty(2, dtype=self.dt, device='cuda')

    def det_ws(self, fill='nan'):
        nbytes = _B().lib().raw('mm_vec_pdist_det_ws_bytes')(self.dtc, self.kind, self.n, self.c['m'])
        esz = 4 if self.c['dname'] == 'f32' else 8
        assert nbytes % esz == 0 and nbytes >= 64
        if fill == 'nan':
            return torch.full((nbytes // esz, ), float('nan'), dtype=self.dt, device='cuda')
        return torch.full((nbytes, ), 0xFF, dtype=torch.uint8, device='cuda')

    def atomic_ws(self):
        nbytes = _B().lib().raw('mm_vec_pdist_ws_bytes')(self.dtc, self.x.shape[0], self.c['m'])
        return torch.full((nbytes, ), 255, dtype=torch.uint8, device='cuda')      # the library clears what it needs

    def enqueue(self, det, ws):
        """the C call alone, on the current stream, into self.out / self.grad: capture-safe; returns the code"""
        B = _B()
        c, lib, x = self.c, B.lib(), self.x
        name = (DET if det else ATOMIC)[c['entry']]
        some = lambda t: B.ptr(t) if t is not None and t.numel() else None      # noqa: E731
        stream = B.stream_of(x)
        if c['entry'] == 'bwd':
            return lib.raw(name)(self.dtc, self.kind, B.ptr(x), some(self.side), self.n, c['m'], self.rb, self.re, int(c['squared']),
                                 B.ptr(self.grad), B.ptr(ws), stream)
        loss = vc.loss_of(c)
        code, alpha, eps = vc.LOSS_CODE[loss['kind']], float(loss.get('alpha', 1.0)), 1.0 / (loss.get('epoch', 0) + 1)
        if c['entry'] == 'subset':
            return lib.raw(name)(self.dtc, self.kind, code, B.ptr(x), some(self.side), some(self.scale), x.shape[0], c['m'], some(self.idx),
                                 self.n, self.rb, self.re, alpha, eps, vc.terms_of(c), None, B.ptr(self.out), B.ptr(self.grad), B.ptr(ws), stream)
        return lib.raw(name)(self.dtc, self.kind, code, B.ptr(x), some(self.side), some(self.scale), self.n, c['m'], self.rb, self.re, alpha,
                             eps, vc.terms_of(c), None, B.ptr(self.out), B.ptr(self.grad), B.ptr(ws), stream)

    def run(self, det=True, ws=None):
        """(loss record [2], grad) as device tensors, the outputs pre-filled with NaN (a row never written is seen); the atomic
        minibatch entry gets a zero-filled gradient, as in tests/test_vec_oracle_gpu.py"""
        if ws is None:
            ws = self.det_ws() if det else self.atomic_ws()
        self.grad.fill_(0.0 if (self.c['batch'] and not det) else float('nan'))
        self.out.fill_(float('nan'))
        rc = self.enqueue(det, ws)
        torch.cuda.synchronize()
        assert rc == 0, (self.c['id'], det, rc)
        if self.c['entry'] == 'bwd':
            self.out.zero_()
        return self.out.clone(), self.grad.clone()

    def result(self, res):
        """a result in the form of vec_cases.evaluate, numpy fp64"""
        out, grad = res
        g = grad.double().cpu().numpy()
        if self.c['entry'] == 'bwd':
            return g
        o = out.double().cpu().numpy()
        return float(o[0]), g, float(o[1])


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def plus_zero(t):
    """every element is +0 (torch.equal takes -0 for 0)"""
    return bool((t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) == 0).all())


def run_case(sweep, c, failures, keep=None):
    call = Call(c)
    det = call.run(True)
    if not C.n_pairs(c):      # a range without a pair: a zero loss record and an all-zero gradient, finalize alone
        ok = float(det[0].abs().max()) == 0.0 and float(det[1].abs().max()) == 0.0
        print(f"{c['id']}: no pair, {'all zero' if ok else 'NOT ZERO'}")
        if not ok:
            failures.append(f"{c['id']}: a range without a pair is not all zero")
    else:
        atomic = call.run(False)
        C.hold(sweep, c, call.result(atomic), call.result(det), failures)
    if c['batch']:      # rows outside the batch: exactly +0
        rest = torch.ones(vc.N_TABLE, dtype=torch.bool, device='cuda')
        rest[call.idx] = False
        if not plus_zero(det[1][rest]):
            failures.append(f"{c['id']}: gradient rows outside the batch are not +0")
    if keep is not None:
        keep[c['id']] = (call, det)
    return call, det


# ---- 1. accuracy: every case against the oracle, under both rules ----------------------------------------------------------------------
GROUPS = [(d, k) for d in C.DNAMES for k in vc.KINDS]
GROUP_IDS = [f'{d}-{k}' for d, k in GROUPS]


def _mine(cases, dname, kind):
    return [c for c in cases if c['dname'] == dname and c['kind'] == kind]


@pytest.mark.parametrize('dname,kind', GROUPS, ids=GROUP_IDS)
def test_every_instantiation(dname, kind):
    """n = 131 (17 chunks, a ragged last one of 3 rows): every padded width at both ends x {bwd squared, bwd plain, stress, a
    quotient term selection}, and the losses without a scale at the primary width"""
    failures = []
    cases = _mine(C.instantiation_cases(), dname, kind)
    assert len(cases) == 4 * (18 if kind == 'euclidean' else 17) + 2
    for c in cases:
        run_case('instantiations', c, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname,kind', GROUPS, ids=GROUP_IDS)
def test_sizes(dname, kind):
    """one pair, three pairs, a size AT a chunk boundary and one row past it, one column past a 256-column workgroup"""
    failures = []
    cases = _mine(C.size_cases(), dname, kind)
    assert len(cases) == 4 * len(C.SIZES)
    for c in cases:
        run_case('sizes', c, failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname,kind', GROUPS, ids=GROUP_IDS)
def test_row_shards(dname, kind):
    """every range against the oracle's explicit pair list; each shard's result is bitwise repeatable; the shards of
    vec_cases.shards(131) add up to the whole within the sum of the bounds"""
    failures, results = [], {}
    cases = _mine(C.shard_cases(), dname, kind)
    assert len(cases) == 4 * 7
    for c in cases:
        call, det = run_case('shards', c, failures, keep=results)
        if not same(det, call.run(True)):
            failures.append(f"{c['id']}: two calls differ")
    for c in cases:
        if c['rows'] is not None:
            continue
        parts = [C.BY_ID[vc.case(c['entry'], c['kind'], c['m'], c['dname'], c['squared'], c['loss'], rows=r)['id']] for r in vc.shards(vc.N)]
        call, det = results[c['id']]
        whole = call.result(det)
        got = [results[p['id']][0].result(results[p['id']][1]) for p in parts]
        summed = tuple(sum(g[k] for g in got) for k in range(3)) if c['loss'] else sum(got)
        bound = {q: sum(vc.errors(p, C.oracle(p)[0], r)[q][1] for p, r in zip(parts + [c], got + [whole])) for q in vc.errors(c, C.oracle(c)[0], whole)}
        errs = {q: (e, bound[q]) for q, (e, _) in vc.errors(c, whole, summed).items()}
        print(f"{c['id']} shards summed against the whole: " + ', '.join(f'{q} {e:.3e} / {a:.3e}' for q, (e, a) in errs.items()))
        for q, (e, a) in errs.items():
            if not e <= a:
                failures.append(f"{c['id']}: shards summed, {q}: {e:.3e} > {a:.3e}")
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('dname,kind', GROUPS, ids=GROUP_IDS)
def test_minibatches(dname, kind):
    """batches of 2, 17 and 70 of 200 nodes, widths 3, 11, 24, 64, both losses; an asymmetric dense matrix; a row shard of a batch"""
    failures = []
    cases = _mine(C.minibatch_cases(), dname, kind)
    assert len(cases) == 24 + (4 if kind == 'lorentz' else 0)
    for c in cases:
        run_case('minibatches', c, failures)
    assert not failures, '\n'.join(failures)


# ---- 2. the same bits ----------------------------------------------------------------------------------------------------------------
def bit_cases(dname, kind):
    m = vc.PRIMARY[kind]
    out = [vc.case(entry, kind, m, dname, sq, loss, n=n) for n in (vc.N, 257) for entry in ('bwd', 'loss') for sq, loss in vc._variants(entry)]
    out += [vc.case('subset', kind, w, dname, True, loss, batch=70) for w in (m, 64) for _, loss in vc._variants('subset') if w in C.SUB_WIDTHS]
    return [C.BY_ID[c['id']] for c in out]


@pytest.mark.parametrize('dname,kind', GROUPS, ids=GROUP_IDS)
def test_bitwise(dname, kind):
    """torch.equal on grad_x and the loss record: the same call again; det_ws full of NaN, of 0xFF bytes, and one that keeps the
    previous call's records; eager against a captured and replayed graph; the deterministic entry, then the atomic entry, then
    the deterministic entry again"""
    for c in bit_cases(dname, kind):
        call = Call(c)
        first = call.run(True)
        assert bool(torch.isfinite(first[1]).all()) and bool(torch.isfinite(first[0]).all()), c['id']
        kept = call.det_ws('nan')
        for k, ws in enumerate((None, kept, call.det_ws('ff'), kept, call.det_ws('ff'))):
            assert same(first, call.run(True, ws=ws)), (c['id'], k)
        call.run(False)
        assert same(first, call.run(True, ws=kept)), (c['id'], 'after the atomic entry')
        # captured and replayed: the call allocates nothing and does not synchronise
        ws = call.det_ws('nan')
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert call.enqueue(True, ws) == 0
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = call.enqueue(True, ws)
        assert rc == 0, c['id']
        for k in range(2):
            call.grad.fill_(float('nan'))
            call.out.fill_(float('nan'))
            ws.fill_(float('nan'))
            graph.replay()
            torch.cuda.synchronize()
            if c['entry'] == 'bwd':
                call.out.zero_()
            assert same(first, (call.out, call.grad)), (c['id'], 'replay', k)
        del graph


@pytest.mark.parametrize('dname,kind', GROUPS, ids=GROUP_IDS)
def test_a_minibatch_is_the_full_batch_of_its_gathered_rows(dname, kind):
    """mm_vec_pdist_loss_subset_det on (x, idx, dense) against mm_vec_pdist_loss_det on x[idx] with the targets
    dense[idx[a], idx[b]], a < b by position: loss and scale gradient the same bits, grad[idx] the same bits, every other row +0"""
    B = _B()
    cases = [c for c in _mine(C.minibatch_cases(), dname, kind) if not c.get('brows')]
    for c in cases:
        call = Call(c)
        sub = call.run(True)
        bs, m = c['batch'], c['m']
        idx = call.idx
        xg = call.x[idx].contiguous()
        a, b = torch.triu_indices(bs, bs, 1, device='cuda')
        target = call.side[idx[a], idx[b]].contiguous()
        grad = torch.full_like(xg, float('nan'))
        out = torch.full((2, ), float('nan'), dtype=call.dt, device='cuda')
        loss = vc.loss_of(c)
        ws = torch.full((B.lib().raw('mm_vec_pdist_det_ws_bytes')(call.dtc, call.kind, bs, m), ), 0xFF, dtype=torch.uint8, device='cuda')
        B.lib().call(DET['loss'], call.dtc, call.kind, vc.LOSS_CODE[loss['kind']], B.ptr(xg), B.ptr(target), B.ptr(call.scale), bs, m, 0, bs,
                     float(loss.get('alpha', 1.0)), 1.0 / (loss.get('epoch', 0) + 1), vc.terms_of(c), None, B.ptr(out), B.ptr(grad), B.ptr(ws),
                     B.stream_of(xg))
        torch.cuda.synchronize()
        assert torch.equal(sub[0], out), (c['id'], sub[0], out)
        assert torch.equal(sub[1][idx], grad), c['id']
        rest = torch.ones(vc.N_TABLE, dtype=torch.bool, device='cuda')
        rest[idx] = False
        assert plus_zero(sub[1][rest]), c['id']


# ---- 3. no environment switch selects or alters these kernels -----------------------------------------------------------------------------
def digest_cases():
    out = []
    for dname in C.DNAMES:
        for kind, m in (('lorentz', 11), ('lorentz', 24), ('sphere', 6), ('euclidean', 10)):
            for sq, loss in vc._variants('bwd'):
                out.append(vc.case('bwd', kind, m, dname, sq, loss) if m != 24 else None)
            out.append(vc.case('loss', kind, m, dname, True, 'stress') if m != 24 else None)
            if m in C.SUB_WIDTHS:
                out.append(vc.case('subset', kind, m, dname, True, 'stress', batch=70))
    return [C.BY_ID[c['id']] for c in out if c is not None]


def digests():
    out = {}
    for c in digest_cases():
        res = Call(c).run(True)
        out[c['id']] = hashlib.sha256(b''.join(t.cpu().numpy().tobytes() for t in res)).hexdigest()
    return out


_OWN = {}
_DIED = []      # a child that aborted, crashed or hung: no further child is started
CHILD_TIMEOUT = 90


@pytest.mark.parametrize('env', vc.ENVS[1:], ids=[vc.env_id(e) for e in vc.ENVS[1:]])
def test_no_environment_switch_changes_a_bit(env):
    """the digests of DIGEST_CASES in a fresh child under `env` against this process's"""
    if _DIED:
        pytest.fail(f'not started: an earlier child died ({_DIED[0]})')
    if not _OWN:
        _OWN.update(digests())
        assert len(_OWN) >= 20
    e = {k: v for k, v in os.environ.items() if k not in vc.ENV_KEYS}
    e.update(env)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--digests'], env=e, capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                           cwd=ROOT)
    except subprocess.TimeoutExpired:
        _DIED.append(f'{vc.env_id(env)}: no end within {CHILD_TIMEOUT} s')
        pytest.fail(_DIED[0])
    print(f'child {vc.env_id(env)}: {time.time() - t0:.1f} s, exit status {r.returncode}')
    if r.returncode in (134, 139, 124, 137) or r.returncode < 0:
        _DIED.append(f'{vc.env_id(env)}: exit status {r.returncode}')
        pytest.fail(_DIED[0] + '\n' + r.stdout[-3000:] + r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    theirs = json.loads(r.stdout.strip().splitlines()[-1])
    assert theirs == _OWN, [k for k in _OWN if theirs.get(k) != _OWN[k]]


# ---- 4. the routes -------------------------------------------------------------------------------------------------------------------------
def _manifold(kind, m, deterministic):
    from graphembed import manifolds as M
    return {'lorentz': M.Lorentz, 'sphere': M.Sphere, 'euclidean': M.Euclidean}[kind](m, deterministic=deterministic)


def _embedding(mans, n, dt, points):
    from graphembed.modules import ManifoldEmbedding
    torch.set_default_dtype(dt)
    try:
        with torch.device('cuda'):
            emb = ManifoldEmbedding(n, mans)
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for x, p in zip(emb.xs, points):
            x.copy_(_dev(p, dt))
        for s in emb.scales:
            s.fill_(vc.SCALE_RAW)
    return emb


def _dataset(kind, m, n, dname):
    """graph distances whose normalised squares are the case table's targets (up to the normalisation)"""
    from graphembed.data.dataset import GraphDataset
    t = vc._targets(kind, m, n, dname, None, 'stress', vc.EPOCH, float(np.float32(vc.SCALE_RAW)))[0]
    return GraphDataset(_dev(t, DT[dname]).sqrt())


def _calls(spy):
    return [name for name in spy.calls if 'pdist' in name or 'pairs_loss' in name or name == 'mm_product_loss']


def _one_step(emb, objective):
    for p in emb.parameters():
        p.grad = None
    with C.CallSpy() as spy:
        loss = objective()
        loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in emb.parameters())
    return _calls(spy), loss.detach().clone(), [p.grad.clone() for p in emb.parameters()]


@pytest.mark.parametrize('kind,m', [('lorentz', 11), ('sphere', 6), ('euclidean', 10), ('lorentz', 24)])
@pytest.mark.parametrize('how', ['keyword', 'torch switch'])
def test_routes(how, kind, m):
    """deterministic=True, or None under torch.use_deterministic_algorithms(True): pdist's backward, fused_objective on the full
    batch and BatchedObjective on a minibatch take the _det entries and none of the atomic ones, and give the same bits twice;
    deterministic=False under the switch, and the default without it, keep the atomic routes"""
    from graphembed.modules import BatchedObjective
    import grass_cases as gc
    n, dname, dt = 65, 'f32', torch.float32
    pts = [vc.points(kind, m, n, dname)]
    data = _dataset(kind, m, n, dname)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:17]      # host-side, distinct, unsorted
    g = _dev(vc._upstream(kind, m, n, dname, True)[0], dt)
    assert not torch.are_deterministic_algorithms_enabled()

    def routes(emb, loss_name):
        fn, kw = gc.objective(loss_name)
        man = emb.manifolds[0]
        out = {}
        xl = emb.xs[0].detach().clone().requires_grad_()
        with C.CallSpy() as spy:
            (man.pdist(xl, squared=True) * g).sum().backward()
        out['pdist'] = (_calls(spy), xl.grad.clone())
        out['fused'] = _one_step(emb, lambda: emb.fused_objective(fn, data[None], None, **kw))
        out['batched'] = _one_step(emb, lambda: BatchedObjective(fn, data, emb)(idx, **kw))
        return out

    try:
        if how == 'torch switch':
            torch.use_deterministic_algorithms(True)
        emb = _embedding([_manifold(kind, m, True if how == 'keyword' else None)], n, dt, pts)
        for loss_name in ('stress', 'quotient'):
            a, b = routes(emb, loss_name), routes(emb, loss_name)
            assert a['pdist'][0][-1] == DET['bwd'] and a['fused'][0] == [DET['loss']] and a['batched'][0] == [DET['subset']], a
            for what in a:
                assert not any(name in ATOMIC_ALL for name in a[what][0]), (what, a[what][0])
                assert b[what][0] == a[what][0]
                flat = lambda r: [t for part in r[1:] for t in (part if isinstance(part, list) else [part])]      # noqa: E731
                assert same(flat(a[what]), flat(b[what])), (loss_name, what)
            gx = a['batched'][2][0]
            rest = torch.ones(n, dtype=torch.bool, device='cuda')
            rest[idx.cuda()] = False
            assert plus_zero(gx[rest]) and float(gx[~rest].abs().max()) > 0
        off = _embedding([_manifold(kind, m, False)], n, dt, pts)      # deterministic=False: atomic whatever the switch says
        r = routes(off, 'stress')
        assert not any(name.endswith('_det') for what in r for name in r[what][0]), r
        assert any(name in ATOMIC_ALL for name in r['fused'][0]) and any(name in ATOMIC_ALL for name in r['batched'][0])
    finally:
        torch.use_deterministic_algorithms(False)
    plain = _embedding([_manifold(kind, m, None)], n, dt, pts)          # the default without the switch: as before
    r = routes(plain, 'stress')
    assert not any(name.endswith('_det') for what in r for name in r[what][0]), r


def test_a_product_with_a_deterministic_factor_takes_the_per_factor_kernels():
    import grass_cases as gc
    n, dname, dt = 65, 'f32', torch.float32
    fn, kw = gc.objective('stress')
    pts = [vc.points('lorentz', 11, n, dname), vc.points('sphere', 6, n, dname)]
    target = _dataset('lorentz', 11, n, dname)[None]
    emb = _embedding([_manifold('lorentz', 11, True), _manifold('sphere', 6, None)], n, dt, pts)
    calls, loss, grads = _one_step(emb, lambda: emb.fused_objective(fn, target, None, **kw))
    assert 'mm_product_loss' in calls and DET['bwd'] in calls, calls
    assert not any(name in ('mm_product_pairs_loss', ATOMIC['loss'], DET['loss']) for name in calls), calls
    again = _one_step(emb, lambda: emb.fused_objective(fn, target, None, **kw))
    assert torch.equal(grads[0], again[2][0])                       # the deterministic factor's gradient: the same bits
    plain = _embedding([_manifold('lorentz', 11, None), _manifold('sphere', 6, None)], n, dt, pts)
    calls = _one_step(plain, lambda: plain.fused_objective(fn, target, None, **kw))[0]
    assert calls == ['mm_product_pairs_loss'], calls


def test_a_batch_with_a_repeated_index_gathers_and_matches_the_oracle():
    """host-side indices with a repeat: take_rows and the deterministic FULL-batch kernel on the gathered rows; the result is the
    oracle's objective over the pairs of x[idx] (the repeated node twice, one pair of distance ~0)"""
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    from oracle import step as ostep
    kind, m, n, dname, dt = 'lorentz', 11, 65, 'f32', torch.float32
    x = vc.points(kind, m, n, dname)
    emb = _embedding([_manifold(kind, m, True)], n, dt, [x])
    data = _dataset(kind, m, n, dname)
    idx = torch.tensor([5, 40, 12, 5, 63, 0, 31])
    calls, loss, grads = _one_step(emb, lambda: BatchedObjective(StressLoss(), data, emb)(idx))
    assert calls == ['mm_pair_gather', DET['loss']] or calls == [DET['loss']], calls
    i, j = ostep.pair_list(n, idx.numpy())
    keep = i != j          # (the pair of the repeated node with itself: d2 = eps^2, its gradient vanishes; the oracle skips it)
    dense = data.pdists.double().cpu().numpy()
    value, gs, sg = ostep.objective([(kind, m)], [x], [float(np.float32(vc.SCALE_RAW))], {'kind': 'stress'}, target=dense[i, j][keep],
                                    pairs=(i[keep], j[keep]))
    value += float((dense[i, j][~keep] ** 2).sum())
    c = dict(vc.case('loss', kind, m, dname, True, 'stress', n=n), scale=True)
    errs = vc.errors(c, (value, gs[0], sg[0]), (float(loss), grads[0].double().cpu().numpy(), float(grads[1])))
    print(errs)
    assert all(e <= a for e, a in errs.values()), errs


def test_native_train_step_refuses_a_deterministic_vector_manifold():
    from graphembed.native_step import NativeTrainStep
    from graphembed.objectives import StressLoss
    from graphembed.optim import RiemannianSGD
    kind, m, n, dname, dt = 'lorentz', 11, 65, 'f32', torch.float32
    target = _dataset(kind, m, n, dname)[None]
    emb = _embedding([_manifold(kind, m, True)], n, dt, [vc.points(kind, m, n, dname)])
    opts = lambda e: [RiemannianSGD(list(e.xs), lr=1e-3, exact=True), RiemannianSGD(list(e.scales), lr=1e-4)]      # noqa: E731
    with pytest.raises(ValueError, match='deterministic'):
        NativeTrainStep(emb, StressLoss(), target, opts(emb))
    plain = _embedding([_manifold(kind, m, None)], n, dt, [vc.points(kind, m, n, dname)])
    step = NativeTrainStep(plain, StressLoss(), target, opts(plain))
    assert bool(torch.isfinite(step()))
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(ValueError, match='deterministic'):
            step()
    finally:
        torch.use_deterministic_algorithms(False)


# ---- 5. training ---------------------------------------------------------------------------------------------------------------------------
def _train(kind, m, opt, batch, graphed, steps=20, n=65):
    from graphembed.graphed import GraphedTrainStep
    from graphembed.modules import BatchedObjective
    from graphembed.objectives import StressLoss
    from graphembed.optim import RiemannianAdam, RiemannianSGD
    dname, dt = 'f32', torch.float32
    emb = _embedding([_manifold(kind, m, True)], n, dt, [vc.points(kind, m, n, dname)])
    data = _dataset(kind, m, n, dname)
    if opt == 'rsgd':
        opts = [RiemannianSGD(list(emb.xs), lr=2e-3, exact=True, max_grad_norm=20), RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)]
    else:
        opts = [RiemannianAdam(list(emb.xs), lr=2e-3, exact=True, max_grad_norm=20), RiemannianSGD(list(emb.scales), lr=1e-4, max_grad_norm=500)]
    fn = StressLoss()
    gen = torch.Generator().manual_seed(7)
    batches = [torch.randperm(n, generator=gen)[:batch] for _ in range(steps)] if batch else [None] * steps
    cur = torch.zeros(batch or 1, dtype=torch.int64, device='cuda')      # the step's node ids: a device buffer a captured step reads
    objective = BatchedObjective(fn, data, emb)
    queue = list(batches[:3]) if graphed and batch else []      # the batches of the warm-up steps GraphedTrainStep.capture runs itself

    def loss_fn():
        if queue and not torch.cuda.is_current_stream_capturing():
            cur.copy_(queue.pop(0))
        return objective(cur) if batch else emb.fused_objective(fn, data[None], None)

    losses = []
    if graphed:
        step = GraphedTrainStep(loss_fn, opts, warmup=3).capture()
        assert not queue
        losses = [v.clone() for v in step.warmup_losses]
        for b in batches[3:]:
            if batch:
                cur.copy_(b)
            losses.append(step().clone())
    else:
        for b in batches:
            if batch:
                cur.copy_(b)
            for o in opts:
                o.zero_grad(set_to_none=True)
            loss = loss_fn()
            loss.backward()
            for o in opts:
                o.step()
            losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    state = [v.detach().clone() for o in opts for p in o.param_groups[0]['params'] for k, v in sorted(o.state[p].items()) if torch.is_tensor(v)]
    return [emb.xs[0].detach().clone(), emb.scales[0].detach().clone(), torch.stack(losses)] + state


@pytest.mark.parametrize('batch', [None, 17], ids=['full', 'batch17'])
@pytest.mark.parametrize('opt', ['rsgd', 'radam'])
@pytest.mark.parametrize('kind,m', [('lorentz', 11), ('sphere', 6)])
def test_twenty_steps_end_in_the_same_bits(kind, m, opt, batch):
    """twenty steps of a 65-node embedding from one initialisation, twice eagerly and twice as a GraphedTrainStep replay: points,
    scale, every loss and the optimizer state torch.equal — between the repeats and between eager and replayed.  (The default
    atomic route may differ between two such runs; it is not asserted on.)"""
    runs = {(g, k): _train(kind, m, opt, batch, g) for g in (False, True) for k in (0, 1)}
    ref = runs[(False, 0)]
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    assert not torch.equal(ref[0], _dev(vc.points(kind, m, 65, 'f32'), torch.float32))
    if opt == 'radam':
        assert len(ref) > 3      # exp_avg, exp_avg_sq, step
    for key, run in runs.items():
        assert len(run) == len(ref)
        for k, (a, b) in enumerate(zip(ref, run)):
            assert torch.equal(a, b), (key, k, float((a.double() - b.double()).abs().max()))


# ---- last: the figures ---------------------------------------------------------------------------------------------------------------------
def test_print_worst_ratios():
    """(last in the file) per sweep, dtype and quantity the worst error / bound, e_det / allowance, e_det / S, e_atomic / S"""
    worst = {}
    for sweep, dname, q, r_bound, r_allow, r_det, r_atomic, cid in C.RECORDS:
        w = worst.setdefault((sweep, dname, q), [0.0, 0.0, 0.0, 0.0, 0])
        w[0], w[1], w[2], w[3], w[4] = max(w[0], r_bound), max(w[1], r_allow), max(w[2], r_det), max(w[3], r_atomic), w[4] + 1
    print('sweep | dtype | quantity | calls | error / bound | e_det / allowance | e_det / S | e_atomic / S')
    for (sweep, dname, q), (r_bound, r_allow, r_det, r_atomic, count) in sorted(worst.items()):
        print(f'{sweep} | {dname} | {q} | {count} | {r_bound:.3f} | {r_allow:.3f} | {r_det:.2e} | {r_atomic:.2e}')


if __name__ == '__main__':
    if sys.argv[1:] == ['--digests']:
        print(json.dumps(digests()))
