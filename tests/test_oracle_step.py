"""Pins oracle.step (one training step in fp64: oracle/exact.c distances, numpy losses, the port's optimizer maps with LAPACK
factorisations) — the checker of tests/test_step_oracle_gpu.py.  CPU only.

* against the recorded reference: the 20-epoch tree40 traces (losses, x20, scales), the three-step RiemannianAdam traces
  (points, exp_avg, exp_avg_sq) and the two-step RSGD traces of the per-manifold goldens;
* against oracle.ref_port in fp64 on seeded inputs: they differ by the bias of the reference's 2x2 / 3x3 closed forms only;
* the condition that keeps the GPU tolerances honest: on the inputs of the GPU cases, the port's plain fp32 evaluation of the
  step stays within ONE THIRD of the tolerance the GPU test applies."""
import itertools

import numpy as np
import pytest
import torch

import step_cases as sc
from conftest import load_golden
from oracle import step as ostep

# The reference's eps-fudged closed forms (SPD(2): Cholesky + eigenvalues, SPD(3): eigenvalues) bias its fp64 results by
# 1e-8 ... 1e-6: the tolerance at which test_oracle_golden.py / test_oracle_exact.py hold oracle/exact.c to
# recordings of those sizes.  Everything else agrees to fp64 rounding.
BIAS = 5e-6
ROUNDING = 1e-9


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def tol_of(factors):
    return BIAS if any(k == 'spd' and d <= 3 for k, d in factors) else ROUNDING


# ------------------------------------------------------------------------------------------------- the recorded reference
TREE40 = {'euclidean10': [('euclidean', 10)], 'lorentz11': [('lorentz', 11)], 'spd3': [('spd', 3)],
          'product': [('lorentz', 6), ('sphere', 6), ('spd', 2)]}


@pytest.mark.parametrize('case', list(TREE40))
@pytest.mark.parametrize('loss_name', ['stress', 'quotient'])
def test_tree40_training_trace(case, loss_name):
    """20 free-running full-batch epochs on tree40 with the reference's production RSGD settings, every factor layout recorded:
    the tolerances of test_tree40_training_trace_fused (losses 2e-5, x20 2e-4, scales 1e-6)."""
    G = load_golden('callers')
    factors = TREE40[case]
    base = f'tree40/{case}/{loss_name}'
    state = dict(xs=[np.array(G[f'{base}/x0_{k}'], np.float64) for k in range(len(factors))], scales=[0.5] * len(factors))
    prule = dict(opt='rsgd', lr=0.01, exact=True, max_grad_norm=20)
    srule = dict(opt='rsgd', lr=1e-4, max_grad_norm=500)
    losses = []
    for epoch in range(20):
        loss = {'kind': 'stress'} if loss_name == 'stress' else {'kind': 'quotient', 'epoch': epoch, 'alpha': 1.0}
        out = ostep.train_step(factors, state['xs'], state['scales'], loss, prule, srule, target=G['tree40/target'])
        losses.append(out['loss'])
        state = dict(xs=out['new_xs'], scales=out['new_scales'])
    assert rel(losses, G[f'{base}/losses']) <= 2e-5
    for k in range(len(factors)):
        assert rel(state['xs'][k], G[f'{base}/x20_{k}']) <= 2e-4
    assert np.abs(np.array(state['scales']) - G[f'{base}/scales20']).max() <= 1e-6


RADAM = {'spd2': ('spd', 2), 'spd3': ('spd', 3), 'spd4': ('spd', 4), 'lorentz11': ('lorentz', 11), 'lorentz6': ('lorentz', 6),
         'sphere6': ('sphere', 6), 'euclidean10': ('euclidean', 10)}


@pytest.mark.parametrize('key', list(RADAM))
def test_radam_three_step_traces(key):
    G = load_golden('radam')
    factor = RADAM[key]
    man = ostep.manifold(factor)
    tol = tol_of([factor])
    base = f'{key}/f64'
    seen = 0
    for exact, clip, nc in itertools.product([0, 1], [0, 1], [0, 1]):
        tag = f'{base}/exact{exact}_clip{clip}_nc{nc}'
        rule = dict(opt='radam', lr=0.05, betas=(0.9, 0.99), nc=bool(nc), max_grad_norm=2.0 if clip else None, exact=bool(exact))
        x, state = torch.from_numpy(np.array(G[f'{base}/x0'])), {}
        for k in range(3):
            x, state, diag = ostep.apply_rule(man, x, torch.from_numpy(np.array(G[f'{base}/g{k}'])), rule, state)
            assert rel(x.numpy(), G[f'{tag}/x{k + 1}']) <= tol, f'{tag}/x{k + 1}'
            if clip:
                assert ((diag['rgrad_norm'] > 2.0) == diag['binds']).all()
        assert state['step'] == 4
        assert rel(state['exp_avg'].numpy(), G[f'{tag}/exp_avg']) <= tol * 10, tag      # (x10: as tests/test_radam.py)
        assert rel(state['exp_avg_sq'].numpy(), G[f'{tag}/exp_avg_sq']) <= tol * 10, tag
        seen += 1
    assert seen == 8


RSGD_KEYS = {'spd2': ('spd', 2), 'spd3': ('spd', 3), 'spd4': ('spd', 4), 'spd5': ('spd', 5), 'spd6': ('spd', 6),
             'lorentz3': ('lorentz', 3), 'lorentz11': ('lorentz', 11), 'lorentz48': ('lorentz', 48), 'sphere6': ('sphere', 6),
             'sphere64': ('sphere', 64), 'euclidean10': ('euclidean', 10), 'euclidean40': ('euclidean', 40)}


@pytest.mark.parametrize('key', list(RSGD_KEYS))
def test_rsgd_two_step_traces(key):
    G = load_golden(key)
    factor = RSGD_KEYS[key]
    man = ostep.manifold(factor)
    tol = tol_of([factor])
    base = 'f64/rsgd'
    x0, g1, g2 = (torch.from_numpy(np.array(G[f'{base}/{q}'])) for q in ('x0', 'g1', 'g2'))
    seen = 0
    for exact, clip, mom in itertools.product([0, 1], [0, 1], [0, 1]):
        tag = f'{base}/exact{exact}_clip{clip}_mom{mom}'
        if f'{tag}/x1' not in G:
            continue
        rule = dict(opt='rsgd', lr=0.05, momentum=0.9 if mom else 0.0, dampening=0.1 if mom else 0.0,
                    max_grad_norm=2.0 if clip else None, exact=bool(exact))
        x1, st, _ = ostep.apply_rule(man, x0, g1, rule, {})
        assert rel(x1.numpy(), G[f'{tag}/x1']) <= tol, tag
        x2, st, _ = ostep.apply_rule(man, x1, g2, rule, st)
        assert rel(x2.numpy(), G[f'{tag}/x2']) <= tol, tag
        if mom:
            assert rel(st['momentum_buffer'].numpy(), G[f'{tag}/buf2']) <= tol, tag
        seen += 1
    assert seen == 8


# ------------------------------------------------------------------------------------------------------- against the port
SMALL = [c for c in sc.CASES if c['n'] <= 300]
# one larger case per family (the whole pair list through autograd on the CPU: seconds)
LARGER = [sc.case('cpu-spd3-n700', 'fused', [('spd', 3)], 700, 'f32', 'rsgd', 'rsgd', 'median'),
          sc.case('cpu-spd4-n700', 'fused', [('spd', 4)], 700, 'f32', 'rsgd', 'rsgd', 'median', loss='quotient'),
          sc.case('cpu-lorentz11-n1000', 'fused', [('lorentz', 11)], 1000, 'f32', 'rsgd', 'rsgd', 'median'),
          sc.case('cpu-sphere6-n1000', 'fused', [('sphere', 6)], 1000, 'f32', 'rsgd_retr', 'rsgd', 'median'),
          sc.case('cpu-euclidean10-n1000', 'fused', [('euclidean', 10)], 1000, 'f32', 'adam', 'rsgd', 'median'),
          sc.case('cpu-csphd-n1025', 'fused', sc.CSPHD, 1025, 'f32', 'rsgd', 'rsgd', 'median')]


def run_port(c, dtype):
    """K steps of the case: oracle and port from the same state; the next state is what the PORT wrote (as the device's will
    be).  Yields (k, state, want, got, regime)."""
    state, data = sc.initial(c)
    for k in range(sc.K):
        prule, srule, want, regime = sc.oracle_step(c, state, data, k)
        got = ostep.port_step(c['factors'], state['xs'], state['scales'], sc.loss_of(c, k), prule, srule,
                              target=data.get('target'), dense=data.get('dense'), idx=sc.batch_of(c, data, k),
                              point_states=state['point_states'], scale_states=state['scale_states'], dtype=dtype)
        yield k, state, want, got, regime
        state = sc.next_state(c, got)


@pytest.mark.parametrize('c', [c for c in SMALL if c['dname'] == 'f64'], ids=sc.ids([c for c in SMALL if c['dname'] == 'f64']))
def test_oracle_against_the_port_in_fp64(c):
    """Same step, two restatements (exact.c + numpy losses against autograd through the port): rounding, except for the
    documented bias of the port's 2x2 / 3x3 closed forms."""
    tol = tol_of(c['factors'])
    for k, state, want, got, regime in run_port(c, torch.float64):
        assert abs(got['loss'] - want['loss']) <= tol * abs(want['loss'])
        for i in range(len(c['factors'])):
            assert rel(got['grads'][i], want['grads'][i]) <= tol * 10, (k, i)
            assert rel(got['new_xs'][i], want['new_xs'][i]) <= tol * 10, (k, i)
            assert abs(got['scale_grads'][i] - want['scale_grads'][i]) <= tol * 10 * max(abs(want['scale_grads'][i]), 1e-3 * abs(want['loss']))
            assert abs(got['new_scales'][i] - want['new_scales'][i]) <= tol * 10
            for name in ('momentum_buffer', 'exp_avg', 'exp_avg_sq'):
                if name in want['point_states'][i]:
                    assert rel(got['point_states'][i][name], want['point_states'][i][name]) <= tol * 10, (k, i, name)


F32 = [c for c in SMALL if c['dname'] == 'f32'] + LARGER


@pytest.mark.parametrize('c', F32, ids=sc.ids(F32))
def test_fp32_port_stays_within_a_third_of_the_gpu_tolerances(c, request):
    """The condition that keeps the GPU tolerances honest: a plain fp32 evaluation of the step (the port) on the GPU cases'
    inputs errs by at most a third of what the GPU test allows.  A family that misses it gets other inputs, not another
    tolerance."""
    worst = {}
    for k, state, want, got, regime in run_port(c, torch.float32):
        for q, r in sc.worst(sc.errors(c, state, want, got)).items():
            worst[q] = max(worst.get(q, 0.0), r)
    print(f'[port fp32] {c["id"]}: ' + ', '.join(f'{q} {r:.3f}' for q, r in sorted(worst.items())))
    bad = {q: r for q, r in worst.items() if r > 1.0 / 3}
    assert not bad, bad
