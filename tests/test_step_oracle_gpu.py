"""The training-step kernels (spd_fused_step_kernel, vec_fused_step_kernel, product_step_kernel, the unfused launches of
mm_train_step_run, the per-parameter and multi-parameter optimizer kernels) against an fp64 oracle, ONE STEP AT A TIME.

Teacher forcing: for each of K = 3 consecutive steps the device's parameters, scales and optimizer state are copied to the
host, oracle.step computes the step from exactly those values, the device step is issued, and everything the step wrote is
compared: loss, p.grad of points and scales, the displacement of every point and scale, momentum buffers, exp_avg,
exp_avg_sq, Adam's step counter.  Nothing accumulates between the two, so the tolerances are those of a single kernel
(step_cases.TOL; tests/test_oracle_step.py shows that a plain fp32 evaluation stays within a third of them on these inputs).
Steps 2 and 3 of a fused route read the tables / padded copy the previous step kernel wrote (MM_WS_PREPARED — asserted),
so a stale table shows as a wrong loss and gradient in the next comparison.

Every case asserts the route it names (entry points called, workspace flags, what the library says it fuses) and the regime
it names (share of points whose clip binds, median norm of the tangent step — from the oracle's per-point norms) before it
compares, and prints both (-rA)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}


# ------------------------------------------------------------------------------------------------------------ device side
def _manifolds(c):
    from graphembed import manifolds as M
    mk = {'spd': M.SymmetricPositiveDefinite, 'lorentz': M.Lorentz, 'sphere': M.Sphere, 'euclidean': M.Euclidean}
    return [mk[k](d) for k, d in c['factors']]


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device='cuda', dtype=dt)


def _optimizer(params, rule, dt):
    from graphembed.optim import RiemannianAdam, RiemannianSGD
    if rule['opt'] == 'radam':
        return RiemannianAdam(params, lr=1.0, betas=rule['betas'], nc=rule.get('nc', False), max_grad_norm=None,
                              exact=rule.get('exact', False))
    return RiemannianSGD(params, lr=1.0, momentum=rule.get('momentum', 0.0), dampening=rule.get('dampening', 0.0),
                         max_grad_norm=None, exact=rule.get('exact', False))


def _preload(opt, p, st, dt):
    for name, v in st.items():
        if name == 'step':
            opt.state[p]['step'] = torch.tensor(float(v), dtype=torch.float64, device='cuda')
        else:
            opt.state[p][name] = _dev(np.asarray(v, np.float64), dt).reshape(p.shape).contiguous()   # (0-dim for a scale)


def _host_state(opt, p):
    out = {}
    for name in ('momentum_buffer', 'exp_avg', 'exp_avg_sq', 'step'):
        if opt is not None and name in opt.state.get(p, {}):
            v = opt.state[p][name]
            out[name] = float(v) if name == 'step' else v.detach().double().cpu().numpy()
    return out


class Device:
    """The embedding, optimizers and stepper of a case on the GPU."""

    def __init__(self, c, state, data, comm=None):
        from graphembed.modules import ManifoldEmbedding
        from graphembed.objectives import QuotientLoss, StressLoss
        self.c, self.dt = c, DT[c['dname']]
        dt = self.dt
        torch.set_default_dtype(dt)
        try:
            with torch.device('cuda'):
                self.emb = emb = ManifoldEmbedding(c['n'], _manifolds(c))
        finally:
            torch.set_default_dtype(torch.float32)
        with torch.no_grad():
            for p, x in zip(emb.xs, state['xs']):
                p.copy_(_dev(x, dt))
            for p, s in zip(emb.scales, state['scales']):
                p.fill_(s)
        prule, srule = sc.POINT_RULES[c['rule']], sc.SCALE_RULES[c['scale_rule']]
        self.opt_p = _optimizer(list(emb.xs), prule, dt)
        self.opt_s = None
        if srule is None:
            emb.burnin(True)                                    # frozen scales: read by the objective, not stepped
            self.opt_s = _optimizer(list(emb.scales), dict(opt='rsgd'), dt)
        else:
            self.opt_s = _optimizer(list(emb.scales), srule, dt)
        for p, st in zip(emb.xs, state['point_states']):
            _preload(self.opt_p, p, st, dt)
        for p, st in zip(emb.scales, state['scale_states']):
            _preload(self.opt_s, p, st, dt)
        self.frozen = srule is None
        self.fn = StressLoss() if c['loss'] == 'stress' else QuotientLoss(inc_l1=c['loss'] != 'quotient_l2',
                                                                          inc_l2=c['loss'] != 'quotient_l1')
        self.target = _dev(data['target'], dt) if 'target' in data else None
        self.dense = _dev(data['dense'], dt) if 'dense' in data else None
        self.step = None
        if c['route'] != 'eager':
            from graphembed.native_step import NativeTrainStep
            kw = {}
            if c['route'] == 'sharded':
                from graphembed.parallel import PairShard
                kw = dict(shard=PairShard(c['n'], world=1, rank=0), comm=comm)
            self.step = NativeTrainStep(emb, self.fn, self.target, [self.opt_p, self.opt_s], dense=self.dense, **kw)

    def set_targets(self, data):
        """The targets as the oracle has them now (step_cases.settle_targets), written into the tensors the step reads."""
        if self.dense is not None:
            self.dense.copy_(_dev(data['dense'], self.dt))
        else:
            self.target.copy_(_dev(data['target'], self.dt))
            if self.step is not None and self.step.target.data_ptr() != self.target.data_ptr():
                self.step.target.copy_(self.step.shard.slice(self.target) if self.step.shard is not None else self.target)

    def read(self):
        """Host copy of everything a step reads."""
        emb = self.emb
        torch.cuda.synchronize()
        return dict(xs=[p.detach().double().cpu().numpy() for p in emb.xs], scales=[float(p) for p in emb.scales],
                    point_states=[_host_state(self.opt_p, p) for p in emb.xs],
                    scale_states=[{} if self.frozen else _host_state(self.opt_s, p) for p in emb.scales])

    def run(self, k, prule, srule, idx):
        """Issue step k with the oracle's hyper-parameters; returns (what the step wrote, entry points called, ws flags)."""
        from graphembed import _backend as B
        for g in self.opt_p.param_groups:
            g['lr'], g['max_grad_norm'] = prule['lr'], prule['max_grad_norm']
        if srule is not None:
            for g in self.opt_s.param_groups:
                g['lr'], g['max_grad_norm'] = srule['lr'], srule['max_grad_norm']
        kw = {} if self.c['loss'] == 'stress' else dict(epoch=sc.loss_of(self.c, k)['epoch'], alpha=sc.loss_of(self.c, k)['alpha'])
        lib, calls, flags = B.lib(), [], []
        orig = lib.call

        def spy(name, *a):
            calls.append(name)
            if name == 'mm_train_step_run':
                flags.append(self.step._desc.ws_flags)
            return orig(name, *a)
        lib.call = spy
        try:
            if self.step is not None:
                if idx is None:
                    loss = self.step(**kw)
                else:
                    loss = self.step(indices=torch.from_numpy(idx).cuda(), **kw)
            else:
                loss = self.emb.fused_objective(self.fn, self.target, None, **kw)
                assert loss is not None
                for o in (self.opt_p, self.opt_s):
                    o.zero_grad(set_to_none=True)
                loss.backward()
                self.opt_p.step()
                if not self.frozen:
                    self.opt_s.step()
        finally:
            del lib.call
        torch.cuda.synchronize()
        emb = self.emb
        after = self.read()
        got = dict(loss=float(loss), grads=[p.grad.detach().double().cpu().numpy() for p in emb.xs],
                   scale_grads=[float(p.grad) if p.grad is not None else float('nan') for p in emb.scales],
                   new_xs=after['xs'], new_scales=after['scales'], point_states=after['point_states'],
                   scale_states=after['scale_states'])
        return got, calls, flags


# ------------------------------------------------------------------------------------------------------------------ routes
def _expected_eager_calls(c):
    """Entry points of the eager optimizers: one fused launch per parameter, or ONE per group for the vector-space parameters
    of a momentum-free RSGD / an Adam group (mm_vec_*_step_multi)."""
    prule, srule = sc.POINT_RULES[c['rule']], sc.SCALE_RULES[c['scale_rule']]

    def name(fam, rule):
        stem = 'mm_spd_' if fam == 'spd' else 'mm_vec_'
        if rule['opt'] == 'radam':
            return stem + 'radam_step'
        return stem + ('rsgd_momentum_step' if rule.get('momentum', 0) else 'rsgd_step')
    want = []
    for rule, fams in ((prule, [f[0] for f in c['factors']]), (srule, ['euclidean'] * len(c['factors']))):
        if rule is None:
            continue
        vec = [f for f in fams if f != 'spd']
        grouped = len(fams) >= 2 and len(vec) >= 2 and not rule.get('momentum', 0)
        want += [name('euclidean', rule) + '_multi'] if grouped else [name(f, rule) for f in vec]
        want += [name('spd', rule) for f in fams if f == 'spd']
    return sorted(want)


def assert_route(c, dev, k, calls, flags, idx):
    """The case took the route it names (a case that silently falls to another route fails); returns its description."""
    from graphembed import _backend as B
    single = len(c['factors']) == 1
    kind, dim = c['factors'][0]
    dtc = B.MM_F32 if c['dname'] == 'f32' else B.MM_F64
    if c['route'] == 'eager':
        steps = sorted(n for n in calls if '_step' in n and 'train_step' not in n)
        assert steps == _expected_eager_calls(c), (steps, _expected_eager_calls(c))
        assert not any(n.endswith('_map') or n.endswith('_norm') or n.endswith('_exp') or n.endswith('_retr') for n in calls), calls
        generic = bool(c['env'].get('MM_VEC_RULE_GENERIC')) or any(f != 'spd' and d > 16 for f, d in c['factors'])
        if c['env']:
            assert all(os.environ.get(e) == v for e, v in c['env'].items()), 'the switch is set in this process'
        return f"eager optimizers: {', '.join(steps)}; vector rule {'generic (run-time m)' if generic else 'register-resident (m <= 16)'}"
    # one call into the library and nothing else: no separate optimizer or objective launches from Python
    assert calls == ['mm_train_step_run'], calls
    if single and kind == 'spd':
        fusable = dim <= B.lib().raw('mm_spd_fused_step_max_dim')()
    elif single:
        fusable = bool(B.lib().raw('mm_vec_fused_step_supports')(dtc, {'euclidean': B.EUCLIDEAN, 'lorentz': B.LORENTZ,
                                                                       'sphere': B.SPHERE}[kind], dim))
    else:
        fusable = True
    if c['env']:
        assert all(os.environ.get(e) == v for e, v in c['env'].items()), 'the switch is set in this process'
    if c['route'] == 'sharded':
        d = dev.step._desc
        assert d.comm and d.reduce_buf and d.reduce_count == dev.step.flat.numel() and d.row_begin == 0 and d.row_end >= c['n'] - 1
        return f'one-call step sharded over a one-rank communicator (all-reduce of {d.reduce_count} values, ws_flags {flags[0]})'
    if c['route'] == 'unfused':
        assert not fusable and not dev.step._prepared_single and flags == [0], (fusable, flags)
        return f'one-call step, unfused launches (ws_flags {flags[0]})' + (f' under {c["env"]}' if c['env'] else '')
    assert fusable, 'the library does not fuse this step'
    if c['route'] == 'minibatch':
        assert dev.step._desc.batch == idx.size and dev.step._desc.batch_idx
        if kind == 'spd':      # (a vector factor's minibatch step does not rewrite the padded copy: prepared again every step)
            assert flags == [B.MM_WS_PREPARED if k else 0], (k, flags)
        else:
            assert flags == [0], (k, flags)
        return f'one-call minibatch step over {idx.size} of {c["n"]} nodes (ws_flags {flags[0]})'
    if single:
        assert dev.step._prepared_single
        assert flags == [B.MM_WS_PREPARED if k else 0], (k, flags)
    else:
        assert flags[0] & B.MM_WS_PREPARED == (B.MM_WS_PREPARED if k else 0), (k, flags)
    return f"fused one-call step (ws_flags {flags[0]}: MM_WS_PREPARED {'set' if flags[0] & B.MM_WS_PREPARED else 'clear'})"


# ----------------------------------------------------------------------------------------- the device's output on its own
def _lorentz_offset(x):
    """|<x, x>_L + 1| / x0^2 per point, evaluated in fp64."""
    x = torch.as_tensor(x, dtype=torch.float64)
    return ((-(x[:, 0]**2) + (x[:, 1:]**2).sum(-1) + 1).abs() / x[:, 0]**2).max().item()


def _sphere_offset(x):
    """| |x| - 1 | per point, evaluated in fp64."""
    return (torch.as_tensor(x, dtype=torch.float64).norm(dim=-1) - 1).abs().max().item()


def assert_invariants(c, dev, state, want, got, prule):
    from oracle import ref_port as rp
    from oracle import step as ostep
    eps = sc.ULP[c['dname']]
    for i, ((kind, dim), x, st) in enumerate(zip(c['factors'], dev.emb.xs, got['point_states'])):
        xd = x.detach()
        if kind == 'spd':
            assert torch.equal(xd, xd.transpose(-2, -1)), 'SPD points exactly symmetric'
            torch.linalg.cholesky(xd.double().cpu())           # raises if a point left the cone
            for name in ('momentum_buffer', 'exp_avg'):
                if name in st:
                    assert np.array_equal(st[name], np.swapaxes(st[name], -1, -2)), f'{name} exactly symmetric'
        elif kind in ('lorentz', 'sphere'):
            # The bound is the reference's own: its exp / retr (lorentz.py:44-62, sphere.py:46-59) evaluated in the case's
            # dtype from the same point, gradient and state leaves the manifold by the rounding of cosh^2 - sinh^2 (cos^2 +
            # sin^2) plus what the stored point and the tangent were off already — neither exp re-projects, so a few ulp per
            # step add up over the three steps, in the reference as on the device.  The device may be off by at most three
            # times that (the rule of check_grad in tests/test_spd_gpu.py), plus 4 ulp for the rounding of the stored result.
            dt = DT[c['dname']]
            x0 = torch.as_tensor(state['xs'][i], dtype=dt)
            ref, _, _ = ostep.apply_rule(rp.make(kind, dim), x0, torch.as_tensor(want['grads'][i], dtype=dt), prule,
                                         ostep._state_in(state['point_states'][i], x0.shape, dt))
            offset = _lorentz_offset if kind == 'lorentz' else _sphere_offset
            off, ref_off = offset(xd.cpu()), offset(ref)
            what = '<x, x>_L + 1 (in ulp x0^2)' if kind == 'lorentz' else '|x| - 1 (in ulp)'
            print(f'          {what}: device {off / eps:.1f}, the reference formula in {c["dname"]} {ref_off / eps:.1f}')
            assert off <= 3 * ref_off + 4 * eps, f'{what}: {off / eps:.1f}, the reference formula gives {ref_off / eps:.1f}'
    for g in got['grads']:
        assert np.isfinite(g).all()


def assert_workspace_is_a_fresh_preparation(c, dev):
    """After a fused step the workspace holds what a preparation computes from the NEW points (the assertion of
    test_tables_written_by_the_step_equal_a_fresh_preparation; the vector factor's padded copy as in
    test_fused_vector_step_matches_the_eager_loop)."""
    from graphembed import _backend as B
    step, x, n, dt = dev.step, dev.emb.xs[0], c['n'], dev.dt
    kind, d = c['factors'][0]
    if kind == 'spd':
        fresh = torch.zeros_like(step.ws)
        B.lib().call('mm_spd_prepare', B.dtype_code(x), B.ptr(x), n, d, B.ptr(fresh), B.stream_of(x))
        torch.cuda.synchronize()
        head = 64 + (n * 4 + 63) // 64 * 64
        assert torch.equal(step.ws[:head], fresh[:head])
        esz = x.element_size()
        end = head + (step.ws.numel() - 2048 * 32 - 31 - head) // esz * esz
        a, b = step.ws[head:end].view(dt), fresh[head:end].view(dt)
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6 if dt == torch.float32 else 1e-14, atol=0)
    else:
        pad = next(p for p in (4, 8, 12, 16, 24, 32, 48, 64) if p >= d)
        ws = step.ws.view(dt)
        acc, slots = n * (pad + 1), 2 * 256
        assert not ws[:acc + slots].any()
        xpad = ws[acc + slots:acc + slots + (n + 1) * pad].view(n + 1, pad)
        assert torch.equal(xpad[:n, :d], x.detach().view(n, d)) and not xpad[:, d:].any() and not xpad[n].any()


# ------------------------------------------------------------------------------------------------------------------- a case
def run_case(c, comm=None):
    """K teacher-forced steps; returns {quantity: worst error / allowed}.  Prints route and regime of every step."""
    state, data = sc.initial(c)
    dev = Device(c, state, data, comm)
    worst = {}
    for k in range(sc.K):
        state = dev.read()                                   # 1. what the device holds
        prule, srule, want, regime = sc.oracle_step(c, state, data, k)     # 2. the oracle's step from exactly those values
        if regime['targets_moved']:
            dev.set_targets(data)
        idx = sc.batch_of(c, data, k)
        got, calls, flags = dev.run(k, prule, srule, idx)    # 3. the device's step
        route = assert_route(c, dev, k, calls, flags, idx)
        print(f'[step {k + 1}] {c["id"]}: {route}; {sc.describe(regime)}')
        errs = sc.errors(c, state, want, got)                # 4. everything the step wrote
        ratios = sc.worst(errs)
        print('          ' + ', '.join(f'{q} {e:.2e}/{a:.2e}' for q, (e, a) in sorted(errs.items())))
        for q, r in ratios.items():
            worst[q] = max(worst.get(q, 0.0), r)
        bad = {q: errs[q] for q, r in ratios.items() if not r <= 1.0}
        assert not bad, f'step {k + 1}: (error, allowed) {bad}'
        if idx is not None:                                  # rows of p.grad outside the batch: exactly zero
            rest = np.ones(c['n'], dtype=bool)
            rest[idx] = False
            assert not got['grads'][0][rest].any()
        assert_invariants(c, dev, state, want, got, prule)
        if c['route'] == 'fused' and len(c['factors']) == 1 and c['n'] in (65, 129):
            assert_workspace_is_a_fresh_preparation(c, dev)
    print(f'[worst] {c["id"]}: ' + ', '.join(f'{q} {r:.4f}' for q, r in sorted(worst.items())))
    return worst


IN_PROCESS = [c for c in sc.CASES if not c['env'] and c['route'] != 'sharded']
CHILD = [c for c in sc.CASES if c['env']]
SHARDED = [c for c in sc.CASES if c['route'] == 'sharded']


@pytest.mark.parametrize('c', IN_PROCESS, ids=sc.ids(IN_PROCESS))
def test_step_against_the_oracle(c):
    run_case(c)


@pytest.mark.parametrize('c', CHILD, ids=sc.ids(CHILD))
def test_step_against_the_oracle_under_a_switch(c):
    """The routes only an environment switch reaches (read once per process by the library): the case runs in a child."""
    from graphembed import _backend as B
    if 'MM_VEC_STEP_UNFUSED' in c['env']:
        kind, dim = c['factors'][0]
        assert B.lib().raw('mm_vec_fused_step_supports')(B.MM_F32 if c['dname'] == 'f32' else B.MM_F64,
                                                         {'euclidean': B.EUCLIDEAN, 'lorentz': B.LORENTZ, 'sphere': B.SPHERE}[kind],
                                                         dim), 'fused without the switch'
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), c['id']],
                       env=dict(os.environ, **c['env']), capture_output=True, text=True, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.fixture(scope='module')
def comm():
    from graphembed.comm import Communicator, available
    assert available(), 'librccl could not be bound'
    c = Communicator(0, 1, Communicator.unique_id(), torch.device('cuda', 0))
    yield c
    c.destroy()


@pytest.mark.parametrize('c', SHARDED, ids=sc.ids(SHARDED))
def test_sharded_step_against_the_oracle(c, comm):
    """mm_train_step_run with a communicator: objective, ONE all-reduce of {gradients, loss, scale gradients}, then the step
    kernels on the reduced p.grad (no accumulators to finish)."""
    run_case(c, comm)


if __name__ == '__main__':
    run_case(sc.BY_ID[sys.argv[1]])
