"""The fused Riemannian Adam step on the kappa-stereographic manifold (mm_stereo_radam_step, csrc/stereo.hip;
Stereographic.radam_step): one step at a time against the long-double oracle of tests/stereo_radam_cases.py, whole traces
through RiemannianAdam against the recorded reference (optim/radam.py on Universal), the call log of a product step and a
captured minibatch step (objective through an index buffer, optimizer, stabilize) against eager steps.

Tolerance rule of the single steps (stereo_cases.bound): fp64 <= 1e-11 of the scale (max |x|, max |exp_avg|, max exp_avg_sq);
fp32 <= twice the recorded reference-fp32 trace's own deviation from the oracle's trace at that step and quantity, never asked
below 16 * 2^-24 of the scale."""
import numpy as np
import pytest
import torch

import stereo_cases as S
import stereo_product_cases as P
import stereo_radam_cases as A
from grass_cases import CallSpy
from graphembed import _backend as B
from test_stereo_gpu import DT, NP, check, cuda, dev

pytestmark = pytest.mark.gpu

CASE_IDS = [A.case_id(c) for c in A.CASES]
SETTING_IDS = [A.setting_id(s) for s in A.SETTINGS]


def abi_step(x, eg, m1, v, t, c_raw, mode, setting, inplace=False):
    """one mm_stereo_radam_step from the given state; returns (x_new, exp_avg, exp_avg_sq, step) - the moments are updated in place"""
    exact, clip, nc = setting
    n, m = x.shape
    step = torch.tensor(float(t), dtype=torch.float64, device=x.device)
    ticket = torch.zeros(1, dtype=torch.int32, device=x.device)
    out = x if inplace else torch.full_like(x, float('nan'))
    B.lib().call('mm_stereo_radam_step', B.dtype_code(x), B.ptr(x), B.ptr(eg), B.ptr(m1), B.ptr(v), B.ptr(step), B.ptr(ticket), n, m,
                 B.ptr(c_raw), mode, S.C_MIN, A.LR, A.BETAS[0], A.BETAS[1], int(nc), A.EPS, -1.0 if clip is None else float(clip),
                 int(exact), B.ptr(out), B.stream_of(x))
    assert int(ticket) == 0, 'the ticket is re-armed'
    return out, m1, v, float(step)


@pytest.mark.parametrize('setting', A.SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize('case', A.CASES, ids=CASE_IDS)
def test_one_step_at_a_time_against_the_oracle(case, setting):
    """Each of the three steps starts from the ORACLE's state (point, both moments, step counter) rounded to the dtype; the rows
    ZERO_ROWS of steps two and three have a zero gradient and non-zero moments."""
    R = S.recorded()
    x0, c_raw, gs = A.make_inputs(case)
    mode = A.mode_of(case)
    assert not gs[1][list(A.ZERO_ROWS)].any() and gs[0][list(A.ZERO_ROWS)].all()
    failures = []
    for dname in ('f64', 'f32'):
        want_trace = A.trace(case, setting, dname)
        for k in range(3):
            x, m1, v, t = want_trace[k]
            xr, mr, vr = (np.asarray(a).astype(NP[dname]) for a in (x, m1, np.broadcast_to(v, x.shape)))
            if k:
                assert np.abs(mr[list(A.ZERO_ROWS)]).min() > 0, 'the zero-gradient rows carry non-zero moments'
            want = A.step(xr, gs[k], mr, vr[:, :1], t, c_raw, mode, dname, setting)
            for inplace in (False, True):
                got = abi_step(cuda(xr, dname), cuda(gs[k], dname), cuda(mr, dname), cuda(vr, dname), t, cuda(np.array([c_raw]), dname),
                               mode, setting, inplace)
                if inplace:   # x_new may equal x: the same numbers
                    assert all(torch.equal(a, b) for a, b in zip(got[:3], first[:3])), 'the in-place call differs'
                    continue
                first = got
                ref = (lambda what: R.get(A.key(case, setting, f'{what}{k + 1}', 'f32'))) if dname == 'f32' else (lambda what: None)
                tag = f'{A.case_id(case)} {A.setting_id(setting)} step {k + 1}'
                assert got[3] == t + 1, (tag, got[3])
                check(failures, f'{tag} x', dname, got[0].cpu().numpy(), want[0], np.abs(want[0]).max(),
                      None if ref('x') is None else _shifted(ref('x'), want_trace[k + 1][0], want[0]))
                check(failures, f'{tag} exp_avg', dname, got[1].cpu().numpy(), want[1], np.abs(want[1]).max(),
                      None if ref('exp_avg') is None else _shifted(ref('exp_avg'), want_trace[k + 1][1], want[1]))
                vg = got[2].cpu().numpy()
                assert np.array_equal(vg, np.broadcast_to(vg[:, :1], vg.shape)), 'one scalar per point, stored over its m entries'
                check(failures, f'{tag} exp_avg_sq', dname, vg[:, 0], want[2][:, 0], np.abs(want[2]).max(),
                      None if ref('exp_avg_sq') is None else _shifted(ref('exp_avg_sq'), want_trace[k + 1][2][:, 0], want[2][:, 0]))
    assert not failures, '\n'.join(failures)


def _shifted(ref32, trace_value, want):
    """the reference-fp32 trace's deviation from the oracle's trace, carried over to `want` (`check` measures ref32 against want)"""
    return np.asarray(want, dtype=S.LD) + (np.asarray(ref32, dtype=S.LD) - np.asarray(trace_value, dtype=S.LD))


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('case', A.CASES, ids=CASE_IDS)
def test_whole_traces_through_the_optimizer_follow_the_reference(case, dname):
    """Three steps of RiemannianAdam on a ManifoldParameter against the recorded trace at the tolerances of tests/test_radam.py:
    2e-4 (fp32) / 1e-7 (fp64) of the largest entry, ten times that for the moments; state['step'] == 4."""
    from graphembed.manifolds import Stereographic
    from graphembed.modules import ManifoldParameter
    from graphembed.optim import RiemannianAdam
    R = S.recorded()
    tol = 2e-4 if dname == 'f32' else 1e-7
    m, c_init, fixed = case
    x0, c_raw, gs = A.make_inputs(case)
    for setting in A.SETTINGS:
        exact, clip, nc = setting
        if A.key(case, setting, 'x1', dname) not in R:   # (a reference fp32 trace that was not finite is not recorded)
            assert dname == 'f32'
            continue
        man = Stereographic(m, c_init=c_init, c_min=S.C_MIN, keep_sign_fixed=fixed).to(device=dev(), dtype=DT[dname])
        p = ManifoldParameter(cuda(x0, dname), manifold=man)
        opt = RiemannianAdam([p], lr=A.LR, betas=A.BETAS, nc=nc, max_grad_norm=clip, exact=exact)
        with CallSpy() as spy:
            for k in range(3):
                p.grad = cuda(gs[k], dname)
                opt.step()
                ref = R[A.key(case, setting, f'x{k + 1}', dname)]
                err = np.abs(p.data.double().cpu().numpy() - ref).max() / np.abs(ref).max()
                assert err <= tol, (A.setting_id(setting), k + 1, err)
        assert spy.calls == ['mm_stereo_radam_step'] * 3, spy.calls
        assert float(opt.state[p]['step']) == 4.0
        ref = R[A.key(case, setting, 'exp_avg_sq3', dname)]
        got = opt.state[p]['exp_avg_sq'].double().cpu().numpy()
        assert np.abs(got[:, 0] - ref).max() / max(np.abs(ref).max(), 1e-30) <= 10 * tol, A.setting_id(setting)
        ref = R[A.key(case, setting, 'exp_avg3', dname)]
        err = np.abs(opt.state[p]['exp_avg'].double().cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-30)
        assert err <= 10 * tol, (A.setting_id(setting), err)


# ---- a product step ---------------------------------------------------------------------------------------------------------------
ROUTE_CASE = P.CASES[3]   # n = 65, ds = [5, 5], c = (0.01, -0.3)
BATCHES = [np.random.RandomState(21 + k).permutation(65)[:23] for k in range(3)]


class Dense:
    """GraphDataset's protocol: `pdists` is the dense target matrix on the GPU"""

    def __init__(self, dname):
        full = torch.from_numpy(P.pairs_of(ROUTE_CASE)[1].astype(NP[dname]))
        dense = torch.zeros(65, 65, dtype=full.dtype)
        a, b = torch.triu_indices(65, 65, 1)
        dense[a, b] = full
        self.pdists = (dense + dense.T).to(dev())

    def __getitem__(self, i):
        n = 65 if i is None else len(i)
        src = self.pdists if i is None else self.pdists[i.to(dev())][:, i.to(dev())]
        p, q = torch.triu_indices(n, n, 1)
        return src[p, q]


def setup(dname):
    """the embedding of ROUTE_CASE with the optimizer of the reference's product grid: RiemannianAdam, the points exact"""
    from graphembed.modules import BatchedObjective, StereographicProductEmbedding
    from graphembed.objectives import StressLoss
    from graphembed.optim import RiemannianAdam
    emb = StereographicProductEmbedding(65, [5, 5]).to(device=dev(), dtype=DT[dname])
    xs, craws = P.make_inputs(ROUTE_CASE)
    with torch.no_grad():
        for p, man, x, c in zip(emb.xs, emb.manifolds, xs, craws):
            p.copy_(cuda(x, dname))
            man.c.fill_(float(c))
    opt = RiemannianAdam([dict(params=list(emb.xs), lr=0.05, exact=True), dict(params=list(emb.curvature_params), lr=0.05)])
    return emb, opt, BatchedObjective(StressLoss(), Dense(dname), emb)


def minibatch_step(emb, opt, objective, idx):
    opt.zero_grad(set_to_none=True)
    loss = objective(idx)
    loss.backward()
    opt.step()
    emb.stabilize()
    return loss.detach()


@pytest.mark.parametrize('dname', ['f32', 'f64'])
def test_a_product_step_with_adam_is_one_launch_per_factor(dname):
    emb, opt, objective = setup(dname)
    with CallSpy() as spy:
        for k in range(2):
            minibatch_step(emb, opt, objective, torch.from_numpy(BATCHES[k]))
    assert spy.calls.count('mm_stereo_radam_step') == 2 * 2 and 'mm_stereo_map' not in spy.calls, spy.calls
    assert spy.calls.count('mm_stereo_product_loss_subset') == 2 and spy.calls.count('mm_vec_radam_step_multi') == 2, spy.calls
    assert spy.calls.count('mm_stereo_stabilize') == 2 * 2 and len(spy.calls) == 2 * (1 + 2 + 1 + 2), spy.calls
    assert all(float(opt.state[p]['step']) == 3.0 for p in emb.xs)
    assert all(bool(torch.isfinite(p).all()) for p in emb.xs)


def test_a_captured_minibatch_step_equals_eager_steps_bitwise():
    """The objective through an index vector in a static device buffer, the optimizer and stabilize, captured once on a single
    stream and replayed three times with a new batch copied into the buffer between replays, against three eager steps with the
    same batches: bitwise, every kernel on the path sums in a fixed order; the replay follows the curvature updates and the Adam
    step counter without re-capture."""
    dname = 'f32'
    batches = [torch.from_numpy(b).to(dev()) for b in BATCHES]
    emb0, opt0, ob0 = setup(dname)
    for k in range(3):
        minibatch_step(emb0, opt0, ob0, batches[k])
    emb, opt, ob = setup(dname)
    params = list(emb.xs) + list(emb.curvature_params)
    start = [p.detach().clone() for p in params]
    buf = batches[0].clone()

    def rewind():
        with torch.no_grad():
            for p, v in zip(params, start):
                p.copy_(v)
                opt.state[p]['exp_avg'].zero_()
                opt.state[p]['exp_avg_sq'].zero_()
                opt.state[p]['step'].fill_(1.0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: allocator pools, the optimizer's state, the cached workspace
        minibatch_step(emb, opt, ob, buf)
    torch.cuda.current_stream().wait_stream(side)
    rewind()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with CallSpy() as spy:
        with torch.cuda.graph(graph):
            minibatch_step(emb, opt, ob, buf)
    assert spy.calls.count('mm_stereo_product_loss_subset') == 1 and spy.calls.count('mm_stereo_radam_step') == 2, spy.calls
    assert 'mm_stereo_map' not in spy.calls and 'mm_stereo_product_loss' not in spy.calls, spy.calls
    rewind()                         # (capturing does not execute)
    for k in range(3):
        buf.copy_(batches[k])
        graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(params, list(emb0.xs) + list(emb0.curvature_params)):
        assert torch.equal(got.detach(), want.detach())
    for p, p0 in zip(params, list(emb0.xs) + list(emb0.curvature_params)):
        assert float(opt.state[p]['step']) == float(opt0.state[p0]['step']) == 4.0
        assert torch.equal(opt.state[p]['exp_avg'], opt0.state[p0]['exp_avg'])
    assert float(emb.manifolds[0].c.detach()) != float(start[2]), 'the curvature did not move'
