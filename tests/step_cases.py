"""Cases, inputs, regimes and tolerances of the step-against-oracle tests (tests/test_oracle_step.py on the CPU,
tests/test_step_oracle_gpu.py on the device).  Not a test module; plain numpy / torch-CPU, no GPU needed.

A case is one embedding (factors, n, dtype) driven for K = 3 teacher-forced steps by one point rule and one scale rule.
Everything that decides the REGIME of a step is derived from the oracle at the state the step starts from
(`tune`): the learning rate from the median norm of the tangent step, the clip threshold from the per-point norms of the
Riemannian gradient.  Both are ordinary hyper-parameters that the optimizers read at every step (a learning-rate
scheduler changes them the same way), so the device runs exactly the rule the oracle ran."""
import numpy as np
import torch

from oracle import ref_port as rp
from oracle import step as ostep

K = 3
ULP = {'f32': float(np.finfo(np.float32).eps), 'f64': float(np.finfo(np.float64).eps)}

# device against oracle, per quantity (fp32, fp64) — the table of DESIGN.md §5 "Training steps against the oracle"
TOL = {
    'loss': {'f32': 2e-5, 'f64': 1e-11},            # relative (test_config4_product_pair_kernel_full_size)
    'grad_spd': {'f32': 2e-5, 'f64': 1e-10},        # of max|grad| (test_spd_full_size)
    'grad_vec': {'f32': 3e-4, 'f64': 1e-9},         # of max|grad| (test_config4_product_pair_kernel_full_size)
    'scale_grad': {'f32': 2e-4, 'f64': 1e-9},       # of max(|g|, 1e-3 |loss|) (the same test)
    'disp': {'f32': 2e-5, 'f64': 1e-10},            # of max|x' - x|, plus 8 ulp of max|x| (the rounding of the stored point)
    'state': {'f32': 2e-5, 'f64': 1e-10},           # momentum buffer / exp_avg: of max|state| (linear in the gradient)
    'state_sq': {'f32': 4e-5, 'f64': 2e-10},        # exp_avg_sq: twice that (quadratic in the norm)
}
STEP_NORM = (0.1, 1.0)      # the median tangent step, in the manifold's metric
STEP_AIM = 0.3
SCALE_MOVE = 0.05           # |s' - s| aimed at for a trainable scale

POINT_RULES = {
    'rsgd': dict(opt='rsgd', exact=True),
    'rsgd_retr': dict(opt='rsgd', exact=False),
    'momentum': dict(opt='rsgd', exact=True, momentum=0.5, dampening=0.1),
    'momentum_retr': dict(opt='rsgd', exact=False, momentum=0.9, dampening=0.3),
    'adam': dict(opt='radam', exact=True, betas=(0.9, 0.99), nc=False),
    'adam_nc': dict(opt='radam', exact=False, betas=(0.9, None), nc=True),
}
SCALE_RULES = {
    'rsgd': dict(opt='rsgd', clip=True),
    'rsgd_noclip': dict(opt='rsgd', clip=False),
    'momentum': dict(opt='rsgd', clip=True, momentum=0.5),
    'adam': dict(opt='radam', clip=True, betas=(0.9, 0.999), nc=False),
    'frozen': None,
}


def case(cid, route, factors, n, dname, rule, scale_rule, clip, loss='stress', init='perturb', batch=None, adam_t0=1,
         env=None, spread=0.3, big=False):
    return dict(id=cid, route=route, factors=[tuple(f) for f in factors], n=n, dname=dname, rule=rule, scale_rule=scale_rule,
                clip=clip, loss=loss, init=init, batch=batch, adam_t0=adam_t0, env=env or {}, spread=spread, big=big)


CSPHD = [('lorentz', 6), ('sphere', 6), ('spd', 2)]                        # H^5 x S^5 x SPD(2), BASELINE config 4
FOUR = [('euclidean', 5), ('lorentz', 4), ('sphere', 3), ('spd', 3)]

# Not the full cross product: every rule meets every family and both dtypes once at a tail size, every family meets every size
# once, the BASELINE sizes take the rule their config uses (RSGD exact, clip 20 — here: the clip at the oracle's median).
CASES = [
    # ---- (a) the fused one-call step ------------------------------------------------------------------------------------
    case('a-spd3-n131-rsgd-f32', 'fused', [('spd', 3)], 131, 'f32', 'rsgd', 'rsgd', 'median'),
    case('a-spd2-n65-rsgd_retr-f64', 'fused', [('spd', 2)], 65, 'f64', 'rsgd_retr', 'rsgd_noclip', None),
    case('a-spd3-n129-momentum-f64', 'fused', [('spd', 3)], 129, 'f64', 'momentum', 'rsgd', 'all'),
    case('a-spd4-n257-adam-f32', 'fused', [('spd', 4)], 257, 'f32', 'adam', 'adam', 'median', loss='quotient'),
    case('a-spd5-n65-adam_nc-f32', 'fused', [('spd', 5)], 65, 'f32', 'adam_nc', 'momentum', 'none', loss='quotient'),
    case('a-spd4-n3-momentum-f32', 'fused', [('spd', 4)], 3, 'f32', 'momentum', 'frozen', 'none', init='rand'),
    case('a-spd5-n2-adam-f64', 'fused', [('spd', 5)], 2, 'f64', 'adam', 'rsgd', 'all', adam_t0=10),
    case('a-spd2-n129-adam_nc-f64', 'fused', [('spd', 2)], 129, 'f64', 'adam_nc', 'adam', 'median', loss='quotient_l1'),
    case('a-lorentz11-n257-rsgd-f32', 'fused', [('lorentz', 11)], 257, 'f32', 'rsgd', 'rsgd', 'median'),
    case('a-lorentz3-n65-momentum-f32', 'fused', [('lorentz', 3)], 65, 'f32', 'momentum', 'rsgd', 'none'),
    case('a-lorentz16-n129-adam-f64', 'fused', [('lorentz', 16)], 129, 'f64', 'adam', 'adam', 'median', loss='quotient'),
    case('a-lorentz11-n3-adam_nc-f32', 'fused', [('lorentz', 11)], 3, 'f32', 'adam_nc', 'rsgd_noclip', 'all', loss='quotient'),
    case('a-sphere6-n257-rsgd_retr-f32', 'fused', [('sphere', 6)], 257, 'f32', 'rsgd_retr', 'rsgd_noclip', None),
    case('a-sphere3-n129-momentum-f32', 'fused', [('sphere', 3)], 129, 'f32', 'momentum_retr', 'momentum', 'median'),
    case('a-sphere16-n65-adam-f32', 'fused', [('sphere', 16)], 65, 'f32', 'adam', 'adam', 'all', loss='quotient_l2'),
    case('a-sphere6-n2-rsgd-f64', 'fused', [('sphere', 6)], 2, 'f64', 'rsgd', 'rsgd', 'none'),
    case('a-euclidean10-n40-rsgd-f64', 'fused', [('euclidean', 10)], 40, 'f64', 'rsgd', 'rsgd', 'median', init='rand'),   # BASELINE
    case('a-euclidean1-n65-adam-f32', 'fused', [('euclidean', 1)], 65, 'f32', 'adam', 'rsgd', 'median', loss='quotient'),
    case('a-euclidean24-n129-momentum-f32', 'fused', [('euclidean', 24)], 129, 'f32', 'momentum', 'adam', 'all'),
    case('a-euclidean32-n257-adam_nc-f64', 'fused', [('euclidean', 32)], 257, 'f64', 'adam_nc', 'frozen', 'none', loss='quotient'),
    case('a-csphd-n129-rsgd-f32', 'fused', CSPHD, 129, 'f32', 'rsgd', 'rsgd', 'median'),
    case('a-csphd-n65-adam-f64', 'fused', CSPHD, 65, 'f64', 'adam', 'adam', 'median', loss='quotient'),
    case('a-csphd-n257-momentum-f32', 'fused', CSPHD, 257, 'f32', 'momentum', 'rsgd', 'all'),
    case('a-four-n131-adam_nc-f32', 'fused', FOUR, 131, 'f32', 'adam_nc', 'momentum', 'none', loss='quotient'),
    case('a-four-n2-rsgd_retr-f64', 'fused', FOUR, 2, 'f64', 'rsgd_retr', 'rsgd_noclip', None),
    # product_step_kernel<T, SD> without an SPD factor (SD = 0: two and three vector factors), and one vector factor + SPD
    case('a-l4e3-n131-rsgd-f32', 'fused', [('lorentz', 4), ('euclidean', 3)], 131, 'f32', 'rsgd', 'rsgd', 'median'),
    case('a-s5l8e7-n65-adam-f64', 'fused', [('sphere', 5), ('lorentz', 8), ('euclidean', 7)], 65, 'f64', 'adam', 'adam', 'median',
         loss='quotient'),
    case('a-e6spd2-n129-momentum-f32', 'fused', [('euclidean', 6), ('spd', 2)], 129, 'f32', 'momentum', 'rsgd', 'all'),
    # the BASELINE sizes (one per family: the oracle costs CPU seconds per step there)
    case('a-spd3-n5000-rsgd-f32', 'fused', [('spd', 3)], 5000, 'f32', 'rsgd', 'rsgd', 'median', big=True),
    case('a-spd4-n2274-rsgd-f32', 'fused', [('spd', 4)], 2274, 'f32', 'rsgd', 'rsgd', 'median', loss='quotient', big=True),
    case('a-lorentz11-n4039-rsgd-f32', 'fused', [('lorentz', 11)], 4039, 'f32', 'rsgd', 'rsgd', 'median', big=True),
    case('a-csphd-n1025-rsgd-f32', 'fused', CSPHD, 1025, 'f32', 'rsgd', 'rsgd', 'median', big=True),
    # ---- (b) the unfused one-call step ------------------------------------------------------------------------------------
    case('b-spd6-n65-rsgd-f64', 'unfused', [('spd', 6)], 65, 'f64', 'rsgd', 'rsgd', 'median', spread=0.2),
    case('b-spd6-n129-adam-f32', 'unfused', [('spd', 6)], 129, 'f32', 'adam', 'adam', 'all', spread=0.2),
    case('b-euclidean64-n3-rsgd_retr-f32', 'unfused', [('euclidean', 64)], 3, 'f32', 'rsgd_retr', 'rsgd', 'all'),   # (m > 32: no symmetric pair kernel)
    case('b-lorentz24-n129-momentum-f32', 'unfused', [('lorentz', 24)], 129, 'f32', 'momentum', 'rsgd', 'median'),
    case('b-sphere24-n257-adam-f32', 'unfused', [('sphere', 24)], 257, 'f32', 'adam', 'momentum', 'median', loss='quotient'),
    case('b-euclidean24-n65-rsgd-f64-env', 'unfused', [('euclidean', 24)], 65, 'f64', 'rsgd', 'rsgd', 'median',
         env={'MM_VEC_STEP_UNFUSED': '1'}),     # (fused without the switch)
    # ---- (c) the eager optimizers behind fused_objective(...).backward() ----------------------------------------------------
    case('c-spd3-n129-adam-f32', 'eager', [('spd', 3)], 129, 'f32', 'adam', 'adam', 'median', loss='quotient'),
    case('c-lorentz11-n129-momentum-f32', 'eager', [('lorentz', 11)], 129, 'f32', 'momentum', 'rsgd', 'median'),
    case('c-sphere16-n65-adam_nc-f64', 'eager', [('sphere', 16)], 65, 'f64', 'adam_nc', 'momentum', 'all', loss='quotient'),
    case('c-lorentz24-n257-adam-f32', 'eager', [('lorentz', 24)], 257, 'f32', 'adam', 'adam', 'median'),
    case('c-sphere24-n65-momentum-f64', 'eager', [('sphere', 24)], 65, 'f64', 'momentum_retr', 'rsgd', 'none'),
    case('c-euclidean64-n129-adam-f32', 'eager', [('euclidean', 64)], 129, 'f32', 'adam', 'rsgd_noclip', 'median'),
    case('c-csphd-n129-rsgd-f32', 'eager', CSPHD, 129, 'f32', 'rsgd', 'rsgd', 'median'),    # multi-parameter group launches
    case('c-csphd-n65-adam-f64', 'eager', CSPHD, 65, 'f64', 'adam', 'adam', 'all', loss='quotient'),
    case('c-lorentz11-n65-rsgd-f32-env', 'eager', [('lorentz', 11)], 65, 'f32', 'rsgd', 'rsgd', 'median',
         env={'MM_VEC_RULE_GENERIC': '1'}),
    case('c-sphere6-n129-adam-f32-env', 'eager', [('sphere', 6)], 129, 'f32', 'adam', 'adam', 'median',
         env={'MM_VEC_RULE_GENERIC': '1'}),
    # ---- (d) node minibatches: step(indices=idx) ----------------------------------------------------------------------------
    case('d-spd3-n129-b50-momentum-f32', 'minibatch', [('spd', 3)], 129, 'f32', 'momentum', 'rsgd', 'median', batch=50),
    case('d-spd4-n257-b100-adam-f32', 'minibatch', [('spd', 4)], 257, 'f32', 'adam', 'adam', 'median', loss='quotient', batch=100),
    case('d-spd3-n65-b23-rsgd-f64', 'minibatch', [('spd', 3)], 65, 'f64', 'rsgd', 'rsgd', 'all', batch=23),
    case('d-lorentz11-n257-b100-adam-f32', 'minibatch', [('lorentz', 11)], 257, 'f32', 'adam', 'rsgd', 'median', batch=100),
    case('d-lorentz11-n129-b50-momentum-f64', 'minibatch', [('lorentz', 11)], 129, 'f64', 'momentum', 'adam', 'median',
         loss='quotient', batch=50),
    # ---- (e) the sharded form on a one-rank communicator: the step kernels take their gradient from p.grad -----------------
    case('e-spd3-n129-adam-f32', 'sharded', [('spd', 3)], 129, 'f32', 'adam', 'rsgd', 'median', loss='quotient'),
    case('e-lorentz11-n257-momentum-f32', 'sharded', [('lorentz', 11)], 257, 'f32', 'momentum', 'rsgd', 'median'),
]
BY_ID = {c['id']: c for c in CASES}


def ids(cases):
    return [c['id'] for c in cases]


# ------------------------------------------------------------------------------------------------------------------- inputs
def _round(a, dname):
    """Values the case's dtype represents exactly: the device and the oracle start from the same numbers."""
    return np.asarray(a, dtype=np.float32 if dname == 'f32' else np.float64).astype(np.float64)


def _on_manifold(kind, x, dname):
    """Put the rounded points back on the manifold IN the case's arithmetic, so that the stored values are the points (an
    fp32-rounded Lorentz point is 1e-7 off the hyperboloid for an fp64 kernel: a rule that re-projects and one that does not
    would then differ by that much, far above the fp64 tolerances, with neither at fault)."""
    x = torch.as_tensor(x, dtype=torch.float32 if dname == 'f32' else torch.float64)
    if kind == 'spd':
        x = 0.5 * (x + x.transpose(-2, -1))
    elif kind == 'lorentz':
        x = rp.Lorentz(x.shape[-1]).projx(x)
    elif kind == 'sphere':
        x = x / x.norm(dim=-1, keepdim=True)
    return x.double().numpy()


def _tangent(kind, man, x, gen):
    u = torch.randn(x.shape, dtype=torch.float64, generator=gen)
    return man.proju(x, u)


def points(factor, n, init, spread, gen, dname):
    """The reference's initialisation (`rand`), optionally followed by ManifoldEmbedding.perturb(spread): a retraction along a
    random tangent of that norm."""
    kind, dim = factor
    man = ostep.manifold(factor)
    x = man.rand(n, dtype=torch.float64, generator=gen)
    if init == 'perturb':
        u = _tangent(kind, man, x, gen)
        u = u / man.norm(x, u, keepdim=True) * spread
        x = man.retr(x, u)
    else:
        assert init == 'rand', init
    return _on_manifold(kind, x.numpy(), dname)


def _seed(c):
    import zlib
    return zlib.crc32(c['id'].encode()) % (2**31)


def initial(c):
    """(state, data): the parameters and optimizer state a case starts from, and its targets."""
    gen = torch.Generator().manual_seed(_seed(c))
    n, k = c['n'], len(c['factors'])
    xs = [points(f, n, c['init'], c['spread'], gen, c['dname']) for f in c['factors']]
    scales = [float(np.float32(v)) for v in ([0.5] if k == 1 else [0.5, 0.3, 0.7, 0.4][:k])]
    data = {}
    if c['batch'] is None:
        t = torch.rand(n * (n - 1) // 2, dtype=torch.float64, generator=gen) * 0.9 + 0.05
        data['target'] = _round(t.numpy(), c['dname'])
    else:
        t = torch.rand(n, n, dtype=torch.float64, generator=gen) * 0.9 + 0.05
        t = torch.triu(t, 1)
        data['dense'] = _round((t + t.T).numpy(), c['dname'])
        data['batches'] = [torch.randperm(n, generator=gen)[:c['batch']].numpy().astype(np.int64) for _ in range(K)]
    state = dict(xs=xs, scales=scales, point_states=[{} for _ in xs], scale_states=[{} for _ in xs])
    # preloaded optimizer state: random tangents at the points of the size of the gradient, positive second moments
    value, grads, sgrads = objective(c, state, data, 0)
    prule, srule = POINT_RULES[c['rule']], SCALE_RULES[c['scale_rule']]
    for i, (f, x, g) in enumerate(zip(c['factors'], xs, grads)):
        man = ostep.manifold(f)
        xt, gt = torch.from_numpy(x), torch.from_numpy(g)
        gn = man.norm(xt, man.egrad2rgrad(xt, gt), keepdim=True)
        med = float(gn.median())
        u = _tangent(f[0], man, xt, gen)
        u = u / man.norm(xt, u, keepdim=True) * med * (0.5 + torch.rand(gn.shape, dtype=torch.float64, generator=gen))
        if prule['opt'] == 'rsgd' and prule.get('momentum', 0):
            state['point_states'][i] = {'momentum_buffer': _round(u.numpy(), c['dname'])}
        elif prule['opt'] == 'radam':
            v = (med * (0.5 + torch.rand(gn.shape, dtype=torch.float64, generator=gen)))**2
            state['point_states'][i] = {'exp_avg': _round(u.numpy(), c['dname']),
                                        'exp_avg_sq': _round(v.expand(xt.shape).numpy(), c['dname']), 'step': c['adam_t0']}
    for i, g in enumerate(sgrads):
        if srule is None:
            continue
        if srule['opt'] == 'rsgd' and srule.get('momentum', 0):
            state['scale_states'][i] = {'momentum_buffer': _round(0.7 * g, c['dname'])}
        elif srule['opt'] == 'radam':
            state['scale_states'][i] = {'exp_avg': _round(-0.4 * g, c['dname']), 'exp_avg_sq': _round(1.3 * g * g, c['dname']),
                                        'step': c['adam_t0']}
    return state, data


def loss_of(c, k):
    """Stress; quotient with epoch 0, 1, 2 across the three steps and alpha != 1 (plus its l1-only and l2-only forms)."""
    if c['loss'] == 'stress':
        return {'kind': 'stress'}
    return {'kind': 'quotient', 'epoch': k, 'alpha': 1.25, 'inc_l1': c['loss'] != 'quotient_l2', 'inc_l2': c['loss'] != 'quotient_l1'}


def batch_of(c, data, k):
    return None if c['batch'] is None else data['batches'][k]


KINK_MARGIN = 1e-4     # |q| of every quotient term: a hundred times the fp32 rounding of a distance


def settle_targets(c, state, data, k, d2):
    """QuotientLoss is a sum of |q|: its derivative jumps where a term crosses zero, and a pair that sits within rounding of
    such a kink gets the other sign in another precision — a gradient error of one pair's full weight (1e-3 of the largest
    entry at n = 1000) that says nothing about the kernel.  With millions of pair-terms per case some do sit there.  So the
    targets of the pairs within KINK_MARGIN of a kink AT THE STATE THE STEP STARTS FROM are moved by 1e-3 (of themselves)
    before the step — on the host copy, which the device then reads too.  Returns the number of targets moved."""
    loss = loss_of(c, k)
    if loss['kind'] == 'stress':
        return 0
    idx = batch_of(c, data, k)
    i, j = ostep.pair_list(c['n'], idx)
    md = sum(ostep.softplus(s) * d for s, d in zip(state['scales'], d2))
    moved = 0
    for _ in range(8):
        gd = ostep.pair_targets(data.get('target'), data.get('dense'), i, j)
        near = ostep.kink_distance(loss, gd, md) < KINK_MARGIN
        if not near.any():
            return moved
        moved += int(near.sum())
        new = _round(gd[near] * (1 + 1e-3), c['dname'])
        if 'dense' in data:
            data['dense'][i[near], j[near]] = new
            data['dense'][j[near], i[near]] = new
        else:
            data['target'][near] = new
    raise AssertionError('targets keep landing on a kink of the quotient loss')


def objective(c, state, data, k, d2=None):
    return ostep.objective(c['factors'], state['xs'], state['scales'], loss_of(c, k), target=data.get('target'),
                           dense=data.get('dense'), idx=batch_of(c, data, k), d2=d2)


# ------------------------------------------------------------------------------------------------------------------- regime
def _f32(v):
    return float(np.float32(v))


def tune(c, state, data, k, obj):
    """Hyper-parameters of step k, chosen from the oracle at the state the step starts from:
    * max_grad_norm — 'median': the median Riemannian gradient norm (of the points the step has a gradient for); 'all': half
      the smallest; 'none': twice the largest; None: no clip at all;
    * lr — so that the median tangent step has norm STEP_AIM in the manifold's metric (the step norm is linear in lr).
    Scales: clip at half of |g| (binds) or none; lr so that the scale moves by SCALE_MOVE.
    Returns (point_rule, scale_rule)."""
    value, grads, sgrads = obj
    idx = batch_of(c, data, k)
    rows = slice(None) if idx is None else np.sort(idx)
    norms = []
    for f, x, g in zip(c['factors'], state['xs'], grads):
        man = ostep.manifold(f)
        xt, gt = torch.from_numpy(x), torch.from_numpy(g)
        norms.append(man.norm(xt, man.egrad2rgrad(xt, gt), keepdim=True).reshape(-1).numpy()[rows])
    norms = np.concatenate(norms)      # (one clip value per parameter group: all factors share it)
    prule = dict(POINT_RULES[c['rule']])
    prule['max_grad_norm'] = {None: None, 'median': _f32(np.median(norms)), 'all': _f32(0.5 * norms.min()),
                              'none': _f32(2.0 * norms.max())}[c['clip']]
    probe = dict(prule, lr=1.0)
    steps = []
    for f, x, g, st in zip(c['factors'], state['xs'], grads, state['point_states']):
        xt = torch.from_numpy(x)
        _, _, dg = ostep.apply_rule(ostep.manifold(f), xt, torch.from_numpy(g), probe, ostep._state_in(st, xt.shape, torch.float64))
        steps.append(dg['step_norm'][rows])
    prule['lr'] = _f32(STEP_AIM / np.median(np.concatenate(steps)))
    srule = SCALE_RULES[c['scale_rule']]
    if srule is not None:
        srule = dict(srule)
        clip = srule.pop('clip')
        gmin = min(abs(g) for g in sgrads)
        srule['max_grad_norm'] = _f32(0.5 * gmin) if clip else None
        probe = dict(srule, lr=1.0)
        moves = []
        for s, g, st in zip(state['scales'], sgrads, state['scale_states']):
            st_ = torch.tensor([[s]], dtype=torch.float64)
            ns, _, _ = ostep.apply_rule(ostep.FLAT, st_, torch.tensor([[g]], dtype=torch.float64), probe,
                                        ostep._state_in(st, (1, 1), torch.float64))
            moves.append(abs(float(ns) - s))
        srule['lr'] = _f32(SCALE_MOVE / max(moves))
    return prule, srule


def oracle_step(c, state, data, k):
    """(point_rule, scale_rule, want, regime): the oracle's step k from `state`, with the regime it provably is in.
    May move targets in `data` (`settle_targets`, regime['targets_moved']): the device must read the same ones."""
    d2 = ostep.pair_distances(c['factors'], state['xs'], batch_of(c, data, k))
    moved = settle_targets(c, state, data, k, d2)
    obj = objective(c, state, data, k, d2)
    prule, srule = tune(c, state, data, k, obj)
    idx = batch_of(c, data, k)
    want = ostep.train_step(c['factors'], state['xs'], state['scales'], loss_of(c, k), prule, srule, target=data.get('target'),
                            dense=data.get('dense'), idx=idx, point_states=state['point_states'],
                            scale_states=state['scale_states'], obj=obj)
    rows = slice(None) if idx is None else np.sort(idx)
    binds = np.concatenate([d['binds'][rows] for d in want['diag']])
    steps = np.concatenate([d['step_norm'][rows] for d in want['diag']])
    regime = dict(clip=c['clip'], bind_share=float(binds.mean()), median_step=float(np.median(steps)),
                  max_step=float(steps.max()), lr=prule['lr'], max_grad_norm=prule['max_grad_norm'], targets_moved=moved)
    # the case is in the regime it names — asserted from the oracle's per-point norms, before anything is compared
    assert STEP_NORM[0] <= regime['median_step'] <= STEP_NORM[1], regime
    if c['clip'] == 'median':
        assert 0.2 <= regime['bind_share'] <= 0.8, regime
    elif c['clip'] == 'all':
        assert regime['bind_share'] == 1.0, regime
    else:
        assert regime['bind_share'] == 0.0, regime
    if srule is not None and SCALE_RULES[c['scale_rule']]['clip']:
        assert all(d['binds'].all() for d in want['scale_diag']), 'the scale clip binds'
    return prule, srule, want, regime


def describe(regime):
    return (f"clip={regime['clip']} binds on {100 * regime['bind_share']:.0f}% of the points, median step "
            f"{regime['median_step']:.3f} (max {regime['max_step']:.3f}), lr={regime['lr']:.4g}"
            + (f", {regime['targets_moved']} targets moved off a kink" if regime['targets_moved'] else ''))


def next_state(c, got):
    """The state the next step starts from: what the step under test wrote (`new_xs`, `new_scales`, states)."""
    return dict(xs=[np.asarray(x, dtype=np.float64) for x in got['new_xs']], scales=[float(s) for s in got['new_scales']],
                point_states=got['point_states'], scale_states=got['scale_states'])


# --------------------------------------------------------------------------------------------------------------- comparison
def errors(c, state, want, got):
    """Per quantity: (error, allowed) of `got` against the oracle's `want`, in the units of TOL.  `got` has the keys of
    oracle.step.train_step's result (numpy fp64)."""
    dn = c['dname']
    out = {}
    lref = want['loss']
    out['loss'] = (abs(got['loss'] - lref), TOL['loss'][dn] * abs(lref))
    for i, f in enumerate(c['factors']):
        fam = f'{f[0]}{f[1]}'
        g, w = np.asarray(got['grads'][i], np.float64), want['grads'][i]
        key = 'grad_spd' if f[0] == 'spd' else 'grad_vec'
        out[f'grad/{fam}'] = (np.abs(g - w).max(), TOL[key][dn] * np.abs(w).max())
        x = state['xs'][i]
        dw, dg = want['new_xs'][i] - x, np.asarray(got['new_xs'][i], np.float64) - x
        out[f'disp/{fam}'] = (np.abs(dg - dw).max(), TOL['disp'][dn] * np.abs(dw).max() + 8 * ULP[dn] * np.abs(x).max())
        for name, tkey in (('momentum_buffer', 'state'), ('exp_avg', 'state'), ('exp_avg_sq', 'state_sq')):
            if name in want['point_states'][i]:
                w_ = want['point_states'][i][name]
                g_ = np.asarray(got['point_states'][i][name], np.float64).reshape(w_.shape)
                out[f'{name}/{fam}'] = (np.abs(g_ - w_).max(), TOL[tkey][dn] * np.abs(w_).max())
        if 'step' in want['point_states'][i]:
            out[f'adam_step/{fam}'] = (abs(float(got['point_states'][i]['step']) - want['point_states'][i]['step']), 0.0)
        if want['scale_diag'][i] is not None:      # (a frozen scale has no gradient: requires_grad is off, modules.py:36-39)
            sg, sw = got['scale_grads'][i], want['scale_grads'][i]
            out[f'scale_grad/{fam}'] = (abs(sg - sw), TOL['scale_grad'][dn] * max(abs(sw), 1e-3 * abs(lref)))
        s = state['scales'][i]
        dsw, dsg = want['new_scales'][i] - s, got['new_scales'][i] - s
        out[f'scale_disp/{fam}'] = (abs(dsg - dsw), TOL['disp'][dn] * abs(dsw) + 8 * ULP[dn] * abs(s))
        for name, tkey in (('momentum_buffer', 'state'), ('exp_avg', 'state'), ('exp_avg_sq', 'state_sq')):
            if name in want['scale_states'][i]:
                w_ = float(want['scale_states'][i][name])
                out[f'scale_{name}/{fam}'] = (abs(float(got['scale_states'][i][name]) - w_), TOL[tkey][dn] * abs(w_))
        if 'step' in want['scale_states'][i]:
            out[f'scale_adam_step/{fam}'] = (abs(float(got['scale_states'][i]['step']) - want['scale_states'][i]['step']), 0.0)
    return out


def worst(errs):
    """{quantity: error / allowed} (inf when nothing is allowed and the error is not zero)."""
    return {q: (e / a if a > 0 else (0.0 if e == 0 else float('inf'))) for q, (e, a) in errs.items()}
