"""Cases, inputs and fp64 oracles of the Grassmann node-minibatch objective (mm_grass_pdist_loss_subset) and of the fused
RiemannianAdam step of Grassmann / Stiefel points (mm_mat_radam_step), under the ABSOLUTE tolerance rule of tests/mat_cases.py
(`measure`, `Quantity.bound`, `check`): bound_f32 = max(32 cond, 2 port32) + 16 2^-24 S, built from oracle/ref_port.py alone.
Host code only; nothing here runs a kernel.  tests/test_grass_subset_host.py walks everything below on the CPU and holds
bound_f32 <= CAP S; tests/test_grass_subset_gpu.py and tests/test_mat_radam_gpu.py make the same calls.

Minibatch objective.  Shapes mat_cases.ROW_SHAPES (one per P, padded and unpadded N), regimes mat_cases.regimes, n_total = 257,
bs in BATCHES: tiles are 16 rows x 64 columns, so 65 and 130 cross one and two column blocks and leave a ragged last row tile,
2 and 3 are the one- and three-pair batches.  The batch is a fixed-seed randperm slice forced to contain node 0 and node
n_total - 1, not monotone.  The dense target matrix is fp32 in [0.5, 3.5] and deliberately NOT symmetric: reading
dense[idx[b]][idx[a]] is caught.  The quotient loss has kinks at m = alpha g and m + 1/(epoch+1) = alpha g (a fixed-seed matrix
comes within 3e-7 of one at (6,3) `spread` bs = 130), so every target of a batch pair whose relative margin to either kink is
below MARGIN in the fp64 oracle is multiplied by 1.01 (in fp32), repeatedly, until both margins hold: cases are nudged, never
dropped.  Compared: loss, grad_x [n_total, N, p] (S = the largest per-node magnitude sum of the oracle's per-pair
contributions), grad_scale (S = the magnitude sum of its per-pair terms), with the exclusions of mat_cases.loss_compared and
dist_compared and no others: no grad_x at p = 2 `uniform`, no grad_scale in `init`.

Adam.  Three consecutive steps from empty state as ONE measured function of (x, g0, g1, g2): after every step x_new (scale
'map'), exp_avg and exp_avg_sq (scale max|W|).  Gradients vectors('radam0..2'); at cnt >= 8 point 5 has a zero gradient in all
three steps (zero tangent with zero moment) and point 7 in steps 2 and 3 (the decaying moment).  Clip at the median gradient
norm of the first step."""
import functools

import torch

import mat_cases as mc
from mat_cases import CAP, U32, Quantity, check, measure, pair_slice, points, ref, rows_of, vectors  # noqa: F401

gc = mc.gc
N_TOTAL = 257
BATCHES = (2, 3, 65, 130)
LOSSES = ('stress', 'quotient')
SHAPES = mc.ROW_SHAPES
MARGIN = 1e-3
QUOTIENT = gc.QUOTIENT

RADAM_SHAPES = list(mc.ROW_SHAPES) + [(2, 1), (7, 3), (8, 4), (9, 1)]
RADAM_STIEFEL_ONLY = [(3, 3), (4, 4)]
RADAM_CNT = (1, 63, 64, 65, 130)
RADAM_LR = 0.05
BETAS = (0.9, 0.999)
VARIANTS = {'grassmann_svd': ('grassmann', 'svd', False), 'grassmann_qr': ('grassmann', 'qr', False),
            'grassmann_exp': ('grassmann', 'svd', True), 'stiefel_svd': ('stiefel', 'svd', False),
            'stiefel_qr': ('stiefel', 'qr', False)}


def radam_shapes(kind):
    return RADAM_SHAPES + (RADAM_STIEFEL_ONLY if kind == 'stiefel' else [])


# ---- the minibatch objective -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_idx(n_total, bs, perm=False):
    """int64 node ids of the batch: a fixed-seed randperm slice that contains node 0 and node n_total - 1 and is not monotone
    (`perm`: bs = n_total, the whole permutation)"""
    g = torch.Generator().manual_seed(gc._seed('batch', n_total, bs))
    order = torch.randperm(n_total, generator=g)
    if perm:
        assert bs == n_total
        return order
    rest = order[(order != 0) & (order != n_total - 1)][:bs - 2]
    idx = torch.cat([torch.tensor([n_total - 1]), rest, torch.tensor([0])])   # last node first, node 0 last: not monotone
    assert idx.numel() == bs and torch.unique(idx).numel() == bs
    return idx


@functools.lru_cache(maxsize=None)
def raw_dense(n_total):
    g = torch.Generator().manual_seed(gc._seed('dense', n_total))
    d = (torch.rand(n_total, n_total, dtype=torch.float64, generator=g) * 3.0 + 0.5).float()
    assert not torch.equal(d, d.T)
    return d


def _margins(md, tg):
    """the two relative distances of a pair from the kinks of the quotient loss"""
    ag = tg * QUOTIENT['alpha']
    return (md / ag - 1.0).abs(), (ag / (md + 1.0 / (QUOTIENT['epoch'] + 1)) - 1.0).abs()


@functools.lru_cache(maxsize=None)
def _model_dists(regime, N, p, n_total, bs, perm):
    idx = batch_idx(n_total, bs, perm)
    i, j = ref.triu_pairs(bs)
    x = points(regime, n_total, N, p).double()
    d2 = mc.OracleGrassmann(N, p).dist(x[idx[i]], x[idx[j]], squared=True)
    return idx[i], idx[j], torch.nn.functional.softplus(torch.tensor(gc.SCALE_RAW, dtype=torch.float64)) * d2


@functools.lru_cache(maxsize=None)
def dense(regime, N, p, bs, n_total=N_TOTAL, perm=False):
    """the fp32 target matrix of the case: raw_dense with the targets of the batch's pairs nudged away from the kinks"""
    ni, nj, md = _model_dists(regime, N, p, n_total, bs, perm)
    d = raw_dense(n_total).clone()
    for _ in range(64):
        a, b = _margins(md, d[ni, nj].double())
        bad = (a < MARGIN) | (b < MARGIN)
        if not bool(bad.any()):
            return d
        d[ni[bad], nj[bad]] = d[ni[bad], nj[bad]] * 1.01   # fp32 arithmetic: what the kernels will read
    raise AssertionError('the targets could not be nudged away from the kinks')


def kink_margin(regime, N, p, bs, n_total=N_TOTAL, perm=False):
    ni, nj, md = _model_dists(regime, N, p, n_total, bs, perm)
    a, b = _margins(md, dense(regime, N, p, bs, n_total, perm)[ni, nj].double())
    return float(torch.minimum(a, b).min())


def subset_compared(regime, N, p):
    """mat_cases.loss_compared and the p = 2 `uniform` exclusion of mat_cases.dist_compared"""
    names = mc.loss_compared(regime, N, p)
    return tuple(n for n in names if not (n == 'grad_x' and mc._closed_form_uniform(regime, N, p)))


@functools.lru_cache(maxsize=None)
def subset_quantities(regime, N, p, bs, loss_name, ranges=(None, ), n_total=N_TOTAL, perm=False):
    """{(rows, 'loss' | 'grad_x' | 'grad_scale'): Quantity} of the objective over the batch's pairs of rows `rows` (batch positions)"""
    man = mc.OracleGrassmann(N, p)
    idx = batch_idx(n_total, bs, perm)
    i, j = ref.triu_pairs(bs)
    ni, nj = idx[i], idx[j]
    D = dense(regime, N, p, bs, n_total, perm)

    def scatter(ti, tj):
        return torch.zeros(n_total, N, p, dtype=ti.dtype).index_add_(0, ni, ti).index_add_(0, nj, tj)

    def fn(x):
        xi, xj = x[ni].clone().requires_grad_(True), x[nj].clone().requires_grad_(True)
        s = torch.tensor(gc.SCALE_RAW, dtype=x.dtype, requires_grad=True)
        d2 = man.dist(xi, xj, squared=True)
        md = torch.nn.functional.softplus(s) * d2
        tg = D[ni, nj].to(x.dtype)
        vals, kinds = {}, {}
        for r in ranges:
            lo, hi = pair_slice(bs, r)
            if lo == hi:
                continue
            loss = gc.oracle_loss(loss_name, tg[lo:hi], md[lo:hi])
            ti, tj, gs, dldm = torch.autograd.grad(loss, [xi, xj, s, md], retain_graph=True)
            per_pair_s = dldm * d2.detach() * torch.sigmoid(s.detach())
            vals[(r, 'loss')], kinds[(r, 'loss')] = loss.detach().reshape(1), 'dist'
            vals[(r, 'grad_x')], kinds[(r, 'grad_x')] = scatter(ti, tj), float(scatter(ti.abs(), tj.abs()).max())
            vals[(r, 'grad_scale')], kinds[(r, 'grad_scale')] = gs.reshape(1), float(per_pair_s.abs().sum())
        return vals, kinds
    return measure(fn, (points(regime, n_total, N, p), ), ('subset', regime, N, p, bs, loss_name, n_total, perm))


# row shards of the batch at bs = 130: mat_cases.rows_of and the two ranges that complete COVER, a disjoint cover of the batch's rows
COVER = ((0, 1), (1, 43), (43, 86), (86, 128), (128, 129), (129, 130))
SHARDS = rows_of(130) + ((1, 43), (86, 128))
assert rows_of(130)[1:5] == ((0, 1), (43, 86), (128, 129), (129, 130))


def ranges_of(bs):
    return SHARDS if bs == 130 else (None, )


def loss_spec(loss_name):
    """(loss kind, alpha, eps, terms) as the C ABI takes them"""
    from graphembed import _backend as B
    if loss_name == 'stress':
        return B.LOSS_STRESS, 1.0, 1.0, 3
    return B.LOSS_QUOTIENT, float(QUOTIENT['alpha']), 1.0 / (QUOTIENT['epoch'] + 1), 3


def subset_cases():
    for N, p in SHAPES:
        for regime in mc.regimes(N, p):
            for bs in BATCHES:
                for loss_name in LOSSES:
                    yield N, p, regime, bs, loss_name


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
def oracle_manifold(kind, retr, N, p):
    man = ref.make(kind, N, p)
    if retr == 'qr':
        man.retr = mc._retr_qr(kind, man)
    return man


@functools.lru_cache(maxsize=None)
def radam_grads(cnt, N, p):
    """the three gradients: point 5 never moves, point 7 gets a gradient in the first step only"""
    gs = [vectors(f'radam{k}', cnt, N, p).clone() for k in range(3)]
    if cnt >= 8:
        for k in range(3):
            gs[k][5] = 0
        gs[1][7] = 0
        gs[2][7] = 0
    return tuple(gs)


@functools.lru_cache(maxsize=None)
def radam_clip(kind, cnt, N, p):
    man = ref.make(kind, N, p)
    x, g = points('uniform', cnt, N, p).double(), radam_grads(cnt, N, p)[0].double()
    return float(man.norm(x, man.egrad2rgrad(x, g)).median())


@functools.lru_cache(maxsize=None)
def radam_quantities(variant, cnt, N, p, nc, lr=RADAM_LR, clip='median'):
    """{'x1', 'exp_avg1', 'exp_avg_sq1', ..., 'exp_avg_sq3'}: the whole three-step trajectory as one measured function"""
    kind, retr, exact = VARIANTS[variant]
    man = oracle_manifold(kind, retr, N, p)
    if clip == 'median':
        clip = radam_clip(kind, cnt, N, p)

    def fn(x, g0, g1, g2):
        state, vals, kinds = {}, {}, {}
        for k, g in enumerate((g0, g1, g2)):
            x = ref.radam_step(man, x, g, state, lr=lr, betas=BETAS, nc=nc, max_grad_norm=clip, exact=exact)
            assert state['step'] == k + 2
            vals[f'x{k + 1}'], kinds[f'x{k + 1}'] = x, 'map'
            vals[f'exp_avg{k + 1}'], kinds[f'exp_avg{k + 1}'] = state['exp_avg'], 'dist'
            vals[f'exp_avg_sq{k + 1}'], kinds[f'exp_avg_sq{k + 1}'] = state['exp_avg_sq'], 'dist'
        return vals, kinds
    return measure(fn, (points('uniform', cnt, N, p), ) + radam_grads(cnt, N, p), ('radam', variant, cnt, N, p, nc, lr, clip))


# ---- two minibatch training steps ------------------------------------------------------------------------------------------------
TRAIN = dict(N=5, p=2, regime='spread', bs=65, lr=0.01, clip=100.0)   # the reference grid's optimizer settings (run_grid.py:24-36)


@functools.lru_cache(maxsize=None)
def train_batches(n_total=N_TOTAL, bs=TRAIN['bs']):
    """two batches that share 30 nodes and differ in 35"""
    g = torch.Generator().manual_seed(gc._seed('train batches', n_total, bs))
    order = torch.randperm(n_total, generator=g)
    b1, b2 = order[:bs], torch.cat([order[bs:2 * bs - 30], order[:30]])
    assert b2.numel() == bs and torch.unique(b2).numel() == bs and len(set(b1.tolist()) & set(b2.tolist())) == 30
    return b1, b2


@functools.lru_cache(maxsize=None)
def train_quantities(n_total=N_TOTAL):
    """points and both moments after two steps objective (stress, fixed scale) -> backward -> RiemannianAdam(exact, clipped) on
    the two batches: one measured function of the initial points"""
    N, p = TRAIN['N'], TRAIN['p']
    man = mc.OracleGrassmann(N, p)
    D = raw_dense(n_total)
    i, j = ref.triu_pairs(TRAIN['bs'])

    def fn(x):
        state = {}
        sp = torch.nn.functional.softplus(torch.tensor(gc.SCALE_RAW, dtype=x.dtype))
        for b in train_batches(n_total):
            ni, nj = b[i], b[j]
            xr = x.clone().requires_grad_(True)
            loss = ref.stress_loss(D[ni, nj].to(x.dtype), sp * man.dist(xr[ni], xr[nj], squared=True))
            g, = torch.autograd.grad(loss, [xr])
            x = ref.radam_step(man, x, g, state, lr=TRAIN['lr'], betas=BETAS, max_grad_norm=TRAIN['clip'], exact=True)
        vals = {'x': x, 'exp_avg': state['exp_avg'], 'exp_avg_sq': state['exp_avg_sq']}
        return vals, {'x': 'map', 'exp_avg': 'dist', 'exp_avg_sq': 'dist'}
    return measure(fn, (points(TRAIN['regime'], n_total, N, p), ), ('train', n_total))
