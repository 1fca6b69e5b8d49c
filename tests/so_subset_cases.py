"""Cases, inputs and the long-double oracle of the SO(n) node-minibatch kernels (csrc/so.hip with SUB: mm_so_pdist_fwd_subset,
mm_so_pdist_bwd_subset, mm_so_pdist_loss_subset), under the ABSOLUTE tolerance rule of tests/mat_cases.py (`measure`,
`Quantity.bound`, `check`, verbatim) with the scales S of tests/so_cases.py.  Host code only; nothing here runs a kernel.
tests/test_so_subset_host.py walks everything below on the CPU and holds bound_f32 <= CAP S for every compared quantity, with no
exclusions; tests/test_so_subset_gpu.py makes the same calls.

What tests/so_cases.py has (`points`, `_pair_any`, `_w`, `loss_terms_ld` / `loss_terms_torch`, `_scatter`, `upstream`) is composed
with an index vector: n_total = 257, bs in BATCHES — tiles are 16 rows x 64 columns, so 65 and 130 cross one and two column blocks
and leave a ragged last row tile, 2 and 3 are the one- and three-pair batches — N in (2, 3, 4), regimes `init` and `spread`, both
losses.  The batch is grass_subset_cases.batch_idx (not monotone, contains node 0 and node 256); the dense targets are
grass_subset_cases.raw_dense (fp32, deliberately NOT symmetric) with every target of a batch pair within MARGIN of a kink of the
quotient loss multiplied by 1.01 (in fp32) until clear: cases are nudged, never dropped; one matrix per (regime, N, bs) serves both
losses.

Quantities:
  objective     loss, grad_x [n_total, N, N] and grad_scale per row range (bs = 130: grass_subset_cases.SHARDS, of which COVER is a
                disjoint cover of the batch's rows);
  pair vector   `val` and `grad` (the upstream pattern of mat_cases.upstream over the batch's pairs, scattered by node) squared and
                non-squared; the non-squared gradient is compared in `spread` only, as in so_cases (in `init` it is a unit vector
                field of points 1e-2 apart);
  repeat        the pair-vector quantities at bs = 65 with positions 7 and 40 naming the same node (`spread`);
  train         two minibatch steps stress objective -> RiemannianAdam (retraction) as ONE measured function of the points.
S: values and the loss max|W|; grad_x and the pair-vector gradient the largest per-node magnitude sum of the oracle's per-pair
contributions; grad_scale the magnitude sum of its per-pair terms; points after a step max(1, max|W|).  

SO(2) `init` has two distinct points only (u = +-1e-2 J / sqrt 2), and at bs = 2, bs = 3 and in the one-pair range (128, 129) of
bs = 130 every pair of the batch coincides: the oracle's gradients, pair values and grad_scale are exactly 0 there, so S = 0, and
bound_f32 <= CAP S can only mean a bound of 0 (the rule's cond is not 0: the perturbation draws move the two table rows apart).
`held` says so: a quantity with S = 0 is held to EXACT zeros — 18 of the 408, counted by the host test, which asserts that their
oracle value is exactly 0."""
import functools

import numpy as np
import torch

import grass_subset_cases as gsc
import so_cases as sc
from so_cases import CAP, DIMS, LOSSES, REGIMES, Quantity, check, measure, pair_slice, points, upstream  # noqa: F401

LD = sc.LD
N_TOTAL = 257
BATCHES = (2, 3, 65, 130)
MARGIN = 1e-3
SHARDS, COVER = gsc.SHARDS, gsc.COVER
REPEAT = dict(bs=65, a=7, b=40, regime='spread')
TRAIN = dict(N=3, regime='spread', bs=65, lr=0.01, clip=100.0)   # the reference grid's optimizer settings
BETAS = gsc.BETAS


def batch_idx(bs, repeat=False):
    idx = gsc.batch_idx(N_TOTAL, bs)
    if repeat:
        idx = idx.clone()
        idx[REPEAT['b']] = idx[REPEAT['a']]
    return idx


def _nodes(bs, repeat=False):
    """(node of the row side, node of the column side) of the batch's pairs, in pair order"""
    idx = batch_idx(bs, repeat)
    i, j = torch.triu_indices(bs, bs, 1)
    return idx[i], idx[j]


def ranges_of(bs):
    return SHARDS if bs == 130 else (None, )


# ---- the dense targets -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_dists(regime, N, bs):
    ni, nj = _nodes(bs)
    x = points(regime, N_TOTAL, N).double()
    d2 = sc.pair_ld(sc._ld(x[ni]), sc._ld(x[nj]), grad=False)[0]
    return ni, nj, sc._t(sc._softplus(sc.SCALE_RAW) * d2)


@functools.lru_cache(maxsize=None)
def _nudged(regime, N, bs):
    ni, nj, md = _model_dists(regime, N, bs)
    d = gsc.raw_dense(N_TOTAL).clone()
    touched = torch.zeros(md.numel(), dtype=torch.bool)
    for _ in range(64):
        a, b = gsc._margins(md, d[ni, nj].double())
        bad = (a < MARGIN) | (b < MARGIN)
        if not bool(bad.any()):
            return d, int(touched.sum())
        touched |= bad
        d[ni[bad], nj[bad]] = d[ni[bad], nj[bad]] * 1.01   # fp32 arithmetic: what the kernels will read
    raise AssertionError('the targets could not be nudged away from the kinks')


def dense(regime, N, bs):
    """the fp32 target matrix of the case: raw_dense with the targets of the batch's pairs nudged away from the kinks"""
    return _nudged(regime, N, bs)[0]


def nudged_pairs(regime, N, bs):
    return _nudged(regime, N, bs)[1]


def kink_margin(regime, N, bs):
    ni, nj, md = _model_dists(regime, N, bs)
    a, b = gsc._margins(md, dense(regime, N, bs)[ni, nj].double())
    return float(torch.minimum(a, b).min())


# ---- quantities ------------------------------------------------------------------------------------------------------------------
def _scatter(ni, nj, ti, tj):
    return sc._scatter(N_TOTAL, ni, nj, ti, tj)


def _tt(a):
    """a long-double array or scalar as a float64 tensor; tensors as they are"""
    return a if isinstance(a, torch.Tensor) else sc._t(a)


def _terms(x, ni, nj, loss_name, tg):
    """per pair: loss term, its d / d scale_raw, d / d x_j [N, N] (= -d / d x_i) — long double arrays (oracle) or float32 tensors"""
    d2, dy = sc._pair_any(x[ni], x[nj])
    if sc._is64(x):
        sp, sig = sc._softplus(sc.SCALE_RAW), 1 / (1 + np.exp(-LD(sc.SCALE_RAW)))
        l, dldm = sc.loss_terms_ld(loss_name, sp * d2, sc._ld(tg))
        return l, dldm * d2 * sig, (dldm * sp)[:, None, None] * dy
    sr = torch.tensor(sc.SCALE_RAW, dtype=x.dtype)
    sp, sig = torch.nn.functional.softplus(sr), torch.sigmoid(sr)
    l, dldm = sc.loss_terms_torch(loss_name, sp * d2, tg.to(x.dtype))
    return l, dldm * d2 * sig, (dldm * sp).reshape(-1, 1, 1) * dy


@functools.lru_cache(maxsize=None)
def loss_quantities(regime, N, bs, loss_name):
    """{(rows, 'loss' | 'grad_x' | 'grad_scale'): Quantity} of the objective over the batch's pairs of rows `rows` (batch positions),
    for every range of ranges_of(bs) that has a pair"""
    ni, nj = _nodes(bs)
    tg = dense(regime, N, bs)[ni, nj]

    def fn(x):
        l, per_s, gj = _terms(x, ni, nj, loss_name, tg)
        vals, kinds = {}, {}
        for r in ranges_of(bs):
            lo, hi = pair_slice(bs, r)
            if lo == hi:
                continue
            part = _tt(gj[lo:hi])
            vals[(r, 'loss')], kinds[(r, 'loss')] = _tt(l[lo:hi].sum()).reshape(1), 'dist'
            vals[(r, 'grad_x')] = _scatter(ni[lo:hi], nj[lo:hi], -part, part)
            kinds[(r, 'grad_x')] = float(_scatter(ni[lo:hi], nj[lo:hi], part.abs(), part.abs()).max())
            vals[(r, 'grad_scale')] = _tt(per_s[lo:hi].sum()).reshape(1)
            kinds[(r, 'grad_scale')] = float(abs(per_s[lo:hi]).sum())
        return vals, kinds
    return measure(fn, (points(regime, N_TOTAL, N), ), ('so subset', regime, N, bs))


@functools.lru_cache(maxsize=None)
def pdist_quantities(regime, N, bs, squared, repeat=False):
    """{'val' | 'grad': Quantity} of the batch's pair vector and of the gradient of sum_k upstream_k value_k w.r.t. the full table"""
    ni, nj = _nodes(bs, repeat)

    def fn(x):
        d2, dy = sc._pair_any(x[ni], x[nj])
        val, dv = sc._w(d2, squared)
        val, dy = sc._out(val), sc._out(dv[:, None, None] * dy)
        gj = upstream(val.numel()).to(val.dtype).reshape(-1, 1, 1) * dy
        return ({'val': val, 'grad': _scatter(ni, nj, -gj, gj)},
                {'val': 'dist', 'grad': float(_scatter(ni, nj, gj.abs(), gj.abs()).max())})
    return measure(fn, (points(regime, N_TOTAL, N), ), ('so subset', regime, N, bs))


def pdist_compared(regime, squared):
    return ('val', 'grad') if squared or regime == 'spread' else ('val', )


def held(q):
    """the Quantity the GPU tests compare against: q itself, or — S = 0, see the module docstring — a bound of exactly 0"""
    return q if q.scale > 0 else Quantity(q.want, 0.0, 0.0, 0.0)


def repeat_pair():
    """position of the pair (a, b) of REPEAT in the batch's pair vector"""
    return pair_slice(REPEAT['bs'], (REPEAT['a'], REPEAT['a'] + 1))[0] + REPEAT['b'] - REPEAT['a'] - 1


def loss_spec(loss_name):
    return gsc.loss_spec(loss_name)


def cases():
    for N in DIMS:
        for regime in REGIMES:
            for bs in BATCHES:
                yield N, regime, bs


def compared(N):
    """(tag, name, Quantity) of everything the GPU tests hold to the rule at this size, one point set at a time (the quantity sets
    of one (regime, bs) share the oracle's pair lists: their perturbation draws carry one key)"""
    for regime in REGIMES:
        for bs in BATCHES:
            for loss_name in LOSSES:
                for (rows, name), q in loss_quantities(regime, N, bs, loss_name).items():
                    yield f'so subset {N} {regime} bs={bs} {loss_name} rows={rows}', f'so_subset_{name}', q
            for squared in (True, False):
                q = pdist_quantities(regime, N, bs, squared)
                for name in pdist_compared(regime, squared):
                    yield f'so subset pdist {N} {regime} bs={bs}', f'so_subset_pdist_{"d2" if squared else "d"}_{name}', q[name]


def repeat_compared(N):
    for squared in (True, False):
        q = pdist_quantities(REPEAT['regime'], N, REPEAT['bs'], squared, True)
        for name in ('val', 'grad'):
            yield f'so subset pdist {N} repeated node', f'so_subset_repeat_{"d2" if squared else "d"}_{name}', q[name]


# ---- the stochastic-neighbour objective on the batch's pair vector ---------------------------------------------------------------
SNE = dict(N=3, regime='spread', bs=65, alpha=1.3)


@functools.lru_cache(maxsize=None)
def sne_quantities():
    """loss, grad_x [n_total, N, N] and grad_scale of StochasticNeighborLoss(inclusive)(dense[idx[a], idx[b]], softplus(scale) d2)
    on the batch: the long-double formulas of tests/sne_cases.py on the oracle's pair vector (port32: the loss's own torch ops)"""
    import sne_cases
    N, bs, alpha = SNE['N'], SNE['bs'], SNE['alpha']
    ni, nj = _nodes(bs)
    tg = gsc.raw_dense(N_TOTAL)[ni, nj]

    def fn(x):
        d2, dy = sc._pair_any(x[ni], x[nj])
        if sc._is64(x):
            sp, sig = sc._softplus(sc.SCALE_RAW), 1 / (1 + np.exp(-LD(sc.SCALE_RAW)))
            loss, gmd = sne_cases.oracle_of(tg.double().numpy(), sp * d2, 'incl', alpha)
            per_s, gj = gmd * d2 * sig, _tt((gmd * sp)[:, None, None] * dy)
        else:
            from graphembed.objectives import StochasticNeighborLoss
            sr = torch.tensor(sc.SCALE_RAW, dtype=x.dtype)
            sp, sig = torch.nn.functional.softplus(sr), torch.sigmoid(sr)
            md = (sp * d2).requires_grad_(True)
            loss = StochasticNeighborLoss(native=False)(tg.to(x.dtype), md, alpha=alpha)
            gmd, = torch.autograd.grad(loss, [md])
            loss, per_s, gj = loss.detach(), gmd * d2 * sig, (gmd * sp).reshape(-1, 1, 1) * dy
        vals = {'loss': _tt(loss).reshape(1), 'grad_x': _scatter(ni, nj, -gj, gj), 'grad_scale': _tt(per_s.sum()).reshape(1)}
        return vals, {'loss': 'dist', 'grad_x': float(_scatter(ni, nj, gj.abs(), gj.abs()).max()), 'grad_scale': float(abs(per_s).sum())}
    return measure(fn, (points(SNE['regime'], N_TOTAL, N), ), ('so subset sne', ))


# ---- two minibatch training steps ------------------------------------------------------------------------------------------------
def train_batches():
    """two batches that share 30 nodes and differ in 35"""
    return gsc.train_batches(N_TOTAL, TRAIN['bs'])


@functools.lru_cache(maxsize=None)
def train_quantities():
    """points and both moments after two steps objective (stress, fixed scale) -> backward -> RiemannianAdam (polar retraction,
    clipped) on the two batches: one measured function of the initial points (oracle/ref_port.py's radam_step on St(N, N))"""
    from oracle import ref_port as ref
    N = TRAIN['N']
    man = ref.Stiefel(N, N)
    D = gsc.raw_dense(N_TOTAL)
    i, j = torch.triu_indices(TRAIN['bs'], TRAIN['bs'], 1)

    def fn(x):
        state = {}
        for b in train_batches():
            ni, nj = b[i], b[j]
            gj = _tt(_terms(x, ni, nj, 'stress', D[ni, nj])[2])
            x = ref.radam_step(man, x, _scatter(ni, nj, -gj, gj), state, lr=TRAIN['lr'], betas=BETAS, max_grad_norm=TRAIN['clip'],
                               exact=False)
        vals = {'x': x, 'exp_avg': state['exp_avg'], 'exp_avg_sq': state['exp_avg_sq']}
        return vals, {'x': 'map', 'exp_avg': 'dist', 'exp_avg_sq': 'dist'}
    return measure(fn, (points(TRAIN['regime'], N_TOTAL, N), ), ('so subset train', ))
