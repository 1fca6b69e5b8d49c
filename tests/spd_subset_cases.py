"""Cases, inputs, the fp64 oracle and the rule of the node-minibatch form of the affine-invariant SPD pair kernel
(csrc/spd_pair.hpp: spd_pdist_bwd_kernel<T, D, TI, LOSS, SQ, NCX, SUB = true>, reached through mm_spd_pdist_loss_subset and
graphembed.modules._SingleSubsetLoss): D = 2 .. 9 x {fp32, fp64} x {stress, quotient} = 32 instantiations.  Host code only;
nothing here runs a kernel.  tests/test_spd_subset_host.py walks everything below on the CPU, tests/test_spd_subset_gpu.py makes
the calls.

Inputs.  N_TOTAL = 257 points per (regime, D) in the regimes `init`, `mid`, `wide` of tests/spd_point_cases.py (same formulas):
rounded to float32, symmetrised bit for bit, widened afterwards, so fp32 kernels, fp64 kernels and the oracle see the same numbers.
Index vectors: grass_subset_cases.batch_idx(N_TOTAL, bs) — distinct, not monotone, containing node 0 and node 256; bs = 257 is
the whole table as a permutation.  Raw scale grass_cases.SCALE_RAW, quotient loss grass_cases.QUOTIENT, window [1e-8, 1e8].

Dense targets, one fp32 matrix per (regime, D, bs) serving both losses: grass_subset_cases.raw_dense(257) — deliberately NOT
symmetric — times the median model distance of the batch's pairs (targets and distances have one magnitude), diagonal 0 (as
GraphDataset builds it); the target of a batch pair within MARGIN = 1e-3 of a kink of the quotient loss (m = alpha t,
alpha t = m + eps) is multiplied by 1.01 in fp32 until clear: cases are nudged, never dropped (`kink_margin`, `nudged`).

Oracle: oracle.step.objective([('spd', D)], [x], [SCALE_RAW], loss, dense=, idx=, pairs=) — oracle/exact.c in fp64: the loss, the
dense [257, D, D] gradient (zero rows outside the batch) and the scale gradient.  A row range of the batch is the explicit pair
list of that range.

Rule (that of grass_cases.check, S written out):   e_sub <= 2 e_full + 64 eps(dtype) S
    e_sub   deviation of the in-kernel minibatch from the oracle
    e_full  deviation FROM THE SAME ORACLE of the established route on the same GPU in the same test: gather x[idx], the
            pair-vector targets dense[idx[a], idx[b]], the full-batch fused kernel (mm_spd_pdist_loss, held by
            tests/test_spd_gpu.py and tests/test_spd_shift_gpu.py), the gradient rows scattered into zeros
    S       loss |W|; grad_x max|W|; grad_scale the magnitude sum sigmoid(s) sum |slope d2| of its per-pair terms
No absolute tolerance is invented.  So that the relative rule cannot hide a wrong pair, the GPU test also requires, per case, the
allowance actually granted to grad_x to be below HALF of `one_pair_effect`: the move of the oracle's grad_x when the single pair of
the case with the median |dense[i][j] - dense[j][i]| gets its transposed target.  The host test holds the teeth of every case
that has a pair: transposing `dense` moves grad_x by at least TRANSPOSE_MIN S, one_pair_effect is at least ONE_PAIR_MIN S.

Cases (not a cross product; CASE_COUNTS, asserted by the host test), per dtype:
    instantiations  D = 2 .. 9 x {init, mid, wide} x {stress, quotient}, bs = 130, all rows:                       48
    batch sizes     D in {2, 3, 4, 6}, `mid`, both losses, bs in {2, 3, 65, 129, 257}: one and three pairs; one column past a
                    64-column block and one past a 128-column block (the fp32 D = 2, 3 backward takes two columns per lane);
                    the whole table as a permutation:                                                                40
    row shards      D in {3, 4, 6}, `mid`, both losses, bs = 130, every range of grass_subset_cases.SHARDS (8: all rows, one
                    row, the middle third, a one-pair row, the last row — no pair —, an empty range, and the two ranges that
                    complete COVER, a disjoint cover of the batch's rows):                                           48
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grass_subset_cases as gsc  # noqa: E402
from grass_cases import DT, QUOTIENT, SCALE_RAW, CallSpy, _seed, deviation, eps_of  # noqa: E402,F401
from grass_subset_cases import COVER, SHARDS, loss_spec  # noqa: E402,F401
from mat_cases import pair_slice  # noqa: E402
from oracle import step as ostep  # noqa: E402

N_TOTAL = 257
DIMS = (2, 3, 4, 5, 6, 7, 8, 9)
DNAMES = ('f32', 'f64')
REGIMES = ('init', 'mid', 'wide')
LOSSES = ('stress', 'quotient')
MARGIN = 1e-3
WMIN, WMAX = 1e-8, 1e8
BS = 130
BATCH_DIMS, BATCH_SIZES = (2, 3, 4, 6), (2, 3, 65, 129, 257)
SHARD_DIMS = (3, 4, 6)
MASKED_DIMS, MASKED_SIZES = (3, 4, 6), (65, 130)
ABI_DIMS, ABI_BS = (3, 4, 6), 65
TRANSPOSE_MIN, ONE_PAIR_MIN = 0.05, 5e-4
CASE_COUNTS = {'instantiations': 48, 'batch sizes': 40, 'row shards': 48}
NAMES = ('loss', 'grad_x', 'grad_scale')
LOSS = {'stress': {'kind': 'stress'}, 'quotient': dict(kind='quotient', **QUOTIENT)}
# (regime, D) -> what is added to the seed of its points: a case that missed a threshold of the teeth got another draw, the
# thresholds stayed.  The first draws gave: `mid` D = 2 one_pair_effect 4.1e-4 S and D = 6 3.7e-4 S (quotient, bs = 257), `mid`
# D = 4 a transposed matrix 4.6e-2 S (stress, the one-row shard).
POINT_DRAW = {('mid', 2): (2, ), ('mid', 4): (4, ), ('mid', 6): (1, )}

Case = collections.namedtuple('Case', 'regime D bs loss rows')
Oracle = collections.namedtuple('Oracle', 'loss grad_x grad_scale S')   # fp64 tensors [1], [N_TOTAL, D, D], [1]; S: name -> scale


def case_id(c):
    return f'spd({c.D}) {c.regime} {c.loss} bs={c.bs}' + ('' if c.rows is None else f' rows={c.rows[0]}:{c.rows[1]}')


def instantiation_cases():
    return [Case(regime, D, BS, loss, None) for D in DIMS for regime in REGIMES for loss in LOSSES]


def batch_size_cases():
    return [Case('mid', D, bs, loss, None) for D in BATCH_DIMS for loss in LOSSES for bs in BATCH_SIZES]


def shard_cases():
    return [Case('mid', D, BS, loss, rows) for D in SHARD_DIMS for loss in LOSSES for rows in SHARDS]


SWEEPS = {'instantiations': instantiation_cases, 'batch sizes': batch_size_cases, 'row shards': shard_cases}


def all_cases():
    return [c for sweep in SWEEPS.values() for c in sweep()]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _T(a):
    return np.swapaxes(a, -1, -2)


@functools.lru_cache(maxsize=None)
def points(regime, D):
    """float32 [N_TOTAL, D, D], symmetric bit for bit (the formulas of spd_point_cases.points)"""
    rng = np.random.default_rng(_seed('spd subset point', regime, N_TOTAL, D, *POINT_DRAW.get((regime, D), ())))
    if regime == 'wide':
        a = rng.standard_normal((N_TOTAL, D, D))
        x = a @ _T(a) + np.eye(D)
    else:
        s = rng.standard_normal((N_TOTAL, D, D))
        s = 0.5 * (s + _T(s))
        s *= (0.1 if regime == 'init' else 1.5) / np.sqrt((s * s).sum((-2, -1), keepdims=True))
        w, v = np.linalg.eigh(s)
        x = (v * np.exp(w)[:, None, :]) @ _T(v)
    t = torch.from_numpy(np.ascontiguousarray(x)).float()
    return 0.5 * (t + t.transpose(-1, -2))


def batch_idx(bs):
    return gsc.batch_idx(N_TOTAL, bs, perm=bs == N_TOTAL)


@functools.lru_cache(maxsize=None)
def second_batch(bs=ABI_BS):
    """a batch of the same size with no node of batch_idx(bs): the other nodes in descending order, rotated by 7 (not monotone)"""
    taken = set(batch_idx(bs).tolist())
    rest = torch.tensor([k for k in range(N_TOTAL - 1, -1, -1) if k not in taken])[:bs]
    assert rest.numel() == bs
    return torch.roll(rest, 7)


def batch_pairs(idx, rows=None):
    """(node i, node j) of the pairs (a, b), a < b, of the batch positions whose row a lies in `rows`, in pair-vector order"""
    a, b = np.triu_indices(idx.numel(), 1)
    lo, hi = pair_slice(idx.numel(), rows)
    nodes = idx.numpy()
    return nodes[a[lo:hi]], nodes[b[lo:hi]]


def _xs(regime, D):
    return [points(regime, D).double().numpy()]


@functools.lru_cache(maxsize=None)
def _d2(regime, D, idx_key):
    """squared distances of the batch's pairs (the oracle's, fp64)"""
    idx = torch.tensor(idx_key)
    return ostep.pair_distances([('spd', D)], _xs(regime, D), pairs=batch_pairs(idx))[0]


def model_dists(regime, D, idx):
    return ostep.softplus(SCALE_RAW) * _d2(regime, D, tuple(idx.tolist()))


def _margins(md, tg):
    return ostep.kink_distance(LOSS['quotient'], tg, md)


def _nudge(dm, regime, D, idx):
    """dm with the targets of idx's pairs at least MARGIN away from both kinks; returns the number of pairs that were moved"""
    i, j = batch_pairs(idx)
    md = model_dists(regime, D, idx)
    moved = np.zeros(md.shape, dtype=bool)
    for _ in range(64):
        bad = _margins(md, dm[i, j].double().numpy()) < MARGIN
        if not bad.any():
            return int(moved.sum())
        moved |= bad
        dm[i[bad], j[bad]] = dm[i[bad], j[bad]] * 1.01     # fp32 arithmetic: the value the kernels read
    raise AssertionError('the targets could not be nudged away from the kinks')


@functools.lru_cache(maxsize=None)
def _dense(regime, D, bs, with_second):
    idx = batch_idx(bs)
    med = float(np.median(model_dists(regime, D, idx)))
    dm = (gsc.raw_dense(N_TOTAL).double() * med).float()
    dm.fill_diagonal_(0.0)
    moved = _nudge(dm, regime, D, idx)
    if with_second:
        moved += _nudge(dm, regime, D, second_batch(bs))
    assert float((dm - dm.T).abs().max()) > 0.5 * med
    return dm, moved


def dense(regime, D, bs, with_second=False):
    """the fp32 target matrix [N_TOTAL, N_TOTAL] of the case (read-only).  `with_second`: the pairs of second_batch(bs) are clear
    of the kinks too — they share no pair with the first batch, whose targets (and oracle) stay what they are."""
    return _dense(regime, D, bs, with_second)[0]


def nudged(c):
    return _dense(c.regime, c.D, c.bs, False)[1]


def kink_margin(c, idx=None, dm=None):
    idx = batch_idx(c.bs) if idx is None else idx
    dm = dense(c.regime, c.D, c.bs) if dm is None else dm
    i, j = batch_pairs(idx)
    return float(_margins(model_dists(c.regime, c.D, idx), dm[i, j].double().numpy()).min()) if i.size else float('inf')


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def n_pairs(c):
    lo, hi = pair_slice(c.bs, c.rows)
    return hi - lo


def objective_of(regime, D, dm, idx, loss_name, rows=None):
    """the Oracle of the pairs of `rows` of the batch `idx` against the targets dm[idx[a]][idx[b]]"""
    i, j = batch_pairs(idx, rows)
    lo, hi = pair_slice(idx.numel(), rows)
    d2 = _d2(regime, D, tuple(idx.tolist()))[lo:hi]
    dmn = dm.double().numpy()
    value, grads, sgrads = ostep.objective([('spd', D)], _xs(regime, D), [SCALE_RAW], LOSS[loss_name], dense=dmn, pairs=(i, j), d2=[d2])
    _, slope = ostep.loss_and_slope(LOSS[loss_name], dmn[i, j], ostep.softplus(SCALE_RAW) * d2)
    gx = torch.from_numpy(np.ascontiguousarray(grads[0]))
    assert gx.shape == (N_TOTAL, D, D) and np.isfinite(value) and bool(torch.isfinite(gx).all())
    S = {'loss': abs(value), 'grad_x': float(gx.abs().max()), 'grad_scale': ostep.sigmoid(SCALE_RAW) * float(np.abs(slope * d2).sum())}
    return Oracle(torch.tensor([value], dtype=torch.float64), gx, torch.tensor([sgrads[0]], dtype=torch.float64), S)


@functools.lru_cache(maxsize=None)
def oracle(c):
    """computed once per case, shared, never modified"""
    return objective_of(c.regime, c.D, dense(c.regime, c.D, c.bs), batch_idx(c.bs), c.loss, c.rows)


def gathered_oracle(c, ascending=True):
    """the same objective as the reference evaluates it: on gathered points with the gathered pair-vector targets
    dense[idx[a]][idx[b]] (a < b, pair-vector order), the gradient rows scattered into zeros.  The oracle evaluates a pair from
    its lower-numbered point (exact.spd_pairs takes lo < hi), and which of the two points is factorised first moves d^2 and its
    gradient by a few ulp.  `ascending`: the points are gathered in ascending node order, so every pair is evaluated in the
    orientation `oracle` uses and the two differ by the order of their sums alone; otherwise in batch order, x[idx]."""
    idx = batch_idx(c.bs)
    i, j = batch_pairs(idx, c.rows)
    a, b = np.triu_indices(c.bs, 1)
    lo, hi = pair_slice(c.bs, c.rows)
    a, b = a[lo:hi], b[lo:hi]
    take = idx
    if ascending:
        take, order = torch.sort(idx)
        pos = np.empty(c.bs, dtype=np.int64)
        pos[order.numpy()] = np.arange(c.bs)       # batch position -> row of the gathered copy
        a, b = pos[a], pos[b]
    xb = points(c.regime, c.D).double()[take].numpy()
    tg = dense(c.regime, c.D, c.bs).double().numpy()[i, j]
    value, grads, sgrads = ostep.objective([('spd', c.D)], [xb], [SCALE_RAW], LOSS[c.loss], target=tg, pairs=(a, b))
    gx = torch.zeros(N_TOTAL, c.D, c.D, dtype=torch.float64)
    gx[take] = torch.from_numpy(np.ascontiguousarray(grads[0]))
    return torch.tensor([value], dtype=torch.float64), gx, torch.tensor([sgrads[0]], dtype=torch.float64)


def median_pair_of(dm, idx, rows=None):
    """(node i, node j) of the pair of `rows` of the batch with the median |dm[i][j] - dm[j][i]|"""
    i, j = batch_pairs(idx, rows)
    dmn = dm.double().numpy()
    k = np.argsort(np.abs(dmn[i, j] - dmn[j, i]), kind='stable')[i.size // 2]
    return int(i[k]), int(j[k])


def median_pair(c):
    return median_pair_of(dense(c.regime, c.D, c.bs), batch_idx(c.bs), c.rows)


def pair_effect_of(regime, D, dm, idx, loss_name, rows=None):
    """max |move of the oracle's grad_x| (absolute, not divided by S) when median_pair_of(dm, idx, rows) gets its transposed
    target.  The objective is a sum over the pairs: the move is the difference of that ONE pair's term under the two targets."""
    i, j = median_pair_of(dm, idx, rows)
    xs, pair = _xs(regime, D), (np.array([i]), np.array([j]))
    g = [ostep.objective([('spd', D)], xs, [SCALE_RAW], LOSS[loss_name], target=np.array([float(t)]), pairs=pair)[1][0]
         for t in (dm[i, j], dm[j, i])]
    return float(np.abs(g[1] - g[0]).max())


@functools.lru_cache(maxsize=None)
def one_pair_effect(c):
    return pair_effect_of(c.regime, c.D, dense(c.regime, c.D, c.bs), batch_idx(c.bs), c.loss, c.rows)


def one_pair_effect_literal(c):
    """the same move from the whole objective, evaluated again with that one target replaced"""
    i, j = median_pair(c)
    other = dense(c.regime, c.D, c.bs).clone()
    other[i, j] = other[j, i]
    moved = objective_of(c.regime, c.D, other, batch_idx(c.bs), c.loss, c.rows).grad_x
    return float((moved - oracle(c).grad_x).abs().max())


def transpose_effect(c):
    """max |move of the oracle's grad_x| when the whole target matrix is transposed"""
    moved = objective_of(c.regime, c.D, dense(c.regime, c.D, c.bs).T.contiguous(), batch_idx(c.bs), c.loss, c.rows).grad_x
    return float((moved - oracle(c).grad_x).abs().max())


# ---- the rule --------------------------------------------------------------------------------------------------------------------
RECORDS = []   # (sweep, dname, quantity, e_sub / allowance, e_sub / S, e_full / S, tag): printed last by the GPU test


def allowance(e_full, S, dt):
    return 2 * e_full + 64 * eps_of(dt) * S


def hold(sweep, tag, dname, full, sub, want, failures):
    """the rule for the three quantities of one call: `full` and `sub` are (loss [1], grad_x, grad_scale [1]) of the established
    route and of the in-kernel minibatch, `want` the Oracle.  Prints every figure before it judges; returns the allowances."""
    granted = {}
    for name, f, s, w in zip(NAMES, full, sub, want[:3]):
        S = want.S[name]
        e_full, e_sub = deviation(f, w), deviation(s, w)
        allow = allowance(e_full, S, DT[dname])
        line = f'{tag} {dname} {name}: e_sub {e_sub:.3e} e_full {e_full:.3e} allowance {allow:.3e} S {S:.3e}'
        print(line)
        RECORDS.append((sweep, dname, name, e_sub / max(allow, 1e-300), e_sub / max(S, 1e-300), e_full / max(S, 1e-300), tag))
        if not e_sub <= allow:
            failures.append(line)
        granted[name] = allow
    return granted
