"""Cases, inputs, fp64 oracles and the rule of the bit-deterministic SPD pair kernels (csrc/spd_det.hpp: spd_det::pair_kernel<T, D,
LOSS, SQ> and spd_det::finalize_kernel<T, D>, reached through mm_spd_pdist_bwd_det / mm_spd_pdist_loss_det):
D = 2 .. 9 x {fp32, fp64} x {bwd squared, bwd not squared, stress, quotient} = 64 instantiations.  Host code only; nothing here
runs a kernel.  tests/test_spd_det_host.py walks everything below on the CPU, tests/test_spd_det_gpu.py makes the calls.

Inputs.  Points: the leading n of spd_subset_cases.points(regime, D) (257 per regime in `init`, `mid`, `wide`; the atomic
full-batch route has met the one-pair teeth on exactly these points); the one n = 1025 case draws its own with the `mid` formula.
One vector u of uniform [0.5, 3.5) randoms per (regime, D, n), no smooth structure, serves every kind:
    targets   u x the median model distance of the case's pairs, fp32; a target within MARGIN = 1e-3 of a kink of the quotient
              loss is multiplied by 1.01 in fp32 until clear — nudged, never dropped
    upstream  g = u x a random sign, fp32 (the gradient is linear in g: no scale is needed)
fp32 values, widened for fp64 and for the oracles.  Raw scale grass_cases.SCALE_RAW, quotient loss grass_cases.QUOTIENT,
window [1e-8, 1e8].  A row range takes the slice of the pair vector it owns (the layout of mm_spd_pdist_fwd's `out`).

Oracles (fp64):  losses   oracle.step.objective (oracle/exact.c) on the explicit pair list of the range
                 bwd      the fp64 port's pdist (oracle.ref_port.SPD through oracle.step.manifold: LAPACK factorisations at
                          every D) with autograd for the given g, symmetric part

Rule (the project's):   e_det <= 2 e_atomic + 64 eps(dtype) S
    e_det     deviation of the _det entry from the oracle
    e_atomic  deviation FROM THE SAME ORACLE of mm_spd_pdist_bwd / mm_spd_pdist_loss on the same GPU in the same test
    S         loss |W|; grad_x max|W|; grad_scale sigmoid(s) sum |slope d2| (as spd_subset_cases)
and, so that the relative rule cannot hide a wrong pair: the allowance actually granted to grad_x must be below HALF of the
case's `one_pair_effect` — the move of the oracle's grad_x when ONE pair (the one with the median |u[k] - u[k + 1]|) gets its
SUCCESSOR's g resp. target.  The host test holds the teeth: one_pair_effect >= ONE_PAIR_MIN S (5e-4, the project's).

Sizes.  At these n every geometry has rows_per_chunk = 8 (asserted by the host test against mm_spd_pdist_det_geometry):
n = 64 is 8 full chunks (a size AT a chunk boundary), 65 one row past it (9 chunks, a ragged last one of one row), 129 / 130 /
257 are 17 / 17 / 33 chunks with ragged last ones; 257 is one column past a 256-column workgroup; 1025 is 5 column groups x 129
chunks.  n = 2, 3: one and three pairs.

Cases (CASE_COUNTS, asserted by the host test), per dtype:
    instantiations  D = 2 .. 9 x {init, mid, wide} x 4 kinds, n = 130, all rows:                                       96
    sizes           D in {2, 3, 4, 6}, `mid`, 4 kinds, n in {2, 3, 64, 65, 129, 257}:                                  96
    row shards      D in {3, 4, 6}, `mid`, 4 kinds, n = 130, every range of grass_subset_cases.SHARDS (8):             96
    large           SPD(3), `mid`, n = 1025, bwd_sq (fp32 only in the GPU test):                                       1
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

import spd_subset_cases as S  # noqa: E402
from grass_cases import DT, QUOTIENT, SCALE_RAW, CallSpy, _seed, deviation, eps_of  # noqa: E402,F401
from grass_subset_cases import COVER, SHARDS  # noqa: E402,F401
from mat_cases import pair_slice  # noqa: E402
from oracle import exact  # noqa: E402
from oracle import step as ostep  # noqa: E402

DIMS, DNAMES, REGIMES = S.DIMS, S.DNAMES, S.REGIMES
KINDS = ('bwd_sq', 'bwd_nsq', 'stress', 'quotient')
LOSS_KINDS = ('stress', 'quotient')
WMIN, WMAX, MARGIN, ONE_PAIR_MIN = S.WMIN, S.WMAX, S.MARGIN, S.ONE_PAIR_MIN
N_INST = 130
SIZE_DIMS, SIZES = (2, 3, 4, 6), (2, 3, 64, 65, 129, 257)
SHARD_DIMS, N_SHARD = (3, 4, 6), 130
# (an upstream gradient, not a loss: at n = 1025 a node's loss gradient adds 1024 pair terms and ONE replaced target moves it by
# 4.8e-4 S (stress), 1.4e-4 S (quotient) — below ONE_PAIR_MIN; under a g of random signs the terms add incoherently and one pair
# moves the sum by 4.7e-3 S.  The threshold stayed.  Loss slots of several column groups: the n = 257 cases, 2 x 33 slots.)
LARGE = ('mid', 3, 1025, 'bwd_sq')
ROWS_PER_CHUNK = 8      # of every geometry up to n = 8192 (the host test asserts it for the sizes used)
CASE_COUNTS = {'instantiations': 96, 'sizes': 96, 'row shards': 96, 'large': 1}
NAMES = ('loss', 'grad_x', 'grad_scale')

Case = collections.namedtuple('Case', 'regime D n kind rows')
Oracle = collections.namedtuple('Oracle', 'loss grad_x grad_scale S')   # fp64 tensors [1], [n, D, D], [1] (bwd kinds: grad_x only)


def case_id(c):
    return f'spd({c.D}) {c.regime} {c.kind} n={c.n}' + ('' if c.rows is None else f' rows={c.rows[0]}:{c.rows[1]}')


def instantiation_cases():
    return [Case(regime, D, N_INST, kind, None) for D in DIMS for regime in REGIMES for kind in KINDS]


def size_cases():
    return [Case('mid', D, n, kind, None) for D in SIZE_DIMS for kind in KINDS for n in SIZES]


def shard_cases():
    return [Case('mid', D, N_SHARD, kind, rows) for D in SHARD_DIMS for kind in KINDS for rows in SHARDS]


def large_cases():
    return [Case(*LARGE, None)]


SWEEPS = {'instantiations': instantiation_cases, 'sizes': size_cases, 'row shards': shard_cases, 'large': large_cases}


def all_cases():
    return [c for sweep in SWEEPS.values() for c in sweep()]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points(regime, D, n):
    """float32 [n, D, D], symmetric bit for bit"""
    if n <= S.N_TOTAL:
        return S.points(regime, D)[:n].contiguous()
    assert regime == 'mid'
    rng = np.random.default_rng(_seed('spd det point', regime, n, D))
    s = rng.standard_normal((n, D, D))
    s = 0.5 * (s + np.swapaxes(s, -1, -2))
    s *= 1.5 / np.sqrt((s * s).sum((-2, -1), keepdims=True))
    w, v = np.linalg.eigh(s)
    t = torch.from_numpy(np.ascontiguousarray((v * np.exp(w)[:, None, :]) @ np.swapaxes(v, -1, -2))).float()
    return 0.5 * (t + t.transpose(-1, -2))


def _x64(regime, D, n):
    return points(regime, D, n).double().numpy()


def pairs_of(n, rows=None):
    """(i, j, lo, hi): the node pairs of the rows of the range in pair-vector order, and the range's slice of the pair vector"""
    i, j = np.triu_indices(n, 1)
    lo, hi = pair_slice(n, rows)
    return i[lo:hi], j[lo:hi], lo, hi


@functools.lru_cache(maxsize=None)
def d2_all(regime, D, n):
    i, j, _, _ = pairs_of(n)
    return ostep.pair_distances([('spd', D)], [_x64(regime, D, n)], pairs=(i, j))[0]


@functools.lru_cache(maxsize=None)
def _raw(regime, D, n):
    rng = np.random.default_rng(_seed('spd det raw', regime, D, n))
    k = n * (n - 1) // 2
    return rng.random(k) * 3.0 + 0.5, np.where(rng.random(k) < 0.5, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _targets(regime, D, n):
    md = ostep.softplus(SCALE_RAW) * d2_all(regime, D, n)
    tg = torch.from_numpy(_raw(regime, D, n)[0] * float(np.median(md))).float()
    moved = np.zeros(md.shape, dtype=bool)
    for _ in range(64):
        bad = ostep.kink_distance(S.LOSS['quotient'], tg.double().numpy(), md) < MARGIN
        if not bad.any():
            return tg, int(moved.sum())
        moved |= bad
        tg[torch.from_numpy(bad)] = tg[torch.from_numpy(bad)] * 1.01     # fp32 arithmetic: the value the kernels read
    raise AssertionError('the targets could not be nudged away from the kinks')


def targets(regime, D, n):
    """fp32 pair vector of all pairs (read-only)"""
    return _targets(regime, D, n)[0]


def nudged(regime, D, n):
    return _targets(regime, D, n)[1]


@functools.lru_cache(maxsize=None)
def upstream(regime, D, n):
    """fp32 pair vector of all pairs (read-only): random magnitudes, random signs"""
    u, sign = _raw(regime, D, n)
    return torch.from_numpy(u * sign).float()


def loaded(c):
    """what the kernel loads for the case's range: g (bwd kinds) or the targets (losses), fp32"""
    _, _, lo, hi = pairs_of(c.n, c.rows)
    full = targets(c.regime, c.D, c.n) if c.kind in LOSS_KINDS else upstream(c.regime, c.D, c.n)
    return full[lo:hi].contiguous()


def kink_margin(c):
    i, j, lo, hi = pairs_of(c.n, c.rows)
    md = ostep.softplus(SCALE_RAW) * d2_all(c.regime, c.D, c.n)[lo:hi]
    return float(ostep.kink_distance(S.LOSS['quotient'], loaded(c).double().numpy(), md).min()) if hi > lo else float('inf')


def n_pairs(c):
    lo, hi = pair_slice(c.n, c.rows)
    return hi - lo


# ---- the oracles -----------------------------------------------------------------------------------------------------------------
def _bwd_oracle(regime, D, n, squared, g, rows):
    _, _, lo, hi = pairs_of(n, rows)
    x = points(regime, D, n).double().requires_grad_()
    # (oracle.step.manifold: ref_port.SPD with LAPACK factorisations at every D — the reference's eps-fudged closed forms of
    # SPD(2), SPD(3) are off by 1e-7 of the gradient, which an fp64 kernel would be charged with)
    out = ostep.manifold(('spd', D)).pdist(x, squared=squared)[lo:hi]
    gx, = torch.autograd.grad((out * g.double()).sum(), x) if hi > lo else (torch.zeros_like(x), )
    return 0.5 * (gx + gx.transpose(1, 2))


def objective_of(c, vec):
    """the Oracle of the case with `vec` (fp32, the range's slice) as upstream gradient / targets"""
    i, j, lo, hi = pairs_of(c.n, c.rows)
    zero = torch.zeros(1, dtype=torch.float64)
    if c.kind in LOSS_KINDS:
        d2 = d2_all(c.regime, c.D, c.n)[lo:hi]
        tg = vec.double().numpy()
        value, grads, sgrads = ostep.objective([('spd', c.D)], [_x64(c.regime, c.D, c.n)], [SCALE_RAW], S.LOSS[c.kind], target=tg,
                                               pairs=(i, j), d2=[d2])
        _, slope = ostep.loss_and_slope(S.LOSS[c.kind], tg, ostep.softplus(SCALE_RAW) * d2)
        gx = torch.from_numpy(np.ascontiguousarray(grads[0]))
        scales = {'loss': abs(value), 'grad_x': float(gx.abs().max()) if gx.numel() else 0.0,
                  'grad_scale': ostep.sigmoid(SCALE_RAW) * float(np.abs(slope * d2).sum())}
        out = Oracle(torch.tensor([value], dtype=torch.float64), gx, torch.tensor([sgrads[0]], dtype=torch.float64), scales)
    else:
        gx = _bwd_oracle(c.regime, c.D, c.n, c.kind == 'bwd_sq', vec, c.rows)
        out = Oracle(zero, gx, zero, {'loss': 0.0, 'grad_x': float(gx.abs().max()), 'grad_scale': 0.0})
    assert out.grad_x.shape == (c.n, c.D, c.D) and bool(torch.isfinite(out.grad_x).all())
    return out


@functools.lru_cache(maxsize=None)
def oracle(c):
    """computed once per case, shared, never modified"""
    return objective_of(c, loaded(c))


def successors(c):
    """per pair of the range the value of its SUCCESSOR in the full pair vector (the last pair of all: its predecessor's; n = 2
    has one pair and no neighbour: 1.5 times its own value)"""
    _, _, lo, hi = pairs_of(c.n, c.rows)
    full = targets(c.regime, c.D, c.n) if c.kind in LOSS_KINDS else upstream(c.regime, c.D, c.n)
    nxt = torch.cat([full[1:], full[-2:-1]]) if full.numel() > 1 else full * 1.5
    return nxt[lo:hi].contiguous()


def median_pair(c):
    """position k (in the range's slice) of the pair with the median |value - successor's value|"""
    v, w = loaded(c).double().numpy(), successors(c).double().numpy()
    assert v.size >= 1
    return int(np.argsort(np.abs(v - w), kind='stable')[v.size // 2])


@functools.lru_cache(maxsize=None)
def one_pair_effect(c):
    """max |move of the oracle's grad_x| (absolute) when the pair median_pair(c) gets its successor's g / target.  The objective
    is a sum over the pairs: the move is the difference of that ONE pair's term under the two values."""
    i, j, lo, hi = pairs_of(c.n, c.rows)
    k = median_pair(c)
    a, b = float(loaded(c)[k]), float(successors(c)[k])
    x, pair = _x64(c.regime, c.D, c.n), (np.array([i[k]]), np.array([j[k]]))
    if c.kind in LOSS_KINDS:
        g = [ostep.objective([('spd', c.D)], [x], [SCALE_RAW], S.LOSS[c.kind], target=np.array([t]), pairs=pair)[1][0] for t in (a, b)]
        return float(np.abs(g[1] - g[0]).max())
    unit = exact.spd_pairs_grad(x, pair[0], pair[1], np.ones(1), squared=c.kind == 'bwd_sq', wmin=WMIN, wmax=WMAX)
    return float(np.abs(unit).max() * abs(b - a))


def one_pair_effect_literal(c):
    """the same move from the whole oracle, evaluated again with that one value replaced"""
    k = median_pair(c)
    other = loaded(c).clone()
    other[k] = successors(c)[k]
    return float((objective_of(c, other).grad_x - oracle(c).grad_x).abs().max())


# ---- the rule --------------------------------------------------------------------------------------------------------------------
RECORDS = []   # (sweep, dname, quantity, e_det / allowance, e_det / S, e_atomic / S, tag): printed last by the GPU test


def allowance(e_atomic, scale, dt):
    return 2 * e_atomic + 64 * eps_of(dt) * scale


def names_of(c):
    return NAMES if c.kind in LOSS_KINDS else ('grad_x', )


def hold(sweep, tag, dname, c, atomic, det, want, failures):
    """the rule for the quantities of one call: `atomic` and `det` are (loss [1], grad_x, grad_scale [1]) of the two modes, `want`
    the Oracle.  Prints every figure before it judges; returns the allowances."""
    granted = {}
    for k, name in enumerate(NAMES):
        if name not in names_of(c):
            continue
        scale = want.S[name]
        e_atomic, e_det = deviation(atomic[k], want[k]), deviation(det[k], want[k])
        allow = allowance(e_atomic, scale, DT[dname])
        line = f'{tag} {dname} {name}: e_det {e_det:.3e} e_atomic {e_atomic:.3e} allowance {allow:.3e} S {scale:.3e}'
        print(line)
        RECORDS.append((sweep, dname, name, e_det / max(allow, 1e-300), e_det / max(scale, 1e-300), e_atomic / max(scale, 1e-300), tag))
        if not e_det <= allow:
            failures.append(line)
        granted[name] = allow
    return granted
