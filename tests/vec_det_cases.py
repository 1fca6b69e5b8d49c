"""Cases, inputs, fp64 oracles and the rules of the bit-deterministic vector pair kernels (csrc/vec_det.hpp: vec_det::pair_kernel
<T, KIND, MP, LOSS, SUB> and vec_det::finalize_kernel<T, KIND, MP>, reached through mm_vec_pdist_bwd_det / mm_vec_pdist_loss_det /
mm_vec_pdist_loss_subset_det).  Host code only; nothing here runs a kernel.  tests/test_vec_det_host.py walks everything below on
the CPU, tests/test_vec_det_gpu.py makes the calls.

Cases are vec_cases.case(...) dicts, inputs vec_cases.inputs, oracle values vec_cases.evaluate (oracle/exact.c, fp64), bounds
vec_cases.errors (GREL, TOL, RAISED by case id): the ordered atomic twin is held to these bounds on these inputs under
MM_VEC_BWD_ORDERED=1, and the new kernel shares its per-pair arithmetic — no new tolerance.  Next to them the rule of
spd_det_cases:  e_det <= 2 e_atomic + 64 eps(dtype) S,  e_atomic the deviation FROM THE SAME ORACLE of the default atomic entry on
the same GPU in the same test,  S: loss |W|; grad_x max|W|; grad_scale sigmoid(s) sum |slope d2|.

    instantiations  n = 131: every width of vec_cases.WIDTHS x 3 kinds x {f32, f64} x {bwd squared, bwd plain, stress, one of
                    the quotient's three term selections (vec_cases' rotation)}, scale SCALE_RAW; at the PRIMARY widths also
                    the two losses without a scale
    sizes           PRIMARY widths, the 4 calls, both dtypes: n = 2, 3, K R = 64 (AT a chunk boundary), K R + 1 = 65 (a ragged
                    last chunk of one row), 257 (one column past a 256-column workgroup); R = ROWS_PER_CHUNK = 8 is what
                    mm_vec_pdist_det_geometry answers there (asserted by the host test)
    shards          n = 131, PRIMARY widths: vec_cases.RANGES (row_begin on no boundary; an empty range; the last row, which
                    holds no pair) and vec_cases.shards(131), which add up to the whole
    minibatches     batches 2, 17, 70 of the N_TABLE-node table (unsorted indices), every kind, widths 3, 11, 24, 64, both
                    losses, both dtypes; one batch with an ASYMMETRIC dense matrix (`asym`: its lower triangle x ASYM — the kernel
                    must read dense[idx[a]][idx[b]], a < b by position, not its transpose); one row shard of a batch (`brows`)
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_cases as sc  # noqa: E402
import vec_cases as vc  # noqa: E402
from grass_cases import CallSpy  # noqa: E402,F401
from oracle import step as ostep  # noqa: E402

DNAMES = ('f32', 'f64')
EPS = {'f32': float(np.finfo(np.float32).eps), 'f64': float(np.finfo(np.float64).eps)}
ROWS_PER_CHUNK = 8
K_CHUNKS = 8
SIZES = (2, 3, K_CHUNKS * ROWS_PER_CHUNK, K_CHUNKS * ROWS_PER_CHUNK + 1, 257)
SUB_WIDTHS = (3, 11, 24, 64)
ASYM = 1.3                     # the lower triangle of the asymmetric dense matrix is this multiple of the upper one
ASYM_CASE = ('lorentz', 11, 17)
BROWS_CASE = ('lorentz', 11, 70, (23, 51))
QUANTITIES = ('loss', 'grad', 'scale_grad')


def _widths(kind):
    return [m for m in vc.WIDTHS if m >= (1 if kind == 'euclidean' else 2)]


def instantiation_cases():
    out = []
    for dname in DNAMES:
        for ki, kind in enumerate(vc.KINDS):
            for index, m in enumerate(_widths(kind)):
                for entry in ('bwd', 'loss'):
                    for sq, loss in vc._variants(entry, index + ki):
                        out.append(vc.case(entry, kind, m, dname, sq, loss))
            for sq, loss in vc._variants('loss'):
                out.append(vc.case('loss', kind, vc.PRIMARY[kind], dname, sq, loss, scale=False))
    return out


def size_cases():
    return [vc.case(entry, kind, vc.PRIMARY[kind], dname, sq, loss, n=n)
            for dname in DNAMES for kind in vc.KINDS for entry in ('bwd', 'loss') for sq, loss in vc._variants(entry) for n in SIZES]


def shard_ranges():
    return list(vc.RANGES) + list(vc.shards(vc.N))


def shard_cases():
    return [vc.case(entry, kind, vc.PRIMARY[kind], dname, sq, loss, rows=rows)
            for dname in DNAMES for kind in vc.KINDS for entry in ('bwd', 'loss') for sq, loss in vc._variants(entry)
            for rows in [None] + shard_ranges()]      # (None: the whole the shards add up to)


def whole_of(c):
    return vc.case(c['entry'], c['kind'], c['m'], c['dname'], c['squared'], c['loss'], n=c['n'])


def minibatch_cases():
    out = []
    for dname in DNAMES:
        for kind in vc.KINDS:
            for m in SUB_WIDTHS:
                for sq, loss in vc._variants('subset'):
                    for b in vc.BATCHES:
                        out.append(vc.case('subset', kind, m, dname, sq, loss, batch=b))
        kind, m, b = ASYM_CASE
        for sq, loss in vc._variants('subset'):
            c = vc.case('subset', kind, m, dname, sq, loss, batch=b)
            out.append(dict(c, id=c['id'] + '-asym', asym=True))
        kind, m, b, rows = BROWS_CASE
        for sq, loss in vc._variants('subset'):
            c = vc.case('subset', kind, m, dname, sq, loss, batch=b)
            out.append(dict(c, id=c['id'] + f'-brows{rows[0]}_{rows[1]}', brows=rows))
    return out


SWEEPS = {'instantiations': instantiation_cases, 'sizes': size_cases, 'shards': shard_cases, 'minibatches': minibatch_cases}


@functools.lru_cache(maxsize=None)
def _all():
    seen, out = set(), []
    for name, sweep in SWEEPS.items():
        for c in sweep():
            if c['id'] not in seen:
                seen.add(c['id'])
                out.append(c)
    return tuple(out)


def all_cases():
    return list(_all())


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _asym_dense(kind, m, n, dname, batch, loss, epoch, scale):
    dense = np.array(vc._targets(kind, m, n, dname, batch, loss, epoch, scale)[0])
    low = np.tril_indices(dense.shape[0], -1)
    dense[low] = sc._round(dense[low] * ASYM, dname)
    dense.setflags(write=False)
    return dense


def batch_slice(c):
    """[lo, hi) of the batch's pair list that the case's row range of the BATCH owns"""
    b = c['batch']
    rb, re = c.get('brows') or (0, b)
    off = lambda r: r * (2 * b - r - 1) // 2       # noqa: E731  (mm_pair_offset)
    return off(rb), off(re)


# Targets redrawn, {case id: bump}: whole-range loss cases of one-coordinate manifolds in which the pair `one_pair_effect` replaces
# moved the oracle's gradient by less than twice the fp32 allowance (0.98 x and 1.6 x with vec_cases' targets).  The recipe is
# vec_cases._targets' (uniform [0.05, 0.95), rounded to the dtype, step_cases.settle_targets); only the seed differs.
# Sphere(2): the first bump gives 5.8 x.  Euclidean(1) is weak by construction, not by the draw: an end point of the line adds 130
# stress terms of one sign, so max|grad| is 3527 and 3e-4 of it is what ONE typical pair contributes — bumps 1 .. 7 give 0.15,
# 0.50, 0.29, 0.01, 2.09, 1.58, 0.58 x, and 5 is taken.  In that one fp32 case the bound can hide a typical single pair; its
# fp64 twin (ratio 3e5) and the e_det rule (64 eps S is 400 times tighter there) cannot.
REDRAWN = {'loss-euclidean1-f32-stress-n131': 5, 'loss-sphere2-f32-quotient_l2-n131': 1}


@functools.lru_cache(maxsize=None)
def _redrawn_targets(cid):
    import torch
    c = BY_ID[cid]
    assert c['entry'] == 'loss' and c['rows'] is None and not c['batch']
    inp = vc.inputs(c)
    gen = torch.Generator().manual_seed(vc._seed('vec det targets', cid, REDRAWN[cid]))
    data = {'target': sc._round((torch.rand(inp['d2'].size, dtype=torch.float64, generator=gen) * 0.9 + 0.05).numpy(), c['dname'])}
    sc.settle_targets(dict(n=c['n'], dname=c['dname'], loss=c['loss'], batch=None), dict(scales=[inp['scale']]), data, c['epoch'], [inp['d2']])
    data['target'].setflags(write=False)
    return data['target']


def inputs(c):
    """vec_cases.inputs, with the asymmetric dense matrix / the batch's row range / a redrawn target vector applied"""
    inp = dict(vc.inputs(c))
    if c['id'] in REDRAWN:
        inp['target'] = _redrawn_targets(c['id'])
    if c.get('asym'):
        inp['dense'] = _asym_dense(c['kind'], c['m'], c['n'], c['dname'], c['batch'], c['loss'], c['epoch'], inp['scale'])
    if c.get('brows'):
        lo, hi = batch_slice(c)
        inp['pairs'] = (inp['pairs'][0][lo:hi], inp['pairs'][1][lo:hi])
        inp['d2'] = inp['d2'][lo:hi]
    return inp


def n_pairs(c):
    return int(inputs(c)['pairs'][0].size)


def call_rows(c):
    """(n of the launch, row_begin, row_end) of the C call"""
    n = c['batch'] or c['n']
    rb, re = c.get('brows') or c['rows'] or (0, n)
    return n, rb, re


def loaded(c):
    """per pair of the case what the kernel loads: the upstream gradient (bwd) or the target (loss, subset), fp64"""
    inp = inputs(c)
    if c['entry'] == 'bwd':
        return np.asarray(inp['g'], dtype=np.float64)
    i, j = inp['pairs']
    return ostep.pair_targets(inp['target'], inp['dense'], i, j)


def kink_margin(c):
    if not c['loss'] or not n_pairs(c):
        return float('inf')
    inp = inputs(c)
    md = ostep.softplus(inp['scale']) * inp['d2']
    return float(ostep.kink_distance(vc.loss_of(c), loaded(c), md).min())


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def _weights(c, g, d2):
    return g if c['squared'] else np.where(g != 0, g / (2.0 * np.sqrt(np.where(d2 > 0, d2, 1.0))), 0.0)


def evaluate(c, values=None):
    """(want, S): `want` as vec_cases.evaluate returns it — the gradient [n, m] (bwd) or (loss, gradient, d loss / d raw scale) —
    and the scales S of the e_det rule per quantity.  `values` replaces what `loaded` returns (the one-pair teeth)."""
    inp = inputs(c)
    factor = (c['kind'], c['m'])
    i, j = inp['pairs']
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    vals = loaded(c) if values is None else values
    if c['entry'] == 'bwd':
        grad = ostep._d2_and_grad(factor, inp['x'], lo, hi, _weights(c, vals, inp['d2']))
        return grad, {'grad': float(np.abs(grad).max()) if grad.size else 0.0}
    spec = vc.loss_of(c)
    value, grads, sgrads = ostep.objective([factor], [inp['x']], [inp['scale']], spec, target=vals, pairs=(i, j), d2=[inp['d2']])
    _, slope = ostep.loss_and_slope(spec, vals, ostep.softplus(inp['scale']) * inp['d2'])
    scales = {'loss': abs(value), 'grad': float(np.abs(grads[0]).max()), 'scale_grad': ostep.sigmoid(inp['scale']) * float(np.abs(slope * inp['d2']).sum())}
    return (value, grads[0], sgrads[0]), scales


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    return evaluate(BY_ID[cid])


def oracle(c):
    """computed once per case, shared, never modified"""
    return _oracle(c['id'])


BY_ID = {c['id']: c for c in _all()}


def grad_of(want):
    return want[1] if isinstance(want, tuple) else want


def grad_allowance(c):
    """what vec_cases.errors grants the gradient of the case"""
    want = oracle(c)[0]
    got = want if c['entry'] == 'bwd' else (want[0], want[1], want[2] if c['scale'] else 0.0)
    return vc.errors(c, want, got)['grad'][1]


def one_pair_effect(c):
    """max |move of the oracle's grad_x| when ONE pair — the one with the median |value - successor's value| — gets its
    SUCCESSOR's upstream gradient / target (the last pair: its predecessor's; a single pair: 1.5 times its own).  The objective is
    a sum over the pairs: the move is the difference of that ONE pair's term under the two values."""
    inp = inputs(c)
    v = loaded(c)
    assert v.size >= 1
    nxt = np.concatenate([v[1:], v[-2:-1]]) if v.size > 1 else v * 1.5
    k = int(np.argsort(np.abs(v - nxt), kind='stable')[v.size // 2])
    i, j = inp['pairs'][0][k:k + 1], inp['pairs'][1][k:k + 1]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    factor, d2 = (c['kind'], c['m']), inp['d2'][k:k + 1]
    if c['entry'] == 'bwd':
        dw = _weights(c, nxt[k:k + 1], d2) - _weights(c, v[k:k + 1], d2)
        return float(np.abs(ostep._d2_and_grad(factor, inp['x'], lo, hi, dw)).max())
    g = [ostep.objective([factor], [inp['x']], [inp['scale']], vc.loss_of(c), target=t, pairs=(i, j), d2=[d2])[1][0]
         for t in (v[k:k + 1], nxt[k:k + 1])]
    return float(np.abs(g[1] - g[0]).max())


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
RECORDS = []   # (sweep, dname, quantity, e_det / bound, e_det / allowance, e_det / S, e_atomic / S, id): printed last by the GPU test


def _deviations(c, want, got):
    """{quantity: |got - want| (max over a tensor)}"""
    if c['entry'] == 'bwd':
        return {'grad': float(np.abs(np.asarray(got, np.float64) - want).max()) if want.size else 0.0}
    out = {'loss': abs(got[0] - want[0]), 'grad': float(np.abs(np.asarray(got[1], np.float64) - want[1]).max())}
    if c['scale']:
        out['scale_grad'] = abs(got[2] - want[2])
    return out


def hold(sweep, c, atomic, det, failures):
    """Both rules for one call: `det` and `atomic` as vec_cases.evaluate returns a result (atomic may be None: vec_cases.errors
    alone).  Prints every figure before it judges."""
    want, S = oracle(c)
    errs = vc.errors(c, want, det)
    e_det = _deviations(c, want, det)
    e_atomic = _deviations(c, want, atomic) if atomic is not None else None
    for q, (err, allowed) in errs.items():
        line = f"{c['id']} {q}: error {err:.3e} bound {allowed:.3e}"
        ratio2 = 0.0
        if e_atomic is not None and q in e_det:
            allow = 2 * e_atomic[q] + 64 * EPS[c['dname']] * S[q]
            line += f' | e_det {e_det[q]:.3e} e_atomic {e_atomic[q]:.3e} allowance {allow:.3e} S {S[q]:.3e}'
            ratio2 = e_det[q] / max(allow, 1e-300)
            if not e_det[q] <= allow:
                failures.append(line + ': e_det > 2 e_atomic + 64 eps S')
        print(line)
        if not err <= allowed:
            failures.append(line + ': above the bound of vec_cases.errors')
        RECORDS.append((sweep, c['dname'], q, err / allowed if allowed > 0 else (0.0 if err == 0 else float('inf')), ratio2,
                        e_det.get(q, 0.0) / max(S.get(q, 0.0), 1e-300),
                        (e_atomic or {}).get(q, 0.0) / max(S.get(q, 0.0), 1e-300), c['id']))
