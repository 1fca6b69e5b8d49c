"""Cases, inputs, expected values and the host model of the dispatch for the mixed-manifold pair kernels
(csrc/product_pairs.hip: every ordered pair; csrc/product_sym.hip: every unordered pair once) against the fp64 oracle
(tests/test_product_cases_host.py on the CPU, tests/test_product_oracle_gpu.py on the device).  Not a test module; plain
numpy / torch-CPU, no GPU needed.

The table is ENUMERATED from the dispatch, one case per instantiation of `product_pair_kernel<T, NV, SD, LOSS, PW, IDX, KC>`
and `product_sym_kernel<T, NV, SD, LOSS, KC>`, and built so that a kernel standing in for another cannot pass:
* every vector factor of a case has a width of its own and the raw scales are distinct, so no two factors are interchangeable;
* the SPD factor stands first, in the middle or last in the caller's list (the kernels take it out of the list: the vector
  factors keep their order, the loss slots keep the caller's positions);
* `route` says which instantiation a case takes under an environment, and the host test holds the set of all routes equal to
  the set of kernels in the built library (profiles/product_oracle.md has the table)."""
import functools
import itertools
import zlib

import numpy as np
import torch

import step_cases as sc
from oracle import step as ostep

KIND_CODE = {'euclidean': 0, 'lorentz': 1, 'sphere': 2}      # MM_EUCLIDEAN, MM_LORENTZ, MM_SPHERE (include/mm_manifolds.h)
LOSS_CODE = {'stress': 1, 'quotient': 2}                     # MM_LOSS_STRESS, MM_LOSS_QUOTIENT
CNAME = {'f32': 'float', 'f64': 'double'}
SYM_MIN_N = {'f32': 1536, 'f64': 640}                        # product_sym_applies: below, the ordered kernel (unless forced)
SYM_WIDTH = 8                                                # kPSW; a Euclidean factor keeps coordinate 7 for the constant 1
N, N_TABLE = 131, 200                                        # two full 64-column blocks + 3 columns; rows of a minibatch's tables
ALPHA = 1.25                                                 # (what step_cases.loss_of uses)

# the environments the device test runs under (the library reads each switch once per process)
ENVS = [{}, {'MM_PRODUCT_SYM': '1'}, {'MM_PRODUCT_RT_KINDS': '1'}, {'MM_PRODUCT_SYM': '1', 'MM_PRODUCT_RT_KINDS': '1'},
        {'MM_PRODUCT_TI': '16'}]
ENV_KEYS = ('MM_PRODUCT_SYM', 'MM_PRODUCT_ORDERED', 'MM_PRODUCT_RT_KINDS', 'MM_PRODUCT_PW16', 'MM_PRODUCT_TI')


def env_id(env):
    return '+'.join(f"{k[len('MM_PRODUCT_'):].lower()}{v}" for k, v in sorted(env.items())) or 'default'


# ---------------------------------------------------------------------------------------------------- the dispatch, on the host
def _on(env, key):
    return env.get(key, '')[:1] == '1'


def route(dtype, factors, n, loss, subset, env):
    """(form, T, NV, SD, LOSS, PW, IDX, KC) of the pair kernel that `mm_product_pairs_loss[_subset]` launches for these
    arguments under the environment `env` — product_pairs_t, product_pairs_launch, product_sym_applies,
    product_sym.hip::launch and for_kind_code restated.  `form` is 'pair' (ordered) or 'sym' (PW and IDX are None there).
    `loss` may carry the quotient's term selection ('quotient_l1'): the kernels read it at run time.
    (A row range without a pair launches no pair kernel at all; that is not modelled.)"""
    vec = [(k, d) for k, d in factors if k != 'spd']
    spd = [d for k, d in factors if k == 'spd']
    assert len(spd) <= 1 and len(vec) <= 3 and (vec or spd), factors
    assert all(1 <= d <= 16 for _, d in vec) and all(d in (2, 3) for d in spd), factors
    nv, sd = len(vec), (spd[0] if spd else 0)
    loss_code = LOSS_CODE[loss.split('_')[0]]
    code = 0
    for f, (k, _) in enumerate(vec):                 # two bits per vector factor, in list order, the SPD factor skipped
        code |= KIND_CODE[k] << (2 * f)
    rt = _on(env, 'MM_PRODUCT_RT_KINDS')
    sym = not _on(env, 'MM_PRODUCT_ORDERED') and not subset
    sym = sym and (_on(env, 'MM_PRODUCT_SYM') or n >= SYM_MIN_N[dtype])
    sym = sym and all(d <= (SYM_WIDTH - 1 if k == 'euclidean' else SYM_WIDTH) for k, d in vec)
    if sym:
        kc = code if nv in (1, 2) and not rt else -1
        return ('sym', CNAME[dtype], nv, sd, loss_code, None, None, kc)
    widest = max([d for _, d in vec], default=0)
    pw = 8 if widest <= 8 and not _on(env, 'MM_PRODUCT_PW16') else 16
    kc = code if pw == 8 and nv in (1, 2) and not rt else -1
    return ('pair', CNAME[dtype], nv, sd, loss_code, pw, bool(subset), kc)


def name(r):
    """The demangled kernel name as tools/kernel_meta.py reports it."""
    form, t, nv, sd, loss, pw, idx, kc = r
    if form == 'sym':
        return f'product_sym_kernel<{t}, {nv}, {sd}, {loss}, {kc}>'
    return f'product_pair_kernel<{t}, {nv}, {sd}, {loss}, {pw}, {"true" if idx else "false"}, {kc}>'


def route_of(c, env):
    return route(c['dname'], c['factors'], c['batch'] or c['n'], c['loss'], c['batch'] is not None, env)


# ------------------------------------------------------------------------------------------------------------------- the table
def _fid(factors):
    return 'x'.join(f"{'p' if k == 'spd' else k[0]}{d}" for k, d in factors)


def case(factors, dname, loss, epoch=0, n=N, rows=None, batch=None, init='perturb', tdraw=0, group=None, primary=False):
    """One call of mm_product_pairs_loss (rows: a row range of the pair list, None = all) or, with `batch`, of
    mm_product_pairs_loss_subset on `batch` nodes of tables of N_TABLE rows.  `loss`: 'stress', 'quotient' (both terms),
    'quotient_l1', 'quotient_l2'; `epoch` sets the quotient's eps = 1 / (epoch + 1).  `tdraw`: which draw of the targets."""
    factors = tuple((k, int(d)) for k, d in factors)
    cid = f"{_fid(factors)}-{dname}-{loss}{'' if loss == 'stress' else f'-e{epoch}'}-n{n}"
    cid += (f'-rows{rows[0]}_{rows[1]}' if rows else '') + (f'-b{batch}of{N_TABLE}' if batch else '')
    cid += ('-rand' if init == 'rand' else '') + (f'-t{tdraw}' if tdraw else '')
    nv = sum(1 for k, _ in factors if k != 'spd')
    sd = max([d for k, d in factors if k == 'spd'], default=0)
    return dict(id=cid, factors=factors, dname=dname, loss=loss, epoch=epoch, n=n, rows=rows, batch=batch, init=init, tdraw=tdraw,
                nv=nv, sd=sd, group=group, primary=primary)


# widths, by kind: index 0 is the widest the symmetric form takes
_WIDTHS = {'lorentz': [8, 3, 5, 6, 2, 4, 7], 'sphere': [8, 4, 6, 3, 5, 2, 7], 'euclidean': [7, 1, 5, 3, 6, 2, 4]}
_WIDE = [9, 16, 12, 11]          # first PW = 16, last supported, two in between
_NAMES = ('euclidean', 'lorentz', 'sphere')
_TRIPLES = {0: ('euclidean', 'lorentz', 'sphere'), 2: ('sphere', 'euclidean', 'lorentz'), 3: ('lorentz', 'sphere', 'euclidean')}
_TERMS = ('quotient', 'quotient_l1', 'quotient_l2')


def _layouts():
    """(group, vector kinds, SD): 'narrow' — every vector factor at most 8 wide (PW = 8 and the symmetric form: one layout per
    kind code of one and two vector factors, one per (3, SD) and (0, SD): those read the kinds at run time) — and 'wide' (one
    per (NV, SD): PW = 16 reads the kinds at run time too; the kinds rotate so that each is met at every NV)."""
    out = []
    for sd in (0, 2, 3):
        for nv in (0, 1, 2, 3):
            if nv == 0 and sd == 0:
                continue
            kinds = list(itertools.product(_NAMES, repeat=nv)) if nv < 3 else [_TRIPLES[sd]]
            out += [('narrow', k, sd) for k in kinds]
            if nv:
                r = (sd + nv) % 3
                out.append(('wide', tuple(_NAMES[(r + f) % 3] for f in range(nv)), sd))
    return out


def _factors(index, group, kinds, sd):
    """The factor list of layout `index`: distinct widths drawn from the kinds' pools (rotated by the layout's index, so that
    every pool entry is met), one factor above 8 in a wide layout, the SPD factor at position index % (NV + 1)."""
    used, vec = set(), []
    wide_at = index % len(kinds) if group == 'wide' and kinds else -1
    for f, k in enumerate(kinds):
        pool = _WIDE if f == wide_at else _WIDTHS[k]
        for t in range(len(pool)):
            w = pool[(index + f + t) % len(pool)]
            if w not in used:
                break
        else:
            raise AssertionError('no free width')
        used.add(w)
        vec.append((k, w))
    if sd:
        vec.insert(index % (len(kinds) + 1), ('spd', sd))
    return vec


def _build():
    cases, table = [], []
    seen_primary = set()
    layouts = _layouts()
    # Euclidean 8 fits PW = 8 and not the symmetric node table: under MM_PRODUCT_SYM=1 these fall to the ordered kernel
    extra = [('euclid8', (('euclidean', 8), ), None), ('euclid8', (('euclidean', 8), ('lorentz', 5), ('spd', 2)), None)]
    for index, (group, kinds, sd) in enumerate(layouts + extra):
        factors = list(kinds) if group == 'euclid8' else _factors(index, group, kinds, sd)
        nv = sum(1 for k, _ in factors if k != 'spd')
        sd = max([d for k, d in factors if k == 'spd'], default=0)
        primary = group == 'narrow' and (nv, sd) not in seen_primary
        seen_primary.add((nv, sd)) if primary else None
        quot, epoch, bs = _TERMS[index % 3], (0, 2)[index % 2], (131, 65)[index % 2]
        table.append(dict(index=index, group=group, factors=tuple(factors), nv=nv, sd=sd, primary=primary))
        for dname in ('f32', 'f64'):
            for loss, ep in (('stress', 0), (quot, epoch)):
                kw = dict(group=group, primary=primary)
                cases.append(case(factors, dname, loss, ep, **kw))
                cases.append(case(factors, dname, loss, ep, batch=bs, **kw))
                if not primary:
                    continue
                # the sizes: one pair; one live lane in the second column block; row shards and ranges of the pair list
                cases.append(case(factors, dname, loss, ep, n=2, **kw))
                cases.append(case(factors, dname, loss, ep, n=65, **kw))
                for rows in shards(N) + RANGES:
                    cases.append(case(factors, dname, loss, ep, rows=rows, **kw))
            if primary:      # the second call of the workspace contract: other targets
                loss, ep = (('stress', 0), (quot, epoch))[index % 2]
                cases.append(case(factors, dname, loss, ep, tdraw=1, **kw))
    # the reference's own initialisation (`rand`: all points within 0.01 ... 0.1 of the origin), once per family.  Lorentz and
    # sphere in fp64 only: at d ~ 0.01 the inner product is 1 +- 5e-5, of which fp32 holds 9 bits — acosh / acos of it is
    # wrong in the third digit in ANY fp32 evaluation, the reference's included, and no entry of the table is for that.
    for factor, dnames in ((('spd', 3), ('f32', 'f64')), (('euclidean', 5), ('f32', 'f64')), (('lorentz', 6), ('f64', )),
                           (('sphere', 4), ('f64', ))):
        for dname in dnames:
            cases.append(case([factor], dname, 'stress', init='rand', group='rand'))
            cases.append(case([factor], dname, 'quotient', 2, init='rand', group='rand'))
    return cases, table


RANGES = [(17, 90), (5, 5), (130, 131)]      # an inner range, an empty one, the last row (which holds no pair)


def shards(n, world=3):
    """The row ranges of the library's own sharding rule (mm_shard_rows, restated in graphembed._backend.shard_rows)."""
    from graphembed import _backend as B
    return [tuple(B.shard_rows(n, world, r)) for r in range(world)]


CASES, LAYOUTS = _build()
BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES), 'case ids are unique'


def cases_for(env):
    """What runs under an environment: everything, except under MM_PRODUCT_TI=16 (64-row workgroups with a 3-row tail; small
    launches otherwise only ever run ti = 4) one kind code per (NV, SD, dtype) at n = 131 on the ordered kernel."""
    if 'MM_PRODUCT_TI' in env:
        return [c for c in CASES if c['primary'] and c['n'] == N and c['rows'] is None and not c['tdraw']]
    return CASES


def whole_of(c):
    """The case over the full row range that a row-range case is a part of."""
    return BY_ID[case(c['factors'], c['dname'], c['loss'], c['epoch'])['id']]


# ------------------------------------------------------------------------------------------------------------------- inputs
# seeds redrawn because more than 1 % of the quotient targets sat within KINK_MARGIN of a kink: {targets key: bump}
REDRAWN = {}
MAX_MOVED_SHARE = 0.01


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2**31)


def loss_of(c):
    return sc.loss_of(c, c['epoch'])       # (stress; quotient with alpha = 1.25, eps = 1 / (epoch + 1), its l1 / l2 selection)


def terms_of(c):
    return {'stress': 3, 'quotient': 3, 'quotient_l1': 1, 'quotient_l2': 2}[c['loss']]


def scales_of(c):
    k = len(c['factors'])
    return [float(np.float32(v)) for v in ([0.5] if k == 1 else [0.5, 0.3, 0.7, 0.4][:k])]     # as step_cases.initial


@functools.lru_cache(maxsize=None)
def _points(factors, rows, dname, init):
    gen = torch.Generator().manual_seed(_seed('points', factors, rows, dname, init))
    return tuple(sc.points(f, rows, init, 0.3, gen, dname) for f in factors)


@functools.lru_cache(maxsize=None)
def _batch_idx(factors, dname, batch):
    gen = torch.Generator().manual_seed(_seed('idx', factors, dname, batch))
    return torch.randperm(N_TABLE, generator=gen)[:batch].numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def _d2(factors, rows, dname, init, batch):
    idx = None if batch is None else _batch_idx(factors, dname, batch)
    return tuple(ostep.pair_distances(list(factors), list(_points(factors, rows, dname, init)), idx))


@functools.lru_cache(maxsize=None)
def _targets(factors, n, dname, init, batch, tdraw, loss, epoch):
    """(pair vector | dense matrix, number of targets moved off a kink) — the recipe of step_cases.initial, then
    step_cases.settle_targets' rule on the host copy; the whole pair list of the n points, whatever rows a case takes."""
    key = ('targets', factors, n, dname, init, batch, tdraw)
    gen = torch.Generator().manual_seed(_seed(*key, REDRAWN.get(key, 0)))
    rows = N_TABLE if batch else n
    data = {}
    if batch is None:
        t = torch.rand(n * (n - 1) // 2, dtype=torch.float64, generator=gen) * 0.9 + 0.05
        data['target'] = sc._round(t.numpy(), dname)
    else:
        t = torch.triu(torch.rand(rows, rows, dtype=torch.float64, generator=gen) * 0.9 + 0.05, 1)
        data['dense'] = sc._round((t + t.T).numpy(), dname)
        data['batches'] = {epoch: _batch_idx(factors, dname, batch)}
    c = dict(n=rows, dname=dname, loss=loss, batch=batch)
    state = dict(scales=scales_of(dict(factors=factors)))
    moved = sc.settle_targets(c, state, data, epoch, _d2(factors, rows, dname, init, batch))
    out = data['dense'] if batch else data['target']
    out.setflags(write=False)
    return out, moved


def pair_slice(c):
    """[lo, hi) of the case's rows in the pair vector of its n points."""
    rb, re = c['rows'] or (0, c['n'])
    off = lambda r: r * (2 * c['n'] - r - 1) // 2       # noqa: E731  (mm_pair_offset)
    return off(rb), off(re)


def inputs(c):
    """dict(xs, scales, idx, target (the rows' slice of the pair vector) | dense, moved, pairs (i, j node ids))"""
    f, batch = c['factors'], c['batch']
    rows = N_TABLE if batch else c['n']
    xs = _points(f, rows, c['dname'], c['init'])
    t, moved = _targets(f, c['n'], c['dname'], c['init'], batch, c['tdraw'], c['loss'], c['epoch'])
    out = dict(xs=xs, scales=scales_of(c), moved=moved, idx=None, target=None, dense=None)
    if batch:
        out['idx'], out['dense'] = _batch_idx(f, c['dname'], batch), t
        out['pairs'] = ostep.pair_list(rows, out['idx'])
        out['npairs_whole'] = out['pairs'][0].size
    else:
        lo, hi = pair_slice(c)
        i, j = ostep.pair_list(c['n'])
        out['target'], out['pairs'] = t[lo:hi], (i[lo:hi], j[lo:hi])
        out['npairs_whole'] = i.size
    return out


@functools.lru_cache(maxsize=None)
def _expected(cid):
    c = BY_ID[cid]
    inp = inputs(c)
    rows = N_TABLE if c['batch'] else c['n']
    d2 = _d2(c['factors'], rows, c['dname'], c['init'], c['batch'])
    if c['batch']:
        return ostep.objective(list(c['factors']), list(inp['xs']), inp['scales'], loss_of(c), dense=inp['dense'], idx=inp['idx'],
                               d2=list(d2))
    lo, hi = pair_slice(c)
    return ostep.objective(list(c['factors']), list(inp['xs']), inp['scales'], loss_of(c), target=inp['target'],
                           pairs=inp['pairs'], d2=[d[lo:hi] for d in d2])


def expected(c):
    """(loss, [gradient per factor, full-size: zero rows outside a minibatch], [d loss / d raw scale]) from oracle.step.objective
    on the case's own pair list."""
    return _expected(c['id'])


def shares(c):
    """Per factor: (its share of the weighted distance sum md, its share of sum |d loss / d md| softplus(s) d2 — the weights
    every gradient of the call is made of), summed over the case's pairs."""
    inp = inputs(c)
    rows = N_TABLE if c['batch'] else c['n']
    lo, hi = (0, None) if c['batch'] else pair_slice(c)
    d2 = [d[lo:hi] for d in _d2(c['factors'], rows, c['dname'], c['init'], c['batch'])]
    parts = [ostep.softplus(s) * d for s, d in zip(inp['scales'], d2)]
    md = sum(parts)
    i, j = inp['pairs']
    gd = ostep.pair_targets(inp['target'], inp['dense'], i, j)
    _, slope = ostep.loss_and_slope(loss_of(c), gd, md)
    return [(float(p.sum() / md.sum()), float((np.abs(slope) * p).sum() / (np.abs(slope) * md).sum())) for p in parts]


def kink_distances(c):
    inp = inputs(c)
    rows = N_TABLE if c['batch'] else c['n']
    lo, hi = (0, None) if c['batch'] else pair_slice(c)
    d2 = [d[lo:hi] for d in _d2(c['factors'], rows, c['dname'], c['init'], c['batch'])]
    md = sum(ostep.softplus(s) * d for s, d in zip(inp['scales'], d2))
    i, j = inp['pairs']
    return ostep.kink_distance(loss_of(c), ostep.pair_targets(inp['target'], inp['dense'], i, j), md)


# --------------------------------------------------------------------------------------------------------------- comparison
TOL = sc.TOL        # the project's table, imported — not restated

# per-case bounds above the table, from the rule of profiles/product_oracle.md: {case id: {quantity: bound}} — max(table,
# 2 x the error of oracle/ref_port.py in float32 on the CPU on the same inputs against the same oracle)
PORT_BOUND = {}


def errors(c, want, got):
    """{quantity: (error, allowed)} of (loss, grads, scale_grads) against the oracle's, in the units of the table."""
    dn = c['dname']
    lref, gref, sref = want
    loss, grads, sgrads = got
    extra = PORT_BOUND.get(c['id'], {})
    out = {'loss': (abs(loss - lref), max(TOL['loss'][dn], extra.get('loss', 0.0)) * abs(lref))}
    for k, (f, g, w) in enumerate(zip(c['factors'], grads, gref)):
        key, q = ('grad_spd' if f[0] == 'spd' else 'grad_vec'), f'grad/{k}:{f[0]}{f[1]}'
        g = np.asarray(g, np.float64)
        assert g.shape == w.shape, (g.shape, w.shape)
        err = np.abs(g - w).max() if np.isfinite(g).all() else float('inf')       # (an unwritten row is NaN)
        out[q] = (err, max(TOL[key][dn], extra.get(q, 0.0)) * np.abs(w).max())
        q = f'scale_grad/{k}:{f[0]}{f[1]}'
        out[q] = (abs(sgrads[k] - sref[k]) if np.isfinite(sgrads[k]) else float('inf'),
                  max(TOL['scale_grad'][dn], extra.get(q, 0.0)) * max(abs(sref[k]), 1e-3 * abs(lref)))
    if not np.isfinite(loss):
        out['loss'] = (float('inf'), out['loss'][1])
    return out


worst = sc.worst


def swapped_kinds(c):
    """The case's factor list with the KINDS of its two vector factors exchanged (widths and points stay): what a kernel with
    a transposed kind code computes."""
    vec = [k for k, (kind, _) in enumerate(c['factors']) if kind != 'spd']
    assert len(vec) == 2
    f = list(c['factors'])
    a, b = vec
    f[a], f[b] = (c['factors'][b][0], f[a][1]), (c['factors'][a][0], f[b][1])
    return f
