"""Cases, inputs, expected values and the host model of the dispatch for the vector-manifold pair kernels (Euclidean, Lorentz,
sphere: csrc/vec.hip — forward, ordered backward, node minibatches, finalize; csrc/vec_sym.hip / vec_sym.hpp — every unordered
pair once; csrc/vec_gram.hip / vec_gram_bwd64.hpp — the matrix cores) against the fp64 oracle (tests/test_vec_cases_host.py on
the CPU, tests/test_vec_oracle_gpu.py on the device).  Not a test module; plain numpy / torch-CPU, no GPU needed.

The table is ENUMERATED from the dispatch: every padded width class MP and every matrix-core k-step class KS is met at both
of its ends (full, and one past the previous class), for every kind, dtype, loss kind and `squared` the entry instantiates,
at n = 131 (a ragged last 64-row tile, dead lanes in the 256-wide column block, a tail of the 8-row unroll, a partial last
32- / 16-tile and two super-tiles per side on the matrix cores).  `route` says which instantiations a call launches under an
environment; the host test holds the set of all routes equal to the set of kernels in the built library
(profiles/vec_oracle.md has the table)."""
import functools
import zlib

import numpy as np
import torch

import step_cases as sc
from oracle import ref_port as rp
from oracle import step as ostep

KINDS = ('euclidean', 'lorentz', 'sphere')
KIND_CODE = {'euclidean': 0, 'lorentz': 1, 'sphere': 2}      # MM_EUCLIDEAN, MM_LORENTZ, MM_SPHERE (include/mm_manifolds.h)
LOSS_CODE = {None: 0, 'stress': 1, 'quotient': 2}            # MM_LOSS_NONE, MM_LOSS_STRESS, MM_LOSS_QUOTIENT
CNAME = {'f32': 'float', 'f64': 'double'}
ENTRIES = ('fwd', 'fwd_gram', 'bwd', 'bwd_gram', 'loss', 'subset')      # mm_vec_pdist_<entry> (subset: mm_vec_pdist_loss_subset)
N, N_TABLE = 131, 200
EPOCH, ALPHA = 2, 1.25                                       # the quotient's eps = 1 / (EPOCH + 1); alpha as step_cases.loss_of
SCALE_RAW = 0.5                                              # the trainable scale; softplus applied by the kernels
NO_SCALE_RAW = float(np.log(np.e - 1.0))                     # scale_raw = NULL means a factor of 1 = softplus(log(e - 1))
MAX_DIM = 64                                                 # kVecMaxDim
GRAM_MAX_N = 32768                                           # vec_gram_supports
SYM_MAX_N = 1 << 22                                          # kSpdMaxNodes
SUB_MAX_ROWS = 64                                            # kVecSubMaxRows
NEAR = 0.1                                                   # fp32 plain backward: pairs closer than this get zero upstream weight
MAX_MASKED_SHARE = 0.10

# every MP class (4 8 12 16 24 32 48 64) at both ends; 3 is the low end of the fp32 matrix cores' first class
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64)
PRIMARY = {'lorentz': 11, 'sphere': 6, 'euclidean': 10}      # the width per kind that runs the sizes beyond n = 131
SIZES = (2, 65, 257)
RANGES = [(37, 90), (5, 5), (130, 131)]      # row_begin on no tile boundary; an empty range; the last row (which holds no pair)
BATCHES = (2, 17, 70)                        # one pair; a 16-row group plus one row; more rows than kVecSubMaxRows
FWD_HEIGHT_N = (1025, 1537, 2049, 3100)      # vec_fwd_t reaches 4, 8, 16, 32 rows per tile there on 256 CUs

# the environments the device test runs under (the library reads each switch once per process).  The two pairs: the ordered
# VALU kernel with a fused loss at fp32 Lorentz / sphere 17 <= m <= 32 is behind the matrix cores AND the symmetric form, and
# the ordered matrix-core kernel with a fused loss at m <= 16 is behind the VALU default AND the symmetric tiles.
ENVS = [{}, {'MM_VEC_BWD_ORDERED': '1'}, {'MM_VEC_LOSS_GRAM': '1'}, {'MM_VEC_LOSS_VALU': '1'}, {'MM_GRAM_BWD_ORDERED': '1'},
        {'MM_GRAM_BWD_ORDERED': '0'}, {'MM_GRAM_BWD_PARTS': '2'}, {'MM_GRAM_BWD_PARTS': '1'}, {'MM_VEC_SUBSET_ROWS': '64'},
        {'MM_VEC_BWD_ORDERED': '1', 'MM_VEC_LOSS_VALU': '1'}, {'MM_VEC_LOSS_GRAM': '1', 'MM_GRAM_BWD_ORDERED': '1'}]
ENV_KEYS = ('MM_VEC_BWD_ORDERED', 'MM_VEC_LOSS_GRAM', 'MM_VEC_LOSS_VALU', 'MM_GRAM_BWD_ORDERED', 'MM_GRAM_BWD_PARTS',
            'MM_VEC_SUBSET_ROWS', 'MM_GRAM_BWD_TPW', 'MM_VEC_BWD_GRID', 'MM_VEC_BWD_CROSS')


def env_id(env):
    return '+'.join(f"{k[len('MM_'):].lower()}{v}" for k, v in sorted(env.items())) or 'default'


# ---------------------------------------------------------------------------------------------------- the dispatch, on the host
def _on(env, key):
    return env.get(key, '')[:1] == '1'


def pad_dim(m):
    """vecfn.hpp"""
    return next(p for p in (4, 8, 12, 16, 24, 32, 48, 64) if m <= p or p == 64)


def ks32(m):
    """k-steps of v_mfma_f32_32x32x2_f32: ceil(m / 2) rounded up to a dispatch class (an odd m zero-pads half a step)"""
    return next(k for k in (2, 4, 6, 8, 12, 16) if (m + 1) // 2 <= k or k == 16)


def ks64(m):
    """k-steps of v_mfma_f64_16x16x4_f64: ceil(m / 4), 1 .. 4"""
    return min((m + 3) // 4, 4)


def sym_supports(dname, kind, m):
    """vec_sym_supports"""
    return 1 <= m <= (32 if dname == 'f32' or kind == 'euclidean' else 16)


def gram_supports(dname, kind, n, m):
    """vec_gram_supports"""
    return kind in ('lorentz', 'sphere') and n <= GRAM_MAX_N and m <= (32 if dname == 'f32' else 16)


def gram_bwd_supports(dname, kind, n, m, squared):
    """vec_gram_bwd_supports: also the fp32 squared Euclidean distance (one spare column for the row sums: m <= 31)"""
    return gram_supports(dname, kind, n, m) or (dname == 'f32' and kind == 'euclidean' and bool(squared) and m <= 31 and n <= GRAM_MAX_N)


def refused(entry, dname, kind, m, n, squared=True):
    """Whether the entry answers MM_ERR_UNSUPPORTED before anything is launched."""
    if entry == 'fwd_gram':
        return kind == 'euclidean' or n > GRAM_MAX_N or (dname == 'f32' and m > 32)
    if entry == 'bwd_gram':
        return not gram_bwd_supports(dname, kind, n, m, squared)
    return m > MAX_DIM


def _gram_bwd_name(dname, kind, m, loss_code, env):
    k = KIND_CODE[kind]
    if dname == 'f64':
        return f'vec_gram_bwd_f64_kernel<{k}, {ks64(m)}, {loss_code}>'
    forced = env.get('MM_GRAM_BWD_ORDERED')
    ordered = (forced[:1] == '1') if forced is not None else kind == 'euclidean'
    ks = 2 if kind == 'euclidean' else ks32(m)      # (the squared Euclidean distance has no Gram: one instantiation)
    return f"vec_gram_bwd_{'' if ordered else 'sym_'}f32_kernel<{k}, {ks}, {loss_code}>"


def route(entry, dname, kind, m, n, loss, squared, batch, env):
    """The pair-kernel instantiations (with the preparation / finalize kernel of the form) one call of mm_vec_pdist_<entry>
    launches for these arguments under the environment `env`, spelled as tools/kernel_meta.kernels() demangles them —
    mm_vec_pdist_fwd / vec_fwd_t, mm_vec_pdist_fwd_gram, vec_bwd_t, vec_sym.hip::pairs_mp, vec_gram_bwd_launch,
    mm_vec_pdist_loss and vec_loss_subset_t restated.  `n`: the points of the launch (a minibatch: its size).  `loss` may carry
    the quotient's term selection ('quotient_l1'): the kernels read it at run time.  [] for a refusal.  (A row range without a
    pair launches only the preparation / finalize kernel; that is not modelled.)"""
    assert entry in ENTRIES and kind in KINDS and m >= 1, (entry, kind, m)
    if refused(entry, dname, kind, m, n, squared):
        return []
    t, k, mp = CNAME[dname], KIND_CODE[kind], pad_dim(m)
    code = LOSS_CODE[loss.split('_')[0] if loss else None]
    sq = 'true' if squared or code else 'false'
    finalize = f'vec_pdist_finalize_kernel<{t}, {k}, {mp}>'
    if entry == 'fwd':
        return [f'vec_pdist_fwd_kernel<{t}, {k}, {mp}>']
    if entry == 'fwd_gram':
        return [f'vec_gram_fwd_f32_kernel<{k}, {ks32(m)}>' if dname == 'f32' else f'vec_gram_fwd_f64_kernel<{k}>']
    if entry == 'bwd_gram':
        return [_gram_bwd_name(dname, kind, m, 0, env)]
    if entry == 'subset':
        return [f'vec_pdist_bwd_kernel<{t}, {k}, {mp}, 8, {code}, true>', finalize]
    if entry == 'loss':
        assert code, loss
        force_gram, force_valu = _on(env, 'MM_VEC_LOSS_GRAM'), _on(env, 'MM_VEC_LOSS_VALU')
        if gram_supports(dname, kind, n, m) and not force_valu and (force_gram or (dname == 'f32' and m > 16)):
            return [_gram_bwd_name(dname, kind, m, code, env)]
    if not _on(env, 'MM_VEC_BWD_ORDERED') and sym_supports(dname, kind, m) and n <= SYM_MAX_N:
        return [f'vec_sym_prep_kernel<{t}, {mp}>', f'vec_pdist_bwd_sym_kernel<{t}, {k}, {mp}, {code}, {sq}>']
    return [f'vec_pdist_bwd_kernel<{t}, {k}, {mp}, 64, {code}, false>', finalize]


def fwd_tile_height(n, rb, re, cus):
    """Rows per tile of vec_pdist_fwd_kernel, a launch argument (vec_fwd_t): 32, halved while the launch has fewer than four
    workgroups per CU, down to 2.  None when nothing is launched."""
    gx = (n + 255) // 256 - (rb + 1) // 256
    if re <= rb or gx <= 0:
        return None
    ti = 32
    while ti > 2 and gx * ((re - rb + ti - 1) // ti) < 4 * cus:
        ti //= 2
    return ti


def subset_rows(env):
    """Rows per workgroup of the minibatch launch (vec_loss_subset_t)."""
    v = int(env.get('MM_VEC_SUBSET_ROWS', 0) or 0)
    return min(SUB_MAX_ROWS, (v + 7) // 8 * 8 if v > 0 else 16)


def route_of(c, env):
    return route(c['entry'], c['dname'], c['kind'], c['m'], c['batch'] or c['n'], c['loss'], c['squared'], c['batch'], env)


def form_of(names):
    """'fwd' | 'fwd_gram' | 'sym' | 'ordered' | 'subset' | 'gram_sym' | 'gram_ordered' | 'gram_f64' | 'refused'"""
    if not names:
        return 'refused'
    nm = names[-1] if names[0].startswith('vec_sym_prep') else names[0]
    for prefix, form in (('vec_pdist_fwd_kernel', 'fwd'), ('vec_gram_fwd', 'fwd_gram'), ('vec_pdist_bwd_sym_kernel', 'sym'),
                         ('vec_gram_bwd_sym_f32', 'gram_sym'), ('vec_gram_bwd_f32', 'gram_ordered'), ('vec_gram_bwd_f64', 'gram_f64')):
        if nm.startswith(prefix):
            return form
    return 'subset' if nm.endswith('true>') else 'ordered'


def variant(c, env):
    """What tells one launch of the case from another: the instantiations, and the launch arguments a switch pins."""
    names = route_of(c, env)
    extra = None
    if c['entry'] == 'subset':
        extra = subset_rows(env)
    elif form_of(names) == 'gram_sym':
        extra = env.get('MM_GRAM_BWD_PARTS')
    return tuple(names), extra


# ------------------------------------------------------------------------------------------------------------------- the table
_TERMS = ('quotient', 'quotient_l1', 'quotient_l2')


def case(entry, kind, m, dname, squared=True, loss=None, n=N, rows=None, batch=None, scale=True, refuse=False, primary=False):
    """One call of mm_vec_pdist_<entry>: `rows` a row range of the pair list (None = all); `batch` nodes of a table of N_TABLE
    rows (subset); `loss`: None (fwd / bwd: `squared` applies), 'stress', 'quotient' (both terms), 'quotient_l1', 'quotient_l2';
    `scale`: False passes scale_raw = NULL."""
    what = loss if loss else ('sq' if squared else 'plain')
    cid = f'{entry}-{kind}{m}-{dname}-{what}-n{n}'
    cid += (f'-rows{rows[0]}_{rows[1]}' if rows else '') + (f'-b{batch}of{N_TABLE}' if batch else '')
    cid += ('' if scale else '-noscale') + ('-refused' if refuse else '')
    return dict(id=cid, entry=entry, kind=kind, m=int(m), dname=dname, squared=bool(squared) or bool(loss), loss=loss, n=n,
                rows=rows, batch=batch, scale=scale, refuse=refuse, primary=primary, epoch=EPOCH)


def shards(n, world=3):
    """The row ranges of the library's own sharding rule (mm_shard_rows, restated in graphembed._backend.shard_rows)."""
    from graphembed import _backend as B
    return [tuple(B.shard_rows(n, world, r)) for r in range(world)]


def _variants(entry, index=0):
    """(squared, loss) settings of an entry: both `squared`; stress and one of the quotient's three term selections"""
    if entry in ('loss', 'subset'):
        return [(True, 'stress'), (True, _TERMS[index % 3])]
    return [(True, None), (False, None)]


def _build():
    cases = {}

    def add(*a, **kw):
        c = case(*a, **kw)
        if c['id'] in cases and kw.get('primary'):
            cases[c['id']]['primary'] = True
        cases.setdefault(c['id'], c)

    for dname in ('f32', 'f64'):
        for ki, kind in enumerate(KINDS):
            widths = [m for m in WIDTHS if m >= (1 if kind == 'euclidean' else 2)]
            for index, m in enumerate(widths):
                for entry in ('fwd', 'bwd', 'loss', 'subset'):
                    for sq, loss in _variants(entry, index + ki):
                        add(entry, kind, m, dname, sq, loss, batch=BATCHES[-1] if entry == 'subset' else None)
                # the matrix cores: what the entries take (the rest is refused: one case per refusal below)
                for sq in (True, False):
                    if not refused('fwd_gram', dname, kind, m, N):
                        add('fwd_gram', kind, m, dname, sq)
                    if kind != 'euclidean' and not refused('bwd_gram', dname, kind, m, N, sq):
                        add('bwd_gram', kind, m, dname, sq)
            # the sizes, the row ranges, the batch sizes and scale_raw = NULL: one width per kind
            m = PRIMARY[kind]
            for entry in ENTRIES:
                for sq, loss in _variants(entry):
                    if refused(entry, dname, kind, m, N, sq):
                        continue
                    if entry == 'subset':
                        for b in BATCHES:
                            add(entry, kind, m, dname, sq, loss, batch=b, primary=True)
                        add(entry, kind, m, dname, sq, loss, batch=BATCHES[1], scale=False, primary=True)
                        continue
                    add(entry, kind, m, dname, sq, loss, primary=True)
                    for n in SIZES:
                        add(entry, kind, m, dname, sq, loss, n=n, primary=True)
                    for rows in shards(N) + RANGES:
                        add(entry, kind, m, dname, sq, loss, rows=rows, primary=True)
                    if entry == 'loss':
                        add(entry, kind, m, dname, sq, loss, scale=False, primary=True)
    # the fp32 squared Euclidean distance on the matrix cores (W = g, no Gram: one instantiation per form)
    for m in (1, 16, 17, 31):
        add('bwd_gram', 'euclidean', m, 'f32', True)
    # the forward's row-tile height
    for n in FWD_HEIGHT_N:
        add('fwd', 'lorentz', PRIMARY['lorentz'], 'f32', True, n=n)
    add('fwd', 'lorentz', PRIMARY['lorentz'], 'f64', True, n=FWD_HEIGHT_N[2])
    # one case per refusal the entries state
    for entry in ('fwd', 'bwd', 'loss', 'subset'):
        add(entry, 'euclidean', MAX_DIM + 1, 'f32', True, 'stress' if entry in ('loss', 'subset') else None,
            batch=BATCHES[1] if entry == 'subset' else None, refuse=True)
    add('fwd_gram', 'euclidean', 10, 'f32', refuse=True)
    add('fwd_gram', 'lorentz', 33, 'f32', refuse=True)
    add('fwd_gram', 'lorentz', 2, 'f32', n=GRAM_MAX_N + 1, refuse=True)
    add('fwd_gram', 'sphere', 2, 'f64', n=GRAM_MAX_N + 1, refuse=True)
    add('bwd_gram', 'lorentz', 33, 'f32', refuse=True)
    add('bwd_gram', 'sphere', 17, 'f64', refuse=True)
    add('bwd_gram', 'euclidean', 10, 'f32', False, refuse=True)
    add('bwd_gram', 'euclidean', 32, 'f32', True, refuse=True)
    add('bwd_gram', 'euclidean', 10, 'f64', True, refuse=True)
    add('bwd_gram', 'lorentz', 2, 'f32', n=GRAM_MAX_N + 1, refuse=True)
    return list(cases.values())


CASES = _build()
BY_ID = {c['id']: c for c in CASES}
CONTROL = BY_ID[case('fwd', 'lorentz', PRIMARY['lorentz'], 'f32')['id']]      # its route depends on no switch
for _c in CASES:
    assert _c['refuse'] == (route_of(_c, {}) == []), _c['id']


def cases_for(env):
    """What runs under an environment: everything by default; under a switch the cases whose launch differs from the default
    one (under two switches: also from the launch under either alone), plus one control."""
    if not env:
        return CASES
    others = [{}] + ([{k: v} for k, v in env.items()] if len(env) > 1 else [])
    return [c for c in CASES if not c['refuse'] and all(variant(c, env) != variant(c, o) for o in others)] + [CONTROL]


def whole_of(c):
    """The case over the full row range that a row-range case is a part of."""
    return BY_ID[case(c['entry'], c['kind'], c['m'], c['dname'], c['squared'], c['loss'], n=c['n'])['id']]


def parts_of(c):
    """The three row-shard cases of a whole n = N primary case."""
    return [BY_ID[case(c['entry'], c['kind'], c['m'], c['dname'], c['squared'], c['loss'], rows=r)['id']] for r in shards(N)]


# ------------------------------------------------------------------------------------------------------------------- inputs
# one uniform coordinate in place of `rand`, where `rand` puts 31 .. 50 % of the pairs within NEAR of each other: (kind, m) ->
# half-width of the draw (sphere: angle, at most 2.4 rad between two points — away from the antipodal singularity too;
# Lorentz: rapidity; Euclidean: the coordinate)
ONE_COORDINATE = {('sphere', 2): 1.2, ('lorentz', 2): 1.5, ('euclidean', 1): 1.5}
# seeds redrawn: {key: bump}
REDRAWN = {}


def _seed(*key):
    return zlib.crc32(repr(key + (REDRAWN.get(key, 0), )).encode()) % (2**31)


@functools.lru_cache(maxsize=None)
def points(kind, m, rows, dname):
    """The reference's `rand` with ir = 0.3 (0.5 for the sphere), rounded to the case's dtype and put back on the manifold in
    that dtype; read-only."""
    gen = torch.Generator().manual_seed(_seed('points', kind, m, rows, dname))
    if (kind, m) in ONE_COORDINATE:
        t = (torch.rand(rows, dtype=torch.float64, generator=gen) * 2 - 1) * ONE_COORDINATE[(kind, m)]
        x = {'sphere': torch.stack([torch.cos(t), torch.sin(t)], 1), 'lorentz': torch.stack([torch.cosh(t), torch.sinh(t)], 1),
             'euclidean': t[:, None]}[kind]
    else:
        x = rp.make(kind, m).rand(rows, ir=0.5 if kind == 'sphere' else 0.3, dtype=torch.float64, generator=gen)
    x = sc._on_manifold(kind, sc._round(x.numpy(), dname), dname)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch_idx(kind, m, dname, batch):
    gen = torch.Generator().manual_seed(_seed('idx', kind, m, dname, batch))
    return torch.randperm(N_TABLE, generator=gen)[:batch].numpy().astype(np.int64)      # unsorted


@functools.lru_cache(maxsize=None)
def _d2(kind, m, rows, dname, batch):
    idx = None if batch is None else batch_idx(kind, m, dname, batch)
    d = ostep.pair_distances([(kind, m)], [points(kind, m, rows, dname)], idx)[0]
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _upstream(kind, m, n, dname, squared):
    """Upstream gradients of the whole pair list of the n points (plain backward); (g, share of pairs masked)."""
    gen = torch.Generator().manual_seed(_seed('g', kind, m, n, dname))
    g = sc._round(torch.randn(n * (n - 1) // 2, dtype=torch.float64, generator=gen).numpy(), dname)
    near = np.zeros(g.shape, dtype=bool)
    if dname == 'f32' and not squared:
        # d(acosh q)/dq, d(acos q)/dq and d(sqrt q)/dq are singular at d = 0: an fp32 ulp of q of a close pair moves its weight
        # by percents in ANY fp32 evaluation, so the plain distance is checked on the pairs further than NEAR apart
        near = np.sqrt(_d2(kind, m, n, dname, None)) < NEAR
        g = np.where(near, 0.0, g)
    g.setflags(write=False)
    near.setflags(write=False)
    return g, near


def raw_scale(c):
    return float(np.float32(SCALE_RAW)) if c['scale'] else NO_SCALE_RAW


def loss_of(c):
    return sc.loss_of(c, c['epoch'])       # (stress; quotient with alpha = 1.25, eps = 1 / (epoch + 1), its l1 / l2 selection)


def terms_of(c):
    return {'stress': 3, 'quotient': 3, 'quotient_l1': 1, 'quotient_l2': 2}[c['loss']]


@functools.lru_cache(maxsize=None)
def _targets(kind, m, n, dname, batch, loss, epoch, scale):
    """(pair vector | dense matrix, number of targets moved off a kink) — the recipe of step_cases.initial, then
    step_cases.settle_targets' rule on the host copy; the whole pair list of the n points, whatever rows a case takes."""
    gen = torch.Generator().manual_seed(_seed('targets', kind, m, n, dname, batch))
    rows = N_TABLE if batch else n
    data = {}
    if batch is None:
        t = torch.rand(n * (n - 1) // 2, dtype=torch.float64, generator=gen) * 0.9 + 0.05
        data['target'] = sc._round(t.numpy(), dname)
    else:
        t = torch.triu(torch.rand(rows, rows, dtype=torch.float64, generator=gen) * 0.9 + 0.05, 1)
        data['dense'] = sc._round((t + t.T).numpy(), dname)
        data['batches'] = {epoch: batch_idx(kind, m, dname, batch)}
    c = dict(n=rows, dname=dname, loss=loss, batch=batch)
    moved = sc.settle_targets(c, dict(scales=[scale]), data, epoch, [_d2(kind, m, rows, dname, batch)])
    out = data['dense'] if batch else data['target']
    out.setflags(write=False)
    return out, moved


def pair_slice(c):
    """[lo, hi) of the case's rows in the pair vector of its n points."""
    rb, re = c['rows'] or (0, c['n'])
    off = lambda r: r * (2 * c['n'] - r - 1) // 2       # noqa: E731  (mm_pair_offset)
    return off(rb), off(re)


def inputs(c):
    """dict(x, pairs (i, j node ids), d2 (the oracle's, per pair of the case), and per entry: g + masked (bwd), target | dense +
    idx, moved, scale (loss, subset))"""
    k, m, dn, batch = c['kind'], c['m'], c['dname'], c['batch']
    rows = N_TABLE if batch else c['n']
    out = dict(x=points(k, m, rows, dn), idx=None, target=None, dense=None, g=None, moved=0, scale=raw_scale(c))
    if c['refuse']:
        return out
    if batch:
        out['idx'] = batch_idx(k, m, dn, batch)
        out['pairs'] = ostep.pair_list(rows, out['idx'])
        out['d2'] = _d2(k, m, rows, dn, batch)
        out['dense'], out['moved'] = _targets(k, m, c['n'], dn, batch, c['loss'], c['epoch'], out['scale'])
        out['npairs_whole'] = out['pairs'][0].size
        return out
    lo, hi = pair_slice(c)
    i, j = ostep.pair_list(c['n'])
    out['pairs'], out['d2'], out['npairs_whole'] = (i[lo:hi], j[lo:hi]), _d2(k, m, rows, dn, None)[lo:hi], i.size
    if c['entry'] in ('bwd', 'bwd_gram'):
        g, near = _upstream(k, m, c['n'], dn, c['squared'])
        out['g'], out['masked'] = g[lo:hi], near[lo:hi]
    elif c['loss']:
        t, out['moved'] = _targets(k, m, c['n'], dn, None, c['loss'], c['epoch'], out['scale'])
        out['target'] = t[lo:hi]
    return out


def masked_share(c):
    """Share of the case's pairs that get zero upstream weight (fp32 plain backward); 0 elsewhere."""
    if c['entry'] not in ('bwd', 'bwd_gram') or c['refuse']:
        return 0.0
    near = inputs(c)['masked']
    return float(near.mean()) if near.size else 0.0


def evaluate(c, kind=None, x=None, loss=None, squared=None):
    """What the call of case `c` returns, from the oracle (oracle/exact.c through oracle.step): fwd — the pair vector (d^2 or d);
    bwd — the gradient [n, m]; loss / subset — (loss, gradient (full-size: zero rows outside a minibatch), d loss / d raw scale).
    `kind`, `x`, `loss`, `squared` replace the case's own: what a kernel standing in for another would compute."""
    inp = inputs(c)
    kind = kind or c['kind']
    x = inp['x'] if x is None else np.ascontiguousarray(x, dtype=np.float64)
    squared = c['squared'] if squared is None else squared
    factor = (kind, x.shape[1])
    same = kind == c['kind'] and x is inp['x']
    i, j = inp['pairs']
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    d2 = inp['d2'] if same else ostep._d2_and_grad(factor, x, lo, hi)
    if c['entry'] in ('fwd', 'fwd_gram'):
        return d2 if squared else np.sqrt(d2)
    if c['entry'] in ('bwd', 'bwd_gram'):
        g = inp['g']
        w = g if squared else np.where(g != 0, g / (2.0 * np.sqrt(np.where(d2 > 0, d2, 1.0))), 0.0)      # d (sqrt d2) = d d2 / (2 d)
        return ostep._d2_and_grad(factor, x, lo, hi, w)
    spec = loss_of(dict(c, loss=loss or c['loss']))
    if c['batch']:
        return ostep.objective([factor], [x], [inp['scale']], spec, dense=inp['dense'], idx=inp['idx'], d2=[d2])
    return ostep.objective([factor], [x], [inp['scale']], spec, target=inp['target'], pairs=(i, j), d2=[d2])


@functools.lru_cache(maxsize=None)
def _expected(cid):
    want = evaluate(BY_ID[cid])
    if isinstance(want, tuple):
        value, grads, sgrads = want
        return value, grads[0], sgrads[0]
    return want


def expected(c):
    """The oracle's value of `evaluate` for the case itself, cached: fwd — pair vector; bwd — gradient; loss / subset —
    (loss, gradient, d loss / d raw scale)."""
    return _expected(c['id'])


def formula_backward(c, dtype):
    """The gradient of a bwd / bwd_gram case by the ORACLE'S OWN FORMULA (oracle/exact.c: vec_q, vec_val, the pair's two
    contributions), evaluated by numpy in `dtype` (np.float32, np.float64, np.longdouble) on the case's inputs: what rounding
    alone does to that formula at that input — the measure a bound may be raised by (profiles/vec_oracle.md)."""
    inp = inputs(c)
    x, g = inp['x'].astype(dtype), inp['g'].astype(dtype)
    i, j = inp['pairs']
    a, b = x[i], x[j]
    one, eps = dtype(1), dtype(1e-8)
    if c['kind'] == 'euclidean':
        q = ((b - a) * (b - a)).sum(1)
        dq = np.ones_like(q) if c['squared'] else dtype(0.5) / np.sqrt(np.maximum(q, eps))
        ga, gb = -2 * (b - a), 2 * (b - a)
    elif c['kind'] == 'lorentz':
        sign = np.where(np.arange(c['m']) == 0, one, -one).astype(dtype)
        t = np.maximum(a[:, 0] * b[:, 0] - (a[:, 1:] * b[:, 1:]).sum(1), one)
        z = np.sqrt(t * t - one)
        d = np.maximum(np.log(t + z), eps)
        dq = (2 * d if c['squared'] else one) / np.maximum(z, eps)
        ga, gb = sign * b, sign * a
    else:
        q = np.minimum(np.maximum((a * b).sum(1), dtype(-1 + 1e-16)), dtype(1 - 1e-16))
        th = np.maximum(np.arccos(q), eps)
        dq = -(2 * th if c['squared'] else one) / np.maximum(np.sqrt(one - q * q), eps)
        ga, gb = b, a
    w = (g * dq)[:, None]
    grad = np.zeros(x.shape, dtype=dtype)
    np.add.at(grad, i, w * ga)
    np.add.at(grad, j, w * gb)
    return grad


def formula_error(c):
    """max |formula in the case's dtype - formula in long double| / max |gradient|: the rounding error of the oracle's own
    formula at the case's input, in the unit of GREL."""
    exact = formula_backward(c, np.longdouble)
    own = formula_backward(c, np.float32 if c['dname'] == 'f32' else np.float64)
    return float(np.abs(own.astype(np.longdouble) - exact).max() / np.abs(exact).max())


def kink_distances(c):
    inp = inputs(c)
    md = ostep.softplus(inp['scale']) * inp['d2']
    i, j = inp['pairs']
    return ostep.kink_distance(loss_of(c), ostep.pair_targets(inp['target'], inp['dense'], i, j), md)


# --------------------------------------------------------------------------------------------------------------- comparison
# The project's tolerances, imported or restated where their module is a GPU test module (tests/test_vec_gpu.py):
ABS = {'f32': 1e-6, 'f64': 1e-12}       # forward: ABS + REL |ref|, on d^2 (tests/test_vec_gpu.py)
REL = {'f32': 2e-5, 'f64': 1e-10}
GREL = {'f32': 5e-4, 'f64': 1e-9}       # plain backward: of max|grad| of the call (tests/test_vec_gpu.py)
TOL = sc.TOL                            # fused loss: 'loss', 'grad_vec', 'scale_grad' 

# Bounds above the table, by case id: {case id: {quantity: bound}}.  The rule (profiles/vec_oracle.md has the measurements): where
# a case misses its bound, the oracle's own formula is evaluated in the case's dtype and in long double at that input
# (`formula_error`); the bound may be raised to at most 3 x that rounding error (summation order), never from the kernel's
# output.  tests/test_vec_cases_host.py holds every entry to the rule.
# Lorentz(2), fp64, plain distance: the closest pair of the draw is 1.9e-4 apart, its weight 1 / sqrt(q^2 - 1) carries the
# rounding of q = x0 y0 - x1 y1 (terms up to 5.5) relative to q - 1 = 1.7e-8, and that pair's weight IS max|grad|: the oracle
# itself is 1.14e-9 of max|grad| from the long-double value — above the table's 1e-9.
RAISED = {
    'bwd-lorentz2-f64-plain-n131': {'grad': 3.4e-9},
    'bwd_gram-lorentz2-f64-plain-n131': {'grad': 3.4e-9},
}
RAISE_FACTOR = 3.0


def errors(c, want, got):
    """{quantity: (error, allowed)} of what the call returned against `want` (both as `evaluate` returns them)."""
    dn = c['dname']
    if c['entry'] in ('fwd', 'fwd_gram'):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (got.shape, want.shape)
        if not c['squared']:
            got, want = got * got, want * want      # the plain distance is held to the bound of its square
        if not want.size:
            return {'d2': (0.0, 1.0)}
        if not np.isfinite(got).all():              # (an unwritten pair is NaN)
            return {'d2': (float('inf'), 1.0)}
        return {'d2': (float((np.abs(got - want) / (ABS[dn] + REL[dn] * np.abs(want))).max()), 1.0)}
    if c['entry'] in ('bwd', 'bwd_gram'):
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape, (got.shape, want.shape)
        err = float(np.abs(got - want).max()) if np.isfinite(got).all() else float('inf')
        return {'grad': (err, max(GREL[dn], RAISED.get(c['id'], {}).get('grad', 0.0)) * float(np.abs(want).max()))}
    (lref, gref, sref), (loss, grad, sgrad) = want, got
    grad = np.asarray(grad, np.float64)
    assert grad.shape == gref.shape, (grad.shape, gref.shape)
    out = {'loss': (abs(loss - lref) if np.isfinite(loss) else float('inf'), TOL['loss'][dn] * abs(lref))}
    out['grad'] = (float(np.abs(grad - gref).max()) if np.isfinite(grad).all() else float('inf'),
                   TOL['grad_vec'][dn] * float(np.abs(gref).max()))
    if c['scale']:
        out['scale_grad'] = (abs(sgrad - sref) if np.isfinite(sgrad) else float('inf'),
                             TOL['scale_grad'][dn] * max(abs(sref), 1e-3 * abs(lref)))
    else:
        out['scale_grad'] = (abs(sgrad) if np.isfinite(sgrad) else float('inf'), 0.0)      # no scale: exactly zero
    return out


worst = sc.worst
