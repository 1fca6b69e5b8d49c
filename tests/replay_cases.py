"""The table of tests/test_replay_gpu.py: one row per accumulating entry point of include/mm_manifolds.h (every entry that takes
an mm_stream_t and whose name contains `_bwd`, `_loss` or `kl_loss`), per dtype and shape.  Host code only; nothing here runs a
kernel.  tests/test_replay_cases_host.py walks the table on the CPU, tests/test_replay_gpu.py captures every row's call in a graph
and replays it with the inputs A, B, A.

A row names
    entry, family, dname     the C entry point, the family whose cases module supplies inputs, oracle and bound, the dtype
    a, b                     two cases of that module with the same entry, dtype, shape and launch geometry (`geometry`) that differ
                             in the points and in the target / upstream vector / dense matrix
    buffers                  {buffer: (contract, the header line that states it)} for the workspace and, for the minibatch entries
                             whose header asks for it, the gradient: ANY = "may hold anything / cleared by the call" (the GPU test
                             fills it with 0xFF bytes before every replay), ZERO = "pass zero-filled" (the test zeroes it, and does
                             nothing more)
    deterministic            True: no float atomics, a replay is held to torch.equal with the eager call; False: summed with float
                             atomics, held to grass_cases.check's rule e_replay <= 2 e_eager + 64 eps max|oracle|
    minibatch, outside       True: rows of the gradient outside the batch are checked, and (what, the header line that promises it):
                             PLUS_ZERO = every bit zero, in every family
    cleared                  None, or (formula, bytes) of the region the call clears before it accumulates, for the rows whose
                             cleared region is at least HAZARD_BYTES — the size of the recorded failure (csrc/clear.hpp,
                             profiles/vec_deterministic.md: grad_x [200, 64] fp32 = 51 200 bytes)
    same_points              None, or why A and B share the points (the module provides one draw of them)
    one_side                 None, or why A and B share the target / upstream vector (the module provides one)
    keep_ws                  True: before the third replay the workspace is left as the second replay left it
    unroll                   True: the row is also recorded twice in ONE graph (A's buffers, then a second set holding B, one shared
                             workspace), as GraphedTrainStep(unroll=2) does

Where the cases come from.  SO(n) and Grassmann: the regimes of so_cases / mat_cases (`init` and `spread`, `uniform` and `spread`)
are two draws of the points at one shape; the subset modules nudge their dense matrix per regime.  Vector manifolds: vec_cases has
ONE draw per (kind, m, n, dtype), so B is that draw's POINTS with the node order reversed, against the same target / upstream
vector / dense matrix: the same points under other labels meet other targets, which is another problem of the same shape.  Its
oracle is vec_cases.evaluate(case, x=...), the module's own override for other points; A's is vec_cases.expected.  The bounds of
vec_cases.errors are relative to the oracle's own value (GREL, TOL), so they apply to B as they stand.  Only smooth settings are
taken (squared distances, the stress loss): a relabelled draw must not land on a kink of the quotient loss or in the masked
neighbourhood of the plain fp32 backward that vec_cases settled for its own draw.

Products: product_cases enumerates a second draw of the TARGETS on the same points (`tdraw`, its workspace-contract cases); the
minibatch B is that constructor at the enumerated batch.  mm_product_loss takes the same layout's squared pair distances.

SPD: the regimes `mid` and `wide` of spd_det_cases' instantiation cases at SPD(3), n = 130 (two draws of points, targets and upstream).

Stein: the regimes `spread` and `init` of stein_cases at SPD(3), n = 65 / batch 65 of 257; the pair-vector backward's B is the
module's pdiv_oracle on the `init` points (its own test sweeps `spread`).  Constant curvature: stereo_cases' (65, 8, c = 1, free)
in `init` and `spread`; stereo_product_cases' (65, (8, 8, 8)) in both regimes; stereo_subset_cases' (129, 65, (5, 5)) `init` and
the same tuple in `spread` through the module's own constructor.

SNE and SST: the regimes `near` and `mid` of sne_cases / sst_cases at n = 65 are two draws of both pair vectors.

Every bound is an existing one of the project (vec_cases.errors, mat_cases.Quantity.bound, product_cases.errors, the rule of
sne_cases.check / sst_cases.bound_of, stereo_cases.bound, grass_cases.check for the Stein rows, step_cases.TOL for the SPD rows);
nothing here states a tolerance."""
import functools
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HEADER = os.path.join(ROOT, 'include', 'mm_manifolds.h')
HAZARD_BYTES = 51200
ANY, ZERO = 'any', 'zero'
PLUS_ZERO = '+0'
ESZ = {'f32': 4, 'f64': 8}
EPS = {'f32': float(np.finfo(np.float32).eps), 'f64': float(np.finfo(np.float64).eps)}
QUANTITIES = ('loss', 'grad', 'scale_grad')


def accumulating_entries(text=None):
    """names of the header's entry points that take an mm_stream_t and contain `_bwd`, `_loss` or `kl_loss`, in header order"""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    out = []
    for m in re.finditer(r'\b(mm_\w+)\s*\(([^;{}]*?)\)\s*;', text):
        name, args = m.group(1), m.group(2)
        if 'mm_stream_t' in args and any(k in name for k in ('_bwd', '_loss', 'kl_loss')) and name not in out:
            out.append(name)
    return out


# ---- the header's promises, quoted --------------------------------------------------------------------------------------------------
Q_VEC_WS = '(accumulators, loss slots, zero-padded points and — as for SPD — 64 KB of self-validating workgroup starts of the backward\'s walk)'
Q_VEC_DET_WS = 'det_ws may hold anything on'
Q_SO_WS = 'ws: mm_so_pdist_ws_bytes(dtype, n, N), cleared by the call.'
Q_SO_LOSS_WS = 'ws: mm_so_pdist_loss_ws_bytes(dtype, n, N).'
Q_SO_SUB_WS = 'serves every batch and a captured step; each call clears it itself.'
Q_GRASS_LOSS_WS = 'ws: mm_grass_pdist_loss_ws_bytes(dtype, n, N, p), cleared by the call itself.'
Q_GRASS_SUB_WS = 'batch of an epoch and a captured step; the call clears it itself.'
Q_GRASS_BWD_WS = 'its ws: mm_grass_pdist_ws_bytes(dtype, n, N, p) bytes, may hold anything: cleared by the call.'
Q_OUTSIDE_PLUS = "rows idx[.] with this shard's partial gradient, every other row with +0"
Q_VEC_DET_OUTSIDE = 'gradient, every other row with +0.'
Q_VEC_SUB_GRAD = 'target matrix, idx int64[bs] distinct, grad_x [n_total, m] OVERWRITTEN — zero rows outside the batch; ws as'

# Entries that match the name rule and are deliberately not rows: neither has a workspace nor a sum over pairs.
EXEMPT = {
    'mm_spd_dist_bwd': 'element-wise over m pairs: one thread owns a pair and stores both gradients; no workspace, nothing accumulates',
    'mm_fast_bwd': 'element-wise closed forms of 2x2 / 3x3 matrices: no workspace, nothing accumulates',
}


def _row(entry, family, module, dname, a, b, geometry, buffers, deterministic, minibatch=False, cleared=None, unroll=False, label='',
         one_side=None, outside=None, same_points=None, keep_ws=False):
    assert (outside is not None) == minibatch
    return dict(entry=entry, family=family, module=module, dname=dname, a=a, b=b, geometry=geometry, buffers=buffers,
                deterministic=deterministic, minibatch=minibatch, cleared=cleared, unroll=unroll, one_side=one_side, outside=outside, same_points=same_points, keep_ws=keep_ws,
                id=f'{entry}-{dname}-{label}' + ('-large' if cleared else ''))


# =====================================================================================================================================
# vector manifolds (vec_cases / vec_det_cases)
VEC_ENTRY = {'bwd': 'mm_vec_pdist_bwd', 'bwd_gram': 'mm_vec_pdist_bwd_gram', 'loss': 'mm_vec_pdist_loss', 'subset': 'mm_vec_pdist_loss_subset'}
VEC_KIND, VEC_M, VEC_BATCH = 'lorentz', 11, 70          # vec_cases.PRIMARY['lorentz']; n = vec_cases.N = 131; 70 of the 200-node table
VEC_LARGE = ('euclidean', 64)                            # fp32, batch 70 of 200: the shape of the recorded failure


def _vec_rows():
    import vec_cases as vc
    rows = []

    def add(short, det, dname, kind, m, large=False):
        c = vc.case(short, kind, m, dname, True, None if short in ('bwd', 'bwd_gram') else 'stress', batch=VEC_BATCH if short == 'subset' else None)
        assert c['id'] in vc.BY_ID, c['id']
        entry = VEC_ENTRY[short] + ('_det' if det else '')
        sub = short == 'subset'
        n_launch = c['batch'] or c['n']
        geometry = dict(entry=entry, dname=dname, kind=kind, m=m, n=n_launch, n_total=vc.N_TABLE if sub else c['n'], rows=(0, n_launch),
                        squared=True, loss=c['loss'])
        if short == 'bwd_gram':
            buffers = {}
        elif det:
            buffers = {'det_ws': (ANY, Q_VEC_DET_WS)}
        else:
            buffers = {'ws': (ANY, Q_VEC_WS)}
            if sub:      # the header: OVERWRITTEN, so the gradient too may hold anything (the test fills it with NaN, as every output)
                buffers['grad'] = (ANY, Q_VEC_SUB_GRAD)
        cleared = None
        if large:
            esz = ESZ[dname]
            if det:      # clear_async over grad_x [n_total, m]
                cleared = ('n_total * m * sizeof(T)', vc.N_TABLE * m * esz)
            else:        # csrc/vec.hip, vec_loss_subset_t: the accumulators of all nodes (the loss slots behind them not counted)
                cleared = ('n_total * (pad_dim(m) + 1) * sizeof(T)', vc.N_TABLE * (vc.pad_dim(m) + 1) * esz)
        rows.append(_row(entry, 'vec', 'vec_det_cases' if det else 'vec_cases', dname, dict(id=c['id'], draw='table'),
                         dict(id=c['id'], draw='reversed'), geometry, buffers, det, sub, cleared, unroll=(short == 'subset' and not det and not large),
                         one_side='vec_cases has one target / upstream draw per shape',
                         label=f'{kind}{m}-n{n_launch}' + (f'of{vc.N_TABLE}' if sub else ''),
                         outside=None if not sub else (PLUS_ZERO, Q_VEC_DET_OUTSIDE if det else Q_VEC_SUB_GRAD)))

    for dname in ('f32', 'f64'):
        for short in ('bwd', 'loss', 'subset'):
            for det in (False, True):
                add(short, det, dname, VEC_KIND, VEC_M)
    add('bwd_gram', False, 'f32', VEC_KIND, VEC_M)
    add('bwd_gram', False, 'f64', VEC_KIND, VEC_M)          # (clears grad_x [n, m] at the head of the call: 131 * 11 * 8 bytes)
    for det in (False, True):
        add('subset', det, 'f32', *VEC_LARGE, large=True)
    # another path of the two full-batch atomic entries: fp32 beyond m = 32 the symmetric pair kernel is not built and the ordered
    # fallback serves the call (vec_cases.route), which clears the accumulators of all nodes at the head of the call
    for short in ('bwd', 'loss'):
        c = vc.case(short, VEC_LARGE[0], VEC_LARGE[1], 'f32', True, None if short == 'bwd' else 'stress')
        assert not any('sym' in name for name in vc.route_of(c, {})), vc.route_of(c, {})
        add(short, False, 'f32', *VEC_LARGE)
    return rows


def _vec_case(row):
    import vec_cases as vc
    assert row['a']['id'] == row['b']['id']
    return vc.BY_ID[row['a']['id']]


def vec_inputs(row, which):
    """{x, side (upstream gradient | target vector | dense matrix), idx, scale} as numpy arrays"""
    import vec_cases as vc
    c = _vec_case(row)
    inp = vc.inputs(c)
    side = inp['dense'] if c['batch'] else (inp['g'] if c['loss'] is None else inp['target'])
    x = inp['x']
    if row[which]['draw'] == 'reversed':      # the points under reversed labels; the target / upstream vector stays (the module has one)
        x = np.ascontiguousarray(x[::-1])
    return dict(x=np.asarray(x, np.float64), side=np.asarray(side, np.float64), idx=inp['idx'], scale=np.array([inp['scale']]))


@functools.lru_cache(maxsize=None)
def _vec_want(rid, which):
    """vec_cases.expected for the draw as it stands; vec_cases.evaluate with its `x` override — the module's own oracle on other
    points — for the relabelled one"""
    import vec_cases as vc
    row = BY_ID[rid]
    c = _vec_case(row)
    if row[which]['draw'] == 'table':
        want = vc.expected(c)
    else:
        want = vc.evaluate(c, x=vec_inputs(row, which)['x'])
        if isinstance(want, tuple):
            want = (want[0], want[1][0], want[2][0])
    if c['loss'] is None:
        return {'grad': want}
    return {'loss': np.array([want[0]]), 'grad': want[1], 'scale_grad': np.array([want[2]])}


def vec_want(row, which):
    return _vec_want(row['id'], which)


def _vec_tuple(c, d):
    return d['grad'] if c['loss'] is None else (float(d['loss'][0]), d['grad'], float(d['scale_grad'][0]))


def vec_judge(row, which, got):
    """{quantity: (error, bound)} by vec_cases.errors"""
    import vec_cases as vc
    c = _vec_case(row)
    return vc.errors(c, _vec_tuple(c, vec_want(row, which)), _vec_tuple(c, got))


# =====================================================================================================================================
# SO(n) (so_cases / so_subset_cases) and Grassmann (mat_cases / grass_subset_cases): mat_cases.Quantity
SO_N, SO_DIM, SO_BS = 65, 3, 65                  # 65: two 64-column blocks, a ragged last one (so_cases.compared, so_subset_cases.BATCHES)
SO_REGIMES = ('init', 'spread')
GRASS_N, GRASS_SHAPE, GRASS_BS = 65, (6, 3), 65  # mat_cases.ROW_SHAPES; p = 3: no closed-form exclusion (mat_cases.dist_compared)
GRASS_REGIMES = ('uniform', 'spread')


def _mat_rows():
    rows = []
    for dname in ('f32', 'f64'):
        for fam, regimes, shape, n, bs, n_total in (('so', SO_REGIMES, (SO_DIM, ), SO_N, SO_BS, 257), ('grass', GRASS_REGIMES, GRASS_SHAPE, GRASS_N, GRASS_BS, 257)):
            entries = [('bwd', False), ('loss', False), ('loss_subset', True)] + ([('bwd_subset', True)] if fam == 'so' else [])
            for short, sub in entries:
                entry = f'mm_{fam}_pdist_{short}'
                module = {('so', False): 'so_cases', ('so', True): 'so_subset_cases', ('grass', False): 'mat_cases', ('grass', True): 'grass_subset_cases'}[(fam, sub)]
                n_launch = bs if sub else n
                geometry = dict(entry=entry, dname=dname, shape=shape, n=n_launch, n_total=n_total if sub else n, rows=(0, n_launch), squared=True,
                                loss='stress' if 'loss' in short else None)
                if fam == 'so':
                    quote = Q_SO_SUB_WS if sub else (Q_SO_WS if short == 'bwd' else Q_SO_LOSS_WS)
                else:
                    quote = Q_GRASS_SUB_WS if sub else (Q_GRASS_BWD_WS if short == 'bwd' else Q_GRASS_LOSS_WS)
                a, b = (dict(regime=r) for r in regimes)
                one_side = None if short == 'loss_subset' else f'{module} has one upstream pattern / target vector per size: its oracle is built on it'
                rows.append(_row(entry, fam, module, dname, a, b, geometry, {'ws': (ANY, quote)}, False, sub, None, unroll=(short == 'loss_subset'), one_side=one_side,
                                 outside=(PLUS_ZERO, Q_OUTSIDE_PLUS) if sub else None,
                                 label='x'.join(str(s) for s in shape) + f'-n{n_launch}' + (f'of{n_total}' if sub else '')))
    return rows


def _mat_quantities(row, which):
    """{quantity: mat_cases.Quantity} of the row's case, under this module's quantity names"""
    regime, g = row[which]['regime'], row['geometry']
    short = row['entry'].split('_pdist_')[1]
    if row['family'] == 'so':
        import so_cases as sc
        import so_subset_cases as ssc
        N = g['shape'][0]
        if short == 'bwd':
            return {'grad': sc.pdist_quantities(regime, g['n'], N, True)[(None, 'grad')]}
        if short == 'loss':
            q = sc.loss_quantities(regime, g['n'], N, 'stress')
            return {'loss': q['loss'], 'grad': q['grad_x'], 'scale_grad': q['grad_scale']}
        if short == 'bwd_subset':
            return {'grad': ssc.held(ssc.pdist_quantities(regime, N, g['n'], True)['grad'])}
        q = ssc.loss_quantities(regime, N, g['n'], 'stress')
        return {'loss': ssc.held(q[(None, 'loss')]), 'grad': ssc.held(q[(None, 'grad_x')]), 'scale_grad': ssc.held(q[(None, 'grad_scale')])}
    import grass_subset_cases as gsc
    import mat_cases as mc
    N, p = g['shape']
    if short == 'bwd':
        assert 'grad' in mc.pdist_compared(regime, g['n'], N, p, True)
        return {'grad': mc.pdist_quantities(regime, g['n'], N, p, True)[(None, 'grad')]}
    names = {'loss': 'loss', 'grad_x': 'grad', 'grad_scale': 'scale_grad'}
    if short == 'loss':
        q = mc.loss_quantities(regime, g['n'], N, p)
        return {names[k]: q[k] for k in mc.loss_compared(regime, N, p)}
    q = gsc.subset_quantities(regime, N, p, g['n'], 'stress')
    return {names[k]: q[(None, k)] for k in gsc.subset_compared(regime, N, p)}


def mat_inputs(row, which):
    import torch
    regime, g = row[which]['regime'], row['geometry']
    short = row['entry'].split('_pdist_')[1]
    sub = row['minibatch']
    if row['family'] == 'so':
        import so_cases as sc
        import so_subset_cases as ssc
        N = g['shape'][0]
        x = sc.points(regime, g['n_total'], N)
        idx = ssc.batch_idx(g['n']) if sub else None
        dense = ssc.dense(regime, N, g['n']) if short == 'loss_subset' else None
        upstream, targets, scale = sc.upstream, sc.targets, sc.SCALE_RAW
    else:
        import grass_cases as gc
        import grass_subset_cases as gsc
        import mat_cases as mc
        N, p = g['shape']
        x = mc.points(regime, g['n_total'], N, p)
        idx = gsc.batch_idx(g['n_total'], g['n']) if sub else None
        dense = gsc.dense(regime, N, p, g['n']) if sub else None
        upstream, targets, scale = mc.upstream, gc.targets, gc.SCALE_RAW
    npairs = g['n'] * (g['n'] - 1) // 2
    side = dense if dense is not None else (upstream(npairs) if 'bwd' in short else targets(g['n']))
    assert isinstance(x, torch.Tensor)
    return dict(x=x.double().numpy(), side=side.double().numpy(), idx=None if idx is None else idx.numpy().astype(np.int64), scale=np.array([scale]))


def mat_want(row, which):
    return {k: q.want.double().numpy() for k, q in _mat_quantities(row, which).items()}


def mat_judge(row, which, got):
    out = {}
    for k, q in _mat_quantities(row, which).items():
        g, w = np.asarray(got[k], np.float64).reshape(-1), q.want.double().numpy().reshape(-1)
        assert g.shape == w.shape, (row['id'], k, g.shape, w.shape)
        out[k] = (float(np.abs(g - w).max()) if np.isfinite(g).all() else float('inf'), q.bound(row['dname']))
    return out


# =====================================================================================================================================
# stochastic-neighbour KL objective (sne_cases): no float atomics, a workspace that needs no clearing
SNE_N, SNE_REGIMES = 65, ('near', 'mid')          # 65: one node past a 64-column block; both regimes have a recorded reference there
SNE_MODE = {'incl': 0, 'excl': 1}                 # MM_SNE_INCLUSIVE, MM_SNE_EXCLUSIVE
Q_SNE_WS = 'ws: mm_sne_kl_ws_bytes(dtype, n) bytes (0 for an unknown dtype, n < 0 or n above the limit); it needs no clearing.'


Q_SST_WS = 'it needs no clearing.  Nothing is allocated and nothing synchronises: the call can be captured in a HIP graph.'


def _kl_rows(family, quote):
    """mm_sne_kl_loss / mm_sst_kl_loss (sst_cases has the same regimes at n = 65, and the same rule as `bound_of`)"""
    rows, entry = [], f'mm_{family}_kl_loss'
    for dname in ('f32', 'f64'):
        for mode in ('incl', 'excl'):
            geometry = dict(entry=entry, dname=dname, n=SNE_N, n_total=SNE_N, rows=(0, SNE_N), squared=True, loss='kl', mode=mode)
            a, b = (dict(regime=r) for r in SNE_REGIMES)
            rows.append(_row(entry, family, f'{family}_cases', dname, a, b, geometry, {'ws': (ANY, quote)}, True, unroll=(mode == 'incl'),
                             label=f'{mode}-n{SNE_N}'))
    return rows


def sst_inputs(row, which):
    import sst_cases as T
    g, m = T.inputs(row['geometry']['n'], row[which]['regime'])
    return dict(x=np.asarray(m, np.float64), side=np.asarray(g, np.float64), idx=None, scale=None)


def sst_want(row, which):
    import sst_cases as T
    rec = T.oracle(row['geometry']['n'], row[which]['regime'], row['geometry']['mode'])
    return {'loss': np.array([float(rec['loss'])]), 'grad': np.asarray(rec['grad'], np.float64)}


def sst_judge(row, which, got):
    """sst_cases.bound_of: 2 e_ref + 64 eps scale"""
    import sst_cases as T
    n, regime, mode, dname = row['geometry']['n'], row[which]['regime'], row['geometry']['mode'], row['dname']
    rec = T.oracle(n, regime, mode)
    out = {}
    for what in ('loss', 'grad'):
        w, g = rec[what], np.asarray(got[what])
        out[what] = (T.deviation(g.reshape(np.shape(w)), w) if np.isfinite(g).all() else float('inf'), T.bound_of(n, regime, mode, dname, what)[0])
    return out


def sne_inputs(row, which):
    """x: the pair vector m of manifold distances; side: the pair vector of graph distances (the target)"""
    import sne_cases as S
    g, m = S.inputs(row['geometry']['n'], row[which]['regime'])
    return dict(x=np.asarray(m, np.float64), side=np.asarray(g, np.float64), idx=None, scale=None)


def sne_want(row, which):
    import sne_cases as S
    loss, grad = S.oracle(row['geometry']['n'], row[which]['regime'], row['geometry']['mode'])
    return {'loss': np.array([float(loss)]), 'grad': np.asarray(grad, np.float64)}


def sne_judge(row, which, got):
    """sne_cases.check's rule: e <= 2 e_ref + 64 eps scale, e_ref the recorded reference's deviation from the same oracle"""
    import sne_cases as S
    n, regime, mode, dname = row['geometry']['n'], row[which]['regime'], row['geometry']['mode'], row['dname']
    out = {}
    for k, what in enumerate(('loss', 'grad')):
        w = S.oracle(n, regime, mode)[k]
        bound = 2 * S.e_ref(n, regime, mode, dname, what) + 64 * S.EPS[dname] * S.scale_of(w)
        g = np.asarray(got[what])
        out[what] = (S.deviation(g.reshape(np.shape(w)), w) if np.isfinite(g).all() else float('inf'), bound)
    return out


# =====================================================================================================================================
# product embeddings (product_cases): mm_product_pairs_loss / _subset on the mixed pair kernel, mm_product_loss on pair vectors
PRODUCT_FACTORS = (('euclidean', 3), ('euclidean', 6), ('spd', 3))      # product_cases.LAYOUTS[38]: primary, two vector factors and SPD(3)
PRODUCT_BATCH = 131                                                     # the batch product_cases enumerates for this layout, of N_TABLE = 200
Q_PRODUCT_WS = '*   ws         mm_product_pairs_ws_bytes; every successful call leaves its accumulators zero, so a'
Q_PRODUCT_SUB_GRAD = ' * the full-size grads[k] — the other rows are NOT touched: pass zero-filled buffers.  row_begin/row_end'
Q_PRODUCT_LOSS_WS = 'size_t mm_product_loss_ws_bytes(int dtype, int nf);'      # (no sentence in the header; flags-less: the call clears its slots)


def _product_case(row, which):
    import product_cases as pc
    g = row['geometry']
    return pc.case(PRODUCT_FACTORS, row['dname'], 'stress', 0, batch=g['n'] if row['minibatch'] else None, tdraw=row[which]['tdraw'])


def _product_rows():
    import product_cases as pc
    rows = []
    for dname in ('f32', 'f64'):
        for entry, sub in (('mm_product_pairs_loss', False), ('mm_product_pairs_loss_subset', True), ('mm_product_loss', False)):
            n = PRODUCT_BATCH if sub else pc.N
            assert pc.case(PRODUCT_FACTORS, dname, 'stress', 0, batch=n if sub else None)['id'] in pc.BY_ID
            geometry = dict(entry=entry, dname=dname, factors=PRODUCT_FACTORS, n=n, n_total=pc.N_TABLE if sub else n, rows=(0, n), squared=True,
                            loss='stress')
            if entry == 'mm_product_loss':
                buffers = {'ws': (ANY, Q_PRODUCT_LOSS_WS)}
            else:      # flags = 0 in every call: the workspace may hold anything, the call clears what it needs
                buffers = {'ws': (ANY, Q_PRODUCT_WS)}
                if sub:
                    buffers['grad'] = (ZERO, Q_PRODUCT_SUB_GRAD)
            rows.append(_row(entry, 'product', 'product_cases', dname, dict(tdraw=0), dict(tdraw=1), geometry, buffers, False, sub, None,
                             unroll=sub, label=f'e3xe6xp3-n{n}' + (f'of{pc.N_TABLE}' if sub else ''),
                             one_side=None, outside=(PLUS_ZERO, Q_PRODUCT_SUB_GRAD) if sub else None,
                             same_points='product_cases has one draw of the points per factor list and a second draw of the targets (tdraw)'))
    return rows


def product_inputs(row, which):
    """xs: the factors' points; side: the target vector / dense matrix of draw `tdraw`; for mm_product_loss xs are the factors'
    squared pair distances (the oracle's, rounded to the dtype: what a forward would hand over)"""
    import product_cases as pc
    import step_cases as sc
    c = _product_case(row, which)
    inp = pc.inputs(c)
    xs = [np.asarray(x, np.float64) for x in inp['xs']]
    if row['entry'] == 'mm_product_loss':
        xs = [np.asarray(sc._round(np.array(d), row['dname']), np.float64) for d in pc._d2(c['factors'], c['n'], c['dname'], c['init'], None)]
    side = inp['dense'] if c['batch'] else inp['target']
    return dict(xs=xs, side=np.asarray(side, np.float64), idx=inp['idx'], scales=np.asarray(inp['scales'], np.float64))


def _product_keys(factors):
    return [f'grad/{k}:{f}{d}' for k, (f, d) in enumerate(factors)], [f'scale_grad/{k}:{f}{d}' for k, (f, d) in enumerate(factors)]


@functools.lru_cache(maxsize=None)
def _product_want(rid, which):
    import product_cases as pc
    from oracle import step as ostep
    row = BY_ID[rid]
    c, inp = _product_case(row, which), product_inputs(row, which)
    gk, sk = _product_keys(c['factors'])
    scales = [float(v) for v in inp['scales']]
    if row['entry'] == 'mm_product_loss':      # the element-wise part of oracle.step.objective on the pair vectors it is handed
        md = sum(ostep.softplus(s) * d for s, d in zip(scales, inp['xs']))
        value, slope = ostep.loss_and_slope(pc.loss_of(c), inp['side'], md)
        out = {'loss': np.array([value])}
        for k, (s, d) in enumerate(zip(scales, inp['xs'])):
            out[gk[k]], out[sk[k]] = slope * ostep.softplus(s), np.array([ostep.sigmoid(s) * float((slope * d).sum())])
        return out
    d2 = list(pc._d2(c['factors'], pc.N_TABLE if c['batch'] else c['n'], c['dname'], c['init'], c['batch']))
    if c['batch']:
        value, grads, sgrads = ostep.objective(list(c['factors']), inp['xs'], scales, pc.loss_of(c), dense=inp['side'], idx=inp['idx'], d2=d2)
    else:
        value, grads, sgrads = ostep.objective(list(c['factors']), inp['xs'], scales, pc.loss_of(c), target=inp['side'],
                                               pairs=pc.inputs(c)['pairs'], d2=d2)
    out = {'loss': np.array([value])}
    for k in range(len(gk)):
        out[gk[k]], out[sk[k]] = grads[k], np.array([sgrads[k]])
    return out


def product_want(row, which):
    return _product_want(row['id'], which)


def product_judge(row, which, got):
    """product_cases.errors (step_cases.TOL, relative to the oracle's own values).  mm_product_loss: its g_out vectors are the
    upstream gradients every factor's point gradient is linear in, and are held to the table's gradient tolerance of that factor"""
    import product_cases as pc
    c = _product_case(row, which)
    gk, sk = _product_keys(c['factors'])
    w = product_want(row, which)
    tup = lambda d: (float(np.asarray(d['loss']).reshape(-1)[0]), [d[k] for k in gk], [float(np.asarray(d[k]).reshape(-1)[0]) for k in sk])   # noqa: E731
    return pc.errors(c, tup(w), tup(got))


# =====================================================================================================================================
# SPD(d), full batch: the atomic entries and their bit-deterministic twins (spd_det_cases: Case(regime, D, n, kind, rows))
SPD_D, SPD_N, SPD_REGIMES = 3, 130, ('mid', 'wide')      # spd_det_cases.instantiation_cases: n = 130, 17 chunks, a ragged last one
Q_SPD_WS = "The workspace is the caller's and may hold anything when it is first"
Q_SPD_SUB_GRAD = 'grad_x   [n_total, d, d], OVERWRITTEN: rows idx[.] with the gradient, every other row with zero'
SPD_ENTRIES = (('mm_spd_pdist_bwd', 'bwd_sq', False), ('mm_spd_pdist_loss', 'stress', False), ('mm_spd_pdist_bwd_det', 'bwd_sq', True),
               ('mm_spd_pdist_loss_det', 'stress', True))


def _spd_rows():
    rows = []
    for dname in ('f32', 'f64'):
        for entry, kind, det in SPD_ENTRIES:
            geometry = dict(entry=entry, dname=dname, shape=(SPD_D, ), n=SPD_N, n_total=SPD_N, rows=(0, SPD_N), squared=True,
                            loss=None if kind == 'bwd_sq' else kind, kind=kind)
            buffers = {'ws': (ANY, Q_SPD_WS)}
            if det:
                buffers['det_ws'] = (ANY, Q_VEC_DET_WS)
            a, b = (dict(regime=r) for r in SPD_REGIMES)
            # keep_ws: before the THIRD replay the workspace stays as the second left it — the self-cleaning accumulators and the
            # table of workgroup starts of B's walk are what A's call finds (before the second replay it is 0xFF bytes, as elsewhere)
            rows.append(_row(entry, 'spd', 'spd_det_cases', dname, a, b, geometry, buffers, det, unroll=(entry == 'mm_spd_pdist_loss'),
                             label=f'spd{SPD_D}-n{SPD_N}', keep_ws=True))
        # the node minibatch (spd_subset_cases.instantiation_cases: batch 130 of the 257-node table, stress)
        geometry = dict(entry='mm_spd_pdist_loss_subset', dname=dname, shape=(SPD_D, ), n=SPD_N, n_total=257, rows=(0, SPD_N), squared=True,
                        loss='stress', kind='stress')
        a, b = (dict(regime=r) for r in SPD_REGIMES)
        rows.append(_row('mm_spd_pdist_loss_subset', 'spd', 'spd_subset_cases', dname, a, b, geometry, {'ws': (ANY, Q_SPD_WS)}, False, True,
                         label=f'spd{SPD_D}-n{SPD_N}of257', keep_ws=True, outside=(PLUS_ZERO, Q_SPD_SUB_GRAD)))
    return rows


def _spd_case(row, which):
    import spd_det_cases as C
    if row['minibatch']:
        import spd_subset_cases as S
        c = S.Case(row[which]['regime'], SPD_D, SPD_N, 'stress', None)
        assert c in S.instantiation_cases() and S.N_TOTAL == row['geometry']['n_total']
        return c
    c = C.Case(row[which]['regime'], SPD_D, SPD_N, row['geometry']['kind'], None)
    assert c in C.instantiation_cases()
    return c


def spd_inputs(row, which):
    import spd_det_cases as C
    c = _spd_case(row, which)
    if row['minibatch']:
        import spd_subset_cases as S
        return dict(x=S.points(c.regime, c.D).double().numpy(), side=S.dense(c.regime, c.D, c.bs).double().numpy(),
                    idx=S.batch_idx(c.bs).numpy().astype(np.int64), scale=np.array([S.SCALE_RAW]))
    return dict(x=C.points(c.regime, c.D, c.n).double().numpy(), side=C.loaded(c).double().numpy(), idx=None, scale=np.array([C.SCALE_RAW]))


def spd_want(row, which):
    import spd_det_cases as C
    if row['minibatch']:
        import spd_subset_cases as S
        o = S.oracle(_spd_case(row, which))
    else:
        o = C.oracle(_spd_case(row, which))
    out = {'grad': o.grad_x.double().numpy()}
    if row['geometry']['loss']:
        out['loss'], out['scale_grad'] = o.loss.double().numpy(), o.grad_scale.double().numpy()
    return out


def spd_judge(row, which, got):
    """spd_det_cases holds its entries to each other (e_det <= 2 e_atomic + 64 eps S), not to a number; the absolute bound of a single
    call is the project's table for an SPD factor (step_cases.TOL: loss, grad_spd, scale_grad), as product_cases.errors applies it"""
    import product_cases as pc
    w, dn = spd_want(row, which), row['dname']
    g = np.asarray(got['grad'], np.float64)
    if not row['geometry']['loss']:
        return {'grad': (float(np.abs(g - w['grad']).max()) if np.isfinite(g).all() else float('inf'), pc.TOL['grad_spd'][dn] * float(np.abs(w['grad']).max()))}
    c = dict(id='', dname=dn, factors=(('spd', SPD_D), ))
    e = pc.errors(c, (float(w['loss'][0]), [w['grad']], [float(w['scale_grad'][0])]),
                  (float(np.asarray(got['loss']).reshape(-1)[0]), [g], [float(np.asarray(got['scale_grad']).reshape(-1)[0])]))
    return {'loss': e['loss'], 'grad': e[f'grad/0:spd{SPD_D}'], 'scale_grad': e[f'scale_grad/0:spd{SPD_D}']}


# =====================================================================================================================================
# Stein-divergence SPD entries (stein_cases).  Its rule is grass_cases.check: e_new <= 2 e_old + 64 eps max|oracle|, e_old the deviation
# from the same oracle of the route before the fused kernels, measured on the same GPU in the same test — so the GPU test runs that
# route (tests/test_stein_loss_gpu.py: old_route, old_pdiv) once per case and hands its deviations to `stein_judge`.
STEIN_D, STEIN_N, STEIN_BS, STEIN_REGIMES = 3, 65, 65, ('spread', 'init')      # stein_cases.SIZES / BATCHES: a ragged second column block
Q_STEIN_WS = '(gradient-transparent), sqrt of it if !squared.  Layouts, workspace (mm_spd_pdist_ws_bytes), row ranges and'
Q_STEIN_OUTSIDE = ' * rows idx[.] with this shard\'s partial gradient, every other row with +0 — no gather, no scatter-add, no zero fill.'
Q_STEIN_BWD_OUTSIDE = ' * the BATCH\'s rows [row_begin, row_end) (bs (bs - 1) / 2 entries for the whole batch), grad_x [n_total,d,d] is OVERWRITTEN'
STEIN_ENTRIES = (('mm_spd_stein_pdiv_bwd', False), ('mm_spd_stein_pdiv_loss', False), ('mm_spd_stein_pdiv_loss_subset', True),
                 ('mm_spd_stein_pdiv_bwd_subset', True))


def _stein_rows():
    rows = []
    for dname in ('f32', 'f64'):
        for entry, sub in STEIN_ENTRIES:
            loss = 'stress' if 'loss' in entry else None
            n = STEIN_BS if sub else STEIN_N
            geometry = dict(entry=entry, dname=dname, shape=(STEIN_D, ), n=n, n_total=257 if sub else n, rows=(0, n), squared=True, loss=loss)
            a, b = (dict(regime=r) for r in STEIN_REGIMES)
            outside = None if not sub else (PLUS_ZERO, Q_STEIN_OUTSIDE if loss else Q_STEIN_BWD_OUTSIDE)
            rows.append(_row(entry, 'stein', 'stein_cases', dname, a, b, geometry, {'ws': (ANY, Q_STEIN_WS)}, False, sub, None,
                             unroll=(entry == 'mm_spd_stein_pdiv_loss_subset'), label=f'spd{STEIN_D}-n{n}' + ('of257' if sub else ''),
                             one_side=None if entry == 'mm_spd_stein_pdiv_loss_subset' or loss else 'stein_cases.upstream is one vector per length',
                             outside=outside, keep_ws=True))
    return rows


def stein_inputs(row, which):
    import stein_cases as T
    g, regime = row['geometry'], row[which]['regime']
    sub, loss = row['minibatch'], g['loss']
    x = T.points(regime, g['n_total'], STEIN_D)
    npairs = g['n'] * (g['n'] - 1) // 2
    side = T.upstream(npairs) if not loss else (T.dense(regime, STEIN_D, g['n']) if sub else T.targets(regime, g['n'], STEIN_D))
    return dict(x=x.double().numpy(), side=side.double().numpy(), idx=T.batch_idx(g['n']).numpy().astype(np.int64) if sub else None,
                scale=np.array([T.SCALE_RAW]))


def stein_want(row, which):
    import stein_cases as T
    import torch
    g, regime = row['geometry'], row[which]['regime']
    if not g['loss']:
        idx = T.batch_idx(g['n']) if row['minibatch'] else torch.arange(g['n'])
        return {'grad': T.pdiv_oracle(T.points(regime, g['n_total'], STEIN_D), idx, True)[1].double().numpy()}
    o = T.batch_oracle(regime, STEIN_D, g['n'], 'stress') if row['minibatch'] else T.full_oracle(regime, g['n'], STEIN_D, 'stress')
    return {'loss': o[0].double().numpy(), 'grad': o[1].double().numpy(), 'scale_grad': o[2].double().numpy()}


def stein_judge(row, which, got, e_old=None):
    """grass_cases.check's rule; `e_old`: {quantity: deviation of the old route from the oracle}, measured by the GPU test"""
    assert e_old is not None, 'the Stein rule needs the old route measured on the same GPU'
    w = stein_want(row, which)
    out = {}
    for q in w:
        g = np.asarray(got[q], np.float64).reshape(-1)
        err = float(np.abs(g - w[q].reshape(-1)).max()) if np.isfinite(g).all() else float('inf')
        out[q] = (err, 2 * e_old[q] + 64 * EPS[row['dname']] * float(np.abs(w[q]).max()))
    return out


# =====================================================================================================================================
# constant curvature: mm_stereo_pdist_bwd (stereo_cases).  No float atomics: a replay returns the eager call's bits.
STEREO_CASES = ((65, 8, 1.0, False, 'init', None), (65, 8, 1.0, False, 'spread', None))      # stereo_cases.CASES: free curvature c = 1
Q_STEREO_WS = 'arguments the library refuses); it needs no clearing.'


def _stereo_rows():
    import stereo_cases as S
    rows = []
    assert all(c in S.CASES for c in STEREO_CASES)
    n, m = STEREO_CASES[0][:2]
    for dname in ('f32', 'f64'):
        geometry = dict(entry='mm_stereo_pdist_bwd', dname=dname, n=n, n_total=n, m=m, rows=(0, n), squared=True, loss=None,
                        c_mode=S.mode_of(1.0, False))
        rows.append(_row('mm_stereo_pdist_bwd', 'stereo', 'stereo_cases', dname, dict(case=STEREO_CASES[0]), dict(case=STEREO_CASES[1]), geometry,
                         {'ws': (ANY, Q_STEREO_WS)}, True, unroll=True, label=f'm{m}-n{n}',
                         one_side='stereo_cases.upstream is one pattern per length'))
    return rows


def stereo_inputs(row, which):
    """x: the points; side: the upstream gradient; scale: the raw curvature parameter (one element, device memory)"""
    import stereo_cases as S
    x, c_raw = S.make_inputs(row[which]['case'])
    n = x.shape[0]
    return dict(x=np.asarray(x, np.float64), side=np.asarray(S.upstream(n * (n - 1) // 2), np.float64), idx=None, scale=np.array([float(c_raw)]))


@functools.lru_cache(maxsize=None)
def _stereo_oracle(case):
    import stereo_cases as S
    x, c_raw = S.make_inputs(case)
    n = case[0]
    return S.pdist_grads(x, c_raw, S.mode_of(case[2], case[3]), True, S.upstream(n * (n - 1) // 2), (0, n))


def stereo_want(row, which):
    wx, wc, _ = _stereo_oracle(row[which]['case'])
    return {'grad': np.asarray(wx, np.float64), 'grad_c': np.array([float(wc)])}


def stereo_judge(row, which, got):
    """stereo_cases.bound with the recorded reference-fp32 deviations, as tests/test_stereo_gpu.py::check applies it"""
    import stereo_cases as S
    case, dn = row[which]['case'], row['dname']
    wx, wc, wcs = _stereo_oracle(case)
    R, tag = S.recorded(), S.case_id(case)
    out = {}
    for q, w, scale, key in (('grad', wx, float(np.abs(wx).max()), 'gx_sq_f32'), ('grad_c', wc, float(wcs), 'gc_sq_f32')):
        ref32 = S.deviation(R[f'{tag}/{key}'], w) if dn == 'f32' else 0.0
        g = np.asarray(got[q], np.float64).reshape(np.shape(w))
        out[q] = (S.deviation(g, w) if np.isfinite(g).all() else float('inf'), S.bound(dn, ref32, scale))
    return out


# products of constant-curvature factors (stereo_product_cases, stereo_subset_cases), the stress setting; no float atomics
STEREO_PRODUCT_CASES = tuple((65, (8, 8, 8), (1.0, -1.0, -0.01), (True, True, False), regime, None) for regime in ('init', 'spread'))
# the minibatch: stereo_subset_cases enumerates (129, 65, (5, 5)) in `init`; B is the same tuple in `spread`, built by the module's own
# make_inputs / dense_of / oracle.  It has no recorded fp32 reference, so its fp32 bound is the rule's floor alone (never looser).
STEREO_SUBSET_CASES = tuple((129, 65, (5, 5), (0.01, -0.3), (False, False), regime, None) for regime in ('init', 'spread'))
Q_STEREO_PRODUCT_WS = 'mm_stereo_pdist_ws_bytes describes, plus (nf + 1) fp64 partials per tile; it needs no clearing.'
Q_STEREO_SUB_WS = ' * ws: mm_stereo_product_ws_bytes(dtype, bs, nf, m) - the BATCH\'s size; it needs no clearing.'
Q_STEREO_SUB_OUTSIDE = 'OVERWRITTEN: rows idx[.] with this shard\'s partial gradient, every other row with exact zeros;'


def _stereo_product_rows():
    import stereo_product_cases as P
    import stereo_subset_cases as SS
    assert all(c in P.CASES for c in STEREO_PRODUCT_CASES) and STEREO_SUBSET_CASES[0] in SS.CASES
    rows = []
    for dname in ('f32', 'f64'):
        for entry, cases, sub in (('mm_stereo_product_loss', STEREO_PRODUCT_CASES, False), ('mm_stereo_product_loss_subset', STEREO_SUBSET_CASES, True)):
            c = cases[0]
            n, ds = (c[1], c[2]) if sub else (c[0], c[1])
            geometry = dict(entry=entry, dname=dname, n=n, n_total=c[0], ms=tuple(ds), rows=(0, n), squared=True, loss='stress',
                            c_modes=tuple(SS.modes_of(c) if sub else P.modes_of(c)))
            rows.append(_row(entry, 'stereo', 'stereo_subset_cases' if sub else 'stereo_product_cases', dname, dict(case=cases[0]),
                             dict(case=cases[1]), geometry, {'ws': (ANY, Q_STEREO_SUB_WS if sub else Q_STEREO_PRODUCT_WS)}, True, sub,
                             unroll=False, label='x'.join(str(d) for d in ds) + f'-n{n}' + (f'of{c[0]}' if sub else ''),
                             outside=(PLUS_ZERO, Q_STEREO_SUB_OUTSIDE) if sub else None))
    return rows


def _stereo_product_oracle(row, which):
    import stereo_product_cases as P
    import stereo_subset_cases as SS
    return (SS if row['minibatch'] else P).oracle(row[which]['case'], 'stress')


def stereo_product_inputs(row, which):
    """xs: the factors' tables; side: the float32 target vector / dense matrix (NaN outside the batch's pairs); scales: raw curvatures"""
    import stereo_product_cases as P
    import stereo_subset_cases as SS
    case = row[which]['case']
    if row['minibatch']:
        xs, craws, idx = SS.make_inputs(case)
        side = SS.dense_of(case)
    else:
        (xs, craws), idx = P.make_inputs(case), None
        side = P.oracle(case, 'stress')['target']
    return dict(xs=[np.asarray(x, np.float64) for x in xs], side=np.asarray(side, np.float64), idx=idx,
                scales=np.asarray([float(c) for c in craws], np.float64))


def stereo_product_want(row, which):
    o = _stereo_product_oracle(row, which)
    out = {'loss': np.array([float(o['loss'])])}
    for k in range(len(o['gx'])):
        out[f'grad/{k}'], out[f'grad_c/{k}'] = np.asarray(o['gx'][k], np.float64), np.array([float(o['gc'][k])])
    return out


def stereo_product_judge(row, which, got):
    """stereo_cases.bound per quantity, with the recorded reference-fp32 deviation where the case has a record
    (tests/test_stereo_product_gpu.py::compare, tests/test_stereo_subset_gpu.py)"""
    import stereo_cases as S
    import stereo_product_cases as P
    import stereo_subset_cases as SS
    case, dn, sub = row[which]['case'], row['dname'], row['minibatch']
    o, R = _stereo_product_oracle(row, which), S.recorded()
    key = (SS if sub else P).key
    idx = SS.batch_of(case) if sub else None

    def ref_dev(what, want):
        k = key(case, 'stress', what, 'f32')
        if dn != 'f32' or k not in R:
            return 0.0
        r = R[k]
        return S.deviation(r[0] if what.startswith('gc') else r, want)

    def one(q, want, scale, what, ref_want=None):
        g = np.asarray(got[q], np.float64).reshape(np.shape(want))
        err = S.deviation(g, want) if np.isfinite(g).all() else float('inf')
        return err, S.bound(dn, ref_dev(what, want if ref_want is None else ref_want), float(scale))

    out = {'loss': one('loss', o['loss'], o['loss_scale'], 'loss')}
    for k in range(len(o['gx'])):
        gx = o['gx'][k]
        out[f'grad/{k}'] = one(f'grad/{k}', gx, np.abs(gx).max(), f'gx{k}', gx[idx] if sub else None)
        out[f'grad_c/{k}'] = one(f'grad_c/{k}', o['gc'][k], o['gcs'][k], f'gc{k}')
    return out


def _stereo_dispatch(k):
    single = (stereo_inputs, stereo_want, stereo_judge)
    multi = (stereo_product_inputs, stereo_product_want, stereo_product_judge)
    return lambda row, *a: (single if row['entry'] == 'mm_stereo_pdist_bwd' else multi)[k](row, *a)


FAMILIES = {'stereo': (_stereo_dispatch(0), _stereo_dispatch(1), _stereo_dispatch(2)), 'stein': (stein_inputs, stein_want, stein_judge), 'spd': (spd_inputs, spd_want, spd_judge), 'product': (product_inputs, product_want, product_judge), 'sne': (sne_inputs, sne_want, sne_judge), 'sst': (sst_inputs, sst_want, sst_judge), 'vec': (vec_inputs, vec_want, vec_judge), 'so': (mat_inputs, mat_want, mat_judge), 'grass': (mat_inputs, mat_want, mat_judge)}


def inputs(row, which):
    return FAMILIES[row['family']][0](row, which)


def want(row, which):
    """{quantity: fp64 array} of the oracle; computed once per case, never modified"""
    return FAMILIES[row['family']][1](row, which)


def judge(row, which, got, e_old=None):
    """{quantity: (error, bound)} of `got` ({quantity: fp64 array}) under the family module's own rule (`e_old`: Stein rows)"""
    if row['family'] == 'stein':
        return stein_judge(row, which, got, e_old)
    return FAMILIES[row['family']][2](row, which, got)


def replay_allowance(row, which, e_eager):
    """{quantity: 2 e_eager + 64 eps max|oracle|}: grass_cases.check's rule for reordered atomic sums"""
    w = want(row, which)
    return {q: 2 * e_eager[q] + 64 * EPS[row['dname']] * (float(np.abs(w[q]).max()) if w[q].size else 0.0) for q in e_eager}


def deviations(row, which, got):
    """{quantity: max |got - oracle|} over the quantities the family's rule compares"""
    w = want(row, which)
    out = {}
    for q in w if row['family'] == 'stein' else judge(row, which, got):
        g = np.asarray(got[q], np.float64).reshape(-1)
        out[q] = float(np.abs(g - w[q].reshape(-1)).max()) if np.isfinite(g).all() else float('inf')
    return out


@functools.lru_cache(maxsize=None)
def _rows():
    return tuple(_vec_rows() + _mat_rows() + _kl_rows('sne', Q_SNE_WS) + _kl_rows('sst', Q_SST_WS) + _product_rows() + _spd_rows() + _stein_rows() + _stereo_rows() + _stereo_product_rows())


ROWS = _rows()
BY_ID = {r['id']: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
GROUPS = sorted({(r['family'], r['dname']) for r in ROWS})
