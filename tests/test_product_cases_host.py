"""The table of tests/product_cases.py, checked on the CPU: the host model of the dispatch reaches exactly the pair-kernel
instantiations the built library holds (closure), and the oracle values the device test compares against can tell one
instantiation from another (every factor contributes, exchanged kinds move the loss, shards partition the whole, no pair
sits on a kink of the quotient loss).  No GPU."""
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import product_cases as pc  # noqa: E402
import step_cases as sc  # noqa: E402
from oracle import step as ostep  # noqa: E402

LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'

# Instantiations no case reaches, by name, each with its reason.  The only ones: PW = 16 without a vector factor — the padded
# width follows the widest vector factor, so an SPD-only product takes PW = 8; the A/B switch MM_PRODUCT_PW16=1 ("always 16
# wide") alone launches these, and the A/B switches are not exercised.
_WHY = 'PW = 16 with NV = 0: reachable only through the A/B switch MM_PRODUCT_PW16'
EXEMPT = {
    'product_pair_kernel<float, 0, 2, 1, 16, false, -1>': _WHY,
    'product_pair_kernel<float, 0, 2, 1, 16, true, -1>': _WHY,
    'product_pair_kernel<float, 0, 2, 2, 16, false, -1>': _WHY,
    'product_pair_kernel<float, 0, 2, 2, 16, true, -1>': _WHY,
    'product_pair_kernel<float, 0, 3, 1, 16, false, -1>': _WHY,
    'product_pair_kernel<float, 0, 3, 1, 16, true, -1>': _WHY,
    'product_pair_kernel<float, 0, 3, 2, 16, false, -1>': _WHY,
    'product_pair_kernel<float, 0, 3, 2, 16, true, -1>': _WHY,
    'product_pair_kernel<double, 0, 2, 1, 16, false, -1>': _WHY,
    'product_pair_kernel<double, 0, 2, 1, 16, true, -1>': _WHY,
    'product_pair_kernel<double, 0, 2, 2, 16, false, -1>': _WHY,
    'product_pair_kernel<double, 0, 2, 2, 16, true, -1>': _WHY,
    'product_pair_kernel<double, 0, 3, 1, 16, false, -1>': _WHY,
    'product_pair_kernel<double, 0, 3, 1, 16, true, -1>': _WHY,
    'product_pair_kernel<double, 0, 3, 2, 16, false, -1>': _WHY,
    'product_pair_kernel<double, 0, 3, 2, 16, true, -1>': _WHY,
}

WHOLE = [c for c in pc.CASES if c['n'] == pc.N and c['rows'] is None]      # the n = 131 cases over every pair, minibatches too
TWO = [c for c in WHOLE if c['nv'] == 2 and not c['batch'] and not c['tdraw']]


def reached():
    """{kernel name: [(environment, case id), ...]} over the table and the device test's environments"""
    out = {}
    for env in pc.ENVS:
        for c in pc.cases_for(env):
            out.setdefault(pc.name(pc.route_of(c, env)), []).append((pc.env_id(env), c['id']))
    return out


# --------------------------------------------------------------------------------------------------------------------- closure
@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_the_table_reaches_every_pair_kernel_in_the_library():
    import kernel_meta
    if not os.path.exists(kernel_meta.LIB):
        pytest.skip('library not built')
    lib = {nm for nm in kernel_meta.kernels() if nm.startswith(('product_pair_kernel<', 'product_sym_kernel<'))}
    got = reached()
    print(f'{len(lib)} pair-kernel instantiations in the library: '
          f'{sum(nm.startswith("product_pair_kernel<") for nm in lib)} ordered, {sum(nm.startswith("product_sym_kernel<") for nm in lib)} '
          f'symmetric; {len(got)} reached by {len(pc.CASES)} cases, {len(EXEMPT)} exempt')
    missing = sorted(set(got) - lib)
    assert not missing, f'cases routed to kernels the library lacks: {[(nm, got[nm][0]) for nm in missing[:10]]}'
    stale = sorted(set(EXEMPT) - lib)
    assert not stale, f'exempt names the library does not hold: {stale}'
    both = sorted(set(EXEMPT) & set(got))
    assert not both, f'exempt AND reached: {both}'
    unreached = sorted(lib - set(got) - set(EXEMPT))
    assert not unreached, f'{len(unreached)} instantiations no case reaches: {unreached[:20]}'


def test_route_model_on_the_known_instantiations():
    """The two routes the suite names elsewhere (tests/test_kernel_budget.py), the thresholds and the switches."""
    r = lambda *a: pc.name(pc.route(*a))      # noqa: E731
    assert r('f32', sc.CSPHD, 1025, 'quotient', False, {}) == 'product_pair_kernel<float, 2, 2, 2, 8, false, 9>'
    assert r('f32', sc.CSPHD, 512, 'stress', True, {}) == 'product_pair_kernel<float, 2, 2, 1, 8, true, 9>'
    assert r('f64', sc.FOUR, 131, 'stress', False, {}) == 'product_pair_kernel<double, 3, 3, 1, 8, false, -1>'
    assert r('f32', sc.CSPHD, 1536, 'stress', False, {}) == 'product_sym_kernel<float, 2, 2, 1, 9>'
    assert r('f32', sc.CSPHD, 1535, 'stress', False, {}).startswith('product_pair_kernel<')
    assert r('f64', sc.CSPHD, 640, 'stress', False, {}) == 'product_sym_kernel<double, 2, 2, 1, 9>'
    assert r('f64', sc.CSPHD, 639, 'stress', False, {}).startswith('product_pair_kernel<')
    assert r('f64', sc.CSPHD, 5000, 'stress', True, {}).startswith('product_pair_kernel<')          # minibatches: ordered
    assert r('f32', sc.CSPHD, 5000, 'stress', False, {'MM_PRODUCT_ORDERED': '1', 'MM_PRODUCT_SYM': '1'}).startswith('product_pair_')
    assert r('f32', sc.CSPHD, 131, 'stress', False, {'MM_PRODUCT_SYM': '1'}) == 'product_sym_kernel<float, 2, 2, 1, 9>'
    assert r('f32', sc.CSPHD, 131, 'stress', False, {'MM_PRODUCT_SYM': '1', 'MM_PRODUCT_RT_KINDS': '1'}) == 'product_sym_kernel<float, 2, 2, 1, -1>'
    assert r('f32', sc.CSPHD, 131, 'stress', False, {'MM_PRODUCT_RT_KINDS': '1'}) == 'product_pair_kernel<float, 2, 2, 1, 8, false, -1>'
    # kind codes: two bits per vector factor in list order, the SPD factor skipped wherever it stands
    assert r('f32', [('sphere', 3), ('spd', 2), ('lorentz', 4)], 131, 'stress', False, {}) == 'product_pair_kernel<float, 2, 2, 1, 8, false, 6>'
    assert r('f32', [('lorentz', 4), ('sphere', 3)], 131, 'stress', False, {}) == 'product_pair_kernel<float, 2, 0, 1, 8, false, 9>'
    # widths: 8 is the last PW = 8, 9 the first PW = 16 (run-time kinds); the symmetric form takes 8 (Euclidean: 7)
    assert r('f32', [('lorentz', 8)], 131, 'stress', False, {}) == 'product_pair_kernel<float, 1, 0, 1, 8, false, 1>'
    assert r('f32', [('lorentz', 9)], 131, 'stress', False, {}) == 'product_pair_kernel<float, 1, 0, 1, 16, false, -1>'
    sym = {'MM_PRODUCT_SYM': '1'}
    assert r('f32', [('lorentz', 8)], 131, 'stress', False, sym) == 'product_sym_kernel<float, 1, 0, 1, 1>'
    assert r('f32', [('euclidean', 7)], 131, 'stress', False, sym) == 'product_sym_kernel<float, 1, 0, 1, 0>'
    assert r('f32', [('euclidean', 8)], 131, 'stress', False, sym) == 'product_pair_kernel<float, 1, 0, 1, 8, false, 0>'
    assert r('f32', [('lorentz', 9)], 131, 'stress', False, sym) == 'product_pair_kernel<float, 1, 0, 1, 16, false, -1>'


def test_the_table_is_built_as_described():
    for lay in pc.LAYOUTS:
        widths = [d for k, d in lay['factors'] if k != 'spd']
        assert len(set(widths)) == len(widths), lay                      # every vector factor has a width of its own
    met = {(k, d) for lay in pc.LAYOUTS for k, d in lay['factors']}
    assert {('sphere', 8), ('lorentz', 8), ('euclidean', 7), ('euclidean', 8), ('euclidean', 1)} <= met
    assert {9, 16} <= {d for k, d in met if k != 'spd'}
    for sd in (2, 3):      # the SPD factor first, in the middle, last
        where = {(lay['factors'].index(('spd', sd)), len(lay['factors'])) for lay in pc.LAYOUTS if lay['sd'] == sd and lay['nv'] >= 2}
        assert {p == 0 for p, k in where} == {True, False} and any(0 < p < k - 1 for p, k in where) and any(p == k - 1 for p, k in where)
    for c in pc.CASES:
        k = len(c['factors'])
        assert pc.scales_of(c) == [float(np.float32(v)) for v in ([0.5] if k == 1 else [0.5, 0.3, 0.7, 0.4][:k])]
    # per (NV, SD, dtype) one kind code runs the sizes; Euclidean 8 falls to the ordered kernel under MM_PRODUCT_SYM=1
    groups = {(c['nv'], c['sd'], c['dname']) for c in pc.CASES}
    assert len(groups) == 22
    for nv, sd, dn in groups:
        mine = [c for c in pc.CASES if (c['nv'], c['sd'], c['dname']) == (nv, sd, dn) and c['primary']]
        assert len({c['factors'] for c in mine}) == 1
        for loss in ('stress', 'quotient'):
            some = [c for c in mine if c['loss'].startswith(loss)]
            assert {c['n'] for c in some} == {2, 65, pc.N}
            assert {c['rows'] for c in some} == set(pc.shards(pc.N) + pc.RANGES + [None])
    assert {c['loss'] for c in pc.CASES} == {'stress', 'quotient', 'quotient_l1', 'quotient_l2'}
    assert {c['epoch'] for c in pc.CASES if c['loss'] != 'stress'} == {0, 2}
    assert {c['batch'] for c in pc.CASES} == {None, 131, 65}
    assert {c['factors'][0][0] for c in pc.CASES if c['init'] == 'rand'} == {'spd', 'euclidean', 'lorentz', 'sphere'}
    for c in pc.CASES:
        if any(f == ('euclidean', 8) for f in c['factors']) and not c['batch']:
            assert pc.route_of(c, {'MM_PRODUCT_SYM': '1'})[0] == 'pair'


# ----------------------------------------------------------------------------------------------------------------- the oracle
def test_the_oracle_of_every_case_is_finite():
    for c in pc.CASES:
        value, grads, sgrads = pc.expected(c)
        assert np.isfinite(value) and all(np.isfinite(g).all() for g in grads) and np.isfinite(sgrads).all(), c['id']
        lo, hi = (0, 1) if c['batch'] else pc.pair_slice(c)
        if hi > lo:
            assert value > 0 and all(np.abs(g).max() > 0 for g in grads), c['id']
        else:
            assert value == 0 and not any(g.any() for g in grads) and not any(sgrads), c['id']


def test_every_factor_contributes():
    """A dropped factor moves md and every gradient weight by its share: above 1 % everywhere, against tolerances of 2e-5 ..
    3e-4."""
    low = []
    for c in WHOLE:
        for f, (of_md, of_grad) in zip(c['factors'], pc.shares(c)):
            if not (of_md > 0.01 and of_grad > 0.01):
                low.append((c['id'], f, of_md, of_grad))
    assert not low, low[:10]


def test_exchanged_kinds_move_the_loss():
    """Two vector factors of different kinds: evaluating each with the other's kind — what a transposed kind code does — moves
    the loss by more than 100 x the fp32 tolerance.  (Two factors of the same kind have a symmetric code: nothing to exchange.)"""
    seen = 0
    for c in TWO:
        a, b = [k for k, _ in c['factors'] if k != 'spd']
        if a == b:
            continue
        inp = pc.inputs(c)
        value, _, _ = pc.expected(c)
        other, _, _ = ostep.objective(pc.swapped_kinds(c), list(inp['xs']), inp['scales'], pc.loss_of(c), target=inp['target'])
        assert abs(other - value) > 100 * pc.TOL['loss']['f32'] * abs(value), (c['id'], value, other)
        seen += 1
    assert seen == 2 * 2 * (6 * 3 + 4)       # 6 mixed codes x 3 SD + the mixed wide / Euclidean-8 layouts, x dtype x loss


# ------------------------------------------------------------------------------------------------------------ shards and kinks
def test_row_shards_partition_the_whole():
    n = pc.N
    rows = pc.shards(n)
    assert rows[0][0] == 0 and rows[-1][1] == n and all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(a < b for a, b in rows)
    for c in pc.CASES:
        if not (c['primary'] and c['rows'] == rows[0]):
            continue
        whole = pc.whole_of(c)
        parts = [pc.BY_ID[pc.case(c['factors'], c['dname'], c['loss'], c['epoch'], rows=r)['id']] for r in rows]
        i, j = pc.inputs(whole)['pairs']
        pi = np.concatenate([pc.inputs(p)['pairs'][0] for p in parts])
        pj = np.concatenate([pc.inputs(p)['pairs'][1] for p in parts])
        assert np.array_equal(pi, i) and np.array_equal(pj, j)
        assert np.array_equal(np.concatenate([pc.inputs(p)['target'] for p in parts]), pc.inputs(whole)['target'])
        value, grads, sgrads = pc.expected(whole)
        assert abs(sum(pc.expected(p)[0] for p in parts) - value) <= 1e-12 * abs(value)
        for k in range(len(grads)):
            assert np.abs(sum(pc.expected(p)[1][k] for p in parts) - grads[k]).max() <= 1e-12 * np.abs(grads[k]).max()
            assert abs(sum(pc.expected(p)[2][k] for p in parts) - sgrads[k]) <= 1e-12 * max(abs(sgrads[k]), 1e-3 * abs(value))
    for rb, re in pc.RANGES:
        c = next(c for c in pc.CASES if c['rows'] == (rb, re))
        i, j = pc.inputs(c)['pairs']
        assert i.size == sum(n - 1 - r for r in range(rb, re)) and (i.size == 0 or (i.min() == rb and i.max() == re - 1 and (j > i).all()))


def test_no_pair_sits_on_a_kink_and_few_targets_moved():
    moved = {}
    for c in pc.CASES:
        inp = pc.inputs(c)
        if c['loss'] == 'stress':
            assert inp['moved'] == 0
            continue
        kd = pc.kink_distances(c)
        assert kd.size == inp['pairs'][0].size                      # no pair is left out
        assert not (kd < sc.KINK_MARGIN).any(), c['id']
        share = inp['moved'] / inp['npairs_whole']
        assert share <= pc.MAX_MOVED_SHARE, (c['id'], inp['moved'])
        moved[c['id']] = inp['moved']
    print(f'targets moved off a kink: {sum(1 for v in moved.values() if v)} of {len(moved)} quotient cases, at most {max(moved.values())} '
          f'per case')
    for cid, m in sorted(moved.items()):
        if m:
            print(f'  {cid}: {m}')
