"""The table of tests/vec_cases.py, checked on the CPU: the host model of the dispatch reaches exactly the vector pair-kernel
instantiations the built library holds (closure), the model says what the dispatch code says at the thresholds and under the
switches, and the oracle values the device test compares against can tell one instantiation from another (a dropped
coordinate, another kind, a flipped Lorentz time sign, the other loss, the other `squared` each move the expected result by more
than ten times the bound; shards partition the whole; no pair sits on a kink of the quotient loss; the fp32 plain backward masks
at most a tenth of a case's pairs).  No GPU."""
import collections
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import step_cases as sc  # noqa: E402
import vec_cases as vc  # noqa: E402

LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
PREFIXES = ('vec_pdist_', 'vec_gram_', 'vec_sym_prep_kernel')

# Instantiations no case reaches through the C ABI, by full name, each with its reason.
EXEMPT = {}

WHOLE = [c for c in vc.CASES if c['n'] == vc.N and c['rows'] is None and not c['refuse']]      # (minibatches of every size too)


def reached():
    """{kernel name: [(environment, case id), ...]} over the table and the device test's environments"""
    out = {}
    for env in vc.ENVS:
        for c in vc.cases_for(env):
            for nm in vc.route_of(c, env):
                out.setdefault(nm, []).append((vc.env_id(env), c['id']))
    return out


# --------------------------------------------------------------------------------------------------------------------- closure
@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_the_table_reaches_every_vector_pair_kernel_in_the_library():
    import kernel_meta
    if not os.path.exists(kernel_meta.LIB):
        pytest.skip('library not built')
    lib = {nm for nm in kernel_meta.kernels() if nm.startswith(PREFIXES)}
    got = reached()
    per = collections.Counter(nm.split('<')[0] for nm in lib)
    print(f'{len(lib)} vector pair-kernel instantiations in the library; {len(got)} reached by {len(vc.CASES)} cases in '
          f'{len(vc.ENVS)} environments, {len(EXEMPT)} exempt')
    for nm, cnt in sorted(per.items()):
        print(f'  {cnt:4d}  {nm}')
    missing = sorted(set(got) - lib)
    assert not missing, f'cases routed to kernels the library lacks: {[(nm, got[nm][0]) for nm in missing[:10]]}'
    stale = sorted(set(EXEMPT) - lib)
    assert not stale, f'exempt names the library does not hold: {stale}'
    both = sorted(set(EXEMPT) & set(got))
    assert not both, f'exempt AND reached: {both}'
    unreached = sorted(lib - set(got) - set(EXEMPT))
    assert not unreached, f'{len(unreached)} instantiations no case reaches: {unreached[:20]}'


def test_route_model_on_the_known_instantiations():
    """The thresholds, each switch, and the k-step classes at odd widths, spelled out."""
    r = vc.route
    sym = lambda t, k, mp, loss, sq: [f'vec_sym_prep_kernel<{t}, {mp}>', f'vec_pdist_bwd_sym_kernel<{t}, {k}, {mp}, {loss}, {sq}>']      # noqa: E731
    ordered = lambda t, k, mp, loss: [f'vec_pdist_bwd_kernel<{t}, {k}, {mp}, 64, {loss}, false>', f'vec_pdist_finalize_kernel<{t}, {k}, {mp}>']      # noqa: E731
    # forward: the padded width alone
    assert r('fwd', 'f32', 'lorentz', 11, 131, None, True, None, {}) == ['vec_pdist_fwd_kernel<float, 1, 12>']
    assert r('fwd', 'f64', 'euclidean', 1, 131, None, False, None, {}) == ['vec_pdist_fwd_kernel<double, 0, 4>']
    assert r('fwd', 'f64', 'sphere', 49, 131, None, True, None, {}) == ['vec_pdist_fwd_kernel<double, 2, 64>']
    assert r('fwd_gram', 'f32', 'lorentz', 11, 131, None, True, None, {}) == ['vec_gram_fwd_f32_kernel<1, 6>']
    assert r('fwd_gram', 'f64', 'sphere', 64, 131, None, True, None, {}) == ['vec_gram_fwd_f64_kernel<2>']
    # the fused loss, m = 16 / 17 in fp32: the symmetric VALU form, then the matrix cores
    assert r('loss', 'f32', 'lorentz', 16, 131, 'stress', True, None, {}) == sym('float', 1, 16, 1, 'true')
    assert r('loss', 'f32', 'lorentz', 17, 131, 'stress', True, None, {}) == ['vec_gram_bwd_sym_f32_kernel<1, 12, 1>']
    assert r('loss', 'f32', 'lorentz', 17, 32769, 'stress', True, None, {}) == sym('float', 1, 24, 1, 'true')      # n <= 32768
    assert r('loss', 'f32', 'lorentz', 17, 32768, 'quotient_l2', True, None, {}) == ['vec_gram_bwd_sym_f32_kernel<1, 12, 2>']
    assert r('loss', 'f32', 'euclidean', 17, 131, 'stress', True, None, {}) == sym('float', 0, 24, 1, 'true')
    # fp64: Lorentz / sphere leave the symmetric form after 16, the Euclidean factor after 32
    assert r('loss', 'f64', 'lorentz', 16, 131, 'quotient', True, None, {}) == sym('double', 1, 16, 2, 'true')
    assert r('loss', 'f64', 'lorentz', 17, 131, 'quotient', True, None, {}) == ordered('double', 1, 24, 2)
    assert r('loss', 'f64', 'euclidean', 32, 131, 'stress', True, None, {}) == sym('double', 0, 32, 1, 'true')
    assert r('loss', 'f64', 'euclidean', 33, 131, 'stress', True, None, {}) == ordered('double', 0, 48, 1)
    assert r('bwd', 'f32', 'sphere', 32, 131, None, False, None, {}) == sym('float', 2, 32, 0, 'false')
    assert r('bwd', 'f32', 'sphere', 33, 131, None, False, None, {}) == ordered('float', 2, 48, 0)
    # each switch
    assert r('bwd', 'f32', 'sphere', 6, 131, None, True, None, {'MM_VEC_BWD_ORDERED': '1'}) == ordered('float', 2, 8, 0)
    assert r('loss', 'f64', 'lorentz', 11, 131, 'stress', True, None, {'MM_VEC_LOSS_GRAM': '1'}) == ['vec_gram_bwd_f64_kernel<1, 3, 1>']
    assert r('loss', 'f32', 'lorentz', 11, 131, 'stress', True, None, {'MM_VEC_LOSS_GRAM': '1'}) == ['vec_gram_bwd_sym_f32_kernel<1, 6, 1>']
    assert r('loss', 'f32', 'lorentz', 24, 131, 'stress', True, None, {'MM_VEC_LOSS_VALU': '1'}) == sym('float', 1, 24, 1, 'true')
    assert r('loss', 'f32', 'lorentz', 24, 131, 'stress', True, None, {'MM_VEC_BWD_ORDERED': '1'}) == ['vec_gram_bwd_sym_f32_kernel<1, 12, 1>']
    assert r('loss', 'f32', 'lorentz', 24, 131, 'stress', True, None, {'MM_VEC_BWD_ORDERED': '1', 'MM_VEC_LOSS_VALU': '1'}) == ordered('float', 1, 24, 1)
    assert r('loss', 'f32', 'lorentz', 24, 131, 'stress', True, None, {'MM_GRAM_BWD_ORDERED': '1'}) == ['vec_gram_bwd_f32_kernel<1, 12, 1>']
    assert r('bwd_gram', 'f32', 'euclidean', 31, 131, None, True, None, {}) == ['vec_gram_bwd_f32_kernel<0, 2, 0>']
    assert r('bwd_gram', 'f32', 'euclidean', 31, 131, None, True, None, {'MM_GRAM_BWD_ORDERED': '0'}) == ['vec_gram_bwd_sym_f32_kernel<0, 2, 0>']
    assert r('bwd_gram', 'f32', 'euclidean', 32, 131, None, True, None, {}) == []                     # refused
    assert r('bwd_gram', 'f32', 'sphere', 6, 131, None, False, None, {'MM_GRAM_BWD_ORDERED': '1'}) == ['vec_gram_bwd_f32_kernel<2, 4, 0>']
    assert r('subset', 'f32', 'lorentz', 11, 70, 'quotient', True, 70, {'MM_VEC_BWD_ORDERED': '1', 'MM_VEC_LOSS_GRAM': '1'}) == \
        ['vec_pdist_bwd_kernel<float, 1, 12, 8, 2, true>', 'vec_pdist_finalize_kernel<float, 1, 12>']      # minibatches: one form
    assert vc.subset_rows({}) == 16 and vc.subset_rows({'MM_VEC_SUBSET_ROWS': '64'}) == 64 and vc.subset_rows({'MM_VEC_SUBSET_ROWS': '100'}) == 64
    # the k-step classes: ceil(m / 2) rounded to 2 4 6 8 12 16 (fp32), ceil(m / 4) (fp64); an odd width pads half a step
    assert [vc.ks32(m) for m in (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)] == [2, 2, 2, 4, 4, 6, 6, 8, 8, 12, 12, 16, 16]
    assert [vc.ks64(m) for m in (2, 4, 5, 8, 9, 12, 13, 16)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [vc.pad_dim(m) for m in (1, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64)] == \
        [4, 4, 8, 8, 12, 12, 16, 16, 24, 24, 32, 32, 48, 48, 64, 64]
    assert r('bwd_gram', 'f64', 'lorentz', 13, 131, None, True, None, {}) == ['vec_gram_bwd_f64_kernel<1, 4, 0>']
    assert r('bwd_gram', 'f32', 'lorentz', 13, 131, None, True, None, {}) == ['vec_gram_bwd_sym_f32_kernel<1, 8, 0>']
    # the forward's row-tile height on 256 CUs
    assert [vc.fwd_tile_height(n, 0, n, 256) for n in (vc.N, ) + vc.FWD_HEIGHT_N] == [2, 4, 8, 16, 32]
    assert vc.fwd_tile_height(131, 5, 5, 256) is None and vc.fwd_tile_height(3100, 0, 3100, 64) == 32


def test_the_table_is_built_as_described():
    by = collections.defaultdict(set)
    for c in WHOLE:
        by[(c['entry'], c['kind'], c['dname'])].add(c['m'])
    lo = {'euclidean': 1, 'lorentz': 2, 'sphere': 2}
    for kind in vc.KINDS:
        widths = {m for m in vc.WIDTHS if m >= lo[kind]}
        for dname in ('f32', 'f64'):
            for entry in ('fwd', 'bwd', 'loss', 'subset'):
                assert by[(entry, kind, dname)] >= widths, (entry, kind, dname)
        if kind != 'euclidean':
            assert by[('bwd_gram', kind, 'f32')] >= {2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32}
            assert by[('bwd_gram', kind, 'f64')] >= {4, 5, 8, 9, 12, 13, 16} and max(by[('bwd_gram', kind, 'f64')]) == 16
            assert by[('fwd_gram', kind, 'f32')] >= {3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32}
            assert by[('fwd_gram', kind, 'f64')] >= widths
    assert 31 in by[('bwd_gram', 'euclidean', 'f32')] and not by[('bwd_gram', 'euclidean', 'f64')]
    assert {c['loss'] for c in vc.CASES} == {None, 'stress', 'quotient', 'quotient_l1', 'quotient_l2'}
    # every form meets each of the quotient's term selections and scale_raw = NULL
    seen = collections.defaultdict(set)
    for env in vc.ENVS:
        for c in vc.cases_for(env):
            if c['loss'] and not c['refuse']:
                form = (vc.form_of(vc.route_of(c, env)), c['dname'])
                seen[form].add(c['loss'])
                if not c['scale']:
                    seen[form].add('noscale')
    assert set(seen) == {(f, d) for d in ('f32', 'f64') for f in ('sym', 'ordered', 'subset')} | {('gram_sym', 'f32'), ('gram_ordered', 'f32'), ('gram_f64', 'f64')}
    for form, what in seen.items():
        assert what == {'stress', 'quotient', 'quotient_l1', 'quotient_l2', 'noscale'}, (form, what)
    # the sizes, ranges and batches: per (entry, kind, dtype) at the kind's primary width
    for c in vc.CASES:
        if not (c['primary'] and c['n'] == vc.N and c['rows'] is None and c['scale']) or c['batch']:
            continue
        mine = [d for d in vc.CASES if (d['entry'], d['kind'], d['m'], d['dname'], d['squared'], d['loss']) ==
                (c['entry'], c['kind'], c['m'], c['dname'], c['squared'], c['loss'])]
        assert {d['n'] for d in mine} >= {2, 65, vc.N, 257}, c['id']
        assert {d['rows'] for d in mine} == set(vc.shards(vc.N) + vc.RANGES + [None]), c['id']
    assert {c['batch'] for c in vc.CASES if c['entry'] == 'subset' and not c['refuse']} == set(vc.BATCHES)
    assert all(sorted(vc.batch_idx(k, vc.PRIMARY[k], 'f32', 70)) != list(vc.batch_idx(k, vc.PRIMARY[k], 'f32', 70)) for k in vc.KINDS)
    # one case per refusal; under a switch only what it changes, plus the control
    assert sum(c['refuse'] for c in vc.CASES) == 14
    for env in vc.ENVS[1:]:
        some = vc.cases_for(env)
        assert some[-1] is vc.CONTROL and len(some) > 1 and all(vc.variant(c, env) != vc.variant(c, {}) for c in some[:-1]), env


# ----------------------------------------------------------------------------------------------------------------- the oracle
def test_the_oracle_of_every_case_is_finite():
    for c in vc.CASES:
        if c['refuse']:
            continue
        want = vc.expected(c)
        npairs = vc.inputs(c)['pairs'][0].size
        if c['entry'] in ('fwd', 'fwd_gram'):
            assert want.shape == (npairs, ) and np.isfinite(want).all() and (want > 0).all(), c['id']
            continue
        value, grad, sgrad = want if c['loss'] else (1.0 if npairs else 0.0, want, 0.0)
        assert np.isfinite(value) and np.isfinite(grad).all() and np.isfinite(sgrad), c['id']
        if npairs:
            assert value > 0 and np.abs(grad).max() > 0, c['id']
        else:
            assert value == 0 and not grad.any() and sgrad == 0, c['id']


def _moved(c, want, other):
    """err / allowed per quantity of `other` held against `want` under the case's own bound"""
    return vc.worst(vc.errors(c, want, other))


def _lorentz_time_flipped(c, want):
    """What a kernel with the time sign of the Minkowski product flipped returns: q = +<x, y> in place of -<x, y>_L in the
    value (acosh of a clamped q: the distance collapses), and coordinate 0 of the gradient with the other sign."""
    if c['entry'] in ('fwd', 'fwd_gram'):
        inp = vc.inputs(c)
        i, j = inp['pairs']
        q = -(inp['x'][i, 0] * inp['x'][j, 0]) + (inp['x'][i, 1:] * inp['x'][j, 1:]).sum(1)
        d = np.arccosh(np.maximum(q, 1.0))
        return d * d if c['squared'] else d
    flip = np.ones(c['m'])
    flip[0] = -1
    return (want[0], want[1] * flip, want[2]) if c['loss'] else want * flip


def test_the_oracle_tells_instantiations_apart():
    """Per (entry, kind, dtype), at the full width of every class it has: each mistake moves what the device is compared with
    by more than 10 x the bound of that comparison, in at least one quantity."""
    weak, seen = [], collections.Counter()
    for c in WHOLE:
        if c['m'] != vc.pad_dim(c['m']) or (c['batch'] and c['batch'] != vc.BATCHES[-1]) or not c['scale']:
            continue
        want = vc.expected(c)
        x = vc.inputs(c)['x']
        mistakes = {}
        dropped = vc.evaluate(c, x=x[:, :-1])                                        # a padding / width mistake
        if c['entry'] in ('fwd', 'fwd_gram'):
            mistakes['last coordinate dropped'] = dropped
        elif c['loss']:
            mistakes['last coordinate dropped'] = (dropped[0], np.pad(dropped[1][0], ((0, 0), (0, 1))), dropped[2][0])
        else:
            mistakes['last coordinate dropped'] = np.pad(dropped, ((0, 0), (0, 1)))
        for kind in vc.KINDS:
            if kind != c['kind']:
                other = vc.evaluate(c, kind=kind)
                mistakes[f'evaluated as {kind}'] = (other[0], other[1][0], other[2][0]) if c['loss'] else other
        if c['kind'] == 'lorentz':
            mistakes['time sign flipped'] = _lorentz_time_flipped(c, want)
        if c['loss']:
            other = vc.evaluate(c, loss='quotient' if c['loss'] == 'stress' else 'stress')
            mistakes['the other loss'] = (other[0], other[1][0], other[2][0])
        else:
            mistakes['the other squared'] = vc.evaluate(c, squared=not c['squared'])
        for what, other in mistakes.items():
            ratios = _moved(c, want, other)
            seen[what.split(' as ')[0]] += 1
            if not max(ratios.values()) > 10:
                weak.append((c['id'], what, ratios))
    print(dict(seen))
    assert not weak, weak[:10]
    assert seen['last coordinate dropped'] > 300 and seen['time sign flipped'] > 100


# ------------------------------------------------------------------------------------------------------------ shards and kinks
def test_row_shards_partition_the_whole():
    n = vc.N
    rows = vc.shards(n)
    assert rows[0][0] == 0 and rows[-1][1] == n and all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(a < b for a, b in rows)
    count = 0
    for c in vc.CASES:
        if not (c['primary'] and c['n'] == n and c['rows'] is None and c['scale']) or c['batch']:
            continue
        parts = vc.parts_of(c)
        i, j = vc.inputs(c)['pairs']
        assert np.array_equal(np.concatenate([vc.inputs(p)['pairs'][0] for p in parts]), i)
        assert np.array_equal(np.concatenate([vc.inputs(p)['pairs'][1] for p in parts]), j)
        want = vc.expected(c)
        if c['entry'] in ('fwd', 'fwd_gram'):
            assert np.array_equal(np.concatenate([vc.expected(p) for p in parts]), want)
        elif c['loss']:
            assert np.array_equal(np.concatenate([vc.inputs(p)['target'] for p in parts]), vc.inputs(c)['target'])
            assert abs(sum(vc.expected(p)[0] for p in parts) - want[0]) <= 1e-12 * abs(want[0])
            assert np.abs(sum(vc.expected(p)[1] for p in parts) - want[1]).max() <= 1e-12 * np.abs(want[1]).max()
            assert abs(sum(vc.expected(p)[2] for p in parts) - want[2]) <= 1e-12 * max(abs(want[2]), 1e-3 * abs(want[0]))
        else:
            assert np.array_equal(np.concatenate([vc.inputs(p)['g'] for p in parts]), vc.inputs(c)['g'])
            assert np.abs(sum(vc.expected(p) for p in parts) - want).max() <= 1e-12 * np.abs(want).max()
        count += 1
    # per dtype, two settings each: fwd bwd loss x 3 kinds, fwd_gram bwd_gram x 2 kinds; + the fp32 squared Euclidean bwd_gram
    assert count == 2 * 2 * (3 * 3 + 2 * 2) + 1
    for rb, re in vc.RANGES:
        c = next(c for c in vc.CASES if c['rows'] == (rb, re))
        i, j = vc.inputs(c)['pairs']
        assert i.size == sum(n - 1 - r for r in range(rb, re)) and (i.size == 0 or (i.min() == rb and i.max() == re - 1 and (j > i).all()))


def test_no_pair_sits_on_a_kink_and_few_targets_moved():
    moved = {}
    for c in vc.CASES:
        if not c['loss'] or c['refuse']:
            continue
        inp = vc.inputs(c)
        if c['loss'] == 'stress':
            assert inp['moved'] == 0
            continue
        kd = vc.kink_distances(c)
        assert kd.size == inp['pairs'][0].size                      # no pair is left out
        assert not (kd < sc.KINK_MARGIN).any(), c['id']
        assert inp['moved'] <= max(1, 0.01 * inp['npairs_whole']), (c['id'], inp['moved'])
        moved[c['id']] = inp['moved']
    print(f'targets moved off a kink: {sum(1 for v in moved.values() if v)} of {len(moved)} quotient cases, at most {max(moved.values())} '
          f'per case')


def test_the_plain_backward_masks_at_most_a_tenth_of_its_pairs():
    """fp32, plain distance: pairs closer than 0.1 get zero upstream weight; no case may lose more than 10 % of its pairs that
    way.  The squared forms and all fp64 cases mask nothing."""
    shares = {}
    for c in vc.CASES:
        if c['entry'] not in ('bwd', 'bwd_gram') or c['refuse']:
            continue
        share = vc.masked_share(c)
        if c['dname'] == 'f64' or c['squared']:
            assert share == 0.0, c['id']
            continue
        assert share <= vc.MAX_MASKED_SHARE, (c['id'], share)
        if c['n'] == vc.N and c['rows'] is None:
            shares[(c['kind'], c['m'])] = share
    top = sorted(shares.items(), key=lambda kv: -kv[1])[:8]
    print('largest masked shares at n = 131: ' + ', '.join(f'{k}({m}) {100 * s:.1f} %' for (k, m), s in top))


def test_every_raised_bound_is_covered_by_the_oracles_own_rounding():
    """vec_cases.RAISED: each entry names a plain or squared backward case, lies above the table and at most 3 x above the
    rounding error of the oracle's own formula in the case's dtype at the case's input."""
    for cid, bounds in vc.RAISED.items():
        c = vc.BY_ID[cid]
        assert set(bounds) == {'grad'} and c['entry'] in ('bwd', 'bwd_gram'), cid
        measured = vc.formula_error(c)
        print(f'{cid}: the formula in {c["dname"]} against long double {measured:.3e} of max|grad|; bound {bounds["grad"]:.3e} '
              f'(table {vc.GREL[c["dname"]]:.1e})')
        assert vc.GREL[c['dname']] < bounds['grad'] <= vc.RAISE_FACTOR * measured, (cid, measured)
