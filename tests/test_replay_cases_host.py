"""The table of tests/replay_cases.py on the CPU: every accumulating entry point of include/mm_manifolds.h is a row or exempt (and
not both), the header lines the rows quote are in the header, A and B of a row share entry, dtype, shape and row range and differ
in their inputs, the large rows clear at least the recorded failure's 51 200 bytes, and the relabelled vector draw's oracle is
vec_cases' own on the draw as it stands.  No GPU."""
import numpy as np
import pytest

import replay_cases as R


def _header():
    with open(R.HEADER) as f:
        return f.read()


def test_every_accumulating_entry_is_a_row_or_exempt():
    entries = R.accumulating_entries()
    assert len(entries) >= 33 and 'mm_vec_pdist_loss_subset' in entries and 'mm_sne_kl_loss' in entries, entries
    assert 'mm_sne_kl_loss' in {r['entry'] for r in R.ROWS}
    assert 'mm_grass_pdist_loss_form' not in entries and 'mm_vec_pdist_fwd' not in entries      # (no stream; no accumulation)
    in_table = {r['entry'] for r in R.ROWS}
    missing = [e for e in entries if e not in in_table and e not in R.EXEMPT]
    assert not missing, f'entries that accumulate and are neither a row of replay_cases.ROWS nor in EXEMPT: {missing}'
    both = sorted(in_table & set(R.EXEMPT))
    assert not both, f'both a row and exempt: {both}'
    unknown = sorted((in_table | set(R.EXEMPT)) - set(entries))
    assert not unknown, f'not an accumulating entry of the header: {unknown}'
    assert all(isinstance(v, str) and len(v) > 10 for v in R.EXEMPT.values())


def test_the_name_rule_on_a_small_header():
    text = '''/* int mm_a_bwd(int x, mm_stream_t stream); a comment is no declaration */
    size_t mm_a_loss_ws_bytes(int dtype);
    int mm_a_fwd(int dtype, mm_stream_t stream);
    int mm_a_bwd_subset(int dtype, const void* x,
                        mm_stream_t stream);
    int mm_b_kl_loss(int dtype, mm_stream_t stream);'''
    assert R.accumulating_entries(text) == ['mm_a_bwd_subset', 'mm_b_kl_loss']


def test_rows_quote_the_header():
    text = _header()
    for r in R.ROWS:
        for name, (contract, quote) in r['buffers'].items():
            assert contract in (R.ANY, R.ZERO), (r['id'], name)
            assert quote in text, (r['id'], name, quote)
        assert r['entry'] in text
        if r['minibatch']:
            what, quote = r['outside']
            assert what == R.PLUS_ZERO and quote in text, (r['id'], quote)


@pytest.mark.parametrize('row', R.ROWS, ids=[r['id'] for r in R.ROWS])
def test_a_and_b_share_the_call_and_differ_in_the_inputs(row):
    g = row['geometry']
    assert g['entry'] == row['entry'] and g['dname'] == row['dname'] and g['rows'] == (0, g['n'])
    a, b = R.inputs(row, 'a'), R.inputs(row, 'b')
    if row['family'] == 'product':
        _product_pair(row, a, b)
        return
    if 'xs' in a:      # products of constant-curvature factors: a list of tables, both draws differ
        assert len(a['xs']) == len(b['xs']) == len(g['ms']) and np.array_equal(a['scales'], b['scales'])
        for p, q, m in zip(a['xs'], b['xs'], g['ms']):
            assert p.shape == q.shape == (g['n_total'], m) and not np.array_equal(p, q) and np.isfinite(p).all() and np.isfinite(q).all()
        assert a['side'].shape == b['side'].shape and not np.array_equal(a['side'], b['side'], equal_nan=True)
        if row['minibatch']:
            assert a['side'].shape == (g['n_total'], g['n_total']) and np.array_equal(a['idx'], b['idx']) and np.unique(a['idx']).size == g['n']
        else:
            assert a['idx'] is None and a['side'].shape == (g['n'] * (g['n'] - 1) // 2, )
        return
    assert a.keys() == b.keys()
    for k in a:      # the same shapes: one set of captured buffers serves both
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (row['id'], k)
    if row['family'] not in ('sne', 'sst'):      # (there the first input is itself a pair vector)
        assert a['x'].shape[0] == g['n_total']
    assert not np.array_equal(a['x'], b['x']), row['id']
    assert np.array_equal(a['side'], b['side']) == bool(row['one_side']), row['id']
    npairs = g['n'] * (g['n'] - 1) // 2
    if row['minibatch']:
        assert a['idx'].shape == (g['n'], ) and np.array_equal(a['idx'], b['idx']) and np.unique(a['idx']).size == g['n']
        if a['side'].ndim == 2:
            assert a['side'].shape == (g['n_total'], g['n_total'])
            i, j = np.triu_indices(g['n'], 1)      # the targets the batch reads differ too
            if not row['one_side']:
                assert not np.array_equal(a['side'][a['idx'][i], a['idx'][j]], b['side'][b['idx'][i], b['idx'][j]])
        else:
            assert a['side'].shape == (npairs, )
    else:
        assert a['idx'] is None and a['side'].shape == (npairs, )
    assert np.isfinite(a['x']).all() and np.isfinite(b['x']).all()


def _product_pair(row, a, b):
    """product rows: lists of factor tables; the module has one draw of the points, so A and B differ in the targets alone"""
    g = row['geometry']
    assert row['same_points'] and len(a['xs']) == len(b['xs']) == len(g['factors'])
    for p, q in zip(a['xs'], b['xs']):
        assert p.shape == q.shape and np.array_equal(p, q) and np.isfinite(p).all()
        assert p.shape[0] == (g['n'] * (g['n'] - 1) // 2 if row['entry'] == 'mm_product_loss' else g['n_total'])
    assert a['side'].shape == b['side'].shape and not np.array_equal(a['side'], b['side'])
    assert np.array_equal(a['scales'], b['scales'])
    if row['minibatch']:
        assert a['side'].shape == (g['n_total'], g['n_total']) and np.array_equal(a['idx'], b['idx']) and np.unique(a['idx']).size == g['n']
        i, j = np.triu_indices(g['n'], 1)
        assert not np.array_equal(a['side'][a['idx'][i], a['idx'][j]], b['side'][b['idx'][i], b['idx'][j]])
    else:
        assert a['idx'] is None and a['side'].shape == (g['n'] * (g['n'] - 1) // 2, )


def test_the_product_oracle_of_an_enumerated_case_is_product_cases_own():
    import product_cases as pc
    for r in R.ROWS:
        if r['family'] != 'product' or r['entry'] == 'mm_product_loss':
            continue
        for which in ('a', 'b'):
            c = R._product_case(r, which)
            if c['id'] not in pc.BY_ID:      # (the minibatch's second target draw: the constructor, not an enumerated case)
                assert r['minibatch'] and which == 'b'
                continue
            mine, (value, grads, sgrads) = R.product_want(r, which), pc.expected(c)
            gk, sk = R._product_keys(c['factors'])
            assert mine['loss'][0] == value
            for k in range(len(gk)):
                assert np.array_equal(mine[gk[k]], grads[k]) and mine[sk[k]][0] == sgrads[k]


def test_large_rows_clear_at_least_the_recorded_failure():
    large = [r for r in R.ROWS if r['cleared']]
    assert {r['entry'] for r in large} == {'mm_vec_pdist_loss_subset', 'mm_vec_pdist_loss_subset_det'}
    for r in large:
        formula, nbytes = r['cleared']
        g = r['geometry']
        print(f"{r['id']}: {formula} = {nbytes} bytes")
        assert nbytes >= R.HAZARD_BYTES, (r['id'], nbytes)
        assert (g['kind'], g['m'], g['n'], g['n_total'], r['dname']) == ('euclidean', 64, 70, 200, 'f32')
    by_entry = {r['entry']: r['cleared'][1] for r in large}
    assert by_entry['mm_vec_pdist_loss_subset_det'] == 200 * 64 * 4 == R.HAZARD_BYTES      # grad_x of the recorded failure
    assert by_entry['mm_vec_pdist_loss_subset'] == 200 * 65 * 4


def test_every_entry_has_one_small_row_per_dtype_and_unrolled_rows_per_family():
    small = {}
    for r in R.ROWS:
        if not r['cleared']:
            small.setdefault(r['entry'], []).append(r['dname'])
    for entry, dnames in small.items():
        assert set(dnames) == {'f32', 'f64'}, (entry, dnames)
    assert {r['family'] for r in R.ROWS if r['unroll']} == {r['family'] for r in R.ROWS}
    for r in R.ROWS:
        assert r['deterministic'] == (r['entry'].endswith('_det') or r['family'] in ('sne', 'sst', 'stereo')), r['id']
        assert r['minibatch'] == ('subset' in r['entry']), r['id']


def test_the_vector_oracle_of_a_is_vec_cases_own():
    """vec_want evaluates oracle.step on the inputs it is handed; on the draw as it stands that is vec_cases.expected, bit for bit
    — so on the relabelled draw it is the same oracle on other inputs"""
    import vec_cases as vc
    import vec_det_cases as vdc
    for r in R.ROWS:
        if r['family'] != 'vec':
            continue
        c = vc.BY_ID[r['a']['id']]
        if r['deterministic']:
            assert c['id'] in vdc.BY_ID and c['id'] not in vdc.REDRAWN
        mine, theirs = R.vec_want(r, 'a'), vc.expected(c)
        if c['loss'] is None:
            assert np.array_equal(mine['grad'], theirs)
        else:
            assert mine['loss'][0] == theirs[0] and np.array_equal(mine['grad'], theirs[1]) and mine['scale_grad'][0] == theirs[2]
        other = R.vec_want(r, 'b')
        assert not np.array_equal(other['grad'], mine['grad'])
        # a relabelling moves no point: the sum of the gradient's magnitudes over the nodes is of the same order
        assert 0.2 < np.abs(other['grad']).max() / np.abs(mine['grad']).max() < 5.0
