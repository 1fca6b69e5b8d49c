"""tests/spd_subset_cases.py on the CPU: the case counts, the kink margins, the oracle against itself (index addressing against
gathered points, shards against the whole) and the TEETH of every case — how far a transposed target matrix, and ONE transposed
target, move the oracle's grad_x.  Nothing here runs a kernel.

Measured (the printed minima, this file, -rA):
    transposing dense   min over the 124 cases with a pair  7.74e-2 S  (threshold TRANSPOSE_MIN = 0.05 S; the one-row shard of D = 6, stress)
    one_pair_effect     min over the same cases            6.06e-4 S  (threshold ONE_PAIR_MIN = 5e-4 S; D = 3, quotient, bs = 257)
    kink_margin         smallest 1.001e-3; at most 80 of a case's pairs nudged
A case that misses a threshold gets another draw of its points (spd_subset_cases.POINT_DRAW), never another threshold."""
import numpy as np
import pytest
import torch

import spd_subset_cases as C

U64 = 2.0**-53


def _with_pairs(cases):
    return [c for c in cases if C.n_pairs(c)]


def test_case_counts():
    for sweep, cases in C.SWEEPS.items():
        assert len(cases()) == C.CASE_COUNTS[sweep] and len(set(cases())) == len(cases()), sweep
    inst = C.instantiation_cases()
    assert {(c.D, c.loss) for c in inst} == {(D, loss) for D in C.DIMS for loss in C.LOSSES}     # x 2 dtypes: the 32 kernels
    assert all({c.regime for c in inst if (c.D, c.loss) == k} == set(C.REGIMES) for k in {(c.D, c.loss) for c in inst})
    assert {c.rows for c in C.shard_cases()} == set(C.SHARDS) and len(C.SHARDS) == 8
    # COVER is a disjoint cover of the batch's rows, and every range of it is a case
    assert C.COVER[0][0] == 0 and C.COVER[-1][1] == C.BS and all(a[1] == b[0] for a, b in zip(C.COVER, C.COVER[1:]))
    assert set(C.COVER) <= set(C.SHARDS)
    assert {C.n_pairs(c) for c in C.shard_cases()} >= {0, 1}                                      # empty and one-pair ranges


def test_inputs():
    for regime in C.REGIMES:
        for D in C.DIMS:
            x = C.points(regime, D)
            assert x.dtype == torch.float32 and x.shape == (C.N_TOTAL, D, D) and torch.equal(x, x.transpose(1, 2))
            assert float(np.linalg.eigvalsh(x.double().numpy()).min()) > 0
    for bs in sorted(set(C.BATCH_SIZES) | {C.BS}):
        idx = C.batch_idx(bs)
        assert idx.numel() == bs and torch.unique(idx).numel() == bs and int(idx.min()) >= 0 and int(idx.max()) < C.N_TOTAL
        assert {0, C.N_TOTAL - 1} <= set(idx.tolist()) and not bool((idx[1:] > idx[:-1]).all())
    a, b = C.batch_idx(C.ABI_BS), C.second_batch()
    assert b.numel() == a.numel() == torch.unique(b).numel() and not set(a.tolist()) & set(b.tolist())
    assert not bool((b[1:] > b[:-1]).all()) and not bool((b[1:] < b[:-1]).all())


def test_dense_targets_and_kink_margins():
    worst, most = np.inf, 0
    for c in C.all_cases():
        dm = C.dense(c.regime, c.D, c.bs)
        assert dm.dtype == torch.float32 and dm.shape == (C.N_TOTAL, C.N_TOTAL) and not torch.equal(dm, dm.T)
        assert float(dm.diagonal().abs().max()) == 0.0
        off = dm[~torch.eye(C.N_TOTAL, dtype=torch.bool)]
        assert float(off.min()) > 0
        km = C.kink_margin(c)
        assert km >= C.MARGIN, (C.case_id(c), km)
        worst, most = min(worst, km), max(most, C.nudged(c))
    for D in C.ABI_DIMS:     # the matrix that serves two disjoint batches: both clear, the first batch's targets untouched
        c = C.Case('mid', D, C.ABI_BS, 'quotient', None)
        both, i, j = C.dense('mid', D, C.ABI_BS, True), *C.batch_pairs(C.batch_idx(C.ABI_BS))
        assert torch.equal(both[i, j], C.dense('mid', D, C.ABI_BS)[i, j])
        assert C.kink_margin(c, dm=both) >= C.MARGIN and C.kink_margin(c, C.second_batch(), both) >= C.MARGIN
    print(f'smallest kink_margin {worst:.3e}, most pairs nudged in one case {most}')


def _close(tag, got, want, S):
    for name, g, w in zip(C.NAMES, got, want):
        err = float((g - w).abs().max())
        assert err <= 64 * U64 * S[name], (tag, name, err, S[name])


def test_index_addressing_equals_gathered_points():
    """the oracle on (x, dense, idx) against the oracle on the gathered points with the gathered pair-vector targets, scattered
    into zeros: within 64 2^-53 S with every pair evaluated in the same orientation (gathered_oracle's docstring).  Gathered
    in batch order — the other orientation for about half the pairs — the figure is printed: up to 78 x 2^-53 S (D = 7, `init`, quotient:
    grad_x), the oracle's own rounding."""
    worst = 0.0
    for c in C.all_cases():
        want = C.oracle(c)
        _close(C.case_id(c), C.gathered_oracle(c), want[:3], want.S)
        if C.n_pairs(c):
            plain = C.gathered_oracle(c, ascending=False)
            worst = max(worst, max(float((g - w).abs().max()) / want.S[name] for name, g, w in zip(C.NAMES, plain, want[:3])))
        outside = torch.ones(C.N_TOTAL, dtype=torch.bool)
        outside[C.batch_idx(c.bs)] = False
        assert not bool(outside.any()) or float(want.grad_x[outside].abs().max()) == 0.0
    print(f'gathered in batch order: within {worst / U64:.1f} x 2^-53 S')
    assert worst <= 1024 * U64     # (a node's gradient sums up to 256 pair terms, each a few ulp apart between the orientations)


def test_shards_add_up():
    for D in C.SHARD_DIMS:
        for loss in C.LOSSES:
            whole = C.oracle(C.Case('mid', D, C.BS, loss, None))
            parts = [C.oracle(C.Case('mid', D, C.BS, loss, rows)) for rows in C.COVER]
            total = [sum(p[k] for p in parts) for k in range(3)]
            _close(f'shards D={D} {loss}', total, whole[:3], whole.S)
            assert abs(sum(p.S['grad_scale'] for p in parts) - whole.S['grad_scale']) <= 64 * U64 * whole.S['grad_scale']
            for rows in C.SHARDS:
                if not C.n_pairs(C.Case('mid', D, C.BS, loss, rows)):
                    empty = C.oracle(C.Case('mid', D, C.BS, loss, rows))
                    assert all(float(t.abs().max()) == 0.0 for t in empty[:3]) and not any(empty.S.values())


def test_teeth():
    """a transposed read of the target matrix, and ONE wrong target, move what the GPU tests compare by far more than they allow"""
    cases = _with_pairs(C.all_cases())
    assert len(cases) == 124      # 136 less the two ranges without a pair, (129, 130) and (5, 5), of the six shard sweeps
    t_min, p_min = (np.inf, ''), (np.inf, '')
    for c in cases:
        S = C.oracle(c).S['grad_x']
        t, p = C.transpose_effect(c) / S, C.one_pair_effect(c) / S
        assert t >= C.TRANSPOSE_MIN, (C.case_id(c), t)
        assert p >= C.ONE_PAIR_MIN, (C.case_id(c), p)
        t_min, p_min = min(t_min, (t, C.case_id(c))), min(p_min, (p, C.case_id(c)))
    print(f'teeth over {len(cases)} cases: transposing dense moves grad_x by >= {t_min[0]:.3e} S ({t_min[1]}), '
          f'one pair by >= {p_min[0]:.3e} S ({p_min[1]})')


def test_one_pair_effect_is_the_literal_one():
    """one_pair_effect evaluates the single pair's term under both targets; the whole objective with that one target replaced
    moves by the same amount"""
    for c in (C.Case('init', 2, C.BS, 'stress', None), C.Case('wide', 9, C.BS, 'quotient', None), C.Case('mid', 6, 257, 'quotient', None),
              C.Case('mid', 3, 2, 'stress', None), C.Case('mid', 4, C.BS, 'quotient', (43, 86)), C.Case('mid', 4, C.BS, 'stress', (128, 129))):
        i, j = C.median_pair(c)
        assert i != j and {i, j} <= set(C.batch_idx(c.bs).tolist())
        a, b = C.one_pair_effect(c), C.one_pair_effect_literal(c)
        assert abs(a - b) <= 1e-9 * a and a > 0, (C.case_id(c), a, b)
