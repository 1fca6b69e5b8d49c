"""The case table and the tolerance rule of tests/spd_point_cases.py, checked on the CPU before any kernel is involved: the table
names every (kernel, D, dtype) instantiation once per regime; for every quantity tests/test_spd_point_oracle_gpu.py compares the
oracle and its conditioning are finite and the rule is not vacuous (bound_f32 <= 1e-3 S — a condition on the case list, not a
measurement of any kernel); what falls over the cap is exactly the documented list; the oracle itself is pinned to 40-digit
arithmetic within a quarter of bound_f64; the reference's float32 arithmetic passes its own bound; the windows bind."""
import collections
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import spd_point_cases as pc  # noqa: E402

MP_ROWS = (0, 1, 2, 64, 129)


def test_table_names_every_instantiation_once_per_regime():
    assert pc.DIMS == (2, 3, 4, 5, 6, 7, 8, 9) and pc.DNAMES == ('f32', 'f64') and len(pc.KERNELS) == 9
    rows = list(pc.table())
    assert len(rows) == len(set(rows)) == 144 * len(pc.ALL_REGIMES)
    per_regime = collections.Counter(r[0] for r in rows)
    assert set(per_regime) == set(pc.ALL_REGIMES) and set(per_regime.values()) == {144}
    assert len(set(pc.KERNELS.values())) == 9      # one entry point of the C ABI each
    # the optimizer cases the issue lists
    kinds = collections.Counter(c[0] for c in pc.STEP_CASES)
    assert kinds == {'rsgd': 4, 'momentum': 2, 'radam': 8} and len(set(pc.STEP_CASES)) == 14
    assert {(c[3], c[4], c[1]) for c in pc.STEP_CASES if c[0] == 'radam'} == {(t, nc, e) for t in (1, 11) for nc in (0, 1) for e in (0, 1)}
    assert {(c[1], c[2]) for c in pc.STEP_CASES if c[0] == 'rsgd'} == {(e, c) for e in (0, 1) for c in (0, 1)}
    try:
        from graphembed import _backend as B
        lib = B.lib()
    except Exception:   # noqa: BLE001  (no library in this tree: the range is the hard-coded one)
        return
    assert lib.raw('mm_spd_max_dim')() == pc.DIMS[-1]


def test_inputs_are_float32_symmetric_and_structured():
    import torch
    for D in pc.DIMS:
        for regime in pc.ALL_REGIMES:
            inp = pc.inputs(regime, D)
            assert all(v.dtype == torch.float32 and v.shape[0] == pc.CNT for v in inp.values())
            for k in ('x', 'y', 'ts', 'buf'):
                assert torch.equal(inp[k], inp[k].transpose(-1, -2)), (regime, D, k)
            for k in ('un', 'eg', 'a'):
                assert not torch.equal(inp[k], inp[k].transpose(-1, -2)), (regime, D, k)
            assert float(torch.linalg.eigvalsh(inp['x'].double()).min()) > 0
            if regime != 'wide':      # partly indefinite (x >= I of `wide` outweighs 3 u at the small D)
                assert float(torch.linalg.eigvalsh(0.5 * (inp['a'] + inp['a'].transpose(-1, -2)).double()).min()) < 0
            assert float(inp['v2'].min()) > 0 and torch.equal(inp['v2'], inp['v2'][:, :1, :1].expand_as(inp['v2']))
        e, m = pc.inputs('edge', D), pc.inputs('mid', D)
        x = e['x']
        assert torch.equal(x[pc.ROW_I], torch.eye(D))
        d = x[pc.ROW_DESC].diagonal()
        assert torch.equal(x[pc.ROW_DESC], torch.diag(d)) and bool((d[1:] < d[:-1]).all())
        d = x[pc.ROW_EQ].diagonal()
        assert torch.equal(x[pc.ROW_EQ], torch.diag(d)) and float(d[-1]) == float(d[-2])
        w = torch.linalg.eigvalsh(x[pc.ROW_ULP].double())
        assert 0 < float(w[1] - w[0]) < 4 * 2.0**-23 * float(w[0])      # (one ulp apart before the entries were rounded)
        assert torch.equal(e['y'][pc.ROW_COIN], x[pc.ROW_COIN]) and not torch.equal(m['y'][pc.ROW_COIN], m['x'][pc.ROW_COIN])
        assert not e['ts'][pc.ROW_ZERO].any() and not e['eg'][pc.ROW_ZERO].any()
        rest = [k for k in range(pc.CNT) if k not in pc.STRUCTURED]
        assert torch.equal(x[rest], m['x'][rest])      # the `mid` batch fixes the scales


@pytest.mark.parametrize('D', pc.DIMS)
def test_rule_is_finite_and_what_is_over_the_cap_is_the_documented_list(D):
    failures, over, windowed_total, count = [], {}, 0, 0
    for tag, name, q, regime, windowed in pc.candidates(D):
        count += 1
        windowed_total += windowed
        b32, b64 = q.bound('f32'), q.bound('f64')
        line = (f'{tag} {name}: cond {q.cond:.3e} port32 {q.port32} S {q.scale:.3e} bound_f32 {b32:.3e} ({b32 / q.scale:.2e} S) '
                f'bound_f64 {b64:.3e}')
        print(line)
        if not (math.isfinite(q.cond) and math.isfinite(q.scale) and q.scale > 0 and b64 <= b32):
            failures.append(line)
        # the reference's own float32 arithmetic passes its bound: the rule can be met
        if q.port32 is not None and not q.port32 <= b32:
            failures.append('float32 port over its own bound: ' + line)
        if not b32 <= pc.CAP * q.scale:
            over[(name, D, regime, windowed)] = b32 / q.scale
    assert count > 0 and windowed_total == 6 * len(pc.REGIMES)
    assert not failures, '\n'.join(failures)
    documented = {k + (False, ) for k in pc.DROPPED_DEFAULT if k[1] == D} | {k + (True, ) for k in pc.DROPPED_WINDOWED if k[1] == D}
    assert set(over) == documented, (over, documented)
    for key, ratio in over.items():      # the documented figure is the measured one (to its two digits)
        listed = (pc.DROPPED_WINDOWED if key[3] else pc.DROPPED_DEFAULT)[key[:3]]
        assert abs(ratio - listed) <= 0.05 * listed, (key, ratio, listed)


def test_dropped_lists():
    assert set(pc.DROPPED_DEFAULT) == {('stein_d_grad_x', 2, 'init'), ('stein_d_grad_y', 2, 'init')}
    assert len(pc.DROPPED_WINDOWED) <= 0.10 * 6 * len(pc.DIMS) * len(pc.REGIMES)
    assert all(k[0].startswith('wdist_') and k[1] in pc.DIMS and k[2] in pc.REGIMES for k in pc.DROPPED_WINDOWED)


@pytest.mark.parametrize('D', pc.DIMS)
def test_windows_bind(D):
    for regime in pc.REGIMES:
        wmin, wmax = pc.window(regime, D)
        eig_share, pair_share = pc.binding_shares(regime, D)
        print(f'spd({D}) {regime}: window [{wmin:.6g}, {wmax:.6g}] clamps {eig_share:.3f} of the eigenvalues, touches {pair_share:.3f} of the pairs')
        assert 1e-6 < wmin < 1 < wmax < 1e6      # narrower than the pair kernels' window: spd_clamps_wide is false
        assert 0.3 <= eig_share <= 0.7 and pair_share >= 0.3


def _mp_rows(D, regime):
    """{quantity: [row][...]} of exp, log, d^2, norm^2, Stein^2 on MP_ROWS in 40-digit arithmetic (Cholesky, eigsy, exp / log of
    the eigenvalues, det)"""
    from mpmath import mp
    inp = pc.inputs(regime, D)
    out = collections.defaultdict(list)
    floor = mp.mpf(10)**-8
    for k in MP_ROWS:
        X, Y, U = (mp.matrix(inp[n][k].double().tolist()) for n in ('x', 'y', 'ts'))
        L = mp.cholesky(X)
        Li = mp.inverse(L)

        def congr(M):
            A = Li * M * Li.T
            return (A + A.T) / 2

        def fun(A, f):
            E, Q = mp.eigsy(A)
            return L * (Q * mp.diag([f(e) for e in E]) * Q.T) * L.T, E
        A = congr(U)
        out['exp'].append(fun(A, mp.exp)[0].tolist())
        lg, E = fun(congr(Y), mp.log)
        out['log'].append(lg.tolist())
        out['d2'].append(max(sum(mp.log(e)**2 for e in E), floor))
        out['norm2'].append(sum(A[i, j]**2 for i in range(D) for j in range(D)))
        out['stein2'].append(max(mp.log(mp.det((X + Y) / 2)) - (mp.log(mp.det(X)) + mp.log(mp.det(Y))) / 2, floor))
    return out


@pytest.mark.parametrize('D', pc.DIMS)
def test_oracle_against_40_digits(D):
    """the fp64 oracle's own error on five rows per regime is at most a quarter of bound_f64"""
    mpmath = pytest.importorskip('mpmath')
    mp = mpmath.mp
    old, mp.dps = mp.dps, 40
    failures = []
    try:
        for regime in pc.REGIMES:
            want = _mp_rows(D, regime)
            maps = pc.map_quantities(regime, D)
            qs = {'exp': maps['exp'], 'log': maps['log'], 'norm2': maps['norm2'], 'd2': pc.dist_quantities(regime, D, True)['val'],
                  'stein2': pc.stein_quantities(regime, D, True)['val']}
            for name, q in qs.items():
                err = 0.0
                for r, k in enumerate(MP_ROWS):
                    w, got = want[name][r], q.want[k]
                    if name in ('exp', 'log'):
                        err = max(err, max(abs(float(w[i][j] - mp.mpf(float(got[i, j])))) for i in range(D) for j in range(D)))
                    else:
                        err = max(err, abs(float(w - mp.mpf(float(got)))))
                ratio = err / q.bound('f64')
                line = f'spd({D}) {regime} {name}: oracle {err:.3e} from 40 digits / bound_f64 {q.bound("f64"):.3e} = {ratio:.3f}'
                print(line)
                if not ratio <= 0.25:
                    failures.append(line)
    finally:
        mp.dps = old
    assert not failures, '\n'.join(failures)
