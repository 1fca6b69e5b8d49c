"""The case list and the tolerance rule of tests/mat_cases.py, checked on the CPU before any kernel is involved: for every case
and quantity that tests/test_mat_oracle_gpu.py compares, the oracle and its conditioning are finite, the rule is not vacuous
(bound_f32 <= 1e-3 S — a condition on the case list, not a measurement of any kernel), and the perturbation is not degenerate
against the reference's own fp32 arithmetic."""
import collections
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mat_cases as mc  # noqa: E402


def test_shapes_cover_every_instantiation():
    pad = lambda N: 4 if N <= 4 else 6 if N <= 6 else 9   # noqa: E731  (pad_rows of csrc/mat_common.hpp)
    assert len(set(mc.SHAPES)) == len(mc.SHAPES) == 26
    by_inst = collections.defaultdict(list)
    for N, p in mc.SHAPES:
        assert 1 <= p <= min(N, 4) and N <= 9
        by_inst[(pad(N), p)].append(N)
    assert set(by_inst) == {(NP, P) for NP in (4, 6, 9) for P in (1, 2, 3, 4)}
    for (NP, P), Ns in by_inst.items():
        assert NP in Ns and (min(Ns) < NP or NP == P), (NP, P, Ns)   # N = NP and, where p allows one, a padded N < NP
    assert {(p, p) for p in (1, 2, 3, 4)} <= set(mc.SHAPES)       # every N = p
    assert set(mc.ROW_SHAPES) | set(mc.COINCIDENT) | set(mc.FUSED) <= set(mc.SHAPES)
    assert sorted(p for _, p in mc.COINCIDENT) == [1, 2, 3, 4]


@pytest.mark.parametrize('shape', mc.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_rule_is_finite_and_not_vacuous(shape):
    N, p = shape
    failures, count = [], 0
    for tag, name, q, lucky in mc.compared(N, p):
        count += 1
        b32, b64 = q.bound('f32'), q.bound('f64')
        line = f'{tag} {name}: cond {q.cond:.3e} port32 {q.port32} S {q.scale:.3e} bound_f32 {b32:.3e} ({b32 / q.scale:.2e} S) bound_f64 {b64:.3e}'
        print(line)
        ok = math.isfinite(q.cond) and math.isfinite(q.scale) and q.scale > 0 and b32 <= mc.CAP * q.scale and b64 <= b32
        # N = p = 1: Q of a 1 x 1 matrix is its sign and x = +-1 is exact in fp32 — the oracle is piecewise constant there
        # (cond = 0 for the retractions, port32 = 0 for the projections)
        # port32 >= cond / 4: the perturbation does not overstate what fp32 arithmetic does to this quantity.  Where the port's fp32
        # result is a matter of luck (mat_cases.compared) it was measured down to cond / 30; there the floor is cond / 64.
        if (N, p) != (1, 1):
            ok = ok and q.cond > 0 and (q.port32 is None or q.port32 >= q.cond / (64 if lucky else 4))
        if not ok:
            failures.append(line)
    assert count > 0
    assert not failures, '\n'.join(failures)


def test_bounds_follow_the_stated_formulas():
    q = mc.Quantity(None, 3.0e-7, 5.0e-6, 2.0)
    assert q.bound('f32') == max(32 * 3.0e-7, 2 * 5.0e-6) + 16 * 2.0**-24 * 2.0
    assert q.bound('f64') == 2.0**-29 * max(64 * 3.0e-7, 4 * 5.0e-6) + 64 * 2.0**-53 * 2.0
    q = mc.Quantity(None, 3.0e-7, None, 2.0)
    assert q.bound('f32') == 32 * 3.0e-7 + 16 * 2.0**-24 * 2.0


def test_oracle_dist_is_the_port_with_an_exact_acos_derivative():
    """OracleGrassmann.dist: the port's value bit for bit (p = 2: to the port's own cancellation); the port's gradient to its own rounding away from sigma = 1; and next
    to sigma = 1 the closed form -2 theta / sin(theta) * y of Gr(N,1) evaluated from the angle itself."""
    import torch
    for N, p in ((5, 2), (6, 3), (4, 1)):
        x = mc.points('uniform', 9, N, p).double()
        a, b = x.clone().requires_grad_(True), torch.roll(x, 1, 0).clone().requires_grad_(True)
        a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        d, d2 = mc.ref.Grassmann(N, p).dist(a, b, squared=True), mc.OracleGrassmann(N, p).dist(a2, b2, squared=True)
        dd, dd2 = d.detach(), d2.detach()
        assert torch.equal(dd, dd2) if p != 2 else float((dd - dd2).abs().max()) <= 1e-13 * float(dd.abs().max())
        g, g2 = torch.autograd.grad(d.sum(), a)[0], torch.autograd.grad(d2.sum(), a2)[0]
        assert float((g - g2).abs().max()) <= (1e-13 if p != 2 else 1e-10) * float(g.abs().max())
    # Gr(2,1), points at the angles t and t + h: d^2 = h^2, d(d^2)/dx = -2 h / sin(h) * y
    t, h = torch.tensor(0.3, dtype=torch.float64), torch.tensor(2.0**-13, dtype=torch.float64)
    x = torch.stack([torch.cos(t), torch.sin(t)]).reshape(1, 2, 1).requires_grad_(True)
    y = torch.stack([torch.cos(t + h), torch.sin(t + h)]).reshape(1, 2, 1)
    g, = torch.autograd.grad(mc.OracleGrassmann(2, 1).dist(x, y, squared=True).sum(), x)
    want = -2 * h / torch.sin(h) * y
    assert float((g - want).abs().max()) <= 1e-15 / float(h)   # (sigma itself carries 1e-16: 1e-16 / sin(h) of the angle)


def test_oracle_p2_values_against_40_digits():
    """The reference's closed form for p = 2 (linalg/fast.py:138-159 with its clamps, then acos^2) in 40-digit arithmetic on the
    130 pairs of Gr(9,2) `uniform`: the oracle's d^2 agrees to a few ulp; the port's own fp64 does not (1.4e-13)."""
    import torch
    from mpmath import acos, mp, mpf, sqrt
    N, p = 9, 2
    x = mc.points('uniform', mc.CNT, N, p).double()
    y = torch.roll(x, 1, 0)
    old_dps, mp.dps = mp.dps, 40
    try:
        want = []
        for k in range(mc.CNT):
            G = [[sum(mpf(float(x[k, r, i])) * mpf(float(y[k, r, j])) for r in range(N)) for j in range(2)] for i in range(2)]
            a, b, c, d = G[0][0], G[0][1], G[1][0], G[1][1]
            S1 = a * a + b * b + c * c + d * d
            S2 = sqrt(max((a * a + b * b - c * c - d * d)**2 + 4 * (a * c + b * d)**2, mpf(10)**-8))
            s1, s2 = sqrt(max((S1 + S2) / 2, mpf(10)**-8)), sqrt(max((S1 - S2) / 2, mpf(10)**-8))
            want.append(acos(min(s1, 1 - mpf(10)**-16))**2 + acos(min(s2, 1 - mpf(10)**-16))**2)
        dev = lambda got: max(abs(float(w - mpf(float(v)))) for w, v in zip(want, got))   # noqa: E731
        oracle, port = dev(mc.OracleGrassmann(N, p).dist(x, y, squared=True)), dev(mc.ref.Grassmann(N, p).dist(x, y, squared=True))
    finally:
        mp.dps = old_dps
    print(f'oracle {oracle:.3e} port {port:.3e}')
    assert oracle <= 16 * 2.0**-53 * 4.5 and port > 10 * oracle
