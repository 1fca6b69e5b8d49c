"""CPU-only checks of the SO(n) feature: the long-double oracle of tests/so_cases.py against independent libraries (numpy's
eigvals, scipy's logm) and its own central differences, the cap on the tolerance rule, and the new entry points — declared,
exported, sized, and refusing bad arguments before anything touches a GPU."""
import ctypes
import os
import re
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import ROOT

import so_cases as sc
from graphembed import _backend as B

NEW = ('mm_so_max_dim', 'mm_so_map', 'mm_so_dist', 'mm_so_pdist_ws_bytes', 'mm_so_pdist_fwd', 'mm_so_pdist_bwd',
       'mm_so_pdist_loss_ws_bytes', 'mm_so_pdist_loss')
LOSS_SLOTS = 256   # csrc/loss.hpp
LD = sc.LD
# sixteen times what the formulation measured against the independent libraries (1.7e-13 for d2, 6.4e-12 for log / the gradient)
TOL_D2, TOL_LOG = 2.7e-12, 1.0e-10
ANGLES = (1e-3, 1e-2, 0.1, 1.0, 2.0)
MEASURED = {}


def _fp64_pairs(N, t, cnt=24):
    """x, y = x expm(Om), Om skew with plane angles t and t / 2 — orthonormal to fp64 rounding; Om itself"""
    import scipy.linalg as sl
    rng = np.random.default_rng(sc._seed('so host', N, t))
    x = np.stack([sl.expm(a - a.T) for a in rng.standard_normal((cnt, N, N))])
    q = np.linalg.qr(rng.standard_normal((cnt, N, N)))[0]
    om = np.zeros((cnt, N, N))
    om[:, 0, 1], om[:, 1, 0] = -t, t
    if N >= 4:
        om[:, 2, 3], om[:, 3, 2] = -t / 2, t / 2
    om = q @ om @ np.swapaxes(q, -1, -2)
    # (expm of an fp64 skew matrix is orthogonal to ~1e-16; re-orthonormalise by the polar factor to be exact about it)
    u, _, vh = np.linalg.svd(x @ np.stack([sl.expm(k) for k in om]))
    ux, _, vhx = np.linalg.svd(x)
    return ux @ vhx, u @ vh


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _note(key, val):
    MEASURED[key] = max(MEASURED.get(key, 0.0), val)
    print(f'{key}: {val:.2e}')


@pytest.mark.parametrize('N', (2, 3, 4, 5))
def test_oracle_against_eigvals_and_logm(N):
    import scipy.linalg as sl
    for t in ANGLES:
        x, y = _fp64_pairs(N, t)
        xl, yl = x.astype(LD), y.astype(LD)
        d2, gy = sc.pair_ld(xl, yl)
        ev = np.linalg.eigvals(np.swapaxes(x, -1, -2) @ y)
        want = (np.arctan2(ev.imag, ev.real)**2).sum(-1)
        e = _rel(d2, want)
        _note(f'd2 vs eigvals N={N}', e)
        assert e <= TOL_D2, (N, t, e)
        logm = np.stack([a @ sl.logm(a.T @ b).real for a, b in zip(x, y)])      # orthogonal.py:26-28
        e = _rel(sc.log_ld(xl, yl), logm)
        _note(f'log vs logm N={N}', e)
        assert e <= TOL_LOG, (N, t, e)
        logyx = np.stack([b @ sl.logm(b.T @ a).real for a, b in zip(x, y)])
        e = _rel(sc.proju_ld(yl, gy), -2 * logyx)                               # proju(y, d d2 / dy) = -2 log_y(x)
        _note(f'proju(grad) vs -2 logm N={N}', e)
        assert e <= TOL_LOG, (N, t, e)
        u = sc.log_ld(xl, yl)
        e = _rel(sc.exp_ld(xl, u), y)                                           # exp(x, log(x, y)) = y
        _note(f'exp(log) N={N}', e)
        assert e <= TOL_LOG, (N, t, e)
        d2u = sc.pair_ld(xl, sc.exp_ld(xl, u), grad=False)[0]                   # dist(x, exp(x, u)) = ||u||_F
        e = _rel(np.sqrt(d2u), np.sqrt((u * u).sum((-2, -1))))
        _note(f'dist(exp) vs |u| N={N}', e)
        assert e <= TOL_LOG, (N, t, e)


@pytest.mark.parametrize('N', (2, 3, 4))
def test_oracle_gradient_against_its_central_differences(N):
    rng = np.random.default_rng(7)
    for regime in sc.REGIMES:
        x = sc._ld(sc.points(regime, 16, N).double())
        y = np.roll(x, 1, 0)
        _, gy = sc.pair_ld(x, y)
        h = LD(1e-6) if regime == 'spread' else LD(1e-7)
        for _ in range(3):
            e = rng.standard_normal(x.shape).astype(LD)
            fd_y = (sc.pair_ld(x, y + h * e, False)[0] - sc.pair_ld(x, y - h * e, False)[0]) / (2 * h)
            fd_x = (sc.pair_ld(x + h * e, y, False)[0] - sc.pair_ld(x - h * e, y, False)[0]) / (2 * h)
            an = (gy * e).sum((-2, -1))
            scale = float(np.abs(gy).max()) * N
            assert float(np.abs(fd_y - an).max()) <= 1e-7 * scale, (N, regime)
            assert float(np.abs(fd_x + an).max()) <= 1e-7 * scale, (N, regime)


def test_oracle_degenerate_pairs():
    for N in sc.DIMS:
        x = sc._ld(sc.points('spread', 4, N).double())
        d2, g = sc.pair_ld(x, x)
        assert float(np.abs(d2).max()) == 0 and float(np.abs(g).max()) == 0
        xc, yc, _ = sc.cut_pairs(N)
        d2 = sc.pair_ld(sc._ld(xc.double()), sc._ld(yc.double()), grad=False)[0]
        assert np.isfinite(d2.astype(np.float64)).all()
        assert float(d2[:-1].min()) > (np.pi - 2e-3)**2 and float(d2[-1]) >= (np.pi - 1e-2)**2   # (one plane near pi; the reflection)
        det = torch.linalg.det(xc.double().transpose(-1, -2) @ yc.double())
        assert float(det[-1]) < -0.99 and float(det[:-1].min()) > 0.99


@pytest.mark.parametrize('N', sc.DIMS)
def test_rule_is_capped_at_1e3_of_the_scale(N):
    """bound_f32 <= 1e-3 S for everything tests/test_so_gpu.py compares in `init` and `spread`: the rule is never vacuous"""
    worst = (0.0, '')
    count = zero_scale = 0
    for tag, name, q in sc.compared(N):
        count += 1
        if q.scale == 0:   # SO(2) `init` has two points only (u = +-1e-2 J / sqrt 2): at n = 2, 3 every pair may coincide
            assert N == 2 and ' init n=' in tag and float(q.want.abs().max()) == 0, (tag, name)
            zero_scale += 1
            continue
        r = q.bound('f32') / q.scale
        worst = max(worst, (r, f'{tag} {name}'))
        assert r <= sc.CAP, (tag, name, r, q.cond, q.port32, q.scale)
        assert q.bound('f64') <= q.bound('f32')
    print(f'N={N}: {count} quantities, worst bound_f32 / S = {worst[0]:.2e} ({worst[1]})')
    assert count >= 90 and zero_scale <= 4


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert B.lib().raw('mm_abi_version')() == 4
    assert B.lib().raw('mm_so_max_dim')() == 4
    assert (B.SO_LOG, B.SO_EXP) == (0, 1) and re.search(r'MM_SO_LOG = 0', src) and re.search(r'MM_SO_EXP = 1', src)


@pytest.mark.parametrize('dtype,size', [(B.MM_F32, 4), (B.MM_F64, 8)])
def test_workspaces_cover_accumulators_and_loss_slots(dtype, size):
    ws, wl = B.lib().raw('mm_so_pdist_ws_bytes'), B.lib().raw('mm_so_pdist_loss_ws_bytes')
    for N in sc.DIMS:
        last = 0
        for n in (1, 2, 63, 64, 65, 257, 2000, 1 << 20, 1 << 30):
            b, bl = ws(dtype, n, N), wl(dtype, n, N)
            assert b >= size * n * N * N and bl >= b + size * 2 * LOSS_SLOTS, (n, N, b, bl)   # acc [N*N][n] (+ 2 x 256 slots)
            assert b >= last and b % 256 == 0
            last = b
    assert ws(dtype, -1, 3) == 0 and wl(dtype, -1, 3) == 0


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    m, d, fwd, bwd, loss = (lib.raw(k) for k in ('mm_so_map', 'mm_so_dist', 'mm_so_pdist_fwd', 'mm_so_pdist_bwd', 'mm_so_pdist_loss'))

    for op in (B.SO_LOG, B.SO_EXP):
        assert m(B.MM_F32, op, None, q, 4, 3, q, None) == -1 and m(B.MM_F32, op, q, None, 4, 3, q, None) == -1
        assert m(B.MM_F32, op, q, q, 4, 3, None, None) == -1 and m(B.MM_F32, op, q, q, -1, 3, q, None) == -1
        assert m(5, op, q, q, 4, 3, q, None) == -1 and m(B.MM_F32, op, q, q, 4, 0, q, None) == -1
        assert m(B.MM_F32, op, q, q, 0, 3, q, None) == 0                       # nothing to do
        for N in (1, 5, 9):
            assert m(B.MM_F32, op, q, q, 4, N, q, None) == -2
    assert m(B.MM_F32, 2, q, q, 4, 3, q, None) == -1 and m(B.MM_F32, -1, q, q, 4, 3, q, None) == -1

    assert d(B.MM_F32, None, q, None, 4, 3, 1, q, None, None, None) == -1 and d(B.MM_F32, q, None, None, 4, 3, 1, q, None, None, None) == -1
    assert d(B.MM_F32, q, q, q, 4, 3, 1, q, q, None, None) == -1               # one gradient without the other
    assert d(B.MM_F32, q, q, None, 4, 3, 1, q, q, q, None) == -1               # gradients without the upstream
    assert d(B.MM_F32, q, q, None, -1, 3, 1, q, None, None, None) == -1 and d(7, q, q, None, 4, 3, 1, q, None, None, None) == -1
    assert d(B.MM_F32, q, q, None, 0, 3, 1, q, None, None, None) == 0
    for N in (1, 5):
        assert d(B.MM_F64, q, q, None, 4, N, 1, q, None, None, None) == -2

    def f(x=q, n=10, N=3, rb=0, re=10, out=q, dtype=B.MM_F32):
        return fwd(dtype, x, n, N, rb, re, 1, out, None)

    def b(x=q, g=q, n=10, N=3, rb=0, re=10, grad=q, ws=q, dtype=B.MM_F32):
        return bwd(dtype, x, g, n, N, rb, re, 1, grad, ws, None)

    def l(x=q, target=q, n=10, N=3, rb=0, re=10, out=q, grad=q, ws=q, kind=B.LOSS_STRESS, dtype=B.MM_F32):
        return loss(dtype, kind, x, target, q, n, N, rb, re, 1.0, 1.0, 3, None, out, grad, ws, None)

    assert f(x=None) == -1 and f(out=None) == -1 and f(rb=5, re=4) == -1 and f(re=11) == -1 and f(rb=-1) == -1 and f(dtype=3) == -1
    assert f(n=(1 << 30) + 1) == -1 and f(rb=4, re=4, out=None) == 0           # an empty range needs no output
    assert b(x=None) == -1 and b(g=None) == -1 and b(grad=None) == -1 and b(ws=None) == -1 and b(re=11) == -1 and b(dtype=3) == -1
    assert l(x=None) == -1 and l(grad=None) == -1 and l(ws=None) == -1 and l(out=None) == -1 and l(target=None) == -1
    assert l(rb=5, re=4) == -1 and l(re=11) == -1 and l(rb=-1) == -1 and l(n=(1 << 30) + 1) == -1
    assert l(kind=99) == -1 and l(kind=B.LOSS_NONE) == -1 and l(dtype=5) == -1
    for N in (1, 5, 9):
        assert f(N=N) == -2 and b(N=N) == -2 and l(N=N) == -2
    assert f(N=0) == -1 and b(N=0) == -1 and l(N=0) == -1
    with pytest.raises(B.BackendError):
        lib.call('mm_so_pdist_loss', B.MM_F32, B.LOSS_STRESS, None, q, q, 10, 3, 0, 10, 1.0, 1.0, 3, None, q, q, q, None)


def test_so_kernels_keep_everything_in_registers():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    if not (os.path.exists(os.path.join(kernel_meta.LLVM, 'llvm-objdump')) and os.path.exists(kernel_meta.LIB)):
        pytest.skip('needs the ROCm llvm tools and the built library')
    ks = {nm: k for nm, k in kernel_meta.kernels().items() if nm.startswith('so::')}
    # map, dist: 3 sizes x 2 dtypes each; pdist forward: x 2 (full batch, node minibatch); the pair kernel: x (3 loss kinds + the
    # non-squared backward) x 2; 2 finalize
    assert len(ks) == 2 * 6 + 2 * 6 + 2 * 4 * 6 + 2, sorted(ks)
    for nm, k in ks.items():
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)


def test_python_class_surface():
    import graphembed.manifolds as M
    assert 'SpecialOrthogonal' in M.__all__ and issubclass(M.SpecialOrthogonal, M.Stiefel)
    assert not hasattr(M, 'OrthogonalGroup') and not hasattr(M, 'SpecialOrthogonalGroup')
    man = M.SpecialOrthogonal(3)
    assert (man.n, man.p, man.dim, man.ndim) == (3, 3, 3, 2) and M.SpecialOrthogonal(4, retr='qr')._retr_op == B.MAT_RETR_QR
    assert M.SpecialOrthogonal(4).dim == 6 and M.SpecialOrthogonal(2).dim == 1
    x = torch.eye(3).repeat(5, 1, 1)
    for call in (lambda: man.dist(x, x), lambda: man.pdist(x), lambda: man.log(x, x), lambda: man.exp(x, x),
                 lambda: man.pdist_loss(x, torch.zeros(1), torch.zeros(10), ('stress', 1.0, 1.0, 3))):
        with pytest.raises(B.BackendError):
            call()
    assert man.rsgd_step(x, x, lr=0.1) is None                    # the fused steps decline CPU tensors
    assert not man._step_eligible(x, x, exact=True)               # `exact` goes the optimizers' generic route over exp

    class Ref:   # the shape of the checkout's SpecialOrthogonalGroup(n, retr='qr')
        n = p = 4

        def retr_qr(self, x, u):
            return x
        retr = retr_qr
    got = M.SpecialOrthogonal.from_reference(Ref())
    assert (got.n, got.p, got._retr_op) == (4, 4, B.MAT_RETR_QR)
    assert 'orthogonal group' in str(got).lower()


def test_overlay_keeps_orthogonal_group_with_the_checkout(tmp_path):
    """under the stand-in checkout of tests/test_overlay_reference.py, manifolds.OrthogonalGroup still comes from the checkout and
    SpecialOrthogonal from this package"""
    import test_overlay_reference as tor
    for rel, text in tor.CHECKOUT.items():
        path = tmp_path / 'graphembed' / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(textwrap.dedent(text).lstrip())
    tor.run('''
        from graphembed import manifolds
        assert origin(manifolds.OrthogonalGroup) == 'reference' and origin(manifolds.SpecialOrthogonalGroup) == 'reference'
        assert origin(manifolds.SpecialOrthogonal) == 'ours' and origin(manifolds.Stiefel) == 'ours'
        assert not issubclass(manifolds.SpecialOrthogonal, manifolds.OrthogonalGroup)
    ''', str(tmp_path))
