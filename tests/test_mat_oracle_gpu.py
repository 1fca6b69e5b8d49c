"""Every (NP, P) x {fp32, fp64} instantiation of the Grassmann / Stiefel kernels (csrc/mat_common.hpp, mat.hip, mat_step.hip,
grass_loss.hip) against the fp64 port of the reference on the CPU (oracle/ref_port.py), under the ABSOLUTE tolerance rule of
tests/mat_cases.py — built from the reference alone (its conditioning under one fp32 rounding of the inputs and its own fp32
arithmetic), never from another GPU route.  Every comparison prints `err / bound`; -rA shows the ratios (profiles/mat_oracle.md)."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grass_cases as gc  # noqa: E402
import mat_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

DNAMES = ['f32', 'f64']
KINDS = ['grassmann', 'stiefel']
ORTHONORMAL = ('exp', 'retr', 'retr_qr', 'projx')
WAVE_UNIFORM_LOOP = ('retr', 'exp', 'log')   # maps with a Jacobi sweep loop


def _sid(s):
    return f'{s[0]}x{s[1]}'


def _manifold(kind, N, p, retr='svd'):
    import graphembed.manifolds as M
    return (M.Grassmann if kind == 'grassmann' else M.Stiefel)(N, p, retr=retr)


def _finish(failures):
    assert not failures, '\n'.join(failures)


# ---- per-point maps ------------------------------------------------------------------------------------------------------------
def _map_args(op, x, u, y, t, a):
    return {'proju': (x, u), 'egrad2rgrad': (x, u), 'transp': (y, u), 'retr': (x, t), 'retr_qr': (x, t), 'projx': (a, None),
            'exp': (x, t), 'log': (x, y)}[op]


def _map_code(op):
    from graphembed import _backend as B
    return {'proju': B.MAT_PROJU, 'egrad2rgrad': B.MAT_PROJU, 'transp': B.MAT_PROJU, 'retr': B.MAT_RETR_SVD, 'retr_qr': B.MAT_RETR_QR,
            'projx': B.MAT_PROJX, 'exp': B.MAT_EXP, 'log': B.MAT_LOG}[op]


def _map_call(man, kind, op, x, u, y, t, a):
    """through the classes, as a caller would"""
    if op == 'transp':
        return man.transp(x, y, u)
    if op == 'projx':
        return man.projx(a) if kind == 'grassmann' else man._orthonormalize(a)
    first, second = _map_args(op, x, u, y, t, a)
    return {'proju': man.proju, 'egrad2rgrad': man.egrad2rgrad, 'retr': man.retr_svd_, 'retr_qr': man.retr_qr_,
            'exp': getattr(man, 'exp', None), 'log': getattr(man, 'log', None)}[op](first, second)


def _orthonormality(q):
    p = q.shape[-1]
    eye = torch.eye(p, dtype=q.dtype, device=q.device)
    return float((q.transpose(-2, -1) @ q - eye).abs().max())


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', mc.SHAPES, ids=_sid)
def test_maps_vs_fp64_oracle(shape, kind, dname):
    from graphembed import _backend as B
    N, p = shape
    dt = mc.DT[dname]
    man = _manifold(kind, N, p)
    kind_code = B.GRASSMANN if kind == 'grassmann' else B.STIEFEL
    failures = []
    with torch.no_grad():
        for regime in mc.regimes(N, p):
            want = mc.map_quantities(kind, regime, N, p)
            inp = [v.to(dt).cuda() for v in mc.map_inputs(kind, regime, N, p)]
            for op in mc.ops_of(kind, N, p):
                tag = f'{kind} {N}x{p} {regime}'
                full = _map_call(man, kind, op, *inp)
                assert full.shape == (mc.CNT, N, p)
                mc.check(tag, op, full, want[op], dname, failures)
                # A lane's result depends on its point only — bit for bit where the map has no data-dependent loop.  The Jacobi
                # sweeps of retr (polar), exp and log run while ANY lane of the wavefront is unconverged (smallmat.hpp): a converged
                # lane then rotates on by ~eps angles, so a point's result depends on its 63 wave-mates.  There the rows of
                # wavefronts that hold the same points in both launches are bitwise equal, and the others stay within the
                # rounding floor of the rule (16 2^-24 S, 64 2^-53 S).
                floor = (16 * mc.U32 if dname == 'f32' else 64 * mc.U64) * want[op].scale
                raw = torch.full((67, N, p), float('nan'), dtype=dt, device='cuda')   # one raw call, guard rows behind the output
                first, second = _map_args(op, *[v[:65].contiguous() for v in inp])
                B.lib().call('mm_mat_map', B.dtype_code(first), kind_code, _map_code(op), B.ptr(first), B.ptr(second), 65, N, p,
                             B.ptr(raw), B.stream_of(first))
                if not bool(torch.isnan(raw[65:]).all()):
                    failures.append(f'{tag} {op} {dname}: raw call at cnt = 65 wrote its guard rows')
                runs = [(f'cnt = {cnt}', cnt, _map_call(man, kind, op, *[v[:cnt] for v in inp])) for cnt in mc.PREFIXES]
                for label, cnt, part in runs + [('raw cnt = 65', 65, raw[:65])]:
                    same = cnt if op not in WAVE_UNIFORM_LOOP else cnt // 64 * 64
                    if not torch.equal(part[:same], full[:same]):
                        failures.append(f'{tag} {op} {dname}: {label}: rows [0, {same}) differ from those of cnt = {mc.CNT}')
                    dev = float((part[same:] - full[same:cnt]).abs().max()) if same < cnt else 0.0
                    if not dev <= floor:
                        failures.append(f'{tag} {op} {dname}: {label}: rows [{same}, {cnt}) are {dev:.3e} from those of cnt = {mc.CNT} '
                                        f'(floor {floor:.3e})')
                if op in ORTHONORMAL:
                    q = full
                    if op == 'exp':   # exp keeps what it is given: a point and a tangent exact in the dtype under test
                        xe = gc.frames(regime, mc.CNT, N, p)
                        xe = xe.to(dt).double() if dname == 'f32' else xe
                        te = mc.ref.make(kind, N, p).proju(xe, mc.vectors('ambient', mc.CNT, N, p).double())
                        q = man.exp(xe.to(dt).cuda(), te.to(dt).cuda())
                    dev, lim = _orthonormality(q), 16 * mc.eps_of(dt) * p
                    print(f'{tag} {op} {dname}: max|Q^T Q - I| {dev:.3e} / {lim:.3e}')
                    if not dev <= lim:
                        failures.append(f'{tag} {op} {dname}: max|Q^T Q - I| {dev:.3e} > {lim:.3e}')
    _finish(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.PIVOT_SHAPES, ids=_sid)
def test_log_with_zero_leading_pivot_vs_fp64_oracle(shape, dname):
    """(y^T x)[0][0] = 0 exactly: the p x p inverse inside log has to swap rows in its first elimination step"""
    N, p = shape
    dt = mc.DT[dname]
    x, y = (v.to(dt).cuda() for v in mc.pivot_inputs(N, p))
    assert not (y.transpose(1, 2) @ x)[:, 0, 0].any()
    failures = []
    with torch.no_grad():
        mc.check(f'grassmann {N}x{p} zero leading pivot', 'log_pivot', _manifold('grassmann', N, p).log(x, y), mc.pivot_quantities(N, p)['log'],
                 dname, failures)
    _finish(failures)


# ---- element-wise dist ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.SHAPES, ids=_sid)
def test_dist_vs_fp64_oracle(shape, dname):
    from graphembed import _backend as B
    N, p = shape
    dt = mc.DT[dname]
    man = _manifold('grassmann', N, p)
    g = mc.upstream(mc.CNT).to(dt).cuda()
    failures = []
    for regime in mc.regimes(N, p):
        x = mc.points(regime, mc.CNT, N, p).to(dt).cuda()
        y = torch.roll(x, 1, 0).contiguous()
        for squared in (True, False):
            names = mc.dist_compared(regime, N, p, squared)
            if not names:
                continue
            want = mc.dist_quantities(regime, N, p, squared)
            tag = f'dist {N}x{p} {regime} {"d2" if squared else "d"}'
            # forward only (no gradient buffers), then the gradient alone (no output buffer): the two launches of autograd
            xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
            d = man.dist(xr, yr, squared=squared)
            got = {'val': d.detach()}
            if 'grad_x' in names:
                got['grad_x'], got['grad_y'] = torch.autograd.grad((d * g).sum(), [xr, yr])
            for name in names:
                mc.check(tag, f'dist_{"d2" if squared else "d"}_{name}@autograd', got[name], want[name], dname, failures)
            # forward and gradient in one launch
            if 'grad_x' in names:
                out = torch.full((mc.CNT + 2, ), float('nan'), dtype=dt, device='cuda')
                gx, gy = (torch.full((mc.CNT + 2, N, p), float('nan'), dtype=dt, device='cuda') for _ in range(2))
                B.lib().call('mm_grass_dist', B.dtype_code(x), B.ptr(x), B.ptr(y), B.ptr(g), mc.CNT, N, p, int(squared), B.ptr(out),
                             B.ptr(gx), B.ptr(gy), B.stream_of(x))
                for name, t in (('val', out), ('grad_x', gx), ('grad_y', gy)):
                    if name in names:
                        mc.check(tag, f'dist_{"d2" if squared else "d"}_{name}@fused', t[:mc.CNT], want[name], dname, failures)
                    if not bool(torch.isnan(t[mc.CNT:]).all()):
                        failures.append(f'{tag} {name} {dname}: guard rows written')
    _finish(failures)


# ---- pdist -----------------------------------------------------------------------------------------------------------------------
def _pdist(man, x, squared, rows=None, g=None):
    """(pair vector, gradient of sum_k g_k d_k) through Grassmann.pdist and autograd"""
    xr = x.clone().requires_grad_(True)
    d = man.pdist(xr, squared=squared, rows=rows)
    if g is None:
        g = mc.upstream(d.numel()).to(x.dtype).cuda()
    gr, = torch.autograd.grad((d * g).sum(), xr)
    return d.detach(), gr


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.SHAPES, ids=_sid)
def test_pdist_vs_fp64_oracle(shape, dname):
    N, p = shape
    dt = mc.DT[dname]
    man = _manifold('grassmann', N, p)
    failures = []
    for regime in mc.regimes(N, p):
        for n in mc.PDIST_N:
            x = mc.points(regime, n, N, p).to(dt).cuda()
            for squared in (True, False):
                names = mc.pdist_compared(regime, n, N, p, squared)
                finite_only = N == p and not squared and dname == 'f64'   # 0/0 in the reference; the kernels' limit is finite
                if not names and not finite_only:
                    continue
                want = mc.pdist_quantities(regime, n, N, p, squared)
                d, gr = _pdist(man, x, squared)
                what = f'pdist_{"d2" if squared else "d"}'
                for name, got in (('val', d), ('grad', gr)):
                    if name in names:
                        mc.check(f'pdist {N}x{p} {regime} n={n}', f'{what}_{name}', got, want[(None, name)], dname, failures)
                if finite_only:
                    assert bool(torch.isfinite(gr).all()), (regime, n)
    _finish(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.ROW_SHAPES, ids=_sid)
def test_pdist_row_ranges_vs_fp64_oracle(shape, dname):
    N, p = shape
    n, dt = 129, mc.DT[dname]
    man = _manifold('grassmann', N, p)
    ranges = mc.rows_of(n)
    failures = []
    for regime in mc.regimes(N, p):
        names = mc.pdist_compared(regime, n, N, p, True)
        want = mc.pdist_quantities(regime, n, N, p, True, ranges)
        x = mc.points(regime, n, N, p).to(dt).cuda()
        full = None
        for rows in ranges:
            d, gr = _pdist(man, x, True, rows)
            lo, hi = mc.pair_slice(n, rows)
            assert d.numel() == hi - lo
            if hi == lo:
                assert not gr.any(), rows
            if rows is None:
                full = d
            tag = f'pdist {N}x{p} {regime} n={n} rows={rows}'
            for name, got in (('val', d), ('grad', gr)):
                if name in names:
                    mc.check(tag, f'pdist_rows_{name}', got, want[(rows, name)], dname, failures)
        with torch.no_grad():
            cuts = (0, 1, n // 3, 2 * n // 3, n - 2, n - 1, n)
            parts = [man.pdist(x, squared=True, rows=(a, b)) for a, b in zip(cuts, cuts[1:])]
        assert torch.equal(torch.cat(parts), full), regime
    _finish(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.ROW_SHAPES, ids=_sid)
def test_pdist_second_column_block_vs_fp64_oracle(shape, dname):
    """n = 257: the forward kernel's second 128-column start block, row tiles of 16 / 32 with a one-row remainder"""
    N, p = shape
    n, dt = 257, mc.DT[dname]
    want = mc.pdist_quantities('uniform', n, N, p, True, (None, ), 2)
    d, gr = _pdist(_manifold('grassmann', N, p), mc.points('uniform', n, N, p).to(dt).cuda(), True)
    failures = []
    for name, got in (('val', d), ('grad', gr)):
        if name in mc.pdist_compared('uniform', n, N, p, True):
            mc.check(f'pdist {N}x{p} uniform n={n}', f'pdist_d2_{name}', got, want[(None, name)], dname, failures)
    _finish(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.COINCIDENT, ids=_sid)
def test_pdist_coincident_points_vs_fp64_oracle(shape, dname):
    """point 7 := point 3: sigma = 1 for that pair.  The oracle's clamp at 1 - 1e-16 keeps its gradient finite in fp64 (-2 per
    principal direction); the kernels use that limit."""
    N, p = shape
    n, dt = 65, mc.DT[dname]
    want = mc.pdist_quantities('spread', n, N, p, True, (None, ), mc.DRAWS, True)
    x = mc.points('spread', n, N, p, True).to(dt).cuda()
    assert torch.equal(x[7], x[3])
    d, gr = _pdist(_manifold('grassmann', N, p), x, True)
    assert bool(torch.isfinite(gr).all())
    failures = []
    for name, got in (('val', d), ('grad', gr)):
        mc.check(f'pdist {N}x{p} spread n={n} coincident', f'pdist_coincident_{name}', got, want[(None, name)], dname, failures)
    _finish(failures)


# ---- the fused routes, absolutely --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('shape', mc.FUSED, ids=_sid)
def test_fused_objective_vs_fp64_oracle_absolute(shape, dname):
    N, p = shape
    n, dt = 65, mc.DT[dname]
    fn, kw = gc.objective('stress')
    failures = []
    for regime in mc.regimes(N, p):
        names = mc.loss_compared(regime, N, p)
        want = mc.loss_quantities(regime, n, N, p)
        emb = gc.embedding(n, N, p, dt, mc.points(regime, n, N, p).double())
        target = gc.targets(n).to(dt).cuda()
        with gc.CallSpy() as spy:
            loss = emb.fused_objective(fn, target, None, **kw)
        assert loss is not None and spy.calls.count('mm_grass_pdist_loss') == 1, spy.calls
        gx, gs = torch.autograd.grad(loss, [emb.xs[0], emb.scales[0]])
        for name, got in (('loss', loss.reshape(1)), ('grad_x', gx), ('grad_scale', gs.reshape(1))):
            if name in names:
                mc.check(f'objective {N}x{p} {regime} n={n}', f'loss_{name}', got, want[name], dname, failures)
    _finish(failures)


@pytest.mark.parametrize('dname', DNAMES)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', mc.FUSED, ids=_sid)
def test_rsgd_step_vs_fp64_oracle_absolute(shape, kind, dname):
    N, p = shape
    cnt, dt = 65, mc.DT[dname]
    x, g = mc.points('uniform', cnt, N, p).to(dt).cuda(), mc.egrad(cnt, N, p).to(dt).cuda()
    clip = mc.step_clip(kind, cnt, N, p)
    assert math.isfinite(clip) and clip > 0
    failures = []
    for retr, exact in mc.STEP_VARIANTS[kind]:
        want = mc.step_quantities(kind, retr, exact, cnt, N, p)
        with gc.CallSpy() as spy:
            new = _manifold(kind, N, p, retr).rsgd_step(x, g, lr=mc.LR, max_grad_norm=clip, exact=exact)
        assert spy.calls == ['mm_mat_rsgd_step'], spy.calls
        mc.check(f'rsgd {kind} {N}x{p} cnt={cnt}', f'step_{"exp" if exact else retr}', new, want['x_new'], dname, failures)
    _finish(failures)
