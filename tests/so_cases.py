"""Cases, inputs, a long-double oracle and the ABSOLUTE tolerance rule of tests/test_so_gpu.py (checked on the CPU by
tests/test_so_host.py): the SO(n) kernels of csrc/so.hip, n = 2 .. 4, fp32 and fp64.  Host code only; nothing here runs a kernel.

The oracle is written out in numpy.longdouble: a cyclic two-sided Jacobi on A = D^T D / 2 (D = y - x) gives (w_k, V), then
    d2 = sum_k psi(w_k),  psi(w) = 4 asin^2(sqrt(w / 2)) = theta_k^2,   psi' = 2 theta / sin theta (2 at w = 0),
    d d2 / dy = D V diag(psi') V^T = -d d2 / dx,
    log_x(y) = x skew(x^T D) V diag(psi' / 2) V^T,
    exp_x(u) = x (V cos(S) V^T + Om V (sin(S) / S) V^T),  Om = skew(x^T u), (S^2, V) = eig(Om^T Om),
and the fused stress / quotient objective on m = softplus(scale) d2 with its point and scale gradients summed per pair.
tests/test_so_host.py holds it to numpy.linalg.eigvals + arctan2 and scipy.linalg.logm.

Inputs are rounded to float32 first and widened afterwards (fp32 kernels, fp64 kernels and the oracle see the same numbers);
y = roll(x, 1) for the element-wise cases.  Regimes:
    init    x = polar(I + u), u skew with ||u||_F = 1e-2                 (the reference's initialisation: pair angles ~1e-2)
    spread  x = expm((G - G^T) / sqrt 2), G ~ 0.35 N(0, 1)               (rotation angles of the pairs reach 1.4 - 2.2)
    cut     pairs with one plane angle within 1e-3 of pi, and one pair with det(x^T y) = -1
Haar-uniform points are deliberately not a regime: their pairs reach theta ~ pi, where the gradient's cond exceeds S.

The rule is that of tests/mat_cases.py, verbatim (its `measure`, `Quantity` and `check` are used as they are):
    bound_f32 = max(32 cond, 2 port32) + 16 2^-24 S,     bound_f64 = 2^-29 max(64 cond, 4 port32) + 64 2^-53 S
    cond    the oracle's response to DRAWS = 8 draws of one fp32 rounding of the point / vector inputs
    port32  the same formulas in float32 torch ops on the CPU (torch.linalg.svd of D)
    S       maps max(1, max|W|); distances max|W|; pair-list gradients max_j sum_i |w_ij| |term_ij|
In `init` and `spread` everything is held to the rule — d2 and d values, the d2 gradient, log, exp, the objective; the
non-squared gradient in `spread` only (in `init` it is a unit vector field of points 1e-2 apart) — and tests/test_so_host.py
asserts bound_f32 <= 1e-3 S for every one of them.  In `cut` only finiteness, |d2 - oracle| under the rule and the
orthogonality of exp outputs are asserted.
"""
import functools
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grass_cases as gc  # noqa: E402
from grass_cases import _seed  # noqa: E402
from mat_cases import (CAP, CNT, DRAWS, PDIST_N, PREFIXES, RATIOS, U32, U64, Quantity, check, measure, pair_slice,  # noqa: E402,F401
                       upstream)

LD = np.longdouble
DT = gc.DT
DIMS = (2, 3, 4)
REGIMES = ('init', 'spread')
SCALE_RAW = gc.SCALE_RAW
QUOTIENT = gc.QUOTIENT
LOSSES = ('stress', 'quotient')
LR = 0.05
ROWS_129 = ((0, 1), (1, 43), (43, 86), (86, 129), (5, 5))   # four non-empty ranges that tile [0, 129) and an empty one


# ---- the long-double oracle ------------------------------------------------------------------------------------------------------
def _ld(t):
    return t.detach().cpu().numpy().astype(LD) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=LD)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _T(a):
    return np.swapaxes(a, -1, -2)


def jacobi_eigh(a, sweeps=30):
    """Cyclic Jacobi on a batch of symmetric matrices [m, N, N] in long double: (w [m, N], V [m, N, N]), a = V diag(w) V^T."""
    a = np.array(a, dtype=LD, copy=True)
    m, N = a.shape[0], a.shape[-1]
    v = np.broadcast_to(np.eye(N, dtype=LD), a.shape).copy()
    tiny = np.finfo(LD).tiny
    for _ in range(sweeps):
        off = sum(np.abs(a[:, p, q]).max(initial=LD(0)) for p in range(N) for q in range(p + 1, N))
        scale = np.abs(a).max(initial=LD(0))
        if off <= np.finfo(LD).eps * LD(1e-3) * scale:
            break
        for p in range(N - 1):
            for q in range(p + 1, N):
                apq, app, aqq = a[:, p, q], a[:, p, p], a[:, q, q]
                live = np.abs(apq) > tiny
                tau = np.where(live, (aqq - app) / np.where(live, 2 * apq, LD(1)), LD(0))
                with np.errstate(over='ignore'):   # (a[p][q] of 1e-4000: tau^2 = inf, t = 0)
                    t = np.where(live, np.where(tau >= 0, LD(1), LD(-1)) / (np.abs(tau) + np.sqrt(1 + tau * tau)), LD(0))
                c = (1 / np.sqrt(1 + t * t))[:, None]
                s = t[:, None] * c
                # a <- J^T a J, v <- v J with J[p][p] = J[q][q] = c, J[p][q] = s, J[q][p] = -s
                for m_ in (a, v):
                    cp, cq = m_[:, :, p].copy(), m_[:, :, q].copy()
                    m_[:, :, p], m_[:, :, q] = c * cp - s * cq, s * cp + c * cq
                rp, rq = a[:, p, :].copy(), a[:, q, :].copy()
                a[:, p, :], a[:, q, :] = c * rp - s * rq, s * rp + c * rq
                a[:, p, q] = a[:, q, p] = 0
    return np.stack([a[:, k, k] for k in range(N)], -1), v


def _psi(w):
    """(theta^2, psi') from the eigenvalues w of D^T D / 2 (s = sin(theta / 2) clamped to 1: the cut locus)"""
    s = np.minimum(np.sqrt(np.maximum(w, LD(0)) / 2), LD(1))
    half = np.arcsin(s)
    small = s < LD(1e-9)
    ratio = np.where(small, LD(1) + s * s / 6, half / np.where(small, LD(1), s))
    cos_half = np.sqrt(np.maximum(1 - s * s, LD(0)))
    dpsi = 2 * ratio / np.where(cos_half > 0, cos_half, LD(1))
    return 4 * half * half, np.where(cos_half > 0, dpsi, LD(0))


def _vfvt(v, f):
    return (v * f[:, None, :]) @ _T(v)


def pair_ld(x, y, grad=True):
    """d2 [m] and d d2 / dy [m, N, N] (= -d d2 / dx) of the pairs (x_k, y_k), long double arrays"""
    D = y - x
    w, v = jacobi_eigh(_T(D) @ D / 2)
    val, dpsi = _psi(w)
    return val.sum(-1), (D @ _vfvt(v, dpsi) if grad else None)


def log_ld(x, y):
    D = y - x
    w, v = jacobi_eigh(_T(D) @ D / 2)
    g = _T(x) @ D
    return x @ ((g - _T(g)) / 2) @ _vfvt(v, _psi(w)[1] / 2)


def exp_ld(x, u):
    g = _T(x) @ u
    om = (g - _T(g)) / 2
    w, v = jacobi_eigh(_T(om) @ om)
    sg = np.sqrt(np.maximum(w, LD(0)))
    small = sg < LD(1e-9)
    sinc = np.where(small, 1 - sg * sg / 6, np.sin(sg) / np.where(small, LD(1), sg))
    return x @ (_vfvt(v, np.cos(sg)) + om @ _vfvt(v, sinc))


def proju_ld(x, u):
    g = _T(x) @ u
    return u - x @ ((g + _T(g)) / 2)


def _softplus(s):
    return np.log1p(np.exp(LD(s)))


def loss_terms_ld(loss_name, m, tg):
    """per-pair (loss term, d term / d m) of objectives.py:16-45 (csrc/loss.hpp) in long double"""
    if loss_name == 'stress':
        r = m - tg
        return r * r, 2 * r
    ag, eps = tg * LD(QUOTIENT['alpha']), LD(1) / (QUOTIENT['epoch'] + 1)
    q1, q2 = m / ag - 1, ag / (m + eps) - 1
    return np.abs(q1) + np.abs(q2), np.sign(q1) / ag - np.sign(q2) * ag / (m + eps)**2


# ---- the same formulas in float32 / float64 torch ops (port32 of the rule; the benchmark's yardstick uses the same on the GPU) ----
def pair_torch(x, y):
    D = y - x
    U, S, Vh = torch.linalg.svd(D)
    s = (S / 2).clamp(max=1)
    half = torch.asin(s)
    ratio = torch.where(s > 1e-20, half / s.clamp_min(1e-20), torch.ones_like(s))
    dpsi = 2 * ratio / (1 - s * s).clamp_min(1e-12).sqrt()
    return (4 * half * half).sum(-1), (U * (S * dpsi).unsqueeze(-2)) @ Vh, (Vh, dpsi)


def log_torch(x, y):
    _, _, (Vh, dpsi) = pair_torch(x, y)
    g = x.transpose(-1, -2) @ (y - x)
    return x @ ((g - g.transpose(-1, -2)) / 2) @ (Vh.transpose(-1, -2) * (dpsi / 2).unsqueeze(-2)) @ Vh


def exp_torch(x, u):
    g = x.transpose(-1, -2) @ u
    om = (g - g.transpose(-1, -2)) / 2
    U, S, Vh = torch.linalg.svd(om)
    sinc = torch.where(S > 1e-6, torch.sin(S) / S.clamp_min(1e-6), 1 - S * S / 6)
    V = Vh.transpose(-1, -2)
    return x @ ((V * torch.cos(S).unsqueeze(-2)) @ Vh + (U * (S * sinc).unsqueeze(-2)) @ Vh)


def loss_terms_torch(loss_name, m, tg):
    if loss_name == 'stress':
        r = m - tg
        return r * r, 2 * r
    ag, eps = tg * QUOTIENT['alpha'], 1.0 / (QUOTIENT['epoch'] + 1)
    q1, q2 = m / ag - 1, ag / (m + eps) - 1
    return q1.abs() + q2.abs(), torch.sign(q1) / ag - torch.sign(q2) * ag / (m + eps)**2


def _is64(t):
    return t.dtype == torch.float64


# ---- inputs (all float32) ------------------------------------------------------------------------------------------------------
def _skew_gauss(rng, n, N):
    g = rng.standard_normal((n, N, N))
    return g - _T(g)


@functools.lru_cache(maxsize=None)
def points(regime, n, N, coincide=False):
    import scipy.linalg as sl
    rng = np.random.default_rng(_seed('so points', regime, n, N))
    a = _skew_gauss(rng, n, N)
    if regime == 'init':
        a = a / np.sqrt((a * a).sum((-2, -1), keepdims=True)) * 1e-2
        u, _, vh = np.linalg.svd(np.eye(N) + a)
        x = u @ vh
    else:
        x = np.stack([sl.expm(0.35 * k / np.sqrt(2.0)) for k in a])
    x = torch.from_numpy(x).float()
    if coincide:
        x[7] = x[3]
    return x


@functools.lru_cache(maxsize=None)
def tangents(regime, n, N):
    """u = x Omega, Omega skew with ||Omega||_F ~ 1e-2 (`init`) / uniform in [0.2, 2] (`spread`), float32"""
    rng = np.random.default_rng(_seed('so tangents', regime, n, N))
    a = _skew_gauss(rng, n, N)
    a = a / np.sqrt((a * a).sum((-2, -1), keepdims=True))
    a = a * (1e-2 if regime == 'init' else rng.uniform(0.2, 2.0, (n, 1, 1)))
    return (points(regime, n, N).double() @ torch.from_numpy(a)).float()


@functools.lru_cache(maxsize=None)
def cut_pairs(N, cnt=16):
    """(x, y, u) float32: y = x R with one plane angle pi - delta, delta log-uniform in [1e-6, 1e-3] (the other plane, N = 4, at an
    angle in [0.2, 1]), u = x log(R); the LAST pair has y = x times a reflection (det x^T y = -1) and u = 0."""
    import scipy.linalg as sl
    rng = np.random.default_rng(_seed('so cut', N, cnt))
    x = points('spread', cnt, N).double().numpy()
    q = np.linalg.qr(rng.standard_normal((cnt, N, N)))[0]
    om = np.zeros((cnt, N, N))
    delta = 10.0**rng.uniform(-6, -3, cnt)
    om[:, 0, 1], om[:, 1, 0] = -(np.pi - delta), np.pi - delta
    if N == 4:
        t = rng.uniform(0.2, 1.0, cnt)
        om[:, 2, 3], om[:, 3, 2] = -t, t
    om = q @ om @ _T(q)
    y = x @ np.stack([sl.expm(k) for k in om])
    u = x @ om
    refl = np.eye(N)
    refl[0, 0] = -1
    y[-1] = x[-1] @ (q[-1] @ refl @ q[-1].T)
    u[-1] = 0
    return torch.from_numpy(x).float(), torch.from_numpy(y).float(), torch.from_numpy(u).float()


def targets(n):
    return gc.targets(n)


# ---- quantities ------------------------------------------------------------------------------------------------------------------
def _w(d2, squared):
    """(value, d value / d d2) of the pair vector entry"""
    if squared:
        return d2, np.ones_like(d2) if isinstance(d2, np.ndarray) else torch.ones_like(d2)
    d = np.sqrt(d2) if isinstance(d2, np.ndarray) else d2.sqrt()
    safe = np.where(d > 0, d, 1) if isinstance(d2, np.ndarray) else torch.where(d > 0, d, torch.ones_like(d))
    return d, (d > 0) * 0.5 / safe


def _pair_any(x, y):
    """d2 and d d2 / dy by the oracle (float64 tensors in) or the float32 port (float32 tensors in); numpy long double / torch out"""
    if not _is64(x):
        v, g, _ = pair_torch(x, y)
        return v, g
    if x.shape[0] < 1000:
        return pair_ld(_ld(x), _ld(y))
    # (the pair lists of one point set serve several quantity sets — d2 and d, both objectives — whose perturbation draws share a
    # key: the long-double Jacobi of 8 000 pairs runs once per draw)
    key = hashlib.sha1(x.numpy().tobytes() + y.numpy().tobytes()).digest()
    if key not in _PAIR_MEMO:
        if len(_PAIR_MEMO) >= 20:
            _PAIR_MEMO.pop(next(iter(_PAIR_MEMO)))
        _PAIR_MEMO[key] = pair_ld(_ld(x), _ld(y))
    return _PAIR_MEMO[key]


_PAIR_MEMO = {}


def _out(a):
    return _t(a) if isinstance(a, np.ndarray) else a


@functools.lru_cache(maxsize=None)
def dist_quantities(regime, N, squared):
    """element-wise dist of CNT pairs (x, roll x): value, grad_x, grad_y of sum_k g_k d_k (each pair is one term: S = max|W|)"""
    x = points(regime, CNT, N)

    def fn(x, y):
        d2, dy = _pair_any(x, y)
        val, dv = _w(d2, squared)
        g = _ld(upstream(CNT)) if _is64(x) else upstream(CNT).float()
        gy = (g * dv)[:, None, None] * dy
        return ({'val': _out(val), 'grad_x': _out(-gy), 'grad_y': _out(gy)}, {'val': 'dist', 'grad_x': 'dist', 'grad_y': 'dist'})
    return measure(fn, (x, torch.roll(x, 1, 0)), ('so dist', regime, N, squared))


@functools.lru_cache(maxsize=None)
def map_quantities(regime, N):
    """log_x(roll x), exp_x(u) and the property proju(y, d d2 / dy) + 2 log_y(x) (= 0: its Quantity carries the gradient's cond)"""
    x, u = points(regime, CNT, N), tangents(regime, CNT, N)

    def fn(x, y, u):
        if _is64(x):
            xl, yl, ul = _ld(x), _ld(y), _ld(u)
            return ({'log': _t(log_ld(xl, yl)), 'exp': _t(exp_ld(xl, ul))}, {'log': 'map', 'exp': 'map'})
        return {'log': log_torch(x, y), 'exp': exp_torch(x, u)}, {'log': 'map', 'exp': 'map'}
    return measure(fn, (x, torch.roll(x, 1, 0), u), ('so maps', regime, N))


@functools.lru_cache(maxsize=None)
def identity_residual(regime, N):
    """proju(y, d (sum_k g_k d2_k) / dy) + 2 g log_y(x) of the CNT pairs (x, roll x) by the oracle, float64.  It vanishes on SO(n);
    the float32-rounded inputs are orthogonal to ~1e-7 only, and the ambient definition leaves a residual of that order."""
    x = _ld(points(regime, CNT, N).double())
    y = np.roll(x, 1, 0)
    g = _ld(upstream(CNT))[:, None, None]
    return _t(proju_ld(y, g * pair_ld(x, y)[1]) + 2 * g * log_ld(y, x))


@functools.lru_cache(maxsize=None)
def cut_quantities(N):
    x, y, _ = cut_pairs(N)

    def fn(x, y):
        d2 = pair_ld(_ld(x), _ld(y), grad=False)[0] if _is64(x) else pair_torch(x, y)[0]
        return {'val': _out(d2)}, {'val': 'dist'}
    return measure(fn, (x, y), ('so cut', N))


def _pairs_of(n):
    i, j = torch.triu_indices(n, n, 1)
    return i, j


def _scatter(n, i, j, ti, tj):
    return torch.zeros(n, *ti.shape[1:], dtype=ti.dtype).index_add_(0, i, ti).index_add_(0, j, tj)


@functools.lru_cache(maxsize=None)
def pdist_quantities(regime, n, N, squared, ranges=(None, ), coincide=False):
    """{(rows, 'val' | 'grad'): Quantity} of SpecialOrthogonal.pdist(x, squared, rows) with the upstream pattern on the slice; the
    per-pair derivatives are formed once per evaluation of the oracle and shared by every row range."""
    i, j = _pairs_of(n)

    def fn(x):
        d2, dy = _pair_any(x[i], x[j])
        val, dv = _w(d2, squared)
        val, dy = _out(val), _out(dv[:, None, None] * dy)
        vals, kinds = {}, {}
        for r in ranges:
            lo, hi = pair_slice(n, r)
            g = torch.zeros(val.numel(), dtype=val.dtype)
            g[lo:hi] = upstream(hi - lo).to(val.dtype)
            gj = g.reshape(-1, 1, 1) * dy
            vals[(r, 'val')], kinds[(r, 'val')] = val[lo:hi], 'dist'
            vals[(r, 'grad')] = _scatter(n, i, j, -gj, gj)
            kinds[(r, 'grad')] = float(_scatter(n, i, j, gj.abs(), gj.abs()).max())
        return vals, kinds
    return measure(fn, (points(regime, n, N, coincide), ), ('so pairs', regime, n, N, coincide))


def _objective(x, loss_name, n):
    """(loss [1], grad_x [n, N, N], grad_scale [1], S of grad_x, S of grad_scale) by the oracle / the float32 port"""
    i, j = _pairs_of(n)
    d2, dy = _pair_any(x[i], x[j])
    if _is64(x):
        sp, sig = _softplus(SCALE_RAW), 1 / (1 + np.exp(-LD(SCALE_RAW)))
        l, dldm = loss_terms_ld(loss_name, sp * d2, _ld(targets(n)))
        per_s = dldm * d2 * sig
        loss, gs, gj = _t(l.sum()), _t(per_s.sum()), _t((dldm * sp)[:, None, None] * dy)
        s_scale = float(np.abs(per_s).sum())
    else:
        sr = torch.tensor(SCALE_RAW, dtype=x.dtype)
        sp, sig = torch.nn.functional.softplus(sr), torch.sigmoid(sr)
        l, dldm = loss_terms_torch(loss_name, sp * d2, targets(n).to(x.dtype))
        per_s = dldm * d2 * sig
        loss, gs, gj = l.sum(), per_s.sum(), (dldm * sp).reshape(-1, 1, 1) * dy
        s_scale = float(per_s.abs().sum())
    return loss.reshape(1), _scatter(n, i, j, -gj, gj), gs.reshape(1), float(_scatter(n, i, j, gj.abs(), gj.abs()).max()), s_scale


@functools.lru_cache(maxsize=None)
def loss_quantities(regime, n, N, loss_name):
    def fn(x):
        loss, gx, gs, s_x, s_s = _objective(x, loss_name, n)
        return {'loss': loss, 'grad_x': gx, 'grad_scale': gs}, {'loss': 'dist', 'grad_x': s_x, 'grad_scale': s_s}
    return measure(fn, (points(regime, n, N), ), ('so pairs', regime, n, N, False))


def oracle_step(x, n, optimizer, exact=False):
    """(loss, grad_x, x_new) of one optimizer step on the stress objective from the points x (float64: the oracle; float32: the
    port): the objective's gradient, then oracle/ref_port.py's rsgd_step / radam_step (rsgd.py:40-82, radam.py:43-98; first
    step, no clip) on St(N, N) with the polar retraction (stiefel.py:66-69) or, `exact`, the exp above"""
    from oracle import ref_port as ref
    loss, gx = _objective(x, 'stress', n)[:2]
    man = ref.Stiefel(x.shape[-1], x.shape[-1])
    man.exp = lambda p, u: _t(exp_ld(_ld(p), _ld(u))) if _is64(p) else exp_torch(p, u)
    if optimizer == 'rsgd':
        return loss, gx, ref.rsgd_step(man, x, gx, lr=LR, exact=exact)[0]
    return loss, gx, ref.radam_step(man, x, gx, {}, lr=LR, exact=exact)


@functools.lru_cache(maxsize=None)
def step_quantities(regime, n, N, optimizer, exact=False):
    def fn(x):
        return {'x_new': oracle_step(x, n, optimizer, exact)[2]}, {'x_new': 'map'}
    return measure(fn, (points(regime, n, N), ), ('so step', regime, n, N, optimizer, exact))


def orth_defect(x):
    x = x.detach().double().cpu()
    return float((x.transpose(-1, -2) @ x - torch.eye(x.shape[-1], dtype=torch.float64)).abs().max())


def orth_bound(x_in, dname):
    """exp_x(u) = x E with E orthogonal up to the rounding of ~8 N multiply-adds per entry: |o^T o - I| <= N |x^T x - I| + 64 N u"""
    N = x_in.shape[-1]
    return N * orth_defect(x_in) + 64 * N * (U32 if dname == 'f32' else U64)


# ---- the list of compared quantities (walked by tests/test_so_host.py; tests/test_so_gpu.py makes the same calls) ----------------
def compared(N):
    """(tag, name, Quantity) of everything the GPU tests hold to the rule at this size in `init` and `spread`"""
    for regime in REGIMES:
        for squared in (True, False):
            q = dist_quantities(regime, N, squared)
            names = ('val', 'grad_x', 'grad_y') if squared or regime == 'spread' else ('val', )
            for name in names:
                yield f'so dist {N} {regime}', f'so_dist_{"d2" if squared else "d"}_{name}', q[name]
        q = map_quantities(regime, N)
        for name in ('log', 'exp'):
            yield f'so map {N} {regime}', f'so_map_{name}', q[name]
        for n in PDIST_N:   # (everything of one point set together: its quantity sets share the oracle's pair lists)
            for squared in (True, False):
                q = pdist_quantities(regime, n, N, squared)
                for name in ('val', 'grad') if squared or regime == 'spread' else ('val', ):
                    yield f'so pdist {N} {regime} n={n}', f'so_pdist_{"d2" if squared else "d"}_{name}', q[(None, name)]
            if n == 129:
                q = pdist_quantities(regime, 129, N, True, ROWS_129)
                for rows in ROWS_129:
                    if pair_slice(129, rows)[0] < pair_slice(129, rows)[1]:
                        for name in ('val', 'grad'):
                            yield f'so pdist {N} {regime} n=129 rows={rows}', f'so_pdist_rows_{name}', q[(rows, name)]
            if n in (65, 130):
                for loss_name in LOSSES:
                    q = loss_quantities(regime, n, N, loss_name)
                    for name in ('loss', 'grad_x', 'grad_scale'):
                        yield f'so objective {N} {regime} {loss_name} n={n}', f'so_loss_{name}', q[name]
    q = pdist_quantities('spread', 65, N, True, (None, ), True)
    for name in ('val', 'grad'):
        yield f'so pdist {N} spread n=65 coincident', f'so_pdist_coincident_{name}', q[(None, name)]
