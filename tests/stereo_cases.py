"""Cases, deterministic inputs and a LONG-DOUBLE numpy oracle of the kappa-stereographic manifold (graphembed.manifolds.Stereographic,
csrc/stereo.hip).  Host code only; it shares no line with the kernels: distances come from the closed form
  D = 1 - 2 c p + c^2 a b,  t = q / D,  d = 2 / sqrt|c| * artanh_c(sqrt|c| sqrt t)
with the inverse functions themselves (numpy's long-double arctanh / arctan, no series), gradients from the chain rule through
dd/dr = 2 / (1 - c r^2), and the maps from the reference's formulas (manifolds/impl/math.py) in long double.

The case list is a stated subset of {n} x {m} x {c_init} x {keep_sign_fixed} x {regime} x {rows}, not the cross product:
  nodes     n in N_SWEEP at m = 5, c_init = 0.01, free sign, `init`                      7
  dims      m in M_SWEEP at n = 64, c_init = 1.0, fixed sign, `spread`                   6
  curvature c_init in C_SWEEP x fixed in {F, T} x regime in {init, spread}, n = 65, m = 8  16
  edge      c_init in {0.01, 1.0} x fixed in {F, T}, n = 65, m = 5 (c > 0 only)           4
  rows      ROWS of (n = 129, m = 13, c_init = -1.0, free, spread) and of (n = 257, m = 16, c_init = 0.01, fixed, init)   12
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LD = np.longdouble
N_SWEEP = (2, 3, 63, 64, 65, 129, 257)
M_SWEEP = (1, 2, 5, 8, 13, 16)
C_SWEEP = (0.01, -0.01, 1.0, -1.0)
C_MIN = 0.001
MIN_NORM = 1e-15
EPS = 1e-8
BALL_EPS = {'f32': 4e-3, 'f64': 1e-5}
FLOOR32 = 16 * 2.0**-24      # the fp32 rule never asks for less than this of the scale
TOL64 = 1e-11                # <= 257 fp64 accumulations x conditioning <= 1 / (1 - 0.49), two digits of margin


def _rows(n):
    """the full range, [0, 1), the middle third, the last row that has a pair, the last row (no pair: an empty pair vector and zero
    gradients), an empty range"""
    return (None, (0, 1), (n // 3, 2 * n // 3), (n - 2, n - 1), (n - 1, n), (5, 5))


def _build():
    cases = [(n, 5, 0.01, False, 'init', None) for n in N_SWEEP]
    cases += [(64, m, 1.0, True, 'spread', None) for m in M_SWEEP]
    cases += [(65, 8, c, fixed, regime, None) for c in C_SWEEP for fixed in (False, True) for regime in ('init', 'spread')]
    cases += [(65, 5, c, fixed, 'edge', None) for c in (0.01, 1.0) for fixed in (False, True)]
    cases += [(129, 13, -1.0, False, 'spread', r) for r in _rows(129)]
    cases += [(257, 16, 0.01, True, 'init', r) for r in _rows(257)]
    return cases


CASES = _build()


def case_id(case):
    n, m, c, fixed, regime, rows = case
    return f'n{n}-m{m}-c{c:g}-{"fix" if fixed else "free"}-{regime}' + ('' if rows is None else f'-r{rows[0]}_{rows[1]}')


def base_of(case):
    """the case without its row range: inputs and recorded pair vectors belong to it"""
    return case[:5] + (None, )


def rows_of(case):
    return (0, case[0]) if case[5] is None else case[5]


# ---- curvature -------------------------------------------------------------------------------------------------------------
def mode_of(c_init, fixed):
    """MM_STEREO_C_FREE / _POSITIVE / _NEGATIVE"""
    return 0 if not fixed else 1 if c_init > 0 else 2


def get_c(c_raw, mode, c_min=C_MIN):
    """(c, dc/dc_raw) of universal.py:27-31 in long double; softplus with torch's threshold of 20"""
    r = LD(c_raw)
    if mode == 0:
        return r + np.sign(r) * LD(c_min), LD(1)
    s = LD(1 if mode == 1 else -1)
    if r > 20:
        return s * (LD(c_min) + r), s
    e = np.exp(r)
    return s * (LD(c_min) + np.log1p(e)), s * e / (1 + e)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """x [n, m] as float32 (both precisions see the same numbers), c_raw as float32"""
    n, m, c_init, fixed, regime, _ = base_of(case)
    seed = 1000 * n + 10 * m + int(fixed) + (3 if c_init < 0 else 0) + {'init': 0, 'spread': 100000, 'edge': 200000}[regime] \
        + (7 if abs(c_init) == 1.0 else 0)
    rng = np.random.RandomState(seed)
    c_raw = np.float32(c_init)
    c = float(get_c(c_raw, mode_of(c_init, fixed))[0])
    if regime == 'init':
        x = rng.uniform(-1e-2, 1e-2, size=(n, m))
    else:
        x = rng.uniform(-0.5, 0.5, size=(n, m))
        x *= 0.699 / (np.sqrt(abs(c)) * np.sqrt((x * x).sum(-1)).max())   # sqrt|c| max|x| <= 0.7 after rounding
        if regime == 'edge':   # a third of the points outside the ball: projx has to act on them
            assert c > 0
            out = np.arange(n) % 3 == 1
            x[out] *= (1.2 / np.sqrt(c)) / np.sqrt((x[out] ** 2).sum(-1, keepdims=True))
    return x.astype(np.float32), c_raw


def upstream(npairs):
    """fixed pattern with both signs"""
    k = np.arange(npairs)
    return (((k * 7) % 11 - 5) / 5.0 + 0.1).astype(np.float32)


def tangent(case, salt=1):
    n, m = case[0], case[1]
    rng = np.random.RandomState(77 + 13 * n + m + salt)
    return rng.uniform(-1, 1, size=(n, m)).astype(np.float32)


def pair_slice(n, rows):
    off = lambda r: r * (2 * n - r - 1) // 2
    return off(rows[0]), off(rows[1])


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def _artan_c(z, c):
    return np.arctanh(z) if c > 0 else np.arctan(z)


def _tan_c(z, c):
    return np.tanh(np.clip(z, -15, 15)) if c > 0 else np.tan(z)


def pdist(x, c_raw, mode, squared, c_min=C_MIN):
    """pair vector (row-major upper triangle), long double, clamped at EPS like universal.py:83"""
    return _pairs(x, c_raw, mode, squared, c_min)[0]


def _pairs(x, c_raw, mode, squared, c_min=C_MIN):
    x = np.asarray(x, dtype=LD)
    n = x.shape[0]
    c, dc = get_c(c_raw, mode, c_min)
    i, j = np.triu_indices(n, 1)
    xi, xj = x[i], x[j]
    a, b, p = (xi * xi).sum(-1), (xj * xj).sum(-1), (xi * xj).sum(-1)
    q = ((xi - xj) ** 2).sum(-1)
    D = np.maximum(1 - 2 * c * p + c * c * a * b, LD(MIN_NORM))
    t = q / D
    r = np.sqrt(t)
    s = np.sqrt(abs(c))
    d = 2 * r if c == 0 else 2 / s * _artan_c(s * r, c)
    val = d * d if squared else d
    return np.maximum(val, LD(EPS)), dict(c=c, dc=dc, i=i, j=j, xi=xi, xj=xj, a=a, b=b, p=p, q=q, D=D, t=t, r=r, d=d)


def pdist_grads(x, c_raw, mode, squared, g, rows=None, c_min=C_MIN):
    """(grad_x [n, m], grad_c_raw, sum |g dF/dc_raw|) of sum_k g_k F_k over the pairs of `rows`; g covers that slice only"""
    x = np.asarray(x, dtype=LD)
    n = x.shape[0]
    _, P = _pairs(x, c_raw, mode, squared, c_min)
    lo, hi = pair_slice(n, rows or (0, n))
    gf = np.zeros(len(P['i']), dtype=LD)
    gf[lo:hi] = np.asarray(g, dtype=LD)
    c, t, r, d, D = P['c'], P['t'], P['r'], P['d'], P['D']
    with np.errstate(divide='ignore', invalid='ignore'):
        dd_dt = 1 / (r * (1 - c * t))                                      # dd/dr = 2 / (1 - c r^2), dr/dt = 1 / (2 r)
        dd_dc = np.zeros_like(d) if c == 0 else -d / (2 * c) + r / (c * (1 - c * t))
    dt_dc = 2 * t * (P['p'] - c * P['a'] * P['b']) / D
    out = 2 * d if squared else LD(1)
    G = gf * out * dd_dt
    G = np.where(gf == 0, LD(0), G)
    ci = (2 * (1 - c * c * P['b'] * t) / D)[:, None] * P['xi'] - (2 * (1 - c * t) / D)[:, None] * P['xj']
    cj = (2 * (1 - c * c * P['a'] * t) / D)[:, None] * P['xj'] - (2 * (1 - c * t) / D)[:, None] * P['xi']
    grad = np.zeros_like(x)
    np.add.at(grad, P['i'], G[:, None] * ci)
    np.add.at(grad, P['j'], G[:, None] * cj)
    per_pair = np.where(gf == 0, LD(0), gf * out * (dd_dt * dt_dc + dd_dc)) * P['dc']
    return grad, per_pair.sum(), np.abs(per_pair).sum()


def mobius_add(x, y, c):
    x2, y2, xy = (x * x).sum(-1, keepdims=True), (y * y).sum(-1, keepdims=True), (x * y).sum(-1, keepdims=True)
    num = (1 + 2 * c * xy + c * y2) * x + (1 - c * x2) * y
    return num / np.maximum(1 + 2 * c * xy + c * c * x2 * y2, LD(MIN_NORM))


def project(x, c, dname):
    if not c > 0:
        return x
    nrm = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), LD(MIN_NORM))
    maxnorm = (1 - LD(BALL_EPS[dname])) / np.sqrt(c)
    return np.where(nrm > maxnorm, x / nrm * maxnorm, x)


def _den(x, c):
    return np.maximum(1 - c * (x * x).sum(-1, keepdims=True), LD(MIN_NORM))


def expmap(x, u, c):
    un = np.maximum(np.sqrt((u * u).sum(-1, keepdims=True)), LD(MIN_NORM))
    s = np.sqrt(abs(c))
    second = _tan_c(s / 2 * (2 / _den(x, c)) * un, c) * u / (s * un)
    return mobius_add(x, second, c)


def maps(x, u, y, c_raw, mode, dname, c_min=C_MIN):
    """every per-point map of the class, long double, keyed by the method's name"""
    x, u, y = (np.asarray(t, dtype=LD) for t in (x, u, y))
    c = get_c(c_raw, mode, c_min)[0]
    s = np.sqrt(abs(c))
    lam = 2 / _den(x, c)
    sub = mobius_add(-x, y, c)
    sn = np.maximum(np.sqrt((sub * sub).sum(-1, keepdims=True)), LD(MIN_NORM))
    out = {'egrad2rgrad': u / lam ** 2, 'proju': u, 'projx': project(x, c, dname), 'exp_noproject': expmap(x, u, c),
           'retr': project(x + u, c, dname), 'log': 2 / s / lam * _artan_c(s * sn, c) * sub / sn}
    out['exp'] = project(out['exp_noproject'], c, dname)
    # transp(x, y, u) = gyr[y, -x] u lambda_x / lambda_y (impl/math.py:1282-1298, 1359-1362)
    gu, gv, w = y, -x, u
    u2, v2 = (gu * gu).sum(-1, keepdims=True), (gv * gv).sum(-1, keepdims=True)
    uv, uw, vw = (gu * gv).sum(-1, keepdims=True), (gu * w).sum(-1, keepdims=True), (gv * w).sum(-1, keepdims=True)
    A = -c * c * uw * v2 + c * vw + 2 * c * c * uv * vw
    Bq = -c * c * vw * u2 - c * uw
    gyr = w + 2 * (A * gu + Bq * gv) / np.maximum(1 + 2 * c * uv + c * c * u2 * v2, LD(MIN_NORM))
    out['transp'] = gyr * lam / (2 / _den(y, c))
    # Universal.norm: the conformal factor at c = 1 (universal.py:48-52)
    out['norm'] = (2 / _den(x, LD(1)) * np.sqrt((u * u).sum(-1, keepdims=True)))[:, 0]
    return out


def rsgd_step(x, egrad, c_raw, mode, dname, lr, max_grad_norm, exact, c_min=C_MIN):
    x, egrad = np.asarray(x, dtype=LD), np.asarray(egrad, dtype=LD)
    c = get_c(c_raw, mode, c_min)[0]
    r = egrad / (2 / _den(x, c)) ** 2
    if max_grad_norm is not None:
        nrm = 2 / _den(x, LD(1)) * np.sqrt((r * r).sum(-1, keepdims=True))
        with np.errstate(divide='ignore'):
            r = r * np.minimum(LD(max_grad_norm) / nrm, LD(1))
    step = -LD(lr) * r
    return project(expmap(x, step, c) if exact else x + step, c, dname)


def stabilize(x, c_raw, mode, dname, r_max, c_min=C_MIN):
    x = np.asarray(x, dtype=LD)
    c = get_c(c_raw, mode, c_min)[0]
    nrm = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)) / LD(r_max), LD(1))
    return project(x / nrm, c, dname)


def train_trace(xs, c_raws, modes, target, dname, epochs, lr=0.01, clr=0.001, clip=20, r_max=5.0):
    """(loss per epoch, c_raw per epoch) of the product training loop in long double: stress loss on the sum of the factors'
    squared distances, one exact RSGD step per factor, one SGD step per curvature, stabilize - the loop of the recorded
    `train40` trace (gen_golden_stereo.py)"""
    xs = [np.asarray(x, dtype=LD) for x in xs]
    cs = [LD(c) for c in c_raws]
    tg = np.asarray(target, dtype=LD)
    losses, curv = [], []
    for _ in range(epochs):
        d2 = sum(pdist(x, c, md, True) for x, c, md in zip(xs, cs, modes))
        losses.append(((d2 - tg) ** 2).sum())
        g = 2 * (d2 - tg)
        grads = [pdist_grads(x, c, md, True, g) for x, c, md in zip(xs, cs, modes)]
        xs = [rsgd_step(x, gr[0], c, md, dname, lr, clip, True) for x, gr, c, md in zip(xs, grads, cs, modes)]
        cs = [c - LD(clr) * gr[1] for c, gr in zip(cs, grads)]
        xs = [stabilize(x, c, md, dname, r_max) for x, c, md in zip(xs, cs, modes)]
        curv.append(list(cs))
    return np.array(losses, dtype=LD), np.array(curv, dtype=LD)


# ---- recorded reference ------------------------------------------------------------------------------------------------------
_files = {}


def recorded():
    """every array of tests/golden/stereo*.npz in one dict (keys: '<case id>/<quantity>')"""
    if not _files:
        for name in sorted(os.listdir(GOLDEN)):
            if name.startswith('stereo') and name.endswith('.npz'):
                with np.load(os.path.join(GOLDEN, name)) as z:
                    _files.update({k: z[k] for k in z.files})
    return _files


def deviation(got, want):
    return float(np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).max()) if np.size(want) else 0.0


def bound(dname, ref32_dev, scale):
    """the tolerance rule: fp64 1e-11 of the scale; fp32 twice the recorded reference-fp32's own deviation from the oracle on the
    same case and quantity, never below 16 * 2^-24 of the scale"""
    if dname == 'f64':
        return TOL64 * scale
    return max(2 * ref32_dev, FLOOR32 * scale)
