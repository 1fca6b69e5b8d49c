"""Cases, inputs, fp64 oracle and the ABSOLUTE tolerance rule of tests/test_spd_point_oracle_gpu.py (checked on the CPU by
tests/test_spd_point_cases_host.py): every (kernel, D, dtype) instantiation of the per-point SPD kernels — spd_dist_fwd_kernel,
spd_dist_bwd_kernel, spd_map_kernel, spd_norm_kernel, spd_eigvalsh_kernel (csrc/spd_pair.hpp), spd_stein_div_kernel
(csrc/spd_stein.hpp) and the optimizer kernels behind mm_spd_rsgd_step, mm_spd_rsgd_momentum_step, mm_spd_radam_step — for
D = 2 .. 9 in fp32 and fp64: 9 x 8 x 2 = 144.  Host code only; nothing here runs a kernel.

Inputs: CNT = 130 points, fixed seeds, rounded to float32 first and widened afterwards (fp32 kernels, fp64 kernels and the
oracle see the same numbers); y = roll(x, 1); the upstream g is stereo_cases.upstream.  Regimes of x:
    init   exp(S), S symmetric Gaussian with ||S||_F = 0.1          (the reference's initialisation)
    mid    exp(S), ||S||_F = 1.5
    wide   A A^T + I, A Gaussian
    edge   the `mid` batch with structured rows (the batch fixes S, no scale is zero):
             row 3  the identity                                   row 4  diag, descending entries (the eigvalsh sort)
             row 5  diag with two equal entries                    row 6  Q diag Q^T, two eigenvalues one fp32 ulp apart
             row 7  a coincident pair, y_7 = x_7                   row 9  a zero tangent and a zero egrad
           (rows 3 .. 6 are also what projx / eigvalsh get there, in place of x + 3 u)
Tangents / ambient gradients are uniform in +-0.3: symmetric for exp, retr and norm; NOT symmetric for proju, egrad2rgrad and
the optimizer steps' egrad (the reference applies sym).  projx and eigvalsh get the non-symmetric, partly indefinite x + 3 u;
log gets y.

Oracle: oracle.step.ExactSPD (LAPACK factorisations for every D, no eps-fudged closed forms) in fp64; the gradients of dist
and stein_div by autograd of the port (through sym(x), sym(y): the kernels return the symmetric gradient); eigvalsh is
numpy.linalg.eigvalsh(sym(x)); the optimizer kernels are one step of oracle.step.apply_rule.

The rule is that of tests/mat_cases.py, unchanged (its `measure`, `Quantity` and `check` are used as they are):
    bound_f32 = max(32 cond, 2 port32) + 16 2^-24 S,     bound_f64 = 2^-29 max(64 cond, 4 port32) + 64 2^-53 S
    cond    the oracle's largest response over DRAWS = 8 draws of one fp32 rounding (1 + delta, |delta| <= 2^-24) of every entry
            of the point and vector inputs (moment buffers included; symmetric inputs are re-symmetrised)
    port32  ExactSPD in float32 on the CPU, ignored where not finite
    S       maps, eigenvalues and optimizer outputs max(1, max|W|); distance, divergence, norm values and gradients max|W|
A quantity is held to the rule only where bound_f32 <= CAP S = 1e-3 S (tests/test_spd_point_cases_host.py asserts it for
everything held).  Under the default window [1e-8, 1e8] everything is held in init / mid / wide / edge except
    the x and y gradients of the NON-squared Stein divergence at D = 2, `init`:   bound_f32 = 2.7e-3 S, 2.4e-3 S
(DROPPED_DEFAULT; the divergences there are ~1e-3 and the reference's own float32 gradient of the
square root is off by 5e-4 there: 2 port32 alone is over the cap).

Binding windows.  Per (D, regime) of init / mid / wide, (wmin, wmax) are the 25 % and 75 % quantiles (rounded to float32) of
the oracle's eigenvalues of L_x^-1 Y L_x^-T over the batch: spd_dist_fwd_kernel then goes through pair_core instead of
pair_value and spd_dist_bwd_kernel through its rho factors; d^2, d and their gradients are compared for all eight D.  Half the
EIGENVALUES of the batch are clamped by construction; a PAIR is touched as soon as one of its D eigenvalues is, so the share of
bound pairs grows with D (0.8 at D = 2, 1.0 from D = 5 on: both figures are printed and held by the host test — the
eigenvalue share within [0.3, 0.7], the pair share >= 0.3).  Note the reference floors d^2 at wmin itself (spd.py:165-167), so
under such a window many d^2 equal wmin; the kernels do the same.  Windowed quantities over the cap: DROPPED_WINDOWED, each with
its bound_f32 / S (at most 10 % of the 6 x 8 x 3 = 144 may be there).

Edge rows are compared like any other row, with two documented exceptions: the NON-squared distance / divergence and their
gradients at the coincident pair (row 7) are only required to be finite — the reference divides by the square root of its own
floor there (1e-4), which turns one input rounding into 1e-3 of S —, so `edge` compares the non-squared quantities on the other
129 rows; and the oracle's own step is not finite at the zero egrad (row 9) under AdamNc at its first step: beta2 = 1 - 1/t = 0
makes exp_avg_sq = ||rgrad||^2 = 0 there and the direction exp_avg / (0 + eps) ~ 1e7, so the port's exp overflows (and its
retraction's 1e14 would be S for the whole batch): x_new of that row is left out of those four cases (exp_avg and exp_avg_sq of
the row are compared).  Under clipping the zero gradient is harmless: clamp(clip / 0, max = 1) = 1 in the port, min(clip / 0, 1)
= 1 in the kernels, and the row is compared like the rest.

Optimizer cases (one step, lr = 0.05; clip = the median of the oracle's Riemannian gradient norms, rounded to float32):
    rsgd      exact in {0, 1} x clip in {none, median}
    momentum  momentum 0.9, dampening 0.1, a non-zero symmetric buffer: (retr, clip), (exp, no clip)
    radam     non-zero symmetric exp_avg, positive exp_avg_sq, betas (0.9, 0.999), eps 1e-8; step counter 0 and 10 steps done
              (the kernel's `step` argument is state['step'] = 1 and 11), nc in {0, 1}, exact in {0, 1}; clip at 10 steps done
compared: x_new, the momentum buffer, exp_avg, exp_avg_sq.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from grass_cases import DT, _seed  # noqa: E402,F401
from mat_cases import CAP, CNT, DRAWS, RATIOS, U32, U64, Quantity, check, measure, upstream  # noqa: E402,F401
from oracle import ref_port as rp  # noqa: E402
from oracle.step import ExactSPD, apply_rule  # noqa: E402

DIMS = (2, 3, 4, 5, 6, 7, 8, 9)
DNAMES = ('f32', 'f64')
REGIMES = ('init', 'mid', 'wide')      # the regimes the windows are built for
ALL_REGIMES = REGIMES + ('edge', )
M_EDGES = (0, 1, 127, 128, 129, 130)   # launches of 128 threads: nothing, one lane, a block less one, a block, one / two lanes more
LR = 0.05
BETAS = (0.9, 0.999)
ADAM_EPS = rp.EPS
ROW_I, ROW_DESC, ROW_EQ, ROW_ULP, ROW_COIN, ROW_ZERO = 3, 4, 5, 6, 7, 9
STRUCTURED = (ROW_I, ROW_DESC, ROW_EQ, ROW_ULP)

# kernel -> its entry point of the C ABI; with DIMS x DNAMES: the 144 instantiations
KERNELS = {
    'spd_dist_fwd_kernel': 'mm_spd_dist_fwd', 'spd_dist_bwd_kernel': 'mm_spd_dist_bwd', 'spd_map_kernel': 'mm_spd_map',
    'spd_norm_kernel': 'mm_spd_norm', 'spd_eigvalsh_kernel': 'mm_spd_eigvalsh', 'spd_stein_div_kernel': 'mm_spd_stein_div',
    'spd_rsgd_step_kernel': 'mm_spd_rsgd_step', 'spd_rsgd_momentum_kernel': 'mm_spd_rsgd_momentum_step',
    'spd_radam_step_kernel': 'mm_spd_radam_step',
}
MAP_OPS = ('egrad2rgrad', 'exp', 'retr', 'log', 'projx', 'proju')      # in the order of MM_SPD_EGRAD2RGRAD .. MM_SPD_PROJU
MAP_NAMES = MAP_OPS + ('norm', 'norm2', 'eigvalsh')
PAIR_NAMES = ('val', 'grad_x', 'grad_y')

# (kind, exact, clip, state['step'] before the call, nc)
STEP_CASES = tuple([('rsgd', e, c, None, None) for e in (0, 1) for c in (0, 1)]
                   + [('momentum', 0, 1, None, None), ('momentum', 1, 0, None, None)]
                   + [('radam', e, int(t0 == 11), t0, nc) for t0 in (1, 11) for nc in (0, 1) for e in (0, 1)])
STEP_OUTPUTS = {'rsgd': ('x_new', ), 'momentum': ('x_new', 'momentum_buffer'), 'radam': ('x_new', 'exp_avg', 'exp_avg_sq')}

# (quantity, D, regime) -> bound_f32 / S, as tests/test_spd_point_cases_host.py measures it
DROPPED_DEFAULT = {('stein_d_grad_x', 2, 'init'): 2.68e-3, ('stein_d_grad_y', 2, 'init'): 2.37e-3}
DROPPED_WINDOWED = {}


def table():
    """(regime, kernel, D, dname): every instantiation once per regime"""
    for regime in ALL_REGIMES:
        for kernel in KERNELS:
            for D in DIMS:
                for dname in DNAMES:
                    yield regime, kernel, D, dname


def step_id(case):
    kind, exact, clip, t0, nc = case
    return f'{kind}{"_exp" if exact else "_retr"}{"_clip" if clip else ""}' + ('' if t0 is None else f'_t{t0}{"_nc" if nc else ""}')


# ---- inputs (all float32) ------------------------------------------------------------------------------------------------------
def _T(a):
    return np.swapaxes(a, -1, -2)


def _sym_f32(a):
    """float64 numpy [n, D, D] -> float32 tensor, symmetric bit for bit"""
    t = torch.from_numpy(np.ascontiguousarray(a)).float()
    return 0.5 * (t + t.transpose(-1, -2))


@functools.lru_cache(maxsize=None)
def points(regime, D):
    rng = np.random.default_rng(_seed('spd point', 'mid' if regime == 'edge' else regime, CNT, D))
    if regime == 'wide':
        a = rng.standard_normal((CNT, D, D))
        x = a @ _T(a) + np.eye(D)
    else:
        s = rng.standard_normal((CNT, D, D))
        s = 0.5 * (s + _T(s))
        s *= (0.1 if regime == 'init' else 1.5) / np.sqrt((s * s).sum((-2, -1), keepdims=True))
        w, v = np.linalg.eigh(s)
        x = (v * np.exp(w)[:, None, :]) @ _T(v)
    if regime == 'edge':
        x[ROW_I] = np.eye(D)
        x[ROW_DESC] = np.diag(np.linspace(2.0, 0.5, D))
        d = np.linspace(0.6, 1.5, D)
        d[-1] = d[-2]
        x[ROW_EQ] = np.diag(d)
        d = np.linspace(0.7, 1.9, D)
        d[1] = d[0] * (1 + 2.0**-23)
        q = np.linalg.qr(rng.standard_normal((D, D)))[0]
        x[ROW_ULP] = (q * d) @ q.T
    return _sym_f32(x)


@functools.lru_cache(maxsize=None)
def vectors(tag, D, symmetric):
    g = torch.Generator().manual_seed(_seed('spd point vectors', tag, CNT, D))
    u = (torch.rand(CNT, D, D, dtype=torch.float64, generator=g) * 2 - 1) * 0.3
    return (rp.sym(u) if symmetric else u).float()


@functools.lru_cache(maxsize=None)
def inputs(regime, D):
    """x, y, ts (symmetric tangent), un (non-symmetric ambient vector), a (x + 3 un), eg (non-symmetric egrad), buf (momentum
    buffer / exp_avg, symmetric), v2 (exp_avg_sq: one positive scalar per point, broadcast over it) — float32, CNT points"""
    x = points(regime, D)
    y = torch.roll(x, 1, 0).clone()
    ts, un, eg = vectors('tangent', D, True).clone(), vectors('ambient', D, False).clone(), vectors('egrad', D, False).clone()
    a = (x.double() + 3 * un.double()).float()
    if regime == 'edge':
        y[ROW_COIN] = x[ROW_COIN]
        ts[ROW_ZERO], un[ROW_ZERO], eg[ROW_ZERO] = 0, 0, 0
        for r in STRUCTURED:
            a[r] = x[r]
    g = torch.Generator().manual_seed(_seed('spd point moments', CNT, D))
    v2 = (0.05 + 0.5 * torch.rand(CNT, 1, 1, dtype=torch.float64, generator=g)).float().expand(CNT, D, D).contiguous()
    return dict(x=x, y=y, ts=ts, un=un, a=a, eg=eg, buf=vectors('buffer', D, True), v2=v2)


def _all_but(row):
    return torch.tensor([k for k in range(CNT) if k != row])


def keep_rows(regime, squared):
    """rows of the pair quantities that are compared (None: all) — see the module docstring on the coincident pair"""
    return _all_but(ROW_COIN) if regime == 'edge' and not squared else None


def step_keep_rows(regime, case, name):
    """rows of an optimizer output that are compared (None: all) — see the module docstring on the zero egrad under AdamNc"""
    kind, _, _, t0, nc = case
    return _all_but(ROW_ZERO) if regime == 'edge' and kind == 'radam' and nc and t0 == 1 and name == 'x_new' else None


# ---- windows -------------------------------------------------------------------------------------------------------------------
def _pair_eigenvalues(regime, D):
    inp = inputs(regime, D)
    x, y = inp['x'].double(), inp['y'].double()
    l_inv, _ = ExactSPD(D).invchol(x)
    return np.linalg.eigvalsh(rp.sym(rp.axat(l_inv, y)).numpy())


@functools.lru_cache(maxsize=None)
def window(regime, D, lo=0.25, hi=0.75):
    w = _pair_eigenvalues(regime, D)
    return float(np.float32(np.quantile(w, lo))), float(np.float32(np.quantile(w, hi)))


def binding_shares(regime, D):
    """(share of the batch's eigenvalues outside the window, share of the pairs with at least one outside)"""
    w = _pair_eigenvalues(regime, D)
    wmin, wmax = window(regime, D)
    out = (w < wmin) | (w > wmax)
    return float(out.mean()), float(out.any(-1).mean())


# ---- quantities ----------------------------------------------------------------------------------------------------------------
def _eigvalsh(a):
    return torch.from_numpy(np.linalg.eigvalsh(rp.sym(a).numpy()))


@functools.lru_cache(maxsize=None)
def map_quantities(regime, D):
    man = ExactSPD(D)

    def fn(x, y, ts, un, a):
        x, y, ts = rp.sym(x), rp.sym(y), rp.sym(ts)
        out = {'egrad2rgrad': man.egrad2rgrad(x, un), 'exp': man.exp(x, ts), 'retr': man.retr(x, ts), 'log': man.log(x, y),
               'projx': man.projx(a), 'proju': man.proju(x, un), 'norm': man.norm(x, ts), 'norm2': man.norm(x, ts, squared=True),
               'eigvalsh': _eigvalsh(a)}
        return out, {k: 'dist' if k in ('norm', 'norm2') else 'map' for k in out}
    inp = inputs(regime, D)
    return measure(fn, tuple(inp[k] for k in ('x', 'y', 'ts', 'un', 'a')), ('spd point maps', regime, D))


def _pair_fn(value, regime, squared):
    keep = keep_rows(regime, squared)

    def fn(x, y):
        xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        d = value(rp.sym(xl), rp.sym(yl))
        gx, gy = torch.autograd.grad((d * upstream(CNT).to(d.dtype)).sum(), [xl, yl])
        out = {'val': d.detach(), 'grad_x': gx, 'grad_y': gy}
        if keep is not None:
            out = {k: v[keep] for k, v in out.items()}
        return out, dict.fromkeys(out, 'dist')
    return fn


@functools.lru_cache(maxsize=None)
def dist_quantities(regime, D, squared, windowed=False):
    """element-wise dist of the CNT pairs (x, y): value, grad_x, grad_y of sum_k g_k d_k (each pair is one term: S = max|W|)"""
    man = ExactSPD(D, *window(regime, D)) if windowed else ExactSPD(D)
    inp = inputs(regime, D)
    return measure(_pair_fn(lambda x, y: man.dist(x, y, squared=squared), regime, squared), (inp['x'], inp['y']),
                   ('spd point dist', regime, D, squared, windowed))


@functools.lru_cache(maxsize=None)
def stein_quantities(regime, D, squared):
    man = ExactSPD(D)
    inp = inputs(regime, D)
    return measure(_pair_fn(lambda x, y: man.stein_div(x, y, squared=squared), regime, squared), (inp['x'], inp['y']),
                   ('spd point stein', regime, D, squared))


@functools.lru_cache(maxsize=None)
def step_clip(regime, D):
    """the median Riemannian gradient norm of the case (both branches of the clip in one launch), a float32 number"""
    man, inp = ExactSPD(D), inputs(regime, D)
    x = inp['x'].double()
    return float(np.float32(man.norm(x, man.egrad2rgrad(x, inp['eg'].double())).median()))


def step_rule(regime, D, case):
    kind, exact, clip, _, nc = case
    rule = {'lr': LR, 'exact': bool(exact), 'max_grad_norm': step_clip(regime, D) if clip else None}
    if kind == 'radam':
        rule.update(opt='radam', betas=BETAS, nc=bool(nc))
    else:
        rule.update(opt='rsgd', momentum=0.9 if kind == 'momentum' else 0.0, dampening=0.1 if kind == 'momentum' else 0.0)
    return rule


@functools.lru_cache(maxsize=None)
def step_quantities(regime, D, case):
    kind, _, _, t0, _ = case
    man, rule, inp = ExactSPD(D), step_rule(regime, D, case), inputs(regime, D)

    def fn(x, eg, buf, v2):
        x, buf = rp.sym(x), rp.sym(buf)
        state = {}
        if kind == 'momentum':
            state = {'momentum_buffer': buf}
        elif kind == 'radam':
            state = {'exp_avg': buf, 'exp_avg_sq': v2[:, :1, :1].expand_as(x), 'step': t0}
        new_x, new_state, _ = apply_rule(man, x, eg, rule, state)
        out = {'x_new': new_x}
        for k in STEP_OUTPUTS[kind][1:]:
            out[k] = new_state[k].expand_as(x).contiguous()
        keep = step_keep_rows(regime, case, 'x_new')
        if keep is not None:
            out['x_new'] = out['x_new'][keep]
        return out, dict.fromkeys(out, 'map')
    return measure(fn, tuple(inp[k] for k in ('x', 'eg', 'buf', 'v2')), ('spd point step', regime, D, case))


# ---- the list of compared quantities (walked by tests/test_spd_point_cases_host.py; the GPU tests make the same calls) --------------
def _d(squared):
    return 'd2' if squared else 'd'


def held(name, D, regime, windowed=False):
    return (name, D, regime) not in (DROPPED_WINDOWED if windowed else DROPPED_DEFAULT)


def candidates(D, regimes=ALL_REGIMES):
    """(tag, name, Quantity, regime, windowed) of everything the rule is evaluated for at this D, dropped quantities included"""
    for regime in regimes:
        q = map_quantities(regime, D)
        for name in MAP_NAMES:
            yield f'spd({D}) {regime}', f'map_{name}', q[name], regime, False
        for squared in (True, False):
            for windowed in (False, True) if regime in REGIMES else (False, ):
                q = dist_quantities(regime, D, squared, windowed)
                for name in PAIR_NAMES:
                    yield (f'spd({D}) {regime}' + (' window %.4g..%.4g' % window(regime, D) if windowed else ''),
                           f'{"wdist" if windowed else "dist"}_{_d(squared)}_{name}', q[name], regime, windowed)
            q = stein_quantities(regime, D, squared)
            for name in PAIR_NAMES:
                yield f'spd({D}) {regime}', f'stein_{_d(squared)}_{name}', q[name], regime, False
        for case in STEP_CASES:
            q = step_quantities(regime, D, case)
            for name in STEP_OUTPUTS[case[0]]:
                yield f'spd({D}) {regime} {step_id(case)}', f'step_{case[0]}_{name}', q[name], regime, False


def compared(D, regimes=ALL_REGIMES):
    for tag, name, q, regime, windowed in candidates(D, regimes):
        if held(name, D, regime, windowed):
            yield tag, name, q, regime, windowed
