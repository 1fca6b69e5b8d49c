"""Cases, inputs, fp64 oracles and the ABSOLUTE tolerance rule of tests/test_mat_oracle_gpu.py (checked on the CPU by
tests/test_mat_cases_host.py): every (NP, P) instantiation of the Grassmann / Stiefel device code (csrc/mat_common.hpp, mat.hip,
mat_step.hip, grass_loss.hip) against oracle/ref_port.py in fp64.  Host code only; nothing here runs a kernel.

Inputs come from grass_cases.frames (regimes `uniform`, `spread`, `init`; N = p: `uniform` only), tangents / ambient vectors are
fixed-seed uniform in [-0.3, 0.3], y = roll(x, 1), and everything is rounded to float32 first and widened afterwards: fp32
kernels, fp64 kernels and the oracle see the same numbers.  The upstream g is stereo_cases.upstream.

The rule, built from the reference alone.  For a quantity with oracle value W and scale S
    cond     = largest max|oracle(perturbed inputs) - W| over DRAWS fixed-seed draws, each multiplying every entry of the point /
               vector inputs (not g, not the targets, not the scale parameter) by 1 + delta, delta uniform in +-2^-24: the oracle's
               response to ONE fp32 rounding of the inputs (the problem's conditioning);
    port32   = max|ref_port in float32 on the CPU - W|, absent where that result is not all finite;
    bound_f32 = max(32 cond, 2 port32) + 16 2^-24 S
    bound_f64 = 2^-29 max(64 cond, 4 port32) + 64 2^-53 S
32 input roundings cover a 9-term Gram chain, at most six Jacobi sweeps of at most six rotations and the transcendental calls;
2 port32 is the stereographic rule (never better than twice the reference's own fp32 arithmetic), which matters where a formula
cancels on purpose (the p = 2 closed-form singular values, log near orthogonal subspaces); fp64 scales both terms by 2^-53 / 2^-24
and doubles the margins because there the oracle's rounding is of the kernel's order.
S: maps max(1, max|W|); distances max|W|; gradients max_j sum_i |g_ij| |term_ij| (the magnitude sum of the oracle's per-pair
contributions; with a mixed-sign g the sum itself cancels).

Compared quantities, per dtype (SHAPES: 26, of them 22 with N > p and the 4 with N = p; regimes: 3, at N = p `uniform` only):
  maps    Grassmann proju projx retr retr_qr transp egrad2rgrad exp, + log at N > p; cnt = 130              (22 x 3 + 4) x 7 + 66 = 556
          Stiefel   proju projx retr retr_qr transp egrad2rgrad                                             (22 x 3 + 4) x 6      = 420
          log with a leading pivot of exactly 0 in y^T x (PIVOT_SHAPES: N > p >= 2)                                                  16
  dist    cnt = 130 pairs (x, roll x), autograd's two launches and the one-launch form:
          d2 value (`uniform`, `spread`; N > p)                                                             22 x 2                =  44
          d2 grad_x, grad_y (all regimes, N = p included; not p = 2 `uniform`)                              (70 - 6) x 2          = 128
          d value (`uniform`, N > p, not Gr(2,1)); d grad_x, grad_y (of those, not p = 2)                   21 + 15 x 2           =  51
  pdist   n in PDIST_N: d2 value / d2 gradient / d value / d gradient, the same selection                   219 + 320 + 105 + 75  = 719
          (and no d2 value of Gr(2,1) `spread` n = 2: its two points coincide, S = 0)
          ROWS of n = 129 at ROW_SHAPES, squared: 4 non-empty ranges, value / gradient                      32 + 44               =  76
          n = 257 at ROW_SHAPES, squared, `uniform`, 2 draws: value / gradient                              4 + 3                 =   7
          coincident points (point 7 := point 3), `spread`, n = 65, COINCIDENT shapes                       4 x 2                 =   8
  fused   pdist_loss (stress, n = 65) at FUSED: loss, grad_x; grad_scale (`uniform`, `spread`; N > p)       17 + 17 + 10          =  44
          rsgd_step (cnt = 65, clip at the median norm, `uniform`) at FUSED: Grassmann svd / qr / exp,
          Stiefel svd / qr                                                                                  7 x 5                 =  35
                                                                                                                          total   2104
Not held to the rule, because max(32 cond, 2 port32) alone exceeds 1e-3 S there — the rule would be vacuous, and
tests/test_mat_cases_host.py holds bound_f32 <= 1e-3 S for everything above:
  * every distance VALUE in `init` (d2 ~ 2e-4 responds to one input rounding with ~1e-3 of itself: 32 cond = 3-7 % of S) and
    d loss / d scale there (the same sum); the d2 GRADIENT in `init` is well conditioned and is compared;
  * every distance value at N = p (all cosines are 1: S ~ 1e-7 from the rounding of the inputs alone), d loss / d scale at N = p;
    the d2 gradient -2 x_i polar(G) is compared, the non-squared gradient is 0/0 in the reference (finite in fp64 is asserted);
  * gradients at p = 2 in `uniform`: the reference's closed-form singular values cancel and its own fp32 gradient is off by 0.1-3 %
    of S (port32), so 2 port32 bounds nothing; `spread` and `init` at p = 2 are compared;
  * the non-squared gradient at `spread` / `init` (cond is 0.1-7 % of S) and everything non-squared on Gr(2,1) (130 points on a
    circle: some pairs are 1e-3 apart and d = sqrt(d2) amplifies).
"""
import functools
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'matrix-manifolds_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import grass_cases as gc  # noqa: E402
from grass_cases import _seed, eps_of, frames, ref  # noqa: E402,F401
from stereo_cases import upstream as _upstream  # noqa: E402

DT = gc.DT
U32, U64 = 2.0**-24, 2.0**-53
DRAWS = 8
CAP = 1e-3
CNT = 130
PREFIXES = (1, 63, 64, 65)
PDIST_N = (2, 3, 65, 129, 130)
LR = 0.05

SHAPES = [(1, 1), (2, 1), (4, 1), (2, 2), (3, 2), (4, 2), (3, 3), (4, 3), (4, 4),
          (5, 1), (6, 1), (5, 2), (6, 2), (5, 3), (6, 3), (5, 4), (6, 4),
          (7, 1), (9, 1), (8, 2), (9, 2), (7, 3), (9, 3), (7, 4), (8, 4), (9, 4)]
ROW_SHAPES = [(4, 1), (5, 2), (6, 3), (9, 4)]
COINCIDENT = [(4, 1), (5, 2), (6, 3), (9, 4)]   # one per P
FUSED = [(2, 1), (3, 3), (4, 4), (6, 4), (7, 3), (8, 4), (9, 1)]   # the shapes test_grass_loss_gpu / test_mat_step_gpu do not list
GRASS_OPS = ('proju', 'projx', 'retr', 'retr_qr', 'transp', 'egrad2rgrad', 'exp', 'log')
STIEFEL_OPS = ('proju', 'projx', 'retr', 'retr_qr', 'transp', 'egrad2rgrad')
STEP_VARIANTS = {'grassmann': (('svd', False), ('qr', False), ('svd', True)), 'stiefel': (('svd', False), ('qr', False))}

RATIOS = {}   # (quantity, dtype) -> (largest err / bound seen, its tag), kept by check()


def regimes(N, p):
    return ('uniform', ) if N == p else ('uniform', 'spread', 'init')


def ops_of(kind, N, p):
    ops = GRASS_OPS if kind == 'grassmann' else STIEFEL_OPS
    return tuple(o for o in ops if not (o == 'log' and N == p))


def _closed_form_uniform(regime, N, p):
    """p = 2 away from the identity: the reference's closed-form singular values cancel, its own fp32 gradient is off by percents"""
    return p == 2 and N > p and regime == 'uniform'


def dist_compared(regime, N, p, squared, n=None):
    """names of the element-wise dist / pdist quantities held to the rule (see the module docstring for what is dropped and why)"""
    if squared:
        names = []
        if N > p and regime != 'init' and not ((N, p) == (2, 1) and n == 2 and regime == 'spread'):
            names.append('val')
        if not _closed_form_uniform(regime, N, p):
            names.append('grad')
    else:
        names = ['val', 'grad'] if regime == 'uniform' and N > p and (N, p) != (2, 1) else []
        if _closed_form_uniform(regime, N, p):
            names.remove('grad')
    return tuple(n_ for name in names for n_ in (('grad_x', 'grad_y') if name == 'grad' and n is None else (name, )))


def pdist_compared(regime, n, N, p, squared):
    return dist_compared(regime, N, p, squared, n)


def loss_compared(regime, N, p):
    """d loss / d scale = sum 2 (md - t) d2 sigmoid: as ill-conditioned as d2 itself at `init`, and ~0 at N = p"""
    return ('loss', 'grad_x', 'grad_scale') if N > p and regime != 'init' else ('loss', 'grad_x')


def rows_of(n):
    """the full range, [0, 1), the middle third, the last row that has a pair, the last row (no pair), an empty range"""
    return (None, (0, 1), (n // 3, 2 * n // 3), (n - 2, n - 1), (n - 1, n), (5, 5))


def pair_slice(n, rows):
    off = lambda r: r * (2 * n - r - 1) // 2   # noqa: E731
    rb, re = (0, n) if rows is None else rows
    return off(rb), off(re)


def upstream(k):
    """fixed pattern with both signs, fp64"""
    return torch.from_numpy(_upstream(k).astype(np.float64))


# ---- inputs (all float32) ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points(regime, n, N, p, coincide=False):
    x = frames(regime, n, N, p).float()
    if coincide:
        x = x.clone()
        x[7] = x[3]
    return x


@functools.lru_cache(maxsize=None)
def vectors(tag, cnt, N, p):
    g = torch.Generator().manual_seed(_seed('vectors', tag, cnt, N, p))
    return ((torch.rand(cnt, N, p, dtype=torch.float64, generator=g) * 2 - 1) * 0.3).float()


@functools.lru_cache(maxsize=None)
def map_inputs(kind, regime, N, p):
    """x, u (ambient), y = roll(x), t (u projected onto the tangent space at x by the oracle, then rounded), a = x + u / 2
    (an ambient full-rank matrix for projx) — float32, CNT points"""
    x = points(regime, CNT, N, p)
    u = vectors('ambient', CNT, N, p)
    t = ref.make(kind, N, p).proju(x.double(), u.double()).float()
    return x, u, torch.roll(x, 1, 0), t, (x.double() + 0.5 * u.double()).float()


# ---- the rule ------------------------------------------------------------------------------------------------------------------
class Quantity:
    __slots__ = ('want', 'cond', 'port32', 'scale')

    def __init__(self, want, cond, port32, scale):
        self.want, self.cond, self.port32, self.scale = want, cond, port32, scale

    def bound(self, dname):
        p32 = 0.0 if self.port32 is None else self.port32
        if dname == 'f32':
            return max(32 * self.cond, 2 * p32) + 16 * U32 * self.scale
        return 2.0**-29 * max(64 * self.cond, 4 * p32) + 64 * U64 * self.scale


def _dev(a, b):
    return float((a.double() - b).abs().max()) if b.numel() else 0.0


def _perturbed(t, key, draw, k):
    g = torch.Generator().manual_seed(_seed('perturb', key, draw, k))
    return t.double() * (1 + (torch.rand(t.shape, dtype=torch.float64, generator=g) * 2 - 1) * U32)


def measure(fn, inputs, key, draws=DRAWS):
    """fn(*inputs) -> ({name: tensor}, {name: 'map' | 'dist' | float}); inputs are float32 tensors.  Returns {name: Quantity}."""
    want, kinds = fn(*[t.double() for t in inputs])
    cond = dict.fromkeys(want, 0.0)
    for d in range(draws):
        got, _ = fn(*[_perturbed(t, key, d, k) for k, t in enumerate(inputs)])
        for name in want:
            cond[name] = max(cond[name], _dev(got[name], want[name]))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            got32, _ = fn(*[t.float() for t in inputs])
    except Exception:   # noqa: BLE001  (a singular fp32 solve: no fp32 port of this quantity)
        got32 = {}
    out = {}
    for name, w in want.items():
        assert torch.isfinite(w).all(), (key, name)
        r = got32.get(name)
        p32 = _dev(r, w) if r is not None and bool(torch.isfinite(r).all()) else None
        s = kinds[name]
        wmax = float(w.abs().max()) if w.numel() else 0.0
        scale = max(1.0, wmax) if s == 'map' else wmax if s == 'dist' else float(s)
        out[name] = Quantity(w.detach(), cond[name], p32, scale)
    return out


def check(tag, what, got, q, dname, failures):
    """One comparison under the rule: prints err / bound, records the worst ratio, appends a line to `failures` on a miss."""
    got = got.detach().double().cpu()
    assert got.shape == q.want.shape, (tag, what, got.shape, q.want.shape)
    err, bnd = (_dev(got, q.want) if bool(torch.isfinite(got).all()) else float('inf')), q.bound(dname)
    ratio = err / bnd if bnd > 0 else (0.0 if err == 0 else float('inf'))
    key = (what.split('@')[0], dname)
    if ratio > RATIOS.get(key, (-1.0, ''))[0]:
        RATIOS[key] = (ratio, tag)
    line = f'{tag} {what} {dname}: err {err:.3e} / bound {bnd:.3e} = {ratio:.3f}  (cond {q.cond:.2e} port32 ' \
           f'{"-" if q.port32 is None else format(q.port32, ".2e")} S {q.scale:.2e})'
    print(line)
    if not err <= bnd:
        failures.append(line)


# ---- oracles -------------------------------------------------------------------------------------------------------------------
class _Acos(torch.autograd.Function):
    """acos whose derivative is formed as -1 / sqrt((1 - s)(1 + s)): 1 - s is exact next to 1, 1 - s*s is not"""

    @staticmethod
    def forward(ctx, s):
        ctx.save_for_backward(s)
        return s.acos()

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return -g * ((1 - s) * (1 + s)).rsqrt()


def _singular_values_2x2(x, eps=ref.EPS):
    """ref_port.singular_values_2x2 with s2^2 = (S1 - sqrt S2)/2 formed as 2 det^2 / (S1 + sqrt S2) while the clamp on S2 is
    idle (S1^2 - S2 = 4 det^2): the same function without the cancellation.  In fp64 the port's own form is 1.4e-13 off the
    40-digit value of d^2 at Gr(9,2) `uniform` (tests/test_mat_cases_host.py), which is bound_f64 there."""
    a, b, c, d = x[..., 0, 0], x[..., 0, 1], x[..., 1, 0], x[..., 1, 1]
    S1 = a**2 + b**2 + c**2 + d**2
    S2 = (a**2 + b**2 - c**2 - d**2)**2 + 4 * (a * c + b * d)**2
    R = torch.sqrt(ref.vclamp(S2, eps))
    s1 = ref.vclamp(0.5 * (S1 + R), eps)
    s2 = ref.vclamp(torch.where(S2 >= eps, 2 * (a * d - b * c)**2 / (S1 + R), 0.5 * (S1 - R)), eps)
    return torch.stack([torch.sqrt(s1), torch.sqrt(s2)], dim=-1)


class OracleGrassmann(ref.Grassmann):
    """ref_port.Grassmann for the fp64 oracle: `dist` is the port's, line by line, with the derivative of acos and the smaller
    singular value of the p = 2 closed form evaluated without cancellation.  torch forms it from 1 - s*s, whose rounding (1e-16 absolute) is 3e-9 of the gradient where 1 - s ~ 1e-8 —
    coincident points, and every shape with 2p > N once the inputs are rounded to float32; measured against 40-digit arithmetic
    the port's fp64 gradient is 1.0e-9 off at Gr(2,1) `init`, n = 3, which is 30 000 x bound_f64, and the kernels (which use
    fma(-s, s, 1)) agree with the 40-digit value.  The float32 port (port32) stays the port itself."""

    def dist(self, x, y, squared=False, keepdim=False):
        if x.dtype != torch.float64:
            return super().dist(x, y, squared, keepdim)
        xty = x.transpose(-2, -1) @ y
        s = _singular_values_2x2(xty) if self.p == 2 else torch.linalg.svdvals(xty)
        s = ref.vclamp(s, -1 + ref.EPS**2, 1 - ref.EPS**2)
        dsq = _Acos.apply(s).pow(2).sum(-1, keepdim=keepdim)
        return dsq if squared else dsq.sqrt()


def _retr_qr(kind, man):
    return (lambda x, u: torch.linalg.qr(x + u)[0]) if kind == 'grassmann' else man.retr_qr   # grassmann.py:71-74 / stiefel.py:62-63


@functools.lru_cache(maxsize=None)
def map_quantities(kind, regime, N, p):
    man = ref.make(kind, N, p)
    ops = ops_of(kind, N, p)

    def fn(x, u, y, t, a):
        out = {'proju': man.proju(x, u), 'egrad2rgrad': man.egrad2rgrad(x, u), 'transp': man.transp(x, y, u),
               'retr': man.retr(x, t), 'retr_qr': _retr_qr(kind, man)(x, t),
               'projx': man.projx(a) if kind == 'grassmann' else man.orthonormalize(a)}
        if 'exp' in ops:
            out['exp'] = man.exp(x, t)
        if 'log' in ops:
            out['log'] = man.log(x, y)
        return out, dict.fromkeys(out, 'map')
    return measure(fn, map_inputs(kind, regime, N, p), ('maps', kind, regime, N, p))


PIVOT_SHAPES = [(N, p) for (N, p) in SHAPES if N > p >= 2]


@functools.lru_cache(maxsize=None)
def pivot_inputs(N, p):
    """log_x(y) whose p x p system y^T x has a leading entry of exactly 0, so that the Gauss-Jordan elimination of the kernel
    has to swap rows in its first step: x = the first p columns of the identity, y = `uniform` frames with columns 0 and 1
    rotated until y[0][0] vanishes (then y^T x = the transposed top block of y).  float32, CNT points."""
    y = frames('uniform', CNT, N, p).clone()
    a, b = y[:, 0, 0].clone(), y[:, 0, 1].clone()
    r = torch.sqrt(a * a + b * b)
    c0, c1 = y[:, :, 0].clone(), y[:, :, 1].clone()
    y[:, :, 0] = (b / r).unsqueeze(-1) * c0 - (a / r).unsqueeze(-1) * c1
    y[:, :, 1] = (a / r).unsqueeze(-1) * c0 + (b / r).unsqueeze(-1) * c1
    y = y.float()
    y[:, 0, 0] = 0.0
    return torch.eye(N, p).expand(CNT, N, p).contiguous(), y


@functools.lru_cache(maxsize=None)
def pivot_quantities(N, p):
    man = ref.Grassmann(N, p)
    return measure(lambda x, y: ({'log': man.log(x, y)}, {'log': 'map'}), pivot_inputs(N, p), ('pivot', N, p))


@functools.lru_cache(maxsize=None)
def dist_quantities(regime, N, p, squared):
    """element-wise dist of CNT pairs (x, roll x): value, grad_x, grad_y of sum_k g_k d_k (each pair is one term: S = max|W|)"""
    man = OracleGrassmann(N, p)
    x = points(regime, CNT, N, p)

    def fn(x, y):
        x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        d = man.dist(x, y, squared=squared)
        gx, gy = torch.autograd.grad((d * upstream(CNT).to(d.dtype)).sum(), [x, y])
        return {'val': d.detach(), 'grad_x': gx, 'grad_y': gy}, {'val': 'dist', 'grad_x': 'dist', 'grad_y': 'dist'}
    return measure(fn, (x, torch.roll(x, 1, 0)), ('dist', regime, N, p, squared))


def _pairs(man, x, squared):
    """(d [npairs], dd/dx_i, dd/dx_j per pair) through autograd of the port on the gathered points"""
    i, j = ref.triu_pairs(x.shape[0])
    xi, xj = x[i].clone().requires_grad_(True), x[j].clone().requires_grad_(True)
    d = man.dist(xi, xj, squared=squared)
    ji, jj = torch.autograd.grad(d.sum(), [xi, xj])
    return i, j, d.detach(), ji, jj


def _scatter(n, i, j, ti, tj):
    return torch.zeros(n, *ti.shape[1:], dtype=ti.dtype).index_add_(0, i, ti).index_add_(0, j, tj)


@functools.lru_cache(maxsize=None)
def pdist_quantities(regime, n, N, p, squared, ranges=(None, ), draws=DRAWS, coincide=False):
    """{(rows, 'val' | 'grad'): Quantity} of Grassmann.pdist(x, squared, rows) with the upstream pattern on the slice.  The
    per-pair derivatives are formed once per evaluation of the oracle and shared by every row range."""
    man = OracleGrassmann(N, p)

    def fn(x):
        i, j, d, ji, jj = _pairs(man, x, squared)
        vals, kinds = {}, {}
        for r in ranges:
            lo, hi = pair_slice(n, r)
            g = torch.zeros(d.numel(), dtype=d.dtype)
            g[lo:hi] = upstream(hi - lo).to(d.dtype)
            gi, gj = g.reshape(-1, 1, 1) * ji, g.reshape(-1, 1, 1) * jj
            vals[(r, 'val')], kinds[(r, 'val')] = d[lo:hi], 'dist'
            vals[(r, 'grad')] = _scatter(n, i, j, gi, gj)
            kinds[(r, 'grad')] = float(_scatter(n, i, j, gi.abs(), gj.abs()).max())
        return vals, kinds
    return measure(fn, (points(regime, n, N, p, coincide), ), ('pdist', regime, n, N, p, squared, coincide), draws)


@functools.lru_cache(maxsize=None)
def loss_quantities(regime, n, N, p):
    """loss, grad_x, grad_scale of stress(targets, softplus(scale) pdist^2) — ref_port.compute_dists / stress_loss on the pair list"""
    man = OracleGrassmann(N, p)

    def fn(x):
        i, j = ref.triu_pairs(n)
        xi, xj = x[i].clone().requires_grad_(True), x[j].clone().requires_grad_(True)
        s = torch.tensor(gc.SCALE_RAW, dtype=x.dtype, requires_grad=True)
        d2 = man.dist(xi, xj, squared=True)
        md = torch.nn.functional.softplus(s) * d2
        tg = gc.targets(n).to(x.dtype)
        loss = ref.stress_loss(tg, md)
        ti, tj, gs = torch.autograd.grad(loss, [xi, xj, s])
        per_pair_s = 2 * (md - tg).detach() * d2.detach() * torch.sigmoid(s.detach())
        vals = {'loss': loss.detach().reshape(1), 'grad_x': _scatter(n, i, j, ti, tj), 'grad_scale': gs.reshape(1)}
        kinds = {'loss': 'dist', 'grad_x': float(_scatter(n, i, j, ti.abs(), tj.abs()).max()), 'grad_scale': float(per_pair_s.abs().sum())}
        return vals, kinds
    return measure(fn, (points(regime, n, N, p), ), ('loss', regime, n, N, p))


def egrad(cnt, N, p):
    return vectors('egrad', cnt, N, p)


@functools.lru_cache(maxsize=None)
def step_clip(kind, cnt, N, p):
    """the median Riemannian gradient norm of the case: both branches of the clip in one launch"""
    man = ref.make(kind, N, p)
    x, g = points('uniform', cnt, N, p).double(), egrad(cnt, N, p).double()
    return float(man.norm(x, man.egrad2rgrad(x, g)).median())


@functools.lru_cache(maxsize=None)
def step_quantities(kind, retr, exact, cnt, N, p):
    man = ref.make(kind, N, p)
    if retr == 'qr':
        man.retr = _retr_qr(kind, man)
    clip = step_clip(kind, cnt, N, p)

    def fn(x, g):
        return {'x_new': ref.rsgd_step(man, x, g, lr=LR, max_grad_norm=clip, exact=exact)[0]}, {'x_new': 'map'}
    return measure(fn, (points('uniform', cnt, N, p), egrad(cnt, N, p)), ('step', kind, retr, exact, cnt, N, p))


# ---- the list of compared quantities (walked by tests/test_mat_cases_host.py; tests/test_mat_oracle_gpu.py makes the same calls) ----
def compared(N, p):
    """(tag, name, Quantity, lucky) of everything the GPU tests hold to the rule at this shape.  `lucky`: the reference's fp32
    arithmetic can be (nearly) exact there, so port32 is no yardstick for cond — one or three pairs (n <= 3), Gr(2,1) where x^T y
    is a two-term dot product, and the two scalar sums of the objective."""
    for tag, name, q in _compared(N, p):
        yield tag, name, q, (N, p) == (2, 1) or ' n=2' in tag or ' n=3' in tag or name in ('loss_loss', 'loss_grad_scale')


def _compared(N, p):
    for regime in regimes(N, p):
        for kind in ('grassmann', 'stiefel'):
            q = map_quantities(kind, regime, N, p)
            for op in ops_of(kind, N, p):
                yield f'{kind} {N}x{p} {regime}', f'map_{op}', q[op]
        for squared in (True, False):
            names = dist_compared(regime, N, p, squared)
            if names:
                q = dist_quantities(regime, N, p, squared)
                for name in names:
                    yield f'dist {N}x{p} {regime}', f'dist_{"d2" if squared else "d"}_{name}', q[name]
            for n in PDIST_N:
                names = pdist_compared(regime, n, N, p, squared)
                if names:
                    q = pdist_quantities(regime, n, N, p, squared)
                    for name in names:
                        yield f'pdist {N}x{p} {regime} n={n}', f'pdist_{"d2" if squared else "d"}_{name}', q[(None, name)]
        if (N, p) in ROW_SHAPES:
            q = pdist_quantities(regime, 129, N, p, True, rows_of(129))
            for rows in rows_of(129):
                for name in pdist_compared(regime, 129, N, p, True):
                    if pair_slice(129, rows)[0] < pair_slice(129, rows)[1]:   # (an empty range: nothing to bound, zeros are asserted)
                        yield f'pdist {N}x{p} {regime} n=129 rows={rows}', f'pdist_rows_{name}', q[(rows, name)]
        if (N, p) in FUSED:
            q = loss_quantities(regime, 65, N, p)
            for name in loss_compared(regime, N, p):
                yield f'objective {N}x{p} {regime} n=65', f'loss_{name}', q[name]
    if (N, p) in PIVOT_SHAPES:
        yield f'grassmann {N}x{p} zero leading pivot', 'map_log_pivot', pivot_quantities(N, p)['log']
    if (N, p) in ROW_SHAPES:
        q = pdist_quantities('uniform', 257, N, p, True, (None, ), 2)
        for name in pdist_compared('uniform', 257, N, p, True):
            yield f'pdist {N}x{p} uniform n=257', f'pdist_d2_{name}', q[(None, name)]
    if (N, p) in COINCIDENT:
        q = pdist_quantities('spread', 65, N, p, True, (None, ), DRAWS, True)
        for name in ('val', 'grad'):
            yield f'pdist {N}x{p} spread n=65 coincident', f'pdist_coincident_{name}', q[(None, name)]
    if (N, p) in FUSED:
        for kind, variants in STEP_VARIANTS.items():
            for retr, exact in variants:
                yield f'rsgd {kind} {N}x{p} cnt=65', f'step_{"exp" if exact else retr}', step_quantities(kind, retr, exact, 65, N, p)['x_new']
