"""Cases, inputs, the fp64 oracle and the rule of the Stein-divergence fused objective and node-minibatch kernels
(csrc/spd_stein_loss.hpp: mm_spd_stein_pdiv_loss, _loss_subset, _fwd_subset, _bwd_subset).  Host code only; nothing here runs a
kernel.  tests/test_stein_loss_host.py walks it on the CPU, tests/test_stein_loss_gpu.py makes the calls.

Oracle: softplus(s) * oracle.ref_port.SPD(d).stein_pdiv(x, squared=True) in fp64 through ref.stress_loss /
ref.quotient_loss(**grass_cases.QUOTIENT) with torch autograd: loss, grad_x (symmetrised) and grad_scale.  For a batch it runs on
x[idx] with the targets dense[idx][:, idx] and the gradient is scattered into zeros.

Rule: grass_cases.check — e_new <= 2 e_old + 64 eps max|oracle| per quantity, e_old the deviation of the route the package took
before the fused kernels (forward kernel, the loss in torch ops, backward kernel; for a batch on the gathered rows), measured on
the same GPU in the same test.

Points: `spread` = a a^T + I, a ~ U[0, 1) (the points of the existing Stein tests); `init` = the reference's initialisation
(exp at the identity of a tangent of norm 0.1), drawn in fp64 on the CPU.  Targets: grass_cases.targets (0.5 ... 3.5) resp.
grass_subset_cases.raw_dense (deliberately NOT symmetric) times the median model distance of the case, so that targets and
divergences have one magnitude (`init`: S ~ 1e-3, `spread`: S ~ 0.1 ... 1).

The quotient loss has kinks at m = alpha t and alpha t = m + eps.  A fixed seed alone cannot keep 32 896 pairs (n = 257) 1e-3 away
from both — a pair falls inside that band with probability ~1e-3 — so, as grass_subset_cases.dense does, the target of a pair
inside the band is multiplied by 1.01 (in fp32: the value the kernels read) until it is clear: no pair and no case is left out, and
kink_margin / batch_kink_margin, asserted by the host test for every case, report the margin that results."""
import functools

import torch

import grass_cases as gc
import grass_subset_cases as gsc
from grass_cases import DT, QUOTIENT, SCALE_RAW, CallSpy, check, ref  # noqa: F401

DIMS_ALL = (2, 3, 4, 5, 6, 7, 8, 9)
DIMS = (3, 5)
SIZES = (2, 3, 33, 65, 130, 257)     # the 32-row tile, the 64-column block, several blocks, a ragged last block
REGIMES = ('spread', 'init')
LOSSES = ('stress', 'quotient')
N_TOTAL = 257
BATCHES = (2, 3, 65, 130)
MARGIN = 1e-3
WMIN = 1e-8
STEP = dict(d=3, n=65, bs=33, lr=0.01)


def _sp():
    return torch.nn.functional.softplus(torch.tensor(SCALE_RAW, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def points(regime, n, d):
    """n SPD(d) points, fp64, CPU"""
    g = torch.Generator().manual_seed(gc._seed('stein points', regime, n, d))
    if regime == 'spread':
        a = torch.rand(n, d, d, dtype=torch.float64, generator=g)
        return (a @ a.transpose(1, 2) + torch.eye(d, dtype=torch.float64)).contiguous()
    x = ref.SPD(d).rand(n, dtype=torch.float64, generator=g)
    return (0.5 * (x + x.transpose(1, 2))).contiguous()


def coincident_points(d=3, n=65):
    """`spread` with row 40 a copy of row 7: one pair with S = 0, where the value clamp binds"""
    x = points('spread', n, d).clone()
    x[40] = x[7]
    return x


def model_dists(x, idx=None):
    """softplus(SCALE_RAW) * Stein divergence of the pairs of x (or x[idx]), fp64, no gradient"""
    with torch.no_grad():
        return _sp() * ref.SPD(x.shape[-1], wmin=WMIN).stein_pdiv(x if idx is None else x[idx], squared=True)


def _margins(md, tg):
    ag = tg * QUOTIENT['alpha']
    return (md / ag - 1.0).abs(), (ag / (md + 1.0 / (QUOTIENT['epoch'] + 1)) - 1.0).abs()


def _nudge(md, tg32):
    """fp32 targets of the pairs with model distances md, every one at least MARGIN away from both kinks"""
    tg32 = tg32.clone()
    for _ in range(64):
        a, b = _margins(md, tg32.double())
        bad = (a < MARGIN) | (b < MARGIN)
        if not bool(bad.any()):
            return tg32
        tg32[bad] = tg32[bad] * 1.01
    raise AssertionError('the targets could not be nudged away from the kinks')


@functools.lru_cache(maxsize=None)
def targets(regime, n, d):
    """the target pair vector of the full batch: fp32-representable values as an fp64 tensor"""
    md = model_dists(points(regime, n, d))
    return _nudge(md, (gc.targets(n) * md.median()).float()).double()


def kink_margin(regime, n, d):
    a, b = _margins(model_dists(points(regime, n, d)), targets(regime, n, d))
    return float(torch.minimum(a, b).min())


def batch_idx(bs):
    return gsc.batch_idx(N_TOTAL, bs)


@functools.lru_cache(maxsize=None)
def dense(regime, d, bs):
    """the fp32 dense target matrix [N_TOTAL, N_TOTAL] of the batch: asymmetric, the batch's pairs clear of the kinks"""
    idx = batch_idx(bs)
    i, j = ref.triu_pairs(bs)
    md = model_dists(points(regime, N_TOTAL, d), idx)
    dm = (gsc.raw_dense(N_TOTAL).double() * md.median()).float()
    dm[idx[i], idx[j]] = _nudge(md, dm[idx[i], idx[j]])
    assert float((dm - dm.T).abs().max()) > 0.5 * float(md.median())
    return dm


def batch_kink_margin(regime, d, bs):
    idx = batch_idx(bs)
    i, j = ref.triu_pairs(bs)
    a, b = _margins(model_dists(points(regime, N_TOTAL, d), idx), dense(regime, d, bs)[idx[i], idx[j]].double())
    return float(torch.minimum(a, b).min())


def oracle_loss(loss_name, gd, md):
    return gc.oracle_loss(loss_name, gd, md)


def objective_of(x, tg, loss_name, idx=None, scale_raw=SCALE_RAW):
    """(loss, grad_x symmetrised [n, d, d] — scattered into zeros for a batch —, grad_scale) in fp64"""
    d = x.shape[-1]
    xf = x.clone().requires_grad_(True)
    s = torch.tensor(scale_raw, dtype=torch.float64, requires_grad=True)
    xb = xf if idx is None else xf[idx]
    md = torch.nn.functional.softplus(s) * ref.SPD(d, wmin=WMIN).stein_pdiv(xb, squared=True)
    loss = oracle_loss(loss_name, tg, md)
    gx, gs = torch.autograd.grad(loss, [xf, s])
    assert torch.isfinite(loss) and torch.isfinite(gx).all() and torch.isfinite(gs)
    return loss.detach().reshape(1), 0.5 * (gx + gx.transpose(1, 2)), gs.reshape(1)


@functools.lru_cache(maxsize=None)
def full_oracle(regime, n, d, loss_name):
    return objective_of(points(regime, n, d), targets(regime, n, d), loss_name)


@functools.lru_cache(maxsize=None)
def batch_oracle(regime, d, bs, loss_name):
    idx = batch_idx(bs)
    i, j = ref.triu_pairs(bs)
    return objective_of(points(regime, N_TOTAL, d), dense(regime, d, bs)[idx[i], idx[j]].double(), loss_name, idx)


def upstream(m):
    """a fixed upstream gradient of a pair vector of m entries (both signs, O(1))"""
    g = torch.Generator().manual_seed(gc._seed('stein upstream', m))
    return torch.randn(m, dtype=torch.float64, generator=g)


def pdiv_oracle(x, idx, squared):
    """(pair vector of x[idx], symmetrised gradient of sum(upstream * value) w.r.t. the full table), fp64"""
    xf = x.clone().requires_grad_(True)
    v = ref.SPD(x.shape[-1], wmin=WMIN).stein_pdiv(xf[idx], squared=squared)
    gx, = torch.autograd.grad((v * upstream(v.numel())).sum(), [xf])
    return v.detach(), 0.5 * (gx + gx.transpose(1, 2))


def loss_spec(loss_name):
    return gsc.loss_spec(loss_name)


def step_oracle(x, grad, optimizer):
    """the points after one step of ref.rsgd_step / ref.radam_step on ref_port.SPD(d) with the gradient `grad` (retraction)"""
    man = ref.SPD(x.shape[-1])
    if optimizer == 'rsgd':
        return ref.rsgd_step(man, x, grad, lr=STEP['lr'])[0]
    return ref.radam_step(man, x, grad, {}, lr=STEP['lr'])
