"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py) — ONE training step in fp64.

The loop body of the reference's trainer (train.py:198-222)

    loss = objective(indices, epoch=epoch, alpha=alpha); zero_grad(); loss.backward(); step()

restated as a function of everything the step reads, returning everything it writes.  The tests feed it the state
the device actually holds before a step and compare what the device wrote afterwards, one step at a time, so
nothing accumulates between the two.

Arithmetic, independent of the library under test:
* squared distances and their gradients: oracle/exact.c (`exact.spd_pairs`, `exact.vec_pairs` and their `_grad`);
* the losses (objectives.py:16-45) and their derivatives: numpy, below;
* the scale enters as softplus(s) * d^2 (modules.py:84-88);
* the optimizer rules: `ref_port.rsgd_step` / `ref_port.radam_step` on the port's manifolds — with
  `torch.linalg` Cholesky and `eigh` for EVERY SPD dimension (`ExactSPD`): the reference's eps-fudged 2x2 / 3x3
  closed forms bias fp64 by 1e-8 to 1e-6.  The value clamps that are the reference's semantics stay
  (`Manifold.norm`'s floor, the sphere's small-step branch, no floor in `SPD.norm`).

`port_step` is the same step in the port's own arithmetic (autograd, closed forms) at a chosen dtype: what a plain
fp32 evaluation of a step gives, the yardstick the GPU tolerances are held against.

A case is described by plain data:
  factors      [('spd', 3), ('lorentz', 11), ...]
  xs, scales   fp64 numpy arrays ([n, d, d] / [n, m]) and floats (the RAW scale s; softplus(s) multiplies d^2)
  target       pair vector of squared graph distances (row-major i < j), or `dense` [n, n] plus `idx`
  loss         {'kind': 'stress'} or {'kind': 'quotient', 'epoch': e, 'alpha': a, 'inc_l1': True, 'inc_l2': True}
  rule         {'opt': 'rsgd', 'lr', 'momentum', 'dampening', 'max_grad_norm', 'exact'} or
               {'opt': 'radam', 'lr', 'betas', 'nc', 'max_grad_norm', 'exact'} or None (frozen: burn-in)
  state        per parameter: {} | {'momentum_buffer'} | {'exp_avg', 'exp_avg_sq', 'step'}
"""
import numpy as np
import torch

from oracle import exact
from oracle import ref_port as rp


class ExactSPD(rp.SPD):
    """`ref_port.SPD` with LAPACK factorisations for every n (no eps-fudged closed forms)."""

    def symeig(self, x):
        return rp._eigh_upper(x)[0]

    def chol(self, x):
        return torch.linalg.cholesky(x)

    def invchol(self, x, ret_chol=False):
        l = torch.linalg.cholesky(x)
        eye = torch.eye(self.n, dtype=x.dtype, device=x.device).expand_as(l)
        l_inv = torch.linalg.solve_triangular(l, eye, upper=False)
        return l_inv, (l if ret_chol else None)


def manifold(factor, closed_forms=False):
    kind, dim = factor
    if kind == 'spd' and not closed_forms:
        return ExactSPD(dim)
    return rp.make(kind, dim)


FLAT = rp.Euclidean(1)   # a scale is one point of R^1 (the optimizers' default manifold)


# ------------------------------------------------------------------------------------------------------------ the objective
def pair_list(n, idx=None):
    """(i, j) node ids of the step's pairs, in the order of the reference's pair vector: all i < j of range(n), or — for a
    node minibatch — (idx[a], idx[b]) for the positions a < b of the batch (the pairs of x[idx], modules.py:86)."""
    if idx is None:
        a, b = np.triu_indices(n, 1)
        return a.astype(np.int64), b.astype(np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    a, b = np.triu_indices(idx.size, 1)
    return idx[a], idx[b]


def pair_targets(target, dense, i, j):
    if dense is not None:
        return np.asarray(dense, dtype=np.float64)[i, j]
    target = np.asarray(target, dtype=np.float64)
    assert target.shape == i.shape, (target.shape, i.shape)
    return target


def loss_and_slope(loss, gd, md):
    """(value, d value / d md) of objectives.py:16-45 on pair vectors: gd graph distances, md manifold distances (squared)."""
    if loss['kind'] == 'stress':
        r = md - gd
        return float((r * r).sum()), 2.0 * r
    assert loss['kind'] == 'quotient', loss
    gd = gd * float(loss.get('alpha', 1.0))
    eps = 1.0 / (loss['epoch'] + 1)
    value, slope = 0.0, np.zeros_like(md)
    if loss.get('inc_l1', True):
        q = md / gd - 1.0
        value += float(np.abs(q).sum())
        slope += np.sign(q) / gd
    if loss.get('inc_l2', True):
        q = gd / (md + eps) - 1.0
        value += float(np.abs(q).sum())
        slope -= np.sign(q) * gd / (md + eps)**2
    return value, slope


def softplus(s):
    return float(np.logaddexp(0.0, s))


def sigmoid(s):
    return float(1.0 / (1.0 + np.exp(-s)))


def _d2_and_grad(factor, x, lo, hi, g=None):
    kind, _ = factor
    if lo.size == 0:
        return np.zeros(0) if g is None else np.zeros_like(x)
    if kind == 'spd':
        return exact.spd_pairs(x, lo, hi) if g is None else exact.spd_pairs_grad(x, lo, hi, g)
    return exact.vec_pairs(kind, x, lo, hi) if g is None else exact.vec_pairs_grad(kind, x, lo, hi, g)


def pair_distances(factors, xs, idx=None, pairs=None):
    """Squared distances of every factor over the step's pair list (the expensive half of `objective`)."""
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    i, j = pair_list(xs[0].shape[0], idx) if pairs is None else _explicit_pairs(pairs)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return [_d2_and_grad(f, x, lo, hi) for f, x in zip(factors, xs)]


def kink_distance(loss, gd, md):
    """Per pair: how far the loss term is from a kink of its |.| (quotient: min |q| over the included terms; stress has
    none).  At a kink the derivative jumps, so an evaluation in another precision may land on the other side."""
    if loss['kind'] == 'stress':
        return np.full(md.shape, np.inf)
    gd = gd * float(loss.get('alpha', 1.0))
    eps = 1.0 / (loss['epoch'] + 1)
    out = np.full(md.shape, np.inf)
    if loss.get('inc_l1', True):
        out = np.minimum(out, np.abs(md / gd - 1.0))
    if loss.get('inc_l2', True):
        out = np.minimum(out, np.abs(gd / (md + eps) - 1.0))
    return out


def _explicit_pairs(pairs):
    i, j = (np.ascontiguousarray(p, dtype=np.int64) for p in pairs)
    assert i.shape == j.shape and i.ndim == 1, (i.shape, j.shape)
    return i, j


def objective(factors, xs, scales, loss, target=None, dense=None, idx=None, d2=None, pairs=None):
    """Loss and the Euclidean gradients of every factor's points (dense: zero rows outside a minibatch; SPD: the symmetric
    part) and raw scales.  `d2`: the result of `pair_distances` on the same points, when the caller has it already.
    `pairs`: an explicit (i, j) list of node pairs in place of `pair_list(n, idx)` — a row shard of the pair vector, say;
    `target` then holds one entry per listed pair (points no listed pair touches get zero gradients)."""
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    n = xs[0].shape[0]
    i, j = pair_list(n, idx) if pairs is None else _explicit_pairs(pairs)
    gd = pair_targets(target, dense, i, j)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    if d2 is None:
        d2 = [_d2_and_grad(f, x, lo, hi) for f, x in zip(factors, xs)]
    md = sum(softplus(s) * d for s, d in zip(scales, d2))
    value, slope = loss_and_slope(loss, gd, md)
    grads = [softplus(s) * _d2_and_grad(f, x, lo, hi, slope) for f, x, s in zip(factors, xs, scales)]
    sgrads = [sigmoid(s) * float((slope * d).sum()) for s, d in zip(scales, d2)]
    return value, grads, sgrads


# ------------------------------------------------------------------------------------------------------- the optimizer rules
def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).clone()


def _state_in(state, shape, dtype):
    out = {}
    for k, v in (state or {}).items():
        out[k] = int(round(float(v))) if k == 'step' else _t(v, dtype).reshape(shape)
    return out


def apply_rule(man, x, grad, rule, state):
    """One optimizer update of one parameter (torch tensors of one dtype): (new_x, new_state, diagnostics).

    Diagnostics, per point: `rgrad_norm` the norm of the Riemannian gradient in the manifold's metric (the quantity the
    clip compares), `binds` whether the clip shortens it, `step_norm` the norm of the tangent vector handed to exp / retr."""
    if rule is None:
        return x.clone(), dict(state or {}), None
    clip = rule.get('max_grad_norm')
    move = bool(rule.get('exact', False))
    with torch.no_grad():
        rg = man.egrad2rgrad(x, grad)
        gn = man.norm(x, rg, keepdim=True)
        binds = gn > clip if clip is not None else torch.zeros_like(gn, dtype=torch.bool)
        gc = rg * torch.clamp(clip / gn, max=1.0) if clip is not None else rg
    if rule['opt'] == 'rsgd':
        momentum = float(rule.get('momentum', 0.0))
        buf = (state or {}).get('momentum_buffer')
        new_x, new_buf = rp.rsgd_step(man, x, grad, lr=rule['lr'], momentum=momentum, dampening=float(rule.get('dampening', 0.0)),
                                      max_grad_norm=clip, exact=move, momentum_buffer=buf)
        new_state = {} if new_buf is None else {'momentum_buffer': new_buf}
        with torch.no_grad():
            if momentum > 0:
                start = grad if buf is None else buf     # rsgd.py:53-54
                tangent = rule['lr'] * (start * momentum + (1 - float(rule.get('dampening', 0.0))) * gc)
            else:
                tangent = rule['lr'] * gc
    else:
        assert rule['opt'] == 'radam', rule
        new_state = dict(state or {})
        t = new_state.get('step', 1)
        new_x = rp.radam_step(man, x, grad, new_state, lr=rule['lr'], betas=rule['betas'], nc=bool(rule.get('nc', False)),
                              max_grad_norm=clip, exact=move)
        with torch.no_grad():
            beta1, beta2 = rule['betas']
            if rule.get('nc', False):
                beta2 = 1 - 1 / t
            m0 = (state or {}).get('exp_avg', torch.zeros_like(x))
            m = m0 * beta1 + (1 - beta1) * gc
            alpha = rule['lr'] * (1 - beta2**t)**0.5 / (1 - beta1**t)
            tangent = alpha * m / (new_state['exp_avg_sq'].sqrt() + rp.EPS)
    with torch.no_grad():
        diag = dict(rgrad_norm=gn.reshape(-1).double().numpy(), binds=binds.reshape(-1).numpy(),
                    step_norm=man.norm(x, tangent, keepdim=True).reshape(-1).double().numpy())
    return new_x, new_state, diag


def _state_out(state):
    return {k: (v if k == 'step' else v.double().numpy()) for k, v in state.items()}


def _update_all(mans, xs, scales, grads, sgrads, point_rule, scale_rule, point_states, scale_states, dtype):
    k = len(mans)
    point_states = point_states or [{}] * k
    scale_states = scale_states or [{}] * k
    out = dict(new_xs=[], new_scales=[], point_states=[], scale_states=[], diag=[], scale_diag=[])
    for man, x, g, st in zip(mans, xs, grads, point_states):
        xt = _t(x, dtype)
        nx, ns, dg = apply_rule(man, xt, _t(g, dtype), point_rule, _state_in(st, xt.shape, dtype))
        out['new_xs'].append(nx.double().numpy())
        out['point_states'].append(_state_out(ns))
        out['diag'].append(dg)
    for s, g, st in zip(scales, sgrads, scale_states):
        st_ = _t(s, dtype).reshape(1, 1)
        ns, nst, dg = apply_rule(FLAT, st_, _t(g, dtype).reshape(1, 1), scale_rule, _state_in(st, (1, 1), dtype))
        out['new_scales'].append(float(ns.reshape(())))
        out['scale_states'].append({k_: (v if k_ == 'step' else v.reshape(())) for k_, v in _state_out(nst).items()})
        out['scale_diag'].append(dg)
    return out


def train_step(factors, xs, scales, loss, point_rule, scale_rule, *, target=None, dense=None, idx=None,
               point_states=None, scale_states=None, obj=None):
    """One step in fp64.  Returns a dict: `loss` (before the update), `grads` / `scale_grads` (Euclidean), `new_xs`,
    `new_scales`, `point_states`, `scale_states`, `diag` / `scale_diag` (per parameter, see `apply_rule`).
    `obj`: the result of `objective` on the same inputs, when the caller has it already (it is the expensive part)."""
    scales = [float(s) for s in scales]
    value, grads, sgrads = obj if obj is not None else objective(factors, xs, scales, loss, target=target, dense=dense, idx=idx)
    mans = [manifold(f) for f in factors]
    out = _update_all(mans, xs, scales, grads, sgrads, point_rule, scale_rule, point_states, scale_states, torch.float64)
    out.update(loss=value, grads=grads, scale_grads=sgrads)
    return out


def port_step(factors, xs, scales, loss, point_rule, scale_rule, *, target=None, dense=None, idx=None,
              point_states=None, scale_states=None, dtype=torch.float32):
    """The same step in the reference port's own arithmetic at `dtype`: autograd through `ref_port.compute_dists` and the
    port's losses (closed-form 2x2 / 3x3 eigenvalues included), then the same rules on the port's manifolds."""
    mans = [manifold(f, closed_forms=True) for f in factors]
    n = np.asarray(xs[0]).shape[0]
    i, j = pair_list(n, idx)
    gd = _t(pair_targets(target, dense, i, j), dtype)
    xr = [_t(x, dtype).requires_grad_() for x in xs]
    sr = [torch.tensor(float(s), dtype=dtype, requires_grad=True) for s in scales]
    ii = None if idx is None else torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    md = rp.compute_dists(mans, xr, sr, ii)
    if loss['kind'] == 'stress':
        value = rp.stress_loss(gd, md)
    else:
        value = rp.quotient_loss(gd, md, epoch=loss['epoch'], alpha=float(loss.get('alpha', 1.0)),
                                 inc_l1=loss.get('inc_l1', True), inc_l2=loss.get('inc_l2', True))
    if md.numel():
        gs = torch.autograd.grad(value, xr + sr)
    else:
        gs = [torch.zeros_like(p) for p in xr + sr]
    k = len(mans)
    grads = [rp.sym(g) if f[0] == 'spd' else g for f, g in zip(factors, gs[:k])]
    grads = [g.detach().double().numpy() for g in grads]
    sgrads = [float(g) for g in gs[k:]]
    out = _update_all(mans, [x.detach() for x in xr], [float(s.detach()) for s in sr], [g.detach() for g in gs[:k]], [g.detach() for g in gs[k:]],
                      point_rule, scale_rule, point_states, scale_states, dtype)
    out.update(loss=float(value.detach()), grads=grads, scale_grads=sgrads)
    return out
