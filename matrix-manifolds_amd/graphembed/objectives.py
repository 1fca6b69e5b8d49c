"""Losses on vectors of *squared* distances used by the path's configs —
counterparts of graphembed/graphembed/objectives.py:16-45 (Stress, Quotient).
PearsonRLoss runs on the differentiable pdist path.  StochasticNeighborLoss is the reference's
KLDiveregenceLoss('sne', inclusive) (objectives.py:48-76) on the kernels of csrc/sne_loss.hip, StochasticTreeLoss its
spanning-tree model ('sste') on the kernels of csrc/sst_loss.hip; the curvature regulariser (graph sampling) is outside
the accelerated path."""
import abc
import math

import torch
from torch.autograd.function import once_differentiable


class ObjectiveFunction:

    @abc.abstractmethod
    def __call__(self, gdists, mdists, *, epoch, alpha):
        pass


class QuotientLoss(ObjectiveFunction):
    """|m/(a g) - 1| (+ |a g/(m + 1/(epoch+1)) - 1|), summed (objectives.py:16-36)."""

    def __init__(self, inc_l1=True, inc_l2=True):
        if not inc_l1 and not inc_l2:
            raise ValueError('At least one of the terms must be included.')
        self.inc_l1 = inc_l1
        self.inc_l2 = inc_l2

    def __call__(self, gdists, mdists, *, epoch, alpha):
        gdists = gdists * alpha
        loss = 0
        if self.inc_l1:
            loss = loss + (mdists / gdists - 1.0).abs().sum()
        if self.inc_l2:
            loss = loss + (gdists / (mdists + 1.0 / (epoch + 1)) - 1.0).abs().sum()
        return loss

    _dyn = None
    _dyn_host = None     # pinned staging buffer of the device copy
    _dyn_value = None    # (alpha, eps) last written to the device copy

    def on_device(self, device):
        """Keep {alpha, eps = 1/(epoch+1)} in device memory from now on: the fused kernels then read them
        there, so a captured HIP graph of a training step (graphembed.graphed) follows the loss's per-epoch
        schedule — call `set_epoch(epoch, alpha)` before each replay — instead of being re-recorded.
        Returns the fp64 tensor [alpha, eps]."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._dyn is None or self._dyn.device != device:
            self._dyn = torch.tensor([1.0, 1.0], dtype=torch.float64, device=device)
            self._dyn_host = torch.empty(2, dtype=torch.float64,
                                         pin_memory=device.type == 'cuda' and torch.cuda.is_available())
            self._dyn_value = (1.0, 1.0)
        return self._dyn

    def set_epoch(self, epoch, alpha, force=False):
        """Writes the schedule of `epoch` into the device-resident parameters (after `on_device`): nothing
        when the values are the ones already there, else an asynchronous copy from a pinned staging buffer
        on the CURRENT stream (the staging buffer is rewritten only after the previous copy has been consumed).
        Stream order makes the new values visible to kernels launched later on that stream; a consumer on
        ANOTHER stream (a graph replayed from a side stream) must wait for the copy — `fused_spec` does so
        for the calling stream, and `wait_schedule()` does it explicitly.  `force=True` rewrites the device
        copy even if the host believes it is current (after the tensor was restored / overwritten externally)."""
        value = (float(alpha), 1.0 / (epoch + 1))
        if value == self._dyn_value and not force:
            return
        if self._dyn.is_cuda:
            if getattr(self, '_dyn_event', None) is not None:
                self._dyn_event.synchronize()   # the previous copy has left the staging buffer (rarely waits)
            self._dyn_host[0], self._dyn_host[1] = value
            self._dyn.copy_(self._dyn_host, non_blocking=True)
            self._dyn_event = torch.cuda.Event()
            self._dyn_event.record()
            self._dyn_stream = torch.cuda.current_stream(self._dyn.device).cuda_stream
        else:
            self._dyn[0], self._dyn[1] = value
        self._dyn_value = value

    def wait_schedule(self):
        """Makes the current stream wait for the last `set_epoch` copy if that was issued on another stream."""
        ev = getattr(self, '_dyn_event', None)
        if ev is None or self._dyn is None or not self._dyn.is_cuda:
            return
        cur = torch.cuda.current_stream(self._dyn.device)
        if cur.cuda_stream != getattr(self, '_dyn_stream', None) and not ev.query():
            cur.wait_event(ev)

    def fused_spec(self, *, epoch, alpha):
        """(kind, alpha, eps, terms[, device {alpha, eps}]) for the fused loss+gradient kernels
        (mm_*_pdist_loss).  After `on_device` the values of this call are also written to the device
        copy — except while a graph is being recorded, where the device copy is what counts."""
        eps = 1.0 / (epoch + 1)
        terms = int(self.inc_l1) | (int(self.inc_l2) << 1)
        if self._dyn is None:
            return ('quotient', float(alpha), eps, terms)
        if not (self._dyn.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.set_epoch(epoch, alpha)
            self.wait_schedule()
        return ('quotient', float(alpha), eps, terms, self._dyn)

    def __str__(self):
        return 'quotient_loss'


class StressLoss(ObjectiveFunction):
    """sum (m - g)^2 (objectives.py:39-45)."""

    def __call__(self, gdists, mdists, *, epoch=None, alpha=None):
        return torch.pow(mdists - gdists, 2).sum()

    def fused_spec(self, *, epoch=None, alpha=None):
        return ('stress', 1.0, 0.0, 0)

    def __str__(self):
        return 'stress_loss'


class PearsonRLoss(ObjectiveFunction):
    """Negative Pearson correlation of the two pair vectors (objectives.py:109-117).  No fused kernel: it
    runs on the differentiable pdist path (`compute_dists`)."""

    def __call__(self, x, y, **kwargs):
        dx, dy = x - x.mean(), y - y.mean()
        return -(dx * dy).sum() / (dx.norm() * dy.norm())

    def __str__(self):
        return 'pearson_r_loss'


def _nodes_of(npairs):
    """n with n (n - 1) / 2 == npairs (1 for an empty pair vector)."""
    n = (1 + math.isqrt(1 + 8 * npairs)) // 2
    if n * (n - 1) // 2 != npairs:
        raise ValueError(f'a pair vector has n (n - 1) / 2 entries; {npairs} is not such a number')
    return n


class _SneKL(torch.autograd.Function):
    """Loss and d loss / d mdists from one C-ABI call (mm_sne_kl_loss): statistics, merge and — only when `mdists`
    requires a gradient — the gradient pass."""

    @staticmethod
    def forward(ctx, gdists, mdists, mode, alpha):
        from graphembed import _backend as B
        B.require_gpu(gdists, mdists)
        lib = B.lib()
        n = _nodes_of(mdists.numel())
        m = mdists.detach().contiguous()
        g = gdists.detach().to(dtype=m.dtype, device=m.device).contiguous()
        if g.numel() != m.numel():
            raise ValueError(f'target has {g.numel()} entries, the pair vector has {m.numel()}')
        dt = B.dtype_code(m)
        with B.on_device(m.device):
            grad = torch.empty_like(m) if ctx.needs_input_grad[1] else None
            out = torch.empty(1, dtype=m.dtype, device=m.device)
            ws = torch.empty(lib.raw('mm_sne_kl_ws_bytes')(dt, n), dtype=torch.uint8, device=m.device)
            lib.call('mm_sne_kl_loss', dt, mode, B.ptr(g), B.ptr(m), n, float(alpha), B.ptr(grad), B.ptr(out), B.ptr(ws),
                     B.stream_of(m))
        ctx.grad = None if grad is None else grad.view(mdists.shape)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, up):
        from graphembed import _backend as B
        return (None, B.take_grads(ctx, up, 'grad')[0], None, None)


class StochasticNeighborLoss(ObjectiveFunction):
    """sum_i KL(P_i(theta_x) || P_i(theta_z)) of the stochastic-neighbour model P_ij(theta) = exp(theta_ij) / sum_k exp(theta_ik)
    over pair vectors — inclusive: theta_x = -alpha g, theta_z = -m; exclusive: swapped (objectives.py:48-76 with
    inference/stochastic_neighbors.py:8-24).  `alpha` is a plain float and has no gradient.

    GPU tensors go through the kernels of csrc/sne_loss.hip (no n x n array, bitwise reproducible); CPU tensors, or
    `native=False`, evaluate the same loss with torch ops on a dense [n, n] theta — differentiable by autograd.  There is no
    `fused_spec`: BatchedObjective feeds it `compute_dists`, so it serves every manifold, product and node minibatch.  A node's
    partition function needs its whole row, so the row-sharded evaluation of graphembed.parallel is not offered."""

    def __init__(self, inclusive=True, native=True):
        self.inclusive = inclusive
        self.native = native

    def __call__(self, gdists, mdists, *, epoch=None, alpha):
        n = _nodes_of(mdists.numel())
        if gdists.numel() != mdists.numel():
            raise ValueError(f'target has {gdists.numel()} entries, the pair vector has {mdists.numel()}')
        if self.native and mdists.is_cuda:
            from graphembed import _backend as B
            return _SneKL.apply(gdists, mdists, B.SNE_INCLUSIVE if self.inclusive else B.SNE_EXCLUSIVE, float(alpha))
        return self._torch_ops(gdists, mdists, n, alpha)

    def _torch_ops(self, gdists, mdists, n, alpha):
        if n < 2:
            return mdists.sum() * 0
        theta_x, theta_z = -alpha * gdists.to(mdists.dtype), -mdists
        if not self.inclusive:
            theta_x, theta_z = theta_z, theta_x
        iu = torch.triu_indices(n, n, 1, device=mdists.device)

        def dense(theta, diagonal):
            full = theta.new_full((n, n), diagonal)
            return full.index_put((torch.cat([iu[0], iu[1]]), torch.cat([iu[1], iu[0]])), torch.cat([theta, theta]))

        def log_partition(full):
            # logsumexp of the rows, each shifted by its own (constant) maximum first: its backward, exp(theta - result), then
            # equals the softmax below to an ulp of 1 instead of an ulp of |theta| — the two cancel in d loss / d theta_x
            shift = full.detach().max(dim=1, keepdim=True).values
            return (shift[:, 0] + torch.logsumexp(full - shift, dim=1)).sum()

        dx, dz = dense(theta_x, -math.inf), dense(theta_z, -math.inf)
        p = torch.softmax(dx, dim=1)
        # sum_j P_ij delta_ij as sum_j P_ij (delta_ij - c_i) + c_i with the constant c_i = mu_i (the rows of P sum to 1): the
        # softmax backward then forms P (delta - mu) from small numbers, not as the difference of two sums of size |delta|
        delta = dense(theta_z - theta_x, 0.0)
        mu = (p * delta).sum(dim=1, keepdim=True).detach()
        return log_partition(dz) - log_partition(dx) - (p * (delta - mu)).sum() - mu.sum()

    def __str__(self):
        return 'kl_loss'


class _SstKL(torch.autograd.Function):
    """Loss and d loss / d mdists from one C-ABI call (mm_sst_kl_loss); the gradient buffer — and with it the inverse of the
    theta_z model or the G M G products — is asked for only when `mdists` requires a gradient."""

    @staticmethod
    def forward(ctx, gdists, mdists, mode, alpha):
        from graphembed import _backend as B
        B.require_gpu(gdists, mdists)
        lib = B.lib()
        n = _nodes_of(mdists.numel())
        m = mdists.detach().contiguous()
        g = gdists.detach().to(dtype=m.dtype, device=m.device).contiguous()
        if g.numel() != m.numel():
            raise ValueError(f'target has {g.numel()} entries, the pair vector has {m.numel()}')
        dt = B.dtype_code(m)
        with B.on_device(m.device):
            grad = torch.empty_like(m) if ctx.needs_input_grad[1] else None
            out = torch.empty(1, dtype=m.dtype, device=m.device)
            ws = torch.empty(lib.raw('mm_sst_kl_ws_bytes')(dt, n), dtype=torch.uint8, device=m.device)
            lib.call('mm_sst_kl_loss', dt, mode, B.ptr(g), B.ptr(m), n, float(alpha), B.ptr(grad), B.ptr(out), B.ptr(ws),
                     B.stream_of(m))
        ctx.grad = None if grad is None else grad.view(mdists.shape)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, up):
        from graphembed import _backend as B
        return (None, B.take_grads(ctx, up, 'grad')[0], None, None)


class _SstTorchOps(torch.autograd.Function):
    """The closed forms of StochasticTreeLoss with torch ops: loss in forward, the chosen gradient convention in backward
    (a custom Function, so the route does not depend on what autograd makes of an inverse held outside the graph)."""

    @staticmethod
    def forward(ctx, gdists, mdists, n, alpha, inclusive, exact):
        m = mdists.detach()
        a, b = -alpha * gdists.detach().to(m.dtype), -m
        tx, tz = (a, b) if inclusive else (b, a)
        iu = torch.triu_indices(n, n, 1, device=m.device)
        cx, cz = tx.max(), tz.max()

        def dense(v):
            full = v.new_zeros((n, n))
            return full.index_put((torch.cat([iu[0], iu[1]]), torch.cat([iu[1], iu[0]])), torch.cat([v, v]))

        def laplacian(w):
            off = dense(w)
            return (torch.diag(off.sum(dim=1)) - off)[1:, 1:]

        def quad(S):   # q(S) per pair, S extended by a zero row and column for node 0
            full = S.new_zeros((n, n))
            full[1:, 1:] = S
            d = torch.diagonal(full)
            return d[iu[0]] + d[iu[1]] - 2 * full[iu[0], iu[1]]

        def model(w, inverse):
            """(sum of log pivots x 2, L^-1 or None); a factorisation that fails gives NaN, as the kernels do"""
            C, info = torch.linalg.cholesky_ex(laplacian(w))
            C = torch.where(info == 0, C, C.new_full((), math.nan))   # (no host read: the route stays asynchronous)
            return 2 * torch.log(torch.diagonal(C)).sum(), (torch.cholesky_inverse(C) if inverse else None)

        # shifted weights: exp(theta - max theta); the shifts of A and of mu . delta cancel because sum mu = n - 1
        wx, wz = torch.exp(tx - cx), torch.exp(tz - cz)
        delta = (tz - cz) - (tx - cx)
        need = ctx.needs_input_grad[1]
        ax, Gx = model(wx, True)
        az, Gz = model(wz, need and inclusive)
        mu = wx * quad(Gx)
        loss = (az - ax) - (mu * delta).sum()
        if need:
            if inclusive:
                grad = mu - wz * quad(Gz)
            elif exact:
                grad = mu * delta - wx * quad(Gx @ laplacian(wx * delta) @ Gx)
            else:
                grad = mu * (tz - tx)
            ctx.grad = grad.view(mdists.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, up):
        return (None, up * ctx.grad, None, None, None, None)


class StochasticTreeLoss(ObjectiveFunction):
    """KL(trees(theta_x) || trees(theta_z)) of the random-spanning-tree model over pair vectors — the reference's
    KLDiveregenceLoss('sste', inclusive) (objectives.py:48-76 with inference/stochastic_trees.py): with w = exp theta, L the
    weighted graph Laplacian without node 0, G = L^-1 and mu_ij = w_ij (G_ii + G_jj - 2 G_ij) the edge marginals,
        loss = log det L(theta_z) - log det L(theta_x) - mu(theta_x) . (theta_z - theta_x),
    inclusive: theta_x = -alpha g, theta_z = -m; exclusive: swapped.  `alpha` is a plain float and has no gradient.

    `exact_gradient` matters for the exclusive loss only.  The reference's backward drops d G / d theta there and returns
    mu (theta_z - theta_x) per pair, which is not the gradient of its loss; False (the default) reproduces that, True gives the
    gradient of the loss as stated, mu delta - w q(G M G).  Loss, inclusive gradient and exact exclusive gradient do not change
    when a constant is added to every m; the reference-form gradient does by its definition.

    GPU tensors go through the kernels of csrc/sst_loss.hip (blocked Cholesky and matrix-core products, bitwise reproducible,
    at most 4096 nodes); CPU tensors, or `native=False`, evaluate the same closed forms with torch ops on dense Laplacians.
    There is no `fused_spec`: BatchedObjective feeds it `compute_dists`, so it serves every manifold, product and node
    minibatch.  The determinant couples every pair, so the row-sharded evaluation of graphembed.parallel is not offered."""

    def __init__(self, inclusive=True, native=True, exact_gradient=False):
        self.inclusive = inclusive
        self.native = native
        self.exact_gradient = exact_gradient

    def __call__(self, gdists, mdists, *, epoch=None, alpha):
        n = _nodes_of(mdists.numel())
        if gdists.numel() != mdists.numel():
            raise ValueError(f'target has {gdists.numel()} entries, the pair vector has {mdists.numel()}')
        if self.native and mdists.is_cuda:
            from graphembed import _backend as B
            mode = (B.SST_INCLUSIVE if self.inclusive else B.SST_EXCLUSIVE if self.exact_gradient
                    else B.SST_EXCLUSIVE_REFERENCE)
            return _SstKL.apply(gdists, mdists, mode, float(alpha))
        if n < 2:
            return mdists.sum() * 0
        return _SstTorchOps.apply(gdists, mdists, n, float(alpha), bool(self.inclusive), bool(self.exact_gradient))

    def __str__(self):
        return 'kl_loss'


class Sum(ObjectiveFunction):

    def __init__(self, *fns):
        self.fns = fns

    def __call__(self, *args, **kwargs):
        return sum(fn(*args, **kwargs) for fn in self.fns)

    def __str__(self):
        return '__'.join(str(f) for f in self.fns)
