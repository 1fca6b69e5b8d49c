"""The special orthogonal group SO(n), n <= 4, on the gfx950 kernels of csrc/so.hip — the counterpart of the reference's
SpecialOrthogonalGroup (graphembed/graphembed/manifolds/orthogonal.py:8-44), whose `dist` is a Python loop of `Tensor.eig()`
(no derivative), whose `log` is a loop of scipy.linalg.logm on the CPU and which has no `exp`.

`SpecialOrthogonal(n)` is St(n, n) with a metric: proju, projx, the retractions, rand, randvec and the three fused optimizer
steps are inherited from `Stiefel`; `dist`, `pdist`, the fused objective `pdist_loss`, `log` and `exp` are new, and so are the
node-minibatch forms `pdist_subset` / `pdist_loss_subset` (csrc/so.hip with SUB: the index vector inside the pair kernels).  The distance is
the ambient function d2(x, y) = sum_k 4 asin^2(sigma_k(y - x) / 2) (csrc/so_pair.hpp), equal to ||log(x^T y)||_F^2 on SO(n).
The reference's connected-component check in `dist` would synchronise and is not made; at the cut locus the distance is finite
and the gradient (undefined there) is finite.

(The module and the class carry names of their own: this package binds neither `OrthogonalGroup` nor `SpecialOrthogonalGroup`,
so that under the overlay those names resolve to the checkout; `SpecialOrthogonal.from_reference(obj)` adopts such an instance.)"""
import torch

from graphembed import _backend as B
from graphembed.manifolds.grassmann import Stiefel


class _SoPdist(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, N, squared, row_begin, row_end):
        B.require_gpu(x)
        xc = x.detach().contiguous()
        n = xc.shape[0]
        npairs = B.pair_offset(n, row_end) - B.pair_offset(n, row_begin)
        ctx.save_for_backward(xc)
        ctx.args = (N, squared, row_begin, row_end)
        ctx.empty = npairs == 0
        if ctx.empty:
            return xc.new_empty(0)
        with B.on_device(xc.device):
            out = torch.empty(npairs, dtype=xc.dtype, device=xc.device)
            B.lib().call('mm_so_pdist_fwd', B.dtype_code(xc), B.ptr(xc), n, N, row_begin, row_end, int(squared), B.ptr(out),
                         B.stream_of(xc))
        return out

    @staticmethod
    def backward(ctx, g):
        xc, = ctx.saved_tensors
        N, squared, row_begin, row_end = ctx.args
        if ctx.empty:
            return (torch.zeros_like(xc), ) + (None, ) * 4
        lib = B.lib()
        g = g.contiguous()
        n = xc.shape[0]
        dt = B.dtype_code(xc)
        with B.on_device(xc.device):
            ws = torch.empty(lib.raw('mm_so_pdist_ws_bytes')(dt, n, N), dtype=torch.uint8, device=xc.device)
            grad = torch.empty_like(xc)
            lib.call('mm_so_pdist_bwd', dt, B.ptr(xc), B.ptr(g), n, N, row_begin, row_end, int(squared), B.ptr(grad),
                     B.ptr(ws), B.stream_of(xc))
        return grad, None, None, None, None


class _SoDist(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, y, N, squared):
        B.require_gpu(x, y)
        if x.dtype != y.dtype or x.device != y.device:   # (both pointers go to the kernel under x's dtype code)
            raise TypeError(f'dist needs both points in one dtype on one device, got {x.dtype} on {x.device} and {y.dtype} on {y.device}')
        xc = x.detach().reshape(-1, N, N).contiguous()
        yc = y.detach().reshape(-1, N, N).contiguous()
        with B.on_device(xc.device):
            out = torch.empty(xc.shape[0], dtype=xc.dtype, device=xc.device)
            B.lib().call('mm_so_dist', B.dtype_code(xc), B.ptr(xc), B.ptr(yc), None, xc.shape[0], N, int(squared), B.ptr(out),
                         None, None, B.stream_of(xc))
        ctx.save_for_backward(xc, yc)
        ctx.args = (N, squared, x.shape, y.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, yc = ctx.saved_tensors
        N, squared, xs, ys = ctx.args
        g = g.reshape(-1).contiguous()
        with B.on_device(xc.device):
            gx, gy = torch.empty_like(xc), torch.empty_like(yc)
            B.lib().call('mm_so_dist', B.dtype_code(xc), B.ptr(xc), B.ptr(yc), B.ptr(g), xc.shape[0], N, int(squared), None,
                         B.ptr(gx), B.ptr(gy), B.stream_of(xc))
        return gx.reshape(xs), gy.reshape(ys), None, None


class _SoPdistLoss(torch.autograd.Function):
    """loss(target, softplus(scale) * pdist(x)^2) with both gradients from one pass over the pairs (mm_so_pdist_loss) — see
    graphembed.manifolds.grassmann._GrassPdistLoss."""

    @staticmethod
    def forward(ctx, x, scale, target, N, spec, row_begin, row_end):
        B.require_gpu(x, target)
        lib = B.lib()
        xc = x.detach().contiguous()
        n = xc.shape[0]
        dt = B.dtype_code(xc)
        lkind, alpha, eps, terms = spec[:4]
        dyn = spec[4] if len(spec) > 4 else None  # device {alpha, eps} (QuotientLoss.on_device)
        tc = target.detach().to(xc.dtype).contiguous()
        npairs = B.pair_offset(n, row_end) - B.pair_offset(n, row_begin)
        if tc.numel() != npairs:
            raise ValueError(f'target has {tc.numel()} entries, the pair range has {npairs}')
        sc = None if scale is None else scale.detach().to(xc.dtype).reshape(1).contiguous()
        with B.on_device(xc.device):
            ws = torch.empty(lib.raw('mm_so_pdist_loss_ws_bytes')(dt, n, N), dtype=torch.uint8, device=xc.device)
            out = torch.empty(2, dtype=xc.dtype, device=xc.device)
            grad = torch.empty_like(xc)
            lib.call('mm_so_pdist_loss', dt, B.LOSS_STRESS if lkind == 'stress' else B.LOSS_QUOTIENT, B.ptr(xc), B.ptr(tc),
                     B.ptr(sc), n, N, row_begin, row_end, alpha, eps, terms, B.dyn_ptr(dyn, xc), B.ptr(out), B.ptr(grad),
                     B.ptr(ws), B.stream_of(xc))
        ctx.grad_x = grad.reshape(x.shape)
        ctx.grad_s = None if scale is None else out[1].reshape(scale.shape).to(scale.dtype)
        return out[0]

    @staticmethod
    def backward(ctx, up):
        gx, gs = B.take_grads(ctx, up, 'grad_x', 'grad_s')
        return gx, gs, None, None, None, None, None


def _subset_ws(cache, tag, sizer, x, N):
    """The workspace of a node-minibatch call: sized by the table and kept in `cache` for the embedding's lifetime (a captured
    graph of the step refers to it); every call clears it itself."""
    key = (tag, x.dtype, x.device, x.shape[0], N)
    ws = cache.get(key) if cache is not None else None
    if ws is None:
        ws = torch.empty(B.lib().raw(sizer)(B.dtype_code(x), x.shape[0], N), dtype=torch.uint8, device=x.device)
        if cache is not None:
            cache[key] = ws
    return ws


class _SoSubsetLoss(torch.autograd.Function):
    """Objective and gradients of a node minibatch inside the SO(n) pair kernel (mm_so_pdist_loss_subset): the index vector
    addresses the rows of the full table, the targets dense[idx[a]][idx[b]] and the gradient rows — no gather, no scatter-add,
    no zero fill (the sibling of graphembed.manifolds.grassmann._GrassSubsetLoss)."""

    @staticmethod
    def forward(ctx, spec, rows, N, cache, idx, dense, x, scale):
        B.require_gpu(x, dense)
        lkind, alpha, eps, terms = spec[:4]
        dyn = spec[4] if len(spec) > 4 else None
        dtype, dev = x.dtype, x.device
        n_total, bs = x.shape[0], idx.numel()
        rb, re = (0, bs) if rows is None else rows
        if dense.dtype != dtype or not dense.is_contiguous() or dense.shape != (n_total, n_total):
            raise ValueError('dense targets must be a contiguous [n, n] matrix of the embedding\'s dtype')
        with B.on_device(dev):
            xc = x.detach().contiguous()
            sc = scale.detach().to(dtype).reshape(1).contiguous()
            ic = idx.to(device=dev, dtype=torch.int64).contiguous()
            out = torch.empty(2, dtype=dtype, device=dev)
            grad = torch.empty_like(xc)
            ws = _subset_ws(cache, 'so loss', 'mm_so_pdist_loss_ws_bytes', xc, N)
            B.lib().call('mm_so_pdist_loss_subset', B.dtype_code(xc), B.LOSS_STRESS if lkind == 'stress' else B.LOSS_QUOTIENT,
                         B.ptr(xc), B.ptr(dense), B.ptr(sc), n_total, N, B.ptr(ic), bs, rb, re, alpha, eps, terms,
                         B.dyn_ptr(dyn, x), B.ptr(out), B.ptr(grad), B.ptr(ws), B.stream_of(x))
        ctx.grads = [grad.reshape(x.shape), out[1].reshape(scale.shape).to(scale.dtype)]
        return out[0]

    @staticmethod
    def backward(ctx, up):
        return (None, None, None, None, None, None) + tuple(B.take_grads(ctx, up, 'grads'))


class _SoSubsetPdist(torch.autograd.Function):
    """The pair vector of a node minibatch of the full table (mm_so_pdist_fwd_subset) and its full-size gradient
    (mm_so_pdist_bwd_subset): rows outside the batch get +0, repeated nodes accumulate."""

    @staticmethod
    def forward(ctx, x, idx, N, squared, rows, cache):
        B.require_gpu(x)
        xc = x.detach().contiguous()
        bs = idx.numel()
        rb, re = (0, bs) if rows is None else rows
        npairs = B.pair_offset(bs, re) - B.pair_offset(bs, rb) if bs >= 2 else 0
        with B.on_device(xc.device):
            ic = idx.to(device=xc.device, dtype=torch.int64).contiguous()
            out = torch.empty(npairs, dtype=xc.dtype, device=xc.device)
            if npairs:
                B.lib().call('mm_so_pdist_fwd_subset', B.dtype_code(xc), B.ptr(xc), xc.shape[0], N, B.ptr(ic), bs, rb, re,
                             int(squared), B.ptr(out), B.stream_of(xc))
        ctx.save_for_backward(xc, ic)
        ctx.args = (N, squared, rb, re, cache, npairs)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, ic = ctx.saved_tensors
        N, squared, rb, re, cache, npairs = ctx.args
        if not npairs:
            return (torch.zeros_like(xc), ) + (None, ) * 5
        g = g.contiguous()
        with B.on_device(xc.device):
            ws = _subset_ws(cache, 'so pdist', 'mm_so_pdist_ws_bytes', xc, N)
            grad = torch.empty_like(xc)
            B.lib().call('mm_so_pdist_bwd_subset', B.dtype_code(xc), B.ptr(xc), B.ptr(g), xc.shape[0], N, B.ptr(ic), ic.numel(),
                         rb, re, int(squared), B.ptr(grad), B.ptr(ws), B.stream_of(xc))
        return grad, None, None, None, None, None


class SpecialOrthogonal(Stiefel):

    def __init__(self, n, retr='svd'):
        super().__init__(n, n, retr)

    @classmethod
    def from_reference(cls, man):
        """A SpecialOrthogonal with the state of `man`: any object with `n` and, optionally, the bound retraction `retr` of
        the checkout's Stiefel family (`retr_qr` / `retr_svd`) — its `SpecialOrthogonalGroup` instance, for one."""
        name = getattr(getattr(man, 'retr', None), '__name__', '')
        return cls(int(man.n), retr='qr' if 'qr' in name else 'svd')

    @property
    def dim(self):
        return self.n * (self.n - 1) // 2

    def _pointwise(self, op, x, u):
        B.require_gpu(x, u)
        if x.dtype != u.dtype or x.device != u.device:
            raise TypeError(f'exp / log need both arguments in one dtype on one device, got {x.dtype} on {x.device} and {u.dtype} on {u.device}')
        if torch.is_grad_enabled() and (x.requires_grad or u.requires_grad):
            raise NotImplementedError('exp / log run under torch.no_grad on the HIP path; only dist/pdist are differentiable')
        shape = torch.broadcast_shapes(x.shape, u.shape)
        xc = x.expand(shape).reshape(-1, self.n, self.n).contiguous()
        uc = u.expand(shape).reshape(-1, self.n, self.n).contiguous()
        with B.on_device(xc.device):
            out = torch.empty_like(xc)
            B.lib().call('mm_so_map', B.dtype_code(xc), op, B.ptr(xc), B.ptr(uc), xc.shape[0], self.n, B.ptr(out),
                         B.stream_of(xc))
        return out.reshape(shape)

    def exp(self, x, u):  # (the reference has none: stiefel.py:59-60)
        return self._pointwise(B.SO_EXP, x, u)

    def log(self, x, y):  # orthogonal.py:26-37
        return self._pointwise(B.SO_LOG, x, y)

    def transp(self, x, y, u):  # base.py:65-66
        return self.proju(y, u)

    def dist(self, x, y, squared=False, keepdim=False):  # orthogonal.py:13-21, without the component check
        shape = torch.broadcast_shapes(x.shape, y.shape)
        d = _SoDist.apply(x.expand(shape), y.expand(shape), self.n, squared).reshape(shape[:-2])
        return d.reshape(*d.shape, 1, 1) if keepdim else d

    def pdist(self, x, squared=False, rows=None):  # base.py:59-63
        assert x.ndim == 3
        rb, re = (0, x.shape[0]) if rows is None else rows
        return _SoPdist.apply(x, self.n, squared, rb, re)

    def pdist_loss(self, x, scale, target, spec, rows=None):
        """Fused `objective(target, softplus(scale) * pdist(x, squared=True))` with its gradients in one pass; `spec` comes
        from `objective_fn.fused_spec(epoch=, alpha=)`."""
        assert x.ndim == 3
        rb, re = (0, x.shape[0]) if rows is None else rows
        return _SoPdistLoss.apply(x, scale, target, self.n, spec, rb, re)

    def subset_form(self, x):
        """Can the node-minibatch kernels (csrc/so.hip, SUB) take the table `x`?  (GPU, fp32 / fp64, [n, N, N], N <= 4.)"""
        return bool(x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.ndim == 3 and x.shape[0] >= 1
                    and tuple(x.shape[-2:]) == (self.n, self.n) and 2 <= self.n <= B.lib().raw('mm_so_max_dim')())

    def pdist_loss_subset(self, x, scale, idx, dense, spec, rows=None, cache=None):
        """`pdist_loss` for the node minibatch `idx` (distinct nodes) of the full table `x` with the targets
        dense[idx[a], idx[b]], inside the pair kernel; None when the tensors are not eligible (the caller then gathers)."""
        if not (self.subset_form(x) and dense.is_cuda):
            return None
        return _SoSubsetLoss.apply(spec, rows, self.n, cache, idx, dense, x, scale)

    def pdist_subset(self, x, idx, squared=False, rows=None, cache=None):
        """`pdist(x[idx], squared, rows)` without the gather: the pair vector of the batch from the full table, and in the
        backward a full-size gradient (rows outside the batch +0).  Repeated nodes are allowed: their gradients accumulate and
        the pair of a node with itself is 0 with a zero gradient.  None when the tensors are not eligible."""
        if not self.subset_form(x):
            return None
        return _SoSubsetPdist.apply(x, idx, self.n, squared, rows, cache)

    def rand_uniform(self, *shape, out=None):  # orthogonal.py:39-44: the first column times the determinant
        xs = super().rand_uniform(*shape, out=out)
        xs[..., 0].mul_(torch.linalg.det(xs).unsqueeze(-1))
        return xs

    def __str__(self):
        return 'Special orthogonal group of {}x{} matrices'.format(self.n, self.n)
