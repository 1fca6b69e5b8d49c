"""Grassmann Gr(n,p) and Stiefel St(n,p) on the gfx950 kernels of csrc/mat.hip — counterparts
of graphembed/graphembed/manifolds/grassmann.py:10-116 and stiefel.py:7-93 (the reference ships
every QR/SVD of these maps to the CPU, linalg/torch_batch.py:94-121)."""
import torch

from graphembed import _backend as B
from graphembed.manifolds.base import Manifold, _like


class _GrassPdist(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, N, p, squared, row_begin, row_end):
        B.require_gpu(x)
        xc = x.detach().contiguous()
        n = xc.shape[0]
        npairs = B.pair_offset(n, row_end) - B.pair_offset(n, row_begin)
        ctx.save_for_backward(xc)
        ctx.args = (N, p, squared, row_begin, row_end)
        ctx.empty = npairs == 0
        if ctx.empty:
            return xc.new_empty(0)
        with B.on_device(xc.device):
            out = torch.empty(npairs, dtype=xc.dtype, device=xc.device)
            B.lib().call('mm_grass_pdist_fwd', B.dtype_code(xc), B.ptr(xc), n, N, p, row_begin, row_end,
                         int(squared), B.ptr(out), B.stream_of(xc))
        return out

    @staticmethod
    def backward(ctx, g):
        xc, = ctx.saved_tensors
        N, p, squared, row_begin, row_end = ctx.args
        if ctx.empty:
            return (torch.zeros_like(xc), ) + (None, ) * 5
        lib = B.lib()
        g = g.contiguous()
        n = xc.shape[0]
        dt = B.dtype_code(xc)
        with B.on_device(xc.device):
            ws = torch.empty(lib.raw('mm_grass_pdist_ws_bytes')(dt, n, N, p), dtype=torch.uint8, device=xc.device)
            grad = torch.empty_like(xc)
            lib.call('mm_grass_pdist_bwd', dt, B.ptr(xc), B.ptr(g), n, N, p, row_begin, row_end, int(squared),
                     B.ptr(grad), B.ptr(ws), B.stream_of(xc))
        return grad, None, None, None, None, None


class _GrassDist(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, y, N, p, squared):
        B.require_gpu(x, y)
        xc = x.detach().reshape(-1, N, p).contiguous()
        yc = y.detach().reshape(-1, N, p).contiguous()
        with B.on_device(xc.device):
            out = torch.empty(xc.shape[0], dtype=xc.dtype, device=xc.device)
            B.lib().call('mm_grass_dist', B.dtype_code(xc), B.ptr(xc), B.ptr(yc), None, xc.shape[0], N, p,
                         int(squared), B.ptr(out), None, None, B.stream_of(xc))
        ctx.save_for_backward(xc, yc)
        ctx.args = (N, p, squared, x.shape, y.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, yc = ctx.saved_tensors
        N, p, squared, xs, ys = ctx.args
        g = g.reshape(-1).contiguous()
        with B.on_device(xc.device):
            gx, gy = torch.empty_like(xc), torch.empty_like(yc)
            B.lib().call('mm_grass_dist', B.dtype_code(xc), B.ptr(xc), B.ptr(yc), B.ptr(g), xc.shape[0], N, p,
                         int(squared), None, B.ptr(gx), B.ptr(gy), B.stream_of(xc))
        return gx.reshape(xs), gy.reshape(ys), None, None, None


class _GrassPdistLoss(torch.autograd.Function):
    """loss(target, softplus(scale) * pdist(x)^2) with both gradients from one pass over the
    pairs (mm_grass_pdist_loss) — see graphembed.manifolds.vector._VecPdistLoss."""

    @staticmethod
    def forward(ctx, x, scale, target, N, p, spec, row_begin, row_end):
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
            ws = torch.empty(lib.raw('mm_grass_pdist_loss_ws_bytes')(dt, n, N, p), dtype=torch.uint8,
                             device=xc.device)
            out = torch.empty(2, dtype=xc.dtype, device=xc.device)
            grad = torch.empty_like(xc)
            lib.call('mm_grass_pdist_loss', dt, B.LOSS_STRESS if lkind == 'stress' else B.LOSS_QUOTIENT,
                     B.ptr(xc), B.ptr(tc), B.ptr(sc), n, N, p, row_begin, row_end, alpha, eps, terms,
                     B.dyn_ptr(dyn, xc), B.ptr(out), B.ptr(grad), B.ptr(ws), B.stream_of(xc))
        ctx.grad_x = grad.reshape(x.shape)
        ctx.grad_s = None if scale is None else out[1].reshape(scale.shape).to(scale.dtype)
        return out[0]

    @staticmethod
    def backward(ctx, up):
        gx, gs = B.take_grads(ctx, up, 'grad_x', 'grad_s')
        return gx, gs, None, None, None, None, None, None


class _GrassSubsetLoss(torch.autograd.Function):
    """Objective and gradients of a node minibatch inside the Grassmann pair kernel (mm_grass_pdist_loss_subset): the
    index vector addresses the rows of the full table, the targets dense[idx[a]][idx[b]] and the gradient rows — no
    gather, no scatter-add, no zero fill (the sibling of graphembed.modules._SingleSubsetLoss).  The workspace is sized
    by the table and kept in `cache` for the embedding's lifetime: a captured graph of the step refers to it."""

    @staticmethod
    def forward(ctx, spec, rows, N, p, cache, idx, dense, x, scale):
        B.require_gpu(x, dense)
        lib = B.lib()
        lkind, alpha, eps, terms = spec[:4]
        dyn = spec[4] if len(spec) > 4 else None
        dtype, dev = x.dtype, x.device
        n_total, bs = x.shape[0], idx.numel()
        rb, re = (0, bs) if rows is None else rows
        dt = B.dtype_code(x)
        if dense.dtype != dtype or not dense.is_contiguous() or dense.shape != (n_total, n_total):
            raise ValueError('dense targets must be a contiguous [n, n] matrix of the embedding\'s dtype')
        with B.on_device(dev):
            xc = x.detach().contiguous()
            sc = scale.detach().to(dtype).reshape(1).contiguous()
            ic = idx.to(device=dev, dtype=torch.int64).contiguous()
            out = torch.empty(2, dtype=dtype, device=dev)
            grad = torch.empty_like(xc)
            key = ('grass', dtype, dev, n_total, N, p)
            ws = cache.get(key) if cache is not None else None
            if ws is None:
                ws = torch.empty(lib.raw('mm_grass_pdist_loss_ws_bytes')(dt, n_total, N, p), dtype=torch.uint8, device=dev)
                if cache is not None:
                    cache[key] = ws
            lib.call('mm_grass_pdist_loss_subset', dt, B.LOSS_STRESS if lkind == 'stress' else B.LOSS_QUOTIENT, B.ptr(xc),
                     B.ptr(dense), B.ptr(sc), n_total, N, p, B.ptr(ic), bs, rb, re, alpha, eps, terms, B.dyn_ptr(dyn, x),
                     B.ptr(out), B.ptr(grad), B.ptr(ws), B.stream_of(x))
        ctx.grads = [grad.reshape(x.shape), out[1].reshape(scale.shape).to(scale.dtype)]
        return out[0]

    @staticmethod
    def backward(ctx, up):
        return (None, None, None, None, None, None, None) + tuple(B.take_grads(ctx, up, 'grads'))


class _MatrixManifold(Manifold):
    _kind = None

    def __init__(self, n, p, retr='svd'):
        self.n = n
        self.p = p
        if retr == 'qr':
            self.retr = self.retr_qr_
            self._retr_op = B.MAT_RETR_QR
        elif retr == 'svd':
            self.retr = self.retr_svd_
            self._retr_op = B.MAT_RETR_SVD
        else:
            raise ValueError('Unknown retraction type {}'.format(retr))

    @property
    def ndim(self):
        return 2

    def zero(self, *shape, out=None):
        return torch.eye(self.n, self.p, **_like(out)).repeat(*shape, 1, 1)

    def zero_vec(self, *shape, out=None):
        return torch.zeros(*shape, self.n, self.p, **_like(out))

    def inner(self, x, u, v, keepdim=False):
        return (u * v).sum((-2, -1), keepdim=keepdim)

    def _map(self, op, x, u=None):
        B.require_gpu(x, u)
        ts = [t for t in (x, u) if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
            raise NotImplementedError('projections / retractions / exp / log run under torch.no_grad on the '
                                      'HIP path; only dist/pdist are differentiable')
        shape = torch.broadcast_shapes(*[t.shape for t in ts])
        xc = x.expand(shape).reshape(-1, self.n, self.p).contiguous()
        uc = None if u is None else u.expand(shape).reshape(-1, self.n, self.p).contiguous()
        with B.on_device(xc.device):
            out = torch.empty_like(xc)
            B.lib().call('mm_mat_map', B.dtype_code(xc), self._kind, op, B.ptr(xc), B.ptr(uc), xc.shape[0],
                         self.n, self.p, B.ptr(out), B.stream_of(xc))
        return out.reshape(shape)

    def proju(self, x, u, inplace=False):
        new = self._map(B.MAT_PROJU, x, u)
        if not inplace:
            return new
        u.set_(new)
        return u

    def retr_qr_(self, x, u):
        return self._map(B.MAT_RETR_QR, x, u)

    def retr_svd_(self, x, u):
        return self._map(B.MAT_RETR_SVD, x, u)

    def _step_eligible(self, x, egrad, exact, buf=None):
        """Can the fused optimizer kernels take these tensors?  (GPU, fp32 / fp64, the kernels' sizes, gradient and
        momentum buffer of the parameter's dtype and shape, contiguous state; Stiefel has no exp.)"""
        ok = (x.is_cuda and egrad.is_cuda and x.dtype in (torch.float32, torch.float64) and x.numel() > 0
              and x.ndim >= 2 and tuple(x.shape[-2:]) == (self.n, self.p) and egrad.shape == x.shape
              and egrad.dtype == x.dtype and not (exact and self._kind == B.STIEFEL))
        if ok and buf is not None:
            ok = buf.is_cuda and buf.is_contiguous() and buf.dtype == x.dtype and buf.shape == x.shape
        if not ok:
            return False
        lib = B.lib()
        return self.n <= lib.raw('mm_mat_max_rows')() and self.p <= lib.raw('mm_mat_max_cols')()

    def rsgd_step(self, x, egrad, *, lr, max_grad_norm=None, exact=False, inplace=False):
        """Fused momentum-free RiemannianSGD update (optim/rsgd.py:63-68,82) in one launch, with this instance's
        retraction (or `exp` when `exact`); `inplace=True` writes the new points over `x` (each thread reads its
        whole point before writing it).  Returns the new points, or None when the tensors are not eligible."""
        if not self._step_eligible(x, egrad, exact):
            return None
        xd = x.detach()
        inplace = inplace and xd.is_contiguous()
        xc = xd.reshape(-1, self.n, self.p).contiguous()
        gc = egrad.detach().reshape(-1, self.n, self.p).contiguous()
        with B.on_device(xc.device):
            out = xc if inplace else torch.empty_like(xc)
            B.lib().call('mm_mat_rsgd_step', B.dtype_code(xc), self._kind, self._retr_op, B.ptr(xc), B.ptr(gc),
                         xc.shape[0], self.n, self.p, float(lr),
                         -1.0 if max_grad_norm is None else float(max_grad_norm), int(bool(exact)), B.ptr(out),
                         B.stream_of(xc))
        return x if inplace else out.reshape(x.shape)

    def rsgd_momentum_step(self, x, egrad, buf, *, lr, momentum, dampening, max_grad_norm=None, exact=False,
                           inplace=False):
        """Fused heavy-ball RiemannianSGD update (optim/rsgd.py:70-80): `buf` (the momentum buffer) is updated and
        transported in place; returns the new points, or None when the tensors are not eligible."""
        if not self._step_eligible(x, egrad, exact, buf):
            return None
        xd = x.detach()
        inplace = inplace and xd.is_contiguous()
        xc = xd.reshape(-1, self.n, self.p).contiguous()
        gc = egrad.detach().reshape(-1, self.n, self.p).contiguous()
        with B.on_device(xc.device):
            out = xc if inplace else torch.empty_like(xc)
            B.lib().call('mm_mat_rsgd_momentum_step', B.dtype_code(xc), self._kind, self._retr_op, B.ptr(xc),
                         B.ptr(gc), B.ptr(buf), xc.shape[0], self.n, self.p, float(lr), float(momentum),
                         float(dampening), -1.0 if max_grad_norm is None else float(max_grad_norm),
                         int(bool(exact)), B.ptr(out), B.stream_of(xc))
        return x if inplace else out.reshape(x.shape)

    def radam_step(self, x, egrad, exp_avg, exp_avg_sq, step, ticket, *, lr, betas, nc, eps, max_grad_norm=None,
                   exact=False, inplace=False):
        """Fused RiemannianAdam update (optim/radam.py:62-98) in one launch (mm_mat_radam_step), with this instance's
        retraction (or `exp` when `exact`): moments updated in place, `step` (device fp64 scalar) advanced by the
        kernel; returns the new points (`x` itself when `inplace`), or None when the tensors are not eligible (CPU
        tensors, non-contiguous or mistyped moments, Stiefel with `exact`)."""
        if not (self._step_eligible(x, egrad, exact, exp_avg) and self._step_eligible(x, egrad, exact, exp_avg_sq)):
            return None
        xd = x.detach()
        inplace = inplace and xd.is_contiguous()
        xc = xd.reshape(-1, self.n, self.p).contiguous()
        gc = egrad.detach().reshape(-1, self.n, self.p).contiguous()
        with B.on_device(xc.device):
            out = xc if inplace else torch.empty_like(xc)
            B.lib().call('mm_mat_radam_step', B.dtype_code(xc), self._kind, self._retr_op, B.ptr(xc), B.ptr(gc),
                         B.ptr(exp_avg), B.ptr(exp_avg_sq), B.ptr(step), B.ptr(ticket), xc.shape[0], self.n, self.p,
                         float(lr), float(betas[0]), float(betas[1] if betas[1] is not None else 0.0), int(bool(nc)),
                         float(eps), -1.0 if max_grad_norm is None else float(max_grad_norm), int(bool(exact)),
                         B.ptr(out), B.stream_of(xc))
        return x if inplace else out.reshape(x.shape)

    def rand(self, *shape, out=None, ir=1e-2):
        x = self.zero(*shape, out=out)
        with torch.no_grad():
            return self._rand_step(x, self.randvec(x, norm=ir))

    def rand_uniform(self, *shape, out=None):
        with torch.no_grad():
            return self.projx(torch.randn(*shape, self.n, self.p, **_like(out)), inplace=True)

    def randvec(self, x, norm):
        with torch.no_grad():
            u = self.proju(x, torch.randn_like(x))
        return u.div_(u.norm(dim=(-2, -1), keepdim=True)).mul_(norm)


class Grassmann(_MatrixManifold):
    _kind = B.GRASSMANN

    def __init__(self, n, p, retr='svd', requires_grad=True):
        super().__init__(n, p, retr)
        self.requires_grad = requires_grad

    @property
    def dim(self):
        return self.p * (self.n - self.p)

    def projx(self, x, inplace=False):  # grassmann.py:55-61
        new = self._map(B.MAT_PROJX, x.detach() if inplace else x)
        if not inplace:
            return new
        x.set_(new)
        return x

    def exp(self, x, u):  # grassmann.py:63-69
        return self._map(B.MAT_EXP, x, u)

    def log(self, x, y):  # grassmann.py:82-89
        return self._map(B.MAT_LOG, x, y)

    def _rand_step(self, x, u):
        return self.exp(x, u)

    def dist(self, x, y, squared=False, keepdim=False):  # grassmann.py:91-96
        shape = torch.broadcast_shapes(x.shape, y.shape)
        d = _GrassDist.apply(x.expand(shape), y.expand(shape), self.n, self.p, squared).reshape(shape[:-2])
        return d.reshape(*d.shape, 1, 1) if keepdim else d

    def pdist(self, x, squared=False, rows=None):  # base.py:59-63
        assert x.ndim == 3
        rb, re = (0, x.shape[0]) if rows is None else rows
        return _GrassPdist.apply(x, self.n, self.p, squared, rb, re)

    def pdist_loss(self, x, scale, target, spec, rows=None):
        """Fused `objective(target, softplus(scale) * pdist(x, squared=True))` with its gradients in
        one pass; `spec` comes from `objective_fn.fused_spec(epoch=, alpha=)`."""
        assert x.ndim == 3
        rb, re = (0, x.shape[0]) if rows is None else rows
        return _GrassPdistLoss.apply(x, scale, target, self.n, self.p, spec, rb, re)

    def subset_form(self, x):
        """Can mm_grass_pdist_loss_subset take a node minibatch of the table `x`?  (GPU, fp32 / fp64, [n, N, p], and an
        instantiation the library has built.)"""
        if not (x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.ndim == 3
                and tuple(x.shape[-2:]) == (self.n, self.p)):
            return False
        return B.lib().raw('mm_grass_pdist_loss_subset_form')(B.dtype_code(x), self.n, self.p) == 1

    def pdist_loss_subset(self, x, scale, idx, dense, spec, rows=None, cache=None):
        """`pdist_loss` for the node minibatch `idx` of the full table `x` with the targets dense[idx[a], idx[b]], inside
        the pair kernel; None when the tensors are not eligible (the caller then gathers)."""
        if not (self.subset_form(x) and dense.is_cuda):
            return None
        return _GrassSubsetLoss.apply(spec, rows, self.n, self.p, cache, idx, dense, x, scale)

    def __str__(self):
        return 'Grassmann manifold of {}x{} matrices'.format(self.n, self.p)


class Stiefel(_MatrixManifold):
    _kind = B.STIEFEL

    @property
    def dim(self):
        return self.p * self.n - self.p * (self.p + 1) // 2

    def _orthonormalize(self, x):  # stiefel.py:47-50: Q of QR with columns signed by diag(R)
        return self._map(B.MAT_PROJX, x)

    def projx(self, x, inplace=False):  # stiefel.py:53-57 (returns x itself when not inplace, as shipped)
        if inplace:
            x.set_(self._orthonormalize(x.detach()))
        return x

    def exp(self, x, u):  # stiefel.py:59-60 (sic: returns the exception class)
        return NotImplementedError

    def log(self, x, y):
        return NotImplementedError

    def dist(self, x, y, squared=False, keepdim=False):
        return NotImplementedError

    def _rand_step(self, x, u):
        return self.retr(x, u)

    def rand_uniform(self, *shape, out=None):
        with torch.no_grad():
            return self._orthonormalize(torch.randn(*shape, self.n, self.p, **_like(out)))

    def __str__(self):
        return 'Stiefel manifold of {}x{} matrices'.format(self.n, self.p)
