"""The kappa-stereographic model of constant curvature with a LEARNABLE curvature — the counterpart of the reference's
`Universal` manifold (manifolds/universal.py, manifolds/impl/math.py) on the gfx950 kernels of csrc/stereo.hip: the Poincare
ball for c > 0, the stereographic projection of the sphere for c < 0, K = -c.

The kernels read the raw curvature parameter from device memory and apply `get_c` themselves; `pdist` / `dist` return
gradients for the points AND for `self.c`.  Under the overlay the name `Universal` keeps resolving to the checkout's class
(this module defines none of that name); `Stereographic.from_universal(obj)` adopts such an instance's state."""
import ctypes

import torch
from torch.nn.functional import softplus

from graphembed import _backend as B
from graphembed.manifolds.base import Manifold

MAX_DIM = 16


def _curv_args(man, like):
    """(c_raw on `like`'s device in its dtype, c_mode, c_min) — a device-side cast at most, no host read of c."""
    c = man.c.detach()
    if c.device != like.device:
        raise B.BackendError(f'the curvature lives on {c.device}, the points on {like.device}: move the manifold with .to(device)')
    if c.dtype != like.dtype:
        c = c.to(like.dtype)
    mode = B.STEREO_C_FREE if not man.sign else B.STEREO_C_POSITIVE if man.sign > 0 else B.STEREO_C_NEGATIVE
    return c.contiguous(), mode, float(man.c_min)


class _StereoPdist(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, c, man, squared, row_begin, row_end):
        B.require_gpu(x)
        lib = B.lib()
        n, m = x.shape
        xc = x.detach().contiguous()
        cr, mode, c_min = _curv_args(man, xc)
        npairs = B.pair_offset(n, row_end) - B.pair_offset(n, row_begin)
        ctx.save_for_backward(xc, cr)
        ctx.args = (mode, c_min, squared, row_begin, row_end, c.dtype)
        with B.on_device(xc.device):
            out = torch.empty(npairs, dtype=xc.dtype, device=xc.device)
            lib.call('mm_stereo_pdist_fwd', B.dtype_code(xc), B.ptr(xc), n, m, row_begin, row_end, int(squared), B.ptr(cr),
                     mode, c_min, B.ptr(out), B.stream_of(xc))
        return out

    @staticmethod
    def backward(ctx, g):
        xc, cr = ctx.saved_tensors
        mode, c_min, squared, row_begin, row_end, cdtype = ctx.args
        lib = B.lib()
        n, m = xc.shape
        dt = B.dtype_code(xc)
        g = g.contiguous()
        with B.on_device(xc.device):
            grad = torch.empty_like(xc) if n >= 2 else torch.zeros_like(xc)   # (n < 2: the call writes nothing but a zero grad_c)
            gc = torch.empty(1, dtype=xc.dtype, device=xc.device)
            ws = torch.empty(lib.raw('mm_stereo_pdist_ws_bytes')(dt, n, m), dtype=torch.uint8, device=xc.device)
            lib.call('mm_stereo_pdist_bwd', dt, B.ptr(xc), B.ptr(g), n, m, row_begin, row_end, int(squared), B.ptr(cr), mode,
                     c_min, B.ptr(grad), B.ptr(gc), B.ptr(ws), B.stream_of(xc))
        return grad, gc.to(cdtype), None, None, None, None


class _StereoDist(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, y, c, man, squared):
        B.require_gpu(x, y)
        m = man.n
        xc = x.detach().reshape(-1, m).contiguous()
        yc = y.detach().reshape(-1, m).contiguous()
        cr, mode, c_min = _curv_args(man, xc)
        with B.on_device(xc.device):
            out = torch.empty(xc.shape[0], dtype=xc.dtype, device=xc.device)
            B.lib().call('mm_stereo_dist', B.dtype_code(xc), B.ptr(xc), B.ptr(yc), None, xc.shape[0], m, int(squared), B.ptr(cr),
                         mode, c_min, B.ptr(out), None, None, None, None, B.stream_of(xc))
        ctx.save_for_backward(xc, yc, cr)
        ctx.args = (mode, c_min, squared, x.shape, y.shape, c.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, yc, cr = ctx.saved_tensors
        mode, c_min, squared, xs, ys, cdtype = ctx.args
        cnt, m = xc.shape
        g = g.reshape(-1).contiguous()
        with B.on_device(xc.device):
            gx, gy = torch.empty_like(xc), torch.empty_like(yc)
            gc = torch.empty(1, dtype=xc.dtype, device=xc.device)
            ws = torch.empty(8 * ((cnt + 127) // 128 + 1), dtype=torch.uint8, device=xc.device)
            B.lib().call('mm_stereo_dist', B.dtype_code(xc), B.ptr(xc), B.ptr(yc), B.ptr(g), cnt, m, int(squared), B.ptr(cr), mode,
                         c_min, None, B.ptr(gx), B.ptr(gy), B.ptr(gc), B.ptr(ws), B.stream_of(xc))
        return gx.reshape(xs), gy.reshape(ys), gc.to(cdtype), None, None

MAX_FACTORS = 8   # mm_stereo_product_*: more factors are MM_ERR_UNSUPPORTED


def _product_call(xs, mans, kind, target, rows, spec, want_loss):
    """mm_stereo_product_loss on detached, contiguous points: (loss [1] or None, [grad_x_k], [grad_c_k])."""
    lib = B.lib()
    n = xs[0].shape[0]
    dt = B.dtype_code(xs[0])
    dev = xs[0].device
    curv = [_curv_args(man, xs[0]) for man in mans]
    _, alpha, eps, terms = spec[:4]
    dyn = spec[4] if len(spec) > 4 else None
    with B.on_device(dev):
        gxs = [torch.empty_like(x) for x in xs]
        gcs = torch.empty(len(xs), dtype=xs[0].dtype, device=dev)
        loss = torch.empty(1, dtype=xs[0].dtype, device=dev) if want_loss else None
        ms = (ctypes.c_int32 * len(xs))(*[x.shape[1] for x in xs])
        ws = torch.empty(lib.raw('mm_stereo_product_ws_bytes')(dt, n, len(xs), ms), dtype=torch.uint8, device=dev)
        fs = B.stereo_factors([(x, cr, gx, gcs[k:k + 1], c_min, x.shape[1], mode)
                               for k, (x, gx, (cr, mode, c_min)) in enumerate(zip(xs, gxs, curv))])
        lib.call('mm_stereo_product_loss', dt, kind, fs, len(xs), B.ptr(target), n, rows[0], rows[1], alpha, eps, terms,
                 B.dyn_ptr(dyn, xs[0]), B.ptr(loss), B.ptr(ws), B.stream_of(xs[0]))
    return loss, gxs, [gcs[k:k + 1] for k in range(len(xs))]


class _StereoProductPdist(torch.autograd.Function):
    """sum_k pdist_k(x_k, squared=True) of a product of Stereographic factors: one forward launch for all factors
    (mm_stereo_product_pdist_fwd) and one pair pass for every gradient (mm_stereo_product_loss with MM_LOSS_NONE)."""

    @staticmethod
    def forward(ctx, mans, rows, *params):
        k = len(mans)
        B.require_gpu(*params[:k])
        xs = [x.detach().contiguous() for x in params[:k]]
        n = xs[0].shape[0]
        curv = [_curv_args(man, xs[0]) for man in mans]
        npairs = B.pair_offset(n, rows[1]) - B.pair_offset(n, rows[0])
        with B.on_device(xs[0].device):
            out = torch.empty(npairs, dtype=xs[0].dtype, device=xs[0].device)
            fs = B.stereo_factors([(x, cr, None, None, c_min, x.shape[1], mode) for x, (cr, mode, c_min) in zip(xs, curv)])
            B.lib().call('mm_stereo_product_pdist_fwd', B.dtype_code(xs[0]), fs, k, n, rows[0], rows[1], B.ptr(out), B.stream_of(xs[0]))
        ctx.save_for_backward(*xs, *[cr for cr, _, _ in curv])
        ctx.args = (mans, rows, [c.dtype for c in params[k:]])
        return out

    @staticmethod
    def backward(ctx, g):
        mans, rows, cdtypes = ctx.args
        k = len(mans)
        xs = list(ctx.saved_tensors[:k])
        # (the saved c_raw copies are the forward's curvatures: the kernels read them, not man.c, in the backward)
        held = [_Held(man, cr) for man, cr in zip(mans, ctx.saved_tensors[k:])]
        _, gxs, gcs = _product_call(xs, held, B.LOSS_NONE, g.contiguous(), rows, (None, 1.0, 0.0, 0), False)
        return (None, None, *gxs, *[gc.to(dt) for gc, dt in zip(gcs, cdtypes)])


class _Held:
    """a manifold's curvature mode with a saved c_raw in place of the live parameter (what `_curv_args` reads)"""

    def __init__(self, man, c):
        self.c, self.sign, self.c_min = c, man.sign, man.c_min


class _StereoProductLoss(torch.autograd.Function):
    """The objective of a product of Stereographic factors in one pair pass (mm_stereo_product_loss): the loss and the
    gradients of every x_k and every curvature; `spec` comes from `objective_fn.fused_spec(epoch=, alpha=)`."""

    @staticmethod
    def forward(ctx, mans, rows, spec, target, *params):
        k = len(mans)
        B.require_gpu(*params[:k])
        xs = [x.detach().contiguous() for x in params[:k]]
        n = xs[0].shape[0]
        npairs = B.pair_offset(n, rows[1]) - B.pair_offset(n, rows[0])
        tc = target.detach().to(xs[0].dtype).contiguous()
        if tc.numel() != npairs:
            raise ValueError(f'target has {tc.numel()} entries, the pair range has {npairs}')
        kind = B.LOSS_STRESS if spec[0] == 'stress' else B.LOSS_QUOTIENT
        loss, gxs, gcs = _product_call(xs, mans, kind, tc, rows, spec, True)
        ctx.grads = gxs + [gc.to(c.dtype) for gc, c in zip(gcs, params[k:])]
        return loss[0]

    @staticmethod
    def backward(ctx, up):
        return (None, None, None, None, *B.take_grads(ctx, up, 'grads'))


class _StereoProductSubsetLoss(torch.autograd.Function):
    """The objective of a NODE MINIBATCH of a product of Stereographic factors inside the pair kernel
    (mm_stereo_product_loss_subset): `params` are the FULL tables and the curvatures, `idx` addresses the tables' rows and the
    targets dense[idx[a]][idx[b]], the gradients come back full-size with exact zeros outside the batch - no gather, no
    scatter-add.  `cache` (a dict kept by the embedding) holds the batch-sized workspace: a captured graph refers to it."""

    @staticmethod
    def forward(ctx, mans, rows, spec, cache, idx, dense, *params):
        k = len(mans)
        B.require_gpu(*params[:k], dense)
        lib = B.lib()
        xs = [x.detach().contiguous() for x in params[:k]]
        n_total, bs = xs[0].shape[0], idx.numel()
        dt, dev = B.dtype_code(xs[0]), xs[0].device
        if dense.dtype != xs[0].dtype or not dense.is_contiguous() or dense.shape != (n_total, n_total):
            raise ValueError('dense targets must be a contiguous [n, n] matrix of the embedding\'s dtype')
        kind = B.LOSS_STRESS if spec[0] == 'stress' else B.LOSS_QUOTIENT
        _, alpha, eps, terms = spec[:4]
        dyn = spec[4] if len(spec) > 4 else None
        curv = [_curv_args(man, xs[0]) for man in mans]
        with B.on_device(dev):
            ic = idx.to(device=dev, dtype=torch.int64).contiguous()
            gxs = [torch.empty_like(x) for x in xs]
            gcs = torch.empty(k, dtype=xs[0].dtype, device=dev)
            loss = torch.empty(1, dtype=xs[0].dtype, device=dev)
            key = (xs[0].dtype, dev, bs)
            ws = cache.get(key)
            if ws is None:
                ms = (ctypes.c_int32 * k)(*[x.shape[1] for x in xs])
                ws = torch.empty(lib.raw('mm_stereo_product_ws_bytes')(dt, bs, k, ms), dtype=torch.uint8, device=dev)
                cache[key] = ws
            fs = B.stereo_factors([(x, cr, gx, gcs[j:j + 1], c_min, x.shape[1], mode)
                                   for j, (x, gx, (cr, mode, c_min)) in enumerate(zip(xs, gxs, curv))])
            lib.call('mm_stereo_product_loss_subset', dt, kind, fs, k, B.ptr(dense), n_total, B.ptr(ic), bs, rows[0], rows[1],
                     alpha, eps, terms, B.dyn_ptr(dyn, xs[0]), B.ptr(loss), B.ptr(ws), B.stream_of(xs[0]))
        ctx.grads = gxs + [gcs[j:j + 1].to(c.dtype) for j, c in enumerate(params[k:])]
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, up):
        return (None, None, None, None, None, None, *B.take_grads(ctx, up, 'grads'))


def product_loss_subset(mans, xs, idx, dense, spec, cache, rows=None):
    """The fused objective of the node minibatch `idx` of the product; see _StereoProductSubsetLoss."""
    rb, re = (0, idx.numel()) if rows is None else rows
    return _StereoProductSubsetLoss.apply(tuple(mans), (int(rb), int(re)), tuple(spec), cache, idx, dense, *xs, *[man.c for man in mans])


def product_pdist(mans, xs, rows=None):
    """The summed squared pair distances of the factors (`mans[k]` on `xs[k]`), differentiable in every x_k and man.c."""
    n = xs[0].shape[0]
    rb, re = (0, n) if rows is None else rows
    return _StereoProductPdist.apply(tuple(mans), (int(rb), int(re)), *xs, *[man.c for man in mans])


def product_loss(mans, xs, target, spec, rows=None):
    """The fused objective of the product; see _StereoProductLoss."""
    n = xs[0].shape[0]
    rb, re = (0, n) if rows is None else rows
    return _StereoProductLoss.apply(tuple(mans), (int(rb), int(re)), tuple(spec), target, *xs, *[man.c for man in mans])


class Stereographic(Manifold, torch.nn.Module):
    """`Universal(n, c_init, c_min, keep_sign_fixed)` of the reference (universal.py:10-17), same state: `n`, `c_min`,
    `sign` (None | 1 | -1) and the raw curvature Parameter `c`."""

    def __init__(self, n, c_init=0.01, c_min=0.001, keep_sign_fixed=False):
        super().__init__()
        if not 1 <= n <= MAX_DIM:
            raise ValueError(f'the stereographic kernels serve 1 <= n <= {MAX_DIM}, got {n}')
        self.n = n
        self.c_min = c_min
        self.sign = None if not keep_sign_fixed else 1 if c_init > 0 else -1
        self.c = torch.nn.Parameter(torch.Tensor([c_init]))

    @classmethod
    def from_universal(cls, obj):
        """A Stereographic with the state of `obj`: any object with `n`, `c`, `c_min` and `sign` — the checkout's
        `Universal` instance, for one.  The curvature is copied, not shared."""
        man = cls(int(obj.n), c_min=float(obj.c_min))
        man.sign = None if not obj.sign else 1 if obj.sign > 0 else -1
        c = obj.c.detach() if isinstance(obj.c, torch.Tensor) else torch.tensor([float(obj.c)])
        man.c = torch.nn.Parameter(c.clone().reshape(1))
        return man

    @property
    def ndim(self):
        return 1

    @property
    def dim(self):
        return self.n

    def get_c(self):   # universal.py:27-31
        if self.sign:
            return self.sign * (self.c_min + softplus(self.c))
        return self.c.sign() * self.c_min + self.c

    def get_K(self):
        return -self.get_c()

    def get_R(self):
        return 1.0 / torch.sqrt(torch.abs(self.get_c()))

    def zero(self, *shape, out=None):
        return torch.zeros(*shape, self.n, out=out)

    def zero_vec(self, *shape, out=None):
        return torch.zeros(*shape, self.n, out=out)

    def inner(self, x, u, v, keepdim=False):   # impl/math.py:225-228 (lambda clamped at MIN_NORM = 1e-15, :187-190)
        lam = 2 / (1 - self.get_c() * x.pow(2).sum(-1, keepdim=True)).clamp_min(1e-15)
        res = lam**2 * (u * v).sum(-1, keepdim=True)
        return res if keepdim else res.squeeze(-1)

    def norm(self, x, u, squared=False, keepdim=False):
        # universal.py:48-52 calls math.norm(x, u) WITHOUT c: the conformal factor is taken at c = 1 (impl/math.py:231,
        # 261-264).  RSGD's clip threshold depends on it, so it is reproduced, here and in mm_stereo_rsgd_step.
        lam = 2 / (1 - x.pow(2).sum(-1, keepdim=keepdim)).clamp_min(1e-15)
        norm = lam * u.norm(dim=-1, keepdim=keepdim, p=2)
        return norm.pow(2) if squared else norm

    # -- per-point maps ----------------------------------------------------------------------------------------------
    def _map(self, op, x, u=None, y=None):
        B.require_gpu(x, u, y)
        ts = [t for t in (x, u, y) if t is not None]
        if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
            raise NotImplementedError('exp/log/retr/proj*/transp are optimizer-side maps (torch.no_grad) on the HIP path; '
                                      'only dist/pdist are differentiable')
        shape = torch.broadcast_shapes(*[t.shape for t in ts])
        flat = [None if t is None else t.detach().expand(shape).reshape(-1, self.n).contiguous() for t in (x, u, y)]
        xc = flat[0]
        cr, mode, c_min = _curv_args(self, xc)
        with B.on_device(xc.device):
            out = torch.empty_like(xc)
            B.lib().call('mm_stereo_map', B.dtype_code(xc), op, B.ptr(flat[0]), B.ptr(flat[1]), B.ptr(flat[2]), xc.shape[0], self.n,
                         B.ptr(cr), mode, c_min, B.ptr(out), B.stream_of(xc))
        return out.reshape(shape)

    def proju(self, x, u, inplace=False):   # universal.py:54-55: the identity
        return u

    def projx(self, x, inplace=False):
        # (universal.py:57-61 returns the UNPROJECTED x when inplace=False - the projection is computed and dropped; here the
        # projected points are returned in both cases, as the other manifolds of this package do)
        new = self._map(B.STEREO_PROJX, x.detach() if inplace else x)
        if inplace:
            x.set_(new)
            return x
        return new

    def egrad2rgrad(self, x, u):
        return self._map(B.STEREO_EGRAD2RGRAD, x, u)

    def exp(self, x, u, project=True):
        return self._map(B.STEREO_EXP if project else B.STEREO_EXP_NOPROJECT, x, u)

    def retr(self, x, u):
        return self._map(B.STEREO_RETR, x, u)

    def log(self, x, y):
        return self._map(B.STEREO_LOG, x, None, y)

    def transp(self, x, y, u):
        return self._map(B.STEREO_TRANSP, x, u, y)

    def rsgd_step(self, x, egrad, *, lr, max_grad_norm=None, exact=False, inplace=False):
        """Fused momentum-free RiemannianSGD update (optim/rsgd.py:63-68,82 of the reference) in one launch;
        `inplace=True` writes the new points over `x` (a thread reads its whole point before writing it)."""
        B.require_gpu(x, egrad)
        xd = x.detach()
        inplace = inplace and xd.is_contiguous()
        xc = xd.reshape(-1, self.n).contiguous()
        gc = egrad.detach().reshape(-1, self.n).to(xc.dtype).contiguous()
        cr, mode, c_min = _curv_args(self, xc)
        with B.on_device(xc.device):
            out = xc if inplace else torch.empty_like(xc)
            B.lib().call('mm_stereo_rsgd_step', B.dtype_code(xc), B.ptr(xc), B.ptr(gc), xc.shape[0], self.n, B.ptr(cr), mode, c_min,
                         float(lr), -1.0 if max_grad_norm is None else float(max_grad_norm), int(bool(exact)), B.ptr(out),
                         B.stream_of(xc))
        return x if inplace else out.reshape(x.shape)

    def radam_step(self, x, egrad, exp_avg, exp_avg_sq, step, ticket, *, lr, betas, nc, eps, max_grad_norm=None, exact=False,
                   inplace=False):
        """Fused RiemannianAdam update (optim/radam.py:62-98 of the reference) in one launch (mm_stereo_radam_step): moments
        updated in place, `step` (device fp64 scalar) advanced by the kernel; returns the new points (`x` itself when
        `inplace`), or None when the tensors are not eligible (CPU tensors, non-contiguous or mistyped moments)."""
        ok = (x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.numel() > 0 and x.shape[-1] == self.n
              and exp_avg.is_contiguous() and exp_avg_sq.is_contiguous() and exp_avg.dtype == x.dtype
              and exp_avg_sq.dtype == x.dtype and exp_avg.shape == x.shape and exp_avg_sq.shape == x.shape)
        if not ok:
            return None
        xd = x.detach()
        inplace = inplace and xd.is_contiguous()
        xc = xd.reshape(-1, self.n).contiguous()
        gc = egrad.detach().reshape(-1, self.n).to(xc.dtype).contiguous()
        cr, mode, c_min = _curv_args(self, xc)
        with B.on_device(xc.device):
            out = xc if inplace else torch.empty_like(xc)
            B.lib().call('mm_stereo_radam_step', B.dtype_code(xc), B.ptr(xc), B.ptr(gc), B.ptr(exp_avg), B.ptr(exp_avg_sq),
                         B.ptr(step), B.ptr(ticket), xc.shape[0], self.n, B.ptr(cr), mode, c_min, float(lr), float(betas[0]),
                         float(betas[1] if betas[1] is not None else 0.0), int(bool(nc)), float(eps),
                         -1.0 if max_grad_norm is None else float(max_grad_norm), int(bool(exact)), B.ptr(out), B.stream_of(xc))
        return x if inplace else out.reshape(x.shape)

    @torch.no_grad()
    def stabilize_(self, x, r_max):
        """products/embedding.py:37-46 of the reference — x / max(|x| / r_max, 1), then projx — over `x`, one launch."""
        B.require_gpu(x)
        xd = x.detach()
        if not xd.is_contiguous():
            raise ValueError('stabilize_ writes in place and needs contiguous points')
        cr, mode, c_min = _curv_args(self, xd)
        with B.on_device(xd.device):
            B.lib().call('mm_stereo_stabilize', B.dtype_code(xd), B.ptr(xd), xd.numel() // self.n, self.n, B.ptr(cr), mode, c_min,
                         float(r_max), B.ptr(xd), B.stream_of(xd))
        return x

    # -- distances -------------------------------------------------------------------------------------------------------
    def dist(self, x, y, squared=False, keepdim=False):
        shape = torch.broadcast_shapes(x.shape, y.shape)
        d = _StereoDist.apply(x.expand(shape), y.expand(shape), self.c, self, bool(squared)).reshape(shape[:-1])
        return d.unsqueeze(-1) if keepdim else d

    def pdist(self, x, squared=False, rows=None):
        """All-pairs distances, row-major upper triangle (base.py:59-63 of the reference); `rows` selects the pair-list
        slice of one shard, as VectorManifold.pdist does.  Differentiable in `x` and in `self.c`."""
        assert x.ndim == 2 and x.shape[1] == self.n
        rb, re = (0, x.shape[0]) if rows is None else rows
        return _StereoPdist.apply(x, self.c, self, bool(squared), int(rb), int(re))

    def rand(self, *shape, out=None, ir=1e-2):   # universal.py:89-91 (under no_grad: the in-place set_ has no derivative)
        with torch.no_grad():
            x = torch.empty(*shape, self.n, out=out).uniform_(-ir, ir)
            if x.is_cuda:
                return self.projx(x, inplace=True)
            # default placement is the host, as in the reference: the projection there is three tensor ops
            c = self.get_c().to(x.dtype)
            if bool(c > 0):
                nrm = x.norm(dim=-1, keepdim=True, p=2).clamp_min(1e-15)
                maxnorm = (1 - (4e-3 if x.dtype == torch.float32 else 1e-5)) / c.abs().sqrt()
                x = torch.where(nrm > maxnorm, x / nrm * maxnorm, x)
            return x

    def randvec(self, x, norm=1):
        raise NotImplementedError

    def __str__(self):
        return f'Stereographic {self.n}-dimensional manifold'
