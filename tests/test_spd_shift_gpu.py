"""SPD pair kernels with the forward on right-aligned column blocks (spd_ws.hpp: the forward's tile map is that of the problem
with s = (bw - n mod bw) mod bw phantom nodes in FRONT, so the ragged wavefront of 64 / 128 columns sits at the thin end of the
triangle; the backward keeps its plain walk and consumes what the shifted forward wrote).
Sizes: n mod bw of 0, 1, small and bw - 1 for both widths (64: SPD(4), fp64; 128: fp32 SPD(2), SPD(3)), one, two and three
blocks, and the forward's 512-column tile boundary.  Everything is compared with the fp64 checker (oracle/exact.c: distances and
spd_pdist_grad) under the rules and tolerances of tests/test_spd_gpu.py, which are imported, not restated.

The inputs are rounded to fp32 once and serve the fp32 and the fp64 launch, so one reference per (n, d, spread) is computed,
shared and left unchanged."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_spd_gpu as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 63, 64, 65, 127, 128, 129, 136, 200, 257, 513]
# The fused objective: the bounds of test_spd_gpu.test_fused_loss_vs_oracle_seeded for the loss, d loss / d x and d loss / d scale.
# They are wider than GRAD_TOL because the residual m - target amplifies the error of d^2: a pair's term carries
# (m - t) d(d^2), and D2_TOL allows d^2 an error of 1e-6 + 2e-5 d^2 — 1e-4 of the d^2 ~ 0.01 of the reference initialisation.  The
# targets below keep |m - t| >= 0.2 m, so that the amplification is at most five whatever the number of pairs (n = 2 has one);
# d loss / d scale is a sum of signed terms and is bounded relative to sum |term| (a bound relative to the NET sum means nothing
# where the terms cancel, as they can completely for the one or three pairs of n = 2, 3).
LOSS_REL = {'f32': 2e-5, 'f64': 2e-6}
FUSED_GX_TOL = {'f32': 2e-4, 'f64': 5e-5}
FUSED_GS_TOL = {'f32': 1e-3, 'f64': 5e-4}


def _points(n, d, spread, gen):
    from oracle import ref_port as rp
    port = rp.SPD(d)
    if spread is None:                                   # the reference initialisation: ||log X|| = 0.1
        return port.rand(n, ir=0.1, dtype=torch.float64, generator=gen)
    scale = spread * (0.6 + 0.4 * torch.rand(n, generator=gen))   # (the generator of test_spd_gpu._series_regime)
    u = torch.randn(n, d * (d + 1) // 2, dtype=torch.float64, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True) * scale.double().reshape(n, 1)
    return port.exp(port.zero(n, dtype=torch.float64), port.from_vec(u))


@functools.lru_cache(maxsize=None)
def _case(n, d, spread=None):
    """fp32-representable points, upstream gradient, the checker's d^2 and gradients: computed once, read-only."""
    from oracle import exact
    gen = torch.Generator().manual_seed(100003 * d + 17 * n + (0 if spread is None else int(spread * 100)))
    x = _points(n, d, spread, gen).float()
    g = torch.randn(n * (n - 1) // 2, generator=gen)     # fp32
    xin = x.double().numpy()
    d2 = exact.spd_pdist(xin)
    grads = {sq: exact.spd_pdist_grad(xin, g.double().numpy(), squared=sq) for sq in (True, False)}
    return dict(x=x, g=g, xin=xin, d2=d2, grads=grads)


def _pdist_checks(n, d, dname, spread=None, squared_forms=(True, False)):
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    c = _case(n, d, spread)
    dt = T.DT[dname]
    man = SPD(d)
    for squared in squared_forms:
        what = f'd={d} n={n} {dname} spread={spread} squared={squared}'
        x = c['x'].to(dt).cuda().requires_grad_()
        out = man.pdist(x, squared=squared)
        assert out.numel() == n * (n - 1) // 2
        T.check_d2(out if squared else out * out, c['d2'], dname, 'd2 ' + what)
        gr, = torch.autograd.grad(out, x, c['g'].to(dt).cuda())
        assert gr.shape == x.shape and bool(torch.isfinite(gr).all())
        T.check_grad(gr, c['grads'][squared], c['xin'], c['g'].double().numpy(), squared, dname,
                     T.GRAD_TOL[dname] * (1 if squared else 5), 'grad ' + what)   # (d: as test_pdist_vs_reference_golden)


@pytest.mark.parametrize('dname', list(T.DT))
@pytest.mark.parametrize('d', [2, 3, 4])
@pytest.mark.parametrize('n', SIZES)
def test_pdist_and_gradient(n, d, dname):
    _pdist_checks(n, d, dname)


@pytest.mark.parametrize('dname', list(T.DT))
@pytest.mark.parametrize('d', [3, 4])
@pytest.mark.parametrize('n', SIZES)
def test_pdist_and_gradient_recentred_path(n, d, dname):
    """Spread 0.35: far rows (fp32: the recentred series, fp64: the Cayley form) on shifted columns."""
    _pdist_checks(n, d, dname, spread=0.35)


@pytest.mark.parametrize('d', [6, 9])
def test_wider_matrices(d):
    _pdist_checks(129, d, 'f32', squared_forms=(True,))


# ------------------------------------------------------------------------------------------------------ fused objective
def _losses():
    from graphembed.objectives import QuotientLoss, StressLoss
    return {'stress': (StressLoss(), {}), 'quotient': (QuotientLoss(), dict(epoch=3, alpha=1.7))}


def _targets(md, kw, gen):
    """Targets of the size of the distances — m / t in [0.5, 0.8] or [1.2, 1.5]: no residual is a cancellation — and kept away
    from the |.| kinks of the quotient terms (test_fused_loss_vs_oracle_seeded)."""
    f = 0.5 + 0.6 * torch.rand(md.shape, dtype=torch.float64, generator=gen)
    f = torch.where(f > 0.8, f + 0.4, f)
    tgt = (md / f).clamp_min(1e-3).float().double()
    if kw:
        for _ in range(12):
            ag = tgt * kw['alpha']
            near = ((md / ag - 1).abs() < 0.05) | ((ag / (md + 1 / (kw['epoch'] + 1)) - 1).abs() < 0.05)
            tgt = torch.where(near, tgt * 1.25, tgt).float().double()
        assert not near.any()
    return tgt


def _objective_reference(fn, kw, d2, tgt, xin, s_raw=0.3):
    """loss, d loss / d x, d loss / d scale and sum |term| of the latter, from the checker's d^2 and gradient."""
    from oracle import exact
    sp = float(np.log1p(np.exp(s_raw)))
    md = (sp * torch.from_numpy(d2)).requires_grad_()
    loss = fn(tgt, md, **kw)
    dl, = torch.autograd.grad(loss, md)
    dl = dl.numpy()
    gx = exact.spd_pdist_grad(xin, dl * sp) if d2.size else np.zeros_like(xin)
    sig = 1.0 / (1.0 + np.exp(-s_raw))
    return float(loss.detach()), gx, float((dl * d2).sum() * sig), float(np.abs(dl * d2).sum() * sig)


def _check_objective(what, dname, loss, gx, gs, ref):
    ref_loss, ref_gx, ref_gs, gs_terms = ref
    assert abs(loss - ref_loss) <= LOSS_REL[dname] * abs(ref_loss), (what, loss, ref_loss)
    T.check_rel(gx, ref_gx, FUSED_GX_TOL[dname], 'grad_x ' + what)
    assert abs(gs - ref_gs) <= FUSED_GS_TOL[dname] * gs_terms, (what, gs, ref_gs, gs_terms)


@pytest.mark.parametrize('dname', list(T.DT))
@pytest.mark.parametrize('d', [2, 3, 4])
@pytest.mark.parametrize('n', SIZES)
def test_fused_loss(n, d, dname):
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    c = _case(n, d)
    dt = T.DT[dname]
    for name, (fn, kw) in _losses().items():
        gen = torch.Generator().manual_seed(31 * n + d)
        tgt = _targets(float(np.log1p(np.exp(0.3))) * torch.from_numpy(c['d2']), kw, gen)
        ref = _objective_reference(fn, kw, c['d2'], tgt, c['xin'])
        x = c['x'].to(dt).cuda().requires_grad_()
        s = torch.tensor(0.3, dtype=dt, device='cuda', requires_grad=True)
        loss = SPD(d).pdist_loss(x, s, tgt.to(dt).cuda(), fn.fused_spec(**kw))
        gx, gs = torch.autograd.grad(loss, [x, s])
        _check_objective(f'{name} d={d} n={n} {dname}', dname, loss.item(), gx, gs.item(), ref)


@pytest.mark.parametrize('dname', list(T.DT))
@pytest.mark.parametrize('d', [2, 3, 4])
@pytest.mark.parametrize('bs', [100, 130])
def test_node_minibatch_inside_the_pair_kernel(bs, d, dname):
    """The SUB form (mm_spd_pdist_loss_subset) at batch sizes that leave a ragged column block: every node goes through the index vector."""
    from graphembed import _backend as B
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    from graphembed.modules import _SingleSubsetLoss
    from oracle import exact
    n_total = 300
    c = _case(n_total, d)
    dt = T.DT[dname]
    gen = torch.Generator().manual_seed(1000 * bs + d)
    idx = torch.randperm(n_total, generator=gen)[:bs]
    xb = c['xin'][idx.numpy()]
    d2b = exact.spd_pdist(xb)
    sp = float(np.log1p(np.exp(0.3)))
    iu = torch.triu_indices(bs, bs, 1)
    for name, (fn, kw) in _losses().items():
        tgt = _targets(sp * torch.from_numpy(d2b), kw, gen)
        dense = torch.full((n_total, n_total), 0.37, dtype=torch.float64)      # (entries outside the batch: never read)
        dense[idx[iu[0]], idx[iu[1]]] = tgt
        dense[idx[iu[1]], idx[iu[0]]] = tgt
        ref_loss, ref_gb, ref_gs, gs_terms = _objective_reference(fn, kw, d2b, tgt, xb)
        ref_gx = np.zeros_like(c['xin'])
        ref_gx[idx.numpy()] = ref_gb
        x = c['x'].to(dt).cuda().requires_grad_()
        s = torch.tensor(0.3, dtype=dt, device='cuda', requires_grad=True)
        loss = _SingleSubsetLoss.apply(fn.fused_spec(**kw), None, SPD(d), (B.FACTOR_SPD, d), None, idx.cuda(),
                                       dense.to(dt).cuda().contiguous(), x, s)
        gx, gs = torch.autograd.grad(loss, [x, s])
        _check_objective(f'subset {name} d={d} bs={bs} {dname}', dname, loss.item(), gx, gs.item(), (ref_loss, ref_gx, ref_gs, gs_terms))
        outside = torch.ones(n_total, dtype=torch.bool)
        outside[idx] = False
        assert bool((gx[outside.cuda()] == 0).all())


# ------------------------------------------------------------------------------------------------------ shards, workspaces
@pytest.mark.parametrize('dname', list(T.DT))
@pytest.mark.parametrize('d', [3, 4])
@pytest.mark.parametrize('n', [129, 257])
def test_row_shards_reproduce_the_unsharded_launch(n, d, dname):
    """The shift depends on n only: which pairs share a forward wavefront is a function of the column, whatever the shard — d^2 of the
    shards, concatenated, is the unsharded d^2 bit for bit, and the gradients add up."""
    from graphembed import _backend as B
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    c = _case(n, d)
    dt = T.DT[dname]
    man = SPD(d)
    x = c['x'].to(dt).cuda().requires_grad_()
    g = c['g'].to(dt).cuda()
    full = man.pdist(x, squared=True)
    gfull, = torch.autograd.grad(full, x, g)
    for k in (1, n // 3, 64, n - 2):
        parts, gsum = [], torch.zeros_like(gfull)
        for rb, re in ((0, k), (k, n)):
            xr = c['x'].to(dt).cuda().requires_grad_()
            part = man.pdist(xr, squared=True, rows=(rb, re))
            lo, hi = B.pair_offset(n, rb), B.pair_offset(n, re)
            assert part.numel() == hi - lo
            if hi > lo:
                gp, = torch.autograd.grad(part, xr, g[lo:hi])
                gsum += gp
            parts.append(part.detach())
        assert torch.equal(torch.cat(parts), full.detach()), (n, d, dname, k)
        T.check_rel(gsum, gfull.detach().double().cpu().numpy(), T.GRAD_TOL[dname], f'sum of shard gradients n={n} k={k}')


@pytest.mark.parametrize('d,dname', [(3, 'f32'), (4, 'f32'), (3, 'f64')])
def test_two_embeddings_through_one_workspace(d, dname):
    """Embeddings of different n — and so different shifts — one after the other through ONE workspace buffer: nothing of one
    launch (node tables, the backward's share table) may reach the other."""
    from graphembed import _backend as B
    lib = B.lib()
    dt_t = T.DT[dname]
    dt = B.dtype_code(torch.zeros(1, dtype=dt_t))
    sizes = [200, 129, 200, 136, 129, 136]
    nbytes = max(lib.raw('mm_spd_pdist_ws_bytes')(dt, n, d) for n in sizes)
    shared = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')

    def run(x, g, ws):
        n = x.shape[0]
        out = torch.empty(n * (n - 1) // 2, dtype=dt_t, device='cuda')
        grad = torch.empty_like(x)
        with B.on_device(x.device):
            lib.call('mm_spd_pdist_fwd', dt, B.ptr(x), n, d, 0, n, 1, 1e-8, 1e8, B.ptr(out), B.ptr(ws), 0, B.stream_of(x))
            lib.call('mm_spd_pdist_bwd', dt, B.ptr(x), B.ptr(g), n, d, 0, n, 1, 1e-8, 1e8, B.ptr(grad), B.ptr(ws), B.MM_WS_PREPARED,
                     B.stream_of(x))
        return out, grad

    for n in sizes:
        c = _case(n, d)
        x, g = c['x'].to(dt_t).cuda().contiguous(), c['g'].to(dt_t).cuda().contiguous()
        out, grad = run(x, g, shared[:lib.raw('mm_spd_pdist_ws_bytes')(dt, n, d)])
        T.check_d2(out, c['d2'], dname, f'd2 n={n} (shared workspace)')
        T.check_rel(grad, c['grads'][True], T.GRAD_TOL[dname], f'grad n={n} (shared workspace)')
        fresh = torch.zeros(lib.raw('mm_spd_pdist_ws_bytes')(dt, n, d), dtype=torch.uint8, device='cuda')
        o2, _ = run(x, g, fresh)
        assert torch.equal(out, o2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ MM_SPD_SHIFT=0
CHILD_SIZES = [65, 129, 200, 513]


def _plain_outputs():
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    res = {}
    for d in (2, 3, 4):
        for dname, dt in T.DT.items():
            for n in CHILD_SIZES:
                c = _case(n, d)
                x = c['x'].to(dt).cuda().requires_grad_()
                out = SPD(d).pdist(x, squared=True)
                gr, = torch.autograd.grad(out, x, c['g'].to(dt).cuda())
                res[f'd2/{d}/{dname}/{n}'] = out.detach().cpu().numpy()
                res[f'grad/{d}/{dname}/{n}'] = gr.cpu().numpy()
    return res


def test_switch_restores_the_plain_walk_in_a_fresh_child(tmp_path):
    """MM_SPD_SHIFT=0 (read once per process: a fresh child) launches the plain tiles.  At the reference initialisation every pair
    takes the close-pair series, so how pairs are grouped into wavefronts cannot change a value: d^2 is the same bit for bit,
    the gradient (float atomics, other order) within GRAD_TOL."""
    path = str(tmp_path / 'plain.npz')
    env = dict(os.environ, MM_SPD_SHIFT='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    ours = _plain_outputs()
    with np.load(path) as z:
        assert sorted(z.files) == sorted(ours)
        for k in z.files:
            if k.startswith('d2/'):
                assert np.array_equal(z[k], ours[k]), k
            else:
                dname = k.split('/')[2]
                T.check_rel(ours[k], z[k], T.GRAD_TOL[dname], k)


if __name__ == '__main__':
    import conftest  # noqa: F401  (the package and the oracle on sys.path)
    np.savez(sys.argv[1], **_plain_outputs())
