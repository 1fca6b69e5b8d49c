"""SPD pdist backward, row sums by lane groups (smallmat.hpp group_reduce_transposed; spd_pair.hpp: four LDS planes per wavefront,
added when a segment's row sums leave) against the fp64 port, through the C ABI, at the shapes where the layout can go wrong:
which lane group owns which columns (n around 64 and 128: one, two, three column blocks, ragged last block), segments shorter
than the 16 rows of a full one (row ranges of 15 and 17 rows, a range that holds one row, tiny n) and slices with an odd row
count, whose masked second slot writes a row of the planes that no atomic may pick up.

The reference is oracle/ref_port.py in float64 on the SAME points (the points are rounded to the tested dtype first, so the
bound holds the kernels alone).  Bounds: those of the backward parity tests of tests/test_spd_gpu.py for these dtypes — pdist
backward GRAD_TOL (fp32 2e-5, fp64 5e-6 of the largest entry of the gradient); fused objective: loss 2e-5, grad_x 2e-4,
d loss / d scale 1e-3 (fp32; test_fused_loss_vs_oracle_seeded)."""
import functools

import numpy as np
import pytest
import torch

from conftest import sym

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'f64': torch.float64}
GRAD_TOL = {'f32': 2e-5, 'f64': 5e-6}   # tests/test_spd_gpu.py
SIZES = [2, 3, 17, 63, 64, 65, 129, 130, 257]


def row_ranges(n):
    """(0, n), the middle third, the last row (no pair: a zero gradient), and ranges of 15 and of 17 rows where n allows."""
    out = [(0, n), (n // 3, 2 * n // 3), (n - 1, n)]
    for rows in (15, 17):
        if n > rows + 1:
            rb = (n - rows) // 2
            out.append((rb, rb + rows))
    return out


@functools.lru_cache(maxsize=None)
def points(d, n, dname):
    """Seeded points, rounded to the tested dtype, and the port's squared distances of them with their graph (float64, CPU)."""
    from oracle import ref_port as rp
    gen = torch.Generator().manual_seed(1000 * d + n)
    x64 = rp.SPD(d).rand(n, dtype=torch.float64, generator=gen).to(DT[dname]).double()
    x64 = 0.5 * (x64 + x64.transpose(1, 2))
    xr = x64.clone().requires_grad_()
    d2 = rp.SPD(d).pdist(xr, squared=True)
    g64 = torch.randn(n * (n - 1) // 2, dtype=torch.float64, generator=gen).to(DT[dname]).double()
    return x64, xr, d2, g64


def rel_err(got, ref):
    got = got.detach().double().cpu().numpy()
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('d,dname', [(2, 'f32'), (3, 'f32'), (4, 'f32'), (3, 'f64')])
def test_backward_of_row_ranges_vs_port(d, dname, n):
    from graphembed import _backend as B
    lib = B.lib()
    T = DT[dname]
    x64, xr, d2, g64 = points(d, n, dname)
    x = x64.to(T).cuda()
    dt = B.dtype_code(x)
    ws = torch.empty(lib.raw('mm_spd_pdist_ws_bytes')(dt, n, d), dtype=torch.uint8, device='cuda')
    for rb, re in row_ranges(n):
        lo, hi = B.pair_offset(n, rb), B.pair_offset(n, re)
        w = torch.zeros_like(g64)
        w[lo:hi] = g64[lo:hi]
        ref, = torch.autograd.grad((d2 * w).sum(), xr, retain_graph=True)
        g = g64[lo:hi].to(T).cuda()
        grad = torch.full_like(x, float('nan'))
        for launch in range(2):   # (the second launch of a walk starts from the share table the first one stored)
            with B.on_device(x.device):
                lib.call('mm_spd_pdist_bwd', dt, B.ptr(x), B.ptr(g), n, d, rb, re, 1, 1e-8, 1e8, B.ptr(grad), B.ptr(ws), 0,
                         B.stream_of(x))
            err = rel_err(grad, sym(ref.numpy()))
            print(f'd={d} {dname} n={n} rows=({rb},{re}) launch {launch}: {err:.3e}')
            assert err <= GRAD_TOL[dname], (d, dname, n, (rb, re), launch, err)
    torch.cuda.synchronize()


def _fused_objective_vs_port(loss_name, n, ranges, apart):
    """mm_spd_pdist_loss over `ranges` of the rows of n points against the port; `apart`: targets kept away from the distances."""
    from graphembed import _backend as B
    from graphembed.objectives import QuotientLoss, StressLoss
    lib = B.lib()
    d, dname, T = 3, 'f32', torch.float32
    fn, kw = {'stress': (StressLoss(), {}), 'quotient': (QuotientLoss(), dict(epoch=3, alpha=1.7))}[loss_name]
    kind, alpha, eps, terms = fn.fused_spec(**kw)[:4]
    x64, xr, d2, _ = points(d, n, dname)
    gen = torch.Generator().manual_seed(31 * n + len(loss_name))
    sr = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    md = torch.nn.functional.softplus(sr) * d2
    # targets of the size of the distances, kept away from the |.| kinks of the quotient terms (test_fused_loss_vs_oracle_seeded)
    u = torch.rand(md.shape, dtype=torch.float64, generator=gen)
    if apart:
        # ... and from the distances themselves, t / m in [0.5, 0.75] or [1.25, 1.5]: a range here can hold ONE pair, and the
        # relative error of a single stress term (m - t)^2 is that of the fp32 distance times 2 m / |m - t| (at most 8 with these
        # targets; the sums over thousands of pairs of the test these bounds come from average that factor out)
        side = torch.where(torch.rand(md.shape, dtype=torch.float64, generator=gen) < 0.5, -1.0, 1.0)
        tgt = (md.detach() * (1.0 + side * (0.25 + 0.25 * u))).clamp_min(1e-3).float().double()
    else:
        tgt = (md.detach() * (0.5 + u)).clamp_min(1e-3).float().double()   # t / m anywhere in [0.5, 1.5]: m ~ t included
    if kw:
        for _ in range(8):
            ag = tgt * kw['alpha']
            near = ((md.detach() / ag - 1).abs() < 0.05) | ((ag / (md.detach() + 1 / (kw['epoch'] + 1)) - 1).abs() < 0.05)
            tgt = torch.where(near, tgt * 1.25, tgt).float().double()
        assert not near.any()
    x = x64.to(T).cuda()
    s = torch.tensor([0.3], dtype=T, device='cuda')
    dt = B.dtype_code(x)
    ws = torch.empty(lib.raw('mm_spd_pdist_ws_bytes')(dt, n, d), dtype=torch.uint8, device='cuda')
    for rb, re in ranges:
        lo, hi = B.pair_offset(n, rb), B.pair_offset(n, re)
        if hi == lo:
            continue   # (no pair: nothing for an objective to sum; the empty range of the backward is covered above)
        ref = fn(tgt[lo:hi], md[lo:hi], **kw)
        ref_gx, ref_gs = torch.autograd.grad(ref, [xr, sr], retain_graph=True)
        t = tgt[lo:hi].to(T).cuda()
        out = torch.full((2,), float('nan'), dtype=T, device='cuda')
        grad = torch.full_like(x, float('nan'))
        with B.on_device(x.device):
            lib.call('mm_spd_pdist_loss', dt, B.LOSS_STRESS if kind == 'stress' else B.LOSS_QUOTIENT, B.ptr(x), B.ptr(t), B.ptr(s), n, d,
                     rb, re, alpha, eps, terms, None, 1e-8, 1e8, B.ptr(out), B.ptr(grad), B.ptr(ws), 0, B.stream_of(x))
        loss, gs = out.double().cpu().tolist()
        e_loss = abs(loss - ref.item()) / abs(ref.item())
        e_gx = rel_err(grad, sym(ref_gx.numpy()))
        e_gs = abs(gs - ref_gs.item()) / abs(ref_gs.item())
        print(f'{loss_name} n={n} rows=({rb},{re}): loss {e_loss:.3e} grad_x {e_gx:.3e} grad_scale {e_gs:.3e}')
        assert e_loss <= 2e-5, (n, (rb, re), loss, ref.item())
        assert e_gx <= 2e-4, (n, (rb, re), e_gx)
        assert e_gs <= 1e-3, (n, (rb, re), gs, ref_gs.item())
    torch.cuda.synchronize()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('loss_name', ['stress', 'quotient'])
def test_fused_objective_of_row_ranges_vs_port(loss_name, n):
    _fused_objective_vs_port(loss_name, n, row_ranges(n), apart=True)


@pytest.mark.parametrize('loss_name', ['stress', 'quotient'])
def test_fused_objective_with_targets_at_the_distances(loss_name):
    """The target distribution of test_fused_loss_vs_oracle_seeded itself (t / m uniform in [0.5, 1.5], pairs with m ~ t
    included), on the ranges of the largest size that hold thousands of pairs: 32 896 and 11 051."""
    n = SIZES[-1]
    _fused_objective_vs_port(loss_name, n, [(0, n), (n // 3, 2 * n // 3)], apart=False)
