"""SPD(3) pair kernels at the shapes where the quotient-ring logarithms (smallmat.hpp: log_series3, log_series3_centred,
log_cayley3 — written on adj(E) instead of E^2) and the forward's two row loops (interior wavefronts store without a mask,
spd_pair.hpp) can go wrong: n = 130 and n = 257 give one full block of 128 columns plus a ragged one, rows above a block and on
its diagonal, columns past n, and — in the forward — an interior and a diagonal wavefront in the same tile; the row shards have
first and last rows that are not tile-aligned, with even and odd row counts.  Distances and gradients against the fp64 checker
(oracle/exact.c) within the bounds of tests/test_spd_gpu.py, which are imported, not restated.

Which logarithm a wavefront row takes is decided by gates on A = L_i^-1 X_j L_i^-T.  That every rewritten form IS reached is
asserted from the inputs — the gates evaluated here in fp64, with a margin for the kernels' rounding — never from the kernel."""
import functools

import numpy as np
import pytest
import torch

import test_spd_gpu as T

pytestmark = pytest.mark.gpu

D = 3
BLOCK = 128   # columns of a wavefront row of the two-column kernels; a regime that holds on 128 columns holds on either half
# the kernels' gates (spd_pair.hpp kCloseGate; smallmat.hpp kCentredGate3, kCayleyGate)
CLOSE_GATE, CENTRED_GATE, CAYLEY_GATE = 0.09, 0.6534, 0.36
# spread -> the logarithm its far / close rows must reach, per dtype
EXPECT = {('close', 'f32'): 'series', ('close', 'f64'): 'series', ('mid', 'f32'): 'centred', ('mid', 'f64'): 'cayley',
          ('wide', 'f32'): 'cayley', ('wide', 'f64'): 'cayley'}
SHARDS = ['full', 'inner', 'tail']


def _shard(n, name):
    return {'full': (0, n), 'inner': (3, 77), 'tail': (n - 5, n)}[name]


def _points(n, spread, gen):
    from oracle import ref_port as rp
    if spread == 'wide':   # the wide generator of test_fused_loss_vs_oracle_seeded
        a = torch.rand(n, D, D, dtype=torch.float64, generator=gen)
        return a @ a.transpose(1, 2) + torch.eye(D, dtype=torch.float64)
    port = rp.SPD(D)
    s = {'close': 0.1, 'mid': 0.35}[spread]
    scale = s * (0.6 + 0.4 * torch.rand(n, generator=gen))   # the generator of _series_regime
    u = torch.randn(n, D * (D + 1) // 2, dtype=torch.float64, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True) * scale.double().reshape(n, 1)
    return port.exp(port.zero(n, dtype=torch.float64), port.from_vec(u))


def _regime_rows(x64):
    """Number of whole wavefront rows (row i, block of 128 columns with a pair above the diagonal) per regime, from the
    generalised eigenvalues in fp64.  A row's gate sees every lane of the block: columns at or below the diagonal are real
    points, columns past n the identity.  Margins of 10 % keep the count independent of the kernels' rounding."""
    n = x64.shape[0]
    nb = (n + BLOCK - 1) // BLOCK
    li = torch.linalg.inv(torch.linalg.cholesky(x64))
    cols = torch.cat([x64, torch.eye(D, dtype=torch.float64).expand(nb * BLOCK - n, D, D)])
    a = li[:, None] @ cols[None] @ li[:, None].transpose(-1, -2)
    w = torch.linalg.eigvalsh(0.5 * (a + a.transpose(-1, -2)))            # [n, nb * BLOCK, 3]
    close = ((w - 1) ** 2).sum(-1)
    m = w.mean(-1)
    centred = ((w - m[..., None]) ** 2).sum(-1) / (m * m)
    mant, k = torch.frexp(m)
    mu = torch.ldexp(torch.ones_like(m), torch.where(mant < 0.70710678118654752, k - 1, k))
    cayley = (((w - mu[..., None]) / (w + mu[..., None])) ** 2).sum(-1)
    count = {'series': 0, 'centred': 0, 'cayley': 0, 'cayley64': 0}
    for b in range(nb):
        sl = slice(b * BLOCK, (b + 1) * BLOCK)
        rows = min((b + 1) * BLOCK, n) - 1                                 # rows with a column of this block above them
        cl, ce, ca = close[:rows, sl], centred[:rows, sl], cayley[:rows, sl]
        series = (cl <= 0.9 * CLOSE_GATE).all(-1)
        far = (cl > 1.1 * CLOSE_GATE).any(-1)
        cen = far & (ce <= 0.9 * CENTRED_GATE).all(-1)
        cay = far & (ce > 1.1 * CENTRED_GATE).any(-1) & (ca <= 0.9 * CAYLEY_GATE).all(-1)
        cay64 = far & (ca <= 0.9 * CAYLEY_GATE).all(-1)                    # fp64 has no recentred series: far rows go to Cayley
        count['series'] += int(series.sum())
        count['centred'] += int(cen.sum())
        count['cayley'] += int(cay.sum())
        count['cayley64'] += int(cay64.sum())
    return count


@functools.lru_cache(maxsize=None)
def _case(n, dname, spread):
    """Inputs (rounded to the kernel's precision), upstream gradient and the checker's d^2: computed once, shared, read-only."""
    from oracle import exact
    gen = torch.Generator().manual_seed(1000 * n + 10 * len(spread) + len(dname))
    x = _points(n, spread, gen).to(T.DT[dname])
    g = torch.randn(n * (n - 1) // 2, dtype=torch.float64, generator=gen).to(T.DT[dname])
    xin = x.double().numpy()
    want = EXPECT[spread, dname]
    count = _regime_rows(x.double())
    reached = count['cayley64'] if (want, dname) == ('cayley', 'f64') else count[want]
    assert reached >= 1, f'n={n} {dname} {spread}: no whole wavefront row in the {want} regime ({count})'
    return x, g, xin, exact.spd_pdist(xin)


def _check(n, dname, spread, shard, squared):
    from graphembed import _backend as B
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    from oracle import exact
    x, g, xin, ref_d2 = _case(n, dname, spread)
    rb, re = _shard(n, shard)
    lo, hi = B.pair_offset(n, rb), B.pair_offset(n, re)
    xr = x.cuda().requires_grad_()
    out = SPD(D).pdist(xr, squared=squared, rows=(rb, re))
    assert out.numel() == hi - lo
    what = f'n={n} {dname} {spread} rows=({rb},{re}) squared={squared}'
    T.check_d2(out if squared else out * out, ref_d2[lo:hi], dname, 'd2 ' + what)
    gr, = torch.autograd.grad(out, xr, g[lo:hi].cuda())
    gfull = np.zeros(n * (n - 1) // 2)
    gfull[lo:hi] = g[lo:hi].double().numpy()
    ref_g = exact.spd_pdist_grad(xin, gfull, squared=squared)
    T.check_rel(gr, ref_g, T.GRAD_TOL[dname] * (1 if squared else 5), 'grad ' + what)   # (d: as test_pdist_vs_reference_golden)


@pytest.mark.parametrize('shard', SHARDS)
@pytest.mark.parametrize('spread', ['close', 'mid', 'wide'])
@pytest.mark.parametrize('dname', list(T.DT))
@pytest.mark.parametrize('n', [130, 257])
def test_ring_forms_vs_checker(n, dname, spread, shard):
    _check(n, dname, spread, shard, True)


@pytest.mark.parametrize('dname', list(T.DT))
def test_ring_forms_distance_not_squared(dname):
    _check(130, dname, 'close', 'inner', False)


@pytest.mark.parametrize('loss_name', ['stress', 'quotient'])
@pytest.mark.parametrize('dname', list(T.DT))
def test_ring_forms_in_the_fused_loss_kernels(dname, loss_name):
    """The fused-objective instantiations of the backward share log_series3 / log_cayley3: the existing check (close and wide
    points, its own bounds) at n = 130."""
    T.test_fused_loss_vs_oracle_seeded(D, 130, dname, loss_name)
