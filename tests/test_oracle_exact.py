"""Pins the plain-C fp64 checker (oracle/exact.c) against the reference-faithful port in fp64,
which is itself pinned against the reference's golden vectors.  CPU only."""
import numpy as np
import pytest
import torch

from conftest import load_golden, sym
from oracle import exact
from oracle import ref_port as rp


@pytest.mark.parametrize('d', [2, 3, 4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize('init', ['rand', 'wide'])
def test_spd_against_reference_golden(d, init):
    G = load_golden(f'spd{d}')
    tag = f'f64/{init}/n33'
    x, g = G[f'{tag}/x'], G[f'{tag}/g']
    # the reference's eps-fudged closed forms (d = 2, 3) bias its fp64 results by up to ~1e-6
    tol = 2e-6 if d <= 3 else 1e-9
    for sq, key in ((True, 'd2'), (False, 'd1')):
        out = exact.spd_pdist(x, squared=sq)
        np.testing.assert_allclose(out * out if not sq else out, G[f'{tag}/{key}'] ** (1 if sq else 2), rtol=tol, atol=1e-7 if d <= 3 else 1e-12)
    gr = exact.spd_pdist_grad(x, g, squared=True)
    ref = sym(G[f'{tag}/grad_d2'])
    assert np.abs(gr - ref).max() <= (5e-6 if d <= 3 else 1e-9) * np.abs(ref).max()
    assert np.abs(gr - np.swapaxes(gr, 1, 2)).max() <= 1e-12 * np.abs(gr).max()


@pytest.mark.parametrize('key,kind,m', [('lorentz11', 'lorentz', 11), ('sphere6', 'sphere', 6), ('euclidean10', 'euclidean', 10),
                                          ('lorentz48', 'lorentz', 48), ('sphere64', 'sphere', 64), ('euclidean40', 'euclidean', 40)])
@pytest.mark.parametrize('init', ['rand', 'wide'])
def test_vec_against_reference_golden(key, kind, m, init):
    G = load_golden(key)
    tag = f'f64/{init}/n33'
    x, g = G[f'{tag}/x'], G[f'{tag}/g']
    np.testing.assert_allclose(exact.vec_pdist(kind, x, True), G[f'{tag}/d2'], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(exact.vec_pdist(kind, x, False), G[f'{tag}/d1'], rtol=1e-9, atol=1e-13)
    for sq, gk in ((True, 'grad_d2'), (False, 'grad_d1')):
        gr = exact.vec_pdist_grad(kind, x, g, sq)
        assert np.abs(gr - G[f'{tag}/{gk}']).max() <= 1e-8 * np.abs(G[f'{tag}/{gk}']).max()


def test_spd4_against_port_seeded():
    gen = torch.Generator().manual_seed(0)
    port = rp.SPD(4)
    x = port.rand(150, ir=1.0, dtype=torch.float64, generator=gen)
    g = torch.randn(150 * 149 // 2, dtype=torch.float64, generator=gen)
    xr = x.clone().requires_grad_()
    d2 = port.pdist(xr, squared=True)
    gr, = torch.autograd.grad((d2 * g).sum(), xr)
    np.testing.assert_allclose(exact.spd_pdist(x.numpy()), d2.detach().numpy(), rtol=1e-10, atol=1e-13)
    ref = sym(gr.numpy())
    assert np.abs(exact.spd_pdist_grad(x.numpy(), g.numpy()) - ref).max() <= 1e-9 * np.abs(ref).max()
    with pytest.raises(np.linalg.LinAlgError):
        exact.spd_pdist(-np.eye(3)[None].repeat(3, 0))


def _pair_subsets(n, gen):
    """Every pair, a random subset (with repeats, in random order) and the empty list."""
    iu = np.triu_indices(n, 1)
    k = gen.integers(0, iu[0].size, size=3 * n)
    return [(iu[0], iu[1]), (iu[0][k], iu[1][k]), (iu[0][:0], iu[1][:0])]


def _grad_over_subset(full_grad_fn, n, lo, hi, gk):
    """The whole-pdist gradient with g zero outside the list (repeated pairs add up): what the pair-list gradient must equal."""
    g = np.zeros(n * (n - 1) // 2)
    np.add.at(g, exact.pair_index(n, lo, hi), gk)
    return full_grad_fn(g)


@pytest.mark.parametrize('d', [2, 3, 4, 6, 9])
@pytest.mark.parametrize('squared', [True, False])
def test_spd_pair_lists_match_pdist(d, squared):
    gen = np.random.default_rng(10 * d + squared)
    n = 41
    x = rp.SPD(d).rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(d)).numpy()
    full = exact.spd_pdist(x, squared=squared)
    for lo, hi in _pair_subsets(n, gen):
        k = exact.pair_index(n, lo, hi)
        out = exact.spd_pairs(x, lo, hi, squared=squared)
        np.testing.assert_allclose(out, full[k], rtol=1e-13, atol=1e-15)
        gk = gen.standard_normal(lo.size)
        ref = _grad_over_subset(lambda g: exact.spd_pdist_grad(x, g, squared=squared), n, lo, hi, gk)
        got = exact.spd_pairs_grad(x, lo, hi, gk, squared=squared)
        scale = max(np.abs(ref).max(), 1e-300)
        assert np.abs(got - ref).max() <= 1e-12 * scale
        untouched = np.setdiff1d(np.arange(n), np.concatenate([lo, hi]))
        assert (got[untouched] == 0).all()


@pytest.mark.parametrize('kind,m', [('lorentz', 11), ('sphere', 2), ('sphere', 64), ('euclidean', 11)])
@pytest.mark.parametrize('squared', [True, False])
def test_vec_pair_lists_match_pdist(kind, m, squared):
    gen = np.random.default_rng(m + squared)
    n = 53
    x = gen.standard_normal((n, m))
    if kind == 'sphere':
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    elif kind == 'lorentz':
        x[:, 0] = np.sqrt(1 + (x[:, 1:] ** 2).sum(1))
    full = exact.vec_pdist(kind, x, squared)
    for lo, hi in _pair_subsets(n, gen):
        k = exact.pair_index(n, lo, hi)
        np.testing.assert_allclose(exact.vec_pairs(kind, x, lo, hi, squared), full[k], rtol=1e-14, atol=0)
        gk = gen.standard_normal(lo.size)
        ref = _grad_over_subset(lambda g: exact.vec_pdist_grad(kind, x, g, squared), n, lo, hi, gk)
        got = exact.vec_pairs_grad(kind, x, lo, hi, gk, squared)
        assert np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)


def test_pair_index_round_trip_at_large_n():
    """pair_index / pair_of_index (the large-n tests' sampling arithmetic) are exact inverses, at the row boundaries and
    around 2^31 and 2^32 / 4 of the largest sizes the GPU tests address."""
    for n in (2, 3, 65600, 70000, 1 << 22, 1 << 24):
        total = n * (n - 1) // 2
        ks = {0, total - 1, total // 2}
        for c in (2 ** 31, 2 ** 30, 2 ** 29):
            ks.update(v for v in (c - 1, c, c + 1) if 0 <= v < total)
        rows = np.array([0, 1, n // 2, n - 2])
        rows = rows[(rows >= 0) & (rows <= n - 2)]
        for r in rows:
            ks.update({int(exact.pair_index(n, r, r + 1)), int(exact.pair_index(n, r, n - 1))})
        k = np.array(sorted(ks), dtype=np.int64)
        lo, hi = exact.pair_of_index(n, k)
        assert ((lo >= 0) & (lo < hi) & (hi < n)).all(), n
        assert (exact.pair_index(n, lo, hi) == k).all(), n


def test_pair_lists_refuse_bad_pairs():
    x = np.eye(3)[None].repeat(4, 0)
    for lo, hi in (([1], [1]), ([2], [1]), ([0], [4]), ([-1], [2])):
        with pytest.raises(ValueError):
            exact.spd_pairs(x, lo, hi)
    with pytest.raises(np.linalg.LinAlgError):
        exact.spd_pairs(-np.eye(3)[None].repeat(3, 0), [0], [1])
