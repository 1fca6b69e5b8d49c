"""CPU-only checks of the Stein-divergence fused objective and node-minibatch entry points (csrc/spd_stein_loss.hpp): the
quotient targets of tests/stein_cases.py keep their margin from the kinks, the oracle against the recorded reference vectors and its
grad_scale against a central difference, the four entries declared / exported / in the signature table, argument errors returned
before anything touches a GPU, the Python hooks, and the registers of the new kernels in the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import stein_cases as C
from graphembed import _backend as B

NEW = ('mm_spd_stein_pdiv_loss', 'mm_spd_stein_pdiv_loss_subset', 'mm_spd_stein_pdiv_fwd_subset', 'mm_spd_stein_pdiv_bwd_subset')


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', C.DIMS)
@pytest.mark.parametrize('regime', C.REGIMES)
def test_no_pair_sits_on_a_kink_of_the_quotient_loss(regime, d):
    """a sign flip of a pair's term cannot pass for rounding: every pair of every case is at least MARGIN away from both kinks"""
    for n in C.SIZES:
        m = C.kink_margin(regime, n, d)
        assert m >= C.MARGIN, (regime, n, d, m)
        t = C.targets(regime, n, d)
        assert t.numel() == n * (n - 1) // 2 and torch.equal(t, t.float().double())
    for bs in C.BATCHES:
        m = C.batch_kink_margin(regime, d, bs)
        assert m >= C.MARGIN, (regime, d, bs, m)
        idx = C.batch_idx(bs)
        assert 0 in idx.tolist() and C.N_TOTAL - 1 in idx.tolist() and (bs < 3 or bool((idx[1:] < idx[:-1]).any()))
        dm = C.dense(regime, d, bs)
        assert dm.dtype == torch.float32 and not torch.equal(dm, dm.T)
    x = C.points(regime, C.N_TOTAL, d)
    assert torch.equal(x, x.transpose(1, 2)) and float(torch.linalg.eigvalsh(x).min()) > 0.5


def test_targets_have_the_magnitude_of_the_divergences():
    for regime in C.REGIMES:
        md = C.model_dists(C.points(regime, 65, 3))
        t = C.targets(regime, 65, 3)
        assert 0.4 * float(md.median()) <= float(t.min()) and float(t.max()) <= 3.6 * 1.01**8 * float(md.median())
    assert float(C.model_dists(C.points('init', 65, 3)).median()) < 1e-2 < float(C.model_dists(C.points('spread', 65, 3)).median())


def test_the_clamp_binds_on_the_coincident_pair():
    x = C.coincident_points()
    v = C.ref.SPD(3, wmin=C.WMIN).stein_pdiv(x, squared=True)
    k = B.pair_offset(65, 7) + 40 - 7 - 1
    assert float(v[k]) == C.WMIN and float(v.min()) == C.WMIN and int((v == C.WMIN).sum()) == 1


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', (2, 3, 4))
def test_oracle_against_the_recorded_reference_vectors(d):
    """values and gradients of stein_pdiv as the reference computed them (tests/golden/gen_golden_stein.py), fp64 vectors; the
    tolerances are those tests/test_spd_gpu.py holds the fp64 kernels to against the same vectors"""
    G = load_golden('stein')
    port = C.ref.SPD(d)
    for init in ('rand', 'wide'):
        for n in (33, 70):
            tag = f'spd{d}/f64/{init}/n{n}'
            x = torch.from_numpy(np.asarray(G[f'{tag}/x'], dtype=np.float64)).requires_grad_()
            g = torch.from_numpy(np.asarray(G[f'{tag}/g'], dtype=np.float64))
            v = port.stein_pdiv(x, squared=True)
            want = np.asarray(G[f'{tag}/div_sq'], dtype=np.float64)
            assert (np.abs(v.detach().numpy() - want) <= 1e-9 + 1e-7 * np.abs(want)).all(), tag
            gx, = torch.autograd.grad((v * g).sum(), x)
            gw = np.asarray(G[f'{tag}/grad_sq'], dtype=np.float64)
            gw = 0.5 * (gw + gw.transpose(0, 2, 1))
            gs = 0.5 * (gx + gx.transpose(1, 2)).numpy()
            assert np.abs(gs - gw).max() <= 5e-7 * np.abs(gw).max(), tag


@pytest.mark.parametrize('loss_name', C.LOSSES)
def test_oracle_grad_scale_against_a_central_difference(loss_name):
    x, tg = C.points('spread', 33, 3), C.targets('spread', 33, 3)
    _, _, gs = C.objective_of(x, tg, loss_name)
    h = 1e-6
    up = C.objective_of(x, tg, loss_name, scale_raw=C.SCALE_RAW + h)[0]
    dn = C.objective_of(x, tg, loss_name, scale_raw=C.SCALE_RAW - h)[0]
    fd = float(up - dn) / (2 * h)
    assert abs(fd - float(gs)) <= 1e-6 * abs(float(gs)), (fd, float(gs))
    # ... and the batch form scatters into zeros
    idx = C.batch_idx(65)
    _, gx, _ = C.batch_oracle('spread', 3, 65, loss_name)
    outside = torch.ones(C.N_TOTAL, dtype=torch.bool)
    outside[idx] = False
    assert float(gx[outside].abs().max()) == 0.0 and float(gx[idx].abs().amax(dim=(1, 2)).min()) > 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert B.lib().raw('mm_abi_version')() == 4


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    loss, sub, fwd, bwd = (lib.raw(k) for k in NEW)
    BIG = 1 << 22
    ARG, UNS = -1, -2

    def lo(x=q, target=q, scale=q, n=20, d=3, rb=0, re=20, terms=3, out=q, grad=q, ws=q, kind=B.LOSS_STRESS, dtype=B.MM_F32):
        return loss(dtype, kind, x, target, scale, n, d, rb, re, 1.0, 1.0, terms, None, 1e-8, out, grad, ws, 0, None)

    def ls(x=q, dense=q, n=20, d=3, idx=q, bs=10, rb=0, re=10, terms=3, out=q, grad=q, ws=q, kind=B.LOSS_STRESS, dtype=B.MM_F32):
        return sub(dtype, kind, x, dense, q, n, d, idx, bs, rb, re, 1.0, 1.0, terms, None, 1e-8, out, grad, ws, 0, None)

    def f(x=q, n=20, d=3, idx=q, bs=10, rb=0, re=10, out=q, ws=q, dtype=B.MM_F32):
        return fwd(dtype, x, n, d, idx, bs, rb, re, 1, 1e-8, out, ws, 0, None)

    def b(x=q, g=q, n=20, d=3, idx=q, bs=10, rb=0, re=10, grad=q, ws=q, dtype=B.MM_F32):
        return bwd(dtype, x, g, n, d, idx, bs, rb, re, 1, 1e-8, grad, ws, 0, None)

    # null pointers; target / dense / idx / g / out only when there are pairs
    assert lo(x=None) == ARG and lo(out=None) == ARG and lo(grad=None) == ARG and lo(ws=None) == ARG and lo(target=None) == ARG
    assert ls(x=None) == ARG and ls(out=None) == ARG and ls(grad=None) == ARG and ls(ws=None) == ARG
    assert ls(dense=None) == ARG and ls(idx=None) == ARG
    assert f(x=None) == ARG and f(ws=None) == ARG and f(out=None) == ARG and f(idx=None) == ARG
    assert b(x=None) == ARG and b(ws=None) == ARG and b(grad=None) == ARG and b(g=None) == ARG and b(idx=None) == ARG
    assert ls(grad=None, bs=1, re=1) == ARG and b(grad=None, bs=0, re=0) == ARG   # (the outputs are written without pairs too)
    # counts and row ranges
    assert lo(n=-1, re=0) == ARG and lo(rb=5, re=4) == ARG and lo(re=21) == ARG and lo(rb=-1) == ARG and lo(n=BIG + 1, re=3) == ARG
    for call in (ls, f, b):
        assert call(bs=-1, re=0) == ARG and call(n=-3) == ARG and call(bs=21, re=21) == ARG      # bs > n_total
        assert call(rb=5, re=4) == ARG and call(re=11) == ARG and call(rb=-1) == ARG
        assert call(n=BIG + 1) == ARG and call(dtype=5) == ARG
    assert lo(dtype=5) == ARG
    # the loss
    for call in (lo, ls):
        assert call(kind=B.LOSS_QUOTIENT, terms=0) == ARG and call(kind=B.LOSS_QUOTIENT, terms=4) == ARG
        assert call(kind=B.LOSS_NONE) == UNS and call(kind=99) == UNS
    # sizes outside 2 ... mm_spd_max_dim()
    dmax = lib.raw('mm_spd_max_dim')()
    for call in (lo, ls, f, b):
        for d in (0, 1, dmax + 1, -2):
            assert call(d=d) == UNS, d
    with pytest.raises(B.BackendError):
        lib.call('mm_spd_stein_pdiv_loss', B.MM_F32, B.LOSS_STRESS, None, q, q, 20, 3, 0, 20, 1.0, 1.0, 3, None, 1e-8, q, q, q, 0, None)


# ---- Python ---------------------------------------------------------------------------------------------------------------------
def test_the_hooks_sit_on_stein_manifolds_only_and_decline_cpu_tensors():
    import graphembed.manifolds as M
    plain, stein = M.SymmetricPositiveDefinite(3), M.SymmetricPositiveDefinite(3, use_stein_div=True)
    assert getattr(plain, 'pdist_loss_subset', None) is None and getattr(plain, 'pdist_subset', None) is None
    assert 'pdist_loss' not in vars(plain) and plain.pdist_loss.__func__ is M.SymmetricPositiveDefinite.pdist_loss
    for name in ('pdist_loss', 'pdist_loss_subset', 'pdist_subset'):
        assert callable(vars(stein)[name]), name
    narrow = M.SymmetricPositiveDefinite(2, use_stein_div=True, wmin=1e-4, wmax=1e4)   # the hooks do not depend on the window
    assert not narrow.clamps_wide and callable(narrow.pdist_loss) and callable(narrow.pdist_subset)
    x = torch.eye(3).repeat(5, 1, 1)
    dense, idx = torch.rand(5, 5), torch.tensor([4, 0, 2])
    assert stein.pdist_loss_subset(x, torch.tensor(0.3), idx, dense, ('stress', 1.0, 1.0, 3)) is None   # the caller gathers
    assert stein.pdist_subset(x, idx) is None and stein.pdist_subset(x, idx, squared=True, rows=(0, 1), cache={}) is None
    with pytest.raises(Exception):
        stein.pdist_loss(x, None, torch.rand(10), ('stress', 1.0, 1.0, 3))   # no quiet CPU fall-back


# ---- registers ------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_spill_only_where_the_backward_does():
    """no scratch anywhere; no spilled register wherever spd_stein_bwd_kernel<T, D, 8> of the same (T, D) has none; at most a
    dozen vector registers and the 64 bytes of the loss staging beside the backward they are modelled on"""
    if not os.path.isfile(os.path.join(ROOT, 'matrix-manifolds_amd', 'lib', 'libmm_manifolds.so')):
        pytest.skip('the library is not built')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernels()
    dmax = B.lib().raw('mm_spd_max_dim')()
    forms = ('0, true', '1, false', '1, true', '2, false', '2, true')
    count = 0
    for T in ('float', 'double'):
        for d in range(2, dmax + 1):
            base = meta[f'spd_stein_bwd_kernel<{T}, {d}, 8>']
            clean = base['vgpr_spill'] == 0 and base['sgpr_spill'] == 0 and base['scratch'] == 0
            pair = [f'spd_stein_pair_kernel<{T}, {d}, 8, {form}>' for form in forms]
            for nm in pair + [f'spd_stein_fwd_subset_kernel<{T}, {d}, 8>', f'spd_stein_loss_finalize_kernel<{T}, {d}>']:
                k = meta[nm]
                count += 1
                assert k['scratch'] == 0, (nm, k)
                if clean:
                    assert k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
            for nm in pair:
                assert meta[nm]['vgpr'] <= base['vgpr'] + 12 and meta[nm]['lds'] <= base['lds'] + 64, (nm, meta[nm], base)
    assert count == 2 * (dmax - 1) * 7
