"""CPU-only checks of the spanning-tree KL objective: the long-double oracle of tests/sst_cases.py against the recorded
reference and its own identities, the two exclusive gradient conventions told apart, the torch-op form of StochasticTreeLoss
against the oracle, and the host side of the new entry points (declared, exported, workspace size, argument errors before
anything touches a GPU, register / scratch budget).

Measured (largest e / bound over the case list): oracle against the fp64 reference 0.85 for the loss (n = 2, where the bound is
2.6e-16) and 0.32 for the gradient; torch-op form under the tolerance rule, loss | gradient: near 0.02 | 0.41 (f32), 0.04 | 0.41
(f64); mid 0.03 | 0.19, 0.05 | 0.33; grid 0.02 | 0.10, 0.01 | 0.12; offset 0.00 | 0.10, 0.00 | 0.06."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import sst_cases as S
from graphembed import _backend as B
from graphembed.objectives import StochasticTreeLoss

NEW = ('mm_sst_kl_ws_bytes', 'mm_sst_kl_loss')
LIMIT = 4096
LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
CASE_IDS = [f'n{n}-{r}' for n, r in S.CASES]
DT = {'f32': torch.float32, 'f64': torch.float64}


@pytest.mark.parametrize('n,regime', S.CASES, ids=CASE_IDS)
def test_oracle_matches_the_recorded_fp64_reference(n, regime):
    """Within n eps64 kappa scale, kappa = |L|_1 |G|_1 of the oracle's own matrices: the backward-error bound of a Cholesky
    solve.  The reference's exclusive gradient is the oracle's 'ref' form.  n = 2: the oracle's inclusive gradient is exactly 0
    (scale 0) where the reference has the rounding of mu_x - mu_z = 1 - 1; it is held to 4 eps64 there."""
    rec = S.recorded(n, regime)
    for key, mode in (('incl', 'incl'), ('excl', 'ref')):
        o = S.oracle(n, regime, mode)
        assert np.isfinite(rec[f'{key}/grad_f64']).all()
        for what in ('loss', 'grad'):
            bound = n * S.EPS['f64'] * o['kappa'] * S.scale_of(o, what)
            if n == 2 and what == 'grad' and mode == 'incl':
                bound = 4 * S.EPS['f64']
            e = S.deviation(rec[f'{key}/{what}_f64'], o[what])
            print(f'n{n}/{regime}/{mode} {what}: e {e:.3e} bound {bound:.3e} kappa {o["kappa"]:.3e}')
            assert e <= bound, (mode, what, e, bound)


def test_case_list_and_inputs_follow_the_stated_rule():
    assert len(S.CASES) == 15 * 2 + 3 * 2
    assert {31, 32, 33, 65} <= {n - 1 for n in S.NS}   # around the panel width and the GEMM tile, and two panels + 1
    for n, regime in S.CASES:
        g, m = S.inputs(n, regime)
        g2, m2 = S.make_inputs(n, regime)
        assert g.dtype == np.float64 and m.dtype == np.float32 and len(g) == len(m) == n * (n - 1) // 2
        assert np.array_equal(g, g2) and np.array_equal(m, m2)
        assert set(np.round(np.sqrt(g * 36)).astype(int)) <= set(range(1, 7))
        if regime in ('grid', 'offset'):
            assert np.array_equal(m * 1024, np.round(m * 1024))
    for n in S.TWIN_NS:
        assert np.array_equal(S.inputs(n, 'offset')[1].astype(np.float64), S.inputs(n, 'grid')[1].astype(np.float64) + S.OFFSET)
        rec = S.recorded(n, 'offset')
        assert 'incl/loss_f64' in rec and 'incl/loss_f32' not in rec     # the fp32 reference cannot evaluate it
    for name in {S.shard_of(n, r) for n, r in S.CASES}:
        assert os.path.getsize(os.path.join(S.GOLDEN, name + '.npz')) < (1 << 20), name


@pytest.mark.parametrize('n,regime', S.CASES, ids=CASE_IDS)
def test_identities_of_the_oracle(n, regime):
    for mode in S.MODES:
        o = S.oracle(n, regime, mode)
        assert abs(float(o['mu'].sum()) - (n - 1)) <= 64 * n * float(np.finfo(S.L).eps) * o['kappa']
        if n == 2:   # one pair: the single tree has probability 1 under both models
            assert float(o['loss']) == 0.0
            if mode != 'ref':
                assert float(o['grad'][0]) == 0.0
            else:    # the reference's form keeps mu delta = theta_z - theta_x
                g, m = S.inputs(n, regime)
                assert abs(float(o['grad'][0]) - (float(m[0]) - S.ALPHA * float(g[0]))) <= 1e-15


@pytest.mark.parametrize('n', S.TWIN_NS)
def test_offset_twins_are_equal(n):
    """A constant added to every m changes neither the loss nor the inclusive and exact exclusive gradients; the reference-form
    gradient mu delta moves by the constant times mu."""
    for mode in S.MODES:
        a, b = S.oracle(n, 'grid', mode), S.oracle(n, 'offset', mode)
        tiny = 64 * n * float(np.finfo(S.L).eps) * a['kappa']
        assert abs(float(a['loss'] - b['loss'])) <= tiny * S.OFFSET * n, mode
        assert S.deviation(a['mu'], b['mu']) <= tiny
        shift = S.OFFSET * a['mu'] if mode == 'ref' else 0
        assert S.deviation(b['grad'], a['grad'] + shift) <= tiny * S.OFFSET, mode


@pytest.mark.parametrize('n,regime', [c for c in S.CASES if c[0] > 2], ids=[i for i, c in zip(CASE_IDS, S.CASES) if c[0] > 2])
def test_the_two_exclusive_gradients_cannot_be_swapped(n, regime):
    ref, exact = S.oracle(n, regime, 'ref'), S.oracle(n, regime, 'excl')
    g, m = S.inputs(n, regime)
    delta = -S.L(S.ALPHA) * g.astype(S.L) + m.astype(S.L)      # theta_z - theta_x of the exclusive loss
    assert S.deviation(ref['grad'], ref['mu'] * delta) == 0.0
    gap = S.deviation(ref['grad'], exact['grad'])
    bound = max(S.bound_of(n, regime, mode, 'f32', 'grad')[0] for mode in ('ref', 'excl'))
    print(f'n{n}/{regime}: gap {gap:.3e} bound {bound:.3e}')
    assert gap > 10 * bound


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('n,regime', S.CASES, ids=CASE_IDS)
def test_torch_op_form_holds_the_tolerance_rule(n, regime, dname):
    g, m = S.inputs(n, regime)
    failures = []
    for mode in S.MODES:
        fn = StochasticTreeLoss(inclusive=mode == 'incl', exact_gradient=mode == 'excl')
        mt = torch.from_numpy(m).to(DT[dname]).requires_grad_()
        loss = fn(torch.from_numpy(g).to(DT[dname]), mt, alpha=S.ALPHA)
        gr, = torch.autograd.grad(loss, mt)
        assert loss.dtype == DT[dname] and gr.shape == mt.shape
        S.check(n, regime, mode, dname, 'loss', loss.detach().numpy(), failures)
        S.check(n, regime, mode, dname, 'grad', gr.numpy(), failures)
    S.print_ratios()
    assert not failures, '\n'.join(failures)


def test_exact_gradient_flag_changes_nothing_for_the_inclusive_loss():
    g, m = S.inputs(17, 'mid')
    out = []
    for exact in (False, True):
        mt = torch.from_numpy(m).double().requires_grad_()
        loss = StochasticTreeLoss(inclusive=True, exact_gradient=exact)(torch.from_numpy(g), mt, alpha=S.ALPHA)
        out.append((float(loss.detach()), torch.autograd.grad(loss, mt)[0]))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


def test_small_sizes_and_the_interface_of_the_class():
    for dt in (torch.float32, torch.float64):
        for inclusive, exact in ((True, False), (False, True)):
            m = torch.tensor([2.7], dtype=dt, requires_grad=True)
            loss = StochasticTreeLoss(inclusive=inclusive, exact_gradient=exact)(torch.tensor([3.0], dtype=dt), m, alpha=S.ALPHA)
            gr, = torch.autograd.grad(loss, m)
            assert float(loss.detach()) == 0.0 and float(gr) == 0.0
    fn = StochasticTreeLoss()
    assert float(fn(torch.ones(0), torch.ones(0), alpha=1.0)) == 0.0   # one node, no pair
    for bad in (2, 4, 5, 7, 2079):
        with pytest.raises(ValueError):
            fn(torch.ones(bad), torch.ones(bad), alpha=1.0)
    with pytest.raises(ValueError):
        fn(torch.ones(3), torch.ones(6), alpha=1.0)
    assert str(fn) == 'kl_loss' and not hasattr(fn, 'fused_spec')
    assert (fn.inclusive, fn.native, fn.exact_gradient) == (True, True, False)


def test_a_disconnected_graph_gives_a_non_finite_loss_in_the_torch_op_form():
    n = 9
    g, m = S.make_inputs(n, 'mid')
    i, j = np.triu_indices(n, 1)
    m = m.copy()
    m[(i == 4) | (j == 4)] = np.inf
    mt = torch.from_numpy(m).double().requires_grad_()
    loss = StochasticTreeLoss(inclusive=True)(torch.from_numpy(g), mt, alpha=S.ALPHA)
    assert not bool(torch.isfinite(loss))


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', plain))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert declared == set(B.SIGNATURES)
    assert re.search(r'MM_SST_INCLUSIVE\s*=\s*0\s*,\s*MM_SST_EXCLUSIVE\s*=\s*1\s*,\s*MM_SST_EXCLUSIVE_REFERENCE\s*=\s*2', plain)
    assert (B.SST_INCLUSIVE, B.SST_EXCLUSIVE, B.SST_EXCLUSIVE_REFERENCE) == (0, 1, 2)
    assert B.SIGNATURES['mm_sst_kl_loss'] == B.SIGNATURES['mm_sne_kl_loss']
    assert B.lib().raw('mm_abi_version')() == 4


@pytest.mark.parametrize('dtype,size', [(B.MM_F32, 4), (B.MM_F64, 8)])
def test_workspace_is_monotone_and_covers_the_matrices(dtype, size):
    ws = B.lib().raw('mm_sst_kl_ws_bytes')
    last = 0
    for n in (0, 1, 2, 3, 32, 33, 34, 65, 66, 257, 1025, LIMIT):
        b = ws(dtype, n)
        if n >= 2:   # L / factor / G and W / Z of both models, M of one; partial maxima, log-pivot sums, row sums
            assert b >= size * 5 * (n - 1) ** 2 + size * 512 + 8 * (2 * ((n + 30) // 32) + n - 1), (n, b)
            assert b <= 1.01 * size * 5 * (n - 1) ** 2 + 16384, (n, b)
        assert b >= last, n
        last = b
    assert ws(dtype, -1) == 0 and ws(dtype, LIMIT + 1) == 0 and ws(9, 100) == 0


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    loss = lib.raw('mm_sst_kl_loss')

    def call(dtype=B.MM_F32, mode=B.SST_INCLUSIVE, target=q, m=q, n=10, grad=q, out=q, ws=q):
        return loss(dtype, mode, target, m, n, 1.3, grad, out, ws, None)
    assert call(target=None) == -1 and call(m=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    assert call(mode=3) == -1 and call(mode=-1) == -1 and call(dtype=5) == -1 and call(n=-1) == -1
    assert call(n=0, out=None) == -1 and call(n=1, out=None) == -1
    for mode in (B.SST_INCLUSIVE, B.SST_EXCLUSIVE, B.SST_EXCLUSIVE_REFERENCE):
        assert call(n=LIMIT + 1, mode=mode) == -2 and call(n=1 << 40, grad=None, mode=mode) == -2
    assert call(n=LIMIT + 1, mode=7) == -1                   # an argument error is reported first
    with pytest.raises(B.BackendError):
        lib.call('mm_sst_kl_loss', B.MM_F32, 0, None, q, 10, 1.3, None, q, q, None)


def test_gpu_route_declines_cpu_tensors_only_when_forced():
    """CPU tensors take the torch-op form; the kernel route itself has no CPU fallback."""
    from graphembed.objectives import _SstKL
    with pytest.raises(B.BackendError):
        _SstKL.apply(torch.ones(3), torch.ones(3), 0, 1.0)


@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = {nm: k for nm, k in kernel_meta.kernels().items() if nm.startswith('sst::')}
    want = {f'sst::sst_{k}_kernel<{t}>' for k in ('diag', 'panel', 'trail', 'finish') for t in ('float', 'double')}
    want |= {f'sst::sst_max_kernel<{t}, {b}>' for t in ('float', 'double') for b in ('false', 'true')}
    want |= {f'sst::sst_{k}_kernel<{t}, {j}>' for k in ('mm', 'pair') for t in ('float', 'double') for j in (0, 1, 2)}
    want |= {f'sst::sst_assemble_kernel<{t}, {b}>' for t in ('float', 'double') for b in ('false, false', 'false, true', 'true, false')}
    assert want <= set(ks), want - set(ks)
    for nm, k in ks.items():
        print(nm, k)
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
        assert k['lds'] <= 65536
