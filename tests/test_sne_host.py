"""CPU-only checks of the stochastic-neighbour KL objective: the long-double oracle of tests/sne_cases.py against the recorded
reference, the torch-op form of StochasticNeighborLoss against the oracle, and the host side of the new entry points
(declared, exported, workspace size, argument errors before anything touches a GPU, register / scratch budget)."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import sne_cases as S
from graphembed import _backend as B
from graphembed.objectives import StochasticNeighborLoss

NEW = ('mm_sne_kl_ws_bytes', 'mm_sne_kl_loss')
LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
CASE_IDS = [f'n{n}-{r}' for n, r in S.CASES]


@pytest.mark.parametrize('n,regime', S.CASES, ids=CASE_IDS)
def test_oracle_matches_the_recorded_fp64_reference(n, regime):
    """<= 1e-11 relative to |loss| and to max|grad| (measured: 2e-13 and 1.2e-13 at worst)."""
    rec = S.recorded(n, regime)
    for mode in S.MODES:
        loss, grad = S.oracle(n, regime, mode)
        assert np.isfinite(rec[f'{mode}/grad_f64']).all() and np.isfinite(rec[f'{mode}/grad_f32']).all()
        assert S.scale_of(grad) >= 0.028          # (every kept case has a gradient worth comparing against)
        el = S.deviation(rec[f'{mode}/loss_f64'], loss) / abs(float(loss))
        eg = S.deviation(rec[f'{mode}/grad_f64'], grad) / S.scale_of(grad)
        print(f'n{n}/{regime}/{mode}: loss {el:.2e} grad {eg:.2e}')
        assert el <= 1e-11 and eg <= 1e-11, (mode, el, eg)


def test_case_list_and_inputs_follow_the_stated_rule():
    assert len(S.CASES) == 7 * 2 + 5 + 3
    for n, regime in S.CASES:
        g, m = S.inputs(n, regime)
        g2, m2 = S.make_inputs(n, regime)
        assert g.dtype == np.uint8 and m.dtype == np.float32 and len(g) == len(m) == n * (n - 1) // 2
        assert np.array_equal(g, g2) and np.array_equal(m, m2)
        assert g.min() >= 1 and g.max() <= 6
    for name in {S.shard_of(n, r) for n, r in S.CASES}:
        assert os.path.getsize(os.path.join(S.GOLDEN, name + '.npz')) < (1 << 20), name


@pytest.mark.parametrize('dname', ['f32', 'f64'])
@pytest.mark.parametrize('n,regime', S.CASES, ids=CASE_IDS)
def test_torch_op_form_holds_the_tolerance_rule(n, regime, dname):
    dt = {'f32': torch.float32, 'f64': torch.float64}[dname]
    g, m = S.inputs(n, regime)
    failures = []
    for mode in S.MODES:
        fn = StochasticNeighborLoss(inclusive=mode == 'incl')
        mt = torch.from_numpy(m).to(dt).requires_grad_()
        loss = fn(torch.from_numpy(g.astype(np.float64)).to(dt), mt, alpha=S.ALPHA)
        gr, = torch.autograd.grad(loss, mt)
        assert loss.dtype == dt and gr.shape == mt.shape
        S.check(n, regime, mode, dname, 'loss', loss.detach().numpy(), failures)
        S.check(n, regime, mode, dname, 'grad', gr.numpy(), failures)
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('inclusive', [True, False])
def test_two_nodes_give_exact_zeros_in_the_torch_op_form(inclusive):
    for dt in (torch.float32, torch.float64):
        m = torch.tensor([2.7], dtype=dt, requires_grad=True)
        loss = StochasticNeighborLoss(inclusive=inclusive)(torch.tensor([3.0], dtype=dt), m, alpha=S.ALPHA)
        gr, = torch.autograd.grad(loss, m)
        assert float(loss.detach()) == 0.0 and float(gr) == 0.0
    assert str(StochasticNeighborLoss()) == 'kl_loss'
    assert not hasattr(StochasticNeighborLoss(), 'fused_spec')


def test_a_length_that_is_no_triangular_number_is_refused():
    fn = StochasticNeighborLoss()
    for bad in (2, 4, 5, 7, 2079):
        with pytest.raises(ValueError):
            fn(torch.ones(bad), torch.ones(bad), alpha=1.0)
    with pytest.raises(ValueError):
        fn(torch.ones(3), torch.ones(6), alpha=1.0)
    assert float(fn(torch.ones(0), torch.ones(0), alpha=1.0)) == 0.0   # one node, no pair


def test_the_name_of_the_reference_class_is_not_defined_here():
    import graphembed.objectives as O
    assert not hasattr(O, 'KLDiveregenceLoss')   # under the overlay that name resolves to the checkout


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', plain))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert declared == set(B.SIGNATURES)
    assert re.search(r'MM_SNE_INCLUSIVE\s*=\s*0\s*,\s*MM_SNE_EXCLUSIVE\s*=\s*1', plain)
    assert (B.SNE_INCLUSIVE, B.SNE_EXCLUSIVE) == (0, 1)
    assert B.lib().raw('mm_abi_version')() == 4


@pytest.mark.parametrize('dtype,size', [(B.MM_F32, 4), (B.MM_F64, 8)])
def test_workspace_is_monotone_and_covers_slab_and_table(dtype, size):
    ws = B.lib().raw('mm_sne_kl_ws_bytes')
    last = 0
    for n in (0, 1, 2, 3, 63, 64, 65, 129, 257, 1025, 5000, 32768):
        b = ws(dtype, n)
        blocks = (n + 63) // 64
        # one record of 6 values per node and block (+ 1: a node is row AND column of its diagonal tile), the node table, fp64 partials
        assert b >= size * 6 * n * (blocks + 1) + size * 6 * n + 8 * ((n + 255) // 256), (n, b)
        assert b >= last, n
        last = b
    assert ws(dtype, 5000) <= 0.1 * 5 * size * (5000 * 4999 // 2)   # the slab stays under a tenth of the pair traffic
    assert ws(dtype, -1) == 0 and ws(dtype, 32769) == 0 and ws(9, 100) == 0


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    loss = lib.raw('mm_sne_kl_loss')

    def call(dtype=B.MM_F32, mode=B.SNE_INCLUSIVE, target=q, m=q, n=10, grad=q, out=q, ws=q):
        return loss(dtype, mode, target, m, n, 1.3, grad, out, ws, None)
    assert call(target=None) == -1 and call(m=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1 and call(dtype=5) == -1 and call(n=-1) == -1
    assert call(n=32769) == -2 and call(n=1 << 40, grad=None) == -2
    assert call(n=32769, mode=7) == -1                   # an argument error is reported first
    with pytest.raises(B.BackendError):
        lib.call('mm_sne_kl_loss', B.MM_F32, 0, None, q, 10, 1.3, None, q, q, None)


def test_gpu_route_declines_cpu_tensors_only_when_forced():
    """CPU tensors take the torch-op form; the kernel route itself has no CPU fallback."""
    from graphembed.objectives import _SneKL
    with pytest.raises(B.BackendError):
        _SneKL.apply(torch.ones(3), torch.ones(3), 0, 1.0)


@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = {nm: k for nm, k in kernel_meta.kernels().items() if nm.startswith('sne::')}
    want = {f'sne::sne_{k}_kernel<{t}, {mode}>' for k in ('stats', 'grad') for t in ('float', 'double') for mode in (0, 1)}
    want |= {f'sne::sne_{k}_kernel<{t}>' for k in ('merge', 'finish') for t in ('float', 'double')}
    assert want <= set(ks), want - set(ks)
    for nm, k in ks.items():
        print(nm, k)
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
