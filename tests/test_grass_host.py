"""CPU-only checks of the Grassmann fused-objective and matrix optimizer entry points: declared and exported, workspace
size, the form table, and argument errors that return before anything touches a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from graphembed import _backend as B

NEW = ('mm_grass_pdist_loss_ws_bytes', 'mm_grass_pdist_loss_form', 'mm_grass_pdist_loss', 'mm_mat_rsgd_step',
       'mm_mat_rsgd_momentum_step')
LOSS_SLOTS = 256   # csrc/loss.hpp


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert B.lib().raw('mm_abi_version')() == 4


@pytest.mark.parametrize('dtype,size', [(B.MM_F32, 4), (B.MM_F64, 8)])
def test_workspace_covers_accumulators_and_loss_slots(dtype, size):
    ws = B.lib().raw('mm_grass_pdist_loss_ws_bytes')
    for N, p in ((4, 1), (5, 2), (9, 4)):
        last = 0
        for n in (1, 2, 63, 64, 65, 257, 2000, 1 << 20, 1 << 30):
            b = ws(dtype, n, N, p)
            assert b >= size * (n * N * p + 2 * LOSS_SLOTS), (n, N, p, b)   # transposed accumulators [N*p][n] + 2 x 256 slots
            assert b >= last, (n, N, p)
            last = b


def test_form_table():
    form = B.lib().raw('mm_grass_pdist_loss_form')
    for dtype in (B.MM_F32, B.MM_F64):
        for N in range(1, 10):
            for p in range(1, min(N, 4) + 1):
                assert form(dtype, N, p) in (0, 1), (dtype, N, p)
        assert form(dtype, 10, 5) == -2 and form(dtype, 10, 2) == -2 and form(dtype, 6, 5) == -2
        assert form(dtype, 3, 4) == -1 and form(dtype, 0, 0) == -1
        assert form(B.MM_F32, 5, 2) == 1   # every fp32 instantiation is symmetric
    assert form(7, 5, 2) == -1


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    loss = lib.raw('mm_grass_pdist_loss')

    def call(x=q, target=q, n=10, N=5, p=2, rb=0, re=10, out=q, grad=q, ws=q, kind=B.LOSS_STRESS, dtype=B.MM_F32):
        return loss(dtype, kind, x, target, q, n, N, p, rb, re, 1.0, 1.0, 3, None, out, grad, ws, None)
    assert call(x=None) == -1 and call(grad=None) == -1 and call(ws=None) == -1 and call(out=None) == -1
    assert call(target=None) == -1                       # pairs in the range need their targets
    assert call(rb=5, re=4) == -1 and call(re=11) == -1 and call(rb=-1) == -1
    assert call(N=2, p=3) == -1                          # p > N
    assert call(n=(1 << 30) + 1, re=10) == -1
    assert call(kind=99) == -1 and call(dtype=5) == -1
    assert call(N=10, p=5) == -2 and call(N=10, p=2) == -2 and call(N=6, p=5) == -2
    with pytest.raises(B.BackendError):
        lib.call('mm_grass_pdist_loss', B.MM_F32, B.LOSS_STRESS, None, q, q, 10, 5, 2, 0, 10, 1.0, 1.0, 3, None, q, q, q, None)

    step, mom = lib.raw('mm_mat_rsgd_step'), lib.raw('mm_mat_rsgd_momentum_step')
    for kind in (B.GRASSMANN, B.STIEFEL):
        for retr in (B.MAT_RETR_SVD, B.MAT_RETR_QR):
            assert step(B.MM_F32, kind, retr, None, q, 4, 5, 2, 0.1, -1.0, 0, q, None) == -1        # null x
            assert step(B.MM_F32, kind, retr, q, None, 4, 5, 2, 0.1, -1.0, 0, q, None) == -1        # null gradient
            assert step(B.MM_F32, kind, retr, q, q, 4, 5, 2, 0.1, -1.0, 0, None, None) == -1        # null x_new
            assert step(B.MM_F32, kind, retr, q, q, 4, 2, 3, 0.1, -1.0, 0, q, None) == -1           # p > N
            assert step(B.MM_F32, kind, retr, q, q, -1, 5, 2, 0.1, -1.0, 0, q, None) == -1
            assert step(B.MM_F32, kind, retr, q, q, 4, 10, 5, 0.1, -1.0, 0, q, None) == -2
            assert mom(B.MM_F32, kind, retr, q, q, None, 4, 5, 2, 0.1, 0.9, 0.1, -1.0, 0, q, None) == -1   # null buffer
            assert mom(B.MM_F32, kind, retr, q, q, q, 4, 10, 5, 0.1, 0.9, 0.1, -1.0, 0, q, None) == -2
            assert step(B.MM_F32, kind, retr, q, q, 0, 5, 2, 0.1, -1.0, 0, q, None) == 0            # nothing to do
    assert step(B.MM_F32, B.STIEFEL, B.MAT_RETR_SVD, q, q, 4, 5, 2, 0.1, -1.0, 1, q, None) == -2    # Stiefel has no exp
    assert mom(B.MM_F64, B.STIEFEL, B.MAT_RETR_QR, q, q, q, 4, 5, 2, 0.1, 0.9, 0.1, -1.0, 1, q, None) == -2
    assert step(B.MM_F32, 2, B.MAT_RETR_SVD, q, q, 4, 5, 2, 0.1, -1.0, 0, q, None) == -1            # unknown kind
    assert step(B.MM_F32, B.GRASSMANN, B.MAT_PROJU, q, q, 4, 5, 2, 0.1, -1.0, 0, q, None) == -1     # not a retraction
    assert step(B.MM_F32, B.GRASSMANN, B.MAT_EXP, q, q, 4, 5, 2, 0.1, -1.0, 0, q, None) == -1


def test_fused_steps_decline_cpu_tensors():
    import torch
    import graphembed.manifolds as M
    man = M.Grassmann(5, 2)
    x, g = torch.eye(5, 2).repeat(3, 1, 1), torch.randn(3, 5, 2)
    assert man.rsgd_step(x, g, lr=0.1) is None
    assert man.rsgd_momentum_step(x, g, g.clone(), lr=0.1, momentum=0.9, dampening=0.0) is None
    assert M.Stiefel(5, 2, retr='qr')._retr_op == B.MAT_RETR_QR and man._retr_op == B.MAT_RETR_SVD
    assert getattr(M.Stiefel(5, 2), 'pdist_loss', None) is None and callable(man.pdist_loss)
