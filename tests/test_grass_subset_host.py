"""CPU-only checks of the Grassmann node-minibatch objective and the fused RiemannianAdam step of Grassmann / Stiefel points
(mm_grass_pdist_loss_subset, mm_grass_pdist_loss_subset_form, mm_mat_radam_step): the tolerance rule of tests/grass_subset_cases.py
is not vacuous on these cases (bound_f32 <= CAP S), the quotient targets keep their margin from the kinks, the symbols are
declared and exported, argument errors return before anything touches a GPU, the form table, and the registers / LDS / scratch of
the kernels in the built library: the full-batch objective kernels as recorded from the build before the shared header, the new
ones within what profiles/grass_minibatch.md lists."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import grass_subset_cases as C
from graphembed import _backend as B

NEW = ('mm_grass_pdist_loss_subset', 'mm_grass_pdist_loss_subset_form', 'mm_mat_radam_step')


# ---- the rule on these cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,p', C.SHAPES)
def test_the_rule_bounds_the_minibatch_objective(N, p):
    seen = 0
    for regime in C.mc.regimes(N, p):
        for bs in C.BATCHES:
            assert C.kink_margin(regime, N, p, bs) >= C.MARGIN, (regime, bs)
            idx = C.batch_idx(C.N_TOTAL, bs)
            assert 0 in idx.tolist() and C.N_TOTAL - 1 in idx.tolist() and bool((idx[1:] < idx[:-1]).any())
            for loss_name in C.LOSSES:
                q = C.subset_quantities(regime, N, p, bs, loss_name, C.ranges_of(bs))
                for (rows, name), v in q.items():
                    if name in C.subset_compared(regime, N, p):
                        assert v.scale > 0 and v.bound('f32') <= C.CAP * v.scale, (regime, bs, loss_name, rows, name, v.bound('f32'), v.scale)
                        seen += 1
    assert seen >= 2 * (3 + 5) * 2   # (every case has a loss and at least one gradient)
    assert C.kink_margin('spread', N, p, 65, 65, True) >= C.MARGIN


def test_the_dense_targets_are_not_symmetric():
    d = C.dense('spread', 6, 3, 130)
    assert d.dtype == torch.float32 and float(d.min()) >= 0.5 and float(d.max()) <= 3.5 * 1.01**8
    assert float((d - d.T).abs().max()) > 1.0


@pytest.mark.parametrize('variant', sorted(C.VARIANTS))
def test_the_rule_bounds_the_adam_trajectory(variant):
    kind = C.VARIANTS[variant][0]
    for N, p in C.radam_shapes(kind):
        for cnt in C.RADAM_CNT:
            for nc in (False, True):
                for name, v in C.radam_quantities(variant, cnt, N, p, nc).items():
                    assert v.bound('f32') <= C.CAP * v.scale, (variant, N, p, cnt, nc, name, v.bound('f32'), v.scale)
            gs = C.radam_grads(cnt, N, p)
            if cnt >= 8:
                assert not any(g[5].any() for g in gs) and gs[0][7].any() and not gs[1][7].any() and not gs[2][7].any()


def test_the_rule_bounds_the_wiring_and_training_trajectories():
    for name, v in C.radam_quantities('grassmann_exp', 65, 5, 2, False, 0.01, 100.0).items():
        assert v.bound('f32') <= C.CAP * v.scale, (name, v.bound('f32'), v.scale)
    b1, b2 = C.train_batches()
    only1, only2 = set(b1.tolist()) - set(b2.tolist()), set(b2.tolist()) - set(b1.tolist())
    assert only1 and only2 and len(only1 | only2 | set(b1.tolist())) < C.N_TOTAL   # shared nodes, nodes of one batch, nodes of neither
    for name, v in C.train_quantities().items():
        assert v.bound('f32') <= C.CAP * v.scale, (name, v.bound('f32'), v.scale)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert B.lib().raw('mm_abi_version')() == 4


def test_form_table():
    form = B.lib().raw('mm_grass_pdist_loss_subset_form')
    for dtype in (B.MM_F32, B.MM_F64):
        for N in range(1, 10):
            for p in range(1, min(N, 4) + 1):
                assert form(dtype, N, p) in (1, -2), (dtype, N, p)
                if dtype == B.MM_F32 or p <= 3:    # the way out is capped
                    assert form(dtype, N, p) == 1, (dtype, N, p)
        assert form(dtype, 10, 5) == -2 and form(dtype, 10, 2) == -2 and form(dtype, 6, 5) == -2
        assert form(dtype, 3, 4) == -1 and form(dtype, 0, 0) == -1
    assert form(7, 5, 2) == -1


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    sub = lib.raw('mm_grass_pdist_loss_subset')

    def call(x=q, dense=q, n_total=20, N=5, p=2, idx=q, bs=10, rb=0, re=10, out=q, grad=q, ws=q, kind=B.LOSS_STRESS, dtype=B.MM_F32):
        return sub(dtype, kind, x, dense, q, n_total, N, p, idx, bs, rb, re, 1.0, 1.0, 3, None, out, grad, ws, None)
    assert call(x=None) == -1 and call(grad=None) == -1 and call(ws=None) == -1 and call(out=None) == -1
    assert call(dense=None) == -1 and call(idx=None) == -1          # pairs in the range need their targets and nodes
    assert call(bs=21, re=21) == -1 and call(bs=-1, re=0) == -1     # bs > n_total
    assert call(rb=5, re=4) == -1 and call(re=11) == -1 and call(rb=-1) == -1
    assert call(N=2, p=3) == -1                                     # p > N
    assert call(n_total=(1 << 30) + 1) == -1 and call(n_total=0, bs=0, re=0) == -1
    assert call(kind=99) == -1 and call(kind=B.LOSS_NONE) == -1 and call(dtype=5) == -1
    assert call(N=10, p=5) == -2 and call(N=10, p=2) == -2 and call(N=6, p=5) == -2
    with pytest.raises(B.BackendError):
        lib.call('mm_grass_pdist_loss_subset', B.MM_F32, B.LOSS_STRESS, None, q, q, 20, 5, 2, q, 10, 0, 10, 1.0, 1.0, 3, None, q, q, q, None)

    adam = lib.raw('mm_mat_radam_step')

    def step(kind=B.GRASSMANN, retr=B.MAT_RETR_SVD, x=q, g=q, m=q, v=q, t=q, tk=q, cnt=4, N=5, p=2, exact=0, out=q, dtype=B.MM_F32):
        return adam(dtype, kind, retr, x, g, m, v, t, tk, cnt, N, p, 0.1, 0.9, 0.999, 0, 1e-8, -1.0, exact, out, None)
    for kind in (B.GRASSMANN, B.STIEFEL):
        for retr in (B.MAT_RETR_SVD, B.MAT_RETR_QR):
            for null in ('x', 'g', 'm', 'v', 't', 'tk', 'out'):
                assert step(kind, retr, **{null: None}) == -1, null
            assert step(kind, retr, N=2, p=3) == -1 and step(kind, retr, cnt=-1) == -1
            assert step(kind, retr, N=10, p=5) == -2 and step(kind, retr, N=10, p=2) == -2 and step(kind, retr, N=6, p=5) == -2
            assert step(kind, retr, cnt=0) == 0                     # nothing to do
            assert step(kind, retr, dtype=5) == -1
    assert step(B.STIEFEL, exact=1) == -2 and step(B.STIEFEL, B.MAT_RETR_QR, exact=1, dtype=B.MM_F64) == -2   # Stiefel has no exp
    assert step(kind=2) == -1                                       # unknown kind
    assert step(retr=B.MAT_PROJU) == -1 and step(retr=B.MAT_EXP) == -1   # not a retraction


# ---- registers -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def meta():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    return kernel_meta.kernels()


# (vgpr incl. accumulation registers, sgpr, spilled vector values, spilled scalars, LDS) of grass_loss_sym_kernel<T, NP, P, LOSS>
# (LOSS 1 = stress, 2 = quotient), recorded with tools/kernel_meta.py from the build BEFORE the kernel moved into grass_loss.hpp;
# scratch is 0 everywhere.  {T: {(NP, P): (stress, quotient)}}
PARENT_FULL_BATCH = {
    'double': {(4, 1): ((78, 68, 0, 0, 512), (86, 76, 0, 0, 512)), (4, 2): ((116, 76, 0, 0, 1024), (120, 84, 0, 0, 1024)),
               (4, 3): ((164, 90, 0, 0, 1536), (178, 98, 0, 0, 1536)), (4, 4): ((234, 100, 0, 0, 2048), (238, 105, 0, 0, 2048)),
               (6, 1): ((92, 76, 0, 0, 768), (96, 84, 0, 0, 768)), (6, 2): ((134, 88, 0, 0, 1536), (138, 96, 0, 0, 1536)),
               (6, 3): ((198, 106, 0, 0, 2304), (203, 106, 0, 7, 2304)), (6, 4): ((261, 106, 6, 9, 3072), (264, 106, 0, 19, 3072)),
               (9, 1): ((106, 88, 0, 0, 1152), (110, 96, 0, 0, 1152)), (9, 2): ((162, 106, 0, 0, 2304), (166, 106, 0, 7, 2304)),
               (9, 3): ((235, 106, 0, 13, 3456), (239, 106, 0, 27, 3456)), (9, 4): ((316, 106, 6, 41, 4608), (320, 106, 0, 55, 4608))},
    'float': {(4, 1): ((26, 50, 0, 0, 256), (30, 56, 0, 0, 256)), (4, 2): ((47, 60, 0, 0, 512), (50, 64, 0, 0, 512)),
              (4, 3): ((72, 66, 0, 0, 768), (74, 70, 0, 0, 768)), (4, 4): ((110, 72, 0, 0, 1024), (112, 76, 0, 0, 1024)),
              (6, 1): ((34, 58, 0, 0, 384), (36, 64, 0, 0, 384)), (6, 2): ((57, 70, 0, 0, 768), (60, 74, 0, 0, 768)),
              (6, 3): ((84, 78, 0, 0, 1152), (86, 82, 0, 0, 1152)), (6, 4): ((126, 86, 0, 0, 1536), (123, 88, 0, 0, 1536)),
              (9, 1): ((47, 69, 0, 0, 576), (49, 75, 0, 0, 576)), (9, 2): ((78, 84, 0, 0, 1152), (80, 88, 0, 0, 1152)),
              (9, 3): ((102, 93, 0, 0, 1728), (104, 97, 0, 0, 1728)), (9, 4): ((150, 106, 0, 0, 2304), (153, 106, 0, 6, 2304))},
}
# the node-minibatch instantiations <..., true>: vector registers (incl. accumulation registers) at most, per (T, NP, P), both losses
SUBSET_VGPR = {
    'double': {(4, 1): 84, (4, 2): 120, (4, 3): 180, (4, 4): 240, (6, 1): 92, (6, 2): 138, (6, 3): 205, (6, 4): 266,
               (9, 1): 106, (9, 2): 165, (9, 3): 241, (9, 4): 324},
    'float': {(4, 1): 32, (4, 2): 50, (4, 3): 77, (4, 4): 115, (6, 1): 36, (6, 2): 59, (6, 3): 89, (6, 4): 126,
              (9, 1): 45, (9, 2): 79, (9, 3): 107, (9, 4): 156},
}
# mat_radam_kernel<T, NP, P>: vector registers (incl. accumulation registers); no spill, no scratch
RADAM_VGPR = {
    'double': {(4, 1): 58, (4, 2): 108, (4, 3): 158, (4, 4): 220, (6, 1): 78, (6, 2): 152, (6, 3): 222, (6, 4): 284,
               (9, 1): 110, (9, 2): 226, (9, 3): 330, (9, 4): 412},
    'float': {(4, 1): 37, (4, 2): 58, (4, 3): 78, (4, 4): 109, (6, 1): 43, (6, 2): 79, (6, 3): 112, (6, 4): 143,
              (9, 1): 58, (9, 2): 116, (9, 3): 166, (9, 4): 213},
}


def test_the_full_batch_objective_kernels_did_not_change(meta):
    for T, table in PARENT_FULL_BATCH.items():
        for (NP, P), per_loss in table.items():
            for loss, want in zip((1, 2), per_loss):
                k = meta[f'mat::grass_loss_sym_kernel<{T}, {NP}, {P}, {loss}, false>']
                got = (k['vgpr'], k['sgpr'], k['vgpr_spill'], k['sgpr_spill'], k['lds'])
                assert got == want and k['scratch'] == 0, (T, NP, P, loss, k)


def test_the_new_kernels_stay_within_the_listed_registers(meta):
    form = B.lib().raw('mm_grass_pdist_loss_subset_form')
    for T, dtype in (('float', B.MM_F32), ('double', B.MM_F64)):
        for (NP, P), most in SUBSET_VGPR[T].items():
            for loss in (1, 2):
                k = meta.get(f'mat::grass_loss_sym_kernel<{T}, {NP}, {P}, {loss}, true>')
                assert (k is not None) == (form(dtype, NP, P) == 1), (T, NP, P)
                if k is not None:   # built: nothing in scratch, so no scratch access inside the row loop
                    assert k['vgpr'] <= most and k['scratch'] == 0 and k['lds'] == PARENT_FULL_BATCH[T][(NP, P)][0][4], (T, NP, P, loss, k)
        for (NP, P), most in RADAM_VGPR[T].items():
            k = meta[f'mat::mat_radam_kernel<{T}, {NP}, {P}>']
            assert k['vgpr'] <= most and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0 and k['scratch'] == 0, (T, NP, P, k)
    doc = open(os.path.join(ROOT, 'profiles', 'grass_minibatch.md')).read()
    assert 'mat_radam_kernel' in doc and 'grass_loss_sym_kernel' in doc


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_the_python_layer_declines_cpu_tensors():
    import graphembed.manifolds as M
    man = M.Grassmann(5, 2)
    x, g = torch.eye(5, 2).repeat(3, 1, 1), torch.randn(3, 5, 2)
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    step, ticket = torch.ones((), dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    assert man.radam_step(x, g, m, v, step, ticket, lr=0.1, betas=(0.9, 0.999), nc=False, eps=1e-8) is None
    assert M.Stiefel(5, 2).radam_step(x, g, m, v, step, ticket, lr=0.1, betas=(0.9, 0.999), nc=False, eps=1e-8, exact=True) is None
    assert float(step) == 1.0 and not m.any()
    dense, idx = torch.rand(3, 3), torch.tensor([2, 0])
    assert man.pdist_loss_subset(x, torch.tensor(0.3), idx, dense, ('stress', 1.0, 1.0, 3)) is None   # the caller gathers
    assert not man.subset_form(x) and getattr(M.Stiefel(5, 2), 'pdist_loss_subset', None) is None
