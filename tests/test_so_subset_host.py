"""CPU-only checks of the SO(n) node-minibatch kernels (mm_so_pdist_fwd_subset, mm_so_pdist_bwd_subset, mm_so_pdist_loss_subset;
csrc/so.hip with SUB): the tolerance rule of tests/so_subset_cases.py is not vacuous on these cases (bound_f32 <= CAP S for every
compared quantity), the quotient targets keep their margin from the kinks, the symbols are declared and exported, argument errors
return before anything touches a GPU, the registers of the new kernels in the built library, and the Python hooks decline CPU
tensors."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

import so_subset_cases as C
from graphembed import _backend as B

NEW = ('mm_so_pdist_fwd_subset', 'mm_so_pdist_bwd_subset', 'mm_so_pdist_loss_subset')


# ---- the rule on these cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', C.DIMS)
def test_the_rule_is_capped_and_the_targets_keep_their_margin(N):
    worst, count, zero_scale, nudged = (0.0, ''), 0, 0, 0
    for regime in C.REGIMES:
        for bs in C.BATCHES:
            margin = C.kink_margin(regime, N, bs)
            assert margin >= C.MARGIN, (regime, bs, margin)
            nudged = max(nudged, C.nudged_pairs(regime, N, bs))
            idx = C.batch_idx(bs)
            assert 0 in idx.tolist() and C.N_TOTAL - 1 in idx.tolist() and bool((idx[1:] < idx[:-1]).any())
    for tag, name, q in C.compared(N):
        count += 1
        assert q.bound('f64') <= q.bound('f32'), (tag, name)
        if q.scale == 0:   # every pair of the batch coincides: held to exact zeros (so_subset_cases.held)
            assert N == 2 and ' init ' in tag and float(q.want.abs().max()) == 0 and C.held(q).bound('f32') == 0, (tag, name)
            zero_scale += 1
            continue
        r = q.bound('f32') / q.scale
        worst = max(worst, (r, f'{tag} {name}'))
        assert r <= C.CAP, (tag, name, r, q.cond, q.port32, q.scale)
        assert C.held(q) is q
    print(f'N={N}: {count} quantities ({zero_scale} with S = 0), worst bound_f32 / S = {worst[0]:.2e} ({worst[1]}); at most {nudged} '
          f'pairs of a case nudged')
    # per N: 2 regimes x 2 losses x (3 + 6 ranges) x 3 objective quantities, and (3 + 4) x 4 batches of pair-vector quantities
    assert count == 2 * 2 * 9 * 3 + 7 * 4 and zero_scale == (18 if N == 2 else 0) and nudged <= 16


def test_every_case_is_counted():
    assert sum(1 for N in C.DIMS for _ in C.compared(N)) == 408


@pytest.mark.parametrize('N', C.DIMS)
def test_the_rule_bounds_the_repeated_node_and_the_training_steps(N):
    idx = C.batch_idx(C.REPEAT['bs'], True)
    assert int(idx[C.REPEAT['a']]) == int(idx[C.REPEAT['b']]) and torch.unique(idx).numel() == C.REPEAT['bs'] - 1
    for tag, name, q in C.repeat_compared(N):
        assert q.scale > 0 and q.bound('f32') <= C.CAP * q.scale, (tag, name, q.bound('f32'), q.scale)
        if name.endswith('val'):
            assert float(q.want[C.repeat_pair()]) == 0.0   # the pair of the node with itself
    if N == C.TRAIN['N']:
        b1, b2 = C.train_batches()
        assert len(set(b1.tolist()) & set(b2.tolist())) == 30 and len(set(b1.tolist()) | set(b2.tolist())) < C.N_TOTAL
        for name, q in C.train_quantities().items():
            assert q.bound('f32') <= C.CAP * q.scale, (name, q.bound('f32'), q.scale)


def test_the_dense_targets_are_not_symmetric():
    d = C.dense('spread', 3, 130)
    assert d.dtype == torch.float32 and float(d.min()) >= 0.5 and float(d.max()) <= 3.5 * 1.01**8
    assert float((d - d.T).abs().max()) > 1.0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
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
    fwd, bwd, loss = (lib.raw(k) for k in NEW)
    BIG = 1 << 30

    def f(x=q, n_total=20, N=3, idx=q, bs=10, rb=0, re=10, out=q, dtype=B.MM_F32, squared=1):
        return fwd(dtype, x, n_total, N, idx, bs, rb, re, squared, out, None)

    def b(x=q, g=q, n_total=20, N=3, idx=q, bs=10, rb=0, re=10, grad=q, ws=q, dtype=B.MM_F32):
        return bwd(dtype, x, g, n_total, N, idx, bs, rb, re, 1, grad, ws, None)

    def l(x=q, dense=q, n_total=20, N=3, idx=q, bs=10, rb=0, re=10, out=q, grad=q, ws=q, kind=B.LOSS_STRESS, dtype=B.MM_F32):
        return loss(dtype, kind, x, dense, q, n_total, N, idx, bs, rb, re, 1.0, 1.0, 3, None, out, grad, ws, None)

    # null pointers (idx, dense, g, out only when there are pairs)
    assert f(x=None) == -1 and f(idx=None) == -1 and f(out=None) == -1
    assert b(x=None) == -1 and b(g=None) == -1 and b(idx=None) == -1 and b(grad=None) == -1 and b(ws=None) == -1
    assert l(x=None) == -1 and l(dense=None) == -1 and l(idx=None) == -1 and l(out=None) == -1 and l(grad=None) == -1 and l(ws=None) == -1
    assert b(grad=None, bs=0, re=0) == -1 and l(ws=None, bs=1, re=1) == -1   # (the outputs are written without pairs too)
    # bad counts and row ranges
    for call in (f, b, l):
        assert call(bs=-1, re=0) == -1 and call(n_total=0, bs=0, re=0) == -1 and call(n_total=-3) == -1
        assert call(rb=5, re=4) == -1 and call(re=11) == -1 and call(rb=-1) == -1
        assert call(n_total=BIG + 1) == -1 and call(dtype=5) == -1 and call(N=0) == -1 and call(N=-2) == -1
        for N in (1, 5, 9):
            assert call(N=N) == -2, N
        # more tiles than one grid dimension holds
        assert call(n_total=BIG, bs=BIG, re=BIG) == -2
    assert l(bs=21, re=21) == -1                                          # the nodes of a batch are distinct: bs <= n_total
    assert f(bs=BIG + 1, re=1) == -1 and b(bs=BIG + 1, re=1) == -1        # repeats allowed: bs <= 2^30
    assert f(bs=BIG, re=1 << 21) == -2                                    # (bs > n_total is no error here: 2^37 tiles are)
    assert l(kind=99) == -1 and l(kind=B.LOSS_NONE) == -1
    # a forward row range of 2^20 rows or more
    assert f(n_total=1 << 20, bs=1 << 20, re=1 << 20) == -2 and f(bs=(1 << 20) + 32, rb=16, re=(1 << 20) + 16) == -2
    # nothing to do: no pair, no launch
    assert f(bs=0, re=0, idx=None, out=None) == 0 and f(bs=1, re=1, idx=None, out=None) == 0
    assert f(rb=4, re=4, idx=None, out=None) == 0 and f(rb=9, re=10, idx=None, out=None) == 0   # (the last row has no pair)
    for squared in (0, 1):
        assert f(bs=0, re=0, squared=squared) == 0
    with pytest.raises(B.BackendError):
        lib.call('mm_so_pdist_loss_subset', B.MM_F32, B.LOSS_STRESS, None, q, q, 20, 3, q, 10, 0, 10, 1.0, 1.0, 3, None, q, q, q, None)


# ---- registers -----------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_keep_everything_in_registers():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernels()
    so = {nm: k for nm, k in meta.items() if re.match(r'so(_\w+)?::', nm)}
    # pdist forward: 3 sizes x 2 dtypes; the pair kernel: x (the squared and the non-squared backward, stress, quotient); each for
    # the minibatch (SUB = true) and the full batch; 12 element-wise kernels and 2 finalize: all in so::, no other SO namespace
    assert len(so) == 2 * (6 + 24) + 12 + 2 and all(nm.startswith('so::') for nm in so), sorted(so)
    assert sum('so_map_kernel' in nm or 'so_dist_kernel' in nm for nm in so) == 12 and sum('so_finalize_kernel' in nm for nm in so) == 2
    for sub in ('true', 'false'):
        assert sum(re.match(rf'so::so_pdist_fwd_kernel<.*, {sub}>$', nm) is not None for nm in so) == 6, sub
        assert sum(re.match(rf'so::so_pdist_sym_kernel<.*, {sub}>$', nm) is not None for nm in so) == 24, sub
    for nm, k in so.items():
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
    # vector registers of the 60 pair kernels as (minibatch, full batch): the register table of profiles/so_minibatch.md, recorded
    # before the two families shared a source
    forms = ('0, true', '0, false', '1, true', '2, true')   # the table's columns after the forward
    vgprs = {('float', 2): ((18, 18), (32, 32), (32, 32), (38, 35), (43, 40)),
             ('float', 3): ((29, 29), (54, 54), (54, 54), (60, 57), (66, 63)),
             ('float', 4): ((48, 48), (91, 91), (91, 91), (92, 94), (99, 96)),
             ('double', 2): ((68, 68), (94, 94), (94, 94), (102, 100), (108, 104)),
             ('double', 3): ((100, 100), (140, 140), (140, 140), (150, 146), (152, 150)),
             ('double', 4): ((122, 122), (202, 202), (202, 202), (210, 208), (216, 212))}
    checked = 0
    for (T, N), row in vgprs.items():
        names = [f'so::so_pdist_fwd_kernel<{T}, {N}'] + [f'so::so_pdist_sym_kernel<{T}, {N}, {form}' for form in forms]
        for name, (v_sub, v_full) in zip(names, row):
            sub, full = so[name + ', true>'], so[name + ', false>']
            assert (sub['vgpr'], full['vgpr']) == (v_sub, v_full), (name, sub['vgpr'], full['vgpr'])
            assert sub['lds'] == full['lds'], name
            checked += 2
    assert checked == 60


# ---- Python --------------------------------------------------------------------------------------------------------------------
def test_the_python_layer_declines_cpu_tensors():
    import graphembed.manifolds as M
    man = M.SpecialOrthogonal(3)
    x = torch.eye(3).repeat(5, 1, 1)
    dense, idx = torch.rand(5, 5), torch.tensor([4, 0, 2])
    assert man.subset_form(x) is False
    assert man.pdist_loss_subset(x, torch.tensor(0.3), idx, dense, ('stress', 1.0, 1.0, 3)) is None   # the caller gathers
    assert man.pdist_subset(x, idx) is None and man.pdist_subset(x, idx, squared=True, rows=(0, 1), cache={}) is None
    for other in (M.Stiefel(3, 3), M.Grassmann(5, 2)):
        assert getattr(other, 'pdist_subset', None) is None   # only SpecialOrthogonal offers the pair-vector hook
    assert getattr(M.Stiefel(3, 3), 'pdist_loss_subset', None) is None
