"""CPU-only checks of the in-kernel node minibatch of a product of constant-curvature factors (mm_stereo_product_loss_subset) and
of the fused Riemannian Adam step (mm_stereo_radam_step): the case list of tests/stereo_subset_cases.py and its kink condition,
the long-double oracle against the recorded fp64 reference (products.Embedding.compute_dists(idx) + objective + autograd), the
host side of the two entry points (declared, exported, workspace of the batch's size, argument errors before anything touches a
GPU, register / LDS / scratch budget of the new kernels) and the CPU behaviour of the Python layer."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import stereo_cases as S
import stereo_product_cases as P
import stereo_subset_cases as C
from graphembed import _backend as B

NEW = ('mm_stereo_product_loss_subset', 'mm_stereo_radam_step')
LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'

# vector registers (vgpr + agpr) of every new instantiation as built: the pair kernels at the values of their full-batch twins
REGISTERS = {
    'subset_loss_kernel<float, 4, {L}>': 121, 'subset_loss_kernel<float, 8, {L}>': 132, 'subset_loss_kernel<float, 16, {L}>': 164,
    'subset_loss_kernel<double, 4, {L}>': 202, 'subset_loss_kernel<double, 8, {L}>': 206, 'subset_loss_kernel<double, 16, {L}>': 254,
    'subset_finalize_kernel<float>': 26, 'subset_finalize_kernel<double>': 44,
    'subset_clear_kernel<float>': 6, 'subset_clear_kernel<double>': 6,
    'radam_kernel<float>': 86, 'radam_kernel<double>': 160,
}


def test_case_list_and_inputs_follow_the_stated_rule():
    assert len(C.CASES) == 6 + 4 + 1 + 6 and len(set(C.CASE_IDS)) == len(C.CASES)
    assert [c[1] for c in C.CASES[:6]] == [2, 3, 64, 65, 129, 257] and all(c[0] == 257 and c[2:6] == ((5, 5), (0.01, -0.3), (False, False), 'spread')
                                                                          for c in C.CASES[:6])
    assert [c[2] for c in C.CASES[6:10]] == [(1, 16), (2, 3, 5, 8), (2, ) * 8, (16, ) * 8] and all(c[:2] == (129, 65) and c[5] == 'spread' for c in C.CASES[6:10])
    assert all(c[3] == tuple(P.C_CYCLE[k % 4] for k in range(len(c[2]))) for c in C.CASES[6:10])
    assert C.CASES[10] == (129, 65, (5, 5), (0.01, -0.3), (False, False), 'init', None)
    assert [c[6] for c in C.CASES[11:]] == list(S._rows(129)) and all(c[:6] == (257, 129, (5, 8), (0.01, -0.3), (False, False), 'spread') for c in C.CASES[11:])
    assert (128, 129) in [c[6] for c in C.CASES] and (5, 5) in [c[6] for c in C.CASES] and C.SHARD_BASE == C.CASES[11]
    assert C.SETTING_IDS == ['stress', 'q1', 'q2', 'q3', 'q3b']
    for case in C.CASES:
        n_total, bs = case[:2]
        xs, craws, idx = C.make_inputs(case)
        assert idx.dtype == np.int64 and idx.shape == (bs, ) and len(set(idx.tolist())) == bs and 0 <= idx.min() and idx.max() < n_total
        assert np.array_equal(idx, C.batch_of(case)) and (bs < 3 or not (np.diff(idx) > 0).all()), 'a fixed permutation slice, not monotone'
        assert all(x.shape == (n_total, d) and x.dtype == np.float32 for x, d in zip(xs, case[2]))
        dense = C.dense_of(case)
        a, b = np.triu_indices(bs, 1)
        _, t = C.pairs_of(C.base_of(case))
        assert dense.dtype == np.float32 and np.array_equal(dense[idx[a], idx[b]], t) and np.array_equal(dense[idx[b], idx[a]], t)
        assert int(np.isfinite(dense).sum()) == bs * (bs - 1) and np.isnan(np.diag(dense)).all()   # every other entry is NaN
        px = C.poisoned(xs[0], idx)
        assert np.array_equal(px[idx], xs[0][idx]) and int(np.isnan(px).any(-1).sum()) == n_total - bs
        rb, re = C.rows_of(case)
        assert 0 <= rb <= re <= bs
    assert C.batch_of(C.CASES[5]).tolist() != list(range(257)) and sorted(C.batch_of(C.CASES[5]).tolist()) == list(range(257))
    path = os.path.join(S.GOLDEN, 'stereo_subset.npz')
    assert os.path.getsize(path) < 1000000
    assert 'product33/idx' in S.recorded() and 'train40/target' in S.recorded()   # the other records keep loading beside `sub/`


@pytest.mark.parametrize('case', C.CASES, ids=C.CASE_IDS)
def test_targets_stay_clear_of_the_quotient_kink(case):
    """target = float32(m F[k mod 4]) over the batch's pairs: both |.| of the quotient loss stay >= 1e-4 from their kink in the
    oracle, for every setting, without reseeding (SALT is empty) and without filtering.  Measured worst margin 1.78e-4
    (ds = (1, 16), eps = 1/2), >= 0.12 for every other case."""
    assert not C.SALT
    m, t = C.pairs_of(C.base_of(case))
    assert t.dtype == np.float32 and len(t) == len(m) == case[1] * (case[1] - 1) // 2
    for setting in C.SETTINGS:
        margin = C.kink_margin(case, setting)
        print(C.case_id(case), setting[0], f'{margin:.3e}')
        assert margin >= C.KINK, (setting[0], margin)


@pytest.mark.parametrize('case', [c for c in C.CASES if C.key(c, 'stress', 'loss', 'f64') in S.recorded()], ids=C.case_id)
def test_oracle_matches_the_recorded_fp64_reference(case):
    """The oracle on the gathered rows against the reference's fp64 minibatch (compute_dists(idx), the objective on
    dense[idx][:, idx], autograd), relative to max m, sum |loss terms|, max |grad_x_k| and sum |g dF/dc_raw|.  The bounds are the
    full-batch ones of test_stereo_product_host.py (twice the figures measured there).  The loss of the 2- and 3-node batches is a
    sum of one or three terms, where nothing averages out: there the bound is the first-order propagation of the pair vector's
    bound, sum_k |g_k| * (bound * max m).  Measured here, worst over the cases:
      init:    pair vector 2.0e-14, loss 2.2e-15, grad_x 2.3e-14, grad_c 4.9e-10
      spread:  pair vector 1.3e-15, loss 1.5e-16 (bs >= 64; 1.0e-15 at bs = 2, 2.7e-15 at bs = 3), grad_x 1.8e-15, grad_c 2.0e-15"""
    R = S.recorded()
    init = case[5] == 'init'
    m, _ = C.pairs_of(C.base_of(case))
    dkey = f'sub/{C.case_id(case)}/dists_f64'
    if case[1] <= 65:
        dv = S.deviation(R[dkey], m) / float(m.max())
        print(f'{C.case_id(case)}: pair vector {dv:.2e}')
        assert dv <= (3.8e-14 if init else 3.0e-15)
    else:
        assert dkey not in R
    idx = C.batch_of(case)
    for name in C.RECORDED:
        o = C.oracle(case, name)
        dl = abs(float(S.LD(R[C.key(case, name, 'loss', 'f64')]) - o['loss'])) / float(o['loss_scale'])
        few = float(3.0e-15 * o['m_max'] * np.abs(P.objective(o['m'], o['target'], C.SETTINGS[C.SETTING_IDS.index(name)])[1]).sum() / o['loss_scale'])
        assert dl <= (2.4e-13 if init else 7.6e-16 if case[1] >= 64 else few), (name, dl)
        for k in range(len(case[2])):
            dx = S.deviation(R[C.key(case, name, f'gx{k}', 'f64')], o['gx'][k][idx]) / float(np.abs(o['gx'][k]).max())
            dc = S.deviation(R[C.key(case, name, f'gc{k}', 'f64')][0], o['gc'][k]) / float(o['gcs'][k])
            print(f'{C.case_id(case)} {name} factor {k}: loss {dl:.2e} grad_x {dx:.2e} grad_c {dc:.2e}')
            assert dx <= (1.6e-13 if init else 7.6e-15) and dc <= (2.8e-8 if init else 2.4e-15), (name, k, dx, dc)


def test_every_case_is_recorded_in_fp32():
    R = S.recorded()
    for case in C.CASES:
        for name in C.SETTING_IDS:
            assert R[C.key(case, name, 'loss', 'f32')].shape == ()
            for k in range(len(case[2])):
                assert R[C.key(case, name, f'gx{k}', 'f32')].shape == (case[1], case[2][k])
                assert R[C.key(case, name, f'gc{k}', 'f32')].shape == (1, )
    for case in C.CASES[:9] + C.CASES[10:12]:
        assert all(C.key(case, name, 'loss', 'f64') in R for name in C.RECORDED)


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', plain))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert declared == set(B.SIGNATURES)
    assert 'mm_stereo_product_loss_subset, mm_pair_gather' in src   # the paragraph on caller-supplied indices names the new entry
    assert B.lib().raw('mm_abi_version')() == 4


def _ms(*m):
    return (ctypes.c_int32 * len(m))(*m)


def test_the_workspace_is_the_batchs():
    """ws = mm_stereo_product_ws_bytes(dtype, bs, nf, m): it does not grow with the table (the GPU tests hand over exactly this
    size with a guard region behind it)."""
    ws = B.lib().raw('mm_stereo_product_ws_bytes')
    for dtype in (B.MM_F32, B.MM_F64):
        assert 0 < ws(dtype, 512, 2, _ms(5, 5)) < ws(dtype, 4039, 2, _ms(5, 5)) // 40
        assert ws(dtype, 32768, 8, _ms(*(2, ) * 8)) > 0 and ws(dtype, 32769, 8, _ms(*(2, ) * 8)) == 0


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p).value
    F32, POS = B.MM_F32, B.STEREO_C_POSITIVE

    def factors(nf=2, m=5, x=q, c=q, gx=q, gc=q, mode=POS, c_min=1e-3, last=None):
        arr = (B.StereoFactor * max(nf, 1))()
        for k in range(max(nf, 1)):
            arr[k] = B.StereoFactor(x, c, gx, gc, c_min, m, mode)
        if last:
            for name, v in last.items():
                setattr(arr[max(nf, 1) - 1], name, v)
        return arr

    def sub(dtype=F32, kind=B.LOSS_STRESS, f='default', nf=2, dense=q, n_total=20, idx=q, bs=10, rb=0, re=10, out=q, ws=q, **kw):
        f = factors(nf, **kw) if f == 'default' else f
        return lib.raw('mm_stereo_product_loss_subset')(dtype, kind, f, nf, dense, n_total, idx, bs, rb, re, 1.0, 0.5, 3, None, out, ws, None)

    assert sub(dtype=5) == -1 and sub(f=None) == -1 and sub(nf=0) == -1 and sub(nf=-1) == -1
    assert sub(m=0) == -1 and sub(c=None) == -1 and sub(mode=3) == -1 and sub(mode=-1) == -1 and sub(c_min=-1.0) == -1
    assert sub(x=None) == -1 and sub(last={'x': None}) == -1 and sub(last={'m': 0}) == -1 and sub(last={'c_mode': 7}) == -1
    assert sub(gx=None) == -1 and sub(gc=None) == -1 and sub(last={'grad_c': None}) == -1
    assert sub(rb=-1) == -1 and sub(re=11) == -1 and sub(rb=6, re=5) == -1      # the range shards the BATCH: re <= bs, not n_total
    assert sub(bs=21, re=21) == -1 and sub(bs=-1, re=0) == -1 and sub(n_total=-1) == -1 and sub(idx=None) == -1 and sub(dense=None) == -1
    assert sub(kind=B.LOSS_NONE) == -1 and sub(kind=3) == -1 and sub(kind=-1) == -1   # an upstream gradient has no dense form
    assert sub(out=None) == -1 and sub(ws=None) == -1
    assert sub(m=17) == -2 and sub(last={'m': 17}) == -2 and sub(nf=9) == -2
    assert sub(n_total=40000, bs=32769, re=32769) == -2 and sub(n_total=1 << 40, bs=1 << 39, re=5) == -2 and sub(n_total=1 << 31) == -2
    assert sub(m=17, mode=7) == -1 and sub(nf=9, last={'m': 0}) == -1 and sub(nf=9, idx=None) == -1   # an argument error is reported first
    with pytest.raises(B.BackendError):
        lib.call('mm_stereo_product_loss_subset', F32, B.LOSS_NONE, factors(), 2, q, 20, q, 10, 0, 10, 1.0, 0.5, 3, None, q, q, None)

    def adam(dtype=F32, x=q, eg=q, m1=q, m2=q, step=q, ticket=q, cnt=4, m=5, c=q, mode=POS, c_min=1e-3, out=q):
        return lib.raw('mm_stereo_radam_step')(dtype, x, eg, m1, m2, ctypes.cast(step, ctypes.POINTER(ctypes.c_double)),
                                               ctypes.cast(ticket, ctypes.POINTER(ctypes.c_uint)), cnt, m, c, mode, c_min, 0.05, 0.9,
                                               0.99, 0, 1e-8, -1.0, 1, out, None)

    assert adam(dtype=5) == -1 and adam(cnt=-1) == -1 and adam(m=0) == -1 and adam(c=None) == -1 and adam(mode=3) == -1 and adam(c_min=-1.0) == -1
    assert adam(x=None) == -1 and adam(eg=None) == -1 and adam(m1=None) == -1 and adam(m2=None) == -1 and adam(out=None) == -1
    assert adam(step=None) == -1 and adam(ticket=None) == -1 and adam(step=None, cnt=0) == -1
    assert adam(m=17) == -2 and adam(m=17, mode=7) == -1
    assert adam(cnt=0, x=None, eg=None, m1=None, m2=None, out=None) == 0       # nothing to do, nothing launched


@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_new_kernels_keep_their_register_lds_and_scratch_budget():
    """Nothing in scratch, nothing spilled, static LDS within 64 KB; vector registers at the values of the build - for the pair and
    finalize kernels those of the full-batch kernels they share their bodies with."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = {nm[len('stereo::'):]: k for nm, k in kernel_meta.kernels().items()
          if nm.startswith('stereo::subset_') or nm.startswith('stereo::radam_')}
    want = {}
    for name, regs in REGISTERS.items():
        for kind in (1, 2) if '{L}' in name else (0, ):
            want[name.format(L=kind)] = regs
    assert set(want) == set(ks), set(want) ^ set(ks)
    for nm, k in ks.items():
        print(nm, k)
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
        assert k['lds'] <= 65536, (nm, k)
        assert k['vgpr'] + k['agpr'] == want[nm], (nm, k, want[nm])
    assert max(k['lds'] for k in ks.values()) == 60192


def test_cpu_tensors_keep_todays_routes():
    from graphembed.manifolds import Stereographic
    from graphembed.modules import ManifoldParameter, StereographicProductEmbedding
    from graphembed.objectives import QuotientLoss, StressLoss
    from graphembed.optim import RiemannianAdam
    man = Stereographic(5)
    assert callable(getattr(Stereographic, 'radam_step', None))
    x = torch.zeros(7, 5)
    step, ticket = torch.ones((), dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    assert man.radam_step(x, x, x.clone(), x.clone(), step, ticket, lr=0.05, betas=(0.9, 0.99), nc=False, eps=1e-8, max_grad_norm=None,
                          exact=True, inplace=False) is None
    # the optimizer does not even ask on the CPU: it composes the update from the class's maps, which refuse CPU tensors
    p = ManifoldParameter(x.clone(), manifold=man)
    p.grad = torch.ones_like(p)
    with pytest.raises(B.BackendError):
        RiemannianAdam([p], lr=0.05).step()
    emb = StereographicProductEmbedding(12, [5, 3])
    dense = torch.ones(12, 12)
    idx = torch.tensor([3, 1, 7, 9])
    for fn in (StressLoss(), QuotientLoss()):
        assert emb.fused_objective(fn, None, idx, dense=dense, validated=True, epoch=1, alpha=1.0) is None
        assert emb.fused_objective(fn, torch.ones(6), idx, dense=dense, epoch=1, alpha=1.0) is None
        assert emb.fused_objective(fn, torch.ones(66), None, dense=dense, epoch=1, alpha=1.0) is None
    assert emb._subset_ws == {}
