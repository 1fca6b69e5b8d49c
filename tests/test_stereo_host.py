"""CPU-only checks of the kappa-stereographic manifold: the long-double oracle of tests/stereo_cases.py against the recorded
reference, the host side of the mm_stereo_* entry points (declared, exported, workspace size, argument errors before anything
touches a GPU, register / scratch budget of the kernels) and the surface of the Python class."""
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
from graphembed import _backend as B

NEW = ('mm_stereo_pdist_ws_bytes', 'mm_stereo_pdist_fwd', 'mm_stereo_pdist_bwd', 'mm_stereo_dist', 'mm_stereo_map',
       'mm_stereo_rsgd_step', 'mm_stereo_stabilize')
LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'
CASE_IDS = [S.case_id(c) for c in S.CASES]
MAPS = ('exp', 'exp_noproject', 'retr', 'projx', 'log', 'transp', 'egrad2rgrad', 'norm')


@pytest.mark.parametrize('case', S.CASES, ids=CASE_IDS)
def test_oracle_matches_the_recorded_fp64_reference(case):
    """Measured worst deviation of the oracle from the reference's fp64 results over the case list, relative to max d / max d^2,
    max |grad_x|, sum |g dF/dc_raw| and max |map|: pair values 5.0e-14 (init) / 1.7e-15 (spread), grad_x 2.5e-14 / 9.5e-16,
    maps 2.5e-14 (log, init) / 5.7e-16, RSGD step 5.7e-16, projx of `edge` 1.2e-15; curvature gradient 8.4e-9 (init) / 3.1e-16
    (spread) - at `init` the REFERENCE's fp64 autograd cancels (w = c r^2 ~ 1e-7: its artanh form loses 1 / w), the oracle does
    not.  The bounds are a factor 4 above these figures."""
    n, m, c_init, fixed, regime, rows = case
    R = S.recorded()
    tag, btag = S.case_id(case), S.case_id(S.base_of(case))
    x, c_raw = S.make_inputs(case)
    mode = S.mode_of(c_init, fixed)
    if regime == 'edge':
        want = S.project(x.astype(S.LD), S.get_c(c_raw, mode)[0], 'f64')
        assert (np.sqrt((x.astype(np.float64) ** 2).sum(-1)) * np.sqrt(float(S.get_c(c_raw, mode)[0])) > 1).sum() >= n // 3
        assert S.deviation(R[f'{btag}/projx_f64'], want) <= 4.8e-15 * float(np.abs(want).max())
        return
    lo, hi = S.pair_slice(n, S.rows_of(case))
    init = regime == 'init'
    for sq, squared in (('d', False), ('sq', True)):
        v = S.pdist(x, c_raw, mode, squared)
        dev = S.deviation(R[f'{btag}/pdist_{sq}_f64'], v) / float(v.max())
        print(f'{tag} {sq}: value {dev:.2e}')
        assert dev <= (2e-13 if init else 7e-15)
        if hi == lo:
            continue
        gx, gc, gcs = S.pdist_grads(x, c_raw, mode, squared, S.upstream(hi - lo), S.rows_of(case))
        dx = S.deviation(R[f'{tag}/gx_{sq}_f64'], gx) / float(np.abs(gx).max())
        # the curvature gradient's scale is the sum of the pairs' MAGNITUDES: at `init` the sum itself cancels
        dc = S.deviation(R[f'{tag}/gc_{sq}_f64'], gc) / float(gcs)
        print(f'{tag} {sq}: grad_x {dx:.2e} grad_c {dc:.2e} (|sum| / sum|.| = {abs(float(gc)) / float(gcs):.2e})')
        assert dx <= (1e-13 if init else 4e-15) and dc <= (3.4e-8 if init else 1.3e-15)
    if rows is None:
        u = S.tangent(case, 1).astype(np.float64) * 0.1
        got = S.maps(x, u, np.roll(x, 1, 0), c_raw, mode, 'f64')
        for k in MAPS:
            dev = S.deviation(R[f'{btag}/{k}_f64'], got[k]) / float(np.abs(got[k]).max())
            assert dev <= (1e-13 if init else 2.3e-15), (k, dev)
        eg = S.tangent(case, 2).astype(np.float64) * 40
        for exact in (0, 1):
            for clip in (None, 20):
                o = S.rsgd_step(x, eg, c_raw, mode, 'f64', 0.01, clip, exact)
                assert S.deviation(R[f'{btag}/rsgd_{exact}_{clip}_f64'], o) <= 2.3e-15 * float(np.abs(o).max())


def test_curvature_gradient_scale_is_the_magnitude_sum():
    """At `init` the reference's own fp32 curvature gradient is off by a large fraction of |sum| while it stays within 7 % of the
    magnitude sum: the scale of every curvature-gradient comparison is sum |g dF/dc_raw|."""
    R = S.recorded()
    seen = 0
    for case in S.CASES:
        if case[4] != 'init' or case[5] is not None or case[0] < 63:
            continue
        x, c_raw = S.make_inputs(case)
        _, gc, gcs = S.pdist_grads(x, c_raw, S.mode_of(case[2], case[3]), True, S.upstream(case[0] * (case[0] - 1) // 2))
        dev32 = S.deviation(R[f'{S.case_id(case)}/gc_sq_f32'], gc)
        assert abs(float(gc)) <= float(gcs) and dev32 <= 0.08 * float(gcs)
        seen += 1
    assert seen >= 5


def test_oracle_matches_the_recorded_product_embedding():
    """The oracle against the reference's recorded fp64 Embedding.stabilize / compute_dists (ds = [5, 5], n = 33) and its 20-epoch
    training trace (n = 40).  Measured: stabilize 6.5e-16 of r_max, compute_dists 5.4e-16 of max, minibatch 4e-16, loss trace
    2.8e-16 relative, curvatures 1.9e-17 absolute; bounds a factor 4 above."""
    R = S.recorded()
    cs = (np.float32(0.01), np.float32(-0.3))
    for k in (0, 1):
        st = S.stabilize(R[f'product33/x{k}'], cs[k], 0, 'f64', 5.0)
        assert S.deviation(R[f'product33/stabilized{k}_f64'], st) <= 2.6e-15 * 5.0
    xs = [R[f'product33/stabilized{k}_f64'] for k in (0, 1)]
    want = sum(S.pdist(x, c, 0, True) for x, c in zip(xs, cs))
    assert S.deviation(R['product33/dists_f64'], want) <= 2.2e-15 * float(want.max())
    idx = R['product33/idx']
    wi = sum(S.pdist(x[idx], c, 0, True) for x, c in zip(xs, cs))
    dev = S.deviation(R['product33/dists_idx_f64'], wi) / float(want.max())
    print(f'minibatch {dev:.2e}')
    assert dev <= 1.6e-15
    tr, cv = S.train_trace([R['train40/x0'], R['train40/x1']], [np.float32(0.01)] * 2, [0, 0], R['train40/target'], 'f64', 20)
    assert float(np.abs((R['train40/loss_f64'] - tr) / tr).max()) <= 1.2e-15
    assert float(np.abs(R['train40/c_f64'] - cv).max()) <= 8e-17
    assert tr[-1] < 0.8 * tr[0]


def test_phi_limit_at_zero_curvature_is_euclidean():
    """c = 0 exactly: the oracle (like the kernels) gives d^2 = 4 q, where the reference returns NaN."""
    x = np.random.RandomState(3).uniform(-1, 1, size=(9, 4)).astype(np.float32)
    i, j = np.triu_indices(9, 1)
    q = ((x[i].astype(np.float64) - x[j]) ** 2).sum(-1)
    got = S.pdist(x, np.float32(0), 0, True, c_min=0.0)
    assert S.deviation(got, 4 * q) <= 1e-15 * float(q.max()) * 4


def test_case_list_and_inputs_follow_the_stated_rule():
    assert len(S.CASES) == 7 + 6 + 16 + 4 + 12 and len(S.CASES) <= 60 and len(set(CASE_IDS)) == len(S.CASES)
    assert {c[0] for c in S.CASES} == set(S.N_SWEEP) and {c[1] for c in S.CASES} >= set(S.M_SWEEP)
    assert {(c[2], c[3]) for c in S.CASES} == {(c, f) for c in S.C_SWEEP for f in (False, True)}
    for case in S.CASES:
        n, m, c_init, fixed, regime, rows = case
        x, c_raw = S.make_inputs(case)
        x2, _ = S.make_inputs(case)
        assert x.dtype == np.float32 and x.shape == (n, m) and np.array_equal(x, x2)
        c = float(S.get_c(c_raw, S.mode_of(c_init, fixed))[0])
        assert (c > 0) == (c_init > 0)
        r = np.sqrt(abs(c)) * np.sqrt((x.astype(np.float64) ** 2).sum(-1)).max()
        if regime == 'spread':
            assert 0.69 <= r <= 0.7
        elif regime == 'edge':
            assert c > 0 and r > 1.1
        else:
            assert r < 0.05
        rb, re = S.rows_of(case)
        assert 0 <= rb <= re <= n
    for n in (129, 257):   # the last row is among the row ranges, and it has no pair
        assert (n - 1, n) in [c[5] for c in S.CASES if c[0] == n] and S.pair_slice(n, (n - 1, n)) == (n * (n - 1) // 2, ) * 2
    g = S.upstream(100)
    assert g.min() < 0 < g.max()
    names = [f for f in os.listdir(S.GOLDEN) if f.startswith('stereo') and f.endswith('.npz')]
    assert names
    for name in names:
        assert os.path.getsize(os.path.join(S.GOLDEN, name)) < (1 << 20), name


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', plain))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert declared == set(B.SIGNATURES)
    assert re.search(r'MM_STEREO_C_FREE\s*=\s*0\s*,\s*MM_STEREO_C_POSITIVE\s*=\s*1\s*,\s*MM_STEREO_C_NEGATIVE\s*=\s*2', plain)
    assert (B.STEREO_C_FREE, B.STEREO_C_POSITIVE, B.STEREO_C_NEGATIVE) == (0, 1, 2)
    for k, name in enumerate(('EGRAD2RGRAD', 'PROJU', 'EXP', 'EXP_NOPROJECT', 'RETR', 'PROJX', 'LOG', 'TRANSP')):
        assert re.search(rf'MM_STEREO_{name}\s*=\s*{k}\b', plain) and getattr(B, f'STEREO_{name}') == k
    assert B.lib().raw('mm_abi_version')() == 4


@pytest.mark.parametrize('dtype,size,rows', [(B.MM_F32, 4, 64), (B.MM_F64, 8, 32)])
def test_workspace_is_monotone_and_covers_the_documented_layout(dtype, size, rows):
    ws = B.lib().raw('mm_stereo_pdist_ws_bytes')
    for m in (1, 5, 16):
        last = 0
        for n in (0, 1, 2, 3, 63, 64, 65, 129, 257, 1025, 4039, 32768):
            b = ws(dtype, n, m)
            nbr, nbc = (n + rows - 1) // rows, (n + 63) // 64
            # one record of m + 1 values per node and tile row / tile column, one fp64 partial per tile
            assert b >= size * (m + 1) * n * (nbr + nbc) + 8 * nbr * nbc, (n, m, b)
            assert b >= last, (n, m)
            last = b
    assert ws(dtype, -1, 5) == 0 and ws(dtype, 32769, 5) == 0 and ws(9, 100, 5) == 0 and ws(dtype, 100, 0) == 0 and ws(dtype, 100, 17) == 0


def test_argument_errors_need_no_gpu():
    lib = B.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    F, P = B.MM_F32, B.STEREO_C_POSITIVE

    def fwd(dtype=F, x=q, n=10, m=5, rb=0, re=10, c=q, mode=P, c_min=1e-3, out=q):
        return lib.raw('mm_stereo_pdist_fwd')(dtype, x, n, m, rb, re, 1, c, mode, c_min, out, None)

    def bwd(dtype=F, x=q, g=q, n=10, m=5, rb=0, re=10, c=q, mode=P, c_min=1e-3, gx=q, gc=q, ws=q):
        return lib.raw('mm_stereo_pdist_bwd')(dtype, x, g, n, m, rb, re, 1, c, mode, c_min, gx, gc, ws, None)

    def dist(dtype=F, x=q, y=q, g=q, cnt=10, m=5, c=q, mode=P, out=q, gx=q, gy=q, gc=q, ws=q):
        return lib.raw('mm_stereo_dist')(dtype, x, y, g, cnt, m, 1, c, mode, 1e-3, out, gx, gy, gc, ws, None)

    def mp(dtype=F, op=B.STEREO_EXP, x=q, u=q, y=q, cnt=10, m=5, c=q, mode=P, out=q):
        return lib.raw('mm_stereo_map')(dtype, op, x, u, y, cnt, m, c, mode, 1e-3, out, None)

    def step(dtype=F, x=q, e=q, cnt=10, m=5, c=q, mode=P, out=q):
        return lib.raw('mm_stereo_rsgd_step')(dtype, x, e, cnt, m, c, mode, 1e-3, 0.01, 20.0, 1, out, None)

    def stab(dtype=F, x=q, cnt=10, m=5, c=q, mode=P, r_max=5.0, out=q):
        return lib.raw('mm_stereo_stabilize')(dtype, x, cnt, m, c, mode, 1e-3, r_max, out, None)

    for fn in (fwd, bwd, dist, mp, step, stab):
        assert fn(dtype=5) == -1 and fn(m=0) == -1 and fn(c=None) == -1 and fn(mode=3) == -1 and fn(mode=-1) == -1, fn.__name__
        assert fn(x=None) == -1 and fn(m=17) == -2, fn.__name__
        assert fn(m=17, mode=7) == -1, fn.__name__                  # an argument error is reported first
    for fn in (fwd, bwd):
        assert fn(rb=-1) == -1 and fn(re=11) == -1 and fn(rb=6, re=5) == -1 and fn(n=-1, re=0) == -1 and fn(c_min=-1.0) == -1
        assert fn(n=32769, re=32769) == -2 and fn(n=1 << 40, re=5) == -2
    assert fwd(out=None) == -1 and bwd(g=None) == -1 and bwd(gx=None) == -1 and bwd(gc=None) == -1 and bwd(ws=None) == -1
    assert dist(out=None, gx=None, gy=None, gc=None) == -1 and dist(gy=None) == -1 and dist(g=None) == -1 and dist(ws=None) == -1
    assert dist(y=None) == -1 and dist(cnt=-1) == -1
    assert mp(op=8) == -1 and mp(op=-1) == -1 and mp(u=None) == -1 and mp(op=B.STEREO_LOG, y=None) == -1 and mp(out=None) == -1
    assert mp(op=B.STEREO_TRANSP, y=None) == -1 and mp(cnt=-1) == -1
    assert step(e=None) == -1 and step(out=None) == -1 and step(cnt=-1) == -1
    assert stab(out=None) == -1 and stab(r_max=0.0) == -1 and stab(cnt=-1) == -1
    with pytest.raises(B.BackendError):
        lib.call('mm_stereo_pdist_fwd', F, None, 10, 5, 0, 10, 1, q, P, 1e-3, q, None)


@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_pair_kernels_keep_their_register_and_scratch_budget():
    """Nothing in scratch; the fp32 pair kernels fit four wavefronts per SIMD (<= 128 vector registers), the fp64 ones three (<= 168)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = {nm: k for nm, k in kernel_meta.kernels().items() if nm.startswith('stereo::')}
    want = {f'stereo::pdist_{d}_kernel<{t}, {mp}>' for d in ('fwd', 'bwd') for t in ('float', 'double') for mp in (4, 8, 16)}
    want |= {f'stereo::{k}_kernel<{t}>' for k in ('pdist_bwd_finalize', 'curv_finalize', 'map', 'dist', 'rsgd', 'stabilize')
             for t in ('float', 'double')}
    assert want <= set(ks), want - set(ks)
    for nm, k in ks.items():
        print(nm, k)
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
        if nm.startswith('stereo::pdist_'):
            assert k['vgpr'] + k['agpr'] <= (128 if '<float' in nm else 168), (nm, k)
            assert k['lds'] <= 65536


def test_class_surface():
    import graphembed.manifolds as M
    from graphembed.manifolds import Manifold, Stereographic
    from graphembed.modules import StereographicProductEmbedding
    man = Stereographic(5)
    assert isinstance(man, Manifold) and isinstance(man, torch.nn.Module) and 'Stereographic' in M.__all__
    for name in ('ndim', 'dim', 'get_c', 'get_K', 'get_R', 'zero', 'zero_vec', 'inner', 'norm', 'proju', 'projx', 'egrad2rgrad',
                 'exp', 'retr', 'log', 'dist', 'pdist', 'transp', 'rand', 'randvec', '__str__', 'rsgd_step', 'from_universal'):
        assert hasattr(man, name), name
    assert (man.ndim, man.dim, man.n, man.c_min, man.sign) == (1, 5, 5, 0.001, None)
    assert str(man) == 'Stereographic 5-dimensional manifold'
    assert list(man.parameters())[0] is man.c and man.c.shape == (1, ) and man.c.dtype == torch.float32
    assert float(man.get_c()) == pytest.approx(0.011) and float(man.get_K()) == pytest.approx(-0.011)
    assert float(man.get_R()) == pytest.approx(0.011 ** -0.5)
    fixed = Stereographic(3, c_init=-1.0, keep_sign_fixed=True)
    assert fixed.sign == -1 and float(fixed.get_c()) == pytest.approx(-(0.001 + np.log1p(np.exp(-1.0))))
    assert float(fixed.get_c()) == pytest.approx(float(S.get_c(np.float32(-1.0), 2)[0]))
    assert man.zero(4).shape == (4, 5) and man.zero_vec(2, 3).shape == (2, 3, 5)
    with pytest.raises(NotImplementedError):
        man.randvec(man.zero(2))
    x = man.rand(7)
    assert x.shape == (7, 5) and float(x.abs().max()) <= 1e-2 and not x.requires_grad
    u = torch.ones(7, 5)
    assert man.proju(x, u) is u
    # Universal.norm's conformal factor is taken at c = 1 (universal.py:48-52)
    assert torch.allclose(man.norm(x, u), 2 / (1 - x.pow(2).sum(-1)) * u.norm(dim=-1))
    assert torch.allclose(man.inner(x, u, u), (2 / (1 - 0.011 * x.pow(2).sum(-1))) ** 2 * 5)

    class Other:   # stands for the checkout's Universal instance
        n, c_min, sign, c = 4, 0.002, -1, torch.nn.Parameter(torch.tensor([-0.25]))
    got = Stereographic.from_universal(Other())
    assert (got.n, got.c_min, got.sign) == (4, 0.002, -1) and float(got.c) == -0.25 and got.c is not Other.c
    for call in (lambda: man.pdist(x), lambda: man.dist(x, x), lambda: man.exp(x, u), lambda: man.projx(x),
                 lambda: man.rsgd_step(x, u, lr=0.1)):
        with pytest.raises(B.BackendError):
            call()
    with pytest.raises(ValueError):
        Stereographic(17)
    assert not hasattr(M, 'Universal') and not hasattr(M, 'OrthogonalGroup')   # under the overlay those resolve to the checkout
    emb = StereographicProductEmbedding(12, [5, 3], r_max=4.0, c_init=-0.5, keep_sign_fixed=True)
    assert len(emb) == 12 and emb.r_max == 4.0 and [p.shape for p in emb.xs] == [(12, 5), (12, 3)]
    assert [p.manifold for p in emb.xs] == list(emb.manifolds) and all(m.sign == -1 for m in emb.manifolds)
    assert [id(c) for c in emb.curvature_params] == [id(m.c) for m in emb.manifolds]
    assert emb.device == emb.xs[0].device and len(list(emb.parameters())) == 4
