"""CPU-only checks of the fused objective of a product of constant-curvature factors (mm_stereo_product_*): the case list of
tests/stereo_product_cases.py and its kink condition, the long-double oracle against the recorded fp64 reference
(products.Embedding + objective + autograd), the host side of the entry points (declared, exported, struct layout, workspace
size, argument errors before anything touches a GPU, register / LDS / scratch budget of the kernels) and the CPU behaviour of
StereographicProductEmbedding."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import stereo_cases as S
import stereo_product_cases as P
from graphembed import _backend as B

NEW = ('mm_stereo_product_ws_bytes', 'mm_stereo_product_pdist_fwd', 'mm_stereo_product_loss')
LLVM_OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'

# vector registers (vgpr + agpr) of every instantiation as built; no scratch, no spill, static LDS <= 64 KB
REGISTERS = {
    'product_fwd_kernel<float, 4>': 70, 'product_fwd_kernel<float, 8>': 70, 'product_fwd_kernel<float, 16>': 86,
    'product_fwd_kernel<double, 4>': 148, 'product_fwd_kernel<double, 8>': 156, 'product_fwd_kernel<double, 16>': 172,
    'product_loss_kernel<float, 4, {L}>': 121, 'product_loss_kernel<float, 8, {L}>': 132, 'product_loss_kernel<float, 16, {L}>': 164,
    'product_loss_kernel<double, 4, {L}>': 202, 'product_loss_kernel<double, 8, {L}>': 206, 'product_loss_kernel<double, 16, {L}>': 254,
    'product_finalize_kernel<float>': 26, 'product_finalize_kernel<double>': 44,
    'product_reduce_kernel<float>': 14, 'product_reduce_kernel<double>': 14,
}


def test_case_list_and_inputs_follow_the_stated_rule():
    assert len(P.CASES) == 6 + 6 + 2 + 6 and len(set(P.CASE_IDS)) == len(P.CASES)
    assert [c[0] for c in P.CASES[:6]] == list(P.N_SWEEP) and all(c[1:5] == ((5, 5), (0.01, -0.3), (False, False), 'init') for c in P.CASES[:6])
    assert [c[1] for c in P.CASES[6:12]] == list(P.SHAPES) and all(c[0] == 65 and c[4] == 'spread' for c in P.CASES[6:12])
    # every padding class as the widest factor, mixed widths, the factor and width limits together
    assert {max(ds) for ds in P.SHAPES} == {4, 8, 16, 2} and (2, ) * 8 in P.SHAPES and (16, ) * 8 in P.SHAPES
    assert [(c[1], c[2], c[3], c[4]) for c in P.CASES[12:14]] == [((8, 8, 8), (1.0, -1.0, -0.01), (True, True, False), r) for r in ('init', 'spread')]
    assert [c[5] for c in P.CASES[14:]] == list(S._rows(129)) and all(c[:2] == (129, (5, 8)) for c in P.CASES[14:])
    assert (128, 129) in [c[5] for c in P.CASES] and S.pair_slice(129, (128, 129))[0] == S.pair_slice(129, (128, 129))[1]
    assert len(P.SETTINGS) == 6 and [s[1:] for s in P.SETTINGS] == [(0, 0, 1.0, 1), (1, 0, 1.0, 1), (2, 1, 1.0, 1), (2, 2, 1.0, 1),
                                                                  (2, 3, 1.0, 1), (2, 3, 0.7, 9)]
    for case in P.CASES:
        n, ds, cs, fixed, regime, rows = case
        xs, craws = P.make_inputs(case)
        xs2, _ = P.make_inputs(case)
        assert len(xs) == len(ds) == len(cs) == len(fixed) <= 8
        for x, x2, d, c_raw, c_init, fx in zip(xs, xs2, ds, craws, cs, fixed):
            assert x.dtype == np.float32 and x.shape == (n, d) and np.array_equal(x, x2) and c_raw == np.float32(c_init)
            c = float(S.get_c(c_raw, S.mode_of(c_init, fx))[0])
            r = np.sqrt(abs(c)) * np.sqrt((x.astype(np.float64) ** 2).sum(-1)).max()
            assert 0.69 <= r <= 0.7 if regime == 'spread' else r < 0.05
        rb, re = P.rows_of(case)
        assert 0 <= rb <= re <= n
    names = [f for f in os.listdir(S.GOLDEN) if f.startswith('stereo_product_') and f.endswith('.npz')]
    assert names and all(os.path.getsize(os.path.join(S.GOLDEN, f)) < (1 << 20) for f in names)
    R = S.recorded()
    assert 'product33/idx' in R and 'train40/target' in R   # the single-factor records keep loading beside the `prod/` keys


@pytest.mark.parametrize('case', P.CASES, ids=P.CASE_IDS)
def test_targets_stay_clear_of_the_quotient_kink(case):
    """target = float32(m F[k mod 4]): every pair has |m / (alpha g) - 1| >= 1e-4 and |alpha g / (m + eps) - 1| >= 1e-4 in the
    oracle, for every setting; no pair is filtered out.  Measured worst margin 1.6e-4 (ds = [1, 16], spread, eps = 1/2: a pair
    with m (F - 1) within 2e-4 of eps), >= 0.1 for every other case."""
    m, t = P.pairs_of(P.base_of(case))
    assert t.dtype == np.float32 and len(t) == len(m) == case[0] * (case[0] - 1) // 2
    f = np.array(P.F)[np.arange(len(m)) % 4]
    assert np.array_equal(t, (m * f.astype(S.LD)).astype(np.float32))
    for setting in P.SETTINGS:
        margin = P.kink_margin(case, setting)
        print(P.case_id(case), setting[0], f'{margin:.3e}')
        assert margin >= P.KINK, (setting[0], margin)


@pytest.mark.parametrize('case', [c for c in P.CASES if P.key(c, 'up', 'loss', 'f64') in S.recorded()], ids=P.case_id)
def test_oracle_matches_the_recorded_fp64_reference(case):
    """Measured worst deviation of the oracle from the reference's fp64 results over the recorded cases, relative to max m,
    sum |loss terms|, max |grad_x_k| and sum |g dF/dc_raw| (the reference's own fp64 curvature sum cancels at `init`):
      init:    pair vector 1.9e-14, loss 1.2e-13, grad_x 7.9e-14, grad_c 1.4e-8
      spread:  pair vector 1.5e-15, loss 3.8e-16, grad_x 3.8e-15, grad_c 1.2e-15
    asserted at twice these figures."""
    R = S.recorded()
    init = case[4] == 'init'
    m, _ = P.pairs_of(P.base_of(case))
    dv = S.deviation(R[f'prod/{P.case_id(P.base_of(case))}/dists_f64'], m) / float(m.max())
    print(f'{P.case_id(case)}: pair vector {dv:.2e}')
    assert dv <= (3.8e-14 if init else 3.0e-15)
    for name in P.SETTING_IDS:
        o = P.oracle(case, name)
        dl = abs(float(S.LD(R[P.key(case, name, 'loss', 'f64')]) - o['loss'])) / float(o['loss_scale'])
        assert dl <= (2.4e-13 if init else 7.6e-16), (name, dl)
        for k in range(len(case[1])):
            dx = S.deviation(R[P.key(case, name, f'gx{k}', 'f64')], o['gx'][k]) / float(np.abs(o['gx'][k]).max())
            dc = S.deviation(R[P.key(case, name, f'gc{k}', 'f64')][0], o['gc'][k]) / float(o['gcs'][k])
            print(f'{P.case_id(case)} {name} factor {k}: loss {dl:.2e} grad_x {dx:.2e} grad_c {dc:.2e}')
            assert dx <= (1.6e-13 if init else 7.6e-15) and dc <= (2.8e-8 if init else 2.4e-15), (name, k, dx, dc)


def test_every_case_is_recorded_in_fp32_and_the_sweeps_in_fp64():
    R = S.recorded()
    for case in P.CASES:
        for name in P.SETTING_IDS:
            for k in range(len(case[1])):
                assert R[P.key(case, name, f'gx{k}', 'f32')].shape == (case[0], case[1][k])
                assert R[P.key(case, name, f'gc{k}', 'f32')].shape == (1, )
        assert f'prod/{P.case_id(P.base_of(case))}/dists_f32' in R
    for case in P.CASES[:12]:
        assert P.key(case, 'q3b', 'loss', 'f64') in R and f'prod/{P.case_id(case)}/dists_f64' in R


def test_new_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, 'include', 'mm_manifolds.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mm_[a-z0-9_]+)\s*\(', plain))
    raw = ctypes.CDLL(B.lib().path)
    for name in NEW:
        assert name in declared and name in B.SIGNATURES and hasattr(raw, name), name
    assert declared == set(B.SIGNATURES)
    assert 'typedef struct mm_stereo_factor' in plain and re.search(r'MM_LOSS_NONE\s*=\s*0', plain) and B.LOSS_NONE == 0
    assert B.lib().raw('mm_abi_version')() == 4


def test_factor_struct_layout_matches_the_header(tmp_path):
    """The ctypes mirror of mm_stereo_factor (graphembed/_backend.py) against the C compiler's layout."""
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    fields = [f[0] for f in B.StereoFactor._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mm_manifolds.h"', 'int main(void) {',
           'printf("%zu\\n", sizeof(mm_stereo_factor));']
    src += [f'printf("{f} %zu\\n", offsetof(mm_stereo_factor, {f}));' for f in fields]
    src += ['return 0; }']
    c = tmp_path / 'layout.c'
    c.write_text('\n'.join(src))
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c11', '-I' + os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split('\n')
    assert int(out[0]) == ctypes.sizeof(B.StereoFactor) == 48
    seen = {}
    for line in out[1:]:
        if line:
            name, off = line.split()
            seen[name] = int(off)
            assert getattr(B.StereoFactor, name).offset == int(off), name
    assert list(seen) == fields == ['x', 'c_raw', 'grad_x', 'grad_c', 'c_min', 'm', 'c_mode']


def _ms(*m):
    return (ctypes.c_int32 * len(m))(*m)


@pytest.mark.parametrize('dtype,size,rows', [(B.MM_F32, 4, 64), (B.MM_F64, 8, 32)])
def test_workspace_is_monotone_and_covers_the_documented_layout(dtype, size, rows):
    ws = B.lib().raw('mm_stereo_product_ws_bytes')
    single = B.lib().raw('mm_stereo_pdist_ws_bytes')
    for ms in ((5, 5), (1, 16), (2, ) * 8, (16, ) * 8, (7, )):
        last = 0
        for n in (0, 1, 2, 3, 63, 64, 65, 129, 257, 1025, 4039, 32768):
            b = ws(dtype, n, len(ms), _ms(*ms))
            nbr, nbc = (n + rows - 1) // rows, (n + 63) // 64
            # per factor one record of m + 1 values per node and tile row / tile column; (nf + 1) fp64 partials per tile
            assert b >= sum(size * (m + 1) * n * (nbr + nbc) for m in ms) + 8 * (len(ms) + 1) * nbr * nbc, (n, ms, b)
            assert b >= last, (n, ms)
            last = b
            # exactly: the single-factor slabs (their own partials taken out) and one block of (nf + 1) partials per tile
            r256 = lambda v: (v + 255) & ~255
            slabs = sum(single(dtype, n, m) - r256(8 * (nbr * nbc + 1)) for m in ms)
            assert b == slabs + r256(8 * ((len(ms) + 1) * nbr * nbc + 1)), (n, ms, b)
    assert ws(dtype, -1, 2, _ms(5, 5)) == 0 and ws(dtype, 32769, 2, _ms(5, 5)) == 0 and ws(9, 100, 2, _ms(5, 5)) == 0
    assert ws(dtype, 100, 0, _ms(5)) == 0 and ws(dtype, 100, 9, _ms(*(2, ) * 9)) == 0 and ws(dtype, 100, 2, None) == 0
    assert ws(dtype, 100, 2, _ms(5, 0)) == 0 and ws(dtype, 100, 2, _ms(17, 5)) == 0


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

    def fwd(dtype=F32, f='default', nf=2, n=10, rb=0, re=10, out=q, **kw):
        f = factors(nf, **kw) if f == 'default' else f
        return lib.raw('mm_stereo_product_pdist_fwd')(dtype, f, nf, n, rb, re, out, None)

    def loss(dtype=F32, kind=B.LOSS_STRESS, f='default', nf=2, target=q, n=10, rb=0, re=10, out=q, ws=q, **kw):
        f = factors(nf, **kw) if f == 'default' else f
        return lib.raw('mm_stereo_product_loss')(dtype, kind, f, nf, target, n, rb, re, 1.0, 0.5, 3, None, out, ws, None)

    for fn in (fwd, loss):
        assert fn(dtype=5) == -1 and fn(f=None) == -1 and fn(nf=0) == -1 and fn(nf=-1) == -1, fn.__name__
        assert fn(m=0) == -1 and fn(c=None) == -1 and fn(mode=3) == -1 and fn(mode=-1) == -1 and fn(c_min=-1.0) == -1, fn.__name__
        assert fn(x=None) == -1 and fn(last={'x': None}) == -1 and fn(last={'m': 0}) == -1 and fn(last={'c_mode': 7}) == -1, fn.__name__
        assert fn(rb=-1) == -1 and fn(re=11) == -1 and fn(rb=6, re=5) == -1 and fn(n=-1, re=0) == -1, fn.__name__
        assert fn(m=17) == -2 and fn(last={'m': 17}) == -2 and fn(nf=9) == -2, fn.__name__
        assert fn(n=32769, re=32769) == -2 and fn(n=1 << 40, re=5) == -2, fn.__name__
        assert fn(m=17, mode=7) == -1 and fn(nf=9, last={'m': 0}) == -1, fn.__name__        # an argument error is reported first
    assert fwd(out=None) == -1 and fwd(gx=None, gc=None, m=17) == -2      # (the forward takes no gradient buffers)
    assert loss(kind=3) == -1 and loss(kind=-1) == -1 and loss(target=None) == -1 and loss(out=None) == -1 and loss(ws=None) == -1
    assert loss(gx=None) == -1 and loss(gc=None) == -1 and loss(last={'grad_c': None}) == -1
    assert loss(kind=B.LOSS_NONE, out=None, m=17) == -2       # MM_LOSS_NONE writes no loss: its loss_out may be NULL
    with pytest.raises(B.BackendError):
        lib.call('mm_stereo_product_loss', F32, 7, factors(), 2, q, 10, 0, 10, 1.0, 0.5, 3, None, q, q, None)


@pytest.mark.skipif(not (os.path.exists(LLVM_OBJDUMP) and shutil.which('c++filt')), reason='needs the ROCm llvm tools and c++filt')
def test_product_kernels_keep_their_register_lds_and_scratch_budget():
    """Nothing in scratch, nothing spilled, static LDS within 64 KB (60 192 bytes for the widest fp64 objective kernel: two
    pair tiles, no third one - g stays in registers); vector registers at the values measured on the build."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    ks = {nm[len('stereo::'):]: k for nm, k in kernel_meta.kernels().items() if nm.startswith('stereo::product_')}
    want = {}
    for name, regs in REGISTERS.items():
        for kind in (0, 1, 2) if '{L}' in name else (0, ):
            want[name.format(L=kind)] = regs
    assert set(want) == set(ks), set(want) ^ set(ks)
    for nm, k in ks.items():
        print(nm, k)
        assert k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (nm, k)
        assert k['lds'] <= 65536, (nm, k)
        assert k['vgpr'] + k['agpr'] == want[nm], (nm, k, want[nm])
    assert max(k['lds'] for k in ks.values()) == 60192


def test_cpu_tensors_take_the_per_factor_route():
    from graphembed.modules import StereographicProductEmbedding
    from graphembed.objectives import QuotientLoss, StressLoss
    assert StereographicProductEmbedding.pair_kernel is True
    emb = StereographicProductEmbedding(12, [5, 3])
    target = torch.ones(66)
    for fn in (StressLoss(), QuotientLoss()):
        assert emb.fused_objective(fn, target, None, epoch=1, alpha=1.0) is None
        assert emb.fused_objective(fn, target, torch.arange(4), rows=None, validated=True, epoch=1, alpha=1.0) is None
    # compute_dists on CPU tensors is today's sum: one Stereographic.pdist per factor, which refuses CPU tensors
    with pytest.raises(B.BackendError):
        emb.compute_dists()
    calls = []
    for man in emb.manifolds:
        man.pdist = (lambda x, squared=False, _m=man: calls.append((_m.n, tuple(x.shape), squared)) or torch.full((x.shape[0] * (x.shape[0] - 1) // 2, ), float(_m.n)))
    d = emb.compute_dists(torch.tensor([3, 1, 7]))
    assert calls == [(5, (3, 5), True), (3, (3, 3), True)] and torch.equal(d, torch.full((3, ), 8.0))
