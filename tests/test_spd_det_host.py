"""The bit-deterministic SPD pair kernels on the CPU: the new C entries exist and refuse bad arguments, the launch geometry is a
bounded pure function of (dtype, n, d), the case table of tests/spd_det_cases.py has the sizes it claims, its oracles have teeth
(ONE pair's value replaced by its successor's moves grad_x by at least ONE_PAIR_MIN S), the register metadata of the spd_det::
kernels, and the Python routing.  Nothing here runs a kernel.

Measured (the printed figures, this file, -rA; profiles/spd_deterministic.md):
    one_pair_effect   min over the 265 cases with a pair 6.26e-4 S (threshold ONE_PAIR_MIN = 5e-4 S; SPD(9) `wide`, quotient, n = 130)
    kink_margin       smallest 1.002e-3; at most 90 of a pair vector's targets nudged (n = 257: 32 896 pairs)
    geometry          at most 171 chunks; the largest det_ws 2592 MiB (n = 2^22, d = 9, fp64: one record per node)"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import spd_det_cases as C

ENTRIES = ('mm_spd_pdist_det_ws_bytes', 'mm_spd_pdist_det_geometry', 'mm_spd_pdist_bwd_det', 'mm_spd_pdist_loss_det')
B_CAP = 64 << 20          # B of include/mm_manifolds.h
MAX_NODES = 1 << 22


def _B():
    from graphembed import _backend as B
    return B


def geometry(dt, n, d):
    ch, rows = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _B().lib().raw('mm_spd_pdist_det_geometry')(dt, n, d, ctypes.byref(ch), ctypes.byref(rows))
    assert rc == 0, (dt, n, d, rc)
    return ch.value, rows.value


def test_symbols_and_prototypes():
    B = _B()
    lib = B.lib()
    for name in ENTRIES:
        assert name in B.SIGNATURES and lib.raw(name) is not None
    # the _det entries take the atomic entries' arguments plus ONE pointer (det_ws) behind ws
    for det, atomic in (('mm_spd_pdist_bwd_det', 'mm_spd_pdist_bwd'), ('mm_spd_pdist_loss_det', 'mm_spd_pdist_loss')):
        a, d = B.SIGNATURES[atomic][1], B.SIGNATURES[det][1]
        assert d == a[:-2] + [ctypes.c_void_p] + a[-2:] and a[-3] == ctypes.c_void_p
    header = open(C.ROOT + '/include/mm_manifolds.h').read()
    for name in ENTRIES:
        assert name + '(' in header
    assert lib.raw('mm_abi_version')() == 4
    # geometry takes no row range
    assert B.SIGNATURES['mm_spd_pdist_det_geometry'][1][:3] == [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    assert len(B.SIGNATURES['mm_spd_pdist_det_geometry'][1]) == 5 and len(B.SIGNATURES['mm_spd_pdist_det_ws_bytes'][1]) == 3


def test_argument_errors():
    """refused before any GPU work (this machine has no GPU): null pointers, bad row ranges, n > 2^22 -> MM_ERR_ARG; eigenvalue
    windows outside spd_clamps_supported -> MM_ERR_UNSUPPORTED"""
    B = _B()
    lib = B.lib()
    bwd, loss, ARG, UNSUP = lib.raw('mm_spd_pdist_bwd_det'), lib.raw('mm_spd_pdist_loss_det'), -1, -2
    p = 4096    # a non-null pointer value: never dereferenced, every call below returns before a launch
    n = 10

    def call_bwd(x=p, g=p, n=n, d=3, rb=0, re=n, wmin=1e-8, wmax=1e8, grad=p, ws=p, det=p, dt=B.MM_F32):
        return bwd(dt, x, g, n, d, rb, re, 1, wmin, wmax, grad, ws, det, 0, None)

    def call_loss(x=p, t=p, n=n, d=3, rb=0, re=n, wmin=1e-8, wmax=1e8, out=p, grad=p, ws=p, det=p, kind=B.LOSS_STRESS, terms=3):
        return loss(B.MM_F32, kind, x, t, p, n, d, rb, re, 0.7, 0.25, terms, None, wmin, wmax, out, grad, ws, det, 0, None)

    for kw in (dict(x=None), dict(grad=None), dict(ws=None), dict(det=None), dict(g=None), dict(rb=-1), dict(re=n + 1),
               dict(rb=5, re=4), dict(n=MAX_NODES + 1, re=MAX_NODES + 1), dict(dt=7)):
        assert call_bwd(**kw) == ARG, kw
    for kw in (dict(x=None), dict(grad=None), dict(ws=None), dict(det=None), dict(t=None), dict(out=None), dict(rb=-1),
               dict(re=n + 1), dict(rb=5, re=4), dict(n=MAX_NODES + 1, re=MAX_NODES + 1), dict(kind=B.LOSS_QUOTIENT, terms=0)):
        assert call_loss(**kw) == ARG, kw
    assert call_loss(kind=0) == UNSUP and call_bwd(d=10) == UNSUP and call_loss(d=1) == UNSUP
    assert call_bwd(wmin=1e-4) == UNSUP and call_bwd(wmax=1e3) == UNSUP            # d >= 3: narrow windows
    assert call_loss(wmin=1e-4) == UNSUP and call_loss(d=2, wmax=1e3) == UNSUP      # the fused objective of every d
    ch, rows = ctypes.c_int64(), ctypes.c_int64()
    geo = lib.raw('mm_spd_pdist_det_geometry')
    for args in ((7, 10, 3), (B.MM_F32, 0, 3), (B.MM_F32, MAX_NODES + 1, 3), (B.MM_F32, 10, 1), (B.MM_F32, 10, 10)):
        assert geo(*args, ctypes.byref(ch), ctypes.byref(rows)) == ARG, args
    assert geo(B.MM_F32, 10, 3, None, ctypes.byref(rows)) == ARG and geo(B.MM_F32, 10, 3, ctypes.byref(ch), None) == ARG


def test_geometry_is_bounded_and_covers():
    """n = 2 ... 4100 and the powers of two up to 2^22, every d and dtype: chunks >= 1, (chunks - 1) rows < n <= chunks rows, the
    slab within max(d^2 n sizeof(T), B), ws_bytes covers the slab plus one {loss, dloss} slot pair per workgroup"""
    B = _B()
    nbytes = B.lib().raw('mm_spd_pdist_det_ws_bytes')
    sizes = list(range(2, 4101)) + [1 << k for k in range(13, 23)]
    most_chunks, largest = 0, 0
    for dt, esz in ((B.MM_F32, 4), (B.MM_F64, 8)):
        for d in C.DIMS:
            prev = None
            for n in sizes:
                ch, rows = geometry(dt, n, d)
                assert ch >= 1 and rows >= 1 and (ch - 1) * rows < n <= ch * rows, (dt, d, n, ch, rows)
                slab = ch * d * d * n * esz
                assert slab <= max(d * d * n * esz, B_CAP), (dt, d, n, ch)
                groups = (n + 255) // 256
                assert nbytes(dt, n, d) >= slab + 2 * groups * ch * esz, (dt, d, n)
                assert nbytes(dt, n, d) <= slab + 2 * groups * ch * esz + 128
                most_chunks, largest = max(most_chunks, ch), max(largest, nbytes(dt, n, d))
                if prev is not None and n >= 8192:
                    assert ch <= prev      # chunks fall as n grows
                prev = ch
    assert most_chunks <= 1024
    print(f'most chunks {most_chunks}, largest det_ws {largest / 2**20:.1f} MiB (n = 2^22, d = 9, fp64: one record per node)')


def test_case_table():
    for sweep, cases in C.SWEEPS.items():
        assert len(cases()) == C.CASE_COUNTS[sweep] and len(set(cases())) == len(cases()), sweep
    inst = C.instantiation_cases()
    assert {(c.D, c.kind, c.regime) for c in inst} == {(D, k, r) for D in C.DIMS for k in C.KINDS for r in C.REGIMES}
    assert {c.n for c in C.size_cases()} == {2, 3, 64, 65, 129, 257}
    assert {c.rows for c in C.shard_cases()} == set(C.SHARDS) and len(C.SHARDS) == 8 and set(C.COVER) <= set(C.SHARDS)
    assert C.COVER[0][0] == 0 and C.COVER[-1][1] == C.N_SHARD and all(a[1] == b[0] for a, b in zip(C.COVER, C.COVER[1:]))
    assert {C.n_pairs(c) for c in C.shard_cases()} >= {0, 1}
    # the sizes against the library's geometry: >= 3 chunks with a ragged last one; one AT a chunk boundary and one past it;
    # several column groups x several chunks
    B = _B()
    geo = {n: geometry(B.MM_F32, n, 3) for n in sorted({c.n for c in C.all_cases()})}
    for dt in (B.MM_F32, B.MM_F64):
        for d in C.DIMS:
            for n in geo:
                if n <= 257:     # (n = 1025 is an SPD(3) fp32 case, checked below: wide fp64 matrices meet the slab cap there)
                    assert geometry(dt, n, d)[1] == C.ROWS_PER_CHUNK, (dt, d, n)
    assert any(ch >= 3 and n % rows for n, (ch, rows) in geo.items())
    assert geo[64] == (8, 8) and geo[65] == (9, 8) and geo[129][0] == 17 and geo[257][0] == 33 and geo[C.N_INST] == (17, 8)
    assert geo[1025] == (129, 8) and (1025 + 255) // 256 == 5


def test_inputs_and_kink_margins():
    worst, most = np.inf, 0
    for c in C.all_cases():
        x = C.points(c.regime, c.D, c.n)
        assert x.dtype == torch.float32 and x.shape == (c.n, c.D, c.D) and torch.equal(x, x.transpose(1, 2))
        v = C.loaded(c)
        assert v.dtype == torch.float32 and v.numel() == C.n_pairs(c)
        if c.kind in C.LOSS_KINDS and C.n_pairs(c):
            assert float(v.min()) > 0
            km = C.kink_margin(c)
            assert km >= C.MARGIN, (C.case_id(c), km)
            worst, most = min(worst, km), max(most, C.nudged(c.regime, c.D, c.n))
        elif C.n_pairs(c) > 8:
            assert float(v.min()) < 0 < float(v.max())      # both signs
    assert float(np.linalg.eigvalsh(C.points(*C.LARGE[:3]).double().numpy()).min()) > 0
    print(f'smallest kink_margin {worst:.3e}, most pairs nudged in one pair vector {most}')


def test_teeth():
    """ONE pair's g / target replaced by its successor's moves the oracle's grad_x by at least ONE_PAIR_MIN S"""
    cases = [c for c in C.all_cases() if C.n_pairs(c)]
    assert len(cases) == 289 - 2 * 12
    p_min = (np.inf, '')
    for c in cases:
        scale = C.oracle(c).S['grad_x']
        p = C.one_pair_effect(c) / scale
        assert p >= C.ONE_PAIR_MIN, (C.case_id(c), p)
        p_min = min(p_min, (p, C.case_id(c)))
    print(f'teeth over {len(cases)} cases: one pair moves grad_x by >= {p_min[0]:.3e} S ({p_min[1]})')


def test_one_pair_effect_is_the_literal_one():
    for c in (C.Case('init', 2, C.N_INST, 'bwd_sq', None), C.Case('wide', 9, C.N_INST, 'quotient', None),
              C.Case('mid', 6, 257, 'bwd_nsq', None), C.Case('mid', 3, 2, 'stress', None),
              C.Case('mid', 4, C.N_SHARD, 'quotient', (43, 86)), C.Case('mid', 4, C.N_SHARD, 'bwd_nsq', (128, 129))):
        a, b = C.one_pair_effect(c), C.one_pair_effect_literal(c)
        assert abs(a - b) <= 1e-8 * a and a > 0, (C.case_id(c), a, b)


def test_bwd_oracle_agrees_with_exact():
    """the two fp64 oracles on the same case: ref_port's autograd gradient for a given g against oracle/exact.c"""
    for c in (C.Case('mid', 3, 65, 'bwd_sq', None), C.Case('wide', 5, 65, 'bwd_nsq', None)):
        i, j, lo, hi = C.pairs_of(c.n, c.rows)
        want = C.exact.spd_pairs_grad(C._x64(c.regime, c.D, c.n), i, j, C.loaded(c).double().numpy(), squared=c.kind == 'bwd_sq',
                                      wmin=C.WMIN, wmax=C.WMAX)
        err = float(np.abs(C.oracle(c).grad_x.numpy() - want).max())
        assert err <= 1e-11 * C.oracle(c).S['grad_x'], (C.case_id(c), err)


def test_register_metadata():
    """tools/kernel_meta.py on the built library: every instantiation is there; fp32 D <= 4 run without scratch and without
    spilled registers; the rest is printed (recorded in profiles/spd_deterministic.md)"""
    import sys
    sys.path.insert(0, C.ROOT + '/tools')
    import kernel_meta
    ks = {k: v for k, v in kernel_meta.kernels().items() if k.startswith('spd_det::')}
    pair = {k: v for k, v in ks.items() if 'pair_kernel' in k}
    assert len(pair) == 64 and len(ks) == 80, (len(pair), len(ks))
    for name, r in sorted(ks.items()):
        print(f'{name}: vgpr {r["vgpr"]} agpr {r["agpr"]} sgpr {r["sgpr"]} vgpr_spill {r["vgpr_spill"]} scratch {r["scratch"]} lds {r["lds"]}')
        if '<float, 2' in name or '<float, 3' in name or '<float, 4' in name:
            assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r)
        assert r['lds'] <= 64      # nothing but the loss record goes through LDS


def test_routing_host_side():
    """the constructor's switch (a TypeError before this mode existed), the Stein refusal, and the gates of the in-kernel
    minibatch / mixed-manifold routes declining a deterministic factor"""
    from graphembed.manifolds import SymmetricPositiveDefinite as SPD
    from graphembed import modules as M
    assert 'deterministic' in inspect.signature(SPD.__init__).parameters
    assert SPD(3).deterministic is None and not SPD(3).is_deterministic()
    assert SPD(3, deterministic=True).is_deterministic() and not SPD(3, deterministic=False).is_deterministic()
    with pytest.raises(ValueError, match='Stein'):
        SPD(3, use_stein_div=True, deterministic=True)
    with pytest.raises(ValueError, match='clamps'):
        SPD(3, wmin=1e-4, deterministic=True)
    assert SPD(3, use_stein_div=True, deterministic=False).use_stein_div
    assert not torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert SPD(3).is_deterministic() and not SPD(3, deterministic=False).is_deterministic()
        assert not SPD(3, use_stein_div=True).is_deterministic()
    finally:
        torch.use_deterministic_algorithms(False)
    assert not SPD(3).is_deterministic()
    for d in (2, 3, 4):
        assert M._single_subset_factor(SPD(d)) is not None and M._single_subset_factor(SPD(d, deterministic=True)) is None
    assert M._pair_kernel_factor(SPD(3)) is not None and M._pair_kernel_factor(SPD(3, deterministic=True)) is None
    from graphembed.manifolds import Euclidean
    assert M._pair_kernel_factors([Euclidean(4), SPD(2)]) is not None
    assert M._pair_kernel_factors([Euclidean(4), SPD(2, deterministic=True)]) is None
