"""The bit-deterministic vector pair kernels on the CPU: the five new C entries exist, are declared and refuse bad arguments before
any GPU call; the launch geometry is a bounded pure function of (dtype, kind, n, m) and gives the rows per chunk the size cases
assume; the case table of tests/vec_det_cases.py has what it claims and its conditions hold on the oracle alone (at most a tenth
of the pairs masked in the fp32 plain backward, no target within the margin of a kink of the quotient loss, ONE pair's value
replaced moves the oracle's gradient by more than twice what vec_cases.errors allows); the register metadata of the vec_det::
kernels against their atomic twins; the Python routing.  Nothing here runs a kernel.

Printed figures (this file, -rA) are recorded in profiles/vec_deterministic.md."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import vec_det_cases as C

vc = C.vc
ENTRIES = ('mm_vec_pdist_det_ws_bytes', 'mm_vec_pdist_det_geometry', 'mm_vec_pdist_bwd_det', 'mm_vec_pdist_loss_det',
           'mm_vec_pdist_loss_subset_det')
TWINS = {'mm_vec_pdist_bwd_det': 'mm_vec_pdist_bwd', 'mm_vec_pdist_loss_det': 'mm_vec_pdist_loss',
         'mm_vec_pdist_loss_subset_det': 'mm_vec_pdist_loss_subset'}
B_CAP = 64 << 20          # B of include/mm_manifolds.h
MAX_NODES = 1 << 22
ARG, UNSUP = -1, -2
TEETH = 2.0               # one replaced pair value moves grad_x by more than this multiple of the allowance


def _B():
    from graphembed import _backend as B
    return B


def geometry(dt, kind, n, m):
    ch, rows = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _B().lib().raw('mm_vec_pdist_det_geometry')(dt, kind, n, m, ctypes.byref(ch), ctypes.byref(rows))
    assert rc == 0, (dt, kind, n, m, rc)
    return ch.value, rows.value


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    B = _B()
    lib = B.lib()                      # loads without a device
    for name in ENTRIES:
        assert name in B.SIGNATURES and lib.raw(name) is not None
    # the _det entries take the atomic entries' arguments, `ws` REPLACED by `det_ws`: the same prototype
    for det, atomic in TWINS.items():
        assert B.SIGNATURES[det] == B.SIGNATURES[atomic], det
        assert B.SIGNATURES[det][1][-2] == ctypes.c_void_p
    header = open(os.path.join(C.ROOT, 'include', 'mm_manifolds.h')).read()
    flat = re.sub(r'\s+', ' ', header)
    for name in ENTRIES:
        assert name + '(' in header
    for det, atomic in TWINS.items():   # declared with the twin's parameter list, the workspace renamed
        params = lambda nm: re.search(r'int %s\((.*?)\);' % nm, flat).group(1)      # noqa: E731
        assert params(det) == params(atomic).replace('void* ws', 'void* det_ws'), det
    assert 'size_t mm_vec_pdist_det_ws_bytes(int dtype, int kind, int64_t n, int m);' in flat
    assert 'int mm_vec_pdist_det_geometry(int dtype, int kind, int64_t n, int m, int64_t* chunks, int64_t* rows_per_chunk);' in flat
    assert lib.raw('mm_abi_version')() == 4
    assert B.SIGNATURES['mm_vec_pdist_det_geometry'][1][:4] == [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    assert len(B.SIGNATURES['mm_vec_pdist_det_geometry'][1]) == 6 and len(B.SIGNATURES['mm_vec_pdist_det_ws_bytes'][1]) == 4


def test_argument_errors():
    """refused before any GPU work (this process has no GPU): null pointers, bad row ranges, a bad dtype or kind, the quotient
    loss without a term -> MM_ERR_ARG; m > mm_vec_max_dim(), n > 2^22, an unknown loss -> MM_ERR_UNSUPPORTED"""
    B = _B()
    lib = B.lib()
    bwd, loss, sub = (lib.raw(nm) for nm in TWINS)
    p = 4096    # a non-null pointer value: never dereferenced, every call below returns before a launch
    n, md = 10, lib.raw('mm_vec_max_dim')()
    assert md == vc.MAX_DIM

    def call_bwd(x=p, g=p, n=n, m=5, rb=0, re=n, grad=p, det=p, dt=B.MM_F32, kind=B.LORENTZ):
        return bwd(dt, kind, x, g, n, m, rb, re, 1, grad, det, None)

    def call_loss(x=p, t=p, n=n, m=5, rb=0, re=n, out=p, grad=p, det=p, lk=B.LOSS_STRESS, terms=3, dt=B.MM_F32, kind=B.SPHERE):
        return loss(dt, kind, lk, x, t, p, n, m, rb, re, 0.7, 0.25, terms, None, out, grad, det, None)

    def call_sub(x=p, dense=p, idx=p, nt=50, bs=n, m=5, rb=0, re=n, out=p, grad=p, det=p, lk=B.LOSS_STRESS, terms=3, dt=B.MM_F64,
                 kind=B.EUCLIDEAN):
        return sub(dt, kind, lk, x, dense, p, nt, m, idx, bs, rb, re, 0.7, 0.25, terms, None, out, grad, det, None)

    for kw in (dict(x=None), dict(grad=None), dict(det=None), dict(g=None), dict(rb=-1), dict(re=n + 1), dict(rb=5, re=4), dict(n=0, re=0),
               dict(m=0), dict(dt=7), dict(kind=3)):
        assert call_bwd(**kw) == ARG, kw
    for kw in (dict(x=None), dict(grad=None), dict(det=None), dict(t=None), dict(out=None), dict(rb=-1), dict(re=n + 1), dict(rb=5, re=4),
               dict(m=0), dict(dt=7), dict(kind=-1), dict(lk=B.LOSS_QUOTIENT, terms=0), dict(lk=B.LOSS_QUOTIENT, terms=4)):
        assert call_loss(**kw) == ARG, kw
    for kw in (dict(x=None), dict(grad=None), dict(det=None), dict(dense=None), dict(idx=None), dict(out=None), dict(rb=-1), dict(re=n + 1),
               dict(rb=5, re=4), dict(bs=51, re=51), dict(nt=0), dict(m=0), dict(dt=7), dict(kind=3), dict(lk=B.LOSS_QUOTIENT, terms=0)):
        assert call_sub(**kw) == ARG, kw
    assert call_bwd(m=md + 1) == UNSUP and call_loss(m=md + 1) == UNSUP and call_sub(m=md + 1) == UNSUP
    assert call_bwd(n=MAX_NODES + 1, re=MAX_NODES + 1) == UNSUP and call_loss(n=MAX_NODES + 1, re=5) == UNSUP
    assert call_sub(nt=MAX_NODES + 2, bs=MAX_NODES + 1, re=5) == UNSUP
    assert call_loss(lk=0) == UNSUP and call_sub(lk=3) == UNSUP
    ch, rows = ctypes.c_int64(), ctypes.c_int64()
    geo = lib.raw('mm_vec_pdist_det_geometry')
    for args in ((7, 1, 10, 3), (B.MM_F32, 3, 10, 3), (B.MM_F32, 1, 0, 3), (B.MM_F32, 1, MAX_NODES + 1, 3), (B.MM_F32, 1, 10, 0),
                 (B.MM_F32, 1, 10, md + 1)):
        assert geo(*args, ctypes.byref(ch), ctypes.byref(rows)) == ARG, args
    assert geo(B.MM_F32, 1, 10, 3, None, ctypes.byref(rows)) == ARG and geo(B.MM_F32, 1, 10, 3, ctypes.byref(ch), None) == ARG


def test_geometry_is_bounded_covers_and_depends_on_its_arguments_alone():
    """n = 2 ... 1100, steps beyond, the powers of two up to 2^22; every kind and dtype, the widths at both ends of the padded
    classes: rows_per_chunk a multiple of 8, (chunks - 1) rows < n <= chunks rows, the slab within max(E n sizeof(T), B), ws_bytes
    covers the slab plus one {loss, dloss} slot pair per workgroup; the same answer under every MM_VEC_* / MM_GRAM_* switch set
    in the environment afterwards and on a second call"""
    B = _B()
    nbytes = B.lib().raw('mm_vec_pdist_det_ws_bytes')
    sizes = list(range(2, 1101)) + list(range(1100, 20000, 997)) + [4039, 5000] + [1 << k for k in range(13, 23)]
    most_chunks, largest, table = 0, 0, {}
    for dt, esz in ((B.MM_F32, 4), (B.MM_F64, 8)):
        for kind in (B.EUCLIDEAN, B.LORENTZ, B.SPHERE):
            for m in (1, 4, 11, 17, 64):
                e = m + (1 if kind == B.EUCLIDEAN else 0)
                for n in sizes:
                    ch, rows = geometry(dt, kind, n, m)
                    table[(dt, kind, n, m)] = (ch, rows)
                    assert ch >= 1 and rows >= 8 and rows % 8 == 0 and (ch - 1) * rows < n <= ch * rows, (dt, kind, m, n, ch, rows)
                    slab = ch * e * n * esz
                    assert slab <= max(e * n * esz, B_CAP), (dt, kind, m, n, ch)
                    groups = (n + 255) // 256
                    assert groups * ch <= 2048 or ch == 1 or rows == 8
                    assert slab + 2 * groups * ch * esz <= nbytes(dt, kind, n, m) <= slab + 2 * groups * ch * esz + 128, (dt, kind, m, n)
                    most_chunks, largest = max(most_chunks, ch), max(largest, nbytes(dt, kind, n, m))
    assert most_chunks <= 1024
    saved = {k: os.environ.get(k) for k in vc.ENV_KEYS}
    try:
        for env in vc.ENVS:
            os.environ.update(env)
        for key in list(table)[::37]:
            assert geometry(*key) == table[key], key
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    # what the size cases assume: 8 rows per chunk at every n of the table, so 64 sits AT a chunk boundary and 65 one row past it
    for c in C.all_cases():
        n = c['batch'] or c['n']
        for dt in (B.MM_F32, B.MM_F64):
            assert geometry(dt, vc.KIND_CODE[c['kind']], n, c['m'])[1] == C.ROWS_PER_CHUNK, c['id']
    assert C.SIZES == (2, 3, 64, 65, 257) and max(C.SIZES[:4]) <= vc.N
    assert geometry(B.MM_F32, B.LORENTZ, 64, 11) == (8, 8) and geometry(B.MM_F32, B.LORENTZ, 65, 11) == (9, 8)
    assert geometry(B.MM_F32, B.LORENTZ, vc.N, 11) == (17, 8) and geometry(B.MM_F64, B.SPHERE, 257, 6) == (33, 8)
    print(f'most chunks {most_chunks}, largest det_ws {largest / 2**20:.1f} MiB; Lorentz(11) n = 4039: {geometry(B.MM_F32, B.LORENTZ, 4039, 11)}')


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def test_case_table():
    inst, sizes, shards, mini = (C.SWEEPS[k]() for k in ('instantiations', 'sizes', 'shards', 'minibatches'))
    ids = [c['id'] for c in inst + sizes + shards + mini]
    assert len(C.all_cases()) == len(set(ids))
    lo = {'euclidean': 1, 'lorentz': 2, 'sphere': 2}
    for dname in C.DNAMES:
        for kind in vc.KINDS:
            widths = {m for m in vc.WIDTHS if m >= lo[kind]}
            for what in ('sq', 'plain', 'stress'):
                got = {c['m'] for c in inst if c['kind'] == kind and c['dname'] == dname and c['scale'] and
                       (c['loss'] or ('sq' if c['squared'] else 'plain')) == what}
                assert got == widths, (dname, kind, what)
            got = {c['m'] for c in inst if c['kind'] == kind and c['dname'] == dname and c['scale'] and (c['loss'] or '').startswith('quotient')}
            assert got == widths, (dname, kind)
            assert sum(1 for c in inst if c['kind'] == kind and c['dname'] == dname and not c['scale']) == 2
            assert {c['m'] for c in inst if not c['scale'] and c['kind'] == kind} == {vc.PRIMARY[kind]}
            mine = [c for c in sizes if c['kind'] == kind and c['dname'] == dname]
            assert len(mine) == 4 * len(C.SIZES) and {c['n'] for c in mine} == set(C.SIZES) and {c['m'] for c in mine} == {vc.PRIMARY[kind]}
            mine = [c for c in shards if c['kind'] == kind and c['dname'] == dname]
            assert len(mine) == 4 * 7 and {c['rows'] for c in mine} == set(C.shard_ranges()) | {None}
            mine = [c for c in mini if c['kind'] == kind and c['dname'] == dname and not c.get('asym') and not c.get('brows')]
            assert {(c['m'], c['batch']) for c in mine} == {(m, b) for m in C.SUB_WIDTHS for b in vc.BATCHES} and len(mine) == 24
            assert {c['loss'].split('_')[0] for c in mine} == {'stress', 'quotient'}
    assert {c['loss'] for c in inst if c['loss']} == {'stress', 'quotient', 'quotient_l1', 'quotient_l2'}
    assert {C.n_pairs(c) for c in shards} >= {0} and any(c['rows'] and c['rows'][0] % 8 for c in shards)
    assert sum(1 for c in mini if c.get('asym')) == 4 and sum(1 for c in mini if c.get('brows')) == 4
    idx = vc.batch_idx('lorentz', 11, 'f32', 70)
    assert sorted(idx) != list(idx)                                              # unsorted indices
    print({k: len(v()) for k, v in C.SWEEPS.items()}, 'cases;', len(C.all_cases()), 'distinct')


def test_the_asymmetric_matrix_tells_the_transposed_read_apart():
    """reading dense[idx[b]][idx[a]] in place of dense[idx[a]][idx[b]] moves the oracle far beyond the bound"""
    for c in (c for c in C.all_cases() if c.get('asym')):
        inp = C.inputs(c)
        assert not np.array_equal(inp['dense'], inp['dense'].T)
        i, j = inp['pairs']
        want = C.oracle(c)[0]
        other = C.evaluate(c, values=np.asarray(inp['dense'], np.float64)[j, i])[0]
        assert max(vc.worst(vc.errors(c, want, other)).values()) > 100, c['id']


def test_conditions_masked_share_kinks_and_teeth():
    """caps on the inputs, from the oracle alone"""
    worst_teeth, worst_kink, worst_mask = (np.inf, ''), (np.inf, ''), (0.0, '')
    count = 0
    for c in C.all_cases():
        if c['entry'] == 'bwd':
            share = vc.masked_share(c)
            if c['dname'] == 'f64' or c['squared']:
                assert share == 0.0, c['id']
            assert share <= vc.MAX_MASKED_SHARE, (c['id'], share)
            worst_mask = max(worst_mask, (share, c['id']))
        if not C.n_pairs(c):
            want = C.oracle(c)[0]
            assert not np.asarray(C.grad_of(want)).any(), c['id']
            continue
        if c['loss'] and c['loss'] != 'stress':
            km = C.kink_margin(c)
            assert km >= C.sc.KINK_MARGIN, (c['id'], km)
            worst_kink = min(worst_kink, (km, c['id']))
        want = C.oracle(c)[0]
        grad = np.asarray(C.grad_of(want))
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0, c['id']
        ratio = C.one_pair_effect(c) / C.grad_allowance(c)
        assert ratio > TEETH, (c['id'], ratio)
        worst_teeth = min(worst_teeth, (ratio, c['id']))
        count += 1
    print(f'{count} cases with a pair: one replaced pair value moves grad_x by >= {worst_teeth[0]:.2f} x the allowance ({worst_teeth[1]}); '
          f'smallest kink margin {worst_kink[0]:.3e} ({worst_kink[1]}); largest masked share {100 * worst_mask[0]:.1f} % ({worst_mask[1]})')


def test_shards_partition_the_whole():
    for dname in C.DNAMES:
        for kind in vc.KINDS:
            for entry in ('bwd', 'loss'):
                for sq, loss in vc._variants(entry):
                    whole = C.BY_ID[vc.case(entry, kind, vc.PRIMARY[kind], dname, sq, loss)['id']]
                    parts = [C.BY_ID[vc.case(entry, kind, vc.PRIMARY[kind], dname, sq, loss, rows=r)['id']] for r in vc.shards(vc.N)]
                    assert sum(C.n_pairs(p) for p in parts) == C.n_pairs(whole)
                    total = sum(np.asarray(C.grad_of(C.oracle(p)[0])) for p in parts)
                    ref = np.asarray(C.grad_of(C.oracle(whole)[0]))
                    assert np.abs(total - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def test_kernel_metadata():
    """tools/kernel_meta.py on the built library: 2 dtypes x 3 kinds x 8 widths x (3 full-batch + 2 minibatch) pair kernels and
    2 x 3 x 8 finalize kernels, nothing else in the namespace (a minibatch's gradient is cleared by mm::clear_async, clear.hpp); a
    pair kernel has no scratch and no spilled registers wherever the
    atomic twin vec_pdist_bwd_kernel of the same (T, KIND, MP, LOSS, SUB) has none; nothing but the loss record and — minibatches —
    the staged rows goes through LDS.  The counts are printed (recorded in profiles/vec_deterministic.md)."""
    import sys
    sys.path.insert(0, os.path.join(C.ROOT, 'tools'))
    import kernel_meta
    if not os.path.exists(kernel_meta.LIB):
        pytest.skip('library not built')
    every = kernel_meta.kernels()
    ks = {k: v for k, v in every.items() if 'vec_det::' in k}
    pair = {k: v for k, v in ks.items() if k.startswith('vec_det::pair_kernel<')}
    fin = {k: v for k, v in ks.items() if k.startswith('vec_det::finalize_kernel<')}
    assert len(pair) == 2 * 3 * 8 * 5 and len(fin) == 2 * 3 * 8
    assert len(ks) == len(pair) + len(fin), sorted(set(ks) - set(pair) - set(fin))
    assert not any('vec_det::clear_kernel' in k for k in every)
    assert not any(k.startswith(('vec_pdist_', 'vec_gram_', 'vec_sym_prep_kernel')) for k in ks)     # the closure tests do not see them
    clean = 0
    for name, r in sorted(pair.items()):
        t, kind, mp, loss, sub = re.match(r'vec_det::pair_kernel<(\w+), (\d+), (\d+), (\d+), (\w+)>$', name).groups()
        assert (loss != '0') or sub == 'false', name
        twin = every[f"vec_pdist_bwd_kernel<{t}, {kind}, {mp}, {'8' if sub == 'true' else '64'}, {loss}, {sub}>"]
        print(f"{name}: vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} vgpr_spill {r['vgpr_spill']} scratch {r['scratch']} lds {r['lds']}"
              f" | twin vgpr {twin['vgpr']} vgpr_spill {twin['vgpr_spill']} scratch {twin['scratch']}")
        if twin['scratch'] == 0 and twin['vgpr_spill'] == 0:
            assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r, twin)
            clean += 1
        esz = 4 if t == 'float' else 8
        assert r['lds'] <= (2 * 4 * esz if sub == 'false' else 64 * int(mp) * esz + 64 * 4 + 2 * 4 * esz + 64), (name, r['lds'])
    for name, r in sorted(fin.items()):
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 0, (name, r)
    print(f'{clean} of {len(pair)} pair kernels have a twin without scratch or spills, and have none themselves')
    assert clean >= 144      # every full-batch kernel


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_routing_host_side():
    """the constructors' keyword (a TypeError before this mode existed) against torch's switch, the gates of the atomic in-kernel
    minibatch / mixed-manifold routes declining a deterministic factor, NativeTrainStep refusing one, and the hook that serves
    the minibatches answering None for a manifold that is not in the mode"""
    from graphembed import modules as M
    from graphembed.manifolds import Euclidean, Lorentz, Sphere
    from graphembed.native_step import NativeTrainStep, _refuse_deterministic
    from graphembed.objectives import StressLoss
    make = {Euclidean: lambda **kw: Euclidean(10, **kw), Lorentz: lambda **kw: Lorentz(11, **kw), Sphere: lambda **kw: Sphere(6, **kw)}
    assert not torch.are_deterministic_algorithms_enabled()
    for cls, new in make.items():
        assert 'deterministic' in inspect.signature(cls.__init__).parameters
        assert new().deterministic is None and not new().is_deterministic()
        assert new(deterministic=True).is_deterministic() and not new(deterministic=False).is_deterministic()
        try:
            torch.use_deterministic_algorithms(True)
            assert new().is_deterministic() and new(deterministic=True).is_deterministic() and not new(deterministic=False).is_deterministic()
        finally:
            torch.use_deterministic_algorithms(False)
        assert not new().is_deterministic()
        assert M._pair_kernel_factor(new()) is not None and M._pair_kernel_factor(new(deterministic=True)) is None
        assert M._single_subset_factor(new()) is not None and M._single_subset_factor(new(deterministic=True)) is None
        assert M._pair_kernel_factors([new(), new(deterministic=False)]) is not None
        assert M._pair_kernel_factors([new(), new(deterministic=True)]) is None
        man = new()
        try:
            torch.use_deterministic_algorithms(True)
            assert M._pair_kernel_factor(man) is None and M._single_subset_factor(man) is None
        finally:
            torch.use_deterministic_algorithms(False)
        assert M._pair_kernel_factor(man) is not None
        # the minibatch hook: None outside the mode, whatever the tensors
        x = torch.zeros(5, man._m)
        assert man.pdist_loss_subset(x, torch.tensor(0.5), torch.arange(3), torch.zeros(5, 5), ('stress', 1.0, 0.0, 3)) is None
        assert new(deterministic=True).pdist_loss_subset(x, torch.tensor(0.5), torch.arange(3), torch.zeros(5, 5), ('stress', 1.0, 0.0, 3)) is None  # CPU tensors
        emb = types.SimpleNamespace(manifolds=[new(deterministic=True)], xs=[], scales=[])
        with pytest.raises(ValueError, match='deterministic') as err:
            NativeTrainStep(emb, StressLoss(), None, [])
        assert str(new(deterministic=True)) in str(err.value)
        _refuse_deterministic([new(), new(deterministic=False)])
    assert Lorentz(11, deterministic=True).sphere.deterministic is None      # (the helper manifold of `rand` is not a factor)
    # Wider than mm_vec_max_dim: no kernel either way — the gates decline as before
    assert M._single_subset_factor(Euclidean(65)) is None
